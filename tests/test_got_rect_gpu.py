"""GOT between token sets of different sizes (v [k, n, d], q [k, m, d], n != m) on the GPU: the tiled class through its
mdl_got_tiled_rect_* entry points (csrc/got_tiled.hip; GOT(), functional.got_tiled) against the reference's own results
(tests/golden/got_rect.npz), against fp64 up to 4096 tokens on either side, the square case as the same code, the data-parallel
decomposition, determinism, partial gradients, bf16 inputs and the absence of library GEMMs."""
import pytest
import torch

from tests._util import golden, rel_err, t
from tests.test_got_rect_cpu import GOLDEN_SHAPES, inputs
from tests.test_got_tiled_gpu import GEMM_OPS, GRAD_TOL, TOL, VAL_TOL, _fp64_ref, got_parts64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _run(v, q, dev, fn=None):
    """(loss, dV, dQ) of GOT(v, q, subsample=None) (or of fn's out[1] + out[0]) on the device."""
    from madeleine_amd import GOT
    vd, qd = v.to(dev).requires_grad_(), q.to(dev).requires_grad_()
    if fn is None:
        loss = GOT(vd, qd, subsample=None)
    else:
        o = fn(vd, qd)
        loss = o[1] + o[0]
    loss.backward()
    return loss.detach(), vd.grad, qd.grad


@pytest.mark.parametrize("k,n,m,d", GOLDEN_SHAPES)
def test_got_rect_vs_golden(dev, k, n, m, d):
    """The reference's own fp32 value and gradients (tests/golden/got_rect.npz) at the project's parity bar, 1e-3 relative.
    Measured on MI355X: at most 6.6e-7 (value), 1.5e-6 (dV), 9.5e-7 (dQ) over the four shapes."""
    g = golden("got_rect")
    tag = f"{k}x{n}x{m}x{d}"
    v, q = inputs(k, n, m, d)
    loss, dv, dq = _run(v, q, dev)
    ref = float(g[tag + "/loss"])
    ev, edv, edq = abs(float(loss) - ref) / abs(ref), rel_err(dv, g[tag + "/dv"]), rel_err(dq, g[tag + "/dq"])
    print(f"\ngot_rect golden {tag}: value {ev:.2e} dV {edv:.2e} dQ {edq:.2e}")
    assert dv.shape == (k, n, d) and dq.shape == (k, m, d)
    assert ev < TOL and edv < TOL and edq < TOL


# measured on MI355X (value | dV | dQ): 1.4e-7 4.4e-7 5.0e-7 (2, 40, 56, 128); 2.7e-7 4.9e-7 5.1e-7 (3, 70, 33, 128); 2.9e-7 8.9e-7 9.3e-7
# (1, 1, 9, 32); 3.7e-7 8.0e-7 5.8e-7 (2, 17, 1, 64); 7.7e-7 7.0e-7 1.1e-6 (2, 130, 200, 128); 1.4e-7 1.1e-6 7.3e-7 (1, 300, 120, 129);
# 2.1e-8 1.2e-6 5.9e-7 (2, 256, 64, 128); 4.5e-8 1.7e-6 1.8e-6 (2, 513, 700, 128); 1.7e-7 1.5e-6 1.0e-6 (2, 700, 90, 1000);
# 1.2e-9 2.1e-6 9.8e-7 (1, 1024, 300, 128); 1.2e-6 1.2e-6 2.2e-6 (1, 300, 1024, 128); 1.9e-8 3.5e-6 2.0e-6 (1, 2048, 640, 128): the level of
# the square shapes.  Bounds: VAL_TOL, GRAD_TOL of tests/test_got_tiled_gpu.py, unchanged.
@pytest.mark.parametrize("k,n,m,d", GOLDEN_SHAPES + [(2, 130, 200, 128), (1, 300, 120, 129), (2, 256, 64, 128), (2, 513, 700, 128),
                                                     (2, 700, 90, 1000), (1, 1024, 300, 128), (1, 300, 1024, 128), (1, 2048, 640, 128)])
def test_got_rect_vs_fp64(dev, k, n, m, d):
    """GOT(v, q, subsample=None) with n != m against the reference algorithm in fp64 (the oracle on the CPU up to 600 tokens, its
    restatement on the GPU beyond), at the bounds committed for these kernels on square shapes."""
    v, q = inputs(k, n, m, d)
    if max(n, m) <= 600:
        ref, gv, gq = _fp64_ref(v, q, dev)
    else:
        v64, q64 = v.to(dev).double().requires_grad_(), q.to(dev).double().requires_grad_()
        r = got_parts64(v64, q64, ckpt=True).sum()
        r.backward()
        ref, gv, gq = float(r.detach()), v64.grad, q64.grad
    loss, dv, dq = _run(v, q, dev)
    ev, edv, edq = abs(float(loss) - ref) / abs(ref), rel_err(dv, gv), rel_err(dq, gq)
    print(f"\ngot_rect fp64 k={k} n={n} m={m} d={d}: value {ev:.2e} dV {edv:.2e} dQ {edq:.2e}")
    assert ev < VAL_TOL and edv < GRAD_TOL and edq < GRAD_TOL


@pytest.mark.parametrize("n,m", [(4096, 512), (512, 4096)])
def test_got_rect_extremes(dev, n, m):
    """4096 tokens on one side (k = 1, d = 128): the value against an fp64 forward, the gradients through a central-difference
    directional derivative of the fp64 forward (the bounds of test_got_tiled_n4096).

    The step is 1e-5 |v| / |u|, ten times shorter than in test_got_tiled_n4096: at (512, 4096) the central difference of the fp64
    forward at 1e-4 is itself 9.5e-5 away from the fp64 autograd derivative of the same function (2.934022e-2 against 2.934300e-2; the
    thresholded costs are piecewise), while the steps 3e-5, 1e-5 and 1e-6 agree with it and with each other to 1.9e-7.  At (4096, 512)
    all four steps agree to 4e-8.  Measured on MI355X (value | directional derivative): 1.8e-7 6.1e-6 at (512, 4096),
    2.9e-8 1.5e-6 at (4096, 512)."""
    k, d = 1, 128
    v, q = inputs(k, n, m, d)
    loss, dv, dq = _run(v, q, dev)
    gv, gq, val = dv.double(), dq.double(), float(loss)
    del loss, dv, dq
    torch.cuda.empty_cache()
    v64, q64 = v.to(dev).double(), q.to(dev).double()
    with torch.no_grad():
        ref = float(got_parts64(v64, q64).sum())
        u = t((k, n, d), f"got_rect:{n}x{m}:u").to(dev).double()
        w = t((k, m, d), f"got_rect:{n}x{m}:w").to(dev).double()
        eps = 1e-5 * float(v64.norm()) / float(u.norm())
        fp = float(got_parts64(v64 + eps * u, q64 + eps * w).sum())
        fm = float(got_parts64(v64 - eps * u, q64 - eps * w).sum())
    fd = (fp - fm) / (2 * eps)
    an = float((gv * u).sum() + (gq * w).sum())
    print(f"\ngot_rect n={n} m={m}: value {abs(val - ref) / abs(ref):.2e} directional derivative {abs(an - fd) / abs(fd):.2e}")
    assert abs(val - ref) < 1e-5 * abs(ref)
    assert abs(an - fd) < 2e-5 * abs(fd)
    torch.cuda.empty_cache()


def test_got_rect_limits(dev):
    from madeleine_amd import GOT
    with pytest.raises(NotImplementedError, match="n=4097, m=8, d=8"):
        GOT(torch.rand(1, 4097, 8, device=dev), torch.rand(1, 8, 8, device=dev), subsample=None)
    with pytest.raises(NotImplementedError, match="n=8, m=4097, d=8"):
        GOT(torch.rand(1, 8, 8, device=dev), torch.rand(1, 4097, 8, device=dev), subsample=None)
    with pytest.raises(ValueError):     # k or d that differ
        GOT(torch.rand(1, 8, 8, device=dev), torch.rand(2, 9, 8, device=dev), subsample=None)
    with pytest.raises(ValueError):
        GOT(torch.rand(1, 8, 8, device=dev), torch.rand(1, 9, 16, device=dev), subsample=None)
    from madeleine_amd import functional as MF
    with pytest.raises(ValueError):     # the resident family stays square
        MF.got(torch.rand(1, 8, 8, device=dev), torch.rand(1, 9, 8, device=dev))
    # empty sides: zero outputs, zero gradients
    for n, m in ((0, 5), (5, 0)):
        a = torch.rand(2, n, 8, device=dev, requires_grad=True)
        b = torch.rand(2, m, 8, device=dev, requires_grad=True)
        o = MF.got_tiled(a, b)
        (o[0] + o[1]).backward()
        assert torch.equal(o.detach(), torch.zeros(2, device=dev))
        assert a.grad.shape == a.shape and b.grad.shape == b.shape
        assert float(a.grad.abs().sum()) == 0.0 and float(b.grad.abs().sum()) == 0.0


@pytest.mark.parametrize("shape", [(0, 8, 8), (2, 0, 8)])
def test_got_resident_empty_problem(dev, shape):
    """The resident class (the training path's: got_route(0, 8, 8) and (2, 0, 8) are 'resident') with k = 0 and with n = 0, as the
    tiled class has it above: tensors of no elements have no storage, the distances are (0, 0) and the gradients are zero."""
    from madeleine_amd import GOT, functional as MF
    from madeleine_amd.loss import got_route
    assert got_route(*shape) == "resident"
    for fn in (MF.got, lambda a, b: GOT(a, b, subsample=None)):
        v = torch.zeros(*shape, device=dev, requires_grad=True)
        q = torch.zeros(*shape, device=dev, requires_grad=True)
        o = fn(v, q)
        o.sum().backward()
        assert torch.equal(o.detach(), torch.zeros_like(o)) and o.numel() in (1, 2)
        assert v.grad.shape == v.shape and q.grad.shape == q.shape
        assert float(v.grad.abs().sum()) == 0.0 and float(q.grad.abs().sum()) == 0.0


def test_got_rect_square_is_the_same_code(dev):
    """(2, 300, 300, 64) through the mdl_got_tiled_rect_* entry points and through the six square ones: the same bits."""
    from madeleine_amd import functional as MF
    v, q = inputs(2, 300, 300, 64)
    res = []
    for fam in (MF.GOT_TILED, MF.GOT_TILED_RECT):
        vd, qd = v.to(dev).requires_grad_(), q.to(dev).requires_grad_()
        o, mm = MF.GOTFn.apply(vd, qd, None, None, fam)
        (o[1] + o[0]).backward()
        res.append((o.detach().clone(), mm.clone(), vd.grad.clone(), qd.grad.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert torch.isfinite(res[0][0]).all() and float(res[0][2].abs().sum()) > 0


def test_got_rect_data_parallel_decomposition(dev):
    """(4, 130, 200, 128): cases [0:1] and [1:4] run with the global extrema (minmax_in) and the summed extremum gradients
    (reduce_dminmax) add up to the full batch in both distances and both gradients."""
    from madeleine_amd import functional as MF
    v, q = inputs(4, 130, 200, 128)
    v, q = v.to(dev), q.to(dev)
    v1, q1 = v.clone().requires_grad_(), q.clone().requires_grad_()
    o1 = MF.got_tiled(v1, q1)
    (o1[0] + o1[1]).backward()
    parts_ = [(v[:1].clone().requires_grad_(), q[:1].clone().requires_grad_()), (v[1:].clone().requires_grad_(), q[1:].clone().requires_grad_())]
    mms = [MF.got_tiled(hv.detach(), hq.detach(), return_extrema=True)[1] for hv, hq in parts_]
    mmg = torch.stack([torch.minimum(mms[0][0::2], mms[1][0::2]), torch.maximum(mms[0][1::2], mms[1][1::2])], 1).reshape(6).contiguous()
    dms = []
    for hv, hq in parts_:   # pass 1: each part's d_minmax (what the all-reduce would sum)
        o = MF.got_tiled(hv.detach().clone().requires_grad_(), hq.detach(), minmax_in=mmg,
                         reduce_dminmax=lambda d: (dms.append(d.clone()), d)[1])
        (o[0] + o[1]).backward()
    total = dms[0] + dms[1]
    outs = []
    for hv, hq in parts_:   # pass 2: finish with the total
        o = MF.got_tiled(hv, hq, minmax_in=mmg, reduce_dminmax=lambda d: total)
        (o[0] + o[1]).backward()
        outs.append(o.detach())
    s = outs[0] + outs[1]
    e = float(((s - o1.detach()).abs() / o1.detach().abs()).max())
    dv = torch.cat([parts_[0][0].grad, parts_[1][0].grad])
    dq = torch.cat([parts_[0][1].grad, parts_[1][1].grad])
    print(f"\ngot_rect data parallel: distances {e:.2e} dV {rel_err(dv, v1.grad):.2e} dQ {rel_err(dq, q1.grad):.2e}")
    assert e < 1e-5
    assert rel_err(dv, v1.grad) < 1e-5 and rel_err(dq, q1.grad) < 1e-5


def test_got_rect_deterministic(dev):
    """Two forward + backward calls give identical bits, the second one after a call at a larger shape, so that the cached workspace
    holds stale data where this shape has its padding columns: at (2, 513, 700, 128) and at (3, 70, 33, 128) (m % 4 != 0)."""
    from madeleine_amd import functional as MF
    for shape, big in (((2, 513, 700, 128), (2, 600, 801, 128)), ((3, 70, 33, 128), (3, 90, 47, 128))):
        v, q = inputs(*shape)
        outs = []
        for rep in range(2):
            if rep:
                _run(*inputs(*big), dev, MF.got_tiled)
            loss, dv, dq = _run(v, q, dev, MF.got_tiled)
            outs.append((loss.clone(), dv.clone(), dq.clone()))
        for a, b in zip(outs[0], outs[1]):
            assert torch.equal(a, b), shape


def test_got_rect_partial_grads_and_bf16(dev):
    """Gradients when only v or only q requires grad equal those of the full call; bf16 inputs are computed in fp32."""
    from madeleine_amd import GOT
    v, q = inputs(2, 40, 56, 128)
    _, dv, dq = _run(v, q, dev)
    a = v.to(dev).requires_grad_()
    GOT(a, q.to(dev), subsample=None).backward()
    assert torch.equal(a.grad, dv)
    b = q.to(dev).requires_grad_()
    GOT(v.to(dev), b, subsample=None).backward()
    assert torch.equal(b.grad, dq)
    vb, qb = v.to(dev).bfloat16(), q.to(dev).bfloat16()
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        lb = GOT(vb, qb, subsample=None)
    lf = GOT(vb.float(), qb.float(), subsample=None)
    assert lb.dtype == torch.float32 and torch.equal(lb, lf)
    # subsample with n != m: the same indices on both sides, equal lengths afterwards (k = 2 <= min(n, m))
    torch.manual_seed(3)
    ls = GOT(v.to(dev), q.to(dev), subsample=256)
    torch.manual_seed(3)
    idx = torch.randperm(2)[:256].to(dev)
    assert torch.equal(ls, GOT(v.to(dev).index_select(1, idx), q.to(dev).index_select(1, idx), subsample=None))


def test_got_rect_issues_no_library_gemm(dev):
    """GOT() forward + backward at (2, 130, 200, 128) under the torch profiler: no aten matmul / GEMM op."""
    from torch.profiler import ProfilerActivity, profile
    from madeleine_amd import GOT
    v, q = inputs(2, 130, 200, 128)
    vd, qd = v.to(dev).requires_grad_(), q.to(dev).requires_grad_()
    GOT(vd, qd, subsample=None).backward()
    with profile(activities=[ProfilerActivity.CPU]) as prof:
        loss = GOT(vd, qd, subsample=None)
        loss.backward()
    torch.cuda.synchronize()
    names = {e.name for e in prof.events()}
    assert not (names & set(GEMM_OPS)), sorted(names & set(GEMM_OPS))
    assert torch.isfinite(loss)
