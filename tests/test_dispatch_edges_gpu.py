"""Every kernel launcher on both sides of its dispatch thresholds.  The launchers pick, from the shape, a tile, a persistent or plain
grid, a token-split count for the dW-type contractions and a GOT size class; the other parity tests reach those branches by the shapes
they happen to use.  Here each parametrization is named after the branch it targets, first asserts through mdl_dispatch_plan (with the
device's own CU count) that the launcher really takes that branch, and then checks the kernel against a plain fp64 reference of the same
operation on the CPU:
  - split-engine products: the fp32-fmaf-chain contract of tests/test_split_gpu.py (elementwise |error| < 4e-7 sum |a b|, 1e-6 relative);
  - exact-fp32 products: the 1e-6 relative tolerance of the exact-fp32 kernels (plus an elementwise 1e-6 sum |a b|);
  - bf16 products: fp64 of the same bf16-representable operands with the output-rounding bounds of tests/test_bf16_gpu.py;
  - gates with RNG dropout: the masks exported by mdl_abmil_gate_dropout_mask replayed in fp64, p in {0.1, 0.3} (16-bit hash fields)
    beside 0.25 (byte fields), with the gate bounds of tests/test_hip_kernels.py / tests/test_bf16_gpu.py;
  - GOT: the fp64 oracle with the tolerances of tests/test_hip_kernels.py::test_got_large_n_vs_fp64_oracle.
Workspaces are taken from memory just filled with NaN, so a split slab a kernel leaves unwritten shows in the result.
The shape of each branch is stated in the comment beside its parametrization, in the form the plan query reports it."""
import pytest
import torch

from oracle import restatement as R
from tests._util import max_rel, rel_err

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
EPS_BF16 = 2.0 ** -8
TOL = 1e-3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _expect_plan(product, T, a, b, want):
    """The launcher of `product` takes the branch `want` (a dict of plan fields) for this shape on this device."""
    from madeleine_amd import _native
    p = _native.dispatch_plan(product, T, a, b, cus=_cus())
    assert {k: p[k] for k in want} == want, (product, T, a, b, p)
    return p


def _u(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float32) * 2 - 1) * scale


def _bf(x):
    return x.to(BF).float()


def _poison(dev, nbytes):
    """Leave `nbytes` of NaN in the allocator's cache: the workspaces allocated next are carved from it."""
    torch.full((int(nbytes) // 4 + 1024,), float("nan"), device=dev)


def _mm(a, b, step=32768):
    """a [M, K] @ b [K, N] in fp64 on the CPU, by row blocks of a."""
    b = b.double()
    return torch.cat([a[i:i + step].double() @ b for i in range(0, a.shape[0], step)])


def _tn(a, b, step=32768):
    """a^T b over the rows (tokens) of a [T, M] and b [T, N], in fp64 on the CPU, by token blocks."""
    out = torch.zeros(a.shape[1], b.shape[1], dtype=torch.float64)
    for i in range(0, a.shape[0], step):
        out += a[i:i + step].double().t() @ b[i:i + step].double()
    return out


def _chain_check(got, ref, mag, elem_tol, what):
    got = got.detach().double().cpu()
    assert rel_err(got, ref) < 1e-6, what
    assert float(((got - ref).abs() / mag.clamp_min(1e-30)).max()) < elem_tol, what


# ------------------------------------------------------------------------------------------------------------------ split TN (dW) product
@pytest.mark.parametrize("T,Mi,N,want", [
    pytest.param(32, 512, 512, dict(splits=1, tps=32, empty=0), id="S1_one_chunk"),                  # S=1, tps=32: one chunk
    pytest.param(33, 512, 512, dict(splits=1, tps=64, empty=0), id="S1_two_chunks_last_partial"),    # S=1, tps=64: 2 chunks, the 2nd 1 token
    pytest.param(64, 256, 512, dict(splits=1, tps=64, empty=0), id="S1_two_full_chunks"),            # S=1, tps=64: 2 whole chunks
    pytest.param(4097, 512, 512, dict(splits=2, tps=2080, empty=0), id="S2_last_split_short"),       # S=2, tps=2080, last split 2017 tokens
    pytest.param(126977, 512, 512, dict(splits=64, tps=2016, empty=1), id="S64_last_split_empty"),   # S=64, tps=2016, last split empty
    pytest.param(172039, 768, 256, dict(splits=86, tps=2016, empty=0), id="S86_above_64"),           # S=86 (> 64), last split 679 tokens
    pytest.param(258055, 512, 256, dict(splits=128, tps=2048, empty=1), id="S128_max_last_empty"),   # S=128 (largest reachable), last empty
])
def test_split_tn_token_splits(dev, T, Mi, N, want):
    """mdl_split_gemm_tn (sp_tn_kernel, the three-stage ring of sp_tn_mainloop3 + the slab reduction) at every split shape."""
    from madeleine_amd import _native
    from madeleine_amd import functional as MF
    _expect_plan("split_tn", T, Mi, N, want)
    x, dy = _u((T, Mi), 11 + T), _u((T, N), 12 + T, 0.5)
    A, B = MF.split_image(x.to(dev)), MF.split_image(dy.to(dev), pad_rows=32)
    _poison(dev, _native.lib().mdl_split_gemm_tn_ws_bytes(T, Mi, N) + N * Mi * 4)
    out = MF.split_gemm_tn(A, B)
    _chain_check(out, _tn(dy, x), _tn(dy.abs(), x.abs()), 4e-7, "dW")


# ------------------------------------------------------------------------------------------------------------------------------- gates
def _gate_inputs(T, H, seed, bf16):
    s = 512 ** -0.5
    E = _u((T, H * 512), seed)
    Wa, Wb = _u((H, 512, 512), seed + 1, s), _u((H, 512, 512), seed + 2, s)
    if bf16:
        E, Wa, Wb = _bf(E), _bf(Wa), _bf(Wb)
    ba, bb, wc = _u((H, 512), seed + 3, s), _u((H, 512), seed + 4, s), _u((H, 512), seed + 5, s)
    bc = _u((H,), seed + 6, s)
    ds = _u((T, H), seed + 7)
    return E, (Wa, ba, Wb, bb, wc, bc), ds


def _masks(dev, T, H, p, seed):
    from madeleine_amd import _native
    lib = _native.lib()
    out = []
    for which in (0, 1):
        m = torch.empty(T, H, 512, dtype=torch.uint8, device=dev)
        _native.check(lib.mdl_abmil_gate_dropout_mask(m.data_ptr(), T, H, which, p, seed, torch.cuda.current_stream().cuda_stream), "mask")
        out.append(m.cpu())
    return out


def _gate64(E, w, ds, p, ka, kb):
    """s[t,c] = bc[c] + sum_j wc[c,j] drop(tanh(E Wa^T + ba)) drop(sigmoid(E Wb^T + bb)) in fp64, head by head (head-major E), and the
    gradients of sum(s * ds): [scores, dE, dWa, dba, dWb, dbb, dwc, dbc]."""
    T, H = ds.shape
    leaves = [x.double().requires_grad_() for x in (E,) + tuple(w)]
    E64, Wa, ba, Wb, bb, wc, bc = leaves
    cols = []
    for c in range(H):
        x = E64[:, c * 512:(c + 1) * 512]
        a = torch.tanh(x @ Wa[c].t() + ba[c])
        b = torch.sigmoid(x @ Wb[c].t() + bb[c])
        if p > 0:
            a = a * ka[:, c].double() / (1 - p)
            b = b * kb[:, c].double() / (1 - p)
        cols.append((a * b) @ wc[c] + bc[c])
    s = torch.stack(cols, dim=1)
    s.backward(ds.double())
    return [s.detach()] + [x.grad for x in leaves]


def _gate_run(dev, E, w, ds, p, seed, dtype, ws_bytes):
    from madeleine_amd import functional as MF
    Ed = E.to(dev).to(dtype).requires_grad_()
    ps = [x.to(dev).requires_grad_() for x in w]
    sc = MF.gate_scores(Ed, *ps, p_drop=p, seed=seed)
    _poison(dev, 2 * ws_bytes)
    sc.backward(ds.to(dev))
    torch.cuda.synchronize()
    return [sc.detach().cpu(), Ed.grad.float().cpu()] + [x.grad.cpu() for x in ps]


GATE_NAMES = ["scores", "dE", "dWa", "dba", "dWb", "dbb", "dwc", "dbc"]


def _check_gate_fp32(got, ref):
    """tests/test_hip_kernels.py::test_gate_eval's bounds."""
    assert rel_err(got[0], ref[0]) < 1e-5 and max_rel(got[0], ref[0]) < TOL, "scores"
    for n, a, b in zip(GATE_NAMES[1:], got[1:], ref[1:]):
        assert rel_err(a, b) < 1e-4, n
        assert max_rel(a, b) < TOL, n


@pytest.mark.parametrize("mode,T,H,p,want", [
    pytest.param("split", 32, 4, 0.1, dict(splits=1, tps=32), id="split-S1_one_chunk-p0.1"),              # S=1, tps=32: one chunk
    pytest.param("split", 33, 4, 0.3, dict(splits=1, tps=64), id="split-S1_two_chunks-p0.3"),             # S=1, tps=64: 2nd chunk 1 token
    pytest.param("split", 4097, 4, 0.25, dict(splits=2, tps=2080), id="split-S2_last_split_short-p0.25"),  # S=2, tps=2080, last 2017
    pytest.param("split", 4097, 2, 0.1, dict(splits=2, tps=2080), id="split-H2_S2-p0.1"),                  # S=2, tps=2080 (H=2)
    pytest.param("fp32", 40, 4, 0.3, dict(splits=1, tps=48), id="fp32-S1_three_chunks-p0.3"),             # S=1, tps=48: 16-token chunks
    pytest.param("fp32", 4097, 4, 0.1, dict(splits=2, tps=2064), id="fp32-S2_last_split_short-p0.1"),    # S=2, tps=2064, last 2033
    pytest.param("fp32", 4097, 4, 0.25, dict(splits=2, tps=2064), id="fp32-S2-p0.25"),                    # S=2, tps=2064, byte-field hash
])
def test_gate_fp32_values_vs_fp64(dev, mode, T, H, p, want):
    """The gate on fp32 token embeddings: the split engine (default GEMM mode) and the exact-fp32 kernels (GEMM mode 'fp32'), forward and
    backward with the in-kernel dropout RNG, against fp64 with the exported masks."""
    from madeleine_amd import _native
    from madeleine_amd import functional as MF
    product = "gate_split_bwd" if mode == "split" else "gate_fp32_bwd"
    _expect_plan(product, T, H, 0, want)
    if mode == "split":
        _expect_plan("gate_split_fwd", T, H, 0, dict(persist=0))
    E, w, ds = _gate_inputs(T, H, 100 + T + H, bf16=False)
    seed = 4242 + T
    ka, kb = _masks(dev, T, H, p, seed)
    lib = _native.lib()
    ws = lib.mdl_abmil_gate_bwd_split_ws_bytes(T, H) if mode == "split" else lib.mdl_abmil_gate_bwd_ws_bytes(T, H)
    old = MF.gemm_mode()
    MF.set_gemm_mode(mode)
    try:
        got = _gate_run(dev, E, w, ds, p, seed, torch.float32, ws)
    finally:
        MF.set_gemm_mode(old)
    _check_gate_fp32(got, _gate64(E, w, ds, p, ka, kb))


@pytest.mark.parametrize("T,H,p,want_fwd,want_bwd", [
    pytest.param(40, 4, 0.25, dict(variant=128), dict(variant=128, extra=128, splits=1, tps=64),
                 id="S1_two_chunks-p0.25"),                     # fwd 128 tile; dX 128; dW 128 kernel, S=1, tps=64: 2nd chunk 8 tokens
    pytest.param(4095, 4, 0.1, dict(variant=128), dict(variant=128, extra=128, splits=1),
                 id="fwd128_dx128-p0.1"),                       # T=4095: fwd 128 tile, dX 128 tile, dW 128 kernel, S=1
    pytest.param(4096, 4, 0.3, dict(variant=256, persist=0), dict(variant=128, extra=256, splits=1),
                 id="fwd256_dx256-p0.3"),                       # T=4096: fwd 256 tile (plain grid), dX 256 tile, dW 128 kernel, S=1
    pytest.param(16383, 4, 0.25, dict(variant=256, persist=1), dict(variant=128, extra=256, splits=8),
                 id="fwd256_persistent_dw128-p0.25"),           # fwd 256 persistent; dW 128 kernel, S=8
    pytest.param(16384, 4, 0.1, dict(variant=256, persist=1), dict(variant=256, extra=256, splits=8),
                 id="dw256-p0.1"),                              # dW 256 kernel from T=16384, S=8
    pytest.param(20000, 4, 0.3, dict(variant=256, persist=0), dict(variant=256, splits=8),
                 id="fwd256_plain_dw256-p0.3"),                 # fwd 256 plain grid (persistence does not pay); dW 256, S=8
    pytest.param(61441, 1, 0.25, dict(variant=256), dict(variant=256, splits=32, tps=1984, empty=1),
                 id="dw256_S32_last_split_empty-p0.25"),       # H=1: S=32, tps=1984, last split empty
])
def test_gate_bf16_vs_fp64(dev, T, H, p, want_fwd, want_bwd):
    """The bf16 gate (mdl_abmil_gate_fwd_bf16 / mdl_abmil_gate_bwd_bf16) on each side of its tile, persistence and dW-kernel thresholds,
    against fp64 of the same bf16-representable E and weights, with the bounds of tests/test_bf16_gpu.py::test_gate_bf16_vs_fp32_kernel
    (bf16 rounding of the stored activations and of dz / dE)."""
    from madeleine_amd import _native
    _expect_plan("gate_bf16_fwd", T, H, 0, want_fwd)
    _expect_plan("gate_bf16_bwd", T, H, 0, want_bwd)
    E, w, ds = _gate_inputs(T, H, 300 + T + H, bf16=True)
    seed = 777 + T
    ka, kb = _masks(dev, T, H, p, seed)
    got = _gate_run(dev, E, w, ds, p, seed, BF, _native.lib().mdl_abmil_gate_bwd_bf16_ws_bytes(T, H))
    ref = _gate64(E, w, ds, p, ka, kb)
    scale = float(ref[0].abs().max())
    assert float((got[0].double() - ref[0]).abs().max()) < 2 * EPS_BF16 * scale, "scores"
    for i in range(1, 8):
        tol = 5e-3 if GATE_NAMES[i] != "dbc" else 1e-5
        assert rel_err(got[i], ref[i]) < tol, GATE_NAMES[i]


# ------------------------------------------------------------------------------------------------------------------------------ Linears
def _linear_case(T, N, K, seed, bf16):
    x, W = _u((T, K), seed), _u((N, K), seed + 1, K ** -0.5)
    b, dy = _u((N,), seed + 2, 0.1), _u((T, N), seed + 3)
    if bf16:
        x, W, dy = _bf(x), _bf(W), _bf(dy)
    return x, W, b, dy


def _linear_run(dev, x, W, b, dy, dtype, ws_bytes):
    from madeleine_amd import functional as MF
    xd = x.to(dev).to(dtype).requires_grad_()
    Wd, bd = W.to(dev).requires_grad_(), b.to(dev).requires_grad_()
    y = MF.linear(xd, Wd, bd)
    assert y.dtype == dtype
    _poison(dev, 2 * ws_bytes)
    y.backward(dy.to(dev).to(dtype))
    torch.cuda.synchronize()
    return y.detach().float().cpu(), xd.grad.float().cpu(), Wd.grad.cpu(), bd.grad.cpu()


@pytest.mark.parametrize("T,N,K,want_fwd,want_bwd", [
    pytest.param(4095, 1024, 1024, dict(variant=4), dict(extra=4, variant=128, splits=1),
                 id="nt128_below_T4096"),                       # T=4095: fwd / dX on the 128 x 256 tile
    pytest.param(4096, 1024, 1024, dict(variant=256, persist=1), dict(extra=256, persist=1, variant=128, splits=1),
                 id="nt256_from_T4096_Kc1024"),                 # T=4096, Kc=1024: fwd / dX on the 256 tile, one tile per workgroup
    pytest.param(4096, 1024, 512, dict(variant=256, persist=4), dict(extra=256, persist=1),
                 id="nt256_persistent_Kc512_4_col_tiles"),      # Kc=512, n_out/256=4: fwd 256 tile, 4 tiles per workgroup; dX (Kc=1024) 256 tile
    pytest.param(4096, 768, 512, dict(variant=4), dict(extra=4),
                 id="nt128_Kc512_3_col_tiles"),                 # Kc=512, n_out/256=3: fwd stays on the 128 x 256 tile
    pytest.param(4096, 256, 1056, dict(variant=4), dict(extra=4),
                 id="nt128_Kc_not_multiple_of_64"),             # Kc=1056 (% 64 != 0): fwd on the 128 x 256 tile
    pytest.param(16383, 256, 512, dict(variant=4), dict(variant=128, splits=4, empty=0),
                 id="tn128_below_T16384"),                      # T=16383: dW on the 128 tile, S=4
    pytest.param(16384, 256, 512, dict(variant=4), dict(variant=256, splits=4, tps=4096, empty=0),
                 id="tn256_from_T16384"),                       # T=16384, N%256==0: dW on the 256 tile, S=4
    pytest.param(16384, 384, 256, dict(variant=2), dict(variant=128),
                 id="tn128_N_not_multiple_of_256"),             # N=384: dW on the 128 tile, fwd on the 128-column tile
    pytest.param(258055, 256, 512, dict(variant=4), dict(variant=256, splits=127, tps=2048, empty=0),
                 id="tn256_S127_above_64"),                     # S=127 (> 64; recomputed from tps: no empty split), last split 7 tokens
])
def test_linear_bf16_vs_fp64(dev, T, N, K, want_fwd, want_bwd):
    """mdl_linear_fwd_bf16 / mdl_linear_bwd_bf16 on each side of the 256-tile NT / TN predicates against fp64 of the same
    bf16-representable operands: Y, dX within one bf16 rounding of the output (2^-8), dW, dbias 1e-5 (tests/test_bf16_gpu.py)."""
    from madeleine_amd import _native
    _expect_plan("linear_bf16_fwd", T, N, K, want_fwd)
    _expect_plan("linear_bf16_bwd", T, N, K, want_bwd)
    x, W, b, dy = _linear_case(T, N, K, 500 + T + N + K, bf16=True)
    y, dx, dW, db = _linear_run(dev, x, W, b, dy, BF, _native.lib().mdl_linear_bwd_bf16_ws_bytes(T, N, K))
    y64 = _mm(x, W.t()) + b.double()
    assert float((y.double() - y64).abs().max()) <= EPS_BF16 * float(y64.abs().max())
    assert rel_err(y, y64) < EPS_BF16
    assert rel_err(dx, _mm(dy, W)) < EPS_BF16
    assert rel_err(dW, _tn(dy, x)) < 1e-5
    assert rel_err(db, dy.double().sum(0)) < 1e-5


@pytest.mark.parametrize("T,N,K,want", [
    pytest.param(4097, 256, 512, dict(variant=1, splits=2, tps=2064), id="wide_N256_S2"),       # lin_wide: S=2, tps=2064, last 2033
    pytest.param(4097, 128, 512, dict(variant=2, splits=2, tps=2064), id="swapped_N128_S2"),    # N%256 != 0: roles swapped, S=2
    pytest.param(1000, 384, 256, dict(variant=2, splits=1, tps=1008), id="swapped_N384_S1"),    # N=384: roles swapped, S=1, partial chunk
    pytest.param(192514, 512, 512, dict(variant=1, splits=96, tps=2016, empty=0), id="wide_S96_above_64"),   # S=96 (> 64), last 1018
])
def test_linear_fp32_vs_fp64(dev, T, N, K, want):
    """mdl_linear_fwd / mdl_linear_bwd (exact fp32, GEMM mode 'fp32'): the wide tile against the role-swapped one, and the token splits
    of the dW contraction, against fp64 at the exact-fp32 kernels' 1e-6."""
    from madeleine_amd import _native
    from madeleine_amd import functional as MF
    _expect_plan("linear_fp32_bwd", T, N, K, want)
    x, W, b, dy = _linear_case(T, N, K, 900 + T + N + K, bf16=False)
    old = MF.gemm_mode()
    MF.set_gemm_mode("fp32")
    try:
        y, dx, dW, db = _linear_run(dev, x, W, b, dy, torch.float32, _native.lib().mdl_linear_bwd_ws_bytes(T, N, K))
    finally:
        MF.set_gemm_mode(old)
    _chain_check(y, _mm(x, W.t()) + b.double(), _mm(x.abs(), W.abs().t()) + b.double().abs(), 1e-6, "Y")
    _chain_check(dx, _mm(dy, W), _mm(dy.abs(), W.abs()), 1e-6, "dX")
    _chain_check(dW, _tn(dy, x), _tn(dy.abs(), x.abs()), 1e-6, "dW")
    _chain_check(db, dy.double().sum(0), dy.double().abs().sum(0), 1e-6, "dbias")


# ------------------------------------------------------------------------------------------------------------------------------------ GOT
def _got_check(dev, k, n, seed):
    from madeleine_amd import functional as MF
    g = torch.Generator().manual_seed(seed)
    v = torch.rand((k, n, 128), generator=g) * 2 - 1
    q = torch.rand((k, n, 128), generator=g) * 2 - 1 + 0.7 * v
    v64, q64 = v.double().requires_grad_(), q.double().requires_grad_()
    ref = R.got(v64, q64)
    ref.backward()
    vd, qd = v.to(dev).requires_grad_(), q.to(dev).requires_grad_()
    o = MF.got(vd, qd)
    (o[0] + o[1]).backward()
    assert abs(float(o.sum()) - float(ref)) < TOL * abs(float(ref))
    assert rel_err(vd.grad, v64.grad) < TOL and rel_err(qd.grad, q64.grad) < TOL


@pytest.mark.parametrize("n,cls", [
    pytest.param(64, 64, id="n64_class64"), pytest.param(65, 128, id="n65_class128"),        # fused kernel: n <= 64 | n <= 128
    pytest.param(128, 128, id="n128_class128"), pytest.param(129, 192, id="n129_class192"),  # n = 129: per-phase launches, 12 x 3 plans
    pytest.param(192, 192, id="n192_class192"), pytest.param(193, 256, id="n193_class256"),  # n = 193: the 16 x 4 plan registers
])
def test_got_size_classes(dev, n, cls):
    """GOT on each side of the n-class limits (k = 2: split sweeps on where the class has them) against the fp64 oracle."""
    _expect_plan("got", 2, n, 0, dict(variant=cls))
    _got_check(dev, 2, n, 40 + n)


@pytest.mark.parametrize("which,n", [
    pytest.param("4k_launch", 193, id="K_eq_cus_over_4-split_4k-n193"),       # K = CUs/4: split sweeps, both sweeps in one 4K launch
    pytest.param("2k_launches", 193, id="K_cus_over_4_plus_1-split_2k-n193"),  # K = CUs/4 + 1: split sweeps, the two as 2K launches
    pytest.param("2k_launches", 129, id="K_eq_cus_over_2-split_2k-n129"),      # K = CUs/2: the last K with split sweeps / half products
    pytest.param("whole", 129, id="K_cus_over_2_plus_1-whole_sweeps-n129"),    # K = CUs/2 + 1: whole sweeps, whole products
])
def test_got_case_count_limits(dev, which, n):
    """The split IPOT sweeps and row-half products of the per-phase classes exist only while 2K (4K) workgroups fit the CUs at once:
    the case counts on each side of those limits, taken from the device's CU count, against the fp64 oracle."""
    cus = _cus()
    k, want = {"4k_launch": (cus // 4, dict(extra=2, persist=1)), "2k_launches": (cus // 4 + 1, dict(extra=1, persist=1)),
               "whole": (cus // 2 + 1, dict(extra=0, persist=0))}[which]
    if which == "2k_launches" and n == 129:
        k = cus // 2
    _expect_plan("got", k, n, 0, want)
    _got_check(dev, k, n, 70 + k + n)
