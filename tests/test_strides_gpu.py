"""Every strided entry point of the C ABI at row strides wider than its rows.  The Python API is contiguous-only, so nothing else in the
suite runs a kernel with ld != width; here every operand that has a stride argument is a view of a wider buffer, in two layouts:
  pad   the minimal pad the ABI allows: ld = width + 4 fp32 / + 8 bf16 elements (rsb = 4 K + 16 bytes for an image) for the first stride
        argument of a call, one more such unit for every further one, so that two strides used in each other's place cannot cancel;
  view  the column slice buf[:, 4 : 4 + width] (bf16: 8 : 8 + width) of a buffer width + 36 (bf16: + 40) elements wide, again one unit
        wider per further stride argument: the base pointer sits 16 bytes into the allocation.
Padding columns of inputs hold NaN; outputs (padding included) and workspaces start as NaN; accumulating calls get finite contents in
the valid region only.  Every case asserts
  (a) the valid region of every output equals, bit for bit, the same call on contiguous copies -- no kernel here uses floating-point
      atomics on its results and no launcher picks a branch by stride, so a stride may change addresses and nothing else;
  (b) every padding element of every output buffer still holds its fill pattern (compared as integers);
  (c) the valid region agrees with a plain fp64 CPU reference within the bound the suite already states for that kernel
      (tests/test_dispatch_edges_gpu.py, tests/test_hip_kernels.py, tests/test_bf16_gpu.py, tests/test_ragged_views_gpu.py).
Shapes are the smallest that reach each tile and a ragged tail; where a shape is chosen for a branch the plan query is asserted first.

The pads here are 4 to 40 elements: they show that a kernel uses the stride it is given, not that its 32-bit offsets hold up to the limit
the launcher accepts.  tests/test_stride_limits_gpu.py runs the runners of this file (_run_gate, _run_linear, the *_runner functions) a
second time on the layout of tests/_wide_cases.py: every stride argument with a limit AT its limit, with rows past byte 2^32, and every
limit-free one (the pooling family, the image writers) with rows past element 2^31.  Still not run anywhere: the exact 32-bit edge of
the kernels listed in _wide_cases.ARGUED, whose smallest T times the limit stride exceeds any buffer a test should take."""
import functools

import numpy as np
import pytest
import torch

from tests._util import max_rel, rel_err
from tests.test_dispatch_edges_gpu import (_chain_check, _check_gate_fp32, _expect_plan, _gate64, _gate_inputs, _linear_case, _mm, _poison,
                                           _tn, _u)

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F32 = torch.float32
EPS_BF16 = 2.0 ** -8
TOL = 1e-3
NAN = float("nan")
MODES = ["pad", "view"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _bits(x):
    x = x.contiguous()
    return x.view(torch.int16 if x.element_size() == 2 else torch.int32 if x.element_size() == 4 else torch.uint8)


class Lay:
    """Allocates the strided operands of one call sequence in one layout ('contig', 'pad' or 'view') and remembers every output buffer
    with its contents before the call, for the stray-write check.  k = index of the stride argument within its call."""

    def __init__(self, mode, dev):
        self.mode, self.dev, self.outs = mode, dev, []

    def buf(self, rows, width, dtype, k):
        unit = 8 if dtype == BF else 4
        if self.mode == "contig":
            ld, off = width, 0
        elif self.mode == "pad":
            ld, off = width + (k + 1) * unit, 0
        else:
            ld, off = width + (40 if dtype == BF else 36) + k * unit, unit
        b = torch.full((rows, ld), NAN, dtype=dtype, device=self.dev)
        v = b[:, off:off + width]
        assert v.data_ptr() % 16 == 0 and (v.stride(0) * v.element_size()) % 16 == 0
        return b, v

    def inp(self, x, k=0, dtype=None):
        _, v = self.buf(x.shape[0], x.shape[1], dtype or x.dtype, k)
        v.copy_(x.to(self.dev))
        return v

    def out(self, rows, width, dtype=F32, k=0, init=None):
        b, v = self.buf(rows, width, dtype, k)
        if init is not None:
            v.copy_(init.to(self.dev))
        self.outs.append((b, v, _bits(b).clone()))
        return v

    def track(self, v_of_b):
        """Registers an input buffer that a later call writes (an image built in place), as out() does."""
        b, v = v_of_b
        self.outs.append((b, v, _bits(b).clone()))

    def check_padding(self):
        for b, v, before in self.outs:
            after = _bits(b).clone()
            off = v.storage_offset() - b.storage_offset()
            after[:, off:off + v.shape[1]] = 0
            before[:, off:off + v.shape[1]] = 0
            assert torch.equal(after, before), "a kernel wrote outside the valid columns of an output"


def _strided_vs_contiguous(dev, mode, run, check_ref, lay=None):
    """run(lay) -> {name: output tensor (valid region)}: runs it contiguously and in `mode`, asserts (a), (b) and, through
    check_ref(outputs as CPU tensors), (c).  `lay`: a layout object of the caller's (tests/test_stride_limits_gpu.py) in place of
    Lay(mode); its check_padding() may clear the buffers it scans, so the outputs are copied out first."""
    base = run(Lay("contig", dev))
    torch.cuda.synchronize()
    base = {k: v.clone() for k, v in base.items()}
    lay = Lay(mode, dev) if lay is None else lay
    got = run(lay)
    torch.cuda.synchronize()
    got = {k: v.clone() for k, v in got.items()}
    assert set(got) == set(base)
    for k in sorted(got):
        assert torch.equal(_bits(got[k]), _bits(base[k])), "%s differs from the contiguous call (%s)" % (k, mode)
    lay.check_padding()
    # (fp32 and bf16 outputs reach the check as fp32, as they always did; fp64 and integer outputs of the newer families as they are)
    check_ref({k: v.float().cpu() if v.is_floating_point() and v.dtype != torch.float64 else v.cpu() for k, v in got.items()})


def _nan(dev, *shape, dtype=F32):
    return torch.full(shape, NAN, dtype=dtype, device=dev)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ws(dev, query, *sizes):
    """A workspace of NaN, sized by the entry point's own query."""
    from madeleine_amd import _native
    n = getattr(_native.lib(), query)(*sizes)
    assert n >= 0, (query, sizes, n)
    return _nan(dev, n // 4 + 16)


# ============================================================================================================================== gates
def _bags_of(T, ragged):
    """Bag lengths over T tokens: four equal (dense) bags, or ragged ones with a single-token bag."""
    if not ragged:
        assert T % 4 == 0
        return [T // 4] * 4
    return [T - T // 3 - 1, 1, T // 3]


@functools.lru_cache(maxsize=None)
def _gate_case(T, H, p, bf16):
    """Inputs, explicit keep masks and the fp64 results of the gate, plus a pooling term (scores of the fp64 forward, a dense and a ragged
    bag split) for the fused attnpool backward: pool[ragged]['term'] = w[t, c] d_pooled[bag(t), c, :].
    The bias gradients are column sums over the tokens, sum_t ds[t, c] x[t, c, j] with x of one sign and nearly constant (b (1 - a^2) ~
    0.45): their size is set by sum_t ds[t, c], which for a mean-free random ds is anywhere between 0 and a few sqrt(T / 3), and a
    RELATIVE bound on them (the 5e-3 of the bf16 gate, which stores a and b rounded to 8 bits) only means something when that sum does
    not cancel.  So ds is shifted, by less than 1 / sqrt(T) per element, to make every head's sum exactly one standard deviation of a
    random draw, sqrt(T / 3): typical conditioning by construction instead of by the luck of a seed."""
    E, w, ds = _gate_inputs(T, H, 7000 + T + H, bf16=bf16)
    ds = (ds.double() + ((T / 3.0) ** 0.5 - ds.double().sum(0)) / T).float()
    g = torch.Generator().manual_seed(T + H)
    ka = (torch.rand((T, H, 512), generator=g) >= p).to(torch.uint8) if p > 0 else None
    kb = (torch.rand((T, H, 512), generator=g) >= p).to(torch.uint8) if p > 0 else None
    ref = _gate64(E, w, ds, p, ka, kb)
    dE0 = _u((T, H * 512), 7100 + T)
    if bf16:
        dE0 = dE0.to(BF).float()
    pool = {}
    for ragged in (False, True):
        if not ragged and T % 4:
            continue
        lens = _bags_of(T, ragged)
        row_bag = torch.repeat_interleave(torch.arange(len(lens)), torch.tensor(lens)).to(torch.int32)
        dp = _u((len(lens), H * 512), 7200 + T + ragged)
        sc = ref[0].float()
        m = torch.stack([sc[row_bag == b].max(0).values for b in range(len(lens))])
        l_ = torch.stack([(sc[row_bag == b] - m[b]).double().exp().sum(0) for b in range(len(lens))]).float()
        wgt = (sc.double() - m.double()[row_bag.long()]).exp() / l_.double()[row_bag.long()]                       # [T, H]
        term = (wgt[:, :, None] * dp.double().view(len(lens), H, 512)[row_bag.long()]).reshape(T, H * 512)
        pool[ragged] = dict(lens=lens, row_bag=row_bag, dp=dp, scores=sc, m=m, l=l_, term=term)
    return E, w, ds, ka, kb, ref, dE0, pool


def _gate_variants(T):
    """(name, accumulate, pooling term: None | False (dense) | True (row_bag), entry point) of the backward calls of one case."""
    v = [("gate_bwd", 0, None, "gate_bwd"), ("gate_bwd_acc", 1, None, "gate_bwd"), ("attnpool_ragged_acc", 1, True, "attnpool_bwd"),
         ("phases_ragged", 0, True, "attnpool_bwd_phases")]
    if T % 4 == 0:
        v += [("attnpool_dense", 0, False, "attnpool_bwd"), ("phases_dense_acc", 1, False, "attnpool_bwd_phases")]
    return v


def _gate_ref_dE(case, acc, pterm):
    _, _, _, _, _, ref, dE0, pool = case
    want = ref[1].clone()
    if pterm is not None:
        want = want + pool[pterm]["term"]
    if acc:
        want = want + dE0.double()
    return want


def _run_gate(dev, lay, case, dtype, T, H, p, forward=True, fwd_contig=False):
    """mdl_abmil_gate_fwd, mdl_abmil_gate_bwd, mdl_abmil_attnpool_bwd and mdl_abmil_attnpool_bwd_phases (phases 1, then 2) of one
    storage type on the layout `lay`: E and dE strided (one ldE serves both), everything else contiguous as the ABI has it.
    fwd_contig: the forward that supplies act_a / act_b reads a contiguous copy of E (for an ldE that only the backward accepts)."""
    from madeleine_amd import _native
    from madeleine_amd import functional as MF
    E, w, ds, ka, kb, _, dE0, pool = case
    sfx = "_bf16" if dtype == BF else ""
    lib = _native.lib()
    Ev = lay.inp(E.to(dtype))
    ps = [x.to(dev) for x in w]
    Wa, ba, Wb, bb, wc, bc = ps
    kad, kbd = (ka.to(dev), kb.to(dev)) if p > 0 else (None, None)
    dsd = ds.to(dev)
    out = {}
    _poison(dev, getattr(lib, "mdl_abmil_gate_fwd%s_ws_bytes" % sfx)(T, H) + 3 * T * H * 512 * 4)
    assert not (forward and fwd_contig)
    sc, a, b = MF.gate_fwd_raw(Ev.contiguous() if fwd_contig else Ev, Wa, ba, Wb, bb, wc, bc, p, 11, kad, kbd, True)
    if forward:
        out.update(scores=sc, act_a=a.view(T, -1), act_b=b.view(T, -1))
    for name, acc, pterm, entry in _gate_variants(T):
        dE = lay.out(T, H * 512, dtype, init=dE0 if acc else None)
        grads = [_nan(dev, *x.shape) for x in (Wa, Wb, ba, bb, wc, bc)]
        ws = _ws(dev, "mdl_abmil_gate_bwd%s_ws_bytes" % sfx, T, H)
        args = [Ev, Ev.stride(0), Wa, Wb, wc, a, b, dsd, dE, acc] + grads + [T, H, float(p), 11, kad, kbd]
        if pterm is not None:
            q = pool[pterm]
            args += [q["scores"].to(dev), q["m"].to(dev), q["l"].to(dev), q["dp"].to(dev), q["row_bag"].to(dev) if pterm else None,
                     0 if pterm else q["lens"][0]]
        args += [ws, _stream()]
        assert dE.stride(0) == Ev.stride(0)
        if entry == "attnpool_bwd_phases":
            MF._call("mdl_abmil_" + entry + sfx, *args, 1)
            MF._call("mdl_abmil_" + entry + sfx, *args, 2)
        else:
            MF._call("mdl_abmil_" + entry + sfx, *args)
        out[name + ".dE"] = dE
        for n, gten in zip(("dWa", "dWb", "dba", "dbb", "dwc", "dbc"), grads):
            out[name + "." + n] = gten.view(gten.shape[0], -1)
    return out


GRAD_ORDER = ("dWa", "dba", "dWb", "dbb", "dwc", "dbc")     # the order of _gate64's results after scores and dE


def _check_gate_f32(case, T, got, forward=True):
    """The bounds of the fp32 gate (and of the split one); without the forward, the scores slot of _check_gate_fp32 gets the reference."""
    ref = case[5]
    if forward:
        assert rel_err(got["scores"], ref[0]) < 1e-5 and max_rel(got["scores"], ref[0]) < TOL, "scores"
    for name, acc, pterm, _ in _gate_variants(T):
        res = [got["scores"] if forward else ref[0].float(), got[name + ".dE"]]
        res += [got[name + "." + n].reshape(r.shape) for n, r in zip(GRAD_ORDER, ref[2:])]
        _check_gate_fp32(res, [ref[0], _gate_ref_dE(case, acc, pterm)] + list(ref[2:]))


def _check_gate_b16(case, T, got, forward=True):
    ref = case[5]
    if forward:
        assert float((got["scores"].double() - ref[0]).abs().max()) < 2 * EPS_BF16 * float(ref[0].abs().max()), "scores"
    for name, acc, pterm, _ in _gate_variants(T):
        assert rel_err(got[name + ".dE"], _gate_ref_dE(case, acc, pterm)) < 5e-3, name + ".dE"
        for n, r in zip(GRAD_ORDER, ref[2:]):
            assert rel_err(got[name + "." + n].reshape(r.shape), r) < (1e-5 if n == "dbc" else 5e-3), name + "." + n


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("T,H,p", [(40, 1, 0.0), (40, 4, 0.25), (300, 1, 0.0), (300, 4, 0.0)])
def test_gate_fp32(dev, mode, T, H, p):
    _expect_plan("gate_fp32_bwd", T, H, 0, dict(splits=1))
    case = _gate_case(T, H, p, False)
    _strided_vs_contiguous(dev, mode, lambda lay: _run_gate(dev, lay, case, F32, T, H, p), lambda got: _check_gate_f32(case, T, got))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("T,H,fwd,want_fwd,want_bwd", [
    pytest.param(300, 1, True, dict(variant=128), dict(variant=128, extra=128), id="T300-H1-tiles128"),
    pytest.param(300, 4, True, dict(variant=128), dict(variant=128, extra=128), id="T300-H4-tiles128"),
    pytest.param(4097, 1, True, dict(variant=256), dict(variant=128, extra=256), id="T4097-H1-fwd256-dx256"),     # ragged last 256 tile
    pytest.param(16385, 1, False, dict(variant=256), dict(variant=256, extra=256), id="T16385-H1-dw256-bwd_only"),
])
def test_gate_bf16(dev, mode, T, H, fwd, want_fwd, want_bwd):
    """The bf16 gate: decides whether mdl_abmil_gate_bwd_bf16 needs ldE == H*512 (it does not: its dW kernels read E in place)."""
    _expect_plan("gate_bf16_fwd", T, H, 0, want_fwd)
    _expect_plan("gate_bf16_bwd", T, H, 0, want_bwd)
    case = _gate_case(T, H, 0.0, True)
    _strided_vs_contiguous(dev, mode, lambda lay: _run_gate(dev, lay, case, BF, T, H, 0.0, forward=fwd), lambda got: _check_gate_b16(case, T, got, fwd))


def _image(lay, x, k, pad_rows=0):
    """The split image of x [rows, K] in the layout's k-th image geometry (row stride rsb = 4 * data.stride(0) bytes), built from a
    contiguous x by mdl_split_image: -> (data view [rows + pad_rows, K] of fp32-sized granules, scale)."""
    from madeleine_amd import functional as MF
    rows, K = x.shape
    b, v = lay.buf(rows + pad_rows, K, F32, k)
    scale = _nan(lay.dev, 2)
    MF._call("mdl_split_image", x, x.stride(0), rows, K, v, v.stride(0) * 4, pad_rows, scale, _stream())
    return v, scale


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("T,H", [(300, 1), (4097, 1), (300, 4)])
def test_gate_split(dev, mode, T, H):
    """mdl_abmil_gate_fwd_split and mdl_abmil_attnpool_bwd_split: the image of E at a wide e_rsb, dE at a wide ldE; phases 3, and 1
    followed by 2; plain and with the pooling term."""
    _expect_plan("gate_split_bwd", T, H, 0, dict(splits=2 if T > 4096 else 1))
    case = _gate_case(T, H, 0.0, False)
    _strided_vs_contiguous(dev, mode, lambda lay: _run_gate_split(dev, lay, case, T, H), lambda got: _check_gate_split(case, got))


SPLIT_VARIANTS = [("plain", 0, None, (3,)), ("plain_acc_1_2", 1, None, (1, 2)), ("ragged_acc", 1, True, (3,)), ("ragged_1_2", 0, True, (1, 2))]


def _run_gate_split(dev, lay, case, T, H, forward=True, fwd_contig=False):
    """mdl_abmil_gate_fwd_split and the SPLIT_VARIANTS of mdl_abmil_attnpool_bwd_split: the image of E is stride argument 0, dE is 1.
    fwd_contig: the forward that supplies act_a / act_b reads an image at its contiguous row stride (for an e_rsb that only the
    backward accepts)."""
    from madeleine_amd import functional as MF
    E, w, ds, _, _, _, dE0, pool = case
    Ei, esc = _image(lay, E.to(dev), 0)
    Ef, fsc = _image(Lay("contig", dev), E.to(dev), 0) if fwd_contig else (Ei, esc)
    Wa, ba, Wb, bb, wc, bc = [x.to(dev) for x in w]
    sc, a, b = _nan(dev, T, H), _nan(dev, T, H, 512), _nan(dev, T, H, 512)
    MF._call("mdl_abmil_gate_fwd_split", Ef, Ef.stride(0) * 4, fsc, Wa, ba, Wb, bb, wc, bc, sc, a, b, T, H, 0.0, 11, None, None,
             _ws(dev, "mdl_abmil_gate_fwd_split_ws_bytes", T, H), _stream())
    assert not (forward and fwd_contig)
    out = dict(scores=sc, act_a=a.view(T, -1), act_b=b.view(T, -1)) if forward else {}
    for name, acc, pterm, phases in SPLIT_VARIANTS:
        dE = lay.out(T, H * 512, F32, k=1, init=dE0 if acc else None)
        grads = [_nan(dev, *x.shape) for x in (Wa, Wb, ba, bb, wc, bc)]
        ws = _ws(dev, "mdl_abmil_gate_bwd_split_ws_bytes", T, H)
        q = pool[pterm] if pterm is not None else None
        pt = [q["scores"].to(dev), q["m"].to(dev), q["l"].to(dev), q["dp"].to(dev), q["row_bag"].to(dev), 0] if q else [None] * 5 + [0]
        for ph in phases:
            MF._call("mdl_abmil_attnpool_bwd_split", Ei, Ei.stride(0) * 4, esc, Wa, Wb, wc, a, b, ds.to(dev), dE, dE.stride(0), acc,
                     *grads, T, H, 0.0, 11, None, None, *pt, None, ws, _stream(), ph, 3)
        out[name + ".dE"] = dE
        for n, gten in zip(("dWa", "dWb", "dba", "dbb", "dwc", "dbc"), grads):
            out[name + "." + n] = gten.view(gten.shape[0], -1)
    return out


def _check_gate_split(case, got, forward=True):
    ref = case[5]
    for name, acc, pterm, _ in SPLIT_VARIANTS:
        res = [got["scores"] if forward else ref[0].float(), got[name + ".dE"]]
        res += [got[name + "." + n].reshape(r.shape) for n, r in zip(GRAD_ORDER, ref[2:])]
        _check_gate_fp32(res, [ref[0], _gate_ref_dE(case, acc, pterm)] + list(ref[2:]))


# ============================================================================================================================ pooling
DENSE, RAGGED = (300, 300, 300), (300, 0, 1, 129)


@functools.lru_cache(maxsize=None)
def _pool_case(H, bf16, lens):
    """E, scores, incoming gradients and starting contents for bags of `lens` tokens, with the fp64 softmax pooling, the weighted
    pooling (scores used as weights) and their gradients."""
    T, n, C = sum(lens), len(lens), H * 512
    E = _u((T, C), 8000 + H + T)
    if bf16:
        E = E.to(BF).float()
    s, dp = _u((T, H), 8100 + H + T, 4.0), _u((n, C), 8200 + H + T)
    dE0, ds0 = _u((T, C), 8300 + H), _u((T, H), 8400 + H)
    if bf16:
        dE0 = dE0.to(BF).float()
    cu = np.concatenate([[0], np.cumsum(lens)])
    res = {}
    for lin in (False, True):
        E64, s64 = E.double().requires_grad_(), s.double().requires_grad_()
        rows = []
        for b, L in enumerate(lens):
            sl = slice(int(cu[b]), int(cu[b + 1]))
            wgt = s64[sl] if lin else torch.softmax(s64[sl], dim=0)
            rows.append(torch.einsum("nh,nhe->he", wgt, E64[sl].view(L, H, 512)).reshape(-1) if L else E64.new_zeros(C))
        ref = torch.stack(rows)
        ref.backward(dp.double())
        res[lin] = (ref.detach(), E64.grad, s64.grad)
    return E, s, dp, dE0, ds0, torch.from_numpy(cu), res


def _check_pool(got, pre, ref, dE0, ds0, bf16, acc):
    """The bounds of tests/test_hip_kernels.py::test_pool_fwd_bwd_dense (bf16 dE: one rounding, tests/test_bf16_gpu.py)."""
    pooled, dE, dsc = ref
    assert rel_err(got[pre + "pooled"], pooled) < 1e-5 and max_rel(got[pre + "pooled"], pooled) < TOL, pre + "pooled"
    want = dE + dE0.double() if acc else dE
    if bf16:
        assert rel_err(got[pre + "dE"], want) < EPS_BF16, pre + "dE"
    else:
        assert rel_err(got[pre + "dE"], want) < 1e-5 and max_rel(got[pre + "dE"], want) < TOL, pre + "dE"
    diff = got[pre + "ds"].double() - (ds0.double() if acc else 0.0)
    assert float((diff - dsc).abs().max()) <= 1e-4 * float(dsc.abs().max()) + 1e-6, pre + "d_scores"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("lens", [DENSE, RAGGED], ids=["dense", "ragged"])
@pytest.mark.parametrize("H", [1, 4])
def test_pool(dev, mode, H, lens, bf16):
    """mdl_abmil_pool_fwd / _bwd and mdl_abmil_wpool_fwd / _bwd (fp32 and bf16 E): dE and d_scores written, then accumulated."""
    run, check = _pool_runner(dev, H, lens, bf16)
    _strided_vs_contiguous(dev, mode, run, check)


def _pool_runner(dev, H, lens, bf16):
    """(run, check) of test_pool."""
    from madeleine_amd import functional as MF
    E, s, dp, dE0, ds0, cu, res = _pool_case(H, bf16, lens)
    T, n, C = sum(lens), len(lens), H * 512
    dtype, sfx = (BF, "_bf16") if bf16 else (F32, "")
    dense = lens == DENSE
    geom = (n, lens[0] if dense else 0, None if dense else cu.to(dev), max(lens), H)

    def run(lay):
        Ev, sd, dpd = lay.inp(E.to(dtype)), s.to(dev), dp.to(dev)
        out = {}
        for lin, pre in ((False, "pool."), (True, "wpool.")):
            pooled, m, l_ = _nan(dev, n, C), _nan(dev, n, H), _nan(dev, n, H)
            MF._call("mdl_abmil_%s_fwd%s" % (pre[:-1], sfx), Ev, Ev.stride(0), sd, pooled, m, l_, *geom,
                     _ws(dev, "mdl_abmil_pool_ws_bytes", n, max(lens), H), _stream())
            out[pre + "pooled"] = pooled
            for acc in ((0,) if lin else (0, 1)):      # (the weighted pooling has no accumulate_scores: d_weights is always written)
                dE = lay.out(T, C, dtype, init=dE0 if acc else None)
                dsc = ds0.to(dev).clone() if acc else _nan(dev, T, H)
                if lin:
                    MF._call("mdl_abmil_wpool_bwd" + sfx, Ev, Ev.stride(0), sd, dpd, dE, acc, dsc, *geom, _stream())
                else:
                    MF._call("mdl_abmil_pool_bwd" + sfx, Ev, Ev.stride(0), sd, pooled, m, l_, dpd, dE, acc, dsc, acc, *geom, _stream())
                out["%sacc%d.dE" % (pre, acc)], out["%sacc%d.ds" % (pre, acc)] = dE, dsc
        return out

    def check(got):
        for lin, pre in ((False, "pool."), (True, "wpool.")):
            for acc in ((0,) if lin else (0, 1)):
                g = {"pooled": got[pre + "pooled"], "dE": got["%sacc%d.dE" % (pre, acc)], "ds": got["%sacc%d.ds" % (pre, acc)]}
                _check_pool(g, "", res[lin], dE0, ds0, bf16, acc)
    return run, check


@functools.lru_cache(maxsize=None)
def _view_case(H, bf16):
    """A 129-index view of the dense bags and the two half-bag views of the ragged ones, in fp64 (views accumulate into dE / d_scores)."""
    from madeleine_amd.model import ragged_view_plan
    out = {}
    for ragged in (False, True):
        lens = RAGGED if ragged else DENSE
        E, s, _, dE0, ds0, cu, _ = _pool_case(H, bf16, lens)
        C = H * 512
        g = torch.Generator().manual_seed(90 + H)
        if ragged:
            np.random.seed(91 + H)
            perm, vcu, max_view = ragged_view_plan(lens)
            segs = [perm[int(vcu[k]):int(vcu[k + 1])].long() for k in range(2 * len(lens))]
            plan = (perm, vcu, max_view)
        else:
            idx = torch.randperm(lens[0], generator=g)[:129].to(torch.int32)
            segs = [b * lens[0] + idx.long() for b in range(len(lens))]
            plan = (idx,)
        dp = _u((len(segs), C), 8500 + H + ragged)
        E64, s64 = E.double().requires_grad_(), s.double().requires_grad_()
        rows = [torch.einsum("th,the->he", torch.softmax(s64[r], dim=0), E64[r].view(-1, H, 512)).reshape(-1) if r.numel() else E64.new_zeros(C)
                for r in segs]
        ref = torch.stack(rows)
        ref.backward(dp.double())
        out[ragged] = (lens, plan, dp, (ref.detach(), E64.grad, s64.grad))
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("H", [1, 4])
def test_pool_views(dev, mode, H, bf16):
    """mdl_abmil_pool_view_fwd / _bwd on a 129-index view of the dense bags, mdl_abmil_pool_rview_fwd / _bwd on both half-bag views of the
    ragged bags (an empty bag, a single-token bag whose first view is empty); the backward accumulates onto finite contents."""
    run, check = _pool_views_runner(dev, H, bf16)
    _strided_vs_contiguous(dev, mode, run, check)


def _pool_views_runner(dev, H, bf16):
    """(run, check) of test_pool_views."""
    from madeleine_amd import functional as MF
    cases = _view_case(H, bf16)
    dtype, sfx = (BF, "_bf16") if bf16 else (F32, "")
    C = H * 512

    def run(lay):
        out = {}
        for ragged, pre in ((False, "view."), (True, "rview.")):
            lens, plan, dp, _ = cases[ragged]
            E, s, _, dE0, ds0, _, _ = _pool_case(H, bf16, lens)
            T, n = sum(lens), len(lens)
            Ev, sd, dpd = lay.inp(E.to(dtype)), s.to(dev), dp.to(dev)
            nseg = 2 * n if ragged else n
            pooled, m, l_ = _nan(dev, nseg, C), _nan(dev, nseg, H), _nan(dev, nseg, H)
            dE, dsc = lay.out(T, C, dtype, init=dE0), ds0.to(dev).clone()
            if ragged:
                perm, vcu, max_view = plan[0].to(dev), plan[1].to(dev), plan[2]
                MF._call("mdl_abmil_pool_rview_fwd" + sfx, Ev, Ev.stride(0), sd, pooled, m, l_, n, perm, vcu, max_view, H,
                         _ws(dev, "mdl_abmil_pool_ws_bytes", nseg, max_view, H), _stream())
                MF._call("mdl_abmil_pool_rview_bwd" + sfx, Ev, Ev.stride(0), sd, pooled, m, l_, dpd, dE, dsc, n, perm, vcu, max_view, H, _stream())
            else:
                idx = plan[0].to(dev)
                MF._call("mdl_abmil_pool_view_fwd" + sfx, Ev, Ev.stride(0), sd, pooled, m, l_, n, lens[0], idx, idx.numel(), H,
                         _ws(dev, "mdl_abmil_pool_ws_bytes", n, idx.numel(), H), _stream())
                MF._call("mdl_abmil_pool_view_bwd" + sfx, Ev, Ev.stride(0), sd, pooled, m, l_, dpd, dE, dsc, n, lens[0], idx, idx.numel(), H,
                         _stream())
            out[pre + "pooled"], out[pre + "dE"], out[pre + "ds"] = pooled, dE, dsc
        return out

    def check(got):
        for ragged, pre in ((False, "view."), (True, "rview.")):
            lens, _, _, ref = cases[ragged]
            _, _, _, dE0, ds0, _, _ = _pool_case(H, bf16, lens)
            _check_pool(got, pre, ref, dE0, ds0, bf16, 1)
    return run, check


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("lens", [DENSE, RAGGED], ids=["dense", "ragged"])
@pytest.mark.parametrize("H", [1, 4])
def test_pool_img(dev, mode, H, lens):
    """mdl_abmil_pool_fwd_img / mdl_abmil_pool_dscores_img on the split image of E at a wide e_rsb; d_scores written and accumulated."""
    run, check = _pool_img_runner(dev, H, lens)
    _strided_vs_contiguous(dev, mode, run, check)


def _pool_img_runner(dev, H, lens):
    """(run, check) of test_pool_img."""
    from madeleine_amd import functional as MF
    E, s, dp, _, ds0, cu, res = _pool_case(H, False, lens)
    T, n, C = sum(lens), len(lens), H * 512
    dense = lens == DENSE
    geom = (n, lens[0] if dense else 0, None if dense else cu.to(dev), max(lens), H)

    def run(lay):
        Ei, esc = _image(lay, E.to(dev), 0)
        sd, dpd = s.to(dev), dp.to(dev)
        pooled, m, l_ = _nan(dev, n, C), _nan(dev, n, H), _nan(dev, n, H)
        MF._call("mdl_abmil_pool_fwd_img", Ei, Ei.stride(0) * 4, esc, sd, pooled, m, l_, *geom, _ws(dev, "mdl_abmil_pool_ws_bytes", n, max(lens), H),
                 _stream())
        out = dict(pooled=pooled)
        for acc in (0, 1):
            dsc = ds0.to(dev).clone() if acc else _nan(dev, T, H)
            MF._call("mdl_abmil_pool_dscores_img", Ei, Ei.stride(0) * 4, esc, sd, pooled, m, l_, dpd, dsc, acc, *geom, _stream())
            out["ds%d" % acc] = dsc
        return out

    def check(got):
        pooled, _, dsc = res[False]
        assert rel_err(got["pooled"], pooled) < 1e-5 and max_rel(got["pooled"], pooled) < TOL
        for acc in (0, 1):
            diff = got["ds%d" % acc].double() - (ds0.double() if acc else 0.0)
            assert float((diff - dsc).abs().max()) <= 1e-4 * float(dsc.abs().max()) + 1e-6, acc
    return run, check


# ============================================================================================================================ Linears
@functools.lru_cache(maxsize=None)
def _lin_case(T, N, K, bf16):
    x, W, b, dy = _linear_case(T, N, K, 9000 + T + N + K, bf16=bf16)
    y64 = _mm(x, W.t()) + b.double()
    return x, W, b, dy, y64, _mm(dy, W), _tn(dy, x), dy.double().sum(0)


def _run_linear(dev, lay, case, dtype, T, N, K, forward=True, backward=True):
    """mdl_linear_fwd(_bf16) with ldx, ldy and mdl_linear_bwd(_bf16) with ldx, ldy / lddy, lddx (three different pads), with dX and
    dbias and without either."""
    from madeleine_amd import functional as MF
    x, W, b, dy = case[:4]
    sfx = "_bf16" if dtype == BF else ""
    Wd, bd = W.to(dev), b.to(dev)
    out = {}
    if forward:
        X, Y = lay.inp(x.to(dtype), 0), lay.out(T, N, dtype, 1)
        MF._call("mdl_linear_fwd" + sfx, X, X.stride(0), Wd, bd, Y, Y.stride(0), T, N, K, _ws(dev, "mdl_linear_fwd%s_ws_bytes" % sfx, T, N, K),
                 _stream())
        out["Y"] = Y
    for full in ((True, False) if backward else ()):
        X, dY = lay.inp(x.to(dtype), 0), lay.inp(dy.to(dtype), 1)
        dX = lay.out(T, K, dtype, 2) if full else None
        dW, db = _nan(dev, N, K), (_nan(dev, N) if full else None)
        MF._call("mdl_linear_bwd" + sfx, X, X.stride(0), Wd, dY, dY.stride(0), dX, dX.stride(0) if full else K, dW, db, T, N, K,
                 _ws(dev, "mdl_linear_bwd%s_ws_bytes" % sfx, T, N, K), _stream())
        if full:
            assert len({X.stride(0) - K, dY.stride(0) - N, dX.stride(0) - K}) == (3 if lay.mode != "contig" else 1)
            out.update(dX=dX, dW=dW, db=db.view(1, -1))
        else:
            out["dW_only"] = dW
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("T,N,K,want", [
    pytest.param(19, 12, 20, dict(variant=0, splits=1), id="small_T"),
    pytest.param(300, 256, 96, dict(variant=1, splits=1), id="wide_ragged_column_dX"),      # K % 256 != 0: the dX tile masks its columns
    pytest.param(300, 128, 256, dict(variant=2, splits=1), id="tall_swapped_dW"),
    pytest.param(4097, 256, 512, dict(variant=1, splits=2), id="wide_S2"),
])
def test_linear_fp32(dev, mode, T, N, K, want):
    _expect_plan("linear_fp32_bwd", T, N, K, want)
    case = _lin_case(T, N, K, False)
    _strided_vs_contiguous(dev, mode, lambda lay: _run_linear(dev, lay, case, F32, T, N, K), lambda got: _check_linear_f32(case, got))


def _check_linear_f32(case, got, forward=True, backward=True):
    x, W, b, dy, y64, dx64, dw64, db64 = case
    if forward:
        _chain_check(got["Y"], y64, _mm(x.abs(), W.abs().t()) + b.double().abs(), 1e-6, "Y")
    if backward:
        _chain_check(got["dX"], dx64, _mm(dy.abs(), W.abs()), 1e-6, "dX")
        for k in ("dW", "dW_only"):
            _chain_check(got[k], dw64, _tn(dy.abs(), x.abs()), 1e-6, k)
        _chain_check(got["db"].view(-1), db64, dy.double().abs().sum(0), 1e-6, "dbias")


def _check_linear_b16(case, got, forward=True, backward=True):
    y64, dx64, dw64, db64 = case[4:]
    if forward:
        assert float((got["Y"].double() - y64).abs().max()) <= EPS_BF16 * float(y64.abs().max())
        assert rel_err(got["Y"], y64) < EPS_BF16
    if backward:
        assert rel_err(got["dX"], dx64) < EPS_BF16
        assert rel_err(got["dW"], dw64) < 1e-5 and rel_err(got["dW_only"], dw64) < 1e-5
        assert rel_err(got["db"].view(-1), db64) < 1e-5


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("T,N,K,fwd,want_fwd,want_bwd", [
    pytest.param(300, 256, 512, True, dict(variant=4), dict(extra=4, variant=128), id="nt128_tn128"),
    pytest.param(4097, 1024, 512, True, dict(variant=256, persist=4), dict(extra=256, variant=128), id="nt256_persistent_dx256"),
    pytest.param(4097, 384, 256, True, dict(variant=2), dict(extra=4, variant=128), id="nt128_col_tile_N384"),
    pytest.param(16385, 256, 512, False, dict(variant=4), dict(variant=256), id="tn256_bwd_only"),
])
def test_linear_bf16(dev, mode, T, N, K, fwd, want_fwd, want_bwd):
    _expect_plan("linear_bf16_fwd", T, N, K, want_fwd)
    _expect_plan("linear_bf16_bwd", T, N, K, want_bwd)
    case = _lin_case(T, N, K, True)
    _strided_vs_contiguous(dev, mode, lambda lay: _run_linear(dev, lay, case, BF, T, N, K, forward=fwd), lambda got: _check_linear_b16(case, got, fwd))


# ======================================================================================================================= split images
def _decode(img, K):
    """fp64 values (times the scale) of a split image [rows, K] given as fp32-sized granules: per 32-column block the fp16 hi plane
    followed by the lo plane."""
    rows = img.shape[0]
    h = img.contiguous().view(torch.float16).view(rows, K // 32, 2, 32).double()
    return (h[:, :, 0] + h[:, :, 1]).reshape(rows, K)


def _check_image(data, scale, x, K):
    """hi = fp16(s x) and lo = fp16(s x - hi) with max |s x| in [2^13, 2^14): |hi + lo - s x| <= 2^-11 |s x - hi| + 2^-25 (the fp16
    subnormal step) <= 2^-22 |s x| + 2^-25."""
    sx = x.double() * scale.double()
    assert bool(((_decode(data, K) - sx).abs() <= 2.0 ** -22 * sx.abs() + 2.0 ** -25).all())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K", [64, 1024, 2048], ids=["K64_reg4", "K1024_reg2", "K2048_loop"])      # one K for each kernel of mdl_split_image_rows
def test_split_image(dev, mode, K):
    """mdl_split_image, mdl_split_image_rows (K <= 512 | K <= 1024 | above) and mdl_split_tile_absmax (with and without chunk_max) with a
    wide ldx and a wide rsb: image rows bit-equal to the contiguous build, nothing written past 4 K bytes of a row."""
    run, check = _split_image_runner(dev, K)
    _strided_vs_contiguous(dev, mode, run, check)


def _split_image_runner(dev, K):
    """(run, check) of test_split_image: X is stride argument 0, the image of mdl_split_image 1, that of mdl_split_image_rows 2."""
    from madeleine_amd import functional as MF
    rows, pad = 300, 32
    x = _u((rows, K), 9500 + K)
    x[7] = 0.0                                     # an all-zero row: no row scale, row_inv = 0
    x[40:80] *= 2.0 ** -12

    def run(lay):
        X = lay.inp(x, 0)
        b1, v1 = lay.buf(rows + pad, K, F32, 1)
        lay.track((b1, v1))
        sc1 = _nan(dev, 2)
        MF._call("mdl_split_image", X, X.stride(0), rows, K, v1, v1.stride(0) * 4, pad, sc1, _stream())
        b2, v2 = lay.buf(rows + pad, K, F32, 2)
        lay.track((b2, v2))
        rinv, sc2 = _nan(dev, rows), _nan(dev, 2)
        MF._call("mdl_split_image_rows", X, X.stride(0), rows, K, v2, v2.stride(0) * 4, pad, rinv, sc2, _stream())
        gate, cm, gate2 = _nan(dev, 2), _nan(dev, (rows + 31) // 32), _nan(dev, 2)
        MF._call("mdl_split_tile_absmax", X, X.stride(0), rows, K, gate, cm, _stream())
        MF._call("mdl_split_tile_absmax", X, X.stride(0), rows, K, gate2, None, _stream())
        return dict(img=v1, scale=sc1.view(1, -1), img_rows=v2, row_inv=rinv.view(1, -1), scale_rows=sc2.view(1, -1), gate=gate.view(1, -1),
                    chunk_max=cm.view(1, -1), gate_alone=gate2.view(1, -1))

    def check(got):
        ax = x.abs().double()
        assert float(got["scale"][0, 1]) == float(ax.max()) and float(got["scale_rows"][0, 1]) == float(ax.max())
        _check_image(got["img"][:rows], got["scale"][0, 0], x, K)
        assert not got["img"][rows:].any() and not got["img_rows"][rows:].any()                    # the zero pad rows
        rinv = got["row_inv"].view(-1).double()
        assert float(rinv[7]) == 0.0 and bool((rinv[torch.arange(rows) != 7] > 0).all())
        s_r = torch.where(rinv > 0, 1.0 / rinv, torch.zeros_like(rinv))
        srx = ax * s_r[:, None]
        assert bool(((srx.max(1).values >= 2.0 ** 13) & (srx.max(1).values < 2.0 ** 14))[torch.arange(rows) != 7].all())
        _check_image(got["img_rows"][:rows], s_r[:, None], x, K)
        want_gate = torch.stack([ax[i:i + 256].max() for i in range(0, rows, 256)])
        want_cm = torch.stack([ax[i:i + 32].max() for i in range(0, rows, 32)])
        assert torch.equal(got["gate"].view(-1).double(), want_gate) and torch.equal(got["gate_alone"].view(-1).double(), want_gate)
        assert torch.equal(got["chunk_max"].view(-1).double(), want_cm)
    return run, check


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("M,N,K", [pytest.param(300, 256, 96, id="tile256"), pytest.param(300, 128, 64, id="narrow_output_tile512x128")])
def test_split_gemm_nt(dev, mode, M, N, K):
    """mdl_split_gemm_nt on both of its kernels (N <= 128 with M > 256 takes the 512 x 128 tile) with wide a_rsb, b_rsb and ldc: with bias,
    with accumulate + row_gate (which keeps the 256 tile), with absmax_out; mdl_split_gemm_nt_group_bias."""
    run, check = _split_nt_runner(dev, M, N, K)
    _strided_vs_contiguous(dev, mode, run, check)


def _split_nt_runner(dev, M, N, K, only_plain=False):
    """(run, check) of test_split_gemm_nt: A is stride argument 0, B 1, C 2.  only_plain: the call with bias and absmax_out alone (the
    other two keep the 256 tile, whose stride limits differ from those of the narrow-output tile)."""
    from madeleine_amd import functional as MF
    a, bw = _u((M, K), 9600 + M + N), _u((N, K), 9700 + N, K ** -0.5)
    zhi = min(M, 512)
    a[256:zhi] = 0.0                                                                 # the second 256-row tile is all zero: its gate is 0
    bias, c0 = _u((N,), 9800, 0.1), _u((M, N), 9900)
    gb, rg = _u((3, N), 9950, 0.1), (torch.arange(M) % 3).to(torch.int32)
    p64, mag = _mm(a, bw.t()), _mm(a.abs(), bw.abs().t())

    def run(lay):
        A, asc = _image(lay, a.to(dev), 0)
        B, bsc = _image(lay, bw.to(dev), 1)
        geo = (A, A.stride(0) * 4, asc, B, B.stride(0) * 4, bsc)
        out = {}
        C1, amax = lay.out(M, N, F32, 2), torch.zeros(1, device=dev)
        MF._call("mdl_split_gemm_nt", *geo, C1, C1.stride(0), M, N, K, bias.to(dev), 0, amax, None, None, None, 3, _stream())
        assert len({A.stride(0) - K, B.stride(0) - K, C1.stride(0) - N}) == (3 if lay.mode != "contig" else 1)
        out.update(bias=C1, absmax=amax.view(1, 1))
        if only_plain:
            return out
        gate = _nan(dev, (M + 255) // 256)
        MF._call("mdl_split_tile_absmax", a.to(dev), K, M, K, gate, None, _stream())
        C2 = lay.out(M, N, F32, 2, init=c0)
        MF._call("mdl_split_gemm_nt", *geo, C2, C2.stride(0), M, N, K, None, 1, None, gate, None, None, 3, _stream())
        C3 = lay.out(M, N, F32, 2)
        MF._call("mdl_split_gemm_nt_group_bias", *geo, C3, C3.stride(0), M, N, K, bias.to(dev), None, None, gb.to(dev), rg.to(dev), 3, _stream())
        out.update(acc_gate=C2, group=C3)
        return out

    def check(got):
        want = p64 + bias.double()
        _chain_check(got["bias"], want, mag + bias.double().abs(), 4e-7, "bias")
        assert abs(float(got["absmax"]) - float(want.abs().max())) <= 1e-6 * float(want.abs().max())
        if only_plain:
            return
        _chain_check(got["acc_gate"], p64 + c0.double(), mag + c0.double().abs(), 4e-7, "accumulate + row_gate")
        assert torch.equal(got["acc_gate"][256:zhi], c0[256:zhi])                    # the gated tile is skipped: contents untouched
        wg = want + gb.double()[rg.long()]
        _chain_check(got["group"], wg, mag + bias.double().abs() + gb.double().abs()[rg.long()], 4e-7, "group_bias")
    return run, check


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("T,want", [pytest.param(33, dict(splits=1, tps=64), id="T33"), pytest.param(4097, dict(splits=2), id="T4097_S2")])
def test_split_gemm_tn(dev, mode, T, want):
    """mdl_split_gemm_tn (the dW product) with wide a_rsb and b_rsb; B carries its 32 zero pad rows inside the strided buffer."""
    _expect_plan("split_tn", T, 256, 128, want)
    run, check = _split_tn_runner(dev, T)
    _strided_vs_contiguous(dev, mode, run, check)


def _split_tn_runner(dev, T):
    """(run, check) of test_split_gemm_tn: A is stride argument 0, B 1."""
    from madeleine_amd import functional as MF
    Mi, N = 256, 128
    x, dy = _u((T, Mi), 9960 + T), _u((T, N), 9970 + T, 0.5)

    def run(lay):
        A, asc = _image(lay, x.to(dev), 0)
        B, bsc = _image(lay, dy.to(dev), 1, pad_rows=32)
        assert (A.stride(0) - Mi != B.stride(0) - N) or lay.mode == "contig"
        out = _nan(dev, N, Mi)
        MF._call("mdl_split_gemm_tn", A, A.stride(0) * 4, asc, Mi, B, B.stride(0) * 4, bsc, N, out, T, None,
                 _ws(dev, "mdl_split_gemm_tn_ws_bytes", T, Mi, N), 3, _stream())
        return dict(dW=out)
    return run, lambda got: _chain_check(got["dW"], _tn(dy, x), _tn(dy.abs(), x.abs()), 4e-7, "dW")
