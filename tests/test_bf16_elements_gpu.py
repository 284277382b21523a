"""The bf16 engine's products and sums, element by element, against fp64 (tests/_bf16_bounds.py states the contract, the references and
every bound; tests/test_bf16_bounds_cpu.py holds the checkers themselves to a CPU emulation and to seeded faults).

Each case hands the same bf16-representable operands to the kernel and to an fp64 reference of the documented operation (torch on the CPU,
or torch fp64 on the device for the threshold shapes), never to another kernel of this project.  An entry point that consumes an earlier
kernel's output (act_a / act_b, mean / rstd, pooled / stat_m / stat_l) is referenced on the values that kernel stored.  Three input kinds
per family -- uniform, row_scaled (token rows times 2^e, e in [-12, 12]: every row has to meet the bound at its own scale) and cancelling
(|result| << mag: the slack term) -- and, for the Linear and the weighted pooling, integer cases that must come out bit for bit.  Every
shape is the smallest that reaches its code path, asserted through mdl_dispatch_plan; strides are wider than the rows; the allocator's
cache is filled with NaN before every backward so that a workspace slab read unwritten shows.  No assertion here is a norm.

Entry points of the header's bf16 section and the tests that call them:
  mdl_linear_bf16_supported, mdl_linear_fwd_bf16, mdl_linear_bwd_bf16       test_linear_tails, test_linear_thresholds
  mdl_abmil_gate_fwd_bf16, mdl_abmil_gate_bwd_bf16                          test_gate_small, test_gate_paths
  mdl_abmil_attnpool_bwd_bf16, mdl_abmil_attnpool_bwd_phases_bf16           test_gate_fused_pooling_term
  mdl_abmil_pool_fwd_bf16, mdl_abmil_pool_bwd_bf16                          test_pool_bags
  mdl_abmil_wpool_fwd_bf16, mdl_abmil_wpool_bwd_bf16                        test_wpool_bags
  mdl_abmil_pool_view_fwd_bf16, mdl_abmil_pool_view_bwd_bf16                test_pool_views[view]
  mdl_abmil_pool_rview_fwd_bf16, mdl_abmil_pool_rview_bwd_bf16              test_pool_views[rview]
  mdl_ln_gelu_drop_fwd_bf16, mdl_ln_gelu_drop_bwd_bf16                      test_layernorm
  mdl_ln_gelu_drop_fwd_groups_bf16, mdl_ln_gelu_drop_bwd_groups_bf16        test_layernorm_groups

The exact Linear cases include K = 1056 (sigma of y 32.5): what they rest on, max |y| <= 256 on the reference, is asserted in every case."""
import numpy as np
import pytest
import torch

from tests import _bf16_bounds as B
from tests.test_dispatch_edges_gpu import _expect_plan, _poison

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NAN = float("nan")
HID = B.HID
EXACT_SEED = 9100
KINDS4 = B.KINDS + ("exact",)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nan(dev, *shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=dev)


def _wide(dev, rows, width, pad, x=None):
    """A bf16 [rows, width] view of a NaN buffer `pad` elements wider (row stride width + pad), holding x where given."""
    v = _nan(dev, rows, width + pad, dtype=BF)[:, :width]
    if x is not None:
        v.copy_(x.to(dev))
    return v


def _ws(dev, query, *sizes):
    """The workspace of the entry point's own query, carved from allocator cache that was just filled with NaN."""
    from madeleine_amd import _native
    n = getattr(_native.lib(), query)(*sizes)
    assert n >= 0, (query, sizes, n)
    _poison(dev, 2 * n + 4096)
    return torch.empty(n // 4 + 16, device=dev)


def _cpu(x):
    return x.detach().float().cpu()


# =============================================================================================================================== Linear
LINEAR_TAILS = ((1, 5, 127, 129, 257), ((128, 32), (384, 96), (256, 1056)))
LINEAR_THRESHOLDS = [
    (4095, 1024, 1024, dict(variant=4), dict(extra=4, variant=128, splits=1), "nt128_below_T4096"),
    (4096, 1024, 1024, dict(variant=256, persist=1), dict(extra=256, persist=1, variant=128, splits=1), "nt256_from_T4096"),
    (4096, 1024, 512, dict(variant=256, persist=4), dict(extra=256, persist=1), "nt256_persistent_4_col_tiles"),
    (16383, 256, 512, dict(variant=4), dict(variant=128, splits=4, empty=0), "tn128_S4_below_T16384"),
    (16384, 256, 512, dict(variant=4), dict(variant=256, splits=4, tps=4096, empty=0), "tn256_S4_from_T16384"),
    (16384, 384, 256, dict(variant=2), dict(variant=128, splits=4), "tn128_N_not_multiple_of_256"),
]


def _run_linear(dev, case):
    """mdl_linear_fwd_bf16 and mdl_linear_bwd_bf16 through the C ABI with four different row strides, each a multiple of 8."""
    from madeleine_amd import _native
    from madeleine_amd import functional as MF
    x, W, b, dy = case["x"], case["W"], case["b"], case["dy"]
    (T, K), N = x.shape, W.shape[0]
    assert _native.lib().mdl_linear_bf16_supported(N, K, 1) == 1
    X, dY, Y, dX = _wide(dev, T, K, 8, x), _wide(dev, T, N, 16, dy), _wide(dev, T, N, 24), _wide(dev, T, K, 32)
    Wd, bd = W.to(dev), b.to(dev)
    MF._call("mdl_linear_fwd_bf16", X, X.stride(0), Wd, bd, Y, Y.stride(0), T, N, K, _ws(dev, "mdl_linear_fwd_bf16_ws_bytes", T, N, K), _stream())
    dW, db = _nan(dev, N, K), _nan(dev, N)
    MF._call("mdl_linear_bwd_bf16", X, X.stride(0), Wd, dY, dY.stride(0), dX, dX.stride(0), dW, db, T, N, K,
             _ws(dev, "mdl_linear_bwd_bf16_ws_bytes", T, N, K), _stream())
    torch.cuda.synchronize()
    return {"Y": _cpu(Y), "dX": _cpu(dX), "dW": _cpu(dW), "db": _cpu(db)}


def _linear(dev, T, N, K, kind, ref_device):
    seed = EXACT_SEED + T + N + K
    case = B.linear_case(T, N, K, seed, kind)
    ref = B.linear_ref(case, ref_device)
    B.check_linear(_run_linear(dev, case), ref, kind, "linear[%dx%dx%d,%s]." % (T, N, K, kind))


@pytest.mark.parametrize("kind", KINDS4)
@pytest.mark.parametrize("N,K", LINEAR_TAILS[1])
@pytest.mark.parametrize("T", LINEAR_TAILS[0])
def test_linear_tails(dev, T, N, K, kind):
    """Row tails of the 128-row tiles (T = 1, 5, 127, 129, 257), the 128-column tile (N = 128, 384), one K chunk, three, and K % 64 != 0;
    the dW product with a partial last 32-token chunk."""
    _expect_plan("linear_bf16_fwd", T, N, K, dict(variant=4 if N % 256 == 0 else 2))
    _expect_plan("linear_bf16_bwd", T, N, K, dict(variant=128, splits=1, chunk=32))
    _linear(dev, T, N, K, kind, "cpu")


@pytest.mark.parametrize("kind", KINDS4)
@pytest.mark.parametrize("T,N,K,want_fwd,want_bwd", [pytest.param(*s[:5], id=s[5]) for s in LINEAR_THRESHOLDS])
def test_linear_thresholds(dev, T, N, K, want_fwd, want_bwd, kind):
    """Both sides of the 256-tile predicates of the NT (forward, dX) and TN (dW) products, persistence over 4 column tiles, four token
    splits with their slab reduction."""
    _expect_plan("linear_bf16_fwd", T, N, K, want_fwd)
    _expect_plan("linear_bf16_bwd", T, N, K, want_bwd)
    _linear(dev, T, N, K, kind, dev)


# ================================================================================================================================= gate
def _gate_masks(dev, T, H, p, seed):
    """The keep masks the kernels derive from (seed, p), exported by mdl_abmil_gate_dropout_mask."""
    from madeleine_amd import functional as MF
    if p == 0:
        return None, None
    out = []
    for which in (0, 1):
        m = torch.empty(T, H, HID, dtype=torch.uint8, device=dev)
        MF._call("mdl_abmil_gate_dropout_mask", m, T, H, which, float(p), seed, _stream())
        out.append(m.cpu())
    return tuple(out)


def _gate_fwd(dev, case, seed):
    """mdl_abmil_gate_fwd_bf16 on E at ldE = H*512 + 8: (E view, device parameters, scores, act_a, act_b)."""
    from madeleine_amd import functional as MF
    T, H, p = case["T"], case["H"], case["p"]
    Ev = _wide(dev, T, H * HID, 8, case["E"])
    ps = {k: case[k].to(dev) for k in ("Wa", "ba", "Wb", "bb", "wc", "bc")}
    sc, a, b = _nan(dev, T, H), _nan(dev, T, H, HID, dtype=BF), _nan(dev, T, H, HID, dtype=BF)
    MF._call("mdl_abmil_gate_fwd_bf16", Ev, Ev.stride(0), ps["Wa"], ps["ba"], ps["Wb"], ps["bb"], ps["wc"], ps["bc"], sc, a, b, T, H, float(p),
             seed, None, None, _ws(dev, "mdl_abmil_gate_fwd_bf16_ws_bytes", T, H), _stream())
    return Ev, ps, sc, a, b


def _gate_bwd(dev, case, Ev, ps, a, b, seed, acc, entry="mdl_abmil_gate_bwd_bf16", pool=(), phases=(None,)):
    """One backward entry point -> the gradients as CPU fp32 tensors."""
    from madeleine_amd import functional as MF
    T, H, p = case["T"], case["H"], case["p"]
    dE = _wide(dev, T, H * HID, 8, case["dE0"] if acc else None)
    assert dE.stride(0) == Ev.stride(0)
    grads = [_nan(dev, H, HID, HID), _nan(dev, H, HID, HID), _nan(dev, H, HID), _nan(dev, H, HID), _nan(dev, H, HID), _nan(dev, H)]
    ws = _ws(dev, "mdl_abmil_gate_bwd_bf16_ws_bytes", T, H)
    args = [Ev, Ev.stride(0), ps["Wa"], ps["Wb"], ps["wc"], a, b, case["ds"].to(dev), dE, acc] + grads + [T, H, float(p), seed, None, None]
    args += list(pool) + [ws, _stream()]
    for ph in phases:
        MF._call(entry, *(args + ([] if ph is None else [ph])))
    torch.cuda.synchronize()
    return dict(zip(("dE", "dWa", "dWb", "dba", "dbb", "dwc", "dbc"), [_cpu(dE)] + [_cpu(g) for g in grads]))


def _check_gate_fwd(case, sc, a, b, ka, kb, what, ref_device):
    a, b = _cpu(a), _cpu(b)
    fwd = B.gate_fwd_ref(case, ref_device)
    B.check(what + "act_a", a, *fwd["act_a"])
    B.check(what + "act_b", b, *fwd["act_b"])
    B.check(what + "scores", _cpu(sc), *B.gate_scores_ref(case, a, b, ka, kb))
    return a, b


def _check_gate_bwd(case, got, a, b, ka, kb, acc, what, ref_device, pool=None):
    for k, v in B.gate_bwd_ref(case, a, b, ka, kb, acc, pool, ref_device).items():
        B.check(what + k, got[k].reshape(v[0].shape), *v)


def _gate(dev, T, H, p, kind, ref_device, backward=True):
    case = B.gate_case(T, H, 4000 + T + H, kind, p)
    seed = 777 + T
    ka, kb = _gate_masks(dev, T, H, p, seed)
    what = "gate[T%d,H%d,p%g,%s]." % (T, H, p, kind)
    Ev, ps, sc, a, b = _gate_fwd(dev, case, seed)
    a32, b32 = _check_gate_fwd(case, sc, a, b, ka, kb, what, ref_device)
    for acc in ((0, 1) if backward else ()):
        got = _gate_bwd(dev, case, Ev, ps, a, b, seed, acc)
        _check_gate_bwd(case, got, a32, b32, ka, kb, acc, what + "acc%d." % acc, ref_device)


@pytest.mark.parametrize("kind", B.KINDS)
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("H", [1, 4])
@pytest.mark.parametrize("T", [1, 5, 40, 129])
def test_gate_small(dev, T, H, p, kind):
    """The 128-row tiles of the forward, dX and dW kernels at one row, a few, a partial second 32-token chunk and a second row tile; the
    dropout RNG replayed in fp64 from the exported masks; dE written and accumulated."""
    _expect_plan("gate_bf16_fwd", T, H, 0, dict(variant=128))
    _expect_plan("gate_bf16_bwd", T, H, 0, dict(variant=128, extra=128, splits=1, chunk=32))
    _gate(dev, T, H, p, kind, "cpu")


@pytest.mark.parametrize("T,H,p,kind,backward,want_fwd,want_bwd", [
    pytest.param(4096, 1, 0.25, "row_scaled", True, dict(variant=256, persist=0), dict(variant=128, extra=256, splits=1),
                 id="fwd256_plain_dx256"),                 # the smallest T of the 256-row forward and dX tiles
    pytest.param(4097, 1, 0.0, "uniform", True, dict(variant=256, persist=0), dict(variant=128, extra=256, splits=2, tps=2080),
                 id="short_last_token_split"),             # S = 2, tps = 2080: the last split has 2017 tokens; a 1-row last 256 tile
    pytest.param(12289, 4, 0.0, "row_scaled", False, dict(variant=256, persist=1), dict(),
                 id="fwd256_persistent"),                  # the smallest (T, H) the plan runs persistent (no H = 1 shape is)
    pytest.param(16384, 1, 0.0, "cancelling", True, dict(variant=256), dict(variant=256, extra=256, splits=4, chunk=64),
                 id="dw256"),                              # the smallest T of the 256 x 256 dW tile
])
def test_gate_paths(dev, T, H, p, kind, backward, want_fwd, want_bwd):
    """The 256-row forward (plain and persistent), dX 256, dW 256 and a short last token split, each at the smallest shape the plan gives."""
    _expect_plan("gate_bf16_fwd", T, H, 0, want_fwd)
    _expect_plan("gate_bf16_bwd", T, H, 0, want_bwd)
    _gate(dev, T, H, p, kind, dev, backward)


@pytest.mark.parametrize("kind", B.KINDS)
@pytest.mark.parametrize("H", [1, 4])
def test_gate_fused_pooling_term(dev, H, kind):
    """mdl_abmil_attnpool_bwd_bf16 and mdl_abmil_attnpool_bwd_phases_bf16 (phases 1, then 2) on two ragged bags of 70 and 59 tokens: the bag
    boundary lies inside the first 128-row tile, the second tile holds one row."""
    lens, p = (70, 59), 0.25
    T = sum(lens)
    case = B.gate_case(T, H, 4500 + H, kind, p)
    seed = 99
    ka, kb = _gate_masks(dev, T, H, p, seed)
    Ev, ps, sc, a, b = _gate_fwd(dev, case, seed)
    what = "attnpool[H%d,%s]." % (H, kind)
    a32, b32 = _check_gate_fwd(case, sc, a, b, ka, kb, what, "cpu")
    # the pooling term's inputs are arguments of the call: the kernel's own scores, their softmax statistics formed here
    row_bag = torch.repeat_interleave(torch.arange(2), torch.tensor(lens)).to(torch.int32)
    s = _cpu(sc)
    m = torch.stack([s[row_bag == k].max(0).values for k in range(2)])
    l_ = torch.stack([(s[row_bag == k] - m[k]).double().exp().sum(0) for k in range(2)]).float()
    dp = B.token_operand((2, H * HID), 4600 + H, kind)
    term = B.gate_pool_term(s, m, l_, dp, row_bag, H)
    pool = [x.to(dev) for x in (s, m, l_, dp, row_bag)] + [0]
    for acc, entry, phases in ((0, "mdl_abmil_attnpool_bwd_bf16", (None,)), (1, "mdl_abmil_attnpool_bwd_bf16", (None,)),
                               (0, "mdl_abmil_attnpool_bwd_phases_bf16", (1, 2)), (1, "mdl_abmil_attnpool_bwd_phases_bf16", (3,))):
        got = _gate_bwd(dev, case, Ev, ps, a, b, seed, acc, entry, pool, phases)
        _check_gate_bwd(case, got, a32, b32, ka, kb, acc, "%s%s.acc%d." % (what, "phases" if "phases" in entry else "fused", acc), "cpu", term)


# ============================================================================================================================== pooling
RAGGED = (333, 0, 1, 63, 65)


def _pool_geom(dev, lens, dense, H):
    cu = torch.tensor(B.bag_rows(lens), dtype=torch.int64)
    return (len(lens), lens[0] if dense else 0, None if dense else cu.to(dev), max(lens), H)


def _pool_E(dev, case):
    """E at ldE = H*512 + 4: a multiple of 4, not of 8."""
    T, C = case["E"].shape
    Ev = _wide(dev, T, C, 4, case["E"])
    assert Ev.stride(0) % 8 == 4
    return Ev


def _run_pool(dev, case, lin, dense, accs):
    """The forward and, per (accumulate, accumulate_scores) of accs, the backward of the softmax (lin: weighted) pooling over whole bags."""
    from madeleine_amd import functional as MF
    lens, H = case["lens"], case["H"]
    T, C, n = sum(lens), H * HID, len(lens)
    geom = _pool_geom(dev, lens, dense, H)
    name = "wpool" if lin else "pool"
    Ev, sd, dpd = _pool_E(dev, case), case["s"].to(dev), case["dp"].to(dev)
    pooled, m, l_ = _nan(dev, n, C), _nan(dev, n, H), _nan(dev, n, H)
    MF._call("mdl_abmil_%s_fwd_bf16" % name, Ev, Ev.stride(0), sd, pooled, m, l_, *geom, _ws(dev, "mdl_abmil_pool_ws_bytes", n, max(lens), H),
             _stream())
    fwd = dict(pooled=_cpu(pooled), m=_cpu(m), l=_cpu(l_))
    outs = []
    for acc, acc_s in accs:
        dE = _wide(dev, T, C, 4, case["dE0"] if acc else None)
        dsc = case["ds0"].to(dev).clone() if acc_s else _nan(dev, T, H)
        _poison(dev, 1 << 20)
        if lin:
            MF._call("mdl_abmil_wpool_bwd_bf16", Ev, Ev.stride(0), sd, dpd, dE, acc, dsc, *geom, _stream())
        else:
            MF._call("mdl_abmil_pool_bwd_bf16", Ev, Ev.stride(0), sd, pooled, m, l_, dpd, dE, acc, dsc, acc_s, *geom, _stream())
        torch.cuda.synchronize()
        outs.append(dict(dE=_cpu(dE), ds=_cpu(dsc)))
    return fwd, outs


@pytest.mark.parametrize("kind", B.KINDS)
@pytest.mark.parametrize("lens,dense", [pytest.param((65, 65, 65), True, id="dense_65"), pytest.param((1, 1), True, id="dense_1"),
                                        pytest.param(RAGGED, False, id="ragged")])
@pytest.mark.parametrize("H", [1, 4])
def test_pool_bags(dev, H, lens, dense, kind):
    """mdl_abmil_pool_fwd_bf16 / _bwd_bf16 over dense and ragged bags (an empty bag, one token, 63, 65, and 333 tokens = three forward
    chunks with their merge), dE and d_scores written and accumulated."""
    case = B.pool_case(lens, H, 5000 + H + sum(lens), kind)
    accs = ((0, 0), (1, 1), (1, 0), (0, 1))
    fwd, outs = _run_pool(dev, case, False, dense, accs)
    what = "pool[H%d,%s]." % (H, kind)
    B.check_pool_fwd(fwd, case, False, what)
    for (acc, acc_s), got in zip(accs, outs):
        B.check_pool_bwd(got, case, False, fwd, acc, acc_s, "%sacc%d%d." % (what, acc, acc_s))


@pytest.mark.parametrize("kind", KINDS4)
@pytest.mark.parametrize("lens,dense", [pytest.param((65, 65, 65), True, id="dense_65"), pytest.param(RAGGED, False, id="ragged")])
@pytest.mark.parametrize("H", [1, 4])
def test_wpool_bags(dev, H, lens, dense, kind):
    """mdl_abmil_wpool_fwd_bf16 / _bwd_bf16: the weighted pooling has exact products, and on the integer case comes out bit for bit."""
    case = B.pool_case(lens, H, 5100 + H + sum(lens), kind)
    accs = ((0, 0), (1, 0))
    fwd, outs = _run_pool(dev, case, True, dense, accs)
    what = "wpool[H%d,%s]." % (H, kind)
    B.check_pool_fwd(fwd, case, True, what)
    for (acc, acc_s), got in zip(accs, outs):
        B.check_pool_bwd(got, case, True, fwd, acc, acc_s, "%sacc%d." % (what, acc))


@pytest.mark.parametrize("kind", B.KINDS)
@pytest.mark.parametrize("which", ["view", "rview"])
@pytest.mark.parametrize("H", [1, 4])
def test_pool_views(dev, H, which, kind):
    """mdl_abmil_pool_view_* on a 33-index view of three dense bags of 65 tokens; mdl_abmil_pool_rview_* on both half-bag views of ragged
    bags of 333, 1 (its first view is empty), 63 and 65 tokens.  The backwards accumulate into dE and d_scores; with d_scores NULL the
    dE-only pass; a row outside every view keeps its contents to the bit."""
    from madeleine_amd import functional as MF
    from madeleine_amd.model import ragged_view_plan
    C = H * HID
    if which == "view":
        lens = (65, 65, 65)
        idx = torch.randperm(65, generator=torch.Generator().manual_seed(3))[:33].to(torch.int32)
        segments = [k * 65 + idx.long() for k in range(3)]
    else:
        lens = (333, 1, 63, 65)
        np.random.seed(17)
        perm, vcu, max_view = ragged_view_plan(lens)
        segments = [perm[int(vcu[k]):int(vcu[k + 1])].long() for k in range(2 * len(lens))]
    case = B.pool_case(lens, H, 5200 + H, kind, segments)
    T, n, S = sum(lens), len(lens), len(segments)
    Ev, sd, dpd = _pool_E(dev, case), case["s"].to(dev), case["dp"].to(dev)
    pooled, m, l_ = _nan(dev, S, C), _nan(dev, S, H), _nan(dev, S, H)
    if which == "view":
        geom = (n, 65, idx.to(dev), idx.numel(), H)
        ws = _ws(dev, "mdl_abmil_pool_ws_bytes", n, idx.numel(), H)
    else:
        geom = (n, perm.to(dev), vcu.to(dev), max_view, H)
        ws = _ws(dev, "mdl_abmil_pool_ws_bytes", S, max_view, H)
    MF._call("mdl_abmil_pool_%s_fwd_bf16" % which, Ev, Ev.stride(0), sd, pooled, m, l_, *geom, ws, _stream())
    fwd = dict(pooled=_cpu(pooled), m=_cpu(m), l=_cpu(l_))
    what = "%s[H%d,%s]." % (which, H, kind)
    B.check_pool_fwd(fwd, case, False, what)
    for with_scores in (True, False):
        dE, dsc = _wide(dev, T, C, 4, case["dE0"]), case["ds0"].to(dev).clone()
        _poison(dev, 1 << 20)
        MF._call("mdl_abmil_pool_%s_bwd_bf16" % which, Ev, Ev.stride(0), sd, pooled, m, l_, dpd, dE, dsc if with_scores else None, *geom, _stream())
        torch.cuda.synchronize()
        got = dict(dE=_cpu(dE), ds=_cpu(dsc))
        if with_scores:
            B.check_pool_bwd(got, case, False, fwd, 1, 1, what + "both.")
        else:
            assert torch.equal(got["ds"], case["ds0"])
            ref = B.pool_bwd_ref(case, False, fwd["pooled"], fwd["m"], fwd["l"], 1, 0)
            B.check_pool_bwd(dict(got, ds=ref["ds"]), case, False, fwd, 1, 0, what + "dE_only.")


# =============================================================================================================== LayerNorm-GELU-Dropout
def _run_ln(dev, case):
    """The forward (mean, rstd, y) and the backward of the plain or the grouped bf16 entry points, with an explicit keep mask at p > 0."""
    from madeleine_amd import functional as MF
    rows, W = case["x"].shape
    grouped = case["groups"] is not None
    x, dy = case["x"].to(dev).to(BF), case["dy"].to(dev).to(BF)
    gam, beta, bias = case["gamma"].to(dev), case["beta"].to(dev), case["bias"].to(dev).contiguous()
    keep = case["keep"].to(dev) if case["keep"] is not None else None
    groups = (torch.tensor(B.bag_rows(case["groups"]), dtype=torch.int64, device=dev), len(case["groups"])) if grouped else ()
    sfx = "_groups_bf16" if grouped else "_bf16"
    y, mean, rstd = _nan(dev, rows, W, dtype=BF), _nan(dev, rows), _nan(dev, rows)
    MF._call("mdl_ln_gelu_drop_fwd" + sfx, x, bias, gam, beta, y, mean, rstd, rows, W, case["eps"], float(case["p"]), 5, keep, *groups, _stream())
    dx, dg, db, dbias = _nan(dev, rows, W, dtype=BF), _nan(dev, W), _nan(dev, W), _nan(dev, *bias.shape)
    ws = _ws(dev, "mdl_ln_gelu_drop_bwd%s_ws_bytes" % ("_groups" if grouped else ""), rows, W, *groups[1:])
    MF._call("mdl_ln_gelu_drop_bwd" + sfx, x, bias, gam, beta, mean, rstd, dy, dx, dg, db, dbias, rows, W, float(case["p"]), 5, keep, *groups, ws,
             _stream())
    torch.cuda.synchronize()
    fwd = dict(y=_cpu(y), mean=_cpu(mean), rstd=_cpu(rstd))
    return fwd, {"dx": _cpu(dx), "dgamma": _cpu(dg), "dbeta": _cpu(db), "dgroup_bias" if grouped else "dbias": _cpu(dbias)}


def _layernorm(dev, rows, W, p, kind, groups):
    case = B.ln_case(rows, W, 6000 + rows + W, kind, p, groups)
    fwd, bwd = _run_ln(dev, case)
    what = "ln[%dx%d,p%g,%s,%s]." % (rows, W, p, kind, "plain" if groups is None else "G%d" % len(groups))
    ref = B.ln_fwd_ref(case, fwd["mean"], fwd["rstd"])
    for k in ("mean", "rstd", "y"):
        B.check(what + k, fwd[k], *ref[k])
    for k, v in B.ln_bwd_ref(case, fwd["mean"], fwd["rstd"]).items():
        B.check(what + k, bwd[k], *v)
    if groups is not None:
        for g, n in enumerate(groups):
            if n == 0:
                assert float(bwd["dgroup_bias"][g].abs().max()) == 0.0, "the empty group"


@pytest.mark.parametrize("kind", B.KINDS)
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("rows", [1, 77, 300])
@pytest.mark.parametrize("W", [256, 512, 2048])
def test_layernorm(dev, W, rows, p, kind):
    """mdl_ln_gelu_drop_fwd_bf16 / _bwd_bf16: the row statistics against fp64, y, dx and the three column reductions from the stored
    statistics; fewer rows than a block iteration, a ragged last one, several blocks."""
    _layernorm(dev, rows, W, p, kind, None)


@pytest.mark.parametrize("kind", B.KINDS)
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("rows", [1, 77, 300])
@pytest.mark.parametrize("W", [256, 512])
def test_layernorm_groups(dev, W, rows, G, p, kind):
    """The grouped entry points at the widths they take beside 1024: one group, and three with an empty one in the middle."""
    groups = [rows] if G == 1 else [rows - rows // 3, 0, rows // 3]
    _layernorm(dev, rows, W, p, kind, groups)
