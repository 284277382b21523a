"""The InfoNCE kernels, element by element, against fp64 (tests/_nce_bounds.py states the contract, the references and every bound;
tests/test_nce_bounds_cpu.py holds the checkers themselves to a CPU emulation and to twelve seeded faults).

Every case goes through the C ABI (mdl_infonce_fwd / _bwd, mdl_infonce_neg_fwd / _bwd) with NaN in the padding rows of Q and P, NaN in
the padding of d_row_loss, NaN-filled outputs and a NaN-filled workspace, and every element of loss, row_loss, dQ, dP and dNeg is held to
its own bound (a zero bound -- padding rows, a problem of one row, M = 0, the padding columns of the explicit-negative dQ / dP -- means
exact; a NaN anywhere fails).  Nothing here reads the workspace.  No assertion is a norm.

In-batch (staged, and fused through MADELEINE_INFONCE_FUSED=1 where Kmax <= 256 and D <= 512): S = 3 problems of cnt = (Kmax, about
Kmax / 2 and no multiple of 32, 1), and one problem with cnt = 0.  The cross product of the issue is pruned to one case per edge:
  - every Kmax of {1, 31, 32, 33, 64, 65, 256, 257} at D = 64, T = 0.07 (the padding to Kp, the 64-lane strides, one and several blocks),
    families, symmetric and the gradient form rotating;
  - every D of {32, 96, 512, 544} at Kmax = 33, T = 1 (D = 64 is the row above), one of them not symmetric;
  - T = 0.001 at D = 512: clustered (the family whose softmax is not saturated there) at Kmax = 33, 65, 256, 257 and at D = 544, both
    gradient forms and both symmetric values among them; uniform (saturated), degenerate and row_scaled once each.
Explicit negatives: every M of {0, 1, 63, 64, 65, 1024, 1025, 4096, 4097} at D = 100 for unpaired N = 33 and paired N = 5 (both sides of
every merge size), unpaired N = 1, 31, 32 and paired N = 1 at M = 65, D = 101, every D of {1, 3, 101, 128} at M = 65, a bank shifted by
4 bytes at D = 128 (4-byte loads with D % 4 == 0), dNeg NULL once per mode; families, T and the gradient form rotate."""
import pytest
import torch

from tests import _nce_bounds as B
from tests._switches import switch  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu
NAN = float("nan")

# (Kmax, D, T, symmetric, family, form)
INBATCH = [
    (1, 64, 0.07, 1, "uniform", "d_row_loss"),
    (31, 64, 0.07, 1, "row_scaled", "d_row_loss"),
    (32, 64, 0.07, 0, "uniform", "d_loss"),
    (33, 64, 0.07, 1, "degenerate", "d_row_loss"),
    (64, 64, 0.07, 1, "row_scaled", "d_loss"),
    (65, 64, 0.07, 1, "uniform", "d_row_loss"),
    (256, 64, 0.07, 1, "row_scaled", "d_row_loss"),
    (257, 64, 0.07, 1, "degenerate", "d_row_loss"),
    (33, 32, 1.0, 1, "uniform", "d_row_loss"),
    (33, 96, 1.0, 1, "row_scaled", "d_row_loss"),
    (33, 96, 1.0, 0, "degenerate", "d_loss"),
    (33, 512, 1.0, 1, "degenerate", "d_row_loss"),
    (33, 544, 1.0, 1, "row_scaled", "d_row_loss"),
    (33, 512, 0.001, 1, "clustered", "d_row_loss"),
    (65, 512, 0.001, 0, "clustered", "d_loss"),
    (256, 512, 0.001, 1, "clustered", "d_loss"),
    (257, 512, 0.001, 1, "clustered", "d_row_loss"),
    (33, 544, 0.001, 0, "clustered", "d_row_loss"),
    (33, 512, 0.001, 1, "uniform", "d_loss"),
    (33, 512, 0.001, 1, "degenerate", "d_row_loss"),
    (65, 512, 0.001, 1, "row_scaled", "d_row_loss"),
]
# (N, M, D, T, paired, family, form, dNeg requested, Neg shifted by 4 bytes)
NEG = [
    (33, 0, 100, 0.07, 0, "uniform", "d_loss", 1, 0),
    (33, 1, 100, 0.07, 0, "row_scaled", "d_row_loss", 1, 0),
    (33, 63, 100, 1.0, 0, "degenerate", "d_row_loss", 1, 0),
    (33, 64, 100, 0.07, 0, "uniform", "d_loss", 1, 0),
    (33, 65, 100, 0.001, 0, "clustered", "d_row_loss", 1, 0),
    (33, 1024, 100, 0.07, 0, "row_scaled", "d_row_loss", 1, 0),
    (33, 1025, 100, 0.001, 0, "clustered", "d_loss", 1, 0),
    (33, 1025, 100, 0.07, 0, "row_scaled", "d_row_loss", 0, 0),
    (33, 4096, 100, 0.07, 0, "uniform", "d_row_loss", 1, 0),
    (33, 4097, 100, 0.001, 0, "clustered", "d_row_loss", 1, 0),
    (33, 4097, 100, 0.07, 0, "uniform", "d_loss", 1, 0),
    (5, 0, 100, 0.07, 1, "uniform", "d_row_loss", 1, 0),
    (5, 1, 100, 0.07, 1, "row_scaled", "d_loss", 1, 0),
    (5, 63, 100, 1.0, 1, "degenerate", "d_row_loss", 1, 0),
    (5, 64, 100, 0.07, 1, "row_scaled", "d_row_loss", 1, 0),
    (5, 65, 100, 0.001, 1, "clustered", "d_loss", 1, 0),
    (5, 1024, 100, 0.07, 1, "uniform", "d_row_loss", 1, 0),
    (5, 1025, 100, 0.001, 1, "clustered", "d_row_loss", 1, 0),
    (5, 4096, 100, 0.07, 1, "row_scaled", "d_loss", 1, 0),
    (5, 4097, 100, 0.001, 1, "clustered", "d_row_loss", 1, 0),
    (1, 65, 101, 0.07, 0, "uniform", "d_loss", 1, 0),
    (31, 65, 101, 0.07, 0, "degenerate", "d_row_loss", 1, 0),
    (32, 65, 101, 0.07, 0, "row_scaled", "d_row_loss", 1, 0),
    (33, 65, 101, 0.001, 0, "clustered", "d_loss", 1, 0),
    (1, 65, 101, 0.07, 1, "row_scaled", "d_row_loss", 1, 0),
    (5, 65, 101, 0.07, 1, "degenerate", "d_row_loss", 1, 0),
    (5, 65, 101, 0.07, 1, "uniform", "d_loss", 0, 0),
    (33, 65, 1, 0.07, 0, "uniform", "d_row_loss", 1, 0),
    (33, 65, 3, 0.07, 0, "row_scaled", "d_row_loss", 1, 0),
    (33, 65, 128, 0.07, 0, "degenerate", "d_loss", 1, 0),
    (5, 65, 1, 0.07, 1, "row_scaled", "d_row_loss", 1, 0),
    (5, 65, 3, 0.07, 1, "uniform", "d_loss", 1, 0),
    (5, 65, 128, 0.001, 1, "clustered", "d_row_loss", 1, 0),
    (33, 65, 128, 0.07, 0, "row_scaled", "d_row_loss", 1, 1),
    (5, 65, 128, 0.07, 1, "row_scaled", "d_row_loss", 1, 1),
]


def inbatch_cases():
    """Every in-batch case of this file, as tests/_nce_bounds.py builds it (also the case list of tests/test_nce_bounds_cpu.py)."""
    for Kmax, D, T, sym, family, form in INBATCH:
        yield B.inbatch_case((Kmax, B.mid_count(Kmax), 1), Kmax, D, T, sym, family, form)
    yield B.inbatch_case((0,), 33, 64, 0.07, 1, "uniform", "d_loss", "empty")


def neg_cases():
    for N, M, D, T, paired, family, form, _dneg, _shift in NEG:
        yield B.neg_case(N, M, D, T, paired, family, form)


def _id(spec):
    return "-".join(str(x) for x in spec)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _nan(dev, *shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=dev)


def _ws(dev, query, *sizes):
    """The workspace of the entry point's own query, every float a NaN."""
    from madeleine_amd import _native
    n = getattr(_native.lib(), query)(*sizes)
    assert n >= 0, (query, sizes, n)
    return _nan(dev, n // 4 + 16)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _run_inbatch(dev, case):
    from madeleine_amd import functional as MF
    S, Kmax, D, T, sym = len(case["cnt"]), case["Kmax"], case["D"], case["T"], case["sym"]
    Q, P, g = case["Q"].to(dev), case["P"].to(dev), case["g"].to(dev)
    cnt = torch.tensor(case["cnt"], dtype=torch.int32, device=dev)
    loss, rows, dQ, dP = _nan(dev, S), _nan(dev, S, Kmax), _nan(dev, S, Kmax, D), _nan(dev, S, Kmax, D)
    ws = _ws(dev, "mdl_infonce_ws_bytes", S, Kmax, D)
    MF._call("mdl_infonce_fwd", Q, P, cnt, loss, rows, S, Kmax, D, float(T), sym, ws, _stream())
    d_loss, d_row = (g, None) if case["form"] == "d_loss" else (None, g)
    MF._call("mdl_infonce_bwd", Q, P, d_loss, d_row, cnt, dQ, dP, S, Kmax, D, float(T), sym, ws, _stream())
    torch.cuda.synchronize()
    return {"loss": loss.cpu(), "row_loss": rows.cpu(), "dQ": dQ.cpu(), "dP": dP.cpu()}


def _exact_zero(what, x):
    assert bool((x == 0).all()), (what, x.flatten()[:8].tolist())


def _check_inbatch(got, case, what):
    B.check_inbatch(got, case, what)
    for s, k in enumerate(case["cnt"]):
        for n in ("row_loss", "dQ", "dP"):                      # rows >= cnt: exactly 0 despite the NaN padding
            _exact_zero("%s%s[%d, %d:]" % (what, n, s, k), got[n][s, k:])
        if k <= 1:                                              # no row or one row: loss and gradients exactly 0
            for n in ("loss", "row_loss", "dQ", "dP"):
                _exact_zero("%s%s[%d]" % (what, n, s), got[n][s])
    for n in ("loss", "row_loss", "dQ", "dP"):
        assert not bool(torch.isnan(got[n]).any()), what + n


def _fusable(spec):
    return spec[0] <= 256 and spec[1] <= 512


@pytest.mark.parametrize("spec", INBATCH, ids=_id)
def test_inbatch_staged(dev, spec, switch):
    switch("MADELEINE_INFONCE_FUSED", 0)
    Kmax, D, T, sym, family, form = spec
    case = B.inbatch_case((Kmax, B.mid_count(Kmax), 1), Kmax, D, T, sym, family, form)
    _check_inbatch(_run_inbatch(dev, case), case, "staged[%s]." % _id(spec))


@pytest.mark.parametrize("spec", [s for s in INBATCH if _fusable(s)], ids=_id)
def test_inbatch_fused(dev, spec, switch):
    """The opt-in one-launch kernels against fp64, independently of what the staged kernels give."""
    switch("MADELEINE_INFONCE_FUSED", 1)
    Kmax, D, T, sym, family, form = spec
    case = B.inbatch_case((Kmax, B.mid_count(Kmax), 1), Kmax, D, T, sym, family, form)
    _check_inbatch(_run_inbatch(dev, case), case, "fused[%s]." % _id(spec))


@pytest.mark.parametrize("fused", [0, 1], ids=["staged", "fused"])
def test_inbatch_single_empty_stain(dev, fused, switch):
    """One problem with cnt = 0: loss 0, every row of row_loss, dQ and dP exactly 0."""
    if fused:
        switch("MADELEINE_INFONCE_FUSED", 1)
    else:
        switch("MADELEINE_INFONCE_FUSED", 0)
    case = B.inbatch_case((0,), 33, 64, 0.07, 1, "uniform", "d_loss", "empty")
    _check_inbatch(_run_inbatch(dev, case), case, "empty[%s]." % ("fused" if fused else "staged"))


@pytest.mark.parametrize("fused", [0, 1], ids=["staged", "fused"])
def test_inbatch_clamped_rows_are_rn_times_dxhat(dev, fused, switch):
    """On a clamped row (|x| < 1e-12) dX = rn dX^ within its bound: the dot of normalize()'s backward is dropped."""
    if fused:
        switch("MADELEINE_INFONCE_FUSED", 1)
    else:
        switch("MADELEINE_INFONCE_FUSED", 0)
    case = B.inbatch_case((33,), 33, 64, 0.07, 1, "degenerate", "d_row_loss", "clamped")
    got = _run_inbatch(dev, case)
    r = B._stain_ref(case["Q"][0], case["P"][0], B.t32(case["T"]), 1, case["g"][0], False, 64, False)
    for n, which in (("dQ", 0), ("dP", 1)):
        rows = r["clamped"][which]
        assert int(rows.sum()) == 2                                   # the all-zero row and the row of norm 1e-13
        B.check("clamped.%s" % n, got[n][0][rows], r["clamped_ref"][which][rows], r[n][1][rows])


def _run_neg(dev, case, dneg, shift):
    from madeleine_amd import functional as MF
    N, M, D, T, paired = case["N"], case["M"], case["D"], case["T"], case["paired"]
    Dq = (D + 31) // 32 * 32
    Q, P = torch.zeros(N, Dq, device=dev), torch.zeros(N, Dq, device=dev)
    Q[:, :D], P[:, :D] = case["Q"].to(dev), case["P"].to(dev)
    flat = _nan(dev, case["Neg"].numel() + 4)
    Neg = flat[1 if shift else 0:][:case["Neg"].numel()].view(case["Neg"].shape)
    Neg.copy_(case["Neg"].to(dev))
    assert Neg.is_contiguous() and (M == 0 or (Neg.data_ptr() % 16 != 0) == bool(shift))
    g = case["g"].to(dev)
    loss, rows, dQ, dP = _nan(dev, 1), _nan(dev, N), _nan(dev, N, Dq), _nan(dev, N, Dq)
    dNeg = torch.full_like(Neg, NAN).contiguous() if dneg else None
    ws = _ws(dev, "mdl_infonce_neg_ws_bytes", N, M, D, paired)
    MF._call("mdl_infonce_neg_fwd", Q, P, Neg, loss, rows, N, M, D, paired, float(T), ws, _stream())
    d_loss, d_row = (g, None) if case["form"] == "d_loss" else (None, g)
    MF._call("mdl_infonce_neg_bwd", Neg, d_loss, d_row, dQ, dP, dNeg, N, M, D, paired, float(T), ws, _stream())
    torch.cuda.synchronize()
    return {"loss": loss.cpu(), "row_loss": rows.cpu(), "dQ": dQ.cpu(), "dP": dP.cpu(), "dNeg": dNeg.cpu() if dneg else None}


@pytest.mark.parametrize("spec", NEG, ids=_id)
def test_explicit_negatives(dev, spec):
    from madeleine_amd import _native
    N, M, D, T, paired, family, form, dneg, shift = spec
    plan = _native.dispatch_plan("infonce_neg", N, M, D)
    want = dict(variant=int(D % 4 == 0), splits=B.neg_splits(M, 0), chunk=B.neg_splits(M, 1), extra=max(1, -(-M // B.NEG_LSE_CH)))
    assert {k: plan[k] for k in want} == want, (spec, plan)
    case = B.neg_case(N, M, D, T, paired, family, form)
    got = _run_neg(dev, case, dneg, shift)
    what = "neg[%s]." % _id(spec)
    B.check_neg(got, case, what)
    for n, x in got.items():
        if x is not None:
            assert not bool(torch.isnan(x).any()), what + n
            if M == 0:                                              # a one-class cross entropy: loss and gradients exactly 0
                _exact_zero(what + n, x)
    Dq = got["dQ"].shape[1]
    if Dq > D:                                                      # the padding columns hold the gradient of their zeros
        _exact_zero(what + "dQ[:, D:]", got["dQ"][:, D:])
        _exact_zero(what + "dP[:, D:]", got["dP"][:, D:])
