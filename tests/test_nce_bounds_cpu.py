"""The checkers of tests/_nce_bounds.py, without a GPU: what tests/test_nce_elements_gpu.py asserts of the InfoNCE kernels is asserted here
of a torch fp32 emulation of the same contract, and of that emulation with one fault seeded.
  (a) The written-out fp64 references are the documented operation: oracle.restatement.info_nce and the ref_loss formula of the
      explicit negatives under torch autograd in fp64 agree with them.
  (b) The emulation passes every checker over the case list of the GPU file (ratio <= 1); the worst ratio per output kind is printed.
  (c) LSE_R covers the measurement it is defined by, over the same case list.
  (d) Twelve seeded faults are each refused in a named case.  Beside each, what the criteria the suite had would have said -- the scalar
      loss within TOL |ref| + 1e-5, rel_err < 1e-4 on the gradients, _grad_ok -- is printed (NCEFAULT lines); the faults of
      EXPECTED_THROUGH went through all three (rel_err 1e-7 to 4e-7 where the per-element ratio is above 100), which is asserted."""
import pytest
import torch

from oracle import restatement as R
from tests import _nce_bounds as B
from tests.test_nce_elements_gpu import INBATCH, NEG, _id, inbatch_cases, neg_cases

TOL = 1e-3           # tests/test_hip_kernels.py, tests/test_infonce_negatives_gpu.py


# ------------------------------------------------------------------------------------------------- (a) the references are the oracle's
def _agrees(name, mine, oracle, scale):
    err = (mine - oracle).abs()
    tol = 1e-9 * mine.abs().amax(-1, keepdim=True) + 1e-11 * scale if mine.dim() > 1 else 1e-9 * mine.abs() + 1e-11 * scale
    assert bool((err <= tol).all()), (name, float((err / tol.clamp_min(1e-300)).max()))


def _grad_scale(x, g, T):
    """rn |g| / T: the size of a gradient row before any cancellation (the noise of fp64 autograd on a saturated row is 1e-16 of it)."""
    return B.normalize64(x)[1][..., None] * float(g[~torch.isnan(g)].abs().max()) / B.t32(T)


@pytest.mark.parametrize("spec", INBATCH, ids=_id)
def test_inbatch_reference_is_the_oracle_under_autograd(spec):
    Kmax, D, T, sym, family, form = spec
    case = B.inbatch_case((Kmax, B.mid_count(Kmax), 1), Kmax, D, T, sym, family, form)
    mine, oracle = B.inbatch_ref(case), B.oracle_inbatch(case)
    _agrees("loss", mine["loss"][0], oracle["loss"], 1.0)
    _agrees("row_loss", mine["row_loss"][0], oracle["row_loss"], 1.0)
    for n, x in (("dQ", "Q"), ("dP", "P")):
        _agrees(n, mine[n][0], oracle[n], _grad_scale(torch.nan_to_num(case[x]), case["g"], T))


@pytest.mark.parametrize("spec", NEG, ids=_id)
def test_negatives_reference_is_the_oracle_under_autograd(spec):
    case = B.neg_case(*spec[:7])
    D = case["D"]
    mine, oracle = B.neg_ref(case), B.oracle_neg(case)
    _agrees("loss", mine["loss"][0], oracle["loss"], 1.0)
    _agrees("row_loss", mine["row_loss"][0], oracle["row_loss"], 1.0)
    for n, x in (("dQ", "Q"), ("dP", "P")):
        _agrees(n, mine[n][0][:, :D], oracle[n], _grad_scale(case[x], case["g"], case["T"]))
    if case["M"]:
        _agrees("dNeg", mine["dNeg"][0], oracle["dNeg"], _grad_scale(case["Neg"], case["g"], case["T"]))


# ------------------------------------------------------------------------------------------------------- (b) the emulation passes
WORST = {}


def _record(kind, ratios):
    for n, r in ratios.items():
        WORST[(kind, n)] = max(WORST.get((kind, n), 0.0), r)
        print("NCEERR emulation worst so far %s %s %.3f" % (kind, n, WORST[(kind, n)]))


@pytest.mark.parametrize("spec", INBATCH + [(33, 64, 0.07, 1, "uniform", "d_loss", "empty")], ids=_id)
def test_emulated_inbatch_passes(spec):
    Kmax, D, T, sym, family, form = spec[:6]
    cnt = (0,) if len(spec) == 7 else (Kmax, B.mid_count(Kmax), 1)
    case = B.inbatch_case(cnt, Kmax, D, T, sym, family, form, "empty" if len(spec) == 7 else "")
    _record("in-batch", B.check_inbatch(B.emulate_inbatch(case), case, "emulated[%s]." % _id(spec)))


@pytest.mark.parametrize("spec", NEG, ids=_id)
def test_emulated_negatives_pass(spec):
    case = B.neg_case(*spec[:7])
    _record("paired" if case["paired"] else "unpaired", B.check_neg(B.emulate_neg(case), case, "emulated[%s]." % _id(spec)))


# ---------------------------------------------------------------------------------------------------------- (c) the measured constant
def test_lse_constant_covers_every_case():
    """LSE_R is the worst torch fp32 log_softmax error, in units of u (1 + |l| + |z - m|), over the reference logits of every case."""
    worst, where = 0.0, None
    for case in inbatch_cases():
        for s, z in enumerate(B.inbatch_ref(case)["logits"]):
            for d, zz in enumerate((z, z.t()) if case["sym"] else (z,)):
                r = B.lse_ratio(zz)
                if r > worst:
                    worst, where = r, ("in-batch", case["Kmax"], case["D"], case["T"], case["family"], "stain %d" % s, "dir %d" % d)
    for case in neg_cases():
        r = B.lse_ratio(B.neg_ref(case)["logits"])
        if r > worst:
            worst, where = r, ("negatives", case["N"], case["M"], case["D"], case["T"], case["family"], "paired %d" % case["paired"])
    print("NCEERR LSE_R measured %.3f at %s (constant %.3f, x %g allowed)" % (worst, where, B.LSE_R, B.LSE_FACTOR))
    assert worst <= B.LSE_R and B.LSE_R <= 1.25 * worst + 0.05, (worst, where)


# ------------------------------------------------------------------------------------------------------------- (d) the seeded faults

def _grad_ok(hip, ref32, ref64):
    """tests/test_hip_kernels.py::_grad_ok as a predicate."""
    e_hip, e_ref = float((hip.double() - ref64).norm()), float((ref32.double() - ref64).norm())
    return e_hip <= max(TOL * float(ref64.norm()), 2.0 * e_ref) + 1e-30


def _old_inbatch(got, case):
    """What the suite's criteria say of `got`, problem by problem: (loss TOL, rel_err < 1e-4 on dQ and dP, _grad_ok on dQ and dP)."""
    ref = B.inbatch_ref(case)
    loss = norm = ok = True
    for s, k in enumerate(case["cnt"]):
        if k == 0:
            continue
        q, p = case["Q"][s, :k].clone().requires_grad_(), case["P"][s, :k].clone().requires_grad_()
        rows = R.info_nce(q, p, case["T"], bool(case["sym"]), reduction="none")
        (rows.mean() * case["g"][s] if case["form"] == "d_loss" else (rows * case["g"][s, :k]).sum()).backward()
        r = float(ref["loss"][0][s])
        loss &= abs(float(got["loss"][s]) - r) <= TOL * abs(r) + 1e-5
        for n, g32 in (("dQ", q.grad), ("dP", p.grad)):
            norm &= B.rel_err(got[n][s, :k], ref[n][0][s, :k]) < 1e-4
            ok &= _grad_ok(got[n][s, :k], g32, ref[n][0][s, :k])
    return loss, norm, ok


def _old_neg(got, case):
    ref, r32 = B.neg_ref(case), B.oracle_neg(case, torch.float32)
    D, r = case["D"], float(B.neg_ref(case)["loss"][0])
    loss = abs(float(got["loss"]) - r) <= TOL * abs(r) + 1e-5
    norm = ok = True
    for n in ("dQ", "dP", "dNeg"):
        a, b = (got[n], ref[n][0]) if n == "dNeg" else (got[n][:, :D], ref[n][0][:, :D])
        norm &= B.rel_err(a, b) < 1e-4
        ok &= _grad_ok(a, r32[n], b)
    return loss, norm, ok


def _fault(number, name, case, what, old, clean_ok, refused):
    through = all(old)
    print("NCEFAULT %2d %-26s refused in %s at %s; the old criteria: loss TOL %s, rel_err < 1e-4 %s, _grad_ok %s"
          % (number, name, what, sorted(n for n, ok in refused.items() if not ok), *("passes" if o else "fails" for o in old)))
    assert all(clean_ok.values()), (name, clean_ok)                 # the emulation without the fault passes the same case
    assert not all(refused.values()), (name, "no output refuses it")
    return through


INBATCH_FAULTS = [
    (1, "col_lse_k_minus_1", (33, 512, 0.001, 1, "clustered", "d_row_loss")),
    (2, "col_lse_over_Kp", (33, 32, 1.0, 1, "uniform", "d_row_loss")),
    (3, "no_delta_at_32", (33, 64, 0.07, 1, "degenerate", "d_row_loss")),
    (4, "g_i_for_g_j", (65, 64, 0.07, 1, "uniform", "d_row_loss")),
    (5, "no_dot_on_longest_row", (256, 64, 0.07, 1, "row_scaled", "d_row_loss")),
    (6, "clamped_as_unclamped", (33, 64, 0.07, 1, "degenerate", "d_row_loss")),
    (7, "mean_over_Kmax", (65, 512, 0.001, 0, "clustered", "d_loss")),
]
NEG_FAULTS = [
    (8, "lse_chunk_dropped", (33, 4097, 100, 0.07, 0, "uniform", "d_loss")),
    (9, "dq_split_dropped", (33, 1025, 100, 0.07, 0, "row_scaled", "d_row_loss")),
    (10, "neighbours_inverse_norm", (5, 65, 100, 0.001, 1, "clustered", "d_loss")),
    (11, "dot_without_T", (33, 65, 100, 0.001, 0, "clustered", "d_row_loss")),
    (12, "tail_columns_unread", (33, 65, 101, 0.001, 0, "clustered", "d_loss")),
]
# measured here: the faults that every criterion the suite had lets through in the case named above, by three orders of magnitude (a
# missing delta beside rows that normalize() scales by 1e12; the projection dropped on the longest row, whose gradient is the smallest).
# The other verdicts are printed, not asserted: several sit near their thresholds.
EXPECTED_THROUGH = {"no_delta_at_32": True, "no_dot_on_longest_row": True}


@pytest.mark.parametrize("number,name,spec", INBATCH_FAULTS, ids=[f[1] for f in INBATCH_FAULTS])
def test_inbatch_fault_is_refused(number, name, spec):
    assert spec in INBATCH
    Kmax, D, T, sym, family, form = spec
    case = B.inbatch_case((Kmax, B.mid_count(Kmax), 1), Kmax, D, T, sym, family, form)
    got = B.emulate_inbatch(case, name)
    through = _fault(number, name, case, "in-batch[%s]" % _id(spec), _old_inbatch(got, case), B.inbatch_passes(B.emulate_inbatch(case), case),
                     B.inbatch_passes(got, case))
    assert through == EXPECTED_THROUGH.get(name, through)


@pytest.mark.parametrize("number,name,spec", NEG_FAULTS, ids=[f[1] for f in NEG_FAULTS])
def test_negatives_fault_is_refused(number, name, spec):
    assert spec in [s[:7] for s in NEG]
    case = B.neg_case(*spec)
    got = B.emulate_neg(case, name)
    through = _fault(number, name, case, "negatives[%s]" % _id(spec), _old_neg(got, case), B.neg_passes(B.emulate_neg(case), case),
                     B.neg_passes(got, case))
    assert through == EXPECTED_THROUGH.get(name, through)
