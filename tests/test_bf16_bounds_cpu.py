"""The checkers of tests/_bf16_bounds.py, without a GPU: what tests/test_bf16_elements_gpu.py asserts of the bf16 kernels is asserted here
of a CPU emulation of the same contract, and of that emulation with one fault seeded.
  (a) The emulation -- torch fp32 products and sums, a bf16 cast and explicit rounding at the engine's rounding points -- passes every
      checker on every input kind at scaled-down shapes: the references alone stay inside the bounds.  The worst ratios are printed.
  (b) Seeded faults are each refused by the per-element checkers.  Beside each, what the criterion the suite had would have said (the norm
      at 2^-8 for bf16 outputs, at 1e-5 for fp32 ones) is asserted too: on the row_scaled inputs most of the faults pass it, which is
      the record of why the per-element tests exist.
  (c) The exact (integer) cases meet max |y| <= 256 for the seeds the GPU tests use."""
import pytest
import torch

from tests import _bf16_bounds as B

T, N, K = 300, 256, 512
EPS_BF16 = 2.0 ** -8


# ------------------------------------------------------------------------------------------------------------------ (a) the emulation passes
@pytest.mark.parametrize("kind", B.KINDS)
def test_emulated_linear_passes(kind):
    case = B.linear_case(T, N, K, 11, kind)
    B.check_linear(B.emulate_linear(case), B.linear_ref(case), kind, "linear[%s]." % kind)


def test_emulated_exact_linear_is_exact():
    case = B.linear_case(T, N, K, 12, "exact")
    B.check_linear(B.emulate_linear(case), B.linear_ref(case), "exact", "linear[exact].")


LENS = (0, 1, 63, 65, 140)


@pytest.mark.parametrize("kind", B.KINDS)
@pytest.mark.parametrize("lin", [False, True], ids=["softmax", "weighted"])
def test_emulated_pooling_passes(kind, lin):
    case = B.pool_case(LENS, 2, 21, kind)
    for acc, acc_s in ((0, 0), (1, 0 if lin else 1)):
        fwd, bwd = B.emulate_pool(case, lin, acc, acc_s)
        B.check_pool_fwd(fwd, case, lin, "pool[%s]." % kind)
        B.check_pool_bwd(bwd, case, lin, fwd, acc, acc_s, "pool[%s,acc%d]." % (kind, acc))


def test_emulated_exact_weighted_pooling_is_exact():
    case = B.pool_case(LENS, 2, 22, "exact")
    for acc in (0, 1):
        fwd, bwd = B.emulate_pool(case, True, acc, 0)
        B.check_pool_fwd(fwd, case, True, "wpool[exact].")
        B.check_pool_bwd(bwd, case, True, fwd, acc, 0, "wpool[exact,acc%d]." % acc)


def _masks(case, seed):
    g = torch.Generator().manual_seed(seed)
    shape = (case["T"], case["H"], B.HID)
    return tuple((torch.rand(shape, generator=g) >= case["p"]).to(torch.uint8) for _ in range(2))


def _check_gate(got, case, ka, kb, acc, what):
    fwd = B.gate_fwd_ref(case)
    for k in ("act_a", "act_b"):
        B.check(what + k, got[k], *fwd[k])
    B.check(what + "scores", got["scores"], *B.gate_scores_ref(case, got["act_a"], got["act_b"], ka, kb))
    bwd = B.gate_bwd_ref(case, got["act_a"], got["act_b"], ka, kb, acc)
    for k, v in bwd.items():
        B.check(what + k, got[k].reshape(v[0].shape), *v)


@pytest.mark.parametrize("kind", B.KINDS)
@pytest.mark.parametrize("p", [0.0, 0.25])
def test_emulated_gate_passes(kind, p):
    case = B.gate_case(45, 2, 31, kind, p)
    ka, kb = _masks(case, 32) if p else (None, None)
    for acc in (0, 1):
        _check_gate(B.emulate_gate(case, ka, kb, acc), case, ka, kb, acc, "gate[%s,p%g,acc%d]." % (kind, p, acc))


def _check_ln(fwd, bwd, case, what):
    ref = B.ln_fwd_ref(case, fwd["mean"], fwd["rstd"])
    for k in ("mean", "rstd", "y"):
        B.check(what + k, fwd[k], *ref[k])
    for k, v in B.ln_bwd_ref(case, fwd["mean"], fwd["rstd"]).items():
        B.check(what + k, bwd[k], *v)


@pytest.mark.parametrize("kind", B.KINDS)
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("groups", [None, [30, 0, 47]], ids=["plain", "groups"])
def test_emulated_layernorm_passes(kind, p, groups):
    case = B.ln_case(77, 256, 41, kind, p, groups)
    fwd, bwd = B.emulate_ln(case)
    _check_ln(fwd, bwd, case, "ln[%s,p%g]." % (kind, p))


# -------------------------------------------------------------------------------------------------------------------- (b) the seeded faults
def _faulty_linear():
    """The row_scaled Linear case with its emulation, reference and bounds.  The last row is made the smallest (2^-12 of the largest), the
    place where a norm cannot see."""
    case = B.linear_case(T, N, K, 51, "row_scaled")
    for k in ("x", "dy"):
        row = case[k][-1]
        case[k][-1] = row / row.abs().max() * 2.0 ** -12 * float(case[k].abs().max())
        case[k] = B.rb(case[k])
    ref = B.linear_ref(case)
    return case, B.emulate_linear(case), ref, B.linear_bounds(ref, "row_scaled")


def _verdicts(name, got, ref, bounds, old_tol):
    """(the per-element checker passes, the norm criterion passes)."""
    return B.passes(got, ref[name][0], *bounds[name]), B.rel_err(got, ref[name][0]) < old_tol


def test_fault_last_row_misses_its_last_k_chunk():
    case, emu, ref, bounds = _faulty_linear()
    assert _verdicts("Y", emu["Y"], ref, bounds, EPS_BF16) == (True, True)
    y = emu["Y"].clone()
    y[-1] = B.rb(case["x"][-1, :K - 32] @ case["W"][:, :K - 32].t() + case["b"])
    assert _verdicts("Y", y, ref, bounds, EPS_BF16) == (False, True)


def test_fault_last_row_misses_the_bias():
    case, emu, ref, bounds = _faulty_linear()
    y = emu["Y"].clone()
    y[-1] = B.rb(case["x"][-1] @ case["W"].t())
    assert _verdicts("Y", y, ref, bounds, EPS_BF16) == (False, True)


def test_fault_one_element_two_ulps_off():
    case, emu, ref, bounds = _faulty_linear()
    y = emu["Y"].clone()
    bits = y.to(B.BF).view(torch.int16)
    bits[T // 2, N // 2] += 2
    assert _verdicts("Y", bits.view(B.BF).float(), ref, bounds, EPS_BF16) == (False, True)
    dx = emu["dX"].clone()
    bits = dx.to(B.BF).view(torch.int16)
    bits[-1, 3] += 2
    assert _verdicts("dX", bits.view(B.BF).float(), ref, bounds, EPS_BF16) == (False, True)


def test_fault_truncation_in_place_of_rounding():
    case, emu, ref, bounds = _faulty_linear()
    y = B.truncate_bf16(case["x"] @ case["W"].t() + case["b"])
    assert _verdicts("Y", y, ref, bounds, EPS_BF16) == (False, True)
    dx = B.truncate_bf16(case["dy"] @ case["W"])
    assert _verdicts("dX", dx, ref, bounds, EPS_BF16) == (False, True)


def test_fault_dw_misses_the_last_token_of_a_partial_chunk():
    """A sum over the tokens cannot show a token that is 2^-24 of the others, by any criterion: this fault is for the uniform inputs, where
    the norm sees it too, and for the integer case, where one token of 2^-12 the norm of dW is refused to the bit."""
    assert T % 32 != 0
    case = B.linear_case(T, N, K, 51, "uniform")
    ref = B.linear_ref(case)
    bounds = B.linear_bounds(ref)
    assert _verdicts("dW", B.emulate_linear(case)["dW"], ref, bounds, 1e-5) == (True, True)
    assert _verdicts("dW", case["dy"][:-1].t() @ case["x"][:-1], ref, bounds, 1e-5) == (False, False)
    assert _verdicts("db", case["dy"][:-1].sum(0), ref, bounds, 1e-5) == (False, False)
    case = B.linear_case(4096, N, K, 52, "exact")
    ref = B.linear_ref(case)
    dW = case["dy"][:-1].t() @ case["x"][:-1]
    with pytest.raises(AssertionError):
        B.check_exact("dW", dW, ref["dW"][0])
    assert float((dW.double() - ref["dW"][0]).abs().max()) == 1.0


def _faulty_pool(lin):
    """Row-scaled bags; the rows of the second bag (one token) and of the third are made small next to the first."""
    case = B.pool_case((140, 1, 63, 65), 2, 61, "row_scaled")
    case["E"][140:] = B.rb(case["E"][140:] * 2.0 ** -18)
    fwd, bwd = B.emulate_pool(case, lin, 1, 0)
    return case, fwd, bwd


def _pool_passes(fn, *args):
    try:
        fn(*args)
    except AssertionError:
        return False
    return True


def test_fault_accumulate_ignored():
    case, fwd, _ = _faulty_pool(False)
    _, wrong = B.emulate_pool(case, False, 0, 0)         # dE written where it had to be added to
    assert not _pool_passes(B.check_pool_bwd, wrong, case, False, fwd, 1, 0)
    ref = B.pool_bwd_ref(case, False, fwd["pooled"], fwd["m"], fwd["l"], 1, 0)
    assert not B.rel_err(wrong["dE"], ref["dE"]) < EPS_BF16          # the one fault of this file that the norm sees as well
    # the gate's dE likewise
    gc = B.gate_case(45, 1, 62, "row_scaled")
    emu = B.emulate_gate(gc, acc=0)
    want = B.gate_bwd_ref(gc, emu["act_a"], emu["act_b"], None, None, 1)["dE"]
    assert not B.passes(emu["dE"], *want)


def test_fault_neighbouring_bags_token_leaks_into_a_pooled_row():
    """Bags 2 and 3 are 2^-18 of bag 0: the largest token of bag 3 is pooled into bag 2's row as well."""
    for lin in (True, False):
        case, fwd, _ = _faulty_pool(lin)
        B.check_pool_fwd(fwd, case, lin)
        seg = list(case["segments"])
        t = seg[3][case["E"][seg[3]].abs().amax(1).argmax()]
        seg[2] = torch.cat([seg[2], t[None]])
        leaky = B.pool_fwd_ref(dict(case, segments=seg), lin, torch.float32)
        assert not _pool_passes(B.check_pool_fwd, leaky, case, lin)
        assert B.rel_err(leaky["pooled"], B.pool_fwd_ref(case, lin)["pooled"]) < 1e-5                 # the norm at 1e-5 lets it through


# --------------------------------------------------------------------------------------------------------- (c) the exact cases stay exact
def test_exact_cases_stay_inside_the_integers_bf16_holds():
    from tests.test_bf16_elements_gpu import EXACT_SEED, LINEAR_TAILS, LINEAR_THRESHOLDS
    for T_, N_, K_ in [(t, n, k) for t in LINEAR_TAILS[0] for n, k in LINEAR_TAILS[1]] + [s[:3] for s in LINEAR_THRESHOLDS]:
        assert K_ <= 1056 and N_ <= 1024
        case = B.linear_case(T_, N_, K_, EXACT_SEED + T_ + N_ + K_, "exact")
        x, W, b, dy = (case[k] for k in ("x", "W", "b", "dy"))        # (integers below 2^24: fp32 holds every partial sum)
        assert float((x @ W.t() + b).abs().max()) <= 256, (T_, N_, K_)
        assert float((dy @ W).abs().max()) <= 256, (T_, N_, K_)
