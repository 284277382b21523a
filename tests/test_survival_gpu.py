"""The survival probe on the device (mdl_cox_fit / mdl_surv_metrics, madeleine_amd.survival) against an fp64 damped Newton reference and
direct O(S^2) recounts on the CPU (tests/_survival_ref.py) over three closed-form cohorts with tied, censored and missing follow-up:
A (S 330, d 4 in ldX 8, cost 1, n_train 1, 63, 64, 65, 255, 256, 257), B (S 330, d 512 > n, cost 4, n_train 1, 64, 65, 257) and L (S 1300,
d 64 in ldX 72, n_train 1024 exactly).  The padding columns hold NaN.  gtol is the default, 1e-3 relative to the gradient at w = 0.

Figures measured on the MI355X are in the docstrings of test_optimality and test_decision_values; every test prints its own."""
import functools
import math
import warnings

import numpy as np
import pytest
import torch

from tests import _survival_ref as R

pytestmark = pytest.mark.gpu
GTOL = 1e-3
DEV = "cuda"


def _table(idx_lists):
    from madeleine_amd.survival import _problem_table
    return _problem_table([torch.as_tensor(t).reshape(-1) for t in idx_lists], DEV)


def _device_X(X, ldX):
    """X [S, d] fp32 on the device as a view of a [S, ldX] buffer (NaN in the padding columns: they are never read)."""
    S, d = X.shape
    buf = torch.full((S, ldX), float("nan"), dtype=torch.float32, device=DEV)
    buf[:, :d] = X.float().to(DEV)
    return buf[:, :d]


def _scores(X_dev, W):
    from madeleine_amd import functional as F
    return F.probe_scores(X_dev, W.unsqueeze(1), torch.zeros(W.shape[0], 1, device=DEV), 2).squeeze(2)


def _run(X_dev, time, event, idx_lists, cost=1.0, **kw):
    """Fit, scores and metrics of a problem list in one launch sequence each; everything back on the host."""
    from madeleine_amd import functional as F
    table, n_train = _table(idx_lists)
    t_dev, e_dev = time.float().to(DEV).contiguous(), event.to(torch.int32).to(DEV).contiguous()
    W, thr, info = F.cox_fit(X_dev, t_dev, e_dev, table, n_train, cost, GTOL, **kw)
    z = _scores(X_dev, W)
    c, chi2, counts = F.survival_metrics(z, t_dev, e_dev, table, n_train, thr)
    torch.cuda.synchronize()
    return dict(W=W.cpu(), thr=thr.cpu(), info=info.cpu(), z=z.cpu(), c=c.cpu(), chi2=chi2.cpu(), counts=counts.cpu())


@functools.lru_cache(maxsize=None)
def _cohort_run(name):
    co = R.cohort(name)
    return co, _run(_device_X(co["X"], co["ldX"]), co["time"], co["event"], [p["idx"] for p in co["problems"]], co["cost"])


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else (t.view(torch.int64) if t.dtype == torch.float64 else t)


def _bits_equal(a, b, p, q, keys=None):
    return all(torch.equal(_bits(a[k][p]), _bits(b[k][q])) for k in (keys or a))


def _same(a, b, rel=1e-12):
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= rel * abs(b)


@pytest.mark.parametrize("name", list(R.COHORTS))
def test_optimality(name):
    """Every legal problem converges, and the fp64 gradient of the primal objective at the returned W is within max(2 gtol g0, 2 r32):
    the stop rule plus the kernel's own fp32 evaluation error, or twice what the reference iteration reaches in fp32.
    Measured on the MI355X: 2-7 Newton steps and 7-217 CG steps per problem; worst fp64 gradient / g0 4.6e-5 (A), 3.8e-6 (B), 8.3e-5 (L)."""
    _optimality(name, *_cohort_run(name))


def _optimality(name, co, out):
    X32 = co["X"].float()
    worst = 0.0
    for p, pr in enumerate(co["problems"]):
        idx = pr["idx"]
        g = R.primal_grad_inf(X32[idx], co["time"][idx], co["event"][idx], out["W"][p], co["cost"])
        bound = max(2 * GTOL * pr["g0"], 2 * pr["r32"])
        print("%s n=%d: steps %d cg %d residual %.2e (kernel) %.2e (fp64) g0 %.2e r32 %.2e" % (
            name, idx.numel(), out["info"][p, 0], out["info"][p, 3], out["info"][p, 2], g, pr["g0"], pr["r32"]))
        assert out["info"][p, 1] == 1, (name, idx.numel(), out["info"][p])
        assert g <= bound, (name, idx.numel(), g, bound)
        worst = max(worst, g / pr["g0"]) if pr["g0"] > 0 else worst
    print("%s worst fp64 gradient / g0 %.2e" % (name, worst))


@pytest.mark.parametrize("name", list(R.COHORTS))
def test_decision_values(name):
    """E_p = max_S |z - z64| / max_S |z64| <= 1e-3 (the project's parity contract) for every problem; where the optimum is w = 0 (one
    training row) the decision values are exactly 0.  The threshold is numpy's median of the training rows' scores as mdl_probe_scores
    gives them, bit for bit: the fit kernel forms its decision values by the same fmaf chain and wave sum.
    Worst E_p measured on the MI355X: A 4.6e-5, B 1.0e-5, L 7.2e-5."""
    _decision_values(name, *_cohort_run(name))


def _decision_values(name, co, out):
    worst = 0.0
    for p, pr in enumerate(co["problems"]):
        z, z64 = out["z"][p].double(), pr["z64"]
        if float(z64.abs().max()) == 0.0:
            assert not bool(z.any()) and float(out["thr"][p]) == 0.0
            continue
        E = float((z - z64).abs().max() / z64.abs().max())
        worst = max(worst, E)
        assert E <= 1e-3, (name, pr["idx"].numel(), E)
        med = float(np.median(out["z"][p][pr["idx"]].numpy()))
        assert float(out["thr"][p]) == med, (name, pr["idx"].numel(), float(out["thr"][p]), med)
    print("%s worst E_p %.2e" % (name, worst))


@pytest.mark.parametrize("name", list(R.COHORTS))
def test_metrics_equal_the_host_recount(name):
    """c_index, chi2 and all six counts from the device's own z and thr equal the host's recount from the same numbers: the integers bit
    for bit, the two doubles to 1e-12 relative."""
    _metrics_equal_the_host_recount(name, *_cohort_run(name))


def _metrics_equal_the_host_recount(name, co, out):
    tm, ev = co["time"].numpy(), co["event"].numpy()
    for p, pr in enumerate(co["problems"]):
        test = R.test_mask(ev, pr["idx"].numpy())
        counts, c, chi2 = R.counts_row(out["z"][p].numpy(), float(out["thr"][p]), tm, ev, test)
        assert out["counts"][p].tolist() == counts, (name, p, out["counts"][p].tolist(), counts)
        got = (float(out["c"][p]), float(out["chi2"][p]))
        assert _same(got[0], c) and _same(got[1], chi2), (name, p, got, c, chi2)
        print("%s n=%d: C %.4f chi2 %.3f counts %s" % (name, pr["idx"].numel(), c, chi2, counts))


@pytest.mark.parametrize("name", list(R.COHORTS))
def test_metrics_against_fp64_optimum(name):
    """With D = max_S |z - z64|: the concordance numerator differs from the fp64 one by at most twice the number of comparable pairs whose
    fp64 score gap is below 2 D (never more than 4 % of the comparable pairs), and the risk group differs only for test cases within 2 D
    of the fp64 threshold, the median of z64 over the training rows.  The same D everywhere: the kernel's threshold is the median of the
    device's own z (test_decision_values), so it lies within D of the fp64 one."""
    _metrics_against_fp64_optimum(name, *_cohort_run(name))


def _metrics_against_fp64_optimum(name, co, out):
    tm, ev = co["time"].numpy(), co["event"].numpy()
    for p, pr in enumerate(co["problems"]):
        test = R.test_mask(ev, pr["idx"].numpy())
        z64 = pr["z64"].numpy()
        D = float((out["z"][p].double() - pr["z64"]).abs().max())
        num64, comp64 = R.concordance(z64, tm, ev, test)
        close = R.close_pairs(z64, tm, ev, test, 2 * D)
        assert int(out["counts"][p, 1]) == comp64
        assert close <= 0.04 * comp64, (name, p, close, comp64)
        assert abs(int(out["counts"][p, 0]) - num64) <= 2 * close, (name, p, int(out["counts"][p, 0]), num64, close)
        thr64 = float(np.median(z64[pr["idx"].numpy()]))
        moved = (out["z"][p].numpy() > float(out["thr"][p])) != (z64 > thr64)
        assert bool((np.abs(z64 - thr64)[moved & test] <= 2 * D).all()), (name, p)


def _hand_cases():
    """(name, z, time, event, thr, expected (c_index, chi2) or None for "as the host recount")."""
    nan = float("nan")
    e8 = [1, 1, 1, 0, 1, 0, 1, 0]
    t8 = [1, 2, 2, 3, 4, 4, 5, 6]
    return [
        ("all risks equal", [0.25] * 6, [1, 2, 3, 4, 5, 6], [1, 1, 0, 1, 1, 0], 0.0, (0.5, None)),
        ("perfectly ordered", [6, 5, 4, 3, 2, 1], [1, 2, 3, 4, 5, 6], [1, 1, 0, 1, 1, 0], 3.5, (1.0, None)),
        ("reversed", [1, 2, 3, 4, 5, 6], [1, 2, 3, 4, 5, 6], [1, 1, 0, 1, 1, 0], 3.5, (0.0, None)),
        # the event at 2 against the censored case at 2 is the only comparable pair, ranked right
        ("an event tied with a censored case", [1.0, 0.0], [2, 2], [1, 0], 0.5, (1.0, None)),
        ("two tied events are not comparable", [1.0, 0.0], [2, 2], [1, 1], 0.5, (nan, None)),
        ("no comparable pair: the only event is last", [3.0, 2.0, 1.0], [1, 2, 3], [0, 0, 1], 1.5, (nan, None)),
        ("one group empty", [1, 2, 3, 4], [1, 2, 3, 4], [1, 0, 1, 1], 9.0, (None, nan)),
        ("missing follow-up is left out", [5, 1, 4, 2, 3, 0], [1, 2, 3, 4, 5, 6], [1, -1, 1, 0, -1, 1], 2.5, None),
        # high = z > 0.  Per event case (n, h, d): (8, 4, 1), (7, 3, 2), (7, 3, 2), (4, 2, 1), (2, 0, 1):
        #   O - E = (1 - 4/8) + (0 - 3/7) + (1 - 3/7) + (1 - 2/4) + (0 - 0) = 8/7
        #   V = 1/4 * 7/7 + 2 * (3/7)(4/7)(5/6) + 1/4 * 3/3 + 0 = 1/2 + 20/49 = 89/98;  chi2 = (64/49) / (89/98) = 128/89
        ("eight cases worked by hand", [1, -1, 1, -1, 1, 1, -1, -1], t8, e8, 0.0, (None, 128.0 / 89.0)),
    ]


@pytest.mark.parametrize("case", _hand_cases(), ids=lambda c: c[0])
def test_metrics_kernel_on_hand_made_scores(case):
    from madeleine_amd import functional as F
    name, z, tm, ev, thr, expected = case
    z, tm, ev = np.array(z, dtype=np.float32), np.array(tm, dtype=np.float32), np.array(ev)
    table = torch.full((1, 1), -1, dtype=torch.int32, device=DEV)
    n_train = torch.zeros(1, dtype=torch.int32, device=DEV)
    c, chi2, counts = F.survival_metrics(torch.from_numpy(z)[None].to(DEV), torch.from_numpy(tm).to(DEV),
                                         torch.from_numpy(ev).to(torch.int32).to(DEV), table, n_train,
                                         torch.tensor([thr], dtype=torch.float32, device=DEV))
    want, c_ref, chi2_ref = R.counts_row(z, np.float32(thr), tm, ev, R.test_mask(ev, np.zeros(0, dtype=np.int64)))
    assert counts[0].tolist() == want
    assert _same(float(c[0]), c_ref) and _same(float(chi2[0]), chi2_ref), (float(c[0]), c_ref, float(chi2[0]), chi2_ref)
    if expected is not None:
        for got, exp in zip((float(c[0]), float(chi2[0])), expected):
            assert exp is None or _same(got, exp), (name, got, exp)
    if name.startswith("eight"):
        assert want == [want[0], want[1], 8, 4, 2, 3]


def test_invariances():
    """Cohort A's seven problems again, in reverse batch order, every training list permuted, and time / event replicated per problem
    instead of shared (stride S instead of 0): W, thr, info and the metrics are bit-identical.  A problem alone (P = 1, its own n_max)
    gives the same bits too."""
    co, ref = _cohort_run("A")
    X_dev = _device_X(co["X"], co["ldX"])
    P = len(co["problems"])
    g = torch.Generator().manual_seed(5)
    lists = [pr["idx"][torch.randperm(pr["idx"].numel(), generator=g)] for pr in reversed(co["problems"])]
    got = _run(X_dev, co["time"][None].repeat(P, 1), co["event"][None].repeat(P, 1), lists, co["cost"])
    for p in range(P):
        assert _bits_equal(ref, got, p, P - 1 - p), p
    for p in (1, 3, 6):
        alone = _run(X_dev, co["time"], co["event"], [co["problems"][p]["idx"]], co["cost"])
        assert _bits_equal(ref, alone, p, 0), p


def test_degenerate_and_refused():
    """A training list without an event gives W = 0 and converged; a list with a repeated index, an index out of range, a case without
    follow-up, or a NaN, infinite or negative time has that problem all NaN and converged = 0 -- and its neighbours unchanged."""
    from madeleine_amd import functional as F
    co, ref = _cohort_run("A")
    X_dev = _device_X(co["X"], co["ldX"])
    S, ev = co["X"].shape[0], co["event"]
    good = [co["problems"][p]["idx"] for p in (1, 4)]
    censored = torch.nonzero(ev == 0)[:40, 0]
    base = good[0].clone()
    repeated, outside, low, unlabeled = base.clone(), base.clone(), base.clone(), base.clone()
    repeated[7] = repeated[50]
    outside[3] = S
    low[0] = -1                                       # inside n_train: the table's padding value is an index out of range there
    unlabeled[11] = int(torch.nonzero(ev == -1)[0, 0])
    lists = [good[0], censored, repeated, good[1], outside, unlabeled, base, base, base, low, good[0]]
    P = len(lists)
    time = co["time"][None].repeat(P, 1)
    time[6, base[5]], time[7, base[9]], time[8, base[60]] = float("nan"), float("inf"), -0.25
    table, n_train = _table(lists)
    t_dev, e_dev = time.to(DEV).contiguous(), ev.to(torch.int32).to(DEV)
    W, thr, info = F.cox_fit(X_dev, t_dev, e_dev, table, n_train, co["cost"], GTOL)
    z = _scores(X_dev, W)
    c, chi2, counts = F.survival_metrics(z, t_dev, e_dev, table, n_train, thr)
    got = dict(W=W.cpu(), thr=thr.cpu(), info=info.cpu(), z=z.cpu(), c=c.cpu(), chi2=chi2.cpu(), counts=counts.cpu())
    for p, q in ((0, 1), (3, 4), (10, 1)):            # the legal neighbours: the bits of the cohort's own run
        assert _bits_equal(got, ref, p, q), p
    assert not bool(got["W"][1].any()) and float(got["thr"][1]) == 0.0 and got["info"][1].tolist() == [0.0, 1.0, 0.0, 0.0]
    for p in (2, 4, 5, 6, 7, 8, 9):
        assert bool(torch.isnan(got["W"][p]).all()) and math.isnan(float(got["thr"][p])), p
        assert float(got["info"][p, 1]) == 0.0 and math.isnan(float(got["info"][p, 2])), p
        assert math.isnan(float(got["c"][p])) and math.isnan(float(got["chi2"][p])), p


def test_refusals():
    from madeleine_amd import functional as F
    from madeleine_amd import fit_cox, survival_probe
    X = torch.zeros(1100, 4, device=DEV)
    t, e = torch.ones(1100, device=DEV), torch.ones(1100, dtype=torch.int32, device=DEV)
    one = torch.ones(1, dtype=torch.int32, device=DEV)
    launches = []
    real = F._call
    try:
        F._call = lambda name, *a, **k: (launches.append(name), real(name, *a, **k))[1]
        with pytest.raises(NotImplementedError, match="at most 1024 training cases"):
            F.cox_fit(X, t, e, torch.zeros(1, 1025, dtype=torch.int32, device=DEV), one)      # n_max = 1025
        with pytest.raises(NotImplementedError):
            F.survival_metrics(torch.zeros(1, 16385, device=DEV), torch.ones(16385, device=DEV),
                               torch.ones(16385, dtype=torch.int32, device=DEV), torch.zeros(1, 4, dtype=torch.int32, device=DEV), one,
                               torch.zeros(1, device=DEV))
    finally:
        F._call = real
    assert launches == []                             # refused by the workspace query: no entry point that launches was called
    with pytest.raises(RuntimeError):
        fit_cox(X.cpu(), t, e, [torch.tensor([0, 1])])
    with pytest.raises(RuntimeError):
        F.cox_fit(X, t, e.long(), torch.zeros(1, 4, dtype=torch.int32, device=DEV), one)      # event must be int32
    bad = torch.zeros(8, 4)
    bad[3, 1] = float("inf")
    with pytest.raises(ValueError):
        survival_probe(bad, torch.ones(8), torch.ones(8, dtype=torch.int64), folds=2)
    with pytest.raises(ValueError):
        survival_probe(torch.zeros(8, 4), {"a": torch.ones(8)}, torch.ones(8), folds=2)


def test_survival_probe_end_to_end():
    """Two endpoints over cohort A (the second with other times and more missing follow-up), 3 folds x 2 repeats: keys, shapes, the fold
    bookkeeping and every number against the pieces called by hand on one problem at a time; exactly two host reads."""
    from madeleine_amd import fit_cox, survival_probe, survival_splits
    from madeleine_amd import functional as F
    co = R.cohort("A")
    X_dev = _device_X(co["X"], co["ldX"])
    t2, e2 = co["time"].flip(0).contiguous(), co["event"].clone()
    e2[::4] = -1
    times, events = {"os": co["time"].numpy(), "pfs": t2}, {"os": co["event"], "pfs": e2.numpy()}
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)      # every fit converges
        res = survival_probe(X_dev, times, events, folds=3, repeats=2, cost=co["cost"])      # also the warm-up of the counted call
    assert set(res) == {("os", 0), ("os", 1), ("pfs", 0), ("pfs", 1)}
    for (name, repeat), r in res.items():
        t, e = (co["time"], co["event"]) if name == "os" else (t2, e2)
        assert set(r) == {"c_index", "logrank_chi2", "logrank_p", "converged", "threshold", "counts"}
        assert r["c_index"].shape == r["logrank_chi2"].shape == r["logrank_p"].shape == r["converged"].shape == r["threshold"].shape == (3,)
        assert r["counts"].shape == (3, 6) and r["converged"].all()
        splits = survival_splits(e, 3, repeat, 0)
        for fold in range(3):
            assert r["counts"][fold, 2] == int((e >= 0).sum()) - splits[fold].numel()
            assert r["counts"][fold, 4] + r["counts"][fold, 5] == int((e == 1).sum()) - int((e[splits[fold]] == 1).sum())
            assert 0.0 <= r["c_index"][fold] <= 1.0
            assert abs(r["logrank_p"][fold] - math.erfc(math.sqrt(r["logrank_chi2"][fold] / 2))) < 1e-15
            # the same problem alone: a problem's result does not depend on its batch
            W, thr, info = fit_cox(X_dev, t, e, [splits[fold]], cost=co["cost"])
            table, n_train = _table([splits[fold]])
            c, chi2, counts = F.survival_metrics(_scores(X_dev, W), t.float().to(DEV), e.to(torch.int32).to(DEV), table, n_train, thr)
            assert r["c_index"][fold] == float(c[0]) and r["logrank_chi2"][fold] == float(chi2[0])
            assert r["threshold"][fold] == float(thr[0]) and r["counts"][fold].tolist() == counts[0].tolist() and bool(info["converged"][0])
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            again = survival_probe(X_dev, times, events, folds=3, repeats=2, cost=co["cost"])
        finally:
            torch.cuda.set_sync_debug_mode(mode)
    syncs = [str(w.message) for w in seen if "called a synchronizing" in str(w.message)]      # one warning per host wait
    assert len(syncs) == 2, syncs                     # the finiteness check and the one read of the results
    assert all(np.array_equal(again[k][m], res[k][m]) for k in res for m in res[k])
