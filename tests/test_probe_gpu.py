"""The few-shot linear probe on the device (mdl_probe_fit / _scores / _metrics, madeleine_amd.probe) against an fp64 Newton reference on
the CPU (tests/_probe_ref.py) over four closed-form cohorts: A (S 160, d 64, C 2), B (S 160, d 48 with ldX 56, C 3), C2 and C4 (S 240,
d 512, C 2 / 4), each with k in (1, 10, 25) and folds 0..3 -- 2 to 100 training rows.

Figures measured on the MI355X at the default gtol = 1e-4 are in test_decision_values' docstring; every test prints its own."""
import functools
import math
import warnings

import numpy as np
import pytest
import torch

from tests import _probe_ref as R

pytestmark = pytest.mark.gpu
GTOL = 1e-4
DEV = "cuda"


def _table(idx_lists):
    from madeleine_amd.probe import _problem_table
    return _problem_table(idx_lists, DEV)


def _device_X(X, ldX):
    """X [S, d] fp32 on the device as a view of a [S, ldX] buffer (NaN in the padding columns: they are never read)."""
    S, d = X.shape
    buf = torch.full((S, ldX), float("nan"), dtype=torch.float32, device=DEV)
    buf[:, :d] = X.float().to(DEV)
    return buf[:, :d]


def _run(X_dev, y, idx_lists, C, **kw):
    """Fit, scores and metrics of a problem list in one launch sequence each; everything back on the host."""
    from madeleine_amd import functional as F
    table, n_train = _table(idx_lists)
    y_dev = y.to(torch.int32).to(DEV)
    W, b, info = F.probe_fit(X_dev, y_dev, table, n_train, C, gtol=GTOL, **kw)
    z = F.probe_scores(X_dev, W, b, C)
    conf, auc = F.probe_metrics(z, y_dev, table, n_train, C)
    torch.cuda.synchronize()
    return dict(W=W.cpu(), b=b.cpu(), info=info.cpu(), z=z.cpu(), conf=conf.cpu(), auc=auc.cpu())


@functools.lru_cache(maxsize=None)
def _cohort_run(name):
    co = R.cohort(name)
    return co, _run(_device_X(co["X"], co["ldX"]), co["y"], [p["idx"] for p in co["problems"]], co["C"])


def _margin(z64, C):
    if C == 2:
        return z64[:, 0].abs()
    top = z64.topk(2, dim=1).values
    return top[:, 0] - top[:, 1]


@pytest.mark.parametrize("name", list(R.COHORTS))
def test_optimality(name):
    """Every problem converges, and the fp64 gradient of the primal objective at the returned (W, b) is within max(2 gtol, 2 r32):
    the stop rule plus the kernel's own fp32 evaluation error, or twice what the reference algorithm reaches in fp32."""
    _optimality(name, *_cohort_run(name))


def _optimality(name, co, out):
    X32 = co["X"].float()
    worst = 0.0
    for p, pr in enumerate(co["problems"]):
        g = R.primal_grad_inf(X32[pr["idx"]], co["y"][pr["idx"]], out["W"][p], out["b"][p], co["C"])
        bound = max(2 * GTOL, 2 * pr["r32"])
        worst = max(worst, g / bound)
        print("%s k=%d fold=%d: steps %d cg %d residual %.2e (kernel) %.2e (fp64) r32 %.2e" % (
            name, pr["k"], pr["fold"], out["info"][p, 0], out["info"][p, 3], out["info"][p, 2], g, pr["r32"]))
        assert out["info"][p, 1] == 1, (name, pr["k"], pr["fold"], out["info"][p])
        assert g <= bound, (name, pr["k"], pr["fold"], g, bound)
    print("%s worst gradient / bound %.3f" % (name, worst))


@pytest.mark.parametrize("name", list(R.COHORTS))
def test_decision_values(name):
    """E_p = max_S |z - z64| / max_S |z64| <= 1e-3 (the project's parity contract) for every problem.
    Worst E_p measured on the MI355X: A 2.6e-6, B 1.2e-5, C2 7.5e-6, C4 3.3e-5."""
    _decision_values(name, *_cohort_run(name))


def _decision_values(name, co, out):
    worst = 0.0
    for p, pr in enumerate(co["problems"]):
        E = float((out["z"][p].double() - pr["z64"]).abs().max() / pr["z64"].abs().max())
        worst = max(worst, E)
        assert E <= 1e-3, (name, pr["k"], pr["fold"], E)
    print("%s worst E_p %.2e" % (name, worst))


@pytest.mark.parametrize("name", list(R.COHORTS))
def test_metrics_against_fp64_optimum(name):
    """With D = max_S |z - z64|: the confusion matrix differs from the fp64 one in at most as many test cases as have an fp64 margin
    below 2 D (never more than 4 % of them), and the AUC by at most the share of (positive, negative) pairs whose fp64 score gap is below
    2 D, plus 1e-6 for the fp32 format of auc_out."""
    _metrics_against_fp64_optimum(name, *_cohort_run(name))


def _metrics_against_fp64_optimum(name, co, out):
    C, y = co["C"], co["y"]
    for p, pr in enumerate(co["problems"]):
        test = R.test_mask(y.clone(), pr["idx"])
        D = float((out["z"][p].double() - pr["z64"]).abs().max())
        close = int((_margin(pr["z64"], C)[test] < 2 * D).sum())
        assert close <= 0.04 * int(test.sum()), (name, pr["k"], pr["fold"], close)
        moved = int((out["conf"][p].long() - R.confusion(pr["z64"], y, test, C)).abs().sum()) // 2
        assert moved <= close, (name, pr["k"], pr["fold"], moved, close)
        if C == 2:
            share = R.close_pair_share(pr["z64"][:, 0], test & (y == 1), test & (y == 0), 2 * D)
        else:
            ls = torch.log_softmax(pr["z64"], 1)
            share = sum(R.close_pair_share(ls[:, c], test & (y == c), test & (y != c), 2 * D) for c in range(C)) / C
        ref = R.auc(pr["z64"], y, test, C)
        assert abs(float(out["auc"][p]) - ref) <= share + 1e-6, (name, pr["k"], pr["fold"], float(out["auc"][p]), ref, share)


def _hand_cases():
    """(name, z [S, cols], y [S], train indices, C) of the hand-made score sets."""
    f = lambda *v: torch.tensor(v, dtype=torch.float32)[:, None]
    i = lambda *v: torch.tensor(v, dtype=torch.int64)
    cases = [
        ("ties", f(0.5, 0.5, -1, 2, 2, 0.5, 3, -1, 0.25, 2), i(1, 0, 0, 1, 0, 1, 1, 1, 0, 0), i(), 2),
        ("all equal", f(*[0.75] * 9), i(1, 0, 0, 1, 0, 1, 1, 0, 0), i(), 2),
        ("positives only in training", f(1, -1, 2, 0.5, -2, 3), i(0, 0, 1, 0, 0, 1), i(2, 5), 2),
        ("negatives absent", f(1, -1, 2), i(1, 1, 1), i(), 2),
        ("z == 0 is class 0", f(0, -0.0, 1e-30, -1e-30, 0, 0), i(1, 0, 1, 0, 0, 1), i(), 2),
        ("unlabeled and training cases", f(3, -3, 1, 1, -1, 2, 0.5, 0.5, 4, -4), i(1, 0, -1, 1, -1, 0, 1, 0, 0, 1), i(0, 1, 8), 2),
    ]
    z3 = torch.tensor([[1, 1, 0], [0, 2, 2], [3, 3, 3], [0, 0, 1], [1, 1, 0], [0, 2, 2], [-1, 0, -1], [2, 1, 2], [3, 3, 3], [5, 0, 0]],
                      dtype=torch.float32)
    cases += [
        ("argmax ties and duplicate rows", z3, i(0, 1, 2, 2, 1, 2, 1, 0, 0, 1), i(), 3),
        ("multiclass all equal", torch.ones(7, 3), i(0, 1, 2, 0, 1, 2, 0), i(), 3),
        ("multiclass class absent from the test set", z3, i(0, 1, 2, 0, 1, 0, 1, 0, 0, 1), i(2), 3),
        ("multiclass unlabeled and training cases", z3, i(0, 1, 2, -1, 1, 2, 1, -1, 0, 1), i(0, 4), 3),
    ]
    return cases


@pytest.mark.parametrize("case", _hand_cases(), ids=lambda c: c[0])
def test_metrics_kernel_on_hand_made_scores(case):
    """Exact ties count 1/2, all scores equal give 0.5, a class without a test case gives NaN, z == 0 is class 0, argmax ties go to the
    lowest index, unlabeled and training cases are left out -- against an fp64 pair count on the host."""
    from madeleine_amd import functional as F
    _, z, y, train, C = case
    table, n_train = _table([train]) if train.numel() else (torch.full((1, 1), -1, dtype=torch.int32, device=DEV),
                                                           torch.zeros(1, dtype=torch.int32, device=DEV))
    conf, auc = F.probe_metrics(z[None].contiguous().to(DEV), y.to(torch.int32).to(DEV), table, n_train, C)
    test = R.test_mask(y.clone(), train)
    assert torch.equal(conf[0].cpu().long(), R.confusion(z.double(), y, test, C))
    ref, got = R.auc(z.double(), y, test, C), float(auc[0])
    assert (math.isnan(ref) and math.isnan(got)) or abs(got - ref) <= 1e-6, (got, ref)


def test_metrics_consistent_with_device_scores():
    """Confusion matrix and AUC of cohort B equal the host's fp64 recount from the device's own decision values."""
    co, out = _cohort_run("B")
    for p, pr in enumerate(co["problems"]):
        test = R.test_mask(co["y"].clone(), pr["idx"])
        assert torch.equal(out["conf"][p].long(), R.confusion(out["z"][p].double(), co["y"], test, co["C"]))
        assert abs(float(out["auc"][p]) - R.auc(out["z"][p].double(), co["y"], test, co["C"])) <= 1e-6


def _check_fit(X, y, idx_lists, C, out):
    """Converged, and the fp64 gradient within 2 gtol (stop rule + fp32 evaluation), for every problem of a run."""
    for p, idx in enumerate(idx_lists):
        g = R.primal_grad_inf(X.float()[idx], y[idx], out["W"][p], out["b"][p], C)
        assert out["info"][p, 1] == 1 and g <= 2 * GTOL, (p, out["info"][p], g)
        test = R.test_mask(y.clone(), idx)
        assert torch.equal(out["conf"][p].long(), R.confusion(out["z"][p].double(), y, test, C))


def test_largest_fit():
    """n = 256 training rows exactly (C 8, k 32), more rows than dimensions."""
    from madeleine_amd.probe import probe_splits
    X, y = R.recipe(320, 64, 8, 0.2)
    idx = [probe_splits(y, 32, 0)]
    assert idx[0].numel() == 256
    out = _run(_device_X(X, 64), y, idx, 8)
    print("largest fit: steps %d cg %d residual %.2e" % (out["info"][0, 0], out["info"][0, 3], out["info"][0, 2]))
    _check_fit(X, y, idx, 8, out)


def test_smallest_fit():
    """C 2, k 1, d 1, P 1."""
    from madeleine_amd.probe import probe_splits
    X, y = R.recipe(24, 1, 2, 0.5)
    idx = [probe_splits(y, 1, 0)]
    out = _run(_device_X(X, 1), y, idx, 2)
    _check_fit(X, y, idx, 2, out)
    W64, b64, _, _ = R.newton_fit(X.float()[idx[0]].double(), y[idx[0]], 2)
    z64 = X.float().double() @ W64.T + b64
    assert float((out["z"][0].double() - z64).abs().max() / z64.abs().max()) <= 1e-3


def _bits_equal(a, b, p, q):
    return all(torch.equal(a[k][p].view(torch.int32) if a[k].dtype == torch.float32 else a[k][p],
                           b[k][q].view(torch.int32) if b[k].dtype == torch.float32 else b[k][q]) for k in a)


def test_mixed_sizes_independence_and_reproducibility():
    """One launch over 36 problems of different n_train (train_idx padded with -1): every problem converges; a problem solved alone
    gives the same bits as inside the batch; a second run gives the same bits."""
    from madeleine_amd.probe import probe_splits
    co = R.cohort("A")
    X_dev = _device_X(co["X"], co["ldX"])
    idx = [probe_splits(co["y"], k, fold) for fold in range(12) for k in R.KS]
    assert len(idx) == 36 and {t.numel() for t in idx} == {2, 20, 50}
    batch = _run(X_dev, co["y"], idx, 2)
    _check_fit(co["X"], co["y"], idx, 2, batch)
    again = _run(X_dev, co["y"], idx, 2)
    assert all(_bits_equal(batch, again, p, p) for p in range(36))
    for p in (0, 17, 34):
        alone = _run(X_dev, co["y"], [idx[p]], 2)
        assert _bits_equal(batch, alone, p, 0), p


def test_nan_prefilled_buffers_and_side_stream():
    """Outputs and workspaces pre-filled with NaN change nothing, and the launches follow the current (non-default) stream."""
    from madeleine_amd import functional as F
    co, ref = _cohort_run("B")
    C, X_dev = co["C"], _device_X(co["X"], co["ldX"])
    table, n_train = _table([p["idx"] for p in co["problems"]])
    y_dev = co["y"].to(torch.int32).to(DEV)
    P, S, d = table.shape[0], X_dev.shape[0], X_dev.shape[1]
    nan = lambda *shape: torch.full(shape, float("nan"), device=DEV)
    ws_fit = torch.full((F._entry("mdl_probe_fit_ws_bytes")(P, table.shape[1], d, C),), 0xFF, dtype=torch.uint8, device=DEV)
    ws_met = torch.full((F._entry("mdl_probe_metrics_ws_bytes")(P, S, C),), 0xFF, dtype=torch.uint8, device=DEV)
    W, b, info, z, auc = nan(P, C, d), nan(P, C), nan(P, 4), nan(P, S, C), nan(P)
    conf = torch.full((P, C, C), -7, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        F._call("mdl_probe_fit", X_dev, X_dev.stride(0), S, d, y_dev, 0, table, n_train, P, table.shape[1], C, 1.0, GTOL, 100, W, b, info,
                ws_fit, F._stream())
        F._call("mdl_probe_scores", X_dev, X_dev.stride(0), S, d, W, b, P, C, z, F._stream())
        F._call("mdl_probe_metrics", z, y_dev, 0, table, n_train, P, table.shape[1], S, C, conf, auc, ws_met, F._stream())
    side.synchronize()
    got = dict(W=W.cpu(), b=b.cpu(), info=info.cpu(), z=z.cpu(), conf=conf.cpu(), auc=auc.cpu())
    assert all(_bits_equal(ref, got, p, p) for p in range(P))


def test_linear_probe_end_to_end():
    """Two tasks over cohort A (the second with every fifth case unlabeled): keys, shapes, and bacc / q_kappa against the fp64 host
    formulae on the returned confusion matrices; AUC and confusion matrix equal to those of the same problems in another batch."""
    from madeleine_amd import linear_probe
    co, batch = _cohort_run("A")
    y2 = co["y"].clone()
    y2[::5] = -1
    with warnings.catch_warnings():
        warnings.simplefilter("error")               # every fit converges: no RuntimeWarning
        res = linear_probe(co["X"].float().numpy(), {"t": co["y"].numpy(), "u": y2}, ks=(1, 10), folds=3, kappa=True)
    assert set(res) == {("t", 1), ("t", 10), ("u", 1), ("u", 10)}
    for (task, k), r in res.items():
        y = co["y"] if task == "t" else y2
        assert set(r) == {"auc", "bacc", "q_kappa", "converged", "confusion"}
        assert r["auc"].shape == r["bacc"].shape == r["q_kappa"].shape == r["converged"].shape == (3,) and r["converged"].all()
        assert r["confusion"].shape == (3, 2, 2)
        for fold in range(3):
            cm = r["confusion"][fold].astype(np.float64)
            assert cm.sum() == int((y >= 0).sum()) - 2 * k
            rec = [cm[c, c] / cm[c].sum() for c in range(2)]
            assert abs(r["bacc"][fold] - sum(rec) / 2) < 1e-12
            po, pe = (cm[0, 0] + cm[1, 1]) / cm.sum(), (cm.sum(1) * cm.sum(0)).sum() / cm.sum() ** 2
            assert abs(r["q_kappa"][fold] - (po - pe) / (1 - pe)) < 1e-12      # two grades: quadratic weights are 0 / 1
            assert 0.0 <= r["auc"][fold] <= 1.0
            if task == "t":      # the same split as problem (k, fold) of the cohort's batch: a problem's result does not depend on its batch
                p = [i for i, pr in enumerate(co["problems"]) if (pr["k"], pr["fold"]) == (k, fold)][0]
                assert r["auc"][fold] == float(batch["auc"][p]) and np.array_equal(r["confusion"][fold], batch["conf"][p].numpy())


def test_refusals():
    from madeleine_amd import functional as F
    from madeleine_amd import fit_logistic, linear_probe
    X = torch.zeros(600, 4, device=DEV)
    y = torch.zeros(600, dtype=torch.int32, device=DEV)
    one = torch.ones(1, dtype=torch.int32, device=DEV)
    with pytest.raises(NotImplementedError):
        F.probe_fit(X, y, torch.zeros(1, 257, dtype=torch.int32, device=DEV), one, 2)
    with pytest.raises(NotImplementedError):
        F.probe_fit(X, y, torch.zeros(1, 4, dtype=torch.int32, device=DEV), one, 9)
    with pytest.raises(NotImplementedError):
        F.probe_metrics(torch.zeros(1, 16385, 1, device=DEV), torch.zeros(16385, dtype=torch.int32, device=DEV),
                        torch.zeros(1, 4, dtype=torch.int32, device=DEV), one, 2)
    with pytest.raises(RuntimeError):
        F.probe_fit(X.cpu(), y, torch.zeros(1, 4, dtype=torch.int32, device=DEV), one, 2)
    with pytest.raises(RuntimeError):
        fit_logistic(X.cpu(), y.cpu(), [torch.tensor([0, 1])], 2)
    bad = torch.zeros(8, 4)
    bad[3, 1] = float("inf")
    with pytest.raises(ValueError):
        linear_probe(bad, torch.tensor([0, 1] * 4), ks=(1,), folds=1)
