"""The full-label linear probe on the device (mdl_logit_fit / mdl_probe_scores / mdl_logit_metrics, madeleine_amd.probe.linear_probe_cv)
against an fp64 Newton reference on the CPU (tests/_probe_cv_ref.py) over five closed-form cohorts with every 17th case unlabeled and
the five default folds of cv_splits: FA (S 400, d 24 in ldX 40, C 2), FB (S 400, d 70 in ldX 72, C 3), FC2 (S 1300, d 512, C 2), FC4
(S 900, d 256, C 4), FC8 (S 650, d 96, C 8) -- 300 to 979 training rows.

Figures measured on the MI355X at the default gtol = 1e-4 are in test_decision_values' docstring; every test prints its own."""
import functools
import math
import warnings

import numpy as np
import pytest
import torch

from tests import _probe_cv_ref as V
from tests import _probe_ref as R

pytestmark = pytest.mark.gpu
GTOL = V.GTOL
DEV = "cuda"
EDGE_N = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
# name -> (S, d, sep, ldX) of the matrices of the size-edge tests; FA's is the cohort's own
EDGE_MATRICES = {"FA": (400, 24, 0.15, 40), "d1": (1300, 1, 0.5, 3), "d1024": (1300, 1024, 0.1, 1024)}


def _table(idx_lists):
    from madeleine_amd.probe import _problem_table
    return _problem_table(idx_lists, DEV)


def _device_X(X, ldX):
    """X [S, d] fp32 on the device as a view of a [S, ldX] buffer (NaN in the padding columns: they are never read)."""
    S, d = X.shape
    buf = torch.full((S, ldX), float("nan"), dtype=torch.float32, device=DEV)
    buf[:, :d] = X.float().to(DEV)
    return buf[:, :d]


def _finish(W, b, info, z, conf, auc):
    torch.cuda.synchronize()
    return dict(W=W.cpu(), b=b.cpu(), info=info.cpu(), z=z.cpu(), conf=conf.cpu(), auc=auc.cpu())


def _run(X_dev, y, idx_lists, C, fit="logit_fit", **kw):
    """Fit, scores and metrics of a problem list in one launch sequence each; everything back on the host."""
    from madeleine_amd import functional as F
    table, n_train = _table(idx_lists)
    y_dev = y.to(torch.int32).to(DEV)
    W, b, info = getattr(F, fit)(X_dev, y_dev, table, n_train, C, gtol=GTOL, **kw)
    z = F.probe_scores(X_dev, W, b, C)
    conf, auc = F.logit_metrics(z, y_dev, table, n_train, C)
    return _finish(W, b, info, z, conf, auc)


@functools.lru_cache(maxsize=None)
def _cohort_run(name):
    co = V.cohort(name)
    return co, _run(_device_X(co["X"], co["ldX"]), co["y"], [p["idx"] for p in co["problems"]], co["C"])


def _margin(z64, C):
    if C == 2:
        return z64[:, 0].abs()
    top = z64.topk(2, dim=1).values
    return top[:, 0] - top[:, 1]


def _E(z, z64):
    return float((z.double() - z64).abs().max() / z64.abs().max())


@pytest.mark.parametrize("name", list(V.COHORTS))
def test_optimality(name):
    """Every fold converges, and the fp64 gradient of the primal objective at the returned (W, b) is within max(2 gtol, 2 r32): the stop
    rule plus the kernel's own fp32 evaluation error, or twice what the same algorithm reaches in fp32 on the host."""
    _optimality(name, *_cohort_run(name))


def _optimality(name, co, out):
    X32 = co["X"].float()
    worst = 0.0
    for p, pr in enumerate(co["problems"]):
        g = R.primal_grad_inf(X32[pr["idx"]], co["y"][pr["idx"]], out["W"][p], out["b"][p], co["C"])
        bound = max(2 * GTOL, 2 * pr["r32"])
        worst = max(worst, g / bound)
        print("%s fold=%d n=%d: steps %d cg %d residual %.2e (kernel) %.2e (fp64) r32 %.2e" % (
            name, pr["fold"], pr["idx"].numel(), out["info"][p, 0], out["info"][p, 3], out["info"][p, 2], g, pr["r32"]))
        assert out["info"][p, 1] == 1, (name, pr["fold"], out["info"][p])
        assert g <= bound, (name, pr["fold"], g, bound)
    print("%s worst gradient / bound %.3f" % (name, worst))


@pytest.mark.parametrize("name", list(V.COHORTS))
def test_decision_values(name):
    """E_p = max_S |z - z64| / max_S |z64| <= 1e-3 (the project's parity contract) for every fold.
    Worst E_p measured on the MI355X: FA 1.7e-7, FB 3.0e-6, FC2 3.2e-7, FC4 1.5e-6, FC8 4.6e-6 (5 to 12 Newton and 40 to 354 CG steps per
    binary fit, 6 to 11 and 82 to 732 per multinomial fit)."""
    _decision_values(name, *_cohort_run(name))


def _decision_values(name, co, out):
    worst = 0.0
    for p, pr in enumerate(co["problems"]):
        E = _E(out["z"][p], pr["z64"])
        worst = max(worst, E)
        assert E <= 1e-3, (name, pr["fold"], E)
    print("%s worst E_p %.2e" % (name, worst))


def _check_metrics(name, fold, C, y, idx, z, z64, conf, auc):
    """The rule of test_probe_gpu.test_metrics_against_fp64_optimum; returns (test cases, close cases)."""
    test = R.test_mask(y.clone(), idx)
    D = float((z.double() - z64).abs().max())
    close = int((_margin(z64, C)[test] < 2 * D).sum())
    assert close <= 0.04 * int(test.sum()), (name, fold, close)
    moved = int((conf.long() - R.confusion(z64, y, test, C)).abs().sum()) // 2
    assert moved <= close, (name, fold, moved, close)
    if C == 2:
        share = R.close_pair_share(z64[:, 0], test & (y == 1), test & (y == 0), 2 * D)
    else:
        ls = torch.log_softmax(z64, 1)
        share = sum(R.close_pair_share(ls[:, c], test & (y == c), test & (y != c) & (y >= 0), 2 * D) for c in range(C)) / C
    ref = R.auc(z64, y, test, C)
    assert abs(float(auc) - ref) <= share + 1e-6, (name, fold, float(auc), ref, share)
    return int(test.sum()), close


@pytest.mark.parametrize("name", list(V.COHORTS))
def test_metrics_against_fp64_optimum(name):
    """With D = max_S |z - z64|: the confusion matrix differs from the fp64 one in at most as many test cases as have an fp64 margin
    below 2 D (never more than 4 % of them), and the AUC by at most the share of (positive, negative) pairs whose fp64 score gap is below
    2 D, plus 1e-6 for the fp32 format of auc_out."""
    _metrics_against_fp64_optimum(name, *_cohort_run(name))


def _metrics_against_fp64_optimum(name, co, out):
    for p, pr in enumerate(co["problems"]):
        n_test, close = _check_metrics(name, pr["fold"], co["C"], co["y"], pr["idx"], out["z"][p], pr["z64"], out["conf"][p], out["auc"][p])
        print("%s fold=%d: %d test cases, %d within 2 D of the boundary" % (name, pr["fold"], n_test, close))


@pytest.mark.parametrize("name", list(V.COHORTS))
def test_metrics_consistent_with_device_scores(name):
    """Confusion matrix and AUC equal the host's fp64 recount from the device's own decision values."""
    co, out = _cohort_run(name)
    for p, pr in enumerate(co["problems"]):
        test = R.test_mask(co["y"].clone(), pr["idx"])
        assert torch.equal(out["conf"][p].long(), R.confusion(out["z"][p].double(), co["y"], test, co["C"]))
        assert abs(float(out["auc"][p]) - R.auc(out["z"][p].double(), co["y"], test, co["C"])) <= 1e-6


# ---- size edges ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _edge_problem(matrix, C):
    """(X fp64, y, ldX, [training indices of EDGE_N]): the first n labeled cases, going round again where the matrix has fewer (a case
    listed twice counts twice, in the kernel and in the reference alike).  Labels: the recipe's formula for C classes."""
    S, d, sep, ldX = EDGE_MATRICES[matrix]
    X, _ = V.recipe(S, d, 2, sep)
    _, y = V.recipe(S, 1, C, sep)
    labeled = torch.nonzero(y >= 0)[:, 0]
    return X, y, ldX, [labeled[torch.arange(n) % labeled.numel()] for n in EDGE_N]


@functools.lru_cache(maxsize=None)
def _edge_run(matrix, C, fit="logit_fit"):
    X, y, ldX, idx = _edge_problem(matrix, C)
    if fit == "probe_fit":
        idx = [t for t in idx if t.numel() <= 256]
    return _run(_device_X(X, ldX), y, idx, C, fit=fit)


@pytest.mark.parametrize("n", EDGE_N)
@pytest.mark.parametrize("C", (2, 3))
@pytest.mark.parametrize("matrix", list(EDGE_MATRICES))
def test_size_edges(matrix, C, n):
    """logit_fit at the row counts on both sides of the wave's row group, the workgroup and the few-shot limit, at d = 1, 24 and 1024:
    converged, fp64 gradient within max(2 gtol, 2 r32), E <= 1e-3.  n = 1 is the exception for E: with one class and a free intercept
    the objective has no minimiser (b runs to infinity), so there is no z64; the fit still has to reach the gradient bound.
    At n <= 256 the few-shot path meets E <= 1e-3 against the same z64.
    Measured on the MI355X: worst E 5.8e-5 (d 1024, C 3, n 64), few-shot 1.3e-4 at the same problem; all others below 1e-5 / 4e-5."""
    X, y, _, idx = _edge_problem(matrix, C)
    p = EDGE_N.index(n)
    out = _edge_run(matrix, C)
    X32, t = X.float(), idx[p]
    g = R.primal_grad_inf(X32[t], y[t], out["W"][p], out["b"][p], C)
    print("%s C=%d n=%d: steps %d cg %d residual %.2e (kernel) %.2e (fp64)" % (matrix, C, n, out["info"][p, 0], out["info"][p, 3],
                                                                             out["info"][p, 2], g))
    assert out["info"][p, 1] == 1, (matrix, C, n, out["info"][p])
    if n == 1:
        assert g <= 2 * GTOL, (matrix, C, n, g)
        return
    ref = V.reference(X32, y, t, C)
    assert g <= max(2 * GTOL, 2 * ref["r32"]), (matrix, C, n, g, ref["r32"])
    E = _E(out["z"][p], ref["z64"])
    print("%s C=%d n=%d: E %.2e" % (matrix, C, n, E))
    assert E <= 1e-3, (matrix, C, n, E)
    if n <= 256:
        few = _edge_run(matrix, C, "probe_fit")
        E_few = _E(few["z"][p], ref["z64"])
        print("%s C=%d n=%d: few-shot E %.2e" % (matrix, C, n, E_few))
        assert E_few <= 1e-3, (matrix, C, n, E_few)


def test_routing():
    """fit_logistic gives probe_fit's bits at a 256-wide table and logit_fit's at a 257-wide one."""
    from madeleine_amd import fit_logistic, functional as F
    X, y, ldX, idx = _edge_problem("FA", 2)
    X_dev, y_dev = _device_X(X, ldX), y.to(torch.int32).to(DEV)
    for width, fit in ((256, F.probe_fit), (257, F.logit_fit)):
        lists = [idx[EDGE_N.index(width)], idx[EDGE_N.index(65)]]
        table, n_train = _table(lists)
        assert table.shape[1] == width
        W, b, info = fit(X_dev, y_dev, table, n_train, 2, gtol=GTOL)
        for arg in (lists, table):
            W2, b2, info2 = fit_logistic(X_dev, y, arg, 2, gtol=GTOL)
            assert torch.equal(W2.view(torch.int32), W.view(torch.int32)) and torch.equal(b2.view(torch.int32), b.view(torch.int32))
            assert torch.equal(info2["iterations"], info[:, 0]) and torch.equal(info2["cg_iterations"], info[:, 3])
            assert torch.equal(info2["residual"], info[:, 2]) and bool(info2["converged"].all())


def test_largest_fit():
    """One binary problem of 13,107 training rows out of S = 16,384 (one fold of five of the largest cohort the metrics accept), d 64:
    converged, the fp64 gradient within max(2 gtol, 2 r32), the confusion matrix equal to the host's recount."""
    from madeleine_amd.probe import cv_splits
    X, y = R.recipe(16384, 64, 2, 0.05)
    idx = cv_splits(y)[0]
    assert idx.numel() == 13107
    out = _run(_device_X(X, 64), y, [idx], 2)
    X32 = X.float()
    g = R.primal_grad_inf(X32[idx], y[idx], out["W"][0], out["b"][0], 2)
    W32, b32, _, _ = V.newton_cg32(X32[idx], y[idx], 2)
    r32 = R.primal_grad_inf(X32[idx], y[idx], W32, b32, 2)
    print("largest fit: steps %d cg %d residual %.2e (kernel) %.2e (fp64) r32 %.2e" % (out["info"][0, 0], out["info"][0, 3],
                                                                                      out["info"][0, 2], g, r32))
    assert out["info"][0, 1] == 1 and g <= max(2 * GTOL, 2 * r32), (out["info"][0], g, r32)
    test = R.test_mask(y.clone(), idx)
    assert torch.equal(out["conf"][0].long(), R.confusion(out["z"][0].double(), y, test, 2))
    W64, b64 = V.newton64(X32[idx], y[idx], 2)
    E = _E(out["z"][0], X32.double() @ W64.T + b64)
    print("largest fit: E %.2e" % E)
    assert E <= 1e-3


def test_widest_fit():
    """d = 1024 with eight classes -- the widest vectors the kernel holds (64 KiB of LDS, every register) -- on 120 training rows."""
    X, y = V.recipe(300, 1024, 8, 0.3)
    idx = torch.nonzero(y >= 0)[:120, 0]
    out = _run(_device_X(X, 1024), y, [idx], 8)
    ref = V.reference(X.float(), y, idx, 8)
    g = R.primal_grad_inf(X.float()[idx], y[idx], out["W"][0], out["b"][0], 8)
    E = _E(out["z"][0], ref["z64"])
    print("widest fit: steps %d cg %d residual %.2e (kernel) %.2e (fp64) r32 %.2e E %.2e" % (
        out["info"][0, 0], out["info"][0, 3], out["info"][0, 2], g, ref["r32"], E))
    assert out["info"][0, 1] == 1 and g <= max(2 * GTOL, 2 * ref["r32"]) and E <= 1e-3


def _bits_equal(a, b, p, q):
    return all(torch.equal(a[k][p].view(torch.int32) if a[k].dtype == torch.float32 else a[k][p],
                           b[k][q].view(torch.int32) if b[k].dtype == torch.float32 else b[k][q]) for k in a)


def test_independence_and_reproducibility():
    """Problems of 1, 257, 489 and 978 training rows in one call (train_idx padded with -1) give the same bits as each problem alone,
    as the same problems in the reverse order, and as a second call."""
    co = V.cohort("FC2")
    X_dev = _device_X(co["X"], co["ldX"])
    full = co["problems"][0]["idx"]
    assert full.numel() == 978
    idx = [full[:1], full[:257], full[::2], full]
    assert [t.numel() for t in idx] == [1, 257, 489, 978]
    batch = _run(X_dev, co["y"], idx, 2)
    assert bool((batch["info"][:, 1] == 1).all())
    again = _run(X_dev, co["y"], idx, 2)
    assert all(_bits_equal(batch, again, p, p) for p in range(4))
    rev = _run(X_dev, co["y"], idx[::-1], 2)
    assert all(_bits_equal(batch, rev, p, 3 - p) for p in range(4))
    for p in range(4):
        alone = _run(X_dev, co["y"], [idx[p]], 2)
        assert _bits_equal(batch, alone, p, 0), p
    _, ref = _cohort_run("FC2")                      # the 978-row problem is fold 0 of the cohort's own batch of five
    assert _bits_equal(batch, ref, 3, 0)


def test_nan_prefilled_buffers_and_side_stream():
    """Outputs pre-filled with NaN and workspaces with 0xFF change nothing, and the launches follow the current (non-default) stream.
    The padding columns of X hold NaN (cohort FB sits in ldX 72)."""
    from madeleine_amd import functional as F
    co, ref = _cohort_run("FB")
    C, X_dev = co["C"], _device_X(co["X"], co["ldX"])
    table, n_train = _table([p["idx"] for p in co["problems"]])
    y_dev = co["y"].to(torch.int32).to(DEV)
    P, S, d = table.shape[0], X_dev.shape[0], X_dev.shape[1]
    nan = lambda *shape: torch.full(shape, float("nan"), device=DEV)
    ws_fit = torch.full((F._entry("mdl_logit_fit_ws_bytes")(P, table.shape[1], d, C),), 0xFF, dtype=torch.uint8, device=DEV)
    ws_met = torch.full((F._entry("mdl_logit_metrics_ws_bytes")(P, S, C),), 0xFF, dtype=torch.uint8, device=DEV)
    W, b, info, z, auc = nan(P, C, d), nan(P, C), nan(P, 4), nan(P, S, C), nan(P)
    conf = torch.full((P, C, C), -7, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        F._call("mdl_logit_fit", X_dev, X_dev.stride(0), S, d, y_dev, 0, table, n_train, P, table.shape[1], C, 1.0, GTOL, 100, W, b, info,
                ws_fit, F._stream())
        F._call("mdl_probe_scores", X_dev, X_dev.stride(0), S, d, W, b, P, C, z, F._stream())
        F._call("mdl_logit_metrics", z, y_dev, 0, table, n_train, P, table.shape[1], S, C, conf, auc, ws_met, F._stream())
    side.synchronize()
    got = dict(W=W.cpu(), b=b.cpu(), info=info.cpu(), z=z.cpu(), conf=conf.cpu(), auc=auc.cpu())
    assert all(_bits_equal(ref, got, p, p) for p in range(P))


def test_refused_problems_leave_their_neighbours_alone():
    """A training index outside [0, S), an unlabeled training case and n_train = 0: NaN in W, b and the residual, converged = 0; the
    folds beside them keep the bits they have in the cohort's own batch."""
    from madeleine_amd import functional as F
    co, ref = _cohort_run("FB")
    C, y, S = co["C"], co["y"], co["X"].shape[0]
    X_dev = _device_X(co["X"], co["ldX"])
    good = [p["idx"] for p in co["problems"]]
    bad_index = good[1].clone()
    bad_index[150] = S
    bad_label = good[2].clone()
    bad_label[7] = 17                                # y[17] = -1
    assert int(y[17]) == -1
    table, n_train = _table([good[0], bad_index, good[3], bad_label, good[4][:1], good[4]])
    n_train[4] = 0
    y_dev = y.to(torch.int32).to(DEV)
    W, b, info = F.logit_fit(X_dev, y_dev, table, n_train, C, gtol=GTOL)
    torch.cuda.synchronize()
    W, b, info = W.cpu(), b.cpu(), info.cpu()
    for p in (1, 3, 4):
        assert bool(torch.isnan(W[p]).all()) and bool(torch.isnan(b[p]).all()) and math.isnan(float(info[p, 2]))
        assert info[p, 1] == 0 and info[p, 0] == 0 and info[p, 3] == 0
    for p, q in ((0, 0), (2, 3), (5, 4)):
        assert torch.equal(W[p].view(torch.int32), ref["W"][q].view(torch.int32)), p
        assert torch.equal(b[p].view(torch.int32), ref["b"][q].view(torch.int32)) and torch.equal(info[p], ref["info"][q]), p


@pytest.mark.parametrize("name", ("FB", "FC2"))
def test_linear_probe_cv_end_to_end(name, monkeypatch):
    """The protocol over a cohort and a second task (every fifth case unlabeled as well), two repeats: keys, shapes, bacc / q_kappa
    against the host formulae, two host reads; for the cohort's own task and repeat 0 -- the cohort's problems -- per-fold AUC and
    confusion matrix hold against the fp64 optimum by the rule above, and equal those of the cohort's own batch."""
    from madeleine_amd import linear_probe_cv
    from madeleine_amd.probe import balanced_accuracy, quadratic_kappa
    co, batch = _cohort_run(name)
    C, y = co["C"], co["y"]
    y2 = y.clone()
    y2[::5] = -1
    X_np = co["X"].float().numpy()
    reads = []
    for method in ("cpu", "item", "__bool__", "tolist", "numpy"):
        orig = getattr(torch.Tensor, method)

        def counted(self, *a, _orig=orig, _method=method, **kw):
            if self.is_cuda:
                reads.append(_method)
            return _orig(self, *a, **kw)

        monkeypatch.setattr(torch.Tensor, method, counted)
    with warnings.catch_warnings():
        warnings.simplefilter("error")               # every fit converges: no RuntimeWarning
        res = linear_probe_cv(X_np, {"t": y.numpy(), "u": y2}, repeats=2, kappa=True)
    monkeypatch.undo()
    assert sorted(reads) == ["__bool__", "cpu"], reads      # the finiteness check and the one read of the results
    assert set(res) == {("t", 0), ("t", 1), ("u", 0), ("u", 1)}
    for (task, repeat), r in res.items():
        labels = y if task == "t" else y2
        assert set(r) == {"auc", "bacc", "q_kappa", "converged", "confusion"}
        assert r["auc"].shape == r["bacc"].shape == r["q_kappa"].shape == r["converged"].shape == (5,) and r["converged"].all()
        assert r["confusion"].shape == (5, C, C) and r["confusion"].sum() == int((labels >= 0).sum())      # every labeled case held out once
        for fold in range(5):
            cm = r["confusion"][fold]
            assert abs(r["bacc"][fold] - balanced_accuracy(cm)) < 1e-12 and abs(r["q_kappa"][fold] - quadratic_kappa(cm)) < 1e-12
            rec = [cm[c, c] / cm[c].sum() for c in range(C)]
            assert abs(r["bacc"][fold] - sum(rec) / C) < 1e-12 and 0.0 <= r["auc"][fold] <= 1.0
    r = res[("t", 0)]
    for p, pr in enumerate(co["problems"]):
        assert r["auc"][p] == float(batch["auc"][p]) and np.array_equal(r["confusion"][p], batch["conf"][p].numpy())
        test = R.test_mask(y.clone(), pr["idx"])
        n_test, close = _check_metrics(name, p, C, y, pr["idx"], batch["z"][p], pr["z64"], torch.from_numpy(r["confusion"][p]),
                                       r["auc"][p])
        cm64 = R.confusion(pr["z64"], y, test, C).numpy()
        support = min(int(cm64[c].sum()) for c in range(C))
        assert abs(r["bacc"][p] - balanced_accuracy(cm64)) <= close / support + 1e-12, (name, p, r["bacc"][p], balanced_accuracy(cm64))


def test_refusals():
    from madeleine_amd import functional as F
    from madeleine_amd import fit_logistic
    y = torch.zeros(600, dtype=torch.int32, device=DEV)
    one = torch.ones(1, dtype=torch.int32, device=DEV)
    small = torch.zeros(1, 4, dtype=torch.int32, device=DEV)
    wide = torch.zeros(1, 16385, dtype=torch.int32, device=DEV)
    with pytest.raises(NotImplementedError):
        F.logit_fit(torch.zeros(600, 4, device=DEV), y, wide, one, 2)
    with pytest.raises(NotImplementedError):
        fit_logistic(torch.zeros(600, 4, device=DEV), y, wide, 2)
    with pytest.raises(NotImplementedError):
        F.logit_fit(torch.zeros(600, 1025, device=DEV), y, small, one, 2)
    with pytest.raises(NotImplementedError):
        F.logit_fit(torch.zeros(600, 4, device=DEV), y, small, one, 9)
    with pytest.raises(NotImplementedError):
        F.logit_metrics(torch.zeros(1, 600, 1, device=DEV), y, wide, one, 2)
    with pytest.raises(NotImplementedError):
        F.logit_metrics(torch.zeros(1, 16385, 1, device=DEV), torch.zeros(16385, dtype=torch.int32, device=DEV), small, one, 2)
    with pytest.raises(RuntimeError):
        F.logit_fit(torch.zeros(600, 4), y, small, one, 2)
