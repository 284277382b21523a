"""Host side of the regression probe (R1-R3, include/madeleine_amd_regress.h): the fifth header and its binding, the refusals that come
before any launch, regression_splits, and the numpy contract of tests/_regress_ref.py held to independent formulas, to scikit-learn and
scipy where they are installed, to seeded faults, and to the cap on what the fp32 storage of W, b and z may cost.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

from madeleine_amd import _build, _native
from tests import _regress_ref as R

P, I32, I64, F32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
FAKE = 1 << 20          # a 16-byte aligned address nothing dereferences: every refusal below comes before the first launch
ARG, UNSUP, ALIGN = (_native._DEFINES[k] for k in ("MDL_E_ARG", "MDL_E_UNSUPPORTED", "MDL_E_ALIGN"))
NAMES = {"mdl_ridge_fit_ws_bytes", "mdl_ridge_fit", "mdl_ridge_scores", "mdl_regress_metrics_ws_bytes", "mdl_regress_metrics"}


# ---- header and ABI ------------------------------------------------------------------------------------------------------------------
def test_the_fifth_header_parses_and_is_bound_beside_the_other_four():
    with open(_build.REGRESS_HEADER) as f:
        sigs, defines = _native._parse_header(f.read())
    assert sigs == _native.REGRESS_SIGNATURES and set(sigs) == NAMES and defines == _native.REGRESS_DEFINES
    assert sigs["mdl_ridge_fit_ws_bytes"] == (I64, [I64, I32, I32, I64, I32])
    assert sigs["mdl_ridge_fit"] == (I32, [P, I64, I64, I32, P, I64, I64, P, P, I64, I32, P, I32, P, P, P, P, P])
    assert sigs["mdl_ridge_scores"] == (I32, [P, I64, I64, I32, P, P, I64, P, P])
    assert sigs["mdl_regress_metrics_ws_bytes"] == (I64, [I64, I64, I64])
    assert sigs["mdl_regress_metrics"] == (I32, [P, P, I64, I64, P, P, I64, I32, I64, I32, P, P, P, P])
    assert defines == {"MDL_RIDGE_MAX_SYS": 1024, "MDL_RIDGE_MAX_TRAIN": 16384, "MDL_RIDGE_MAX_TARGETS": 4096, "MDL_RIDGE_MAX_ALPHAS": 16,
                       "MDL_REG_NTEST": 0, "MDL_REG_PEARSON": 1, "MDL_REG_SPEARMAN": 2, "MDL_REG_R2": 3, "MDL_REG_MAE": 4, "MDL_REG_RMSE": 5}
    lib = _native.lib()
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)                          # exported by the built library
        assert fn.restype is res and fn.argtypes == args, name
    others = (_native.SIGNATURES, _native.VIEW_SIGNATURES, _native.STATS_SIGNATURES, _native.EXPLAIN_SIGNATURES)
    assert not any(NAMES & set(o) for o in others)
    assert not any(set(defines) & set(o) for o in (_native._DEFINES, _native.VIEW_DEFINES, _native.STATS_DEFINES, _native.EXPLAIN_DEFINES))
    assert _build.REGRESS_HEADER in _build._deps()
    assert _native._DEFINES["MDL_PROBE_MAX_CASES"] == 16384      # the bound of S the int64 rank sums rest on


def test_a_header_that_repeats_a_name_is_refused():
    with open(_build.REGRESS_HEADER) as f:
        text = f.read()
    sigs, _ = _native._parse_header(text.replace("mdl_ridge_scores(", "mdl_probe_scores("))
    assert set(sigs) & set(_native.SIGNATURES)          # what the import-time check of _native looks for


def test_the_python_surface_is_exported():
    import madeleine_amd
    from madeleine_amd import functional as F, regress
    for name in ("regression_splits", "fit_ridge", "regression_probe"):
        assert name in madeleine_amd.__all__ and getattr(madeleine_amd, name) is getattr(regress, name)
    assert callable(F.ridge_fit) and callable(F.ridge_scores) and callable(F.regress_metrics)
    assert F.REG_COLUMNS == ("n_test", "pearson", "spearman", "r2", "mae", "rmse")


def test_no_cpu_fallback():
    from madeleine_amd import regress
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        regress.fit_ridge(torch.zeros(4, 2), torch.zeros(4), [torch.arange(3)], (1.0,))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            regress.regression_probe(torch.zeros(8, 2), {"y": np.zeros(8)})


def test_workspace_queries():
    fit, met = _native.lib().mdl_ridge_fit_ws_bytes, _native.lib().mdl_regress_metrics_ws_bytes
    for Pn, n_max, d, T, A in ((5, 922, 512, 1000, 8), (1, 1, 1, 1, 1), (5, 13108, 512, 1, 8), (3, 97, 77, 9, 3)):
        m = min(n_max, d)
        need = 8 * (Pn * d + Pn * T + Pn * m * m * (A + 1) + Pn * T * m) + 4 * (Pn + Pn * A)
        assert need <= fit(Pn, n_max, d, T, A) <= need + 8 * Pn * (A + 2) * (2 * m + 1) + 8 * Pn * T + 16 * 7 and fit(Pn, n_max, d, T, A) % 16 == 0
    assert fit(0, 5, 5, 1, 1) == ARG and fit(5, 0, 5, 1, 1) == ARG and fit(5, 5, 0, 1, 1) == ARG
    assert fit(5, 5, 5, 0, 1) == ARG and fit(5, 5, 5, 1, 0) == ARG
    assert fit(5, 1025, 1025, 1, 1) == UNSUP and fit(5, 16385, 8, 1, 1) == UNSUP and fit(5, 8, 8, 4097, 1) == UNSUP
    assert fit(5, 8, 8, 1, 17) == UNSUP and fit(1 << 31, 8, 8, 1, 1) == UNSUP
    assert fit(5, 16384, 1024, 1, 1) > 0 and fit(5, 1024, 1 << 20, 1, 1) > 0
    for Pn, S, T in ((5, 1153, 1000), (1, 1, 1), (5, 16384, 1)):
        need = Pn * S + 4 * Pn * T * S
        assert need <= met(Pn, S, T) <= need + 16 * Pn + 32 and met(Pn, S, T) % 16 == 0
    assert met(0, 5, 1) == ARG and met(5, 0, 1) == ARG and met(5, 5, 0) == ARG
    assert met(5, 16385, 1) == UNSUP and met(5, 5, 4097) == UNSUP and met(1 << 31, 5, 1) == UNSUP


# ---- refusals before any launch ------------------------------------------------------------------------------------------------------
def _fit(Pn=3, n_max=4, S=10, d=6, ldX=None, T=2, ldY=None, alphas=(1.0, 0.5), A=None, null=None, misalign=None):
    ptr = {k: FAKE for k in ("X", "Y", "train_idx", "n_train", "W_out", "b_out", "info_out", "ws")}
    arr = (F32 * max(len(alphas), 1))(*alphas)
    ptr["alphas"] = ctypes.addressof(arr)                # the one host pointer: it is read before the call returns
    if null:
        ptr[null] = None
    if misalign:
        ptr[misalign[0]] += misalign[1]
    return _native.lib().mdl_ridge_fit(ptr["X"], d if ldX is None else ldX, S, d, ptr["Y"], T if ldY is None else ldY, T, ptr["train_idx"],
                                       ptr["n_train"], Pn, n_max, ptr["alphas"], len(alphas) if A is None else A, ptr["W_out"], ptr["b_out"],
                                       ptr["info_out"], ptr["ws"], None)


def _scores(S=10, d=6, ldX=None, L=5, null=None, misalign=None):
    ptr = {k: FAKE for k in ("X", "W", "b", "Z")}
    if null:
        ptr[null] = None
    if misalign:
        ptr[misalign[0]] += misalign[1]
    return _native.lib().mdl_ridge_scores(ptr["X"], d if ldX is None else ldX, S, d, ptr["W"], ptr["b"], L, ptr["Z"], None)


def _metrics(Pn=3, n_max=4, S=10, T=2, ldY=None, A=2, null=None, misalign=None):
    ptr = {k: FAKE for k in ("Z", "Y", "train_idx", "n_train", "metrics_out", "sums_out", "ws")}
    if null:
        ptr[null] = None
    if misalign:
        ptr[misalign[0]] += misalign[1]
    return _native.lib().mdl_regress_metrics(ptr["Z"], ptr["Y"], T if ldY is None else ldY, T, ptr["train_idx"], ptr["n_train"], Pn, n_max, S,
                                             A, ptr["metrics_out"], ptr["sums_out"], ptr["ws"], None)


@pytest.mark.parametrize("call,null", [(_fit, n) for n in ("X", "Y", "train_idx", "n_train", "alphas", "W_out", "b_out", "info_out", "ws")] +
                         [(_scores, n) for n in ("X", "W", "b", "Z")] +
                         [(_metrics, n) for n in ("Z", "Y", "train_idx", "n_train", "metrics_out", "ws")])
def test_null_pointers_are_refused(call, null):
    assert call(null=null) == ARG


@pytest.mark.parametrize("call,kw,code", [
    (_fit, dict(Pn=0), ARG), (_fit, dict(n_max=0), ARG), (_fit, dict(S=0), ARG), (_fit, dict(d=0), ARG), (_fit, dict(T=0), ARG),
    (_fit, dict(A=0), ARG), (_fit, dict(ldX=5), ARG), (_fit, dict(ldY=1), ARG),
    (_fit, dict(alphas=(1.0, 0.0)), ARG), (_fit, dict(alphas=(-1.0,)), ARG), (_fit, dict(alphas=(float("nan"),)), ARG),
    (_fit, dict(alphas=(1.0, float("inf"))), ARG),
    (_fit, dict(n_max=1025, d=1025), UNSUP), (_fit, dict(n_max=16385), UNSUP), (_fit, dict(T=4097), UNSUP), (_fit, dict(alphas=(1.0,) * 17), UNSUP),
    (_fit, dict(Pn=1 << 31), UNSUP), (_fit, dict(Pn=1 << 20, n_max=1 << 12), UNSUP), (_fit, dict(Pn=40000), UNSUP),      # P A > 65535
    (_fit, dict(misalign=("ws", 8)), ALIGN), (_fit, dict(misalign=("X", 2)), ALIGN), (_fit, dict(misalign=("Y", 1)), ALIGN),
    (_fit, dict(misalign=("W_out", 2)), ALIGN), (_fit, dict(misalign=("train_idx", 2)), ALIGN),
    (_scores, dict(S=0), ARG), (_scores, dict(d=0), ARG), (_scores, dict(L=0), ARG), (_scores, dict(ldX=5), ARG),
    (_scores, dict(S=1 << 31), UNSUP), (_scores, dict(L=1 << 31), UNSUP), (_scores, dict(L=1 << 30, S=1 << 20), UNSUP),
    (_scores, dict(misalign=("Z", 2)), ALIGN), (_scores, dict(misalign=("W", 1)), ALIGN),
    (_metrics, dict(Pn=0), ARG), (_metrics, dict(n_max=0), ARG), (_metrics, dict(S=0), ARG), (_metrics, dict(T=0), ARG),
    (_metrics, dict(A=0), ARG), (_metrics, dict(ldY=1), ARG),
    (_metrics, dict(S=16385), UNSUP), (_metrics, dict(n_max=16385), UNSUP), (_metrics, dict(T=4097), UNSUP), (_metrics, dict(A=17), UNSUP),
    (_metrics, dict(Pn=1 << 31), UNSUP), (_metrics, dict(Pn=1 << 20, T=4096), UNSUP),
    (_metrics, dict(misalign=("ws", 8)), ALIGN), (_metrics, dict(misalign=("metrics_out", 4)), ALIGN),
    (_metrics, dict(misalign=("sums_out", 4)), ALIGN), (_metrics, dict(misalign=("Z", 2)), ALIGN),
])
def test_refusals(call, kw, code):
    assert call(**kw) == code


def test_refusals_come_in_the_family_order():
    """MDL_E_ARG before MDL_E_UNSUPPORTED before MDL_E_ALIGN, whatever else is wrong with the call."""
    assert _fit(alphas=(0.0,), n_max=16385, misalign=("ws", 8)) == ARG
    assert _fit(null="X", T=4097) == ARG and _fit(ldY=1, alphas=(1.0,) * 17) == ARG
    assert _fit(n_max=16385, misalign=("ws", 8)) == UNSUP
    assert _fit(alphas=(1.0,) * 16 + (0.0,)) == ARG and _fit(alphas=(1.0,) * 16 + (float("nan"),), n_max=16385) == ARG      # the 17th too
    assert _scores(ldX=5, S=1 << 31, misalign=("Z", 2)) == ARG and _scores(S=1 << 31, misalign=("Z", 2)) == UNSUP
    assert _metrics(ldY=1, S=16385, misalign=("ws", 8)) == ARG and _metrics(S=16385, misalign=("ws", 8)) == UNSUP


def test_the_other_probes_refuse_as_before():
    """probe_check grew additively: a survival call with the defaults of the new fields is refused and accepted as it was."""
    ws = _native.lib().mdl_cox_order_fit_ws_bytes
    assert ws(3, 1024, 512) > 0 and ws(3, 1025, 512) == UNSUP and ws(0, 4, 4) == ARG


# ---- the command line ----------------------------------------------------------------------------------------------------------------
def test_command_line_options_and_lines():
    from madeleine_amd import probe
    base = ["--slide_embedding_pkl", "e.pkl", "--label_path", "l.csv"]
    args = probe._parse(base + ["--regress", "ki67", "er_pct", "--alphas", "0.1", "1", "--cv_folds", "4"])
    assert args.regress == ["ki67", "er_pct"] and args.alphas == [0.1, 1.0] and args.cv_folds == 4
    plain = probe._parse(base)
    assert plain.regress is None and plain.alphas is None and plain.tasks == ["er", "pr", "her2"]      # without it, nothing changes
    for bad in (["--alphas", "1"], ["--regress", "ki67", "--alphas", "0"], ["--regress", "ki67", "--alphas", "-1"],
                ["--regress", "ki67", "--alphas", "inf"], ["--regress", "ki67", "--bootstrap", "10"]):
        with pytest.raises(SystemExit):
            probe._parse(base + bad)
    assert probe._float_or_nan("12.5") == 12.5 and all(np.isnan(probe._float_or_nan(v)) for v in ("", "n/a", None, "nan"))
    res = {("ki67", r): dict(pearson=np.array([[0.5, 0.25], [0.7, np.nan]]) + r, spearman=np.full((2, 2), 0.4), r2=np.full((2, 2), 0.1),
                             mae=np.full((2, 2), 2.0), rmse=np.full((2, 2), 3.0), n_test=np.array([10, 11])) for r in range(2)}
    lines = probe._regress_lines(res, ["ki67"], 2, (0.1, 1.0))
    assert lines[0] == ("regress=ki67, alpha=0.1, cases=21, pearson=1.1 +/- 0.51, spearman=0.4 +/- 0.0, r2=0.1 +/- 0.0, mae=2.0 +/- 0.0, "
                        "rmse=3.0 +/- 0.0")
    assert lines[1].startswith("regress=ki67, alpha=1, cases=21, pearson=0.75 +/- 0.5,") and len(lines) == 2      # a NaN fold is left out


# ---- regression_splits ---------------------------------------------------------------------------------------------------------------
def test_regression_splits_partition_determinism_and_errors():
    from madeleine_amd import regression_splits
    avail = np.ones(53, dtype=bool)
    avail[[3, 17, 40]] = False
    tr = regression_splits(avail, folds=5, repeat=1, seed_base=7)
    ref = R.splits(avail, 5, 1, 7)
    assert len(tr) == 5 and all(np.array_equal(t.numpy(), r) for t, r in zip(tr, ref))
    all_avail = set(np.nonzero(avail)[0].tolist())
    held = [all_avail - set(t.tolist()) for t in tr]
    assert set().union(*held) == all_avail and sum(len(h) for h in held) == 50 and {len(h) for h in held} == {10}
    assert all((np.diff(t.numpy()) > 0).all() for t in tr)
    again = regression_splits(torch.as_tensor(avail), folds=5, repeat=1, seed_base=7)
    assert all(torch.equal(a, b) for a, b in zip(tr, again))
    other = regression_splits(avail, folds=5, repeat=2, seed_base=7)
    assert any(not torch.equal(a, b) for a, b in zip(tr, other))
    sizes = sorted(23 - t.numel() for t in regression_splits(avail[:25], folds=4))      # 23 available cases: shares of 6, 6, 6, 5
    assert sizes == [5, 6, 6, 6]
    with pytest.raises(ValueError, match="fewer than"):
        regression_splits(np.array([True, False, True]), folds=3)
    with pytest.raises(ValueError, match="more than"):
        regression_splits(np.ones(16384 * 2 + 2, dtype=bool), folds=2, repeat=0)      # 16385 training cases
    with pytest.raises(ValueError):
        regression_splits(avail, folds=1)


# ---- the reference against independent formulas --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(40, 64), (64, 64), (200, 64), (1, 5), (2, 5), (33, 1)])
def test_the_two_forms_agree_and_equal_the_augmented_least_squares(n, d):
    X, Y = R.cohort(300, d, 1, seed=n + d)
    idx = np.random.default_rng(n).choice(300, n, replace=False)
    for alpha in (1e-3, 1.0, 50.0):
        wg, bg = R.ridge(X[idx], Y[idx, 0], alpha, "gram")
        wc, bc = R.ridge(X[idx], Y[idx, 0], alpha, "cov")
        scale = max(np.abs(wg).max(), 1e-30)
        assert np.abs(wg - wc).max() <= 1e-9 * scale + 1e-12 and abs(bg - bc) <= 1e-9 * max(1.0, abs(bg))
        # min |y - X w - b|^2 + alpha |w|^2 as ordinary least squares: sqrt(alpha) I rows under X, a column of ones the penalty never sees
        Xa = np.block([[X[idx].astype(np.float64), np.ones((n, 1))], [np.sqrt(alpha) * np.eye(d), np.zeros((d, 1))]])
        sol = np.linalg.lstsq(Xa, np.concatenate([Y[idx, 0].astype(np.float64), np.zeros(d)]), rcond=None)[0]
        assert np.abs(sol[:d] - wg).max() <= 1e-8 * scale + 1e-12 and abs(sol[d] - bg) <= 1e-8 * max(1.0, abs(bg))
    if n == 1:
        assert not wg.any() and bg == Y[idx[0], 0]


def test_the_reference_against_scikit_learn_and_scipy():
    lm = pytest.importorskip("sklearn.linear_model")
    skm = pytest.importorskip("sklearn.metrics")
    stats = pytest.importorskip("scipy.stats")
    X, Y = R.cohort(300, 32, 1, seed=2)
    y = Y[:, 0].astype(np.float64)
    y[::4] = np.round(y[::4], 1)                          # ties
    for n, alpha in ((20, 0.5), (150, 2.0)):
        idx = np.arange(n)
        w, b = R.ridge(X[idx], y[idx], alpha)
        sk = lm.Ridge(alpha=alpha, solver="cholesky").fit(X[idx].astype(np.float64), y[idx])
        assert np.abs(w - sk.coef_).max() <= 1e-9 and abs(b - sk.intercept_) <= 1e-9
        test = R.held_out(y, idx)
        z = np.round(X[test].astype(np.float64) @ w + b, 2)      # ties in z as well
        m = R.metrics(z, y[test])
        assert abs(m[1] - stats.pearsonr(z, y[test])[0]) <= 1e-12 and abs(m[2] - stats.spearmanr(z, y[test])[0]) <= 1e-12
        assert abs(m[3] - skm.r2_score(y[test], z)) <= 1e-12
        assert abs(m[4] - skm.mean_absolute_error(y[test], z)) <= 1e-12
        assert np.array_equal(R.doubled_ranks(z), np.rint(2 * stats.rankdata(z)).astype(np.int64))


def test_ranks_metrics_and_the_test_set_rule_on_fixed_arrays():
    v = np.array([3.0, -0.0, 0.0, 3.0, 1.0, 3.0], dtype=np.float32)
    assert list(R.doubled_ranks(v)) == [10, 3, 3, 10, 6, 10] and list(R.doubled_ranks_sorted(v)) == [10, 3, 3, 10, 6, 10]
    rng = np.random.default_rng(0)
    w = np.round(rng.standard_normal(5000), 1).astype(np.float32)
    assert np.array_equal(R.doubled_ranks(w), R.doubled_ranks_sorted(w))
    y = np.array([1.0, np.nan, 2.0, np.inf, 4.0, 5.0, 7.0])
    assert list(R.held_out(y, [0, 4, 9, -1])) == [2, 5, 6]
    z, yt = np.array([1.0, 2.0, 4.0]), np.array([1.0, 3.0, 2.0])
    m = R.metrics(z, yt)
    assert m[0] == 3 and abs(m[2] - 0.5) <= 1e-15 and abs(m[3] - (1 - 5.0 / 2.0)) <= 1e-15 and abs(m[4] - 1.0) <= 1e-15
    assert abs(m[5] - np.sqrt(5.0 / 3.0)) <= 1e-15 and abs(m[1] - 1.0 / np.sqrt(28.0 / 3.0)) <= 1e-12
    assert np.isnan(R.metrics(z[:1], yt[:1])[1:]).all() and R.metrics(z[:0], yt[:0])[0] == 0
    const = R.metrics(z, np.array([2.0, 2.0, 2.0]))
    assert np.isnan(const[1:4]).all() and np.isfinite(const[4:]).all()
    tied = R.metrics(np.array([0.0, -0.0, 0.0]), yt)
    assert np.isnan(tied[1:3]).all() and np.isfinite(tied[3:]).all()
    assert np.isnan(R.metrics(np.array([1.0, np.nan, 2.0]), yt)[1:]).all()


# ---- seeded faults the checkers must catch -------------------------------------------------------------------------------------------
def test_seeded_faults_are_caught():
    X, Y = R.cohort(200, 16, 1, seed=4)
    y = np.round(Y[:, 0].astype(np.float64), 1)
    idx = np.arange(60)
    test = R.held_out(y, idx)
    w, b = R.ridge(X[idx], y[idx], 1.0)
    z = np.round(X[test].astype(np.float64) @ w + b, 1)
    good, sums = R.metrics(z, y[test]), R.rank_sums(z, y[test])
    assert (np.bincount(np.unique(z, return_inverse=True)[1]) > 1).any()           # there are ties to break

    def rho_of(rz, ry):
        n = len(rz)
        return (n * (rz * ry).sum() - rz.sum() * ry.sum()) / np.sqrt(float(n * (rz * rz).sum() - rz.sum() ** 2) * float(n * (ry * ry).sum() - ry.sum() ** 2))
    rz, ry = R.doubled_ranks(z), R.doubled_ranks(y[test])
    assert abs(rho_of(rz, ry) - good[2]) <= 1e-15
    off = rz.copy()
    off[0] += 1                                           # a rank off by 1/2 (doubled: by 1)
    assert [int(len(off)), int(off.sum()), int(ry.sum()), int((off * off).sum()), int((ry * ry).sum()), int((off * ry).sum())] != sums
    broken = (2 * np.argsort(np.argsort(z, kind="stable"), kind="stable") + 2).astype(np.int64)      # ties broken by position
    assert int((broken * broken).sum()) != sums[3] and abs(rho_of(broken, ry) - good[2]) > 1e-9
    r2_train = 1.0 - ((y[test] - z) ** 2).sum() / ((y[test] - y[idx].mean()) ** 2).sum()           # R^2 about the training mean
    assert abs(r2_train - good[3]) > 1e-9
    # a penalised intercept: ridge on [X, 1] with the penalty on every coefficient (targets with a mean to shrink: y + 3)
    Xa = np.hstack([X[idx].astype(np.float64), np.ones((60, 1))])
    wp = np.linalg.solve(Xa.T @ Xa + np.eye(17), Xa.T @ (y[idx] + 3.0))
    z64 = X.astype(np.float64) @ w + b
    assert R.parity(X.astype(np.float64) @ wp[:16] + wp[16], z64 + 3.0) > 1e-3
    # alpha added before centring: the Gram of the raw rows, then the intercept from the means
    Xr = X[idx].astype(np.float64)
    wr = Xr.T @ np.linalg.solve(Xr @ Xr.T + np.eye(60), y[idx] - y[idx].mean())
    assert R.parity(X.astype(np.float64) @ wr + (y[idx].mean() - Xr.mean(0) @ wr), z64) > 1e-3


# ---- the precision condition: a cap, not a measurement -------------------------------------------------------------------------------
@pytest.mark.parametrize("S,d,n,kind", [(300, 64, 40, "unit"), (300, 64, 40, "clustered"), (300, 64, 200, "clustered"),
                                        (400, 512, 257, "unit"), (1153, 512, 922, "unit"), (1153, 512, 922, "clustered")])
def test_the_storage_rounding_stays_within_a_tenth_of_the_bound(S, d, n, kind):
    """W and b rounded to fp32 and z accumulated in fp32 move z by at most 1e-4 max |z64| -- a tenth of the 1e-3 the GPU file holds the
    fit to -- for alpha / lambda_max from 1e-6 to 1.  Measured here: at most 3e-5."""
    X, Y = R.cohort(S, d, 1, kind, seed=S + n)
    idx = np.sort(np.random.default_rng(n).choice(S, n, replace=False))
    lam = R.lambda_max(X, idx)
    worst = 0.0
    for rel in (1e-6, 1e-3, 1.0):
        w, b = R.ridge(X[idx], Y[idx, 0], rel * lam)
        worst = max(worst, R.parity(R.stored_scores(X, w, b), R.scores64(X, w, b)))
    print("storage rounding S=%d d=%d n=%d %s: %.2e" % (S, d, n, kind, worst))
    assert worst <= 1e-4
