"""The regression probe on the device (mdl_ridge_fit / mdl_ridge_scores / mdl_regress_metrics, madeleine_amd.regress) against the numpy
fp64 contract of tests/_regress_ref.py.  The entry points are called through the C ABI with every output and workspace filled with
NaN bytes first, and X and Y as views of wider buffers whose padding columns hold NaN.

Bounds.  Fit: z from the returned fp32 W and b, formed in fp64, within 1e-3 max |z64| of the fp64 optimum over the whole cohort (the
sibling probes' contract; tests/test_regress_cpu.py caps what the fp32 storage alone costs at a tenth of it).  Scores: every element
within (d + 2) 2^-24 (sum |x| |w| + |b|).  Metrics, on the z read back: the integers exact, r and rho within 1e-9 absolute, MAE and RMSE
1e-9 relative, R^2 1e-9 max(1, |R^2|) (two-pass fp64 sums at n <= 16384 err below about 4e-12).  Every test prints what it measured."""
import ctypes
import functools
import warnings

import numpy as np
import pytest
import torch

from tests import _regress_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _padded(M, ld):
    """A [rows, cols] fp32 host array on the device as a view of a [rows, ld] buffer with NaN in the padding columns."""
    M = torch.as_tensor(np.asarray(M, dtype=np.float32))
    buf = torch.full((M.shape[0], ld), float("nan"), dtype=torch.float32, device=DEV)
    buf[:, :M.shape[1]] = M.to(DEV)
    return buf[:, :M.shape[1]]


def _nan_bytes(*shape, dtype):
    """A tensor whose every byte is 0xFF: NaN in fp32 and fp64, -1 in the integer types."""
    size = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    return torch.full((size,), 255, dtype=torch.uint8, device=DEV).view(dtype).reshape(shape)


def _table(lists, n_max=None, n_train=None):
    n = [len(t) for t in lists]
    n_max = n_max or max(max(n), 1)
    table = torch.full((len(lists), n_max), -1, dtype=torch.int32)
    for p, t in enumerate(lists):
        table[p, :n[p]] = torch.as_tensor(np.asarray(t, dtype=np.int64)).to(torch.int32)
    return table.to(DEV), torch.tensor(n if n_train is None else n_train, dtype=torch.int32, device=DEV)


def _check(rc, what):
    assert rc == 0, "%s returned %d" % (what, rc)


def _fit(Xd, Yd, table, n_train, alphas):
    from madeleine_amd import _native
    lib = _native.lib()
    (S, d), T, (P, n_max), A = Xd.shape, Yd.shape[1], table.shape, len(alphas)
    nbytes = lib.mdl_ridge_fit_ws_bytes(P, n_max, d, T, A)
    assert nbytes > 0 and nbytes % 16 == 0
    ws = torch.full((nbytes,), 255, dtype=torch.uint8, device=DEV)
    W, b, info = _nan_bytes(P, A, T, d, dtype=torch.float32), _nan_bytes(P, A, T, dtype=torch.float32), _nan_bytes(P, A, 2, dtype=torch.float32)
    arr = (ctypes.c_float * A)(*alphas)
    _check(lib.mdl_ridge_fit(Xd.data_ptr(), Xd.stride(0), S, d, Yd.data_ptr(), Yd.stride(0), T, table.data_ptr(), n_train.data_ptr(), P,
                             n_max, arr, A, W.data_ptr(), b.data_ptr(), info.data_ptr(), ws.data_ptr(),
                             torch.cuda.current_stream().cuda_stream), "mdl_ridge_fit")
    return W, b, info


def _scores(Xd, W, b):
    from madeleine_amd import _native
    S, d = Xd.shape
    Z = _nan_bytes(*b.shape, S, dtype=torch.float32)
    _check(_native.lib().mdl_ridge_scores(Xd.data_ptr(), Xd.stride(0), S, d, W.data_ptr(), b.data_ptr(), b.numel(), Z.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream), "mdl_ridge_scores")
    return Z


def _metrics(Z, Yd, table, n_train):
    from madeleine_amd import _native
    lib = _native.lib()
    P, A, T, S = Z.shape
    nbytes = lib.mdl_regress_metrics_ws_bytes(P, S, T)
    assert nbytes > 0 and nbytes % 16 == 0
    ws = torch.full((nbytes,), 255, dtype=torch.uint8, device=DEV)
    M, sums = _nan_bytes(P, A, T, 6, dtype=torch.float64), _nan_bytes(P, A, T, 6, dtype=torch.int64)
    _check(lib.mdl_regress_metrics(Z.data_ptr(), Yd.data_ptr(), Yd.stride(0), T, table.data_ptr(), n_train.data_ptr(), P, table.shape[1], S,
                                   A, M.data_ptr(), sums.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream),
           "mdl_regress_metrics")
    torch.cuda.synchronize()
    return M.cpu().numpy(), sums.cpu().numpy()


def _host(*tensors):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in tensors]


def _lists(S, ns, seed):
    rng = np.random.default_rng(seed)
    return [np.sort(rng.choice(S, n, replace=False)) for n in ns]


# ---- fit -----------------------------------------------------------------------------------------------------------------------------
NS = (1, 2, 33, 65, 257)
FIT_CASES = {       # S, d, ldX, T, ldY, n_train of the problems, alphas, rows
    "d1": (300, 1, 1, 1, 1, NS, (1.0,), "unit"),
    "d5": (300, 5, 8, 3, 4, NS, (0.1, 1.0, 10.0), "unit"),
    "d77_switch": (300, 77, 80, 9, 12, NS + (76, 77, 78), (0.1, 1.0, 10.0), "unit"),
    "d512": (400, 512, 512, 130, 136, NS, (1.0,), "unit"),
    "gram1024": (1100, 1030, 1032, 1, 1, (1024,), (1.0,), "unit"),
    "cov1024": (1200, 1024, 1024, 1, 3, (1100,), (1.0,), "unit"),
    "clustered": (300, 64, 64, 3, 3, (40, 200), None, "clustered"),       # alpha = 1e-6 lambda_max of each problem: one call each
}


def _parity_of(X, Y, lists, alphas, W, b):
    """Worst max |z - z64| / max |z64| over the problems, z in fp64 from the returned fp32 W and b."""
    W64, b64 = R.ridge_fit(X, Y, lists, alphas)
    z64, z = R.scores64(X, W64, b64), R.scores64(X, W, b)
    worst = 0.0
    for p in range(len(lists)):
        for a in range(len(alphas)):
            for t in range(Y.shape[1]):
                worst = max(worst, R.parity(z[p, a, t], z64[p, a, t]))
    return worst


@pytest.mark.parametrize("name", list(FIT_CASES))
def test_fit_reaches_the_fp64_optimum(name):
    """Measured on the MI355X (worst max |z - z64| / max |z64| per case): see DESIGN 3.22."""
    S, d, ldX, T, ldY, ns, alphas, kind = FIT_CASES[name]
    X, Y = R.cohort(S, d, T, kind, seed=len(name))
    Xd, Yd = _padded(X, ldX), _padded(Y, ldY)
    lists = _lists(S, ns, seed=d)
    calls = [(lists, alphas)] if alphas else [([idx], (1e-6 * R.lambda_max(X, idx),)) for idx in lists]
    for ls, al in calls:
        table, n_train = _table(ls)
        W, b, info = _host(*_fit(Xd, Yd, table, n_train, al))
        assert (info[..., 0] == 1).all() and (info[..., 1] > 0).all(), info
        worst = _parity_of(X, Y, ls, al, W, b)
        print("%s n=%s alphas=%s: worst parity %.2e, smallest pivot ratio %.2e" % (name, [len(t) for t in ls], al, worst, info[..., 1].min()))
        assert worst <= 1e-3, (name, worst)
        for p, idx in enumerate(ls):
            if len(idx) == 1:                        # one training row: W = 0 and b = y exactly
                assert not W[p].any() and (b[p] == Y[idx[0]][None, :]).all()


def test_duplicate_training_rows():
    """A case listed twice counts twice, and two cases with the same embedding are two rows: both are the reference's own reading."""
    S, d, T = 200, 77, 2
    X, Y = R.cohort(S, d, T, seed=5)
    X[10:20] = X[0:10]                               # equal rows under different indices
    lists = [np.concatenate([np.arange(0, 30), np.arange(5, 15)]), np.concatenate([np.arange(0, 100), np.arange(0, 100)])]
    Xd, Yd = _padded(X, 80), _padded(Y, T)
    table, n_train = _table(lists)
    W, b, info = _host(*_fit(Xd, Yd, table, n_train, (0.5,)))
    worst = _parity_of(X, Y, lists, (0.5,), W, b)
    print("duplicates: worst parity %.2e" % worst)
    assert (info[..., 0] == 1).all() and worst <= 1e-3


@functools.lru_cache(maxsize=None)
def _mixed_call():
    """Four problems of one call: clean, a NaN training target in column 1, an index out of range, n_train = 0."""
    S, d, T = 150, 20, 3
    X, Y = R.cohort(S, d, T, seed=9)
    lists = _lists(S, (30, 40, 25, 12), seed=3)
    Y[lists[1][7], 1] = np.nan
    lists[2] = lists[2].copy()
    lists[2][3] = S
    alphas = (0.3, 2.0)
    table, n_train = _table(lists, n_max=48, n_train=[30, 40, 25, 0])
    Xd, Yd = _padded(X, 24), _padded(Y, 4)
    W, b, info = _fit(Xd, Yd, table, n_train, alphas)
    Z = _scores(Xd, W, b)
    M, sums = _metrics(Z, Yd, table, n_train)
    W, b, info, Z = _host(W, b, info, Z)
    return dict(X=X, Y=Y, Xd=Xd, Yd=Yd, lists=lists, alphas=alphas, W=W, b=b, info=info, Z=Z, M=M, sums=sums)


def test_poison_stays_with_its_own_outputs():
    c = _mixed_call()
    W, b, info, M = c["W"], c["b"], c["info"], c["M"]
    assert np.isfinite(W[0]).all() and np.isfinite(b[0]).all() and (info[0, :, 0] == 1).all()
    assert np.isnan(W[1][:, 1]).all() and np.isnan(b[1][:, 1]).all()                      # the NaN target's column only
    assert np.isfinite(W[1][:, [0, 2]]).all() and np.isfinite(b[1][:, [0, 2]]).all() and (info[1, :, 0] == 1).all()
    for p in (2, 3):                                 # refused problems
        assert np.isnan(W[p]).all() and np.isnan(b[p]).all() and (info[p, :, 0] == 0).all() and np.isnan(info[p, :, 1]).all()
        assert np.isnan(M[p][..., 1:]).all()
    assert np.isnan(M[1][:, 1, 1:]).all() and np.isfinite(M[1][:, [0, 2], 1:]).all() and np.isfinite(M[0][..., 1:]).all()
    W64, b64 = R.ridge_fit(c["X"], c["Y"], c["lists"][:2], c["alphas"])
    z64, z = R.scores64(c["X"], W64, b64), R.scores64(c["X"], W[:2], b[:2])
    for p, t in ((0, 0), (0, 1), (0, 2), (1, 0), (1, 2)):
        for a in range(2):
            assert R.parity(z[p, a, t], z64[p, a, t]) <= 1e-3


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def test_bits_do_not_depend_on_the_rest_of_the_call():
    """The covariance form (every problem here has n > d = 20).  Problem 0 of the mixed call, column 2 under alpha 2.0, alone in a call of its own (P = 1, n_max = n, T = 1, A = 1, other strides):
    the same bits in W, b, info, z and the metrics."""
    c = _mixed_call()
    Xd, Yd = _padded(c["X"], 20), _padded(c["Y"][:, 2:3], 1)
    table, n_train = _table(c["lists"][:1])
    W, b, info = _fit(Xd, Yd, table, n_train, (2.0,))
    Z = _scores(Xd, W, b)
    M, sums = _metrics(Z, Yd, table, n_train)
    W, b, info, Z = _host(W, b, info, Z)
    assert np.array_equal(_bits(W[0, 0, 0]), _bits(c["W"][0, 1, 2])) and np.array_equal(_bits(b[0, 0, 0]), _bits(c["b"][0, 1, 2]))
    assert np.array_equal(_bits(info[0, 0]), _bits(c["info"][0, 1])) and np.array_equal(_bits(Z[0, 0, 0]), _bits(c["Z"][0, 1, 2]))
    assert np.array_equal(_bits(M[0, 0, 0]), _bits(c["M"][0, 1, 2])) and np.array_equal(sums[0, 0, 0], c["sums"][0, 1, 2])
    # the covariance form again, alone and as the third problem of a wider table (the Gram form: _gram_call below)
    lists = _lists(150, (60, 21, 90), seed=4)
    Xd, Yd = _padded(c["X"], 24), _padded(c["Y"], 3)
    t3, n3 = _table(lists, n_max=100)
    t1, n1 = _table(lists[2:])
    W3, b3 = _host(*_fit(Xd, Yd, t3, n3, (0.3, 2.0))[:2])
    W1, b1 = _host(*_fit(Xd, Yd, t1, n1, (2.0,))[:2])
    assert np.array_equal(_bits(W1[0, 0]), _bits(W3[2, 1])) and np.array_equal(_bits(b1[0, 0]), _bits(b3[2, 1]))


# ---- the Gram form (n <= d): poison and bits, as for the covariance form above ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gram_call():
    """Four Gram-form problems of one call at d = 64: clean (n 30), a NaN training target in column 1 (n 40), an index out of range
    (n 25), n_train = 0; the fifth (n 64 = d) is the largest Gram system of the call."""
    S, d, T = 150, 64, 3
    X, Y = R.cohort(S, d, T, seed=19)
    lists = _lists(S, (30, 40, 25, 12, 64), seed=6)
    Y[lists[1][11], 1] = np.nan
    lists[2] = lists[2].copy()
    lists[2][0] = -1
    alphas = (0.3, 2.0)
    table, n_train = _table(lists, n_max=70, n_train=[30, 40, 25, 0, 64])
    Xd, Yd = _padded(X, 72), _padded(Y, 4)
    W, b, info = _fit(Xd, Yd, table, n_train, alphas)
    Z = _scores(Xd, W, b)
    M, sums = _metrics(Z, Yd, table, n_train)
    W, b, info, Z = _host(W, b, info, Z)
    return dict(X=X, Y=Y, lists=lists, alphas=alphas, W=W, b=b, info=info, Z=Z, M=M, sums=sums)


def test_gram_form_poison_stays_with_its_own_outputs():
    c = _gram_call()
    W, b, info, M = c["W"], c["b"], c["info"], c["M"]
    for p in (0, 4):
        assert np.isfinite(W[p]).all() and np.isfinite(b[p]).all() and (info[p, :, 0] == 1).all() and np.isfinite(M[p][..., 1:]).all()
    assert np.isnan(W[1][:, 1]).all() and np.isnan(b[1][:, 1]).all() and np.isnan(M[1][:, 1, 1:]).all()      # through y - ybar and Xc^T c
    assert np.isfinite(W[1][:, [0, 2]]).all() and np.isfinite(b[1][:, [0, 2]]).all() and (info[1, :, 0] == 1).all()
    assert np.isfinite(M[1][:, [0, 2], 1:]).all()
    for p in (2, 3):
        assert np.isnan(W[p]).all() and np.isnan(b[p]).all() and (info[p, :, 0] == 0).all() and np.isnan(info[p, :, 1]).all()
        assert np.isnan(M[p][..., 1:]).all()
    keep = [0, 1, 4]
    W64, b64 = R.ridge_fit(c["X"], c["Y"], [c["lists"][p] for p in keep], c["alphas"])
    z64, z = R.scores64(c["X"], W64, b64), R.scores64(c["X"], W[keep], b[keep])
    worst = max(R.parity(z[k, a, t], z64[k, a, t]) for k in range(3) for a in range(2) for t in range(3) if (k, t) != (1, 1))
    print("gram call: worst parity %.2e" % worst)
    assert worst <= 1e-3
    _hold_metrics(M, c["sums"], c["Z"], c["Y"], c["lists"][:3] + [c["lists"][3][:0], c["lists"][4]], "gram call")


def test_gram_form_bits_do_not_depend_on_the_rest_of_the_call():
    """Problems 0 (n 30) and 4 (n 64 = d) of the Gram call, one column under one penalty, each alone in a call of its own: P = 1,
    n_max = n (another leading dimension of the system), T = 1, A = 1, other strides of X and Y -- the same bits everywhere."""
    c = _gram_call()
    for p, a, t in ((0, 1, 2), (4, 0, 1)):
        Xd, Yd = _padded(c["X"], 64), _padded(c["Y"][:, t:t + 1], 1)
        table, n_train = _table([c["lists"][p]])
        W, b, info = _fit(Xd, Yd, table, n_train, (c["alphas"][a],))
        Z = _scores(Xd, W, b)
        M, sums = _metrics(Z, Yd, table, n_train)
        W, b, info, Z = _host(W, b, info, Z)
        assert np.array_equal(_bits(W[0, 0, 0]), _bits(c["W"][p, a, t])) and np.array_equal(_bits(b[0, 0, 0]), _bits(c["b"][p, a, t]))
        assert np.array_equal(_bits(info[0, 0]), _bits(c["info"][p, a])) and np.array_equal(_bits(Z[0, 0, 0]), _bits(c["Z"][p, a, t]))
        assert np.array_equal(_bits(M[0, 0, 0]), _bits(c["M"][p, a, t])) and np.array_equal(sums[0, 0, 0], c["sums"][p, a, t])


# ---- a factorisation that fails ------------------------------------------------------------------------------------------------------
def _collinear(S):
    """Embeddings 3 k x, x = (2^33, 0, 0, 0): any three of them centre to integer multiples (c0, c1, c2) of x with sum 0, their Gram
    matrix 2^66 c c^T is exact and swallows alpha = 1e-30, and the second or third pivot of its Cholesky is exactly 0."""
    X = np.zeros((S, 4), dtype=np.float32)
    X[:, 0] = 3.0 * np.arange(1, S + 1) * 2.0 ** 33
    return X


def test_a_pivot_that_is_not_positive_fails_its_own_fit_only():
    X = _collinear(6)
    Y = np.arange(6, dtype=np.float32)[:, None] ** 2
    table, n_train = _table([np.array([0, 2, 5]), np.array([1, 3, 4])])
    W, b, info = _host(*_fit(_padded(X, 4), _padded(Y, 1), table, n_train, (1e-30, 1e30)))
    assert (info[:, 0, 0] == 0).all() and np.isnan(W[:, 0]).all() and np.isnan(b[:, 0]).all()      # alpha = 1e-30: a zero pivot
    assert (info[:, 1, 0] == 1).all() and np.isfinite(W[:, 1]).all() and np.isfinite(b[:, 1]).all()  # alpha = 1e30: the same systems factorise


def test_regression_probe_announces_failed_factorisations_once():
    from madeleine_amd import regression_probe
    y = np.arange(6, dtype=np.float32) ** 2
    with pytest.warns(RuntimeWarning, match="factorisations failed") as rec:
        out = regression_probe(_collinear(6), {"a": y, "b": -y}, folds=2, alphas=(1e-30,))
    assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1
    for res in out.values():
        assert not res["ok"].any() and np.isnan(res["pearson"]).all() and list(res["n_test"]) == [3, 3]


# ---- scores --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,d,ldX,L", [(150, 20, 24, 24), (300, 77, 80, 70), (333, 512, 512, 130), (64, 1, 1, 64), (65, 33, 40, 1)])
def test_scores_within_the_chain_bound(S, d, ldX, L):
    rng = np.random.default_rng(S + d)
    X, _ = R.cohort(S, d, 1, seed=d)
    W = rng.standard_normal((L, d)).astype(np.float32)
    b = rng.standard_normal(L).astype(np.float32)
    Xd = _padded(X, ldX)
    Z, = _host(_scores(Xd, torch.as_tensor(W).to(DEV), torch.as_tensor(b).to(DEV)))
    err, bound = np.abs(Z - R.scores64(X, W, b)), R.scores_bound(X, W, b)
    print("scores S=%d d=%d L=%d: worst error / bound %.3f" % (S, d, L, (err / bound).max()))
    assert Z.shape == (L, S) and (err <= bound).all()


def test_scores_of_the_fitted_weights():
    c = _mixed_call()
    for p in (0, 1):
        ok = np.isfinite(c["b"][p])
        err = np.abs(c["Z"][p][ok] - R.scores64(c["X"], c["W"][p][ok], c["b"][p][ok]))
        assert (err <= R.scores_bound(c["X"], c["W"][p][ok], c["b"][p][ok])).all()
    assert np.isnan(c["Z"][2]).all() and np.isnan(c["Z"][3]).all() and np.isnan(c["Z"][1][:, 1]).all()


# ---- metrics -------------------------------------------------------------------------------------------------------------------------
def _hold_metrics(M, sums, Z, Y, lists, what):
    """The device's metrics and integer sums against the reference on the same z."""
    Mr, Sr = R.regress_metrics(Z, Y, lists)
    assert np.array_equal(sums, Sr), what
    assert np.array_equal(M[..., 0], Mr[..., 0]), what
    assert np.array_equal(np.isnan(M), np.isnan(Mr)), (what, M, Mr)
    worst = {}
    for c, name in ((1, "pearson"), (2, "spearman"), (3, "r2"), (4, "mae"), (5, "rmse")):
        fin = np.isfinite(Mr[..., c])
        got, ref = M[..., c][fin], Mr[..., c][fin]
        scale = np.ones_like(ref) if c in (1, 2) else (np.maximum(1.0, np.abs(ref)) if c == 3 else np.where(ref == 0, 1.0, np.abs(ref)))
        err = np.abs(got - ref) / scale
        worst[name] = float(err.max()) if err.size else 0.0
        assert (err <= 1e-9).all(), (what, name, worst[name])
    print("%s: worst metric errors %s" % (what, worst))
    return Mr


def test_metrics_of_the_mixed_call():
    c = _mixed_call()
    _hold_metrics(c["M"], c["sums"], c["Z"], c["Y"], c["lists"][:2] + [c["lists"][2], c["lists"][3][:0]], "mixed call")


def test_metrics_with_ties_constant_targets_and_all_tied_scores():
    """Column 0 continuous, column 1 quantised to 5 levels (heavy ties in y), column 2 constant (r, rho, R^2 NaN), column 3 with NaN
    values (fewer test cases); problem 2 trains on one case, so W = 0 and all its z are tied (r and rho NaN, R^2 defined)."""
    S, d = 300, 16
    X, Y = R.cohort(S, d, 4, seed=21)
    Y[:, 1] = np.round(np.clip(Y[:, 1], -1, 1) * 2) / 2
    Y[:, 2] = 0.75
    Y[::7, 3] = np.nan
    lists = _lists(S, (100, 240), seed=8) + [np.array([17])]
    lists[0] = np.sort(lists[0][~np.isnan(Y[lists[0], 3])])      # problem 0 can be fitted for column 3; problem 1 cannot
    Xd, Yd = _padded(X, d), _padded(Y, 6)
    table, n_train = _table(lists)
    W, b, info = _fit(Xd, Yd, table, n_train, (0.1, 1.0))
    Z = _scores(Xd, W, b)
    M, sums = _metrics(Z, Yd, table, n_train)
    Zh, Wh = _host(Z, W)
    Mr = _hold_metrics(M, sums, Zh, Y, lists, "ties")
    assert np.isnan(Mr[:, :, 2, 1:4]).all() and np.isfinite(Mr[:, :, 2, 4:]).all()            # the constant target
    assert not Wh[2][:, :2].any() and np.isnan(Mr[2, :, :2, 1:3]).all() and np.isfinite(Mr[2, :, :2, 3:]).all()      # W = 0
    assert np.isnan(M[1, :, 3, 1:]).all() and np.isfinite(M[0, :, 3, 1:]).all()
    assert len(np.unique(Y[:, 1])) == 5


def test_metrics_with_zero_one_and_two_test_cases_and_signed_zeros():
    """Z is uploaded: -0 and +0 are one value in y and in z; n_test = 0, 1, 2 by training on all but that many cases."""
    S = 12
    Y = np.array([[-0.0, 0.0, 1.0, 1.0, -0.0, 2.0, 0.0, 3.0, -1.0, 0.0, -0.0, 1.0]], dtype=np.float32).T.copy()
    Z = np.array([0.0, -0.0, 0.5, -0.0, 0.0, 0.5, 1.0, -0.0, 0.0, 2.0, 0.0, -0.0], dtype=np.float32)
    lists = [np.arange(S), np.arange(1, S), np.arange(2, S), np.arange(0), np.array([5, 6])]
    Zs = np.tile(Z, (len(lists), 1, 1, 1)).astype(np.float32)
    Zs[:, 0, 0, :] = Z
    table, n_train = _table(lists, n_max=S, n_train=[12, 11, 10, 0, 2])
    M, sums = _metrics(torch.as_tensor(Zs).to(DEV), _padded(Y, 2), table, n_train)
    Mr = _hold_metrics(M, sums, Zs, Y, lists, "signed zeros")
    assert list(M[:, 0, 0, 0]) == [0, 1, 2, 12, 10] and np.isnan(M[:2, 0, 0, 1:]).all() and np.isfinite(Mr[3:, 0, 0, 1:]).all()
    assert sums[3, 0, 0, 1] == 12 * 13 and sums[3, 0, 0, 2] == 12 * 13           # sum of doubled ranks = n (n + 1) whatever the ties


def test_metrics_at_the_largest_cohort():
    """S = 16384 once: the integers (n sum Rz Ry reaches 1e17) and the bounds."""
    S, d = 16384, 4
    X, Y = R.cohort(S, d, 1, seed=77)
    Y[::3, 0] = np.round(Y[::3, 0], 1)               # a third of the targets tied in groups
    lists = _lists(S, (100,), seed=1)
    Xd, Yd = _padded(X, d), _padded(Y, 1)
    table, n_train = _table(lists)
    W, b, info = _fit(Xd, Yd, table, n_train, (1.0,))
    Z = _scores(Xd, W, b)
    M, sums = _metrics(Z, Yd, table, n_train)
    Zh, = _host(Z)
    _hold_metrics(M, sums, Zh, Y, lists, "S = 16384")
    assert M[0, 0, 0, 0] == S - 100 and sums[0, 0, 0, 0] * sums[0, 0, 0, 5] > 5e16


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_regression_probe_against_the_reference_loop():
    """regression_probe on S = 120, d = 32 with two availability groups against ridge() and metrics() over splits() of the same masks.
    Tolerance: the device's z differ from the reference's by the fp32 storage, at most delta = 2 (d + 2) 2^-24 (sum |x| |w| + |b|) per case;
    r, R^2, MAE and RMSE are Lipschitz in z / sigma_z, and delta / sigma_z stays below 1e-5 here, so 1e-4 leaves a factor of ten.  rho is
    exact unless two test scores are closer than 2 delta; each of the k pairs that are may swap two adjacent ranks, which moves
    sum d^2 by at most 2 (n + 1) and rho by at most 12 / (n (n - 1)): rho is held to 1e-9 + 12 k / (n (n - 1))."""
    from madeleine_amd import regression_probe
    S, d, folds, alphas = 120, 32, 4, (0.1, 1.0)
    X, Y = R.cohort(S, d, 3, seed=33)
    Y[5::9, 1] = np.nan
    Y[5::9, 2] = np.nan
    targets = {"ki67": Y[:, 0], "er_pct": Y[:, 1], "pr_pct": Y[:, 2]}
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = regression_probe(torch.as_tensor(X), targets, folds=folds, repeats=2, alphas=alphas, seed_base=3)
    assert set(out) == {(n, r) for n in targets for r in range(2)}
    worst = 0.0
    for (name, repeat), res in out.items():
        y = targets[name]
        for fold, idx in enumerate(R.splits(np.isfinite(y), folds, repeat, 3)):
            test = R.held_out(y, idx)
            assert res["n_test"][fold] == len(test) and res["ok"][fold].all()
            for a, alpha in enumerate(alphas):
                w, b = R.ridge(X[idx], y[idx], alpha)
                z = X[test].astype(np.float64) @ w + b
                delta = 2 * (d + 2) * 2.0 ** -24 * (np.abs(X[test]).astype(np.float64) @ np.abs(w) + abs(b))
                k, n = int((np.diff(np.sort(z)) <= 2 * delta.max()).sum()), len(test)
                ref = R.metrics(z, y[test])
                got = [res[m][fold, a] for m in ("pearson", "spearman", "r2", "mae", "rmse")]
                assert abs(got[1] - ref[2]) <= 1e-9 + 12.0 * k / (n * (n - 1))
                for m, g, r in zip("r rho R2 mae rmse".split(), got, ref[1:]):
                    if m != "rho":
                        worst = max(worst, abs(g - r))
                        assert abs(g - r) <= 1e-4 * max(1.0, abs(r)), (name, repeat, fold, m, g, r)
        assert list(res["alphas"]) == list(alphas)
    print("regression_probe: worst metric difference %.2e" % worst)
