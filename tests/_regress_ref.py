"""The contract of the regression probe (include/madeleine_amd_regress.h) in numpy fp64: the closed-form ridge with an unpenalised
intercept in both forms, regression_splits' dealing, the test-set rule, the six metrics with average ranks written from their
definition, and an emulation of the storage rounding (W and b rounded to fp32, z accumulated in fp32).  No GPU, no library."""
import numpy as np
import torch


# ---- the fit -------------------------------------------------------------------------------------------------------------------------
def ridge(X, y, alpha, form="auto"):
    """(w [d], b) minimising sum (y - X w - b)^2 + alpha |w|^2 over the rows given, in fp64 (y [n, T]: w [d, T], b [T]).  form: "gram"
    solves the n x n system of the centred rows, "cov" the d x d one, "auto" the smaller (the Gram form at n <= d)."""
    X, y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n, d = X.shape
    xm, ym = X.mean(0), y.mean(0)
    Xc, yc = X - xm, y - ym
    if form == "auto":
        form = "gram" if n <= d else "cov"
    if form == "gram":
        w = Xc.T @ np.linalg.solve(Xc @ Xc.T + alpha * np.eye(n), yc)
    else:
        w = np.linalg.solve(Xc.T @ Xc + alpha * np.eye(d), Xc.T @ yc)
    return w, ym - xm @ w


def ridge_fit(X, Y, train_lists, alphas, form="auto"):
    """(W [P, A, T, d], b [P, A, T]) in fp64: ridge() for every problem, penalty and target; NaN where a training target is NaN, the
    list is empty or an index is out of range."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    S, d = X.shape
    T = Y.shape[1]
    W = np.full((len(train_lists), len(alphas), T, d), np.nan)
    b = np.full((len(train_lists), len(alphas), T), np.nan)
    for p, idx in enumerate(train_lists):
        idx = np.asarray(idx, dtype=np.int64)
        if idx.size < 1 or idx.min() < 0 or idx.max() >= S:
            continue
        whole = np.nonzero(~np.isnan(Y[idx]).any(0))[0]      # the targets without a NaN among the training rows: one solve for all
        for a, alpha in enumerate(alphas):
            if whole.size:
                w, b0 = ridge(X[idx], Y[idx][:, whole], float(alpha), form)
                W[p, a, whole], b[p, a, whole] = w.T, b0
    return W, b


def scores64(X, W, b):
    """z [..., S] in fp64 from W [..., d] and b [...]."""
    return np.asarray(W, dtype=np.float64) @ np.asarray(X, dtype=np.float64).T + np.asarray(b, dtype=np.float64)[..., None]


def scores_bound(X, W, b):
    """(d + 2) 2^-24 (sum |x| |w| + |b|) per element: the bound of an fp32 FMA chain of d terms and one addition."""
    X, W, b = (np.asarray(v, dtype=np.float64) for v in (X, W, b))
    return (X.shape[1] + 2) * 2.0 ** -24 * (np.abs(W) @ np.abs(X).T + np.abs(b)[..., None])


def stored_scores(X, w, b):
    """The storage rounding: w and b rounded to fp32, z = fp32 chain over k ascending, then + b in fp32.  X [S, d] fp32."""
    X = np.asarray(X, dtype=np.float32)
    w32, b32 = np.asarray(w).astype(np.float32), np.float32(b)
    acc = np.zeros(X.shape[0], dtype=np.float32)
    for k in range(X.shape[1]):      # a product and a sum rounded separately: never tighter than the device's fused chain
        acc = (acc + X[:, k] * w32[k]).astype(np.float32)
    return (acc + b32).astype(np.float32)


# ---- the splits ----------------------------------------------------------------------------------------------------------------------
def splits(available, folds, repeat=0, seed_base=0):
    """regression_splits' dealing, written out: the available cases shuffled by torch.randperm under the stated seed, case k of the
    shuffled order going to fold k mod folds; fold f trains on the available cases of the other folds, ascending."""
    available = np.asarray(available, dtype=bool)
    idx = np.nonzero(available)[0]
    g = torch.Generator().manual_seed(int(seed_base) + 1000 * int(folds) + int(repeat))
    order = idx[torch.randperm(idx.size, generator=g).numpy()]
    share = [set(order[f::folds].tolist()) for f in range(folds)]
    return [np.array(sorted(set(idx.tolist()) - share[f]), dtype=np.int64) for f in range(folds)]


# ---- the metrics ---------------------------------------------------------------------------------------------------------------------
def held_out(y, train):
    """The test cases of one (problem, target): y finite and the case outside the training list (indices out of range count for nothing)."""
    y = np.asarray(y)
    mask = np.isfinite(y)
    train = np.asarray(train, dtype=np.int64)
    mask[train[(train >= 0) & (train < y.size)]] = False
    return np.nonzero(mask)[0]


def doubled_ranks(v):
    """R_i = 2 #less + #equal + 1 (#equal counts the case itself; -0 == +0; a NaN is neither less nor equal): twice the average rank."""
    v = np.asarray(v)
    less = (v[None, :] < v[:, None]).sum(1)
    equal = (v[None, :] == v[:, None]).sum(1)
    return (2 * less + equal + 1).astype(np.int64)


def doubled_ranks_sorted(v):
    """The same integers from a sort (for lists too long for the O(n^2) definition).  No NaN among v."""
    v = np.asarray(v) + 0.0                       # -0 -> +0: searchsorted orders by value as well, this only makes it plain
    s = np.sort(v)
    left, right = np.searchsorted(s, v, "left"), np.searchsorted(s, v, "right")
    return (2 * left + (right - left) + 1).astype(np.int64)


def rank_sums(z, y):
    """n, sum Rz, sum Ry, sum Rz^2, sum Ry^2, sum Rz Ry as Python ints."""
    big = len(z) > 4096 and not np.isnan(np.asarray(z, dtype=np.float64)).any()
    rz, ry = (doubled_ranks_sorted(z), doubled_ranks_sorted(y)) if big else (doubled_ranks(z), doubled_ranks(y))
    return [int(len(z)), int(rz.sum()), int(ry.sum()), int((rz * rz).sum()), int((ry * ry).sum()), int((rz * ry).sum())]


def metrics(z, y):
    """[n_test, pearson, spearman, r2, mae, rmse] over the test cases' z (fp32 values) and y, in fp64."""
    z, y = np.asarray(z, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = z.size
    out = np.full(6, np.nan)
    out[0] = n
    if n < 2 or np.isnan(z).any():
        return out
    dz, dy, e = z - z.mean(), y - y.mean(), y - z
    z_varies, y_varies = bool((z != z[0]).any()), bool((y != y[0]).any())
    if z_varies and y_varies:
        out[1] = (dz * dy).sum() / (np.sqrt((dz * dz).sum()) * np.sqrt((dy * dy).sum()))
        s = rank_sums(z, y)
        num = s[0] * s[5] - s[1] * s[2]
        out[2] = num / (np.sqrt(float(s[0] * s[3] - s[1] * s[1])) * np.sqrt(float(s[0] * s[4] - s[2] * s[2])))
    if y_varies:
        out[3] = 1.0 - (e * e).sum() / (dy * dy).sum()
    out[4] = np.abs(e).mean()
    out[5] = np.sqrt((e * e).mean())
    return out


def regress_metrics(Z, Y, train_lists):
    """(metrics [P, A, T, 6] fp64, sums [P, A, T, 6] int64) from Z [P, A, T, S] and Y [S, T]."""
    P, A, T, S = Z.shape
    M, R = np.zeros((P, A, T, 6)), np.zeros((P, A, T, 6), dtype=np.int64)
    for p in range(P):
        for t in range(T):
            test = held_out(Y[:, t], train_lists[p])
            for a in range(A):
                M[p, a, t] = metrics(Z[p, a, t, test], Y[test, t])
                R[p, a, t] = rank_sums(Z[p, a, t, test], Y[test, t])
    return M, R


# ---- inputs shared by the CPU and the GPU file ----------------------------------------------------------------------------------------
def cohort(S, d, T, kind="unit", seed=0, noise=0.3):
    """(X [S, d] fp32 with unit-norm rows, Y [S, T] fp32): "unit" rows are normalised Gaussians, "clustered" rows 8 centres plus 5 %
    scatter; the targets are linear in X plus noise."""
    rng = np.random.default_rng(seed)
    if kind == "clustered":
        X = rng.standard_normal((8, d))[rng.integers(0, 8, S)] + 0.05 * rng.standard_normal((S, d))
    else:
        X = rng.standard_normal((S, d))
    X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
    Y = (X.astype(np.float64) @ rng.standard_normal((d, T)) + noise * rng.standard_normal((S, T))).astype(np.float32)
    return X, Y


def lambda_max(X, idx):
    """The largest eigenvalue of the centred Gram matrix of rows idx."""
    Xc = np.asarray(X, dtype=np.float64)[idx]
    Xc = Xc - Xc.mean(0)
    return float(np.linalg.eigvalsh(Xc @ Xc.T if Xc.shape[0] <= Xc.shape[1] else Xc.T @ Xc)[-1])


def parity(z, z64):
    """max |z - z64| / max |z64| over a cohort: the sibling probes' contract holds it to 1e-3."""
    return float(np.abs(np.asarray(z, dtype=np.float64) - z64).max() / np.abs(z64).max())
