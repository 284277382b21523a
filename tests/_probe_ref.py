"""Host side of the linear-probe tests: the closed-form cohorts, an fp64 (or fp32) Newton iteration in the span of the training rows,
and fp64 recounts of the metrics.  Everything here runs on the CPU; nothing of it is shared with the code under test except
probe_splits (the split rule is part of the contract and has its own tests in test_probe_cpu.py)."""
import functools

import torch

# name -> (S, d, C, sep, ldX)
COHORTS = {"A": (160, 64, 2, 0.15, 64), "B": (160, 48, 3, 0.20, 56), "C2": (240, 512, 2, 0.06, 512), "C4": (240, 512, 4, 0.08, 512)}
KS, FOLDS = (1, 10, 25), (0, 1, 2, 3)


def recipe(S, d, C, sep):
    """(X [S, d] fp64, y [S] int64) of the closed-form recipe."""
    i = torch.arange(S, dtype=torch.float64)[:, None]
    j = torch.arange(d, dtype=torch.float64)[None, :]
    y = (7 * torch.arange(S) + torch.arange(S) // 5) % C
    X = sep * torch.sin(0.9 * j + 2.1 * y[:, None].double()) + torch.sin(0.37 * i * (j + 1) + 0.11 * i * i) + 0.5 * torch.cos(1.3 * i + 0.7 * j)
    return X, y


def primal_grad_inf(Xt, yt, W, b, C, cost=1.0):
    """inf-norm of the fp64 gradient of the primal objective at (W [cols, d], b [cols]) over the training rows Xt, yt."""
    Xt, W, b = Xt.double(), W.double(), b.double()
    F = Xt @ W.T + b
    if C == 2:
        R = torch.sigmoid(F) - yt.double()[:, None]
    else:
        R = torch.softmax(F, 1) - torch.nn.functional.one_hot(yt.long(), C).double()
    gW = cost * R.T @ Xt + W
    gb = cost * R.sum(0)
    return float(max(gW.abs().max(), gb.abs().max()))


def newton_fit(Xt, yt, C, cost=1.0, dtype=torch.float64, tol=1e-10, max_iter=40):
    """Newton on (A, b) with W = A^T Xt, in `dtype`.  Returns (W [cols, d], b [cols], own residual, iterations); the iterate with the
    smallest own residual is returned (in fp32 the iteration stalls above tol).  The multinomial system is singular along the common
    shift of b: the step is pinned to sum(db) = 0, and b is returned with zero mean."""
    Xt = Xt.to(dtype)
    n, cols = Xt.shape[0], (1 if C == 2 else C)
    G = Xt @ Xt.T
    Y = yt.to(dtype)[:, None] if C == 2 else torch.nn.functional.one_hot(yt.long(), C).to(dtype)
    A, b = torch.zeros(n, cols, dtype=dtype), torch.zeros(cols, dtype=dtype)
    eye_n, eye_c = torch.eye(n, dtype=dtype), torch.eye(cols, dtype=dtype)

    def state(A, b):
        F = G @ A + b
        if C == 2:
            P = torch.sigmoid(F)
            obj = cost * (torch.nn.functional.softplus(F) - Y * F).sum()
        else:
            P = torch.softmax(F, 1)
            obj = -cost * (torch.log_softmax(F, 1) * Y).sum()
        return P, obj + 0.5 * (A * (G @ A)).sum()

    best = None
    P, obj = state(A, b)
    for it in range(max_iter + 1):
        R = P - Y
        U = cost * R + A
        gb = cost * R.sum(0)
        res = float(max((Xt.T @ U).abs().max(), gb.abs().max()))
        if best is None or res < best[2]:
            best = (A.clone(), b.clone(), res, it)
        if res < tol or it == max_iter or (dtype != torch.float64 and it >= best[3] + 3):
            break
        D = (P * (1 - P))[:, :, None] if C == 2 else torch.diag_embed(P) - P[:, :, None] * P[:, None, :]      # [n, cols, cols]
        J = torch.zeros(n * cols + cols, n * cols + cols, dtype=dtype)
        T = cost * D[:, :, None, :] * G[:, None, :, None]                                                      # [i, c, j, c']
        J[:n * cols, :n * cols] = T.reshape(n * cols, n * cols) + torch.kron(eye_n, eye_c)
        J[:n * cols, n * cols:] = cost * D.reshape(n * cols, cols)
        J[n * cols:, :n * cols] = T.sum(0).reshape(cols, n * cols)
        J[n * cols:, n * cols:] = cost * D.sum(0) + (1.0 if cols > 1 else 0.0)      # + 1 1^T pins sum(db) = 0: the system is regular
        step = torch.linalg.solve(J, -torch.cat([U.reshape(-1), gb]))
        dA, db = step[:n * cols].reshape(n, cols), step[n * cols:]
        t = 1.0
        while True:
            P2, obj2 = state(A + t * dA, b + t * db)
            if obj2 <= obj or t < 1e-3:
                break
            t *= 0.5
        A, b, P, obj = A + t * dA, b + t * db, P2, obj2
    A, b, res, it = best
    return (A.T @ Xt), (b - b.mean() if cols > 1 else b), res, it


def confusion(z, y, test, C):
    """[C, C] int64 (row = truth) over the cases of the boolean mask `test`; z [S, cols]."""
    # z == 0 is class 0; the lowest index among equal maxima
    pred = (z[:, 0] > 0).long() if C == 2 else (z == z.max(1, keepdim=True).values).long().cumsum(1).eq(1).long().argmax(1)
    out = torch.zeros(C, C, dtype=torch.int64)
    for t_, p_ in zip(y[test].tolist(), pred[test].tolist()):
        out[t_, p_] += 1
    return out


def pair_auc(score, pos, neg):
    """Mann-Whitney with ties counted 1/2 over the (pos, neg) pairs, in fp64; NaN without a pair."""
    sp, sn = score[pos].double(), score[neg].double()
    if sp.numel() == 0 or sn.numel() == 0:
        return float("nan")
    d = sp[:, None] - sn[None, :]
    return float(((d > 0).double().sum() + 0.5 * (d == 0).double().sum()) / d.numel())


def auc(z, y, test, C):
    """roc_auc_score of the test cases: by z for C == 2, one-vs-rest macro average by log_softmax(z)[c] otherwise."""
    if C == 2:
        return pair_auc(z[:, 0], test & (y == 1), test & (y == 0))
    ls = torch.log_softmax(z.double(), 1)
    per = [pair_auc(ls[:, c], test & (y == c), test & (y != c) & (y >= 0)) for c in range(C)]
    return sum(per) / C      # NaN if any class has no pair


def close_pair_share(score, pos, neg, gap):
    """Share of the (pos, neg) pairs whose score gap is below `gap`."""
    d = (score[pos].double()[:, None] - score[neg].double()[None, :]).abs()
    return float((d < gap).double().mean()) if d.numel() else 0.0


def test_mask(y, train_idx):
    m = y >= 0
    m[train_idx.long()] = False
    return m


@functools.lru_cache(maxsize=None)
def cohort(name):
    """The cohort, its problems (k, fold, train indices) and the fp64 optimum of each, computed once per session.
    Returns dict(X fp64, y int64, C, ldX, problems=[dict(k, fold, idx, W64, b64, z64, r32)])."""
    from madeleine_amd.probe import probe_splits
    S, d, C, sep, ldX = COHORTS[name]
    X, y = recipe(S, d, C, sep)
    X32 = X.float()
    problems = []
    for k in KS:
        for fold in FOLDS:
            idx = probe_splits(y, k, fold)
            Xt, yt = X32[idx].double(), y[idx]      # the optimum of the problem the device is given: the fp32-rounded features
            W, b, res, _ = newton_fit(Xt, yt, C)
            assert res < 1e-10, (name, k, fold, res)
            W32, b32, _, _ = newton_fit(Xt, yt, C, dtype=torch.float32)
            problems.append(dict(k=k, fold=fold, idx=idx, W64=W, b64=b, z64=X32.double() @ W.T + b,
                                 r32=primal_grad_inf(Xt, yt, W32, b32, C)))
    return dict(X=X, y=y, C=C, ldX=ldX, problems=problems)
