"""Host side of the survival-probe tests: closed-form cohorts with tied and censored follow-up times, a damped Newton iteration on the
primal ridge Cox objective (Breslow ties) in fp64 or fp32, and direct O(S^2) numpy recounts of Harrell's concordance and the median-split
log-rank sums.  Everything here runs on the CPU and is written from the definitions (risk sets as boolean masks, no sorting): nothing of
it is shared with the code under test."""
import functools

import numpy as np
import torch

# name -> (S, d, ldX, sep, scale, cost, training sizes)
COHORTS = {
    "A": (330, 4, 8, 1.5, 1.0, 1.0, (1, 63, 64, 65, 255, 256, 257)),
    "B": (330, 512, 512, 0.3, 0.25, 4.0, (1, 64, 65, 257)),
    "L": (1300, 64, 72, 0.4, 1.0, 1.0, (1024,)),
}


def _frac(x):
    return x - torch.floor(x)


def recipe(S, d, sep, scale=1.0):
    """(X [S, d] fp64, time [S] fp64 on a grid of 0.25, event [S] int64) in closed form, X scaled by `scale`.  A latent risk s in
    [-1, 1) moves the features along cos(0.9 j) and shortens the time; 30 % of the cases are censored before their event, every 13th
    has no follow-up (-1).  The grid makes tie groups, among them ties between an event and a censored case."""
    i = torch.arange(S, dtype=torch.float64)
    j = torch.arange(d, dtype=torch.float64)[None, :]
    s = 2.0 * _frac(i * 0.6180339887498949) - 1.0
    X = scale * (sep * s[:, None] * torch.cos(0.9 * j) + torch.sin(0.37 * i[:, None] * (j + 1) + 0.11 * (i * i)[:, None])
                 + 0.5 * torch.cos(1.3 * i[:, None] + 0.7 * j))
    u = _frac(i * 0.7548776662466927 + 0.31).clamp_min(1e-3)
    T = -torch.log(u) * torch.exp(-2.0 * s)
    n = torch.arange(S)
    censored = (3 * n + n // 7) % 10 < 3
    T = torch.where(censored, T * (0.3 + 0.6 * _frac(i * 0.41421356237)), T)
    time = torch.ceil(T * 4.0).clamp_min(1.0) / 4.0
    event = torch.where(censored, 0, 1)
    event[n % 13 == 5] = -1
    return X, time, event


# ---- the objective and its optimum -------------------------------------------------------------------------------------------------
def _risk(time):
    """R[i, j] = 1 where j is in the risk set of i: t_j >= t_i."""
    return (time[None, :] >= time[:, None])


def cox_objective(Xt, time, event, w, cost=1.0):
    """F(w) = cost * sum_{events i} [log sum_{j in R_i} exp(x_j . w) - x_i . w] + 1/2 |w|^2 and its gradient, in the dtype of Xt."""
    dt = Xt.dtype
    ev = event.to(dt)
    R = _risk(time).to(dt)
    f = Xt @ w
    m = f.max()
    e = torch.exp(f - m)
    S0 = R @ e
    loss = (ev * (torch.log(S0) + m - f)).sum()
    A = R.T @ (ev / S0)
    r = -ev + e * A
    return cost * loss + 0.5 * (w * w).sum(), cost * (Xt.T @ r) + w


def primal_grad_inf(Xt, time, event, w, cost=1.0):
    """inf-norm of the fp64 gradient of F at w over the training rows."""
    return float(cox_objective(Xt.double(), time.double(), event, w.double(), cost)[1].abs().max())


def newton_fit(Xt, time, event, cost=1.0, dtype=torch.float64, tol=1e-12, max_iter=60):
    """Damped Newton on the primal objective in `dtype`: the full d x d Hessian, a backtracking (Armijo) line search.  Returns (w [d],
    own gradient inf-norm, iterations); the iterate with the smallest own gradient is returned (in fp32 the iteration stalls above tol).
    tol is relative to the gradient at w = 0."""
    Xt, time = Xt.to(dtype), time.to(dtype)
    d = Xt.shape[1]
    ev = event.to(dtype)
    R = _risk(time).to(dtype)
    w = torch.zeros(d, dtype=dtype)
    eye = torch.eye(d, dtype=dtype)
    best, g0 = None, None
    for it in range(max_iter + 1):
        obj, g = cox_objective(Xt, time, event, w, cost)
        res = float(g.abs().max())
        g0 = res if g0 is None else g0
        if best is None or res < best[1]:
            best = (w.clone(), res, it)
        if res <= tol * g0 or it == max_iter or (dtype != torch.float64 and it >= best[2] + 3):
            break
        f = Xt @ w
        e = torch.exp(f - f.max())
        S0 = R @ e
        A = R.T @ (ev / S0)
        M = R @ (e[:, None] * Xt)                                # row i: sum_{k in R_i} e_k x_k
        H = eye + cost * (Xt.T @ ((e * A)[:, None] * Xt) - M.T @ ((ev / (S0 * S0))[:, None] * M))
        step = torch.linalg.solve(H, -g)
        slope, t = float(g @ step), 1.0
        while True:
            obj2 = cox_objective(Xt, time, event, w + t * step, cost)[0]
            if bool(obj2 <= obj + 1e-4 * t * slope) or t < 1e-6:
                break
            t *= 0.5
        w = w + t * step
    return best


# ---- the metrics, recounted from their definitions ---------------------------------------------------------------------------------
def test_mask(event, train_idx):
    m = np.isin(np.asarray(event), (0, 1))
    m[np.asarray(train_idx, dtype=np.int64)] = False
    return m


def concordance(z, time, event, test):
    """(numerator, comparable pairs) of Harrell's C over the cases of the mask `test`: pair (i, j) is comparable iff event_i = 1 and
    (t_i < t_j, or t_i = t_j and event_j = 0); it counts 2 if z_i > z_j, 1 if z_i = z_j."""
    z, t, e = np.asarray(z)[test], np.asarray(time)[test], np.asarray(event)[test]
    comp = (e[:, None] == 1) & ((t[:, None] < t[None, :]) | ((t[:, None] == t[None, :]) & (e[None, :] == 0)))
    num = 2 * int((comp & (z[:, None] > z[None, :])).sum()) + int((comp & (z[:, None] == z[None, :])).sum())
    return num, int(comp.sum())


def c_index(num, comparable):
    return num / (2.0 * comparable) if comparable else float("nan")


def logrank(z, thr, time, event, test):
    """The median-split log-rank sums over the cases of `test`, written per individual: dict(O_E, V, chi2, n_test, n_high,
    events_low, events_high).  High risk: z > thr."""
    z, t, e = np.asarray(z)[test], np.asarray(time)[test], np.asarray(event)[test]
    high = z > thr
    O_E, V = 0.0, 0.0
    for i in np.nonzero(e == 1)[0]:
        at_risk = t >= t[i]
        n, h = int(at_risk.sum()), int((at_risk & high).sum())
        dd = int(((e == 1) & (t == t[i])).sum())
        O_E += (1.0 if high[i] else 0.0) - h / n
        if n > 1:
            V += (h / n) * (1.0 - h / n) * (n - dd) / (n - 1)
    return dict(O_E=O_E, V=V, chi2=(O_E * O_E / V if V > 0 else float("nan")), n_test=int(test.sum()), n_high=int(high.sum()),
                events_low=int(((e == 1) & ~high).sum()), events_high=int(((e == 1) & high).sum()))


def counts_row(z, thr, time, event, test):
    """The six integers of mdl_surv_metrics' counts_out for one problem, and (c_index, chi2)."""
    num, comp = concordance(z, time, event, test)
    lr = logrank(z, thr, time, event, test)
    return [num, comp, lr["n_test"], lr["n_high"], lr["events_low"], lr["events_high"]], c_index(num, comp), lr["chi2"]


def close_pairs(z64, time, event, test, gap):
    """Number of comparable pairs whose fp64 score gap is below `gap`."""
    z, t, e = np.asarray(z64)[test], np.asarray(time)[test], np.asarray(event)[test]
    comp = (e[:, None] == 1) & ((t[:, None] < t[None, :]) | ((t[:, None] == t[None, :]) & (e[None, :] == 0)))
    return int((comp & (np.abs(z[:, None] - z[None, :]) < gap)).sum())


def train_lists(event, sizes, seed=0):
    """One training list per size: the first n of a seeded permutation of the cases with follow-up (a different one per list)."""
    labeled = torch.nonzero(torch.as_tensor(event) >= 0)[:, 0]
    out = []
    for q, n in enumerate(sizes):
        g = torch.Generator().manual_seed(seed + 97 * q + n)
        out.append(labeled[torch.randperm(labeled.numel(), generator=g)[:n]])
    return out


@functools.lru_cache(maxsize=None)
def cohort(name):
    """The cohort, its problems and the fp64 optimum of each, computed once per session.  Returns dict(X fp64, time fp32, event int64,
    ldX, cost, problems=[dict(idx, w64, z64, g0, r32)]): g0 the fp64 gradient norm at w = 0, r32 the fp64 gradient norm at what the same
    iteration reaches in fp32."""
    S, d, ldX, sep, scale, cost, sizes = COHORTS[name]
    X, time, event = recipe(S, d, sep, scale)
    X32 = X.float()
    problems = []
    for idx in train_lists(event, sizes):
        Xt, tt, et = X32[idx].double(), time[idx], event[idx]      # the optimum of the problem the device is given: fp32 features
        w, res, _ = newton_fit(Xt, tt, et, cost)
        g0 = primal_grad_inf(Xt, tt, et, torch.zeros(d), cost)
        assert res <= 1e-10 * max(g0, 1e-300), (name, idx.numel(), res, g0)
        w32 = newton_fit(Xt, tt, et, cost, dtype=torch.float32)[0]
        problems.append(dict(idx=idx, w64=w, z64=X32.double() @ w, g0=g0, r32=primal_grad_inf(Xt, tt, et, w32, cost)))
    return dict(X=X, time=time.float(), event=event, ldX=ldX, cost=cost, problems=problems)
