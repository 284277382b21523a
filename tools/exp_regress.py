"""Times the regression probe (madeleine_amd.regress, include/madeleine_amd_regress.h) at the shapes of DESIGN 3.22, all with d = 512,
5 folds and A = 8 penalties: S = 1153 for T = 1 and T = 1000 targets and S = 16384 for T = 1 (folds of 922 and 13107 training rows > d:
the covariance form), and S = 600 for T = 1000 (480 training rows <= d: the Gram form).  Fit, scores and metrics are timed by device
events after one warm-up run at the same shape; the torch restatement is warmed by one run at the same shape as well.  The same run
times three restatements of the whole evaluation:
  torch   on the device in fp64: torch.linalg.cholesky / cholesky_solve per (fold, penalty), argsort-based ranks (ties not averaged)
  numpy   an fp64 loop on the CPU (the BLAS threads the environment allows; the figures of DESIGN 3.22 are from 16)
  sklearn sklearn.linear_model.Ridge(solver="cholesky") per (fold, penalty) with numpy metrics, where scikit-learn is importable

    python tools/exp_regress.py [--json OUT.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from madeleine_amd import functional as F          # noqa: E402
from madeleine_amd.regress import regression_splits  # noqa: E402
from madeleine_amd.survival import _problem_table  # noqa: E402

ALPHAS = (0.01, 0.03, 0.1, 0.3, 1.0, 3.0, 10.0, 30.0)


def cohort(S, d, T, seed=0):
    g = torch.Generator().manual_seed(seed)
    X = torch.nn.functional.normalize(torch.randn(S, d, generator=g), dim=1)
    Y = X @ torch.randn(d, T, generator=g) + 0.3 * torch.randn(S, T, generator=g)
    return X.contiguous(), Y.contiguous()


def device_run(X, Y, table, n_train):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ev[0].record()
    W, b, info = F.ridge_fit(X, Y, table, n_train, ALPHAS)
    ev[1].record()
    Z = F.ridge_scores(X, W, b)
    ev[2].record()
    M = F.regress_metrics(Z, Y, table, n_train)
    ev[3].record()
    torch.cuda.synchronize()
    return M, [ev[i].elapsed_time(ev[i + 1]) for i in range(3)], bool((info[..., 0] > 0).all())


def _pearson_rows(a, b, xp):
    a = a - a.mean(-1, keepdims=True) if xp is np else a - a.mean(-1, keepdim=True)
    b = b - b.mean(-1, keepdims=True) if xp is np else b - b.mean(-1, keepdim=True)
    return (a * b).sum(-1) / xp.sqrt((a * a).sum(-1) * (b * b).sum(-1))


def torch_run(X, Y, lists):
    """[P, A, T, 3] Pearson, Spearman (ordinal ranks), R^2 on the device in fp64."""
    X64, Y64 = X.double(), Y.double()
    S = X.shape[0]
    out = []
    for idx in lists:
        idx = idx.to(X.device)
        test = torch.ones(S, dtype=torch.bool, device=X.device)
        test[idx] = False
        xm, ym = X64[idx].mean(0), Y64[idx].mean(0)
        Xc, Yc = X64[idx] - xm, Y64[idx] - ym
        gram = Xc.shape[0] <= Xc.shape[1]
        K = Xc @ Xc.T if gram else Xc.T @ Xc
        rhs = Yc if gram else Xc.T @ Yc
        yt = Y64[test].T                                              # [T, n_test]
        ry = torch.argsort(torch.argsort(yt, dim=-1), dim=-1).double()
        per_alpha = []
        for alpha in ALPHAS:
            L = torch.linalg.cholesky(K + alpha * torch.eye(K.shape[0], dtype=torch.float64, device=X.device))
            c = torch.cholesky_solve(rhs, L)
            W = Xc.T @ c if gram else c                               # [d, T]
            z = (X64[test] @ W + (ym - xm @ W)).T                     # [T, n_test]
            rz = torch.argsort(torch.argsort(z, dim=-1), dim=-1).double()
            r2 = 1.0 - ((yt - z) ** 2).sum(-1) / ((yt - yt.mean(-1, keepdim=True)) ** 2).sum(-1)
            per_alpha.append(torch.stack([_pearson_rows(z, yt, torch), _pearson_rows(rz, ry, torch), r2], -1))
        out.append(torch.stack(per_alpha))
    return torch.stack(out)


def numpy_run(X, Y, lists, fit=None):
    """The same on the CPU in fp64; fit(Xtrain, Ytrain, alpha) -> (W [d, T], b [T]) replaces the closed form (scikit-learn)."""
    X64, Y64 = X.double().numpy(), Y.double().numpy()
    S = X64.shape[0]
    out = np.zeros((len(lists), len(ALPHAS), Y64.shape[1], 3))
    for p, idx in enumerate(lists):
        idx = idx.numpy()
        test = np.ones(S, dtype=bool)
        test[idx] = False
        xm, ym = X64[idx].mean(0), Y64[idx].mean(0)
        Xc, Yc = X64[idx] - xm, Y64[idx] - ym
        gram = Xc.shape[0] <= Xc.shape[1]
        if fit is None:
            K = Xc @ Xc.T if gram else Xc.T @ Xc
            rhs = Yc if gram else Xc.T @ Yc
        yt = Y64[test].T
        ry = np.argsort(np.argsort(yt, -1), -1).astype(np.float64)
        for a, alpha in enumerate(ALPHAS):
            if fit is None:
                c = np.linalg.solve(K + alpha * np.eye(K.shape[0]), rhs)
                W = Xc.T @ c if gram else c
                b = ym - xm @ W
            else:
                W, b = fit(X64[idx], Y64[idx], alpha)
            z = (X64[test] @ W + b).T
            rz = np.argsort(np.argsort(z, -1), -1).astype(np.float64)
            out[p, a, :, 0] = _pearson_rows(z, yt, np)
            out[p, a, :, 1] = _pearson_rows(rz, ry, np)
            out[p, a, :, 2] = 1.0 - ((yt - z) ** 2).sum(-1) / ((yt - yt.mean(-1, keepdims=True)) ** 2).sum(-1)
    return out


def _sklearn_fit():
    try:
        from sklearn.linear_model import Ridge
    except ImportError:
        return None

    def fit(Xt, Yt, alpha):
        m = Ridge(alpha=alpha, solver="cholesky").fit(Xt, Yt)
        return m.coef_.T, m.intercept_
    return fit


def _wall(fn, sync=False):
    t0 = time.perf_counter()
    out = fn()
    if sync:
        torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("exp_regress: needs a ROCm device")
    rows = []
    for S, d, T in ((1153, 512, 1), (1153, 512, 1000), (16384, 512, 1), (600, 512, 1000)):
        Xh, Yh = cohort(S, d, T)
        lists = regression_splits(np.ones(S, dtype=bool), folds=5)
        X, Y = Xh.cuda(), Yh.cuda()
        table, n_train = _problem_table(lists, X.device)
        device_run(X, Y, table, n_train)                              # warm-up: module load, allocator
        M, (t_fit, t_scores, t_metrics), ok = device_run(X, Y, table, n_train)
        torch_run(X, Y, lists)                                        # warm-up at the timed shape, as for the device path
        torch.cuda.synchronize()
        Tt, t_torch = _wall(lambda: torch_run(X, Y, lists), sync=True)
        Nn, t_numpy = _wall(lambda: numpy_run(Xh, Yh, lists))
        sk = _sklearn_fit()
        t_sklearn = _wall(lambda: numpy_run(Xh, Yh, lists, sk))[1] if sk else None
        dev = M[..., [1, 2, 3]].cpu().numpy()
        row = dict(S=S, d=d, T=T, folds=5, A=len(ALPHAS), n_train=int(n_train.max()), form="gram" if int(n_train.max()) <= d else "covariance",
                   factorised=ok, fit_ms=t_fit, scores_ms=t_scores, metrics_ms=t_metrics, device_ms=t_fit + t_scores + t_metrics,
                   torch_ms=t_torch, numpy_ms=t_numpy, sklearn_ms=t_sklearn, numpy_threads=torch.get_num_threads(),
                   max_abs_diff_pearson_r2_vs_numpy=float(np.abs(dev[..., [0, 2]] - Nn[..., [0, 2]]).max()),
                   max_abs_diff_torch_vs_numpy=float(np.abs(Tt.cpu().numpy() - Nn).max()))
        rows.append(row)
        print(json.dumps(row), flush=True)
    print("%6s %5s %5s %11s | %9s %9s %9s %9s | %9s %9s %9s" % ("S", "d", "T", "form", "fit ms", "scores", "metrics", "device", "torch",
                                                                 "numpy", "sklearn"))
    for r in rows:
        print("%6d %5d %5d %11s | %9.2f %9.2f %9.2f %9.2f | %9.2f %9.2f %9s" % (
            r["S"], r["d"], r["T"], r["form"], r["fit_ms"], r["scores_ms"], r["metrics_ms"], r["device_ms"], r["torch_ms"], r["numpy_ms"],
            "-" if r["sklearn_ms"] is None else "%.2f" % r["sklearn_ms"]))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
