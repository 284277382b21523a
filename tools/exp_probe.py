"""Times the reference's whole linear-probing protocol on the device -- 3 tasks x k in (1, 10, 25) x 10 folds = 90 binary fits over
S = 1153 embeddings of d = 512 (an ACROBAT-sized cohort), scoring and metrics -- and the same 90 fits by a host solver in the same
process (scipy L-BFGS where scipy imports, else an fp64 Newton iteration in torch).  Device figures come from device events after
warm-up; the split by entry point from functional.KernelTimer in a further run.  Prints one JSON line.

    python tools/exp_probe.py [--reps 10]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from madeleine_amd import functional as F  # noqa: E402
from madeleine_amd.probe import _problem_table, linear_probe, probe_splits  # noqa: E402

S, D, KS, FOLDS = 1153, 512, (1, 10, 25), 10


def cohort():
    """Embeddings with three weakly separable binary tasks (closed form, fp64 -> fp32)."""
    i = np.arange(S, dtype=np.float64)[:, None]
    j = np.arange(D, dtype=np.float64)[None, :]
    tasks = {t: ((m * np.arange(S) + np.arange(S) // 5) % 2) for t, m in (("er", 7), ("pr", 3), ("her2", 5))}
    X = np.sin(0.37 * i * (j + 1) + 0.11 * i * i) + 0.5 * np.cos(1.3 * i + 0.7 * j)
    for n, y in enumerate(tasks.values()):
        X = X + 0.06 * np.sin(0.9 * j + 2.1 * y[:, None] + n)
    return X.astype(np.float32), tasks


def host_fit(Xt, yt, gtol=1e-4):
    """One fit on the host in fp64; returns (iterations, seconds)."""
    s = 2.0 * yt - 1.0
    t0 = time.perf_counter()
    try:
        from scipy.optimize import minimize

        def fun(v):
            m = s * (Xt @ v[:-1] + v[-1])
            r = -s / (1.0 + np.exp(m))
            return np.logaddexp(0.0, -m).sum() + 0.5 * v[:-1] @ v[:-1], np.append(Xt.T @ r + v[:-1], r.sum())

        res = minimize(fun, np.zeros(Xt.shape[1] + 1), jac=True, method="L-BFGS-B", options={"gtol": gtol, "maxiter": 10000})
        it = int(res.nit)
    except ImportError:
        X_, y_ = torch.from_numpy(Xt), torch.from_numpy(yt)
        G, a, b, it = X_ @ X_.T, torch.zeros(len(yt), dtype=torch.float64), torch.zeros((), dtype=torch.float64), 0
        for it in range(50):
            p = torch.sigmoid(G @ a + b)
            u, w = p - y_ + a, p * (1 - p)
            if max(float((X_.T @ u).abs().max()), abs(float((p - y_).sum()))) <= gtol:
                break
            J = torch.zeros(len(yt) + 1, len(yt) + 1, dtype=torch.float64)
            J[:-1, :-1], J[:-1, -1], J[-1, :-1], J[-1, -1] = torch.eye(len(yt)) + w[:, None] * G, w, w @ G, w.sum()
            step = torch.linalg.solve(J, -torch.cat([u, (p - y_).sum()[None]]))
            a, b = a + step[:-1], b + step[-1]
    return it, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    X, tasks = cohort()
    Xd = torch.from_numpy(X).cuda()
    probs = [(torch.from_numpy(y), probe_splits(y, k, f)) for y in tasks.values() for k in KS for f in range(FOLDS)]
    table, n_train = _problem_table([p[1] for p in probs], Xd.device)
    y_dev = torch.stack([p[0] for p in probs]).to(torch.int32).cuda()

    def device_protocol():
        W, b, info = F.probe_fit(Xd, y_dev, table, n_train, 2)
        conf, auc = F.probe_metrics(F.probe_scores(Xd, W, b, 2), y_dev, table, n_train, 2)
        return info, auc

    for _ in range(3):
        info, auc = device_protocol()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.reps):
        device_protocol()
    e1.record()
    torch.cuda.synchronize()
    device_ms = e0.elapsed_time(e1) / args.reps
    F.TIMER = F.KernelTimer()
    for _ in range(args.reps):
        device_protocol()
    split = {k: round(v[0], 4) for k, v in F.TIMER.report().items()}
    F.TIMER = None
    t0 = time.perf_counter()
    res = linear_probe(X, tasks)                    # end to end from host arrays: splits, copies, launches, the two reads
    torch.cuda.synchronize()
    e2e_ms = (time.perf_counter() - t0) * 1e3
    info = info.cpu().numpy()
    host = [host_fit(X[idx.numpy()].astype(np.float64), y[idx].numpy().astype(np.float64)) for y, idx in probs]
    print(json.dumps({
        "problems": len(probs), "S": S, "d": D, "device_ms_per_protocol": round(device_ms, 4), "reps": args.reps,
        "device_ms_by_entry_point": split, "linear_probe_end_to_end_ms": round(e2e_ms, 3),
        "newton_steps": {"min": int(info[:, 0].min()), "max": int(info[:, 0].max()), "mean": round(float(info[:, 0].mean()), 2)},
        "cg_steps": {"min": int(info[:, 3].min()), "max": int(info[:, 3].max()), "mean": round(float(info[:, 3].mean()), 2)},
        "converged": int(info[:, 1].sum()), "mean_auc": round(float(np.mean([r["auc"].mean() for r in res.values()])), 4),
        "host_solver": "scipy L-BFGS-B fp64" if "scipy" in sys.modules else "torch fp64 Newton",
        "host_fits_ms": round(sum(h[1] for h in host) * 1e3, 2), "host_iterations_mean": round(float(np.mean([h[0] for h in host])), 1)}))


if __name__ == "__main__":
    main()
