"""Times the cross-validated full-label linear probe on the device -- fit / scores / metrics by device events -- for three protocols:
"binary": 3 binary tasks x 5 folds over S = 1153 embeddings of d = 512 (an ACROBAT-sized cohort), "four_class": one 4-class task x 5
folds over the same matrix, "large": one binary task x 5 folds at S = 16384 (13,107 training rows per fold, the largest the entry points
accept).  Reports the Newton and CG step counts per fit, and the same fits by an fp64 Newton iteration on the host (torch) in the same
process.  Prints one JSON line per protocol.

    python tools/exp_probe_cv.py [--reps 5] [--only binary four_class large]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from madeleine_amd import functional as F  # noqa: E402
from madeleine_amd.probe import _problem_table, cv_splits, linear_probe_cv  # noqa: E402

D, FOLDS = 512, 5


def cohort(S, tasks):
    """Embeddings [S, D] with weakly separable tasks (closed form, fp64 -> fp32); tasks: name -> (multiplier, classes)."""
    i = np.arange(S, dtype=np.float64)[:, None]
    j = np.arange(D, dtype=np.float64)[None, :]
    labels = {t: ((m * np.arange(S) + np.arange(S) // 5) % C) for t, (m, C) in tasks.items()}
    X = np.sin(0.37 * i * (j + 1) + 0.11 * i * i) + 0.5 * np.cos(1.3 * i + 0.7 * j)
    for n, y in enumerate(labels.values()):
        X = X + 0.06 * np.sin(0.9 * j + 2.1 * y[:, None] + n)
    return X.astype(np.float32), labels


def host_fit(Xt, yt, C, gtol=1e-4):
    """One fit on the host: fp64 Newton on the primal unknowns [W | b], full steps halved on the objective.  Returns (iterations, s)."""
    t0 = time.perf_counter()
    X = torch.from_numpy(Xt).double()
    n, d = X.shape
    cols = 1 if C == 2 else C
    Xa = torch.cat([X, torch.ones(n, 1, dtype=torch.float64)], 1)
    y = torch.from_numpy(yt)
    Y = y.double()[:, None] if C == 2 else torch.nn.functional.one_hot(y.long(), C).double()
    pen = torch.ones(d + 1, dtype=torch.float64)
    pen[d] = 0.0
    T = torch.zeros(cols, d + 1, dtype=torch.float64)

    def state(T):
        Fv = Xa @ T.T
        if C == 2:
            return torch.sigmoid(Fv), (torch.nn.functional.softplus(Fv) - Y * Fv).sum() + 0.5 * (T * T * pen).sum()
        return torch.softmax(Fv, 1), -(torch.log_softmax(Fv, 1) * Y).sum() + 0.5 * (T * T * pen).sum()

    P, obj = state(T)
    it = 0
    for it in range(50):
        G = (P - Y).T @ Xa + T * pen
        if float(G.abs().max()) <= gtol:
            break
        m = d + 1
        H = torch.zeros(cols, m, cols, m, dtype=torch.float64)
        for c in range(cols):
            for c2 in range(c, cols):
                w = P[:, 0] * (1 - P[:, 0]) if C == 2 else P[:, c] * ((1.0 if c == c2 else 0.0) - P[:, c2])
                H[c, :, c2, :] = H[c2, :, c, :] = (Xa * w[:, None]).T @ Xa
            H[c, :, c, :] += torch.diag(pen)
        if cols > 1:
            H[:, d, :, d] += 1.0                    # pins the common shift of b
        step = torch.linalg.solve(H.reshape(cols * m, cols * m), -G.reshape(-1)).reshape(cols, m)
        t = 1.0
        while True:
            P2, obj2 = state(T + t * step)
            if obj2 <= obj or t < 1e-3:
                break
            t *= 0.5
        T, P, obj = T + t * step, P2, obj2
    return it, time.perf_counter() - t0


def protocol(name, S, tasks, reps):
    X, labels = cohort(S, tasks)
    C = next(iter(tasks.values()))[1]
    Xd = torch.from_numpy(X).cuda()
    probs = [(torch.from_numpy(y), idx) for y in labels.values() for idx in cv_splits(y, FOLDS)]
    table, n_train = _problem_table([p[1] for p in probs], Xd.device)
    y_dev = torch.stack([p[0] for p in probs]).to(torch.int32).cuda()

    def device_protocol():
        W, b, info = F.logit_fit(Xd, y_dev, table, n_train, C)
        conf, auc = F.logit_metrics(F.probe_scores(Xd, W, b, C), y_dev, table, n_train, C)
        return info, auc

    info, auc = device_protocol()                   # warm-up
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        device_protocol()
    e1.record()
    torch.cuda.synchronize()
    device_ms = e0.elapsed_time(e1) / reps
    F.TIMER = F.KernelTimer()
    for _ in range(reps):
        device_protocol()
    split = {k: round(v[0], 4) for k, v in F.TIMER.report().items()}
    F.TIMER = None
    t0 = time.perf_counter()
    res = linear_probe_cv(X, labels, folds=FOLDS)   # end to end from host arrays: splits, copies, launches, the two reads
    torch.cuda.synchronize()
    e2e_ms = (time.perf_counter() - t0) * 1e3
    info = info.cpu().numpy()
    host = [host_fit(X[idx.numpy()], y[idx].numpy(), C) for y, idx in probs]
    print(json.dumps({
        "protocol": name, "problems": len(probs), "S": S, "d": D, "C": C, "n_train": [int(n_train.min()), int(n_train.max())],
        "device_ms_per_protocol": round(device_ms, 3), "reps": reps, "device_ms_by_entry_point": split,
        "linear_probe_cv_end_to_end_ms": round(e2e_ms, 3),
        "newton_steps": [int(v) for v in info[:, 0]], "cg_steps": [int(v) for v in info[:, 3]], "converged": int(info[:, 1].sum()),
        "residual_max": float(info[:, 2].max()), "mean_auc": round(float(np.mean([r["auc"].mean() for r in res.values()])), 4),
        "host_solver": "torch fp64 Newton", "host_fits_ms": round(sum(h[1] for h in host) * 1e3, 2),
        "host_iterations_mean": round(float(np.mean([h[0] for h in host])), 1)}), flush=True)


PROTOCOLS = {"binary": (1153, {"er": (7, 2), "pr": (3, 2), "her2": (5, 2)}), "four_class": (1153, {"grade": (7, 4)}),
             "large": (16384, {"er": (7, 2)})}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", nargs="+", default=list(PROTOCOLS), choices=list(PROTOCOLS))
    args = ap.parse_args()
    for name in args.only:
        protocol(name, *PROTOCOLS[name], args.reps)


if __name__ == "__main__":
    main()
