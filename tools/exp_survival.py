"""Times a cross-validated survival probe on the device -- 5 folds x 2 endpoints = 10 ridge Cox fits of 922-923 training rows over
S = 1153 embeddings of d = 512 (an ACROBAT-sized cohort), scoring, concordance and log-rank -- and the same 10 fits by the fp64 damped
Newton reference of tests/_survival_ref.py on the CPU in the same process.  Device figures come from device events around the
repetitions after warm-up; the split by entry point from functional.KernelTimer in a further run.  Prints one JSON line.

    python tools/exp_survival.py [--reps 10]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from madeleine_amd import functional as F  # noqa: E402
from madeleine_amd.survival import GTOL, _problem_table, survival_probe, survival_splits  # noqa: E402
from tests import _survival_ref as R  # noqa: E402

S, D, FOLDS, COST = 1153, 512, 5, 1.0


def cohort():
    """Embeddings, and two endpoints with tied and censored times (closed form): the second has shorter, coarser times and every fifth
    event turned into a censored case."""
    X, t, e = R.recipe(S, D, 0.3, 0.25)
    e = torch.where(e < 0, 1, e)                     # every case has follow-up: 922-923 training rows per fold, as on the manifest
    t2 = torch.ceil(t * 0.75 * 2.0) / 2.0
    e2 = torch.where((torch.arange(S) % 5 == 0) & (e == 1), 0, e)
    return X.float(), {"os": t.float(), "pfs": t2.float()}, {"os": e, "pfs": e2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    X, times, events = cohort()
    Xd = X.cuda()
    probs = [(name, idx) for name in times for idx in survival_splits(events[name], FOLDS)]
    table, n_train = _problem_table([p[1] for p in probs], Xd.device)
    t_dev = torch.stack([times[p[0]] for p in probs]).cuda()
    e_dev = torch.stack([events[p[0]] for p in probs]).to(torch.int32).cuda()
    zero_b = torch.zeros(len(probs), 1, device=Xd.device)

    def device_protocol():
        W, thr, info = F.cox_fit(Xd, t_dev, e_dev, table, n_train, COST, GTOL)
        z = F.probe_scores(Xd, W.unsqueeze(1), zero_b, 2).squeeze(2)
        return W, info, F.survival_metrics(z, t_dev, e_dev, table, n_train, thr)

    for _ in range(3):
        W, info, (c_index, chi2, counts) = device_protocol()
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
    survival_probe(X.numpy(), times, events, folds=FOLDS, cost=COST)      # end to end from host arrays: splits, copies, launches, reads
    torch.cuda.synchronize()
    e2e_ms = (time.perf_counter() - t0) * 1e3
    info, W = info.cpu().numpy(), W.cpu()
    host_s, host_it, worst = 0.0, [], 0.0
    for p, (name, idx) in enumerate(probs):
        t0 = time.perf_counter()
        w64, _, it = R.newton_fit(X[idx].double(), times[name][idx], events[name][idx], COST, tol=1e-10)
        host_s += time.perf_counter() - t0
        host_it.append(it)
        z64 = X.double() @ w64
        worst = max(worst, float((X.double() @ W[p].double() - z64).abs().max() / z64.abs().max()))
    print(json.dumps({
        "problems": len(probs), "S": S, "d": D, "n_train": [int(n_train.min()), int(n_train.max())], "gtol": GTOL,
        "device_ms_per_protocol": round(device_ms, 4), "reps": args.reps, "device_ms_by_entry_point": split,
        "survival_probe_end_to_end_ms": round(e2e_ms, 3),
        "newton_steps": {"min": int(info[:, 0].min()), "max": int(info[:, 0].max()), "mean": round(float(info[:, 0].mean()), 2)},
        "cg_steps": {"min": int(info[:, 3].min()), "max": int(info[:, 3].max()), "mean": round(float(info[:, 3].mean()), 2)},
        "converged": int(info[:, 1].sum()), "mean_c_index": round(float(c_index.mean()), 4),
        "mean_logrank_chi2": round(float(chi2.mean()), 2),
        "host_solver": "torch fp64 damped Newton (tests/_survival_ref.py), relative tol 1e-10",
        "host_fits_ms": round(host_s * 1e3, 2), "host_iterations_mean": round(float(np.mean(host_it)), 1),
        "worst_decision_value_error_vs_host": float("%.3g" % worst)}))


if __name__ == "__main__":
    main()
