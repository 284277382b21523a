"""Measures the device smooth rank against the host function it can replace, on an MI355X, at [300, 512],
[1153, 512] (ACROBAT's cohort) and [20000, 512] seeded gaussian embeddings.  Per shape, after one warm-up call of each leg and with
the legs alternated inside one process:

  1. functional.smooth_rank by device events, split into its stages (Gram, tridiagonalisation, bisection + finish), and the call as a
     whole by a host clock around call + synchronise;
  2. its launch count (2 min(n, d));
  3. utils.smooth_rank_measure (torch.svd on the CPU) on the same matrix by a host clock, with torch's thread count -- without the
     device-to-host copy that the host path also pays;
  4. the relative deviation of the device rank, and of the host function's unrounded value, from the fp64 oracle (numpy's fp64 SVD).

       python tools/exp_rank.py [--steps 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from madeleine_amd import functional as MF  # noqa: E402
from madeleine_amd.utils import smooth_rank_measure  # noqa: E402

SHAPES = [(300, 512), (1153, 512), (20000, 512)]
EPS = 1e-7


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def oracle(E):
    S = np.linalg.svd(E.astype(np.float64), compute_uv=False)
    p = S / np.abs(S).sum() + EPS
    p = p[:E.shape[1]]
    return float(np.exp(-np.sum(p * np.log(p))))


def host_unrounded(E):
    _, S, _ = torch.svd(E)
    p = S / torch.norm(S, p=1) + EPS
    p = p[:E.shape[1]]
    return torch.exp(-torch.sum(p * torch.log(p))).item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("exp_rank.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    report = {"device": torch.cuda.get_device_name(0), "cpu_threads": torch.get_num_threads(), "steps": a.steps, "shapes": []}
    for n, d in SHAPES:
        E_np = np.random.default_rng(n).standard_normal((n, d)).astype(np.float32)
        E_cpu, E = torch.from_numpy(E_np), torch.from_numpy(E_np).to(dev)
        want = oracle(E_np)
        rank, _, _ = MF.smooth_rank_stages(E, EPS)                 # warm-up of both legs
        smooth_rank_measure(E_cpu)
        stages = {"gram": [], "tridiagonal": [], "eigen_finish": []}
        call_ms, cpu_ms = [], []
        for _ in range(a.steps):
            _, _, ms = MF.smooth_rank_stages(E, EPS)
            for k, v in ms.items():
                stages[k].append(v)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r, _ = MF.smooth_rank(E, EPS)
            torch.cuda.synchronize()
            call_ms.append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            smooth_rank_measure(E_cpu)
            cpu_ms.append(1e3 * (time.perf_counter() - t0))
        k = min(n, d)
        row = {"n": n, "d": d, "launches": 2 * k if k >= 2 else 4,
               "device_stage_ms": {s: stats(v) for s, v in stages.items()},
               "device_total_ms": stats([sum(x) for x in zip(*stages.values())]),
               "device_call_and_sync_ms": stats(call_ms), "cpu_svd_ms": stats(cpu_ms),
               "oracle": want, "device_rel_dev": abs(float(rank) - want) / want,
               "cpu_fp32_rel_dev": abs(host_unrounded(E_cpu) - want) / want}
        report["shapes"].append(row)
        print("[%d, %d]: device %.3f ms (Gram %.3f, tridiagonal %.3f, bisection + finish %.3f), call + sync %.3f ms, %d launches; "
              "CPU svd %.1f ms on %d threads; rel. dev. device %.1e, CPU fp32 %.1e"
              % (n, d, row["device_total_ms"]["median"], row["device_stage_ms"]["gram"]["median"],
                 row["device_stage_ms"]["tridiagonal"]["median"], row["device_stage_ms"]["eigen_finish"]["median"],
                 row["device_call_and_sync_ms"]["median"], row["launches"], row["cpu_svd_ms"]["median"], report["cpu_threads"],
                 row["device_rel_dev"], row["cpu_fp32_rel_dev"]), flush=True)
    line = json.dumps(report)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
