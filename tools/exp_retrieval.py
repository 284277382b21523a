"""Measures the retrieval kernels on an MI355X.  Device events after one warm-up call of each leg, the legs
alternated inside one process:

  1. functional.retrieval (paired, k = 10, cosine) on closed-form cohorts of [1153, 512] (ACROBAT's size) and [16384, 512], against what
     a user writes in torch on the same tensors: F.normalize -> mm -> topk -> two comparisons against the diagonal (which forms the
     [S, S] matrix, 1 GiB at 16384, through the library GEMM this package does not otherwise use);
  2. the fraction of the 157.3 TFLOP/s exact-fp32 MFMA peak the whole call reaches (2 S^2 d useful flop);
  3. the largest |pair_sim - fp64 cosine| of each cohort beside tol(d) = (d + 4) 2^-23;
  4. cross_stain_retrieval on a store the size of `exp_store.py --embed`'s: --cases cases x 2 stains of --rows rows x 512 (host clock
     around a synchronise: it embeds both stains and reads its metrics back).

       python tools/exp_retrieval.py [--steps 5] [--cases 48] [--rows 30000] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench as BN  # noqa: E402
from madeleine_amd import MADELEINE, DeviceSlideStore, cross_stain_retrieval  # noqa: E402
from madeleine_amd import functional as MF  # noqa: E402

SHAPES = [(1153, 512), (16384, 512)]
PEAK_TF = 157.3
K = 10


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def timed(f):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    out = f()
    ev1.record()
    ev1.synchronize()
    del out
    return ev0.elapsed_time(ev1)


def field(rows, d, a, b, c, seed):
    i = np.arange(rows, dtype=np.float64)[:, None]
    j = np.arange(d, dtype=np.float64)[None, :]
    x = np.sin(i * a + j * b + seed) * c
    return x - np.floor(x) - 0.5


def cohort(n, d, noise=3.5, seed=0.25):
    base = field(n, d, 12.9898, 78.233, 43758.5453, seed)
    return base.astype(np.float32), (base + noise * field(n, d, 4.1414, 269.5, 183.3, seed + 1.0)).astype(np.float32)


def torch_path(Q, Kg):
    S = torch.nn.functional.normalize(Q) @ torch.nn.functional.normalize(Kg).t()
    val, idx = torch.topk(S, K, dim=1)
    diag = S.diagonal().unsqueeze(1)
    return (S > diag).sum(1), (S == diag).sum(1) - 1, val, idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--cases", type=int, default=48)
    ap.add_argument("--rows", type=int, default=30000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("exp_retrieval.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    report = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "k": K, "shapes": []}
    for n, d in SHAPES:
        Qn, Kn = cohort(n, d)
        Q, Kg = torch.from_numpy(Qn).to(dev), torch.from_numpy(Kn).to(dev)
        r = MF.retrieval(Q, Kg, k=K)                # warm-up of both legs
        t = torch_path(Q, Kg)
        agree = bool(torch.equal(r.greater.long() + r.equal.long(), t[0] + t[1]))      # near-ties may differ: reported, not asserted
        unit = lambda X: X.astype(np.float64) / np.maximum(np.sqrt((X.astype(np.float64) ** 2).sum(1, keepdims=True)), 1e-12)
        pair64 = (unit(Qn) * unit(Kn)).sum(1)
        err = float(np.abs(r.pair_sim.cpu().numpy().astype(np.float64) - pair64).max())
        del t
        ours, theirs = [], []
        for _ in range(a.steps):
            ours.append(timed(lambda: MF.retrieval(Q, Kg, k=K)))
            theirs.append(timed(lambda: torch_path(Q, Kg)))
        ms = statistics.median(ours)
        row = {"n": n, "d": d, "chunks": MF.retrieval_chunks(n, n)[0], "retrieval_ms": stats(ours), "torch_ms": stats(theirs),
               "tflops": 2.0 * n * n * d / (ms * 1e9), "fraction_of_fp32_mfma_peak": 2.0 * n * n * d / (ms * 1e9) / PEAK_TF,
               "max_pair_sim_error": err, "tol": (d + 4) * 2.0 ** -23, "ranks_agree_with_torch": agree,
               "median_rank": float((1 + r.greater + r.equal).float().median())}
        report["shapes"].append(row)
        print("[%d, %d]: retrieval %.3f ms (%d chunks, %.1f TF, %.0f %% of %.1f), torch normalize-mm-topk-compare %.3f ms; "
              "max |pair_sim - s64| %.2e (tol %.2e); ranks agree with torch: %s"
              % (n, d, ms, row["chunks"], row["tflops"], 100 * row["fraction_of_fp32_mfma_peak"], PEAK_TF,
                 statistics.median(theirs), err, row["tol"], agree), flush=True)
        del Q, Kg, r
    # ---- cross_stain_retrieval on a store of the embed measurement's size
    n, rows, D = a.cases, a.rows, 512
    g = torch.Generator().manual_seed(7)
    base = torch.randn(rows + 2 * n, D, generator=g)
    bags = [[base[c:c + rows], base[n + c:n + c + rows]] for c in range(n)]      # overlapping windows: distinct bags, one allocation
    st = DeviceSlideStore(bags, ["case%05d" % c for c in range(n)], ["HE", "HER2"], dev)
    torch.manual_seed(42)
    model = MADELEINE(BN.make_cfg(2, D)).to(dev).eval()
    cross_stain_retrieval(st, model)
    torch.cuda.synchronize()
    wall = []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        res = cross_stain_retrieval(st, model)
        torch.cuda.synchronize()
        wall.append(1e3 * (time.perf_counter() - t0))
    report["cross_stain"] = {"cases": n, "rows_per_bag": rows, "stains": 1, "ms": stats(wall), "bags_per_s": 2 * n / (statistics.median(wall) * 1e-3),
                             "metrics": res["HER2"]["he_to_stain"]}
    print("cross_stain_retrieval, %d cases x 2 stains of %d rows: %.1f ms (%.0f bags/s)"
          % (n, rows, statistics.median(wall), report["cross_stain"]["bags_per_s"]), flush=True)
    line = json.dumps(report)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
