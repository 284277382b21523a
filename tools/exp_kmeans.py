#!/usr/bin/env python
"""Measures k-means over the slide store at --cases bags x --rows rows x 512, k in {16, 64, 256}, for an fp32 and a
bf16 store.  Measurement only: no test runs this.  Every GPU step is a child process of its own under its own timeout, and the first
one that fails, faults or runs out of time ends the run: nothing more is started on the device after it.

  0. `tools/micro/hbm_rate quick` in a child of its own, when that binary has been built
     (hipcc --offload-arch=gfx950 -O3 tools/micro/hbm_rate.hip -o tools/micro/hbm_rate), else "not measured".
  1. per (store dtype, k), by device events after a warm-up, the legs alternated: functional.kmeans_assign (ms, TB/s over the rows read
     once, TF over 2 T k D), functional.kmeans_update (ms, TB/s over the rows read once), functional.kmeans_hist (ms), and a torch
     restatement on the same device and rows, its assign alone (X @ C.T -> argmax) and one Lloyd step (-> index_add_; in row blocks, so that [T, k] fits
     beside the store; the 16-bit store is widened block by block as a user would).  functional.kmeans_seed once (k centres, 2 launches
     each).

       python tools/exp_kmeans.py [--cases 48] [--rows 30000] [--steps 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
D = 512
STEP_TIMEOUT = 240          # seconds per child


def leg(dtype_name, k, cases, rows, steps):
    import torch
    from madeleine_amd import cluster
    from madeleine_amd import functional as MF
    dev = torch.device("cuda:0")
    dtype = {"fp32": torch.float32, "bf16": torch.bfloat16}[dtype_name]
    T = cases * rows
    g = torch.Generator(device=dev).manual_seed(1)
    X = torch.empty(T, D, device=dev, dtype=dtype)
    for a in range(0, T, rows):                                # (no fp32 copy of a 16-bit store at any time)
        X[a:a + rows] = (torch.randn(rows, D, device=dev, generator=g) + torch.linspace(-3, 3, D, device=dev)).to(dtype)
    off = torch.arange(cases + 1, dtype=torch.int64) * rows
    src = cluster.RowSource(X, off.to(dev), list(range(cases)), [rows] * cases, off[:-1])
    C = src.rows_at(torch.arange(k) * (T // k))
    labels, dist, stats = MF.kmeans_assign(*src.args(), C)

    def timed(f):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        out = f()
        ev1.record()
        ev1.synchronize()
        del out
        return ev0.elapsed_time(ev1)

    def restatement():
        sums, cnt = torch.zeros(k, D, device=dev), torch.zeros(k, device=dev)
        hn = 0.5 * (C * C).sum(1)
        for a in range(0, T, rows):
            xb = X[a:a + rows].float()
            lab = (xb @ C.T - hn).argmax(1)
            sums.index_add_(0, lab, xb)
            cnt.index_add_(0, lab, torch.ones(rows, device=dev))
        return sums / cnt.clamp(min=1)[:, None]

    def restatement_assign():
        hn = 0.5 * (C * C).sum(1)
        return torch.cat([(X[a:a + rows].float() @ C.T - hn).argmax(1) for a in range(0, T, rows)])

    ws_a = MF._ws_for("mdl_kmeans_assign_ws_bytes", dev, src.n_chunks, k, D)
    ws_u = MF._ws_for("mdl_kmeans_update_ws_bytes", dev, T, k, D)
    legs = {"assign": lambda: MF.kmeans_assign(*src.args(), C, labels, dist, stats, ws_a),
            "update": lambda: MF.kmeans_update(*src.args(False), labels, C, None, None, ws_u),
            "hist": lambda: MF.kmeans_hist(labels, src.cu, k),
            "torch": restatement, "torch_assign": restatement_assign}
    for f in legs.values():
        f()
    ms = {n: [] for n in legs}
    for i in range(max(1, steps)):
        for n in (sorted(legs) if i % 2 == 0 else sorted(legs, reverse=True)):
            ms[n].append(timed(legs[n]))
    u = torch.rand(k, device=dev, dtype=torch.float64)
    seed_ms = timed(lambda: MF.kmeans_seed(*src.args(), u))
    nbytes = float(T) * D * X.element_size()
    med = {n: statistics.median(v) for n, v in ms.items()}
    res = {"dtype": dtype_name, "k": k, "T": T, "ms": {n: {"median": med[n], "min": min(v), "max": max(v), "n": len(v)} for n, v in ms.items()},
           "assign_tb_per_s": nbytes / med["assign"] / 1e9, "assign_tf": 2.0 * T * k * D / med["assign"] / 1e9,
           "update_tb_per_s": nbytes / med["update"] / 1e9, "torch_over_assign_update": med["torch"] / (med["assign"] + med["update"]),
           "torch_assign_over_assign": med["torch_assign"] / med["assign"],
           "seed_ms_once": seed_ms}
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=48)
    ap.add_argument("--rows", type=int, default=30000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", nargs=2, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg[0], int(a.leg[1]), a.cases, a.rows, a.steps)
    res, lines = {"geometry": {"cases": a.cases, "rows_per_bag": a.rows, "D": D}, "legs": []}, []
    hbm = os.path.join(ROOT, "tools", "micro", "hbm_rate")
    if os.path.exists(hbm):
        p = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT), hbm, "quick"], capture_output=True, text=True)
        if p.returncode != 0:
            print("hbm_rate quick ended with status %d: nothing more is started" % p.returncode)
            return p.returncode
        res["hbm_rate_quick"] = p.stdout.strip().splitlines()[-12:]
        lines.extend(["hbm_rate quick:"] + ["    " + ln for ln in res["hbm_rate_quick"]])
    else:
        res["hbm_rate_quick"] = "not measured"
        lines.append("hbm_rate quick: not measured")
    for dtype in ("fp32", "bf16"):
        for k in (16, 64, 256):
            cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--leg", dtype, str(k),
                   "--cases", str(a.cases), "--rows", str(a.rows), "--steps", str(a.steps)]
            p = subprocess.run(cmd, capture_output=True, text=True)
            out = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not out:
                print("\n".join(lines))
                print("the step %s k %d ended with status %d: nothing more is started\n%s" % (dtype, k, p.returncode, p.stderr[-2000:]))
                return p.returncode or 1
            r = json.loads(out[-1][7:])
            res["legs"].append(r)
            m = r["ms"]
            lines.append("%s k %3d: assign %.3f ms (min %.3f max %.3f) = %.2f TB/s, %.1f TF; update %.3f ms = %.2f TB/s; hist %.3f ms; "
                         "torch assign %.3f ms = %.2f x assign; torch step %.3f ms = %.2f x assign + update; seed once %.1f ms"
                         % (dtype, k, m["assign"]["median"], m["assign"]["min"], m["assign"]["max"], r["assign_tb_per_s"], r["assign_tf"],
                            m["update"]["median"], r["update_tb_per_s"], m["hist"]["median"], m["torch_assign"]["median"], r["torch_assign_over_assign"], m["torch"]["median"],
                            r["torch_over_assign_update"], r["seed_ms_once"]))
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
