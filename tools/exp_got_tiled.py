"""Forward + backward time and peak device memory of the tiled GOT class (functional.got_tiled) against a torch fp32 restatement of the
reference algorithm (madeleine/utils/loss.py:278-302: bmm products, autograd through every IPOT iteration) on the same GPU.

    python tools/exp_got_tiled.py [--shapes 4x1024x128,1x2048x128,1x4096x128,4x512x512] [--reps 3]

Prints one JSON line per shape and implementation.  Library GEMMs are used by the restatement only."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def torch_got(v, q):
    from tests.test_got_tiled_gpu import got_parts64   # the restatement is dtype-agnostic: run in fp32 here
    return got_parts64(v, q).sum()


def run(fn, v, q, reps):
    dev = v.device
    times = []
    for r in range(reps + 1):
        vd, qd = v.clone().requires_grad_(), q.clone().requires_grad_()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        loss = fn(vd, qd)
        e1.record()
        loss.backward()
        e2.record()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(dev) - base
        if r:
            times.append((e0.elapsed_time(e1), e1.elapsed_time(e2)))
        del loss, vd, qd
        torch.cuda.empty_cache()
    fwd = min(t[0] for t in times)
    bwd = min(t[1] for t in times)
    return fwd, bwd, peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4x1024x128,1x2048x128,1x4096x128,4x512x512")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true", help="time the tiled class only")
    a = ap.parse_args()
    from madeleine_amd import functional as MF
    dev = torch.device("cuda:0")
    for sh in a.shapes.split(","):
        k, n, d = (int(x) for x in sh.split("x"))
        g = torch.Generator(device=dev).manual_seed(0)
        v = torch.rand(k, n, d, device=dev, generator=g) * 2 - 1
        q = torch.rand(k, n, d, device=dev, generator=g) * 2 - 1 + 0.7 * v
        impls = [("tiled", lambda x, y: MF.got_tiled(x, y).sum())]
        if not a.no_torch:
            impls.append(("torch_fp32", torch_got))
        for name, fn in impls:
            try:
                fwd, bwd, peak = run(fn, v, q, a.reps)
                rec = {"impl": name, "k": k, "n": n, "d": d, "fwd_ms": round(fwd, 3), "bwd_ms": round(bwd, 3),
                       "total_ms": round(fwd + bwd, 3), "peak_gb": round(peak / 2 ** 30, 3)}
            except torch.cuda.OutOfMemoryError:
                rec = {"impl": name, "k": k, "n": n, "d": d, "error": "out of memory"}
                torch.cuda.empty_cache()
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
