"""InfoNCE with explicit negatives: forward + backward times of the HIP path (device events after warm-up) and the rates they imply
from shapes.  Cases: unpaired N = 256, M = 65,536, D = 512 (three 17.2-GFLOP contractions); paired N = 256, M = 1,024, D = 512
(537 MB of negatives: forward reads them once, backward reads them once more and writes dNeg once).  Per-kernel times: run this
under `rocprofv3 --kernel-trace --stats` in a separate pass (--quick keeps that pass short)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from madeleine_amd import InfoNCE  # noqa: E402
from madeleine_amd import functional as MF  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="3 timed iterations (for a profiler pass)")
    a = ap.parse_args()
    iters = 3 if a.quick else a.iters
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    out = {}
    for name, (N, M, D, paired) in {"unpaired_256x65536x512": (256, 65536, 512, False),
                                     "paired_256x1024x512": (256, 1024, 512, True)}.items():
        q = torch.randn(N, D, device=dev, generator=g).requires_grad_()
        p = torch.randn(N, D, device=dev, generator=g).requires_grad_()
        neg = torch.randn(*((N, M, D) if paired else (M, D)), device=dev, generator=g)
        crit = InfoNCE(temperature=0.001, negative_mode="paired" if paired else "unpaired")
        for want_dneg in (False, True):
            neg.requires_grad_(want_dneg)

            def step():
                q.grad = p.grad = neg.grad = None
                crit(q, p, negative_keys=neg).backward()
            for _ in range(a.warmup):
                step()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                step()
            e1.record()
            torch.cuda.synchronize()
            step_ms = e0.elapsed_time(e1) / iters
            MF.TIMER = MF.KernelTimer(only=("infonce_neg_fwd", "infonce_neg_bwd"))
            for _ in range(iters):
                step()
            r = MF.TIMER.report()
            MF.TIMER = None
            fwd, bwd = r["infonce_neg_fwd"][0], r["infonce_neg_bwd"][0]
            nbytes = 4.0 * neg.numel()
            row = {"step_ms": round(step_ms, 4), "fwd_ms": round(fwd, 4), "bwd_ms": round(bwd, 4)}
            if paired:
                row["fwd_TBps"] = round(nbytes / fwd / 1e9, 3)                       # reads the negatives once
                row["bwd_TBps"] = round(nbytes * (2 if want_dneg else 1) / bwd / 1e9, 3)   # reads them again (+ writes dNeg)
            else:
                flop = 2.0 * N * M * D
                row["fwd_TFps"] = round(flop / fwd / 1e9, 2)
                row["bwd_TFps"] = round(flop * (2 if want_dneg else 1) / bwd / 1e9, 2)
            key = "%s_%s" % (name, "dneg" if want_dneg else "nodneg")
            out[key] = row
            print(key, json.dumps(row), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
