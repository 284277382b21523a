#!/usr/bin/env python
"""What does the optimiser step cost?  Five variants on the config-2 model's real parameter set (every tensor of MADELEINE(c2) that
takes a gradient in that config: all but the token_projector), timed with device events, in alternating order:

    a  torch.optim.AdamW(fused=True)
    b  clip_grad_norm_(foreach=True) + torch.optim.AdamW(fused=True)
    c  madeleine_amd.AdamW(skip_nonfinite=False)                        update + commit
    d  madeleine_amd.AdamW()                                            statistics + update + commit
    e  madeleine_amd.AdamW(max_grad_norm=...)                           the same launches, clipping

Each round times `--steps` back-to-back steps of one variant between two events (so a variant whose host side is slower than its
kernels is charged for it); rounds alternate forwards / backwards through the variants.  Printed: per variant the median, minimum and
maximum over the rounds of the time per step, and the spread of (b), the yardstick for "e is no slower than b"; then the kernels' own
time per step of each variant from a short pass under torch's profiler.
Usage: python tools/exp_adamw.py [--rounds 6] [--steps 40] [--warmup 10] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench as BN  # noqa: E402
import madeleine_amd  # noqa: E402
from madeleine_amd import MADELEINE  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--prof-steps", type=int, default=20)
    ap.add_argument("--only", default="abcde", help="variants to run (a profiler pass over two of them)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    _B, M, _N, Dm, _got, stain = BN.CONFIGS["c2"]
    torch.manual_seed(42)
    model = MADELEINE(BN.make_cfg(M, Dm), stain_encoding=stain).to(dev)
    params = [p for n, p in model.named_parameters() if not n.startswith("token_projector.")]
    gen = torch.Generator(device=dev).manual_seed(1)
    for p in params:
        p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-2
    numel = sum(p.numel() for p in params)
    norm = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in params)))
    # half the norm: the first step of (b) clips, every later one multiplies by max_norm / (max_norm + 1e-6) -- the same kernels each step
    max_norm = 0.5 * norm

    torch_opt = torch.optim.AdamW(params, lr=1e-4, fused=True)
    ours = {"c": madeleine_amd.AdamW(params, lr=1e-4, skip_nonfinite=False), "d": madeleine_amd.AdamW(params, lr=1e-4),
            "e": madeleine_amd.AdamW(params, lr=1e-4, max_grad_norm=max_norm)}

    def step_b():
        torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=True)
        torch_opt.step()
    steps = {"a": torch_opt.step, "b": step_b, "c": ours["c"].step, "d": ours["d"].step, "e": ours["e"].step}
    steps = {k: f for k, f in steps.items() if k in a.only}
    for f in steps.values():
        for _ in range(a.warmup):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in steps}
    for r in range(a.rounds):
        order = sorted(steps) if r % 2 == 0 else sorted(steps, reverse=True)
        for k in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            f = steps[k]
            e0.record()
            for _ in range(a.steps):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / a.steps)
    res = {"tensors": len(params), "elements": numel, "steps_per_variant": a.rounds * a.steps, "max_norm": max_norm,
           "skipped": {k: o.skipped_steps() for k, o in ours.items()},
           "us_per_step": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}}
    lines = ["%d tensors, %d elements, %d steps per variant after %d warm-up steps" % (len(params), numel, a.rounds * a.steps, a.warmup)]
    for k, v in sorted(times.items()):
        lines.append("  %s  median %8.1f us  min %8.1f  max %8.1f   (%.0f GB/s at 32 B/element)"
                     % (k, statistics.median(v), min(v), max(v), 32.0 * numel / statistics.median(v) * 1e-3))
    if "b" in times:
        res["b_spread_us"] = max(times["b"]) - min(times["b"])
        lines.append("  spread of b over its rounds: %.1f us" % res["b_spread_us"])
    # the kernels' own time (the rounds above charge a variant for its host side too): torch's profiler over a few steps of each variant
    try:
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile
        res["device_us_per_step"] = {}
        for k, f in sorted(steps.items()):
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                for _ in range(a.prof_steps):
                    f()
                torch.cuda.synchronize()
            kernels = {e.key: e.self_device_time_total / a.prof_steps for e in prof.key_averages()
                       if e.device_type == DeviceType.CUDA and e.self_device_time_total > 0 and not e.key.startswith("Optimizer.")}
            res["device_us_per_step"][k] = {"total": sum(kernels.values()), "kernels": kernels}
            lines.append("  %s  kernels %7.1f us per step: %s" % (k, sum(kernels.values()), ", ".join(
                "%s %.1f" % (n.replace("void ", "").replace("at::native::", "").replace("(anonymous namespace)::", "")[:32], t) for n, t in sorted(kernels.items(), key=lambda kv: -kv[1]))))
    except Exception as e:      # noqa: BLE001 -- a build of torch without the device tracer: the rounds above stand on their own
        lines.append("  (no per-kernel times: %s)" % e)
    text = "\n".join(lines)
    print(text)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n" + json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
