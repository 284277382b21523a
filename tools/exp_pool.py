#!/usr/bin/env python3
"""Pooling forward / scores-backward alone at BASELINE config-2 geometry (64 bags x 4096 tokens x 2048 ch), timed with events over
many launches: A/B of kernel variants (MADELEINE_LIB=tools/ab/<name>.so).  Prints ms and the algorithmic HBM rate of each."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from madeleine_amd import functional as MF  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=40)
ap.add_argument("--bags", type=int, default=64)
ap.add_argument("--tokens", type=int, default=4096)
a = ap.parse_args()
dev = torch.device("cuda:0")
BM, N, H = a.bags, a.tokens, 4
g = torch.Generator(device=dev).manual_seed(0)
E2 = torch.randn(BM * N, H * 512, device=dev, generator=g)
scores = torch.randn(BM * N, H, device=dev, generator=g)
dpool = torch.randn(BM, H * 512, device=dev, generator=g)


def timed(fn):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / a.iters


nbytes = BM * N * H * 512 * 4


def report(what, ms, out):
    print(f"{what} {ms:.4f} ms  {nbytes / ms / 1e9:.3f} TB/s  checksum {out.double().sum().item():.10e}")


for name, Ex, fwd, bwd in (
    ("image", MF.split_image(E2), MF.pool_fwd_img_raw, MF.pool_dscores_img_raw),
    ("fp32", E2, MF.pool_fwd_raw, None),
    ("bf16", E2.bfloat16(), MF.pool_fwd_raw, None),
):
    out = fwd(Ex, scores, BM, N, None, N)
    report(f"pool_fwd[{name}]", timed(lambda: fwd(Ex, scores, BM, N, None, N)), out[0])
    if bwd is not None:
        pooled, m, l = out
        ds = torch.empty_like(scores)
        report(f"pool_dscores[{name}]", timed(lambda: bwd(Ex, scores, pooled, m, l, dpool, ds, 0, BM, N, None, N)), ds)

# the ragged half-bag views of the same rows (fp32): every bag shuffled in place and cut in two; the backward is the scores pass
perm = torch.cat([b * N + torch.randperm(N, device=dev, generator=g) for b in range(BM)]).to(torch.int32)
vcu = (torch.arange(2 * BM + 1, device=dev, dtype=torch.int64) * N) // 2
half = N - N // 2
out = MF.pool_rview_fwd_raw(E2, scores, BM, perm, vcu, half)
report("pool_rview_fwd[fp32]", timed(lambda: MF.pool_rview_fwd_raw(E2, scores, BM, perm, vcu, half)), out[0])
dpool2 = torch.randn(BM, 2, H * 512, device=dev, generator=g)
ds = torch.zeros_like(scores)
ms = timed(lambda: MF.pool_rview_bwd_raw(E2, scores, *out, dpool2, None, ds, BM, perm, vcu, half))
report("pool_rview_dscores[fp32]", ms, ds)
