"""Measures the patch contributions of a probe's decision on the shape of `exp_attention.py`: --cases H&E bags
of --rows rows, H = 4 heads.  Device events after warm-up, the legs alternated inside one process.

  0. `tools/micro/hbm_rate quick` in a child of its own, when that binary has been built
     (hipcc --offload-arch=gfx950 -O3 tools/micro/hbm_rate.hip -o tools/micro/hbm_rate), else "not measured".
  1. The kernel alone (functional.attn_contrib) on E [cases * rows, 4 * 512], fp32 and bf16, C in {1, 8}: ms and the bytes it moves by
     the contract (E once, attn, the output) over its time; next to a torch einsum restatement on the same tensors.
  2. functional.contrib_stats on the [T, 8] result.
  3. DeviceSlideStore.contributions (C = 8, topk = 16) against DeviceSlideStore.attention (topk = 16) over the same cohort: bags/s.

       python tools/exp_contrib.py [--cases 48] [--rows 30000] [--steps 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench as BN  # noqa: E402
from madeleine_amd import MADELEINE, DeviceSlideStore  # noqa: E402
from madeleine_amd import functional as MF  # noqa: E402

H, W = 4, MF.HID


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def timed(f):
    """device milliseconds of f() between two events on the current stream"""
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    out = f()
    ev1.record()
    ev1.synchronize()
    del out
    return ev0.elapsed_time(ev1)


def einsum_restatement(E, attn, U):
    """what a user writes today, given E: widen, contract per head, weigh, add the heads"""
    T, C = E.shape[0], U.shape[0]
    per_head = torch.einsum("thw,chw->thc", E.view(T, H, W).float(), U.view(C, H, W))
    return (per_head * attn[:, :, None]).sum(1)


def alternate(legs, steps):
    for f in legs.values():
        f()
    ms = {name: [] for name in legs}
    for i in range(max(1, steps)):
        for name in (sorted(legs) if i % 2 == 0 else sorted(legs, reverse=True)):
            ms[name].append(timed(legs[name]))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=48)
    ap.add_argument("--rows", type=int, default=30000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--topk", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, rows, k = a.cases, a.rows, a.topk
    T = n * rows
    res, lines = {"geometry": {"cases": n, "rows_per_bag": rows, "heads": H, "T": T}}, []

    hbm = os.path.join(ROOT, "tools", "micro", "hbm_rate")
    if os.path.exists(hbm):                                   # a child of its own, before this process opens the device
        p = subprocess.run([hbm, "quick"], capture_output=True, text=True, timeout=300)
        res["hbm_rate_quick"] = p.stdout.strip().splitlines()[-12:]
    else:
        res["hbm_rate_quick"] = "not measured"
    lines.append("hbm_rate quick: %s" % (res["hbm_rate_quick"] if isinstance(res["hbm_rate_quick"], str) else ""))
    if not isinstance(res["hbm_rate_quick"], str):
        lines.extend("    " + ln for ln in res["hbm_rate_quick"])

    dev = torch.device("cuda:0")
    torch.manual_seed(7)

    # ---- 1. the kernel alone, and the einsum restatement on the same tensors
    attn = torch.rand(T, H, device=dev)
    res["kernel"] = {}
    for dtype, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
        E = torch.randn(T, H * W, device=dev).to(dtype)
        for C in (1, 8):
            U = torch.randn(C, H * W, device=dev)
            ms = alternate({"hip": lambda: MF.attn_contrib(E, attn, U), "einsum": lambda: einsum_restatement(E, attn, U)}, a.steps)
            nbytes = float(T) * (H * W * E.element_size() + 4 * H + 4 * C)
            hip, ein = statistics.median(ms["hip"]), statistics.median(ms["einsum"])
            diff = float((MF.attn_contrib(E, attn, U) - einsum_restatement(E, attn, U)).abs().max())
            res["kernel"]["%s_C%d" % (tag, C)] = {"hip_ms": stats(ms["hip"]), "einsum_ms": stats(ms["einsum"]), "bytes": nbytes,
                                                 "hip_tb_per_s": nbytes / hip / 1e9, "einsum_over_hip": ein / hip, "max_abs_diff": diff}
            lines.append("attn_contrib %s C %d: median %.3f ms (min %.3f max %.3f) = %.2f TB/s over %.2f GB; einsum %.3f ms = %.1f x; "
                         "max |difference| %.2e" % (tag, C, hip, min(ms["hip"]), max(ms["hip"]), nbytes / hip / 1e9, nbytes / 1e9, ein,
                                                    ein / hip, diff))
        if dtype == torch.float32:
            # ---- 2. the statistics of the [T, 8] result
            c8 = MF.attn_contrib(E, attn, U)
            cu = torch.arange(n + 1, device=dev, dtype=torch.int64) * rows
            ms = alternate({"stats": lambda: MF.contrib_stats(c8, cu)}, a.steps)
            res["contrib_stats"] = {"ms": stats(ms["stats"])}
            lines.append("contrib_stats [%d, 8] over %d bags: median %.3f ms (min %.3f max %.3f)"
                         % (T, n, statistics.median(ms["stats"]), min(ms["stats"]), max(ms["stats"])))
            del c8
        del E
    del attn
    torch.cuda.empty_cache()

    # ---- 3. the whole read-out against the attention read-out
    g = torch.Generator().manual_seed(7)
    D = 512
    base = torch.randn(rows + n, D, generator=g)
    st = DeviceSlideStore([[base[c:c + rows]] for c in range(n)], ["case%05d" % c for c in range(n)], ["HE"], dev)
    torch.manual_seed(42)
    model = MADELEINE(BN.make_cfg(2, D)).to(dev).eval()
    Wp, bp = torch.randn(8, 512, generator=g) / 16, torch.randn(8, generator=g)
    feeds = {"contributions": lambda: st.contributions(model, Wp, bp, topk=k), "attention": lambda: st.attention(model, topk=k)}
    ms = alternate(feeds, max(1, a.steps // 2))
    res["store"] = {name: {"ms": stats(v), "bags_per_s_median": n / statistics.median(v) * 1e3} for name, v in ms.items()}
    for name, v in sorted(ms.items()):
        lines.append("store.%-13s median %.1f ms = %.1f bags/s (min %.1f max %.1f ms) over %d bags of %d rows"
                     % (name, statistics.median(v), n / statistics.median(v) * 1e3, min(v), max(v), n, rows))
    out = st.contributions(model, Wp, bp)
    gap = (out["decision"] - (out["stats"][:, 0] + out["const"])).abs()
    denom = out["stats"][:, 1] - out["stats"][:, 2] + out["const"].abs()
    res["store"]["completeness_max"] = float((gap / denom).max())
    lines.append("completeness: max |decision - (sum + const)| / (sum |c| + |const|) = %.2e" % res["store"]["completeness_max"])
    for ln in lines:
        print(ln)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
