"""Measures the device heatmaps on the README cohort: --cases H&E bags of --rows rows x 512, H = 4, fp32 store and
model, coordinates on a jittered grid with 50 % overlap, ds = ps / 4, sigma = 2 canvas pixels.  Device events after warm-up, the legs
alternated inside one process.

  1. DeviceSlideStore.heatmaps (percentile, heads 'all') next to DeviceSlideStore.attention over the same cohort.
  2. functional.heat_render alone, and its stages by device events recorded between the launches of one call
     (functional.heat_render_stages -> mdl_heat_render_marked): clear (memset + tile table), accumulate, the row pass, the column pass
     with level and colour -- at sigma 2 and at r = 0, whose column pass is level + colour alone and whose difference is the taps --
     with the bytes each moves by the contract over its time, next to `tools/micro/hbm_rate quick` of the same run when that binary
     has been built (hipcc --offload-arch=gfx950 -O3 tools/micro/hbm_rate.hip -o tools/micro/hbm_rate), else "not measured".
  3. The same images by the numpy reference of tests/_heat_ref.py on the CPU (ONE bag, one channel; times bags x channels is the
     extrapolation) and by a torch-on-device restatement (index_add_ over footprint offsets + conv2d in float64, per bag), with the
     largest difference of its level from the exact one.

       python tools/exp_heatmap.py [--cases 48] [--rows 30000] [--steps 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench as BN  # noqa: E402
from madeleine_amd import MADELEINE, DeviceSlideStore  # noqa: E402
from madeleine_amd import functional as MF  # noqa: E402
from madeleine_amd import heatmap as HM  # noqa: E402
from tests import _heat_ref as HR  # noqa: E402

PS = 256


def timed(f):
    """device milliseconds of f() between two events on the current stream"""
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    out = f()
    ev1.record()
    ev1.synchronize()
    del out
    return ev0.elapsed_time(ev1)


def alternate(legs, steps):
    for f in legs.values():
        f()
    ms = {name: [] for name in legs}
    for i in range(max(1, steps)):
        for name in (sorted(legs) if i % 2 == 0 else sorted(legs, reverse=True)):
            ms[name].append(timed(legs[name]))
    return {name: statistics.median(v) for name, v in ms.items()}, ms


def grid_coords(rows, rng):
    """rows patches on a near-square grid of stride PS / 2 (50 % overlap), every corner jittered by up to PS / 8"""
    side = int(np.ceil(np.sqrt(rows)))
    i = np.arange(rows)
    return np.stack([(i % side) * (PS // 2), (i // side) * (PS // 2)], 1) + rng.integers(0, PS // 8, (rows, 2))


def torch_restatement(xy, values, ps, ds, W, H, taps):
    """One bag, all channels, on the device: the footprint as the (ps / ds + 1)^2 offsets of a patch's first pixel (the contract's
    footprint is one pixel narrower where the corner is aligned: this restatement is approximate there), index_add_ of value and
    count, conv2d of both with the taps, the quotient."""
    C = values.shape[1]
    k = ps // ds + 1
    px = torch.div(xy, ds, rounding_mode="floor").long()
    oy, ox = torch.meshgrid(torch.arange(k, device=xy.device), torch.arange(k, device=xy.device), indexing="ij")
    X, Y = px[:, 0:1] + ox.reshape(1, -1), px[:, 1:2] + oy.reshape(1, -1)
    ok = (X < W) & (Y < H)
    flat = (Y * W + X)[ok]
    S = torch.zeros(C, H * W, dtype=torch.float64, device=xy.device)
    N = torch.zeros(H * W, dtype=torch.float64, device=xy.device)
    rows = torch.arange(xy.shape[0], device=xy.device)[:, None].expand(-1, k * k)[ok]
    S.index_add_(1, flat, values.double().t()[:, rows])
    N.index_add_(0, flat, torch.ones_like(flat, dtype=torch.float64))
    t = taps.to(xy.device).double() / 4096.0
    planes = torch.cat([S.view(C, 1, H, W), N.view(1, 1, H, W)])
    r = (t.numel() - 1) // 2
    planes = torch.nn.functional.conv2d(planes, t.view(1, 1, 1, -1), padding=(0, r))
    planes = torch.nn.functional.conv2d(planes, t.view(1, 1, -1, 1), padding=(r, 0))
    return planes[:C, 0] / planes[C:, 0].clamp(min=1e-300), N.view(H, W) > 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=48)
    ap.add_argument("--rows", type=int, default=30000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res, lines = {"geometry": {"cases": a.cases, "rows_per_bag": a.rows, "heads": 4, "ps": PS, "ds": PS // 4, "sigma": 2.0}}, []

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
    n, rows, D, ds = a.cases, a.rows, 512, PS // 4
    g = torch.Generator().manual_seed(7)
    base = torch.randn(rows + n, D, generator=g)
    rng = np.random.default_rng(7)
    coords = [[grid_coords(rows, rng)] for _ in range(n)]
    st = DeviceSlideStore([[base[c:c + rows]] for c in range(n)], ["case%05d" % c for c in range(n)], ["HE"], dev, coords=coords,
                          patch_size=PS)
    torch.manual_seed(42)
    model = MADELEINE(BN.make_cfg(2, D)).to(dev).eval()

    # ---- 1. the whole call next to the read-out it starts with
    med, ms = alternate({"heatmaps": lambda: st.heatmaps(model, heads="all", downsample=ds, sigma=2.0),
                         "attention": lambda: st.attention(model)}, a.steps)
    res["store"] = {k: {"median_ms": med[k], "min_ms": min(ms[k]), "max_ms": max(ms[k])} for k in med}
    for k in sorted(med):
        lines.append("store.%-10s median %.2f ms (min %.2f max %.2f) over %d bags of %d rows" % (k, med[k], min(ms[k]), max(ms[k]), n, rows))
    lines.append("heatmaps - attention = %.2f ms = %.0f images/s (4 channels a bag)" % (med["heatmaps"] - med["attention"],
                                                                                     4 * n / (med["heatmaps"] - med["attention"]) * 1e3))

    # ---- 2. the render call and its parts
    att = st.attention(model)
    cu, values = att["cu_seqlens"], HM.heat_values(att, "percentile", "all")
    xy = st.coords_of(None, 0)
    plan = HM.plan_canvases(st.coord_extents, PS, ds)
    rec = torch.zeros(n, MF.HEAT_REC, dtype=torch.int64)
    rec[:, :5] = plan
    rec[1:, 5] = torch.cumsum(plan[:-1, 3] * plan[:-1, 4], 0)
    P = int(rec[-1, 5] + rec[-1, 3] * rec[-1, 4])
    rec_d, lut = rec.to(dev), HM.colormap("jet").to(dev)
    T, C = values.shape
    taps2, taps0 = HM.gaussian_taps(2.0), HM.gaussian_taps(0.0)
    med, ms = alternate({"whole": lambda: MF.heat_render(xy, cu, values, rec, P, ds, taps2, lut, 255, None, rec_d),
                         "whole_r0": lambda: MF.heat_render(xy, cu, values, rec, P, ds, taps0, lut, 255, None, rec_d)}, a.steps)
    stages = {name: {k: [] for k in MF.HEAT_STAGES} for name in ("sigma2", "r0")}
    for i in range(max(1, a.steps) + 1):                      # the first repetition is the warm-up
        for name, taps in (("sigma2", taps2), ("r0", taps0)):
            got = MF.heat_render_stages(xy, cu, values, rec, P, ds, taps, lut, 255, None, rec_d)[3]
            if i:
                for k, v in got.items():
                    stages[name][k].append(v)
    st_med = {name: {k: statistics.median(v) for k, v in d.items()} for name, d in stages.items()}
    fp = (PS // ds + 1) ** 2                                  # pixels under a patch, at most
    plane = float(C) * P
    nbytes = {"clear": plane * MF.HEAT_PLANE_BYTES["clear"],
              "accumulate": T * (8.0 + 4 * C) + 8.0 * T * C * fp,           # xy and values read once; one 8-B atomic a pixel and channel
              "blur_rows": plane * MF.HEAT_PLANE_BYTES["blur_rows"],        # without the halo re-reads
              "blur_cols_colour": plane * MF.HEAT_PLANE_BYTES["blur_cols_colour"]}
    res["render"] = {"pixels": P, "rows": T, "channels": C, "median_ms": med, "stage_ms": st_med, "stage_bytes": nbytes,
                     "stage_GB_per_s": {k: nbytes[k] / st_med["sigma2"][k] / 1e6 for k in nbytes}}
    lines.append("heat_render: %d bags, %d rows, %d channels, %d pixels a channel: whole %.3f ms (r = 0: %.3f ms)"
                 % (n, T, C, P, med["whole"], med["whole_r0"]))
    lines.append("  stage (events of mdl_heat_render_marked)   sigma 2 ms   r = 0 ms   bytes by the contract   GB/s at sigma 2")
    for k in MF.HEAT_STAGES:
        lines.append("  %-42s %9.3f %10.3f %20.3e %15.0f" % (k, st_med["sigma2"][k], st_med["r0"][k], nbytes[k],
                                                             nbytes[k] / st_med["sigma2"][k] / 1e6))
    lines.append("  blur taps alone (sigma 2 - r = 0): rows %.3f ms, columns %.3f ms; level + colour = the column pass at r = 0"
                 % (st_med["sigma2"]["blur_rows"] - st_med["r0"]["blur_rows"],
                    st_med["sigma2"]["blur_cols_colour"] - st_med["r0"]["blur_cols_colour"]))

    # ---- 3. the same images elsewhere
    out = st.heatmaps(model, heads="all", downsample=ds, sigma=2.0)
    cu_h = cu.tolist()
    b0 = slice(cu_h[0], cu_h[1])
    W, H = out["canvas"][0][:2]
    t0 = time.perf_counter()
    ref = HR.render_bag(xy[b0].cpu().numpy(), values[b0, :1].cpu().numpy(), PS, 0, 0, W, H, ds, taps2.tolist(), HM.colormap("jet").numpy(), 255)
    cpu_s = time.perf_counter() - t0
    equal = bool(np.array_equal(ref["level"][0], out["level"][0][0].cpu().numpy()))
    res["numpy_reference"] = {"one_bag_one_channel_s": cpu_s, "extrapolated_s": cpu_s * n * C, "level_equal": equal}
    lines.append("numpy reference: %.2f s for one bag and channel (level equal to the device: %s) -> %.0f s for %d x %d by extrapolation"
                 % (cpu_s, equal, cpu_s * n * C, n, C))

    def torch_all():
        return [torch_restatement(xy[cu_h[b]:cu_h[b + 1]], values[cu_h[b]:cu_h[b + 1]], PS, ds, out["canvas"][b][0], out["canvas"][b][1],
                                  taps2) for b in range(n)]
    med_t, _ = alternate({"torch": torch_all}, a.steps)
    lvl, cov = torch_restatement(xy[b0], values[b0], PS, ds, W, H, taps2)
    mine = out["level"][0].cpu().numpy().astype(np.float64) / 65535.0
    diff = float(np.abs(np.where(cov.cpu().numpy()[None], lvl.cpu().numpy() - mine, 0.0)).max())
    res["torch_restatement"] = {"median_ms": med_t["torch"], "over_heat_render": med_t["torch"] / med["whole"], "max_level_diff": diff}
    lines.append("torch index_add_ + conv2d restatement (fp64, per bag): %.2f ms = %.1f x heat_render; its level differs by at most %.4f "
                 "of the range (footprints of aligned corners, no quantiser)" % (med_t["torch"], med_t["torch"] / med["whole"], diff))
    for ln in lines:
        print(ln)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
