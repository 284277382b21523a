"""Attention heatmaps on the device: patch coordinates and per-patch values of packed bags become RGBA images (functional.heat_render
-> mdl_heat_render, csrc/heat_map.hip; the contract is section V1 of include/madeleine_amd_view.h).

Replaces the host loop around the attention scores that every ABMIL user writes (the CLAM-style heatmap): average the patch scores
over overlapping patch footprints on a down-sampled canvas, blur, colour-map, blend over a thumbnail.  Here the canvases of a whole
cohort are PLANNED on the host (from coordinate extents, O(bags) work) and rendered by four launches per group of bags; the arithmetic
is exact integers, so an image does not depend on its neighbours in the call, on the grouping or on the run.

    taps = gaussian_taps(2.0); lut = colormap('jet')
    out = render(xy, cu, values, patch_size=256, downsample=64, sigma=2.0)      # out['rgba'][b]: [C, H, W, 4] uint8 on the device
    save_png('bag0.png', out['rgba'][0][0])

DeviceSlideStore.heatmaps is the cohort-level top: model -> attention -> these images.
"""
import math
import struct
import zlib

import torch

from . import functional as MF

TAP_SUM = MF.HEAT_TAP_SUM
MAX_RADIUS = MF.HEAT_MAX_R
RENDER_BYTES = 1 << 30      # render(): workspace + outputs of one group of bags stay inside this (a bag that exceeds it goes alone)
_BYTES_PER_PLANE_PIXEL = MF.HEAT_WS_PER_PLANE_PIXEL + 2 + 1 + 4      # workspace | level, covered, rgba


def gaussian_taps(sigma, radius=None):
    """Integer taps [2 r + 1] (int32, host) of a Gaussian of `sigma` canvas pixels that sum to exactly 4096: the real weights scaled
    to 4096, floored, and the missing units handed out by largest remainder -- in symmetric pairs from the centre outwards among equal
    remainders, an odd unit to the centre -- so the result is symmetric.  radius None: ceil(3 sigma), at most 32; sigma = 0 gives
    [4096] (the identity)."""
    sigma = float(sigma)
    if not sigma >= 0.0 or math.isinf(sigma):
        raise ValueError("gaussian_taps: sigma must be a finite number >= 0 (got %r)" % (sigma,))
    if radius is None:
        radius = min(MAX_RADIUS, int(math.ceil(3.0 * sigma)))
    if isinstance(radius, bool) or not isinstance(radius, int) or not 0 <= radius <= MAX_RADIUS:
        raise ValueError("gaussian_taps: radius must be an integer in [0, %d] (got %r)" % (MAX_RADIUS, radius))
    if sigma == 0.0 or radius == 0:
        return torch.tensor([0] * radius + [TAP_SUM] + [0] * radius, dtype=torch.int32)
    w = [math.exp(-0.5 * (k / sigma) ** 2) for k in range(radius + 1)]      # one half, centre first
    total = w[0] + 2.0 * sum(w[1:])
    exact = [TAP_SUM * x / total for x in w]
    half = [int(math.floor(x)) for x in exact]
    missing = TAP_SUM - (half[0] + 2 * sum(half[1:]))
    order = sorted(range(radius + 1), key=lambda k: (-(exact[k] - half[k]), k))      # largest remainder first, then the inner tap
    for k in order:                                         # the centre takes one unit, a pair k >= 1 takes two
        cost = 1 if k == 0 else 2
        if missing >= cost:
            half[k] += 1
            missing -= cost
    half[0] += missing                                      # 0, or the 1 a pair cannot carry
    taps = half[:0:-1] + half
    assert sum(taps) == TAP_SUM and half[0] > 0
    return torch.tensor(taps, dtype=torch.int32)


def _jet(x):
    return (min(max(1.5 - abs(4.0 * x - 3.0), 0.0), 1.0), min(max(1.5 - abs(4.0 * x - 2.0), 0.0), 1.0),
            min(max(1.5 - abs(4.0 * x - 1.0), 0.0), 1.0))


def _coolwarm(x):
    """Moreland's diverging blue-white-red, as the piecewise-linear blend of its three anchors."""
    lo, mid, hi = (59.0, 76.0, 192.0), (221.0, 221.0, 221.0), (180.0, 4.0, 38.0)
    a, b, t = (lo, mid, 2.0 * x) if x < 0.5 else (mid, hi, 2.0 * x - 1.0)
    return tuple((p + (q - p) * t) / 255.0 for p, q in zip(a, b))


_CMAPS = {"jet": _jet, "coolwarm": _coolwarm, "gray": lambda x: (x, x, x)}


def colormap(name):
    """[256, 4] uint8 RGBA (host), opaque, computed from a formula: 'jet' (the piecewise-linear ramps), 'coolwarm' (blue - white - red)
    or 'gray'.  A [256, 4] uint8 tensor is passed through."""
    if torch.is_tensor(name):
        if name.dtype != torch.uint8 or tuple(name.shape) != (256, 4):
            raise ValueError("colormap: a lookup table must be [256, 4] uint8 (got %s %s)" % (tuple(name.shape), name.dtype))
        return name
    if name not in _CMAPS:
        raise ValueError("colormap: unknown colour map %r (have %s)" % (name, ", ".join(sorted(_CMAPS))))
    f = _CMAPS[name]
    return torch.tensor([[int(round(255.0 * c)) for c in f(i / 255.0)] + [255] for i in range(256)], dtype=torch.uint8)


def save_png(path, rgba):
    """Writes rgba [H, W, 4] (or rgb [H, W, 3]) uint8, a tensor on any device or an array, as a PNG: zlib and struct only."""
    img = torch.as_tensor(rgba).detach().cpu().contiguous()
    if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] not in (3, 4) or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError("save_png: needs [H, W, 3 or 4] uint8 (got %s %s)" % (tuple(img.shape), img.dtype))
    H, W, ch = img.shape
    raw = torch.cat([torch.zeros(H, 1, dtype=torch.uint8), img.view(H, W * ch)], 1).numpy().tobytes()      # filter 0 before every row

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 6 if ch == 4 else 2, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def coord_extents(xy, cu):
    """[R, 4] int64 on the host: (xmin, ymin, xmax, ymax) of every bag of xy [T, 2] over cu [R + 1]; an empty bag has (0, 0, -1, -1).
    Segment reductions on the device and ONE host read -- DeviceSlideStore keeps these from set_coords time instead."""
    R = cu.numel() - 1
    lens = (cu[1:] - cu[:-1]).clamp(min=0)
    row_bag = torch.repeat_interleave(torch.arange(R, device=xy.device), lens, output_size=xy.shape[0])
    idx = row_bag[:, None].expand(-1, 2)
    lo = torch.full((R, 2), 2 ** 31 - 1, dtype=torch.int32, device=xy.device).scatter_reduce_(0, idx, xy, "amin")
    hi = torch.full((R, 2), -2 ** 31, dtype=torch.int32, device=xy.device).scatter_reduce_(0, idx, xy, "amax")
    ext = torch.cat([lo, hi], 1).cpu().long()
    ext[lens.cpu() == 0] = torch.tensor([0, 0, -1, -1])
    return ext


def plan_canvases(extents, patch_size, downsample, crop=False):
    """[R, 5] int64 (ps, ox, oy, W, H) on the host.  crop False: origin 0, so the image aligns with a slide thumbnail at the same
    downsample; crop True: the origin is the bag's minimum.  The canvas ends with the last pixel a footprint touches; an empty bag gets
    a 1 x 1 canvas."""
    ext = torch.as_tensor(extents, dtype=torch.int64).reshape(-1, 4)
    R, ds = ext.shape[0], int(downsample)
    ps = torch.as_tensor(patch_size, dtype=torch.int64).reshape(-1)
    if ps.numel() == 1:
        ps = ps.expand(R)
    if ps.numel() != R or ds < 1 or (R and int(ps.min()) < 1):
        raise ValueError("plan_canvases: needs downsample >= 1 and one patch size >= 1, or one per bag (%d bags, got %d)" % (R, ps.numel()))
    empty = ext[:, 2] < ext[:, 0]
    org = ext[:, :2] if crop else torch.zeros(R, 2, dtype=torch.int64)
    org = torch.where(empty[:, None], torch.zeros_like(org), org)
    size = torch.div(ext[:, 2:] - org + ps[:, None] - 1, ds, rounding_mode="floor") + 1
    size = torch.where(empty[:, None], torch.ones_like(size), size).clamp(min=1)
    return torch.cat([ps[:, None], org, size], 1)


def minmax_normalise(values, cu):
    """(v - min) / (max - min) per bag and column of values [T, C] over cu [R + 1], on the device with segment reductions; a constant
    bag maps to 0.5.  NaNs stay NaN (the renderer leaves such a patch out) and do not enter the extrema."""
    T, R = values.shape[0], cu.numel() - 1
    lens = (cu[1:] - cu[:-1]).clamp(min=0)
    row_bag = torch.repeat_interleave(torch.arange(R, device=values.device), lens, output_size=T)
    idx = row_bag[:, None].expand(-1, values.shape[1])
    nan = torch.isnan(values)
    lo = torch.full((R, values.shape[1]), float("inf"), device=values.device).scatter_reduce_(
        0, idx, torch.where(nan, torch.full_like(values, float("inf")), values), "amin")
    hi = torch.full((R, values.shape[1]), float("-inf"), device=values.device).scatter_reduce_(
        0, idx, torch.where(nan, torch.full_like(values, float("-inf")), values), "amax")
    lo, hi = lo[row_bag], hi[row_bag]
    out = torch.where(hi > lo, (values - lo) / (hi - lo), torch.full_like(values, 0.5))
    return torch.where(nan, values, out)


def heat_values(att, source="percentile", heads="mean"):
    """values [T, C] fp32 for render() from a DeviceSlideStore.attention result.  source 'percentile': percentile / 100; 'attention' /
    'raw': the softmax weights / raw scores, min-max normalised per bag and channel (minmax_normalise).  heads 'mean': one channel, the
    mean over the head axis, taken FIRST (of percentile / 100, or of the scores before their min-max); 'all': one channel per head;
    an int: that head."""
    key = {"percentile": "percentile", "attention": "attention", "raw": "raw"}.get(source)
    if key is None or att.get(key) is None:
        raise ValueError("heat_values: source must be 'percentile' (computed with percentile=True), 'attention' or 'raw' (got %r)"
                         % (source,))
    v = att[key]
    if source == "percentile":
        v = v / 100.0
    H = v.shape[1]
    if isinstance(heads, str):
        if heads not in ("mean", "all"):
            raise ValueError("heat_values: heads must be 'mean', 'all' or a head index (got %r)" % (heads,))
        v = v.mean(1, keepdim=True) if heads == "mean" else v
    else:
        if isinstance(heads, bool) or not isinstance(heads, int) or not 0 <= heads < H:
            raise IndexError("heat_values: head %r outside [0, %d)" % (heads, H))
        v = v[:, heads:heads + 1]
    return v if source == "percentile" else minmax_normalise(v, att["cu_seqlens"])


def render(xy, cu, values, patch_size, downsample=None, sigma=0.0, cmap="jet", alpha=255, base=None, crop=False, extents=None,
           canvases=None, taps=None, max_bytes=RENDER_BYTES, lens=None):
    """RGBA images of R bags x C channels, on the device.
      xy [T, 2] int32 level-0 top-left corners, cu [R + 1] int64, values [T, C] fp32 (0 .. 1 is the colour range; NaN leaves the patch
      out), all on the device; patch_size: one int or one per bag (level-0 pixels a patch side); downsample: level-0 pixels per canvas
      pixel (None: the patch size, which must then be one number -- without overlap a patch is exactly one pixel); sigma: Gaussian
      blur in canvas pixels (taps: explicit integer taps instead, see gaussian_taps); cmap: a name of colormap() or a [256, 4] uint8
      table; alpha 0 .. 255; base: per bag an [H, W, 3] uint8 thumbnail of the canvas (or None) to blend over.
      The canvases are planned on the host: canvases [R, 4] = (W, H, ox, oy) per bag when given; else from extents [R, 4] = (xmin, ymin,
      xmax, ymax) per bag -- DeviceSlideStore knows them from set_coords time; None costs one host read (coord_extents) -- with origin 0
      (crop False: aligned with a thumbnail) or at the bag's minimum (crop True).
    Returns {'rgba': list of [C, H, W, 4] uint8, 'level': list of [C, H, W] uint16 (0 .. 65535, the blurred mean), 'covered': list of
    [C, H, W] uint8, 'canvas': list of (W, H, ox, oy), 'downsample'}: views of the packed outputs.  Bags go in groups whose workspace
    and outputs stay inside max_bytes; the images do not depend on the grouping (exact integer arithmetic).  With more than one
    group every call gets its own rows (rebased cu), so the kernel's T < 2^24 limit holds per group, not per cohort; the row cuts come
    from lens (the bag lengths on the host, for a cu that starts at 0) or, without it, from one host read of cu."""
    R = cu.numel() - 1
    if downsample is None:
        if torch.as_tensor(patch_size).numel() != 1:
            raise ValueError("heatmap.render: downsample None means the patch size, which must then be one number")
        downsample = int(torch.as_tensor(patch_size).reshape(-1)[0])
    ds = int(downsample)
    taps = gaussian_taps(sigma) if taps is None else torch.as_tensor(taps, dtype=torch.int32).contiguous()
    lut = MF.h2d(colormap(cmap), xy.device)
    if canvases is not None:
        cv = torch.as_tensor(canvases, dtype=torch.int64).reshape(R, 4)
        ps = torch.as_tensor(patch_size, dtype=torch.int64).reshape(-1)
        plan = torch.cat([(ps.expand(R) if ps.numel() == 1 else ps)[:, None], cv[:, 2:], cv[:, :2]], 1)
    else:
        plan = plan_canvases(coord_extents(xy, cu) if extents is None else extents, patch_size, ds, crop)
    if base is not None and len(base) != R:
        raise ValueError("heatmap.render: base must hold one entry per bag (%d bags, got %d)" % (R, len(base)))
    C = values.shape[1]
    pixels = (plan[:, 3] * plan[:, 4]).tolist()
    budget = max(1, int(max_bytes) // (_BYTES_PER_PLANE_PIXEL * C))      # pixels per group
    cuts, used = [0], 0
    for b, n in enumerate(pixels):
        if used and used + n > budget:
            cuts.append(b)
            used = 0
        used += n
    cuts.append(R)
    row_cuts = None
    if len(cuts) > 2:
        row_cuts = cu.tolist() if lens is None else [0] + torch.cumsum(torch.as_tensor(lens, dtype=torch.int64), 0).tolist()
        if len(row_cuts) != R + 1:
            raise ValueError("heatmap.render: lens must hold one length per bag (%d bags, got %d)" % (R, len(row_cuts) - 1))
    out = {"rgba": [], "level": [], "covered": [], "canvas": [], "downsample": ds}
    for a, e in zip(cuts[:-1], cuts[1:]):
        if e == a:
            continue
        rec = torch.zeros(e - a, MF.HEAT_REC, dtype=torch.int64)
        rec[:, :5] = plan[a:e]
        rec[1:, 5] = torch.cumsum(plan[a:e - 1, 3] * plan[a:e - 1, 4], 0)
        P = int(rec[-1, 5] + rec[-1, 3] * rec[-1, 4])
        under = None
        if base is not None:
            under = torch.zeros(P, 3, dtype=torch.uint8, device=xy.device)
            for b in range(a, e):
                if base[b] is None:
                    continue
                _, _, _, W, H, off = rec[b - a].tolist()
                img = torch.as_tensor(base[b])
                if img.dtype != torch.uint8 or tuple(img.shape) != (H, W, 3):
                    raise ValueError("heatmap.render: the thumbnail of bag %d must be [%d, %d, 3] uint8 (got %s %s)"
                                     % (b, H, W, tuple(img.shape), img.dtype))
                under[off:off + W * H] = img.reshape(-1, 3).to(xy.device)
        if len(cuts) == 2:                                    # one group: the call's own arrays
            g_xy, g_cu, g_values = xy, cu, values
        else:                                                 # a group's own rows, rebased: its launch and the T < 2^24 limit are the group's
            r0, r1 = row_cuts[a], row_cuts[e]
            g_xy, g_cu, g_values = xy[r0:r1], cu[a:e + 1] - r0, values[r0:r1]
        level, covered, rgba = MF.heat_render(g_xy, g_cu, g_values, rec, P, ds, taps, lut, alpha, under)
        for b in range(a, e):
            _, ox, oy, W, H, off = rec[b - a].tolist()
            out["level"].append(level[C * off:C * (off + W * H)].view(C, H, W))
            out["covered"].append(covered[C * off:C * (off + W * H)].view(C, H, W))
            out["rgba"].append(rgba[C * off:C * (off + W * H)].view(C, H, W, 4))
            out["canvas"].append((W, H, ox, oy))
    return out
