"""The heatmap render contract of include/madeleine_amd_view.h (V1) in numpy int64 / uint64: plain loops over patches, np.rint on
float32 for the quantiser.  Not fast and not meant to be: it is what the device is held to bit for bit."""
import numpy as np

TAP_SUM = 4096


def quantise(v):
    """q [n] int64 and keep [n] bool of fp32 values v [n] (step 1)."""
    v = np.asarray(v, dtype=np.float32)
    keep = ~np.isnan(v)
    with np.errstate(invalid="ignore", over="ignore"):
        mid = np.rint(v * np.float32(65535.0))              # one fp32 product, round half to even
    q = np.where(v >= np.float32(1.0), 65535.0, np.where(v > np.float32(0.0), mid, 0.0))
    q = np.where(keep, q, 0.0).astype(np.int64)
    return q, keep


def accumulate(xy, values, ps, ox, oy, W, H, ds):
    """S, N [C, H, W] int64 of one bag (steps 1 - 3).  xy [n, 2] integers, values [n, C] float32."""
    xy = np.asarray(xy, dtype=np.int64).reshape(-1, 2)
    values = np.asarray(values, dtype=np.float32)
    C = values.shape[-1] if values.ndim > 1 else 1
    values = values.reshape(xy.shape[0], C)
    S = np.zeros((C, H, W), dtype=np.int64)
    N = np.zeros((C, H, W), dtype=np.int64)
    for c in range(C):
        q, keep = quantise(values[:, c])
        for i in range(xy.shape[0]):
            if not keep[i]:
                continue
            dx, dy = int(xy[i, 0]) - ox, int(xy[i, 1]) - oy
            x0, x1 = max(dx // ds, 0), min((dx + ps - 1) // ds, W - 1)      # Python's // is floor division
            y0, y1 = max(dy // ds, 0), min((dy + ps - 1) // ds, H - 1)
            if x0 > x1 or y0 > y1:
                continue
            S[c, y0:y1 + 1, x0:x1 + 1] += int(q[i])
            N[c, y0:y1 + 1, x0:x1 + 1] += 1
    return S, N


def blur(A, taps):
    """The row pass, then the column pass, zeros outside, of A [C, H, W] in uint64 (step 4)."""
    taps = [int(t) for t in taps]
    r = (len(taps) - 1) // 2
    A = np.asarray(A).astype(np.uint64)
    C, H, W = A.shape
    pad = np.zeros((C, H, W + 2 * r), dtype=np.uint64)
    pad[:, :, r:r + W] = A
    rows = np.zeros((C, H, W), dtype=np.uint64)
    for k, t in enumerate(taps):
        rows += np.uint64(t) * pad[:, :, k:k + W]
    pad = np.zeros((C, H + 2 * r, W), dtype=np.uint64)
    pad[:, r:r + H, :] = rows
    out = np.zeros((C, H, W), dtype=np.uint64)
    for k, t in enumerate(taps):
        out += np.uint64(t) * pad[:, k:k + H, :]
    return out


def colour(level, covered, lut, alpha, base=None):
    """rgba [C, H, W, 4] uint8 (step 6).  lut [256, 4] uint8, base [H, W, 3] uint8 or None."""
    lut = np.asarray(lut, dtype=np.int64)
    m = level.astype(np.int64)
    idx = (m * 255 + 32767) // 65535
    e = lut[idx]                                             # [C, H, W, 4]
    a = (e[..., 3] * int(alpha) + 127) // 255
    cov = covered.astype(bool)
    out = np.zeros(level.shape + (4,), dtype=np.int64)
    if base is None:
        out[..., :3] = np.where(cov[..., None], e[..., :3], 0)
        out[..., 3] = np.where(cov, a, 0)
    else:
        b = np.broadcast_to(np.asarray(base, dtype=np.int64)[None], level.shape + (3,))
        mix = (e[..., :3] * a[..., None] + b * (255 - a[..., None]) + 127) // 255
        out[..., :3] = np.where(cov[..., None], mix, b)
        out[..., 3] = 255
    return out.astype(np.uint8)


def render_bag(xy, values, ps, ox, oy, W, H, ds, taps, lut, alpha, base=None):
    """One bag: dict S, N, level uint16 [C, H, W], covered uint8 [C, H, W], rgba uint8 [C, H, W, 4]."""
    taps = [int(t) for t in taps]
    r = (len(taps) - 1) // 2
    assert len(taps) == 2 * r + 1 and sum(taps) == TAP_SUM and taps == taps[::-1] and min(taps) >= 0 and taps[r] > 0
    S, N = accumulate(xy, values, int(ps), int(ox), int(oy), int(W), int(H), int(ds))
    S2, N2 = blur(S, taps), blur(N, taps)
    covered = N > 0
    level = np.zeros(S.shape, dtype=np.uint64)
    level[covered] = S2[covered] // N2[covered]
    assert int(level.max(initial=0)) <= 65535
    level, covered = level.astype(np.uint16), covered.astype(np.uint8)
    return {"S": S, "N": N, "level": level, "covered": covered, "rgba": colour(level, covered, lut, alpha, base)}


def render(xy, cu, values, records, ds, taps, lut, alpha, bases=None):
    """All bags of a call: a list of render_bag results.  records: per bag (ps, ox, oy, W, H); bases: per bag [H, W, 3] or None."""
    xy, values, cu = np.asarray(xy), np.asarray(values), [int(c) for c in cu]
    out = []
    for b, (ps, ox, oy, W, H) in enumerate(records):
        a, e = cu[b], cu[b + 1]
        out.append(render_bag(xy[a:e], values[a:e], ps, ox, oy, W, H, ds, taps, lut, alpha,
                              None if bases is None else bases[b]))
    return out
