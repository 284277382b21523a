"""fp64 numpy references of the patch contributions (include/madeleine_amd_explain.h): what tests/test_contrib_*.py hold the kernels,
the model and the store to.  Plain numpy, no torch, no device."""
import numpy as np

U23 = 2.0 ** -23


def contrib(E, attn, U, H):
    """(per_head [T, H, C], total [T, C], abs_head [T, H, C], abs_total [T, C]) in fp64 of head-major E [T, H * W], attn [T, H] and
    U [C, H * W]: per_head[t, h, c] = attn[t, h] sum_e U[c, h W + e] E[t, h W + e], total = the sum over the heads, and the sums of
    the absolute values of the same terms (the scale of the summation bounds)."""
    E, attn, U = np.asarray(E, np.float64), np.asarray(attn, np.float64), np.asarray(U, np.float64)
    T, C = E.shape[0], U.shape[0]
    W = E.shape[1] // H
    Eh, Uh = E.reshape(T, H, W), U.reshape(C, H, W)
    per_head = np.einsum("th,thw,chw->thc", attn, Eh, Uh)
    abs_head = np.einsum("th,thw,chw->thc", np.abs(attn), np.abs(Eh), np.abs(Uh))
    return per_head, per_head.sum(1), abs_head, abs_head.sum(1)


def contrib_int(E, attn, U, H):
    """per_head and total of integer-valued E and U and power-of-two attn in exact arithmetic: the products in int64, the scaling by
    attn last (exact in fp64 for the sizes the tests use)."""
    E, U = np.asarray(E, np.int64), np.asarray(U, np.int64)
    T, C = E.shape[0], U.shape[0]
    W = E.shape[1] // H
    dots = np.einsum("thw,chw->thc", E.reshape(T, H, W), U.reshape(C, H, W))
    per_head = dots.astype(np.float64) * np.asarray(attn, np.float64)[:, :, None]
    return per_head, per_head.sum(1)


def stats(c, cu):
    """(stats [R, 4, C], abs_sum [R, C]) in fp64 of c [T, C] over the bags cu [R + 1]: sum, sum of the terms whose sign bit is clear,
    sum of the terms whose sign bit is set, max |.| (NaN as soon as one term is); an empty bag gives zeros."""
    c = np.asarray(c, np.float64)
    R, C = len(cu) - 1, c.shape[1]
    out, scale = np.zeros((R, 4, C)), np.zeros((R, C))
    for r in range(R):
        seg = c[cu[r]:cu[r + 1]]
        if len(seg) == 0:
            continue
        minus = np.signbit(seg)
        out[r, 0] = seg.sum(0)
        out[r, 1] = np.where(minus, 0.0, seg).sum(0)
        out[r, 2] = np.where(minus, seg, 0.0).sum(0)
        out[r, 3] = np.where(np.isnan(seg).any(0), np.nan, np.abs(np.nan_to_num(seg, nan=0.0)).max(0))
        scale[r] = np.abs(seg).sum(0)
    return out, scale


def head_major(x, H):
    """The last axis of x from the reference's channel order j = e H + h to head-major j' = h W + e."""
    x = np.asarray(x)
    W = x.shape[-1] // H
    return x.reshape(x.shape[:-1] + (W, H)).swapaxes(-1, -2).reshape(x.shape)


def directions(P, bP, W, b, H):
    """(U [C, H * Wd] head-major, const [C]) in fp64 of the projector (P [d, H * Wd] in the reference's column order, bP [d]) and the
    decision rows W [C, d], b [C]: U = W P with head-major columns, const = W bP + b."""
    P, bP, W, b = (np.asarray(v, np.float64) for v in (P, bP, W, b))
    return head_major(W @ P, H), W @ bP + b


def signed_values(c, cu):
    """0.5 + 0.5 c / max_t |c| per bag and column in fp32, in the order of operations of DeviceSlideStore.contribution_maps; a bag
    without evidence is 0.5."""
    c = np.asarray(c, np.float32)
    out = np.empty_like(c)
    for r in range(len(cu) - 1):
        seg = c[cu[r]:cu[r + 1]]
        m = np.abs(seg).max(0) if len(seg) else np.zeros(c.shape[1], np.float32)
        with np.errstate(invalid="ignore", divide="ignore"):
            out[cu[r]:cu[r + 1]] = np.where(m == 0, np.float32(0.5), np.float32(0.5) + np.float32(0.5) * seg / m)
    return out


def topk(c, cu, k):
    """(pos_idx, pos_val, neg_idx, neg_val) [R, C, k] of c [T, C]: per bag and column the k most positive and the k most negative rows
    by a stable numpy sort (ties: the lower row first), padded with -1 and -inf / +inf."""
    c = np.asarray(c, np.float32)
    R, C = len(cu) - 1, c.shape[1]
    pi, ni = np.full((R, C, k), -1, np.int32), np.full((R, C, k), -1, np.int32)
    pv, nv = np.full((R, C, k), -np.inf, np.float32), np.full((R, C, k), np.inf, np.float32)
    for r in range(R):
        seg = c[cu[r]:cu[r + 1]]
        m = min(k, len(seg))
        for j in range(C):
            down = np.argsort(-seg[:, j], kind="stable")[:m]
            up = np.argsort(seg[:, j], kind="stable")[:m]
            pi[r, j, :m], pv[r, j, :m] = down, seg[down, j]
            ni[r, j, :m], nv[r, j, :m] = up, seg[up, j]
    return pi, pv, ni, nv
