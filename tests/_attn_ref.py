"""numpy reference of the attention read-out (include/madeleine_amd.h, A-map), written from its definitions: the fp64 softmax of a
segment, and in integers the stable descending order, the percentile ranks and the top-k under the header's comparison rule (ordinary
float order, -0 == +0, every NaN equal to every other NaN and above +inf).  Test infrastructure; O(n log n) per segment."""
import numpy as np


def rank_key(s):
    """int64 keys whose integer order is the header's order of the fp32 scores `s` (any bit pattern)."""
    u = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32).astype(np.int64)
    u = np.where((u & 0x7FFFFFFF) > 0x7F800000, 0x7FC00000, u)      # every NaN is one value above +inf
    u = np.where(u == 0x80000000, 0, u)                             # -0 is +0
    return np.where(u & 0x80000000, -(u & 0x7FFFFFFF), u)           # sign-magnitude to two's complement


def order_desc(s):
    """rows of the segment, highest score first, ties by the lower row"""
    return np.argsort(-rank_key(s), kind="stable").astype(np.int32)


def percentile(s):
    """(float32)(100.0 * (2 L + E + 1) / (2.0 * n)) per row: L scores strictly below, E equal (itself included)"""
    k = rank_key(s)
    srt = np.sort(k)
    L = np.searchsorted(srt, k, side="left").astype(np.int64)
    E = np.searchsorted(srt, k, side="right").astype(np.int64) - L
    return (100.0 * (2 * L + E + 1).astype(np.float64) / (2.0 * float(len(k)))).astype(np.float32)


def percentile_by_counting(s):
    """the same by the O(n^2) count of the definition"""
    k = rank_key(s)
    L = (k[None, :] < k[:, None]).sum(1)
    E = (k[None, :] == k[:, None]).sum(1)
    return (100.0 * (2 * L + E + 1).astype(np.float64) / (2.0 * float(len(k)))).astype(np.float32)


def topk(s, k):
    """(idx [k] int32, val [k] fp32): the first min(k, n) of the order and their raw scores, padded with -1 / -inf"""
    s = np.ascontiguousarray(s, dtype=np.float32)
    o = order_desc(s)[:k]
    idx = np.full(k, -1, dtype=np.int32)
    val = np.full(k, -np.inf, dtype=np.float32)
    idx[:len(o)] = o
    val[:len(o)] = s[o]
    return idx, val


def softmax64(s):
    """(attn fp64, m fp32) of one segment of finite scores"""
    s = np.asarray(s, dtype=np.float32)
    m = s.max()
    e = np.exp(s.astype(np.float64) - float(m))
    return e / e.sum(), m


def readout(scores, cu, k):
    """The whole read-out of scores [T, H] over the bags of cu: dict of order [H, T], pct [T, H], topk_idx / topk_val [R, H, k]."""
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    T, H = scores.shape
    R = len(cu) - 1
    out = {"order": np.zeros((H, T), np.int32), "pct": np.zeros((T, H), np.float32),
           "topk_idx": np.full((R, H, k), -1, np.int32), "topk_val": np.full((R, H, k), -np.inf, np.float32)}
    for r in range(R):
        a, b = int(cu[r]), int(cu[r + 1])
        for h in range(H):
            if b == a:
                continue
            s = scores[a:b, h]
            out["order"][h, a:b] = order_desc(s)
            out["pct"][a:b, h] = percentile(s)
            out["topk_idx"][r, h], out["topk_val"][r, h] = topk(s, k)
    return out
