"""numpy reference of the retrieval kernels (X1) and the closed-form cohorts of their tests.  No GPU, no RNG library.

The order: descending similarity, -0 = +0, every NaN below -inf, ties by the lower gallery index -- the header's.  exact() applies it
to fp32 similarities that the caller knows exactly (integer data, metric 'dot'); bounds() brackets the counts of a cosine retrieval
between what an fp64 computation says is certainly greater and what is possibly greater or equal under a stated tolerance."""
import numpy as np

NAN_KEY, NO_ENTRY = 1, 0


def tol(d):
    """Worst-case distance of the device's fp32 cosine from the exact one: a length-d fmaf chain on unit vectors accumulates at most
    d half-ulps of a value below 1 (d 2^-24) and the two scaled rows carry a few more from the norm, the division and the product
    (4 2^-24 per side); doubled.  (d + 4) 2^-23."""
    return (d + 4) * 2.0 ** -23


def _field(rows, d, a, b, c, seed):
    i = np.arange(rows, dtype=np.float64)[:, None]
    j = np.arange(d, dtype=np.float64)[None, :]
    x = np.sin(i * a + j * b + seed) * c
    return x - np.floor(x) - 0.5


def cohort(n, m, d, noise, seed):
    """(Q [n, d], K [m, d]) fp32: Q the first n rows of the field frac(sin(12.9898 i + 78.233 j + seed) 43758.5453) - 1/2, K the first m
    rows of the same field plus `noise` times a second one (other constants): gallery row i is a noisy copy of query i, rows past n
    are distractors."""
    rows = max(n, m)
    base = _field(rows, d, 12.9898, 78.233, 43758.5453, seed)
    other = _field(rows, d, 4.1414, 269.5, 183.3, seed + 1.0)
    return base[:n].astype(np.float32), (base[:m] + noise * other[:m]).astype(np.float32)


def integers(n, m, d, seed):
    """(Q, K) fp32 with integer entries in [-8, 8]: products and sums of a 'dot' retrieval are exact in fp32 up to d = 2^17, and ties are
    everywhere."""
    q = np.floor((_field(n, d, 12.9898, 78.233, 43758.5453, seed) + 0.5) * 17.0) - 8.0
    g = np.floor((_field(m, d, 39.3468, 11.135, 24634.6345, seed + 2.0) + 0.5) * 17.0) - 8.0
    return np.clip(q, -8, 8).astype(np.float32), np.clip(g, -8, 8).astype(np.float32)


def keys(S32):
    """The ordered key of fp32 similarities, as int64: larger = retrieved earlier."""
    S32 = np.ascontiguousarray(S32, dtype=np.float32)
    u = S32.view(np.uint32).astype(np.int64)
    u = np.where(S32 == 0, 0, u)
    k = np.where(u & 0x80000000, (~u) & 0xFFFFFFFF, u | 0x80000000)
    return np.where(np.isnan(S32), NAN_KEY, k)


def exact(S32, paired, exclude_diag, k):
    """(greater, equal, pair_sim, topk_idx, topk_val) of the fp32 similarity matrix S32 [n, m] under the header's order; fields of a mode
    that is off are None.  int32 / fp32 arrays, as the device's."""
    S32 = np.ascontiguousarray(S32, dtype=np.float32)
    n, m = S32.shape
    K = keys(S32)
    greater = equal = pair_sim = ti = tv = None
    if paired:
        idx = np.arange(n)
        pk = K[idx, idx][:, None]
        off = np.ones((n, m), dtype=bool)
        off[idx, idx] = False
        greater = ((K > pk) & off).sum(1).astype(np.int32)
        equal = ((K == pk) & off).sum(1).astype(np.int32)
        pair_sim = S32[idx, idx].copy()
        nan = np.isnan(pair_sim)
        greater[nan], equal[nan] = m - 1, 0
    if k:
        ti = np.full((n, k), -1, dtype=np.int32)
        tv = np.full((n, k), -np.inf, dtype=np.float32)
        for i in range(n):
            cols = np.arange(m)
            if exclude_diag:
                cols = cols[cols != i]
            order = cols[np.argsort(-K[i, cols], kind="stable")][:k]      # stable: ties by the lower index
            ti[i, :order.size] = order
            tv[i, :order.size] = S32[i, order] + np.float32(0.0)          # -0 -> +0
    return greater, equal, pair_sim, ti, tv


def unit_rows(X):
    X = np.asarray(X, dtype=np.float64)
    return X / np.maximum(np.sqrt((X * X).sum(1, keepdims=True)), 1e-12)


def cosine64(Q, K):
    return unit_rows(Q) @ unit_rows(K).T


def bounds(S64, t):
    """(lo, hi, pair) of a paired retrieval from exact similarities S64 [n, m]: lo[i] = #{j != i: s_ij > s_ii + t}, what is certainly
    greater; hi[i] = #{j != i: s_ij >= s_ii - t}, what may be greater or equal.  The device must give lo <= greater and
    greater + equal <= hi.  A row with lo != hi is ambiguous at tolerance t."""
    n, m = S64.shape
    idx = np.arange(n)
    pair = S64[idx, idx].copy()
    off = np.ones((n, m), dtype=bool)
    off[idx, idx] = False
    lo = ((S64 > pair[:, None] + t) & off).sum(1)
    hi = ((S64 >= pair[:, None] - t) & off).sum(1)
    return lo, hi, pair


def metrics(greater, equal, ks=(1, 5, 10)):
    """retrieval_metrics, restated."""
    g = np.asarray(greater, dtype=np.int64)
    rank = 1 + g + np.asarray(equal, dtype=np.int64)
    out = {"n": int(g.size)}
    for k in ks:
        out["recall@%d" % k] = float((rank <= k).mean())
        out["recall_optimistic@%d" % k] = float((g < k).mean())
    out["median_rank"] = float(np.median(rank))
    out["mrr"] = float((1.0 / rank).mean())
    return out


# (n, m, d, noise) at seed 0.25: the cosine cohorts of the GPU tests, and the shape whose chunking the launcher chooses.  On every
# one of them the fp64 similarities leave no row ambiguous at tol(d) (test_retrieval_cpu.py asserts it), in either direction for the
# last.  More noise brings more near-ties, not fewer: at 4096 x 4096 noise 4 leaves rows inside the tolerance, 3.5 none (the partner's
# rank still reaches 8).
SEED = 0.25
COSINE_COHORTS = [(300, 300, 64, 2), (257, 400, 77, 3), (1153, 1153, 512, 4), (65, 65, 512, 1), (300, 300, 8, 1), (33, 95, 7, 1),
                  (200, 200, 768, 6)]
LAUNCHER_COHORT = (4096, 4096, 512, 3.5)
