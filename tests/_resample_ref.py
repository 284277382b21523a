"""Host model of the test-set bootstrap (include/madeleine_amd_stats.h, B1-B3), written from its specification in plain numpy -- it
calls nothing of the library.  mix32 / key are the dropout counter hash's (tests/_drop_ref.py); the weighted counts come from sorting.

    a      = mix32(key(seed) ^ lo32(g * 0x9E3779B9))
    b      = mix32(a + r)                                       r = 1 .. R; replicate 0: w = 1
    h_j    = mix32(mix32(b ^ j) + lo32(j * 0x9E3779B9))         j = 0 .. S - 1
    draw_j = (h_j * S) >> 32
    w[s]   = #{j : draw_j == s}
"""
import functools

import numpy as np

from tests._drop_ref import GOLDEN32, M32, key, mix32

_U = np.uint64


@functools.lru_cache(maxsize=64)
def _weights(seed, g, R, S):
    a = mix32(key(seed) ^ ((_U(int(g) & 0xFFFFFFFF) * GOLDEN32) & M32))
    j = np.arange(S, dtype=_U)
    gj = (j * GOLDEN32) & M32
    out = np.ones((R + 1, S), dtype=np.int64)
    for r in range(1, R + 1):
        b = mix32((a + _U(r)) & M32)
        h = mix32((mix32(b ^ j) + gj) & M32)
        out[r] = np.bincount(((h * _U(S)) >> _U(32)).astype(np.int64), minlength=S)
    out.setflags(write=False)
    return out


def weights(seed, g, R, S):
    """int64 [R + 1, S] (read-only, cached): the weights of the replicates 0 .. R of group g."""
    return _weights(int(seed), int(g), int(R), int(S))


def draws(seed, g, r, S):
    """int64 [S]: the S draws of replicate r >= 1."""
    a = mix32(key(seed) ^ ((_U(int(g) & 0xFFFFFFFF) * GOLDEN32) & M32))
    j = np.arange(S, dtype=_U)
    b = mix32((a + _U(r)) & M32)
    return ((mix32((mix32(b ^ j) + ((j * GOLDEN32) & M32)) & M32) * _U(S)) >> _U(32)).astype(np.int64)


def test_mask(y, train_idx, n_train, C=None, events=False):
    """bool [S]: the test cases of one problem.  y: the labels (events=False: a label in [0, C) is a labeled case) or the event flags
    (events=True: 0 / 1 have follow-up).  n_train is clamped into [0, n_max], indices outside [0, S) are passed over."""
    y = np.asarray(y)
    S = y.shape[0]
    test = ((y == 0) | (y == 1)) if events else ((y >= 0) & (y < C))
    idx = np.asarray(train_idx)[:min(max(int(n_train), 0), len(train_idx))]
    idx = idx[(idx >= 0) & (idx < S)]
    test = test.copy()
    test[idx] = False
    return test


def predict(z, C):
    """(pred int64 [S], score float64 [S, cols]) of z float32 [S, cols]: z > 0 and z itself for two classes; else the first maximum
    (found with >, as the kernel does: a NaN never wins) and the fp64 log-softmax shifted by that maximum, summed in class order."""
    z = np.asarray(z, dtype=np.float32)
    if C == 2:
        return (z[:, 0] > 0).astype(np.int64), z.astype(np.float64)
    best, pred = z[:, 0].copy(), np.zeros(z.shape[0], dtype=np.int64)
    for c in range(1, C):
        up = z[:, c] > best
        best[up], pred[up] = z[up, c], c
    z64, b64 = z.astype(np.float64), best.astype(np.float64)
    total = np.zeros(z.shape[0])
    with np.errstate(all="ignore"):
        for c in range(C):
            total = total + np.exp(z64[:, c] - b64)
        return pred, z64 - (b64 + np.log(total))[:, None]


def class_counts(z, y, train_idx, n_train, C, group, seed, R):
    """(confusion int64 [P, R + 1, C, C], auc_num int64 [P, R + 1, cols]) of z float32 [P, S, cols], y [S] or [P, S], train_idx
    [P, n_max], n_train [P], group [P]."""
    z = np.asarray(z, dtype=np.float32)
    P, S, cols = z.shape
    y = np.asarray(y)
    conf = np.zeros((P, R + 1, C, C), dtype=np.int64)
    num = np.zeros((P, R + 1, cols), dtype=np.int64)
    for p in range(P):
        yp = y if y.ndim == 1 else y[p]
        test = test_mask(yp, train_idx[p], n_train[p], C)
        W = weights(seed, group[p], R, S)[:, test]
        pred, score = predict(z[p], C)
        t, q, score = yp[test], pred[test], score[test]
        for r in range(R + 1):
            np.add.at(conf[p, r], (t, q), W[r])
        if np.isnan(score).any():
            num[p] = -1
            continue
        for ci in range(cols):
            side = t == (1 if C == 2 else ci)
            values, inv = np.unique(score[:, ci], return_inverse=True)      # sorted; -0.0 and 0.0 are one value
            for r in range(R + 1):
                inside = np.bincount(inv, weights=W[r] * side, minlength=len(values)).astype(np.int64)
                outside = np.bincount(inv, weights=W[r] * ~side, minlength=len(values)).astype(np.int64)
                below = np.cumsum(outside) - outside
                num[p, r, ci] = int((inside * (2 * below + outside)).sum())
    return conf, num


def surv_counts(z, time, event, train_idx, n_train, group, seed, R):
    """int64 [P, R + 1, 2]: weighted concordance numerator and comparable pairs.  z float32 [P, S]; time, event [S] or [P, S]."""
    z = np.asarray(z, dtype=np.float32)
    P, S = z.shape
    time, event = np.asarray(time, dtype=np.float32), np.asarray(event)
    out = np.zeros((P, R + 1, 2), dtype=np.int64)
    for p in range(P):
        tp, ep = (time if time.ndim == 1 else time[p]), (event if event.ndim == 1 else event[p])
        test = test_mask(ep, train_idx[p], n_train[p], events=True)
        W = weights(seed, group[p], R, S)[:, test]
        zi, ti, ei = z[p][test], tp[test], ep[test]
        comparable = (ei[:, None] == 1) & ((ti[:, None] < ti[None, :]) | ((ti[:, None] == ti[None, :]) & (ei[None, :] == 0)))
        points = 2 * (zi[:, None] > zi[None, :]) + (zi[:, None] == zi[None, :])
        for r in range(R + 1):
            ww = W[r][:, None] * W[r][None, :]
            out[p, r, 0] = int((ww * comparable * points).sum())
            out[p, r, 1] = int((ww * comparable).sum())
    return out


# ---- from counts to the metrics of a replicate, in double ----------------------------------------------------------------------------
def auc_from_counts(conf, num):
    """float64 [...]: the macro-averaged one-vs-rest AUC of confusion [..., C, C] and numerators [..., cols]; NaN where a class or its
    complement has no weight, or the numerator is -1."""
    conf, num = np.asarray(conf, dtype=np.float64), np.asarray(num, dtype=np.float64)
    C, cols = conf.shape[-1], num.shape[-1]
    rows = conf.sum(-1)
    total = rows.sum(-1)
    out = np.zeros(num.shape[:-1])
    with np.errstate(all="ignore"):
        for ci in range(cols):
            pos = rows[..., 1 if C == 2 else ci]
            neg = total - pos
            term = num[..., ci] / (2.0 * pos * neg)
            term = np.where((pos > 0) & (neg > 0) & (num[..., ci] >= 0), term, np.nan)
            out = out + term
    return out / cols


def c_index_from_counts(counts):
    counts = np.asarray(counts, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(counts[..., 1] > 0, counts[..., 0] / (2.0 * counts[..., 1]), np.nan)


def summary(values, level=0.95):
    """(point, lo, hi, n_valid) of values [R + 1]: row 0 and the percentile interval over the finite replicates 1 .. R."""
    values = np.asarray(values, dtype=np.float64)
    rep = values[1:][np.isfinite(values[1:])]
    if rep.size == 0:
        return values[0], np.nan, np.nan, 0
    lo, hi = np.quantile(rep, [(1 - level) / 2, 1 - (1 - level) / 2])
    return values[0], lo, hi, rep.size


def p_value(d):
    """The two-sided bootstrap p of the replicate differences d (finite values only)."""
    d = np.asarray(d, dtype=np.float64)
    d = d[np.isfinite(d)]
    n = d.size
    return min(1.0, 2.0 * min(((d <= 0).sum() + 1) / (n + 1), ((d >= 0).sum() + 1) / (n + 1)))
