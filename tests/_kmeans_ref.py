"""The contract of K1-K4 (include/madeleine_amd_cluster.h) in numpy fp64: exact assign, update, k-means++ seeding and histograms, and the
checkers that hold a device result to them.  The bounds are derived, not measured; u = 2^-24 is the unit roundoff of fp32.

Assign.  The device forms v_tj = x_t . c_j - 0.5 |c_j|^2 as a fmaf chain of depth <= D (|error| <= D u |x||c| to first order), a half
norm (a chain of depth <= D/64 + 6: <= D u 0.5 |c|^2) and one subtraction (u |v|); with a factor 2 of slack
    E_tj = (D + 2) 2u (|x_t| |c_j| + 0.5 |c_j|^2).
d = |x|^2 - 2 v, so a device label L is the argmin of a distance perturbed by at most 2 E: it is accepted iff
    d64(t, L) <= min_j d64(t, j) + 2 (E_tL + E_tj*).            EVERY row is checked.
Dist: |x|^2 carries (D + 2) u |x|^2, 2 v carries 2 E_tL and the subtraction u |d|: |dist_t - d64(t, L)| <= (D + 2) 2u (|x_t| + |c_L|)^2.
Update.  A centroid element is a sum of len members that has passed through at most h(len) additions (the header's formula), each with
relative error u of a partial sum bounded by sum |x_ij| -- h u sum |x_ij| / len = h u mean |x_ij|, doubled for slack -- and the rounding
of the quotient to fp32, u |c64|.  Counts are exact."""
import numpy as np

U = 2.0 ** -24
KM_ROWS, MEAN_ROWS, THREADS, COLS = 128, 1024, 256, 8


def finite_rows(X):
    return np.isfinite(X).all(1)


def distances(X, C):
    """(d64 [T, k], |x| [T], |c| [k]) in fp64; the rows of non-finite x are NaN."""
    X, C = np.asarray(X, np.float64), np.asarray(C, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        xn, cn = (X * X).sum(1), (C * C).sum(1)
        d = xn[:, None] - 2.0 * (X @ C.T) + cn[None, :]
    return d, np.sqrt(xn), np.sqrt(cn)


def assign(X, C):
    """(labels int32 [T], dist fp64 [T]): the argmax of v = x.c - 0.5 |c|^2, the LOWEST index among equals, dist = |x|^2 - 2 v;
    label -1 and dist NaN for a row with a non-finite element.  On integer data every term is exact in fp32 as well."""
    X, C = np.asarray(X, np.float64), np.asarray(C, np.float64)
    fin = finite_rows(X)
    Xf = np.where(fin[:, None], X, 0.0)
    v = Xf @ C.T - 0.5 * (C * C).sum(1)[None, :]
    labels = np.argmax(v, 1).astype(np.int32)               # numpy's argmax returns the first maximum
    dist = (Xf * Xf).sum(1) - 2.0 * v[np.arange(len(X)), labels]
    labels[~fin] = -1
    dist[~fin] = np.nan
    return labels, dist


def inertia(dist):
    return float(np.nansum(np.maximum(dist, 0.0)))


def update(X, labels, C_prev):
    """(C fp64 [k, D], counts int64 [k]): the mean of the rows of every label; a cluster of no member keeps C_prev[j]."""
    X, C = np.asarray(X, np.float64), np.array(C_prev, np.float64)
    k = len(C)
    counts = np.zeros(k, np.int64)
    for j in range(k):
        m = labels == j
        counts[j] = int(m.sum())
        if counts[j]:
            C[j] = X[m].sum(0) / counts[j]
    return C, counts


def seed(X, u):
    """The call positions of k-means++ from the uniforms u [k]: centre 0 is the finite row of rank floor(u0 T_finite); centre j the first
    position whose inclusive prefix of mind (fp32 squared distances to the nearest centre so far, 0 for non-finite rows) exceeds
    u_j * total, and the finite row of rank floor(u_j T_finite) when the total is 0.  Exact (and equal to the device, whose prefix is
    blocked) when the sums are: integer data."""
    X = np.asarray(X, np.float64)
    fin = finite_rows(X)
    idx = np.flatnonzero(fin)
    pos = [int(idx[min(int(u[0] * len(idx)), len(idx) - 1)])]
    mind = np.full(len(X), np.inf)
    for j in range(1, len(u)):
        d = ((np.where(fin[:, None], X, 0.0) - X[pos[-1]]) ** 2).sum(1).astype(np.float32).astype(np.float64)
        mind = np.where(fin, np.minimum(mind, d), 0.0)
        cs = np.cumsum(mind)
        if cs[-1] > 0:
            pos.append(int(np.searchsorted(cs, u[j] * cs[-1], "right")))
        else:
            pos.append(int(idx[min(int(u[j] * len(idx)), len(idx) - 1)]))
    return np.array(pos, np.int64)


def hist(labels, cu, k):
    out = np.zeros((len(cu) - 1, k), np.int32)
    for r in range(len(cu) - 1):
        l = labels[cu[r]:cu[r + 1]]
        l = l[(l >= 0) & (l < k)]
        out[r] = np.bincount(l, minlength=k)
    return out


def depth(n, D):
    """h(len) of the header's K2 comment."""
    slots = -(-D // COLS)
    lpr = 1
    while lpr < slots and lpr < THREADS:
        lpr *= 2
    G = THREADS // lpr
    return -(-min(n, MEAN_ROWS) // G) + (G - 1) + (-(-n // MEAN_ROWS) - 1)


# ---- bounds ------------------------------------------------------------------------------------------------------------------------
def assign_bound(xnorm, cnorm, D):
    """E [T, k]"""
    return (D + 2) * 2 * U * (xnorm[:, None] * cnorm[None, :] + 0.5 * cnorm[None, :] ** 2)


def dist_bound(xnorm, cnorm_of_label, D):
    return (D + 2) * 2 * U * (xnorm + cnorm_of_label) ** 2


# ---- checkers: each returns a list of complaints, empty when the result is within the contract ---------------------------------------
def check_assign(X, C, labels, dist):
    """Every row: a non-finite row has label -1 and dist NaN; any other row a label in [0, k) that is an argmin within the assign bound
    and a dist within the dist bound of d64(t, label)."""
    X, C = np.asarray(X, np.float64), np.asarray(C, np.float64)
    labels, dist = np.asarray(labels), np.asarray(dist, np.float64)
    T, D = X.shape
    bad = []
    if labels.shape != (T,) or dist.shape != (T,):
        return ["shape: labels %s dist %s for T = %d" % (labels.shape, dist.shape, T)]
    fin = finite_rows(X)
    nf = ~fin
    if (labels[nf] != -1).any() or not np.isnan(dist[nf]).all():
        bad.append("a non-finite row has a label or a dist (first at %d)" % int(np.flatnonzero(nf & ((labels != -1) | ~np.isnan(dist)))[0]))
    out = fin & ((labels < 0) | (labels >= len(C)))
    if out.any():
        bad.append("%d finite rows have a label outside [0, k) (first at %d: %d)" % (out.sum(), np.flatnonzero(out)[0], labels[out][0]))
    ok = fin & ~out
    t = np.flatnonzero(ok)
    d64, xn, cn = distances(X[t], C)
    E = assign_bound(xn, cn, D)
    L, star = labels[t], np.argmin(d64, 1)
    a = np.arange(len(t))
    miss = d64[a, L] > d64[a, star] + 2 * (E[a, L] + E[a, star])
    if miss.any():
        i = np.flatnonzero(miss)[0]
        bad.append("%d labels are not an argmin within the bound (first at row %d: label %d at %.9g, best %d at %.9g, slack %.3g)"
                   % (miss.sum(), t[i], L[i], d64[i, L[i]], star[i], d64[i, star[i]], 2 * (E[i, L[i]] + E[i, star[i]])))
    err, lim = np.abs(dist[t] - d64[a, L]), dist_bound(xn, cn[L], D)
    if not (err <= lim).all():
        i = np.flatnonzero(~(err <= lim))[0]
        bad.append("%d dists are outside the bound (first at row %d: %.9g for %.9g, bound %.3g)"
                   % ((~(err <= lim)).sum(), t[i], dist[t[i]], d64[i, L[i]], lim[i]))
    return bad


def check_assign_exact(X, C, labels, dist):
    """Integer data: labels and dist equal the model bit for bit (the lowest index among equal distances)."""
    l, d = assign(X, C)
    labels, dist = np.asarray(labels), np.asarray(dist)
    bad = []
    if labels.shape != l.shape or (labels != l).any():
        i = np.flatnonzero(labels != l)[0] if labels.shape == l.shape else -1
        bad.append("labels differ from the model (first at row %d: %s for %s)" % (i, labels[i] if i >= 0 else "?", l[i] if i >= 0 else "?"))
    d32 = d.astype(np.float32)
    if dist.shape != d32.shape or dist.dtype != np.float32 or (dist.view(np.uint32) != d32.view(np.uint32))[~np.isnan(d32)].any() or \
            (np.isnan(dist) != np.isnan(d32)).any():
        bad.append("dist differs from the model in its bits")
    return bad


def check_update(X, labels, C_prev, C_dev, counts_dev, exact=False):
    """Counts exact; an empty cluster keeps C_prev bit for bit; every element of a non-empty one within 2 h u mean|x| + u |c64| (exact:
    equal to float32(sum64 / count) bit for bit)."""
    X64 = np.asarray(X, np.float64)
    C64, counts = update(X64, np.asarray(labels), C_prev)
    C_dev, counts_dev = np.asarray(C_dev), np.asarray(counts_dev)
    bad = []
    if counts_dev.shape != counts.shape or (counts_dev != counts).any():
        bad.append("counts differ: %s for %s" % (counts_dev.tolist()[:8], counts.tolist()[:8]))
        return bad
    D = X64.shape[1]
    for j in range(len(counts)):
        if counts[j] == 0:
            if (C_dev[j].view(np.uint32) != np.asarray(C_prev, np.float32)[j].view(np.uint32)).any():
                bad.append("the empty cluster %d did not keep its centroid" % j)
            continue
        if exact:
            if (C_dev[j].view(np.uint32) != C64[j].astype(np.float32).view(np.uint32)).any():
                bad.append("cluster %d is not float32(sum64 / count) bit for bit" % j)
            continue
        lim = 2 * depth(int(counts[j]), D) * U * np.abs(X64[labels == j]).mean(0) + U * np.abs(C64[j])
        err = np.abs(C_dev[j].astype(np.float64) - C64[j])
        if not (err <= lim).all():
            i = int(np.argmax(err - lim))
            bad.append("cluster %d (%d members), column %d: %.9g for %.9g, bound %.3g" % (j, counts[j], i, C_dev[j, i], C64[j, i], lim[i]))
    return bad


def check_hist(labels, cu, k, counts_dev):
    want = hist(np.asarray(labels), cu, k)
    got = np.asarray(counts_dev)
    return [] if got.shape == want.shape and (got == want).all() else ["the histogram differs from the model"]
