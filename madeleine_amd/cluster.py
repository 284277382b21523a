"""Morphological prototypes: Lloyd's k-means with k-means++ seeding over patch vectors that stay where they are -- a device matrix or
the bags of a DeviceSlideStore, in any store dtype -- on the HIP kernels of include/madeleine_amd_cluster.h (K1-K4).  The loop is
assign -> update; one 16-byte host read per iteration (the changed-label count and the inertia) decides when to stop.  Every result
is bit-reproducible: no float atomics, fixed summation orders, the host draws only the k uniforms of the seeding.

    res = fit_kmeans(X, 64)                         # X [T, D] fp32 / fp16 / bf16 on the device
    labels, dist = assign_kmeans(X_new, res.centroids)

There is no CPU fallback: a host tensor is an error, not a slower path."""
import collections

import numpy as np
import torch

from . import functional as MF

KMeansResult = collections.namedtuple("KMeansResult", "centroids labels dist counts inertia n_iter converged")
KM_ROWS, KM_MAX_K = MF.KM_ROWS, MF.KM_MAX_K


class RowSource:
    """The rows of a list of stored bags as the kernels address them: store_rows [T_total, D] on the device, off int64 [n_bags + 1]
    (device), and, per listed bag r, bag[r] (the stored bag, -1: no rows), cu[r] (its first call position) and chunk_cu[r] (its first
    chunk of KM_ROWS rows).  The three tables go to the device in ONE upload; `lens` and `starts` (the bags' rows and first store rows)
    stay on the host.  n_rows = T, n_chunks: the totals."""

    def __init__(self, store_rows, off, bag, lens, starts):
        MF._require_store(store_rows)
        bag = torch.as_tensor(bag, dtype=torch.int32).reshape(-1).cpu()
        lens = torch.as_tensor(lens, dtype=torch.int64).reshape(-1).cpu()
        lens = torch.where(bag < 0, torch.zeros_like(lens), lens)
        R = bag.numel()
        host = torch.zeros(2 * (R + 1) + (R + 1) // 2, dtype=torch.int64)      # cu | chunk_cu | bag (int32, two to a word)
        torch.cumsum(lens, 0, out=host[1:R + 1])
        torch.cumsum((lens + (KM_ROWS - 1)) // KM_ROWS, 0, out=host[R + 2:2 * R + 2])
        host[2 * R + 2:].view(torch.int32)[:R] = bag
        self.n_rows, self.n_chunks = int(host[R]), int(host[2 * R + 1])
        table = MF.h2d(host, store_rows.device)
        self.store_rows, self.off = store_rows, off
        self.cu, self.chunk_cu, self.bag = table[:R + 1], table[R + 1:2 * R + 2], table[2 * R + 2:].view(torch.int32)[:R]
        self.lens, self.starts, self.cu_cpu = lens, torch.as_tensor(starts, dtype=torch.int64).reshape(-1).cpu(), host[:R + 1].clone()
        self.dim = store_rows.shape[1]

    def args(self, chunked=True):
        head = (self.store_rows, self.off, self.bag, self.cu)
        return head + (self.chunk_cu, self.n_chunks, self.n_rows) if chunked else head + (self.n_rows,)

    def rows_at(self, positions):
        """The rows at the call positions `positions` (host int64), widened to fp32: [n, D] on the device."""
        pos = torch.as_tensor(positions, dtype=torch.int64).reshape(-1)
        r = torch.searchsorted(self.cu_cpu, pos, right=True) - 1
        # (the last r with cu[r] <= pos: a bag of no rows shares its cu with the next one, which is the one found)
        rows = self.starts[r] + (pos - self.cu_cpu[r])
        return self.store_rows.index_select(0, rows.to(self.store_rows.device)).float()


def _source(X, what):
    if isinstance(X, RowSource):
        return X
    if not isinstance(X, torch.Tensor) or not X.is_cuda:
        raise RuntimeError("madeleine_amd: %s must be a tensor on a ROCm device or a store row source; there is no CPU fallback" % what)
    if X.dim() != 2 or X.shape[0] < 1:
        raise RuntimeError("madeleine_amd: %s must be [T, D] with T >= 1 (got %s)" % (what, tuple(X.shape)))
    off = MF.h2d(torch.tensor([0, X.shape[0]], dtype=torch.int64), X.device)
    return RowSource(X, off, [0], [X.shape[0]], [0])


def _centroids(src, init, k, rng):
    if isinstance(init, torch.Tensor):
        if not init.is_cuda:
            raise RuntimeError("madeleine_amd: init must be a tensor on a ROCm device; there is no CPU fallback")
        if init.dim() != 2 or tuple(init.shape) != (k, src.dim):
            raise ValueError("fit_kmeans: init must be [k, D] = [%d, %d] (got %s)" % (k, src.dim, tuple(init.shape)))
        return init.to(torch.float32).contiguous().clone()
    if init == "k-means++":
        u = MF.h2d(torch.from_numpy(rng.random(k)), src.store_rows.device)
        return MF.kmeans_seed(*src.args(), u)[1]
    if init == "random":
        return src.rows_at(np.sort(rng.choice(src.n_rows, size=k, replace=False)))
    raise ValueError("fit_kmeans: init must be 'k-means++', 'random' or a tensor [k, D] (got %r)" % (init,))


def _lloyd(src, C, max_iter, tol):
    T, k, D, dev = src.n_rows, C.shape[0], src.dim, C.device
    labels = torch.full((T,), -2, device=dev, dtype=torch.int32)
    dist = torch.empty(T, device=dev, dtype=torch.float32)
    stats = torch.empty(2, device=dev, dtype=torch.int64)
    counts = torch.empty(k, device=dev, dtype=torch.int64)
    ws_a = MF._ws_for("mdl_kmeans_assign_ws_bytes", dev, src.n_chunks, k, D, refusal=(MF._KM_LIMITS, KM_MAX_K, k, T))
    ws_u = MF._ws_for("mdl_kmeans_update_ws_bytes", dev, T, k, D, refusal=(MF._KM_LIMITS, KM_MAX_K, k, T))
    nxt = torch.empty_like(C)
    inertia, n_iter, converged = float("nan"), 0, False
    for n_iter in range(1, max_iter + 1):
        MF.kmeans_assign(*src.args(), C, labels, dist, stats, ws_a)
        MF.kmeans_update(*src.args(False), labels, C, nxt, counts, ws_u)
        C, nxt = nxt, C
        host = stats.cpu()                                   # the one host read of the iteration: 16 bytes
        changed, inertia = int(host[0]), float(host.view(torch.float64)[1])
        if n_iter > 1 and changed <= tol * T:
            converged = True
            break
    return KMeansResult(C, labels, dist, counts, inertia, n_iter, converged)


def fit_kmeans(X, k, init="k-means++", max_iter=50, tol=0.0, seed=0, n_init=1) -> KMeansResult:
    """Lloyd's k-means of the rows of X -- a device matrix [T, D] (fp32 / fp16 / bf16, unit column stride, any row stride) or a
    RowSource over stored bags -- into k clusters.  init: 'k-means++' (D^2 sampling on the device from k host uniforms of the seeded
    generator), 'random' (k distinct rows) or a device tensor [k, D].  An iteration is one assign pass and one update pass; the loop
    stops after max_iter of them, or when the share of rows whose label changed in an assign pass is <= tol (0.0: no label changed;
    `converged`).  Returns KMeansResult(centroids [k, D] fp32, labels [T] int32, dist [T] fp32, counts [k] int64, inertia, n_iter,
    converged), tensors on the device: labels, dist and inertia are those of the last assign pass (label -1, dist NaN for a row with a
    non-finite element), centroids and counts the means and sizes of those labels -- a cluster with no member keeps its centroid and
    reports count 0.  n_init > 1: runs with seeds seed, seed + 1, .. and keeps the one of lowest inertia.  Bit-reproducible."""
    src = _source(X, "X")
    k = int(k)
    if not 1 <= k <= KM_MAX_K:
        raise NotImplementedError(MF._KM_LIMITS % (KM_MAX_K, k, src.n_rows))
    if src.n_rows < k:
        raise ValueError("fit_kmeans: %d rows cannot seed %d clusters" % (src.n_rows, k))
    if max_iter < 1 or n_init < 1 or not tol >= 0.0:
        raise ValueError("fit_kmeans: max_iter and n_init must be at least 1 and tol >= 0")
    best = None
    for run in range(1 if isinstance(init, torch.Tensor) else int(n_init)):
        rng = np.random.default_rng(int(seed) + run)
        res = _lloyd(src, _centroids(src, init, k, rng), int(max_iter), float(tol))
        if best is None or res.inertia < best.inertia:
            best = res
    return best


def assign_kmeans(X, centroids):
    """(labels [T] int32, dist [T] fp32) of the rows of X (as in fit_kmeans) under centroids [k, D]: one assign pass, for new slides."""
    src = _source(X, "X")
    if not isinstance(centroids, torch.Tensor) or not centroids.is_cuda:
        raise RuntimeError("madeleine_amd: centroids must be a tensor on a ROCm device; there is no CPU fallback")
    labels, dist, _ = MF.kmeans_assign(*src.args(), centroids.to(torch.float32).contiguous())
    return labels, dist
