"""Host side of k-means over the slide store (K1-K4, include/madeleine_amd_cluster.h): the sixth header and its binding, the workspace
queries and every refusal that comes before a launch, the exported surface and "no CPU fallback", and the numpy contract of
tests/_kmeans_ref.py held to independent formulas, to scipy and scikit-learn where they are installed, and to seeded faults that its
checkers must reject.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

from madeleine_amd import _build, _native
from tests import _kmeans_ref as R

P, I32, I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
FAKE = 1 << 20          # a 16-byte aligned address nothing dereferences: every refusal below comes before the first launch
ARG, UNSUP, ALIGN = (_native._DEFINES[k] for k in ("MDL_E_ARG", "MDL_E_UNSUPPORTED", "MDL_E_ALIGN"))
NAMES = {"mdl_kmeans_assign_ws_bytes", "mdl_kmeans_assign", "mdl_kmeans_update_ws_bytes", "mdl_kmeans_update",
         "mdl_kmeans_seed_ws_bytes", "mdl_kmeans_seed", "mdl_kmeans_hist_ws_bytes", "mdl_kmeans_hist"}
SRC = [P, I32, I64, I64, P, I64, P, P]          # store, dtype, row_stride, T_total, off, n_bags, bag, cu


# ---- header and ABI ------------------------------------------------------------------------------------------------------------------
def test_the_sixth_header_parses_and_is_bound_beside_the_other_five():
    with open(_build.CLUSTER_HEADER) as f:
        sigs, defines = _native._parse_header(f.read())
    assert sigs == _native.CLUSTER_SIGNATURES and set(sigs) == NAMES and defines == _native.CLUSTER_DEFINES
    assert sigs["mdl_kmeans_assign_ws_bytes"] == (I64, [I64, I32, I32])
    assert sigs["mdl_kmeans_assign"] == (I32, SRC + [P, I64, I64, I64, I32, P, I32, P, P, P, P, P])
    assert sigs["mdl_kmeans_update_ws_bytes"] == (I64, [I64, I32, I32])
    assert sigs["mdl_kmeans_update"] == (I32, SRC + [I64, I64, I32, P, P, I32, P, P, P, P])
    assert sigs["mdl_kmeans_seed_ws_bytes"] == (I64, [I64, I64])
    assert sigs["mdl_kmeans_seed"] == (I32, SRC + [P, I64, I64, I64, I32, P, I32, P, P, P, P])
    assert sigs["mdl_kmeans_hist_ws_bytes"] == (I64, [I64, I32])
    assert sigs["mdl_kmeans_hist"] == (I32, [P, P, I64, I64, I32, P, P])
    assert defines == {"MDL_KM_MAX_K": 1024, "MDL_KM_ROWS": 128, "MDL_KM_SORT_ROWS": 2048, "MDL_KM_MEAN_ROWS": 1024}
    assert (R.KM_ROWS, R.MEAN_ROWS) == (defines["MDL_KM_ROWS"], defines["MDL_KM_MEAN_ROWS"])
    lib = _native.lib()
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)                          # exported by the built library
        assert fn.restype is res and fn.argtypes == args, name
    others = (_native.SIGNATURES, _native.VIEW_SIGNATURES, _native.STATS_SIGNATURES, _native.EXPLAIN_SIGNATURES, _native.REGRESS_SIGNATURES)
    assert not any(NAMES & set(o) for o in others)
    assert not any(set(defines) & set(o) for o in (_native._DEFINES, _native.VIEW_DEFINES, _native.STATS_DEFINES, _native.EXPLAIN_DEFINES,
                                                   _native.REGRESS_DEFINES))
    assert _build.CLUSTER_HEADER in _build._deps()


def test_a_header_that_repeats_a_name_is_refused():
    with open(_build.CLUSTER_HEADER) as f:
        text = f.read()
    sigs, _ = _native._parse_header(text.replace("mdl_kmeans_hist(", "mdl_bag_mean("))
    assert set(sigs) & set(_native.SIGNATURES)          # what the import-time check of _native looks for


def test_the_python_surface_is_exported():
    import madeleine_amd
    from madeleine_amd import cluster, functional as F
    from madeleine_amd.store import DeviceSlideStore
    for name in ("fit_kmeans", "assign_kmeans"):
        assert name in madeleine_amd.__all__ and getattr(madeleine_amd, name) is getattr(cluster, name)
    assert all(callable(getattr(F, n)) for n in ("kmeans_assign", "kmeans_update", "kmeans_seed", "kmeans_hist"))
    assert cluster.KMeansResult._fields == ("centroids", "labels", "dist", "counts", "inertia", "n_iter", "converged")
    assert callable(DeviceSlideStore.prototypes) and callable(DeviceSlideStore.prototype_histograms)
    assert (F.KM_ROWS, F.KM_MAX_K) == (128, 1024)


def test_no_cpu_fallback():
    from madeleine_amd import cluster
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cluster.fit_kmeans(torch.zeros(8, 2), 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cluster.assign_kmeans(torch.zeros(8, 2), torch.zeros(2, 2))


# ---- workspace queries and refusals --------------------------------------------------------------------------------------------------
def test_workspace_queries():
    lib = _native.lib()
    a, u, s, h = lib.mdl_kmeans_assign_ws_bytes, lib.mdl_kmeans_update_ws_bytes, lib.mdl_kmeans_seed_ws_bytes, lib.mdl_kmeans_hist_ws_bytes
    for n_chunks, k, D in ((11250, 64, 512), (1, 1, 1), (60, 129, 33), (0, 5, 4)):
        kp, dp = -(-k // 128) * 128, -(-D // 32) * 32
        need = 4 * kp * dp + 4 * kp + 12 * n_chunks
        assert need <= a(n_chunks, k, D) <= need + 4 * 256 and a(n_chunks, k, D) % 16 == 0
    assert a(-1, 5, 4) == ARG and a(5, 0, 4) == ARG and a(5, 5, 0) == ARG
    assert a(5, 1025, 4) == UNSUP and a(1 << 31, 5, 4) == UNSUP and a(5, 1024, 4) > 0
    for T, k, D in ((1440000, 256, 512), (1, 1, 1), (6730, 33, 33)):
        nsc, items = -(-T // 2048), T // 1024 + k
        need = 4 * k * nsc + 4 * k + 4 * (k + 1) + 8 * T + 4 * items * D
        assert need <= u(T, k, D) <= need + 5 * 256 and u(T, k, D) % 16 == 0
    assert u(0, 5, 4) == ARG and u(5, 0, 4) == ARG and u(5, 5, 0) == ARG and u(5, 1025, 4) == UNSUP and u(1 << 31, 5, 4) == UNSUP
    for n_chunks, T in ((11250, 1440000), (1, 1)):
        need = 12 * n_chunks + 5 * T
        assert need <= s(n_chunks, T) <= need + 4 * 256
    assert s(-1, 5) == ARG and s(5, 0) == ARG and s(5, 1 << 31) == UNSUP
    assert h(48, 256) == 0 and h(0, 1) == 0 and h(-1, 4) == ARG and h(4, 0) == ARG and h(4, 1025) == UNSUP and h(1 << 31, 4) == UNSUP


def _assign(**kw):
    a = dict(store=FAKE, dtype=0, row_stride=8, T_total=100, off=FAKE, n_bags=1, bag=FAKE, cu=FAKE, chunk_cu=FAKE, R=1, n_chunks=1, T=100,
             D=8, C=FAKE, k=4, labels=FAKE, dist=FAKE, stats=FAKE, ws=FAKE, stream=None)
    a.update(kw)
    return _native.lib().mdl_kmeans_assign(*a.values())


def _update(**kw):
    a = dict(store=FAKE, dtype=0, row_stride=8, T_total=100, off=FAKE, n_bags=1, bag=FAKE, cu=FAKE, R=1, T=100, D=8, labels=FAKE, C_in=FAKE,
             k=4, C_out=FAKE, counts=FAKE, ws=FAKE, stream=None)
    a.update(kw)
    return _native.lib().mdl_kmeans_update(*a.values())


def _seed(**kw):
    a = dict(store=FAKE, dtype=0, row_stride=8, T_total=100, off=FAKE, n_bags=1, bag=FAKE, cu=FAKE, chunk_cu=FAKE, R=1, n_chunks=1, T=100,
             D=8, u=FAKE, k=4, pos_out=FAKE, C_out=FAKE, ws=FAKE, stream=None)
    a.update(kw)
    return _native.lib().mdl_kmeans_seed(*a.values())


def _hist(**kw):
    a = dict(labels=FAKE, cu=FAKE, R=3, T=100, k=4, counts=FAKE, stream=None)
    a.update(kw)
    return _native.lib().mdl_kmeans_hist(*a.values())


@pytest.mark.parametrize("call,pointers", [
    (_assign, ("store", "off", "bag", "cu", "chunk_cu", "C", "labels", "dist", "stats", "ws")),
    (_update, ("store", "off", "bag", "cu", "labels", "C_in", "C_out", "counts", "ws")),
    (_seed, ("store", "off", "bag", "cu", "chunk_cu", "u", "pos_out", "C_out", "ws")),
    (_hist, ("labels", "cu", "counts"))])
def test_every_refusal_comes_before_a_launch(call, pointers):
    for p in pointers:
        assert call(**{p: None}) == ARG, p
    assert call(k=0) == ARG and call(T=0) == ARG and call(R=-1) == ARG
    assert call(k=1025) == UNSUP and call(T=1 << 31) == UNSUP and call(R=1 << 31) == UNSUP
    if call is not _hist:
        assert call(D=0) == ARG and call(row_stride=7) == ARG and call(dtype=3) == ARG and call(dtype=-1) == ARG
        assert call(T_total=-1) == ARG and call(n_bags=-1) == ARG
        for p, unit in (("store", 8), ("ws", 8), ("off", 4), ("cu", 4), ("bag", 2)):
            assert call(**{p: FAKE + unit}) == ALIGN, p
        assert call(k=1025, ws=FAKE + 8) == UNSUP and call(k=0, ws=FAKE + 8) == ARG          # (1), (2) before (3)
    if call in (_assign, _seed):
        assert call(n_chunks=-1) == ARG and call(n_chunks=1 << 31) == UNSUP and call(chunk_cu=FAKE + 4) == ALIGN
    if call is _assign:
        assert call(C=FAKE + 8) == ALIGN and call(stats=FAKE + 4) == ALIGN and call(labels=FAKE + 2) == ALIGN and call(dist=FAKE + 2) == ALIGN
    if call is _update:
        assert call(C_in=FAKE + 8) == ALIGN and call(C_out=FAKE + 8) == ALIGN and call(counts=FAKE + 4) == ALIGN and call(labels=FAKE + 2) == ALIGN
    if call is _seed:
        assert call(T=3, k=4) == ARG and call(C_out=FAKE + 8) == ALIGN and call(u=FAKE + 4) == ALIGN and call(pos_out=FAKE + 4) == ALIGN
    if call is _hist:
        assert call(cu=FAKE + 4) == ALIGN and call(labels=FAKE + 2) == ALIGN and call(counts=FAKE + 2) == ALIGN


# ---- the numpy contract against independent formulas ---------------------------------------------------------------------------------
def _data(T=1800, D=9, k=6, seed=0):
    g = np.random.default_rng(seed)
    centres = 4.0 * g.standard_normal((k, D))
    X = (centres[g.integers(0, k, T)] + 0.4 * g.standard_normal((T, D)) + np.linspace(-3, 3, D)).astype(np.float32)
    C = X[g.choice(T, k, replace=False)].copy()
    return X.astype(np.float64), C.astype(np.float64)


def test_the_model_against_independent_formulas():
    X, C = _data()
    X[7, 2] = np.nan
    X[900] = np.inf
    labels, dist = R.assign(X, C)
    assert labels[7] == labels[900] == -1 and np.isnan(dist[[7, 900]]).all()
    fin = R.finite_rows(X)
    brute = ((X[fin, None, :] - C[None, :, :]) ** 2).sum(2)          # the distances themselves, not the expanded form
    assert (labels[fin] == brute.argmin(1)).all() and np.allclose(dist[fin], brute.min(1), rtol=1e-10, atol=1e-9)
    assert np.isclose(R.inertia(dist), brute.min(1).sum())
    C2, counts = R.update(X, labels, C)
    for j in range(len(C)):
        assert counts[j] == (labels == j).sum() and np.allclose(C2[j], X[labels == j].mean(0))
    assert counts.sum() == fin.sum()
    # ties go to the lowest index; an empty cluster keeps its centroid
    Ct = np.concatenate([C, C[:2], np.full((1, C.shape[1]), 1e3)])
    lt, _ = R.assign(X, Ct)
    assert (lt == labels).all()
    assert (R.update(X, lt, Ct)[0][-1] == 1e3).all() and R.update(X, lt, Ct)[1][-3:].tolist() == [0, 0, 0]
    cu = np.array([0, 5, 5, 1000, len(X)])
    h = R.hist(labels, cu, len(C))
    assert h.sum() == fin.sum() and (h[1] == 0).all() and h[0].sum() == 5 and (h.sum(0) == counts).all()
    assert R.depth(1, 512) == 1 + 3 and R.depth(1025, 512) == 256 + 3 + 1 and R.depth(3000, 4) == 4 + 255 + 2


def test_the_seeding_model():
    g = np.random.default_rng(1)
    X = g.integers(-8, 9, (500, 5)).astype(np.float64)
    X[3] = np.nan
    u = g.random(6)
    pos = R.seed(X, u)
    assert len(set(pos.tolist())) == 6 and 3 not in pos
    fin = np.flatnonzero(R.finite_rows(X))
    assert pos[0] == fin[int(u[0] * len(fin))]
    mind = np.where(R.finite_rows(X), ((np.nan_to_num(X) - X[pos[0]]) ** 2).sum(1), 0.0)       # centre 1 by the definition, walked
    run, target = 0.0, u[1] * mind.sum()
    for t, m in enumerate(mind):
        run += m
        if run > target:
            break
    assert pos[1] == t
    assert R.seed(np.ones((10, 2)), np.array([0.55, 0.0, 0.95])).tolist() == [5, 0, 9]


def test_the_model_against_scipy_and_scikit_learn():
    X, C = _data(seed=2)
    labels, dist = R.assign(X, C)
    vq = pytest.importorskip("scipy.cluster.vq")
    code, d = vq.vq(X, C)
    assert (code == labels).all() and np.allclose(d ** 2, dist, rtol=1e-9, atol=1e-9)
    skc = pytest.importorskip("sklearn.cluster")
    km = skc.KMeans(n_clusters=len(C), init=C, n_init=1, max_iter=1, tol=0.0, algorithm="lloyd").fit(X)
    assert np.allclose(km.cluster_centers_, R.update(X, labels, C)[0], rtol=1e-9, atol=1e-9)


# ---- the checkers against seeded faults ----------------------------------------------------------------------------------------------
def _clean_int():
    g = np.random.default_rng(5)
    X = g.integers(-8, 9, (700, 6)).astype(np.float64)
    C = g.integers(-8, 9, (5, 6)).astype(np.float64)
    C[4] = C[1]                                                      # an exact tie for every row nearest to 1
    labels, dist = R.assign(X, C)
    return X, C, labels, dist.astype(np.float32)


def _clean_real():
    X, C = _data(T=2600, D=9, k=3, seed=7)
    X[11] = np.nan
    labels, d = R.assign(X, C)
    C32 = np.stack([X[labels == j].sum(0) / (labels == j).sum() for j in range(3)]).astype(np.float32)
    return X, C, labels, d.astype(np.float32), C32, np.bincount(labels[labels >= 0], minlength=3).astype(np.int64)


def test_the_clean_model_passes_its_checkers():
    X, C, labels, dist = _clean_int()
    assert R.check_assign_exact(X, C, labels, dist) == [] and R.check_assign(X, C, labels, dist) == []
    Cn, counts = R.update(X, labels, C)
    assert R.check_update(X, labels, C, Cn.astype(np.float32), counts, exact=True) == []
    X, C, labels, dist, C32, counts = _clean_real()
    assert R.check_assign(X, C, labels, dist) == [] and R.check_update(X, labels, C, C32, counts) == []
    assert counts.max() > R.MEAN_ROWS                                # a cluster of more than one mean chunk
    cu = np.array([0, 100, 100, len(X)])
    assert R.check_hist(labels, cu, 3, R.hist(labels, cu, 3)) == []


def test_seeded_faults_are_rejected():
    X, C, labels, dist = _clean_int()
    # 1. a tie broken to the higher index
    f = labels.copy()
    assert (labels == 1).any()
    f[np.flatnonzero(labels == 1)[0]] = 4
    assert R.check_assign_exact(X, C, f, dist) != []
    Xr, Cr, lr, dr, C32, counts = _clean_real()
    # 2. one tile's labels shifted by one row
    f = lr.copy()
    f[128:256] = np.roll(lr[128:256], 1)
    assert (f != lr).any() and R.check_assign(Xr, Cr, f, dr) != []
    # 3. a dropped tail row: the last row keeps the sentinel and NaN it was pre-filled with
    f, g = lr.copy(), dr.copy()
    f[-1], g[-1] = -7, np.nan
    assert R.check_assign(Xr, Cr, f, g) != []
    g = dr.copy()
    g[-1] = np.nan
    assert R.check_assign(Xr, Cr, lr, g) != []
    # 4. a centroid missing its last 1024-member chunk
    j = int(np.argmax(counts))
    members = np.flatnonzero(lr == j)
    last = (len(members) - 1) // R.MEAN_ROWS * R.MEAN_ROWS
    f = C32.copy()
    f[j] = (Xr[members[:last]].sum(0) / counts[j]).astype(np.float32)
    assert R.check_update(Xr, lr, Cr, f, counts) != []
    # 5. a count off by one
    f = counts.copy()
    f[0] += 1
    assert R.check_update(Xr, lr, Cr, C32, f) != []
    # 6. a stale centroid for a non-empty cluster
    f = C32.copy()
    f[1] = Cr[1].astype(np.float32)
    assert R.check_update(Xr, lr, Cr, f, counts) != []
    # 7. a NaN row given a label
    f = lr.copy()
    f[11] = 0
    assert R.check_assign(Xr, Cr, f, dr) != []
    # 8. a histogram that counts label -1
    cu = np.array([0, 100, len(Xr)])
    f = R.hist(lr, cu, 3)
    f[0, 0] += 1                                                     # row 11 of bag 0 is the NaN row
    assert R.check_hist(lr, cu, 3, f) != []
    # and: a dist one bound off, a label one cluster off, an empty cluster that moved
    g = dr.copy()
    g[5] += 4 * R.dist_bound(np.linalg.norm(Xr[5])[None], np.linalg.norm(Cr[lr[5]])[None], Xr.shape[1])[0] + 1e-3
    assert R.check_assign(Xr, Cr, lr, g) != []
    Ce = np.concatenate([Cr, np.full((1, Xr.shape[1]), 1e3)])
    le, _ = R.assign(Xr, Ce)
    Cn, cn = R.update(Xr, le, Ce)
    f = Cn.astype(np.float32)
    assert R.check_update(Xr, le, Ce, f, cn) == []
    f[3, 0] = 999.0
    assert R.check_update(Xr, le, Ce, f, cn) != []
