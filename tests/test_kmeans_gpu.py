"""K1-K4 (include/madeleine_amd_cluster.h) on the GPU, through the C ABI: bit-exact integer cases against the numpy model of
tests/_kmeans_ref.py (planted ties included), real data against the derived per-row and per-element bounds, Lloyd step by step from the
device's own centroids, a planted partition recovered exactly, the bit contracts (bag order, subsets, row stride, padded k, other
clusters' rows) and the edge cases.  Outputs and workspaces are pre-filled with NaN / a sentinel and guarded on both sides.

Shapes: bag lengths on both sides of a wave, of the 128-row assign chunk and of the 1024-member mean chunk, one absent bag mid-list
(T = 6730: four sort chunks of 2048), D in {4, 33, 512} (under one stage, odd, many stages), k on both sides of an MFMA column block and
of the 128-centroid tile."""
import numpy as np
import pytest
import torch

from madeleine_amd import _native, cluster
from madeleine_amd import functional as MF
from tests import _kmeans_ref as R

pytestmark = pytest.mark.gpu

LENS = [1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 3 * 1024 + 7]
BAGS = [0, 1, 2, 3, 4, 5, -1, 6, 7, 8, 9, 10, 11]
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
KS = [1, 2, 3, 31, 32, 33, 128, 129]
GUARD = 64
ARG = _native._DEFINES["MDL_E_ARG"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


class Source:
    """A store of bags of `lens` rows (one unlisted bag of 5 rows in front), rows `S` [sum(lens), D] fp32 on the host, kept as `dtype`
    at row stride `stride`; the call lists `bags` (-1: absent).  X: the call's rows in call order, fp64."""

    def __init__(self, S, lens, bags, dtype, stride, dev):
        D = S.shape[1]
        lens_all = [5] + list(lens)
        off = np.concatenate([[0], np.cumsum(lens_all)])
        full = torch.full((int(off[-1]), stride), float("nan"), dtype=dtype)
        full[:5, :D] = 7.0
        full[5:, :D] = S.to(dtype)
        self.rows = full.to(dev)[:, :D]
        n = np.array([0 if g < 0 else lens[g] for g in bags], np.int64)
        self.cu_h = np.concatenate([[0], np.cumsum(n)])
        ch = np.concatenate([[0], np.cumsum((n + R.KM_ROWS - 1) // R.KM_ROWS)])
        self.off = torch.from_numpy(off).to(dev)
        self.bag = torch.tensor([g + 1 if g >= 0 else -1 for g in bags], dtype=torch.int32, device=dev)
        self.cu, self.chunk_cu = torch.from_numpy(self.cu_h).to(dev), torch.from_numpy(ch).to(dev)
        self.T, self.n_chunks, self.D, self.R, self.dev = int(self.cu_h[-1]), int(ch[-1]), D, len(bags), dev
        o = off[1:]
        parts = [S[o[g] - 5:o[g] - 5 + lens[g]] for g in bags if g >= 0]
        self.X = torch.cat(parts).to(dtype).double().numpy() if parts else np.zeros((0, D))
        self.head = (self.rows, MF.STORE_DTYPES[dtype], stride, self.rows.shape[0], self.off, self.off.numel() - 1, self.bag, self.cu)


def guarded(n, dtype, fill, dev):
    full = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return full, full[GUARD:GUARD + n]


def untouched(full, n, fill):
    g = torch.cat([full[:GUARD], full[GUARD + n:]]).cpu()
    ref = torch.full_like(g, fill)
    return torch.equal(g.view(torch.uint8) if g.dtype.is_floating_point else g, ref.view(torch.uint8) if g.dtype.is_floating_point else ref)


def ws_for(query, dev, *sizes):
    n = getattr(_native.lib(), query)(*sizes)
    assert n >= 0, (query, sizes, n)
    full, inner = guarded(max(int(n), 16), torch.uint8, 0xA5, dev)
    return full, inner, max(int(n), 16)


def run_assign(src, C, labels_in=None):
    """mdl_kmeans_assign -> (labels, dist, changed, inertia) on the host; guards checked."""
    dev, T, k = src.dev, src.T, C.shape[0]
    Cd = torch.from_numpy(np.asarray(C, np.float32)).to(dev).contiguous()
    lf, lab = guarded(T, torch.int32, -7, dev)
    if labels_in is not None:
        lab.copy_(torch.from_numpy(labels_in).to(dev))
    df, dist = guarded(T, torch.float32, float("nan"), dev)
    sf, stats = guarded(2, torch.int64, -7, dev)
    wf, ws, wn = ws_for("mdl_kmeans_assign_ws_bytes", dev, src.n_chunks, k, src.D)
    MF._call("mdl_kmeans_assign", *src.head, src.chunk_cu, src.R, src.n_chunks, T, src.D, Cd, k, lab, dist, stats, ws, MF._stream())
    torch.cuda.synchronize()
    assert untouched(lf, T, -7) and untouched(df, T, float("nan")) and untouched(sf, 2, -7) and untouched(wf, wn, 0xA5)
    st = stats.cpu()
    return lab.cpu().numpy(), dist.cpu().numpy(), int(st[0]), float(st.view(torch.float64)[1])


def run_update(src, labels, C_prev):
    dev, T, k = src.dev, src.T, C_prev.shape[0]
    Cd = torch.from_numpy(np.asarray(C_prev, np.float32)).to(dev).contiguous()
    of, out = guarded(k * src.D, torch.float32, float("nan"), dev)
    cf, counts = guarded(k, torch.int64, -7, dev)
    wf, ws, wn = ws_for("mdl_kmeans_update_ws_bytes", dev, T, k, src.D)
    lab = torch.from_numpy(np.asarray(labels, np.int32)).to(dev)
    MF._call("mdl_kmeans_update", *src.head, src.R, T, src.D, lab, Cd, k, out, counts, ws, MF._stream())
    torch.cuda.synchronize()
    assert untouched(of, k * src.D, float("nan")) and untouched(cf, k, -7) and untouched(wf, wn, 0xA5)
    return out.cpu().numpy().reshape(k, src.D), counts.cpu().numpy()


def run_seed(src, u):
    dev, k = src.dev, len(u)
    ud = torch.from_numpy(np.asarray(u, np.float64)).to(dev)
    pf, pos = guarded(k, torch.int64, -7, dev)
    of, out = guarded(k * src.D, torch.float32, float("nan"), dev)
    wf, ws, wn = ws_for("mdl_kmeans_seed_ws_bytes", dev, src.n_chunks, src.T)
    MF._call("mdl_kmeans_seed", *src.head, src.chunk_cu, src.R, src.n_chunks, src.T, src.D, ud, k, pos, out, ws, MF._stream())
    torch.cuda.synchronize()
    assert untouched(pf, k, -7) and untouched(of, k * src.D, float("nan")) and untouched(wf, wn, 0xA5)
    return pos.cpu().numpy(), out.cpu().numpy().reshape(k, src.D)


def run_hist(src, labels, k):
    dev = src.dev
    cf, counts = guarded(src.R * k, torch.int32, -7, dev)
    lab = torch.from_numpy(np.asarray(labels, np.int32)).to(dev)
    MF._call("mdl_kmeans_hist", lab, src.cu, src.R, src.T, k, counts, MF._stream())
    torch.cuda.synchronize()
    assert untouched(cf, src.R * k, -7)
    return counts.cpu().numpy().reshape(src.R, k)


def int_rows(T, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, (T, D), generator=g).float()


def int_centroids(k, D, seed):
    """integers in [-8, 8] with planted duplicates: exact ties, which the lowest index wins"""
    C = int_rows(k, D, seed).numpy()
    if k >= 3:
        C[k - 1] = C[0]
    if k >= 32:
        C[17] = C[5]
        C[k - 2] = C[5]
    return C


def real_rows(T, D, seed, clustered=False):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(T, D, generator=g) + torch.linspace(-3.0, 3.0, D).unsqueeze(0)
    if clustered:
        X = 0.3 * X + 4.0 * torch.randn(7, D, generator=g)[torch.randint(0, 7, (T,), generator=g)]
    return X


def stride_for(D, dtype, wide):
    return D if not wide else D + (4 if D % 4 == 0 else 3)


# ---- bit-exact integer cases ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [4, 33, 512])
def test_integer_data_is_bit_exact(dev, D):
    T = sum(LENS)
    S = int_rows(T, D, 10 + D)
    for di, dtype in enumerate(DTYPES):
        src = Source(S, LENS, BAGS, dtype, stride_for(D, dtype, di != 1), dev)
        assert src.T == T
        for k in KS if dtype == torch.float32 else [3, 33, 129]:
            C = int_centroids(k, D, 100 + k)
            labels, dist, changed, inertia = run_assign(src, C)
            assert R.check_assign_exact(src.X, C, labels, dist) == [], (D, dtype, k)
            assert changed == T and inertia == R.inertia(dist.astype(np.float64))
            Cn, counts = run_update(src, labels, C)
            assert R.check_update(src.X, labels, C, Cn, counts, exact=True) == [], (D, dtype, k)
            assert R.check_hist(labels, src.cu_h, k, run_hist(src, labels, k)) == []
            # the labels assign has just written are not "changed" the second time
            l2, d2, changed2, in2 = run_assign(src, C, labels)
            assert changed2 == 0 and (l2 == labels).all() and (d2.view(np.uint32) == dist.view(np.uint32)).all() and in2 == inertia


def test_integer_k_1024_once(dev):
    D, k = 33, 1024
    src = Source(int_rows(sum(LENS), D, 5), LENS, BAGS, torch.float32, D + 3, dev)
    C = int_centroids(k, D, 6)
    labels, dist, _, _ = run_assign(src, C)
    assert R.check_assign_exact(src.X, C, labels, dist) == []
    Cn, counts = run_update(src, labels, C)
    assert R.check_update(src.X, labels, C, Cn, counts, exact=True) == []
    assert R.check_hist(labels, src.cu_h, k, run_hist(src, labels, k)) == []


@pytest.mark.parametrize("D", [4, 33, 512])
def test_integer_seeding_equals_searchsorted(dev, D):
    S = int_rows(sum(LENS), D, 20 + D)
    S[77] = float("nan")
    S[4000, D - 1] = float("inf")
    rng = np.random.default_rng(D)
    for dtype, k in ((torch.float32, 33), (torch.bfloat16, 5), (torch.float16, 2)):
        src = Source(S, LENS, BAGS, dtype, stride_for(D, dtype, True), dev)
        u = rng.random(k)
        u[0] = 0.0 if dtype == torch.float16 else u[0]
        pos, C = run_seed(src, u)
        assert (pos == R.seed(src.X, u)).all(), (D, dtype, pos, R.seed(src.X, u))
        assert (C.view(np.uint32) == src.X[pos].astype(np.float32).view(np.uint32)).all()
    # all rows equal: every total is 0, and the rank rule picks
    src = Source(torch.ones(300, D), [300], [0], torch.float32, D, dev)
    u = np.array([0.5, 0.0, 0.999])
    pos, _ = run_seed(src, u)
    assert pos.tolist() == [150, 0, 299] == R.seed(src.X, u).tolist()


# ---- real data: every row and element within its bound --------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [4, 33, 512])
def test_real_data_within_the_bounds(dev, D):
    T = sum(LENS)
    for ci, dtype in enumerate(DTYPES):
        S = real_rows(T, D, 30 + D + ci, clustered=ci == 1)
        src = Source(S, LENS, BAGS, dtype, stride_for(D, dtype, ci != 2), dev)
        for k in [2, 33, 129] if ci else [1, 31, 32, 128]:
            C = src.X[np.random.default_rng(k).choice(T, k, replace=False)].astype(np.float32)
            labels, dist, changed, inertia = run_assign(src, C)
            assert R.check_assign(src.X, C, labels, dist) == [], (D, dtype, k)
            d64, xn, cn = R.distances(src.X, C)
            dL = d64[np.arange(T), labels]
            assert abs(inertia - np.maximum(dL, 0).sum()) <= T * R.dist_bound(xn, cn[labels], D).max()
            assert changed == T
            Cn, counts = run_update(src, labels, C)
            assert R.check_update(src.X, labels, C, Cn, counts) == [], (D, dtype, k)


def test_lloyd_step_by_step(dev):
    """Six iterations of fit_kmeans(init=C, max_iter=1): each one's labels and new centroids against the fp64 model applied to the
    device's OWN previous centroids, so no trajectory equality is asked and a near-tie cannot make this flaky."""
    T, D, k = 3000, 33, 7
    X = real_rows(T, D, 3, clustered=True).to(dev)
    X64 = X.double().cpu().numpy()
    C = X[torch.from_numpy(np.random.default_rng(1).choice(T, k, replace=False)).to(dev)].clone()
    for it in range(6):
        res = cluster.fit_kmeans(X, k, init=C, max_iter=1)
        assert res.n_iter == 1 and not res.converged
        labels, dist = res.labels.cpu().numpy(), res.dist.cpu().numpy()
        assert R.check_assign(X64, C.cpu().numpy(), labels, dist) == [], it
        assert R.check_update(X64, labels, C.cpu().numpy(), res.centroids.cpu().numpy(), res.counts.cpu().numpy()) == [], it
        C = res.centroids


@pytest.mark.parametrize("k", [2, 3, 33, 129])
@pytest.mark.parametrize("D", [4, 33, 512])
def test_planted_partition_is_recovered(dev, D, k):
    g = np.random.default_rng(D * 1000 + k)
    centres = set()
    while len(centres) < k:                                          # distinct even integers in [-8, 8]: two centres are >= 2 apart
        centres.add(tuple((2 * g.integers(-4, 5, D)).tolist()))
    centres = np.array(sorted(centres), np.float64)
    T = 40 * k + 13
    planted = np.concatenate([np.arange(k), g.integers(0, k, T - k)]).astype(np.int32)
    X = centres[planted] + g.integers(-2, 3, (T, D)) / 8.0          # noise in multiples of 1/8 within +-1/4: exact in bf16
    init = X[:k].copy()                                              # one row per planted cluster
    # the test's own input first, in fp64: at every iteration the gap between best and second best is >= 16 x the assign bound
    C = init
    for _ in range(3):
        d64, xn, cn = R.distances(X, C)
        order = np.sort(d64, 1)
        E = R.assign_bound(xn, cn, D).max(1)
        if k > 1:
            assert ((order[:, 1] - order[:, 0]) >= 16 * 2 * E).all()
        lab, _ = R.assign(X, C)
        assert (lab == planted).all()
        C, cnt = R.update(X, lab, C)
    for dtype in (torch.float32, torch.bfloat16):
        res = cluster.fit_kmeans(torch.from_numpy(X).to(dtype).to(dev), k, init=torch.from_numpy(init).float().to(dev), max_iter=10)
        assert res.converged and res.n_iter <= 3
        assert (res.labels.cpu().numpy() == planted).all()
        assert (res.counts.cpu().numpy() == np.bincount(planted, minlength=k)).all()


# ---- bit contracts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_bit_contracts(dev, dtype):
    D, k, T = 33, 33, sum(LENS)
    S = real_rows(T, D, 9)
    C = S[::200][:k].to(dtype).float().numpy()
    base = Source(S, LENS, BAGS, dtype, D, dev)
    l0, d0, _, _ = run_assign(base, C)
    start = {g: int(base.cu_h[i]) for i, g in enumerate(BAGS) if g >= 0}

    def same(src, bags, Ck=C):
        l, d, _, _ = run_assign(src, Ck)
        for i, g in enumerate(bags):
            if g < 0:
                continue
            a, b, n = int(src.cu_h[i]), start[g], LENS[g]
            assert (l[a:a + n] == l0[b:b + n]).all() and (d[a:a + n].view(np.uint32) == d0[b:b + n].view(np.uint32)).all(), g
        return l

    perm = [11, 3, -1, 0, 9, 10, 1, 2, 8, 7, 6, 5, 4]
    same(Source(S, LENS, perm, dtype, D, dev), perm)                                  # a permuted bag list
    sub = [9, 2, 11]
    same(Source(S, LENS, sub, dtype, D, dev), sub)                                    # a subset of the bags
    same(Source(S, LENS, BAGS, dtype, D + 7, dev), BAGS)                              # another row stride
    far = np.concatenate([C, np.full((130 - k, D), 1.0e4, np.float32)])               # k padded with far-away centroids: a second tile
    same(base, BAGS, far)
    # a cluster's centroid bits do not change when rows of OTHER clusters are removed
    Cn, counts = run_update(base, l0, C)
    j = int(np.argmax(counts))
    thin = l0.copy()
    thin[(l0 != j) & (np.arange(T) % 3 == 0)] = -1
    Ct, ct = run_update(base, thin, C)
    assert ct[j] == counts[j] and (Ct[j].view(np.uint32) == Cn[j].view(np.uint32)).all()
    # two calls give identical bits
    l1, d1, _, _ = run_assign(base, C)
    C1, c1 = run_update(base, l0, C)
    assert (l1 == l0).all() and (d1.view(np.uint32) == d0.view(np.uint32)).all() and (C1.view(np.uint32) == Cn.view(np.uint32)).all()


# ---- edge cases ------------------------------------------------------------------------------------------------------------------------
def test_edge_cases(dev):
    D, T = 33, 700
    S = real_rows(T, D, 4)
    S[5, 3] = float("nan")
    S[130] = float("inf")
    S[699, 32] = float("-inf")
    src = Source(S, [300, 400], [0, 1], torch.float32, D + 3, dev)
    C = np.concatenate([src.X[[10, 20, 30]], np.full((1, D), 500.0)]).astype(np.float32)          # cluster 3 attracts nobody
    labels, dist, changed, inertia = run_assign(src, C)
    assert R.check_assign(src.X, C, labels, dist) == []
    assert (labels[[5, 130, 699]] == -1).all() and np.isnan(dist[[5, 130, 699]]).all() and changed == T - 3
    fin = labels >= 0
    d64, xn, cn = R.distances(src.X[fin], C)
    assert abs(inertia - np.maximum(d64[np.arange(fin.sum()), labels[fin]], 0).sum()) <= T * R.dist_bound(xn, cn[labels[fin]], D).max()
    Cn, counts = run_update(src, labels, C)
    assert R.check_update(src.X, labels, C, Cn, counts) == []
    assert counts[3] == 0 and (Cn[3] == 500.0).all() and counts.sum() == T - 3 and np.isfinite(Cn).all()
    h = run_hist(src, labels, 4)
    assert R.check_hist(labels, src.cu_h, 4, h) == [] and h.sum() == T - 3
    # k = 1
    l1, d1, _, _ = run_assign(src, C[:1])
    assert (l1[fin] == 0).all() and R.check_assign(src.X, C[:1], l1, d1) == []
    # T < k is refused, by the library and by fit_kmeans
    small = Source(real_rows(3, D, 1), [3], [0], torch.float32, D, dev)
    ud = torch.zeros(4, dtype=torch.float64, device=dev)
    out = torch.empty(4 * D, device=dev)
    pos = torch.empty(4, dtype=torch.int64, device=dev)
    rc = _native.lib().mdl_kmeans_seed(small.rows.data_ptr(), 0, D, 3, small.off.data_ptr(), 2, small.bag.data_ptr(), small.cu.data_ptr(),
                                       small.chunk_cu.data_ptr(), 1, 1, 3, D, ud.data_ptr(), 4, pos.data_ptr(), out.data_ptr(),
                                       out.data_ptr(), 0)
    assert rc == ARG
    with pytest.raises(ValueError):
        cluster.fit_kmeans(small.rows[5:], 4)


def test_fit_kmeans_seeded_runs(dev):
    """k-means++ and random init end to end: reproducible bits, labels consistent with the centroids' predecessors, n_init keeps the best."""
    X = real_rows(2000, 33, 8, clustered=True).to(dev)
    a = cluster.fit_kmeans(X, 7, seed=3, max_iter=100)
    b = cluster.fit_kmeans(X, 7, seed=3, max_iter=100)
    assert a.n_iter == b.n_iter and torch.equal(a.labels, b.labels) and torch.equal(a.centroids, b.centroids) and a.inertia == b.inertia
    assert a.converged and int(a.counts.sum()) == 2000
    lab, dist = cluster.assign_kmeans(X, a.centroids)
    assert torch.equal(lab, a.labels)
    r = cluster.fit_kmeans(X, 7, init="random", seed=1, n_init=3, max_iter=20)
    singles = [cluster.fit_kmeans(X, 7, init="random", seed=1 + i, max_iter=20).inertia for i in range(3)]
    assert r.inertia == min(singles)
