"""The retrieval kernels (X1) on the GPU: bit-exact against the numpy reference on integer data at every shape where the kernels take
another path, cosine retrieval against fp64 under the derived tolerance on ambiguity-free cohorts, the bit contract (chunking, stride,
position), degenerate and non-finite inputs, same-cohort neighbours, no host synchronisation, the launcher's own chunking, and
cross_stain_retrieval end to end on a small store with and without stain encoding."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from madeleine_amd import functional as MF
from oracle import recipe
from tests import _retrieval_ref as RR

pytestmark = pytest.mark.gpu

BM, BN = MF.RETR_ROW_BLOCK, MF.RETR_COL_TILE


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def host(res):
    """A Retrieval on the host: numpy arrays, None kept."""
    return tuple(None if t is None else t.cpu().numpy() for t in res)


def same_bits(a, b):
    """Two host results equal bit for bit (NaNs by their bits, -0 apart from +0)."""
    for x, y in zip(a, b):
        if x is None or y is None:
            assert x is None and y is None
            continue
        assert x.shape == y.shape and x.dtype == y.dtype
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)


# ------------------------------------------------------------------------------------------------ 1. exact
# (n, m): one row and column; both sides of the row block (BM) and of the column tile (BN); n < m across a tile boundary; three
# column tiles, which col_chunks = 2 cuts 2 + 1 and the launcher into one each; m small enough for k = m and k > m.
EDGES = [(1, 1), (33, 40), (BM - 1, BN - 1), (BM, BN), (BM + 1, BN + 1), (BM + 1, 2 * BN + 1), (2 * BM + 1, 2 * BN + 1), (100, 3 * BN)]
DIMS = [1, 7, 8, 9, 77, 512]


@functools.lru_cache(maxsize=None)
def integer_case(n, m, d):
    Q, K = RR.integers(n, m, d, 0.5 + n + 3 * m + d)
    S = (Q.astype(np.int64) @ K.astype(np.int64).T)
    assert np.abs(S).max() < 2 ** 24
    return Q, K, S.astype(np.float32)


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("n,m", EDGES, ids=["%dx%d" % e for e in EDGES])
def test_exact_on_integer_data(dev, n, m, d):
    assert (BM, BN) == (128, 128)      # the kernels' constants the list above is built from
    Q, K, S = integer_case(n, m, d)
    Qd, Kd = torch.from_numpy(Q).to(dev), torch.from_numpy(K).to(dev)
    ks = [1, 5, 64] + ([m, m + 3] if m + 3 <= MF.RETR_MAX_K else [])
    for k in ks:
        want = RR.exact(S, True, False, k)
        for chunks in (0, 2):
            got = host(MF.retrieval(Qd, Kd, k=k, metric="dot", paired=True, col_chunks=chunks))
            same_bits(got, want)
    want = RR.exact(S, False, False, 5)
    got = host(MF.retrieval(Qd, Kd, k=5, metric="dot", paired=False))
    assert got[0] is None and got[1] is None and got[2] is None
    same_bits(got, want)
    got = host(MF.retrieval(Qd, Kd, k=0, metric="dot", paired=True))
    assert got[3] is None and got[4] is None
    same_bits(got, RR.exact(S, True, False, 0))


def test_exact_has_ties_everywhere():
    """What makes the exact test a test of the order: at d = 7 most rows tie with their partner somewhere, many inside their top-5."""
    _, _, S = integer_case(BM + 1, 2 * BN + 1, 7)
    g, e, _, ti, tv = RR.exact(S, True, False, 5)
    assert (e > 0).mean() > 0.5 and (tv[:, :-1] == tv[:, 1:]).any(1).mean() > 0.2


# ------------------------------------------------------------------------------------------------ 2. cosine against fp64
@functools.lru_cache(maxsize=None)
def cosine_case(n, m, d, noise):
    Q, K = RR.cohort(n, m, d, noise, RR.SEED)
    S64 = RR.cosine64(Q, K)
    return Q, K, S64, RR.bounds(S64, RR.tol(d))


def check_cosine(dev, n, m, d, noise, k, col_chunks=0):
    Q, K, _, _ = cosine_case(n, m, d, noise)
    return check_cosine_result(n, m, d, noise, k, host(MF.retrieval(torch.from_numpy(Q).to(dev), torch.from_numpy(K).to(dev), k=k, col_chunks=col_chunks)))


def check_cosine_result(n, m, d, noise, k, res):
    """The bounds of check_cosine on `res`, the host() of one retrieval of cosine_case(n, m, d, noise) with this k."""
    Q, K, S64, (lo, hi, pair) = cosine_case(n, m, d, noise)
    t = RR.tol(d)
    assert int((lo != hi).sum()) == 0      # the cohort excuses nothing (asserted on the CPU too)
    g, e, ps, ti, tv = res
    err = float(np.abs(ps.astype(np.float64) - pair).max())
    print("(%d, %d, %d, %s): max |pair_sim - s64| %.3e, tol %.3e; median rank %.1f, worst %d"
          % (n, m, d, noise, err, t, np.median(1 + g + e), (1 + g + e).max()))
    assert (lo <= g).all() and (g + e <= hi).all()
    assert err <= t
    kk = min(k, m)
    rows = np.arange(n)[:, None]
    assert (ti[:, :kk] >= 0).all() and (ti[:, :kk] < m).all() and (ti[:, kk:] == -1).all() and (tv[:, kk:] == -np.inf).all()
    at = S64[rows, ti[:, :kk]]
    assert np.abs(tv[:, :kk].astype(np.float64) - at).max() <= t
    assert (tv[:, :kk - 1] >= tv[:, 1:kk]).all()
    assert all(len(set(r)) == kk for r in ti[:, :kk].tolist())
    left = S64.copy()
    left[rows, ti[:, :kk]] = -np.inf
    assert (left.max(1) <= tv[:, kk - 1].astype(np.float64) + 2 * t).all()
    return g, e, ps, ti, tv


@pytest.mark.parametrize("n,m,d,noise", RR.COSINE_COHORTS, ids=lambda v: str(v))
def test_cosine_against_fp64(dev, n, m, d, noise):
    check_cosine(dev, n, m, d, noise, 10)


# ------------------------------------------------------------------------------------------------ 3. invariance
def test_col_chunks_keep_the_bits(dev):
    Q, K, _, _ = cosine_case(257, 400, 77, 3)
    Qd, Kd = torch.from_numpy(Q).to(dev), torch.from_numpy(K).to(dev)
    base = host(MF.retrieval(Qd, Kd, k=10, col_chunks=1))
    for c in (2, 7, 0):
        same_bits(host(MF.retrieval(Qd, Kd, k=10, col_chunks=c)), base)
    Q, K, _, _ = cosine_case(1153, 1153, 512, 4)
    Qd, Kd = torch.from_numpy(Q).to(dev), torch.from_numpy(K).to(dev)
    assert MF.retrieval_chunks(1153, 1153, 7)[0] == 5 and MF.retrieval_chunks(1153, 1153, 0)[0] == 10
    base = host(MF.retrieval(Qd, Kd, k=64, col_chunks=1))
    for c in (2, 7, 0):
        same_bits(host(MF.retrieval(Qd, Kd, k=64, col_chunks=c)), base)


@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_row_stride_keeps_the_bits(dev, metric):
    """Column slices of wider buffers (ld = d + 24) give the bits of the contiguous call."""
    n, m, d = 150, 260, 77
    Q, K = RR.cohort(n, m, d + 24, 2, 0.75)
    Qw, Kw = torch.from_numpy(Q).to(dev), torch.from_numpy(K).to(dev)
    Qs, Ks = Qw[:, :d], Kw[:, :d]
    assert not Qs.is_contiguous() and not Ks.is_contiguous()
    same_bits(host(MF.retrieval(Qs, Ks, k=7, metric=metric)), host(MF.retrieval(Qs.contiguous(), Ks.contiguous(), k=7, metric=metric)))


def test_position_in_the_gallery_keeps_the_bits(dev):
    """The gallery's non-partner rows permuted and extra rows appended: pair_sim keeps its bits, every old similarity is found again
    with its bits under its new index, and the counts can only grow by what the new rows add."""
    n, m, d, extra = 140, 300, 64, 45
    Q, K = RR.cohort(n, m + extra, d, 2, 1.25)
    perm = np.arange(m)
    perm[n:] = n + np.argsort(RR._field(m - n, 1, 3.3, 1.1, 999.9, 0.1)[:, 0])      # new row j is old row perm[j]
    K1, K2 = K[:m], np.concatenate([K[:m][perm], K[m:]])
    Qd = torch.from_numpy(Q).to(dev)
    a = host(MF.retrieval(Qd, torch.from_numpy(K1.copy()).to(dev), k=64))
    b = host(MF.retrieval(Qd, torch.from_numpy(K2.copy()).to(dev), k=64))
    same_bits((a[2],), (b[2],))
    assert (b[0] >= a[0]).all() and (b[0] + b[1] >= a[0] + a[1]).all() and (b[0] - a[0] <= extra).all()
    inv = np.empty(m, dtype=np.int64)
    inv[perm] = np.arange(m)
    for i in range(n):
        old = {int(inv[j]): v.tobytes() for j, v in zip(a[3][i], a[4][i])}
        new = {int(j): v.tobytes() for j, v in zip(b[3][i], b[4][i])}
        shared = set(old) & set(new)
        assert shared and all(old[j] == new[j] for j in shared)
        # whatever of the old top-k was pushed out lies behind the new list's last entry
        assert all(np.frombuffer(old[j], np.float32)[0] <= b[4][i][-1] for j in set(old) - shared)


# ------------------------------------------------------------------------------------------------ 4. degenerate
def test_every_row_equal(dev):
    from madeleine_amd import retrieval_metrics
    n, m, d = 70, 150, 40
    row = RR.cohort(1, 1, d, 0, 0.3)[0]
    Qd = torch.from_numpy(np.repeat(row, n, 0)).to(dev)
    Kd = torch.from_numpy(np.repeat(row, m, 0)).to(dev)
    for metric in ("cosine", "dot"):
        r = MF.retrieval(Qd, Kd, k=5, metric=metric)
        g, e, ps, ti, tv = host(r)
        assert (g == 0).all() and (e == m - 1).all()
        assert (ti == np.arange(5)[None, :]).all() and (tv == ps[:, None]).all()      # ties by the lower index
        met = retrieval_metrics(r.greater, r.equal)
        assert met["recall@1"] == 0.0 and met["recall_optimistic@1"] == 1.0 and met["median_rank"] == float(m)


def test_duplicate_of_the_partner_adds_one_to_equal(dev):
    Q, K, _, _ = cosine_case(257, 400, 77, 3)
    Qd = torch.from_numpy(Q).to(dev)
    a = host(MF.retrieval(Qd, torch.from_numpy(K).to(dev), k=3))
    K2 = K.copy()
    K2[333] = K[200]                   # a distractor row becomes a copy of the partner of query 200
    b = host(MF.retrieval(Qd, torch.from_numpy(K2).to(dev), k=3))
    was_greater = int(RR.keys(a[2][200:201])[0]) < int(RR.keys(cosine_entry(dev, Q[200], K[333]))[0])
    assert b[1][200] == a[1][200] + 1 and b[0][200] == a[0][200] - int(was_greater)
    same_bits((a[2],), (b[2],))
    others = np.arange(257) != 200
    assert (np.abs(b[0][others] - a[0][others]) <= 1).all()


def cosine_entry(dev, q, k):
    """The device's similarity of two rows, alone: its bits depend on the two rows only."""
    r = MF.retrieval(torch.from_numpy(q[None].copy()).to(dev), torch.from_numpy(k[None].copy()).to(dev))
    return np.float32(r.pair_sim.cpu().numpy()[0])


def test_zero_rows(dev):
    """A zero query has cosine 0 with everything (x / max(|x|, 1e-12)): all ties.  A zero partner scores 0 against its query."""
    Q, K = RR.cohort(40, 60, 24, 1, 0.6)
    Q, K = Q.copy(), K.copy()
    Q[5] = 0
    K[9] = 0
    g, e, ps, ti, tv = host(MF.retrieval(torch.from_numpy(Q).to(dev), torch.from_numpy(K).to(dev), k=4))
    assert g[5] == 0 and e[5] == 59 and ps[5] == 0 and ti[5].tolist() == [0, 1, 2, 3] and (tv[5] == 0).all()
    s9, t = np.delete(RR.cosine64(Q[9:10], K)[0], 9), RR.tol(24)
    assert ps[9] == 0 and int((s9 > t).sum()) <= g[9] and g[9] + e[9] <= int((s9 >= -t).sum())


@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_nan_and_inf_rows(dev, metric):
    n, m, d = 50, 140, 33
    Q, K = RR.cohort(n, m, d, 1, 0.9)
    Q, K = Q.copy(), K.copy()
    Q[7, 3] = np.nan            # a NaN query row: every similarity NaN
    K[11, 0] = np.nan           # a NaN partner row (query 11) that is a NaN non-partner for everyone else
    K[130, 5] = np.nan          # a NaN distractor
    g, e, ps, ti, tv = host(MF.retrieval(torch.from_numpy(Q).to(dev), torch.from_numpy(K).to(dev), k=m if m <= 64 else 64, metric=metric))
    clean = host(MF.retrieval(torch.from_numpy(Q).to(dev), torch.from_numpy(np.delete(K, 130, 0)).to(dev), k=64, metric=metric))
    assert np.isnan(ps[7]) and g[7] == m - 1 and e[7] == 0
    assert np.isnan(tv[7]).all() and ti[7].tolist() == list(range(64))       # all NaN: ties, the lower index first
    assert np.isnan(ps[11]) and g[11] == m - 1 and e[11] == 0
    ok = np.ones(n, dtype=bool)
    ok[[7, 11]] = False
    assert not np.isnan(ps[ok]).any() and not np.isnan(tv[ok]).any()          # 138 numbers come before the two NaNs
    assert not np.isin(ti[ok], [11, 130]).any()
    # the NaN distractor is never ahead of a number: the counts are those of the gallery without it
    assert (g[ok] == clean[0][ok]).all() and (e[ok] == clean[1][ok]).all()
    # the last places of a full list belong to the NaNs
    full = host(MF.retrieval(torch.from_numpy(Q[:3]).to(dev), torch.from_numpy(K[:40]).to(dev), k=40, paired=False, metric=metric))
    assert (full[3][:, -1] == 11).all() and np.isnan(full[4][:, -1]).all() and not np.isnan(full[4][:, :-1]).any()


def test_inf_entries_dot(dev):
    """metric 'dot' with +-inf entries: +inf first, -inf after every number and before a NaN; inf - inf and 0 inf are NaN similarities."""
    d = 8
    Q = np.zeros((2, d), dtype=np.float32)
    Q[:, 0] = 1.0
    Q[1, 1] = 1.0
    K = np.zeros((6, d), dtype=np.float32)
    K[0, 0], K[1, 0], K[2, 0], K[3, 0], K[4, 0] = 2.0, -np.inf, np.inf, -3.0, np.nan
    K[5, 0], K[5, 1] = np.inf, -np.inf          # query 0: inf + 0 (-inf), query 1: inf - inf -- NaN both
    g, e, ps, ti, tv = host(MF.retrieval(torch.from_numpy(Q).to(dev), torch.from_numpy(K).to(dev), k=6, metric="dot"))
    for i in range(2):
        assert ti[i].tolist() == [2, 0, 3, 1, 4, 5]
        assert tv[i, :4].tolist() == [np.inf, 2.0, -3.0, -np.inf] and np.isnan(tv[i, 4:]).all()
    assert ps.tolist() == [2.0, -np.inf] and g.tolist() == [1, 3] and e.tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ 5. neighbours
@pytest.mark.parametrize("n,d,k", [(1, 9, 3), (40, 9, 64), (BM + 1, 7, 5), (2 * BN + 1, 77, 64)])
def test_exclude_diag_neighbours_exact(dev, n, d, k):
    from madeleine_amd import slide_neighbours
    Q, _, _ = integer_case(n, n, d)
    S = (Q.astype(np.int64) @ Q.astype(np.int64).T).astype(np.float32)
    want = RR.exact(S, False, True, k)
    Qd = torch.from_numpy(Q).to(dev)
    got = host(MF.retrieval(Qd, None, k=k, metric="dot", paired=False, exclude_diag=True))
    same_bits(got, want)
    assert not (got[3] == np.arange(n)[:, None]).any()
    idx, sim = slide_neighbours(Qd, k, metric="dot")
    same_bits((idx.cpu().numpy(), sim.cpu().numpy()), want[3:])


def test_slide_neighbours_cosine(dev):
    from madeleine_amd import slide_neighbours
    n, d, k = 300, 64, 8
    E = RR.cohort(n, n, d, 2, RR.SEED)[1]
    idx, sim = slide_neighbours(torch.from_numpy(E).to(dev), k)
    idx, sim = idx.cpu().numpy(), sim.cpu().numpy()
    S64 = RR.cosine64(E, E)
    np.fill_diagonal(S64, -np.inf)
    rows = np.arange(n)[:, None]
    t = RR.tol(d)
    assert not (idx == rows).any() and np.abs(sim - S64[rows, idx]).max() <= t and (sim[:, :-1] >= sim[:, 1:]).all()
    S64[rows, idx] = -np.inf
    assert (S64.max(1) <= sim[:, -1] + 2 * t).all()


# ------------------------------------------------------------------------------------------------ 6. no host synchronisation
def test_no_host_synchronisation(dev):
    Q, K, _, _ = cosine_case(300, 300, 64, 2)
    Qd, Kd = torch.from_numpy(Q).to(dev), torch.from_numpy(K).to(dev)
    want = MF.retrieval(Qd, Kd, k=10)          # warm-up: library load, allocator
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = MF.retrieval(Qd, Kd, k=10)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    same_bits(host(got), host(want))


def test_retrieval_issues_no_library_gemm_sort_or_topk(dev):
    """Under the torch profiler a retrieval call and the whole cross_stain_retrieval of a stain-encoded model issue no aten GEMM, sort
    or top-k op: the similarities, the counts and the lists all come from libmadeleine_amd.so."""
    from torch.profiler import ProfilerActivity, profile
    from madeleine_amd import DeviceSlideStore, cross_stain_retrieval, slide_neighbours
    banned = {"aten::mm", "aten::addmm", "aten::bmm", "aten::baddbmm", "aten::_scaled_mm", "aten::linear", "aten::matmul", "aten::einsum",
              "aten::mv", "aten::addmv", "aten::topk", "aten::sort", "aten::argsort"}
    Q, K, _, _ = cosine_case(300, 300, 64, 2)
    Qd, Kd = torch.from_numpy(Q).to(dev), torch.from_numpy(K).to(dev)
    st = DeviceSlideStore(_store_bags(), ["c%d" % i for i in range(N_CASES)], MODS, dev)
    model = _model(dev, True).eval()

    def work():
        MF.retrieval(Qd, Kd, k=10)
        slide_neighbours(Qd, 5)
        return cross_stain_retrieval(st, model)

    work()
    with profile(activities=[ProfilerActivity.CPU]) as prof:
        res = work()
    torch.cuda.synchronize()
    names = {e.name for e in prof.events()}
    assert res["HER2"]["n"] == N_CASES - len(NO_HER2) and not (names & banned), sorted(names & banned)


# ------------------------------------------------------------------------------------------------ 7. the launcher's own chunking
def test_launcher_chosen_chunks(dev):
    n, m, d, noise = RR.LAUNCHER_COHORT
    assert (n, m, d) == (4096, 4096, 512) and MF.retrieval_chunks(n, m, 0)[0] > 1
    a = check_cosine(dev, n, m, d, noise, 10)
    Q, K, _, _ = cosine_case(n, m, d, noise)
    b = host(MF.retrieval(torch.from_numpy(Q).to(dev), torch.from_numpy(K).to(dev), k=10, col_chunks=1))
    same_bits(a, b)


# ------------------------------------------------------------------------------------------------ 8. end to end
MODS = ["HE", "HER2", "ER"]
D_IN = 64
N_CASES = 8
NO_HER2 = (2, 5)
ONLY_ER = 3


def _model(dev, stain_encoding):
    from madeleine_amd import MADELEINE
    cfg = SimpleNamespace(MODALITIES=MODS, wsi_encoder="abmil", patch_embedding_dim=D_IN, wsi_encoder_hidden_dim=512,
                          activation="softmax", n_heads=4)
    m = MADELEINE(cfg, stain_encoding=stain_encoding)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.state_dict_recipe(shapes, "retrieval").items()}, strict=True)
    return m.to(dev)


def _store_bags():
    """8 cases x 3 modalities, bags of 40 .. 300 rows: every patch of a case is the case's own vector plus noise, so a case's slides
    resemble each other.  HER2 is missing for two cases; ER exists for one case only."""
    g = torch.Generator().manual_seed(11)
    bags = []
    for c in range(N_CASES):
        centre = 2.0 * torch.randn(D_IN, generator=g)
        case = []
        for mi in range(len(MODS)):
            rows = int(torch.randint(40, 301, (1,), generator=g))
            bag = centre + 0.5 * torch.randn(rows, D_IN, generator=g)
            absent = (mi == 1 and c in NO_HER2) or (mi == 2 and c != ONLY_ER)
            case.append(None if absent else bag)
        bags.append(case)
    return bags


@pytest.mark.parametrize("stain_encoding", [False, True], ids=["plain", "stain-encoded"])
def test_cross_stain_retrieval_end_to_end(dev, stain_encoding):
    from madeleine_amd import DeviceSlideStore, cross_stain_retrieval
    bags = _store_bags()
    st = DeviceSlideStore(bags, ["c%d" % i for i in range(N_CASES)], MODS, dev)
    model = _model(dev, stain_encoding).train()
    res = cross_stain_retrieval(st, model, ks=(1, 3))
    assert model.training                                   # restored
    assert set(res) == {"HER2", "ER", "mean"}
    assert res["ER"] == {"n": 1, "cases": [ONLY_ER]}        # one case: reported, no metrics
    cases = [c for c in range(N_CASES) if c not in NO_HER2]
    assert res["HER2"]["n"] == len(cases) and res["HER2"]["cases"] == cases

    # the reference: every bag embedded on its own, fp64 cosines, counts where fp64 leaves no doubt
    model.eval()
    with torch.no_grad():
        def one(bag, mi):
            x = bag.to(dev)
            if stain_encoding:
                return model.attend_packed((x, None, (x.shape[0],)), dev, stain_idx=mi)[0][0]
            return model.encode_he(x[None], dev)[0]
        E_he = torch.stack([one(bags[c][0], 0) for c in cases]).float().cpu().numpy()
        E_st = torch.stack([one(bags[c][1], 1) for c in cases]).float().cpu().numpy()
    for direction, (A, B) in (("he_to_stain", (E_he, E_st)), ("stain_to_he", (E_st, E_he))):
        lo, hi, _ = RR.bounds(RR.cosine64(A, B), RR.tol(512))
        print(direction, "ranks", (1 + lo).tolist())
        assert (lo == hi).all()
        assert res["HER2"][direction] == RR.metrics(lo, np.zeros_like(lo), ks=(1, 3))
    assert res["mean"] == {d: {k: v for k, v in res["HER2"][d].items() if k != "n"} for d in ("he_to_stain", "stain_to_he")}

    # a subset of the cases, in the order asked; a stain by name
    sub = cross_stain_retrieval(st, model, case_indices=[6, 2, 0, 7], stains=["HER2"], ks=(1,))
    assert set(sub) == {"HER2", "mean"} and sub["HER2"]["cases"] == [6, 0, 7] and sub["HER2"]["he_to_stain"]["n"] == 3
    assert not model.training

    # embed keeps its refusal; embed_modality is the way in
    if stain_encoding:
        with pytest.raises(ValueError, match="modality 0 only"):
            st.embed(model, modality=1)
        got = st.embed_modality(model, 1)["embeds"].cpu().numpy()
        assert np.abs(got - E_st).max() <= 1e-4 * np.abs(E_st).max()
    else:
        assert torch.equal(st.embed_modality(model, 1)["embeds"], st.embed(model, modality=1)["embeds"])
