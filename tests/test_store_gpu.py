"""The device-resident slide store on the GPU: mdl_bag_sample's gather against index_select on its own exported indices, the validity,
determinism and batch-independence of its draws, their statistics against chi-square bounds, and the store feeding MADELEINE and
train_loop end to end."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from torch import nn

from madeleine_amd import functional as MF
from madeleine_amd.store import DeviceSlideStore
from oracle import recipe

pytestmark = pytest.mark.gpu

# bag lengths around every threshold of the kernel: 1, 2, N - 1 / N / N + 1 for N = 3, 64, 256, both sides of the 64-row limit of the
# in-wave sort, of the 64-token chunk, and lengths whose Feistel width is odd before rounding (257, 4097) or even (1000)
LENS = [1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 1000, 4097]
TOKENS = [1, 3, 64, 256]
DTYPES = [torch.float32, torch.float16, torch.bfloat16]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _rows(T, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(T, D, generator=g) * 3.0


def _tables(lens, dev, absent_at=(2, 9)):
    """off, bag (every bag once, -1 spliced in at `absent_at`), key_id for a store of bags of `lens` rows."""
    off = torch.zeros(len(lens) + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.tensor(lens), 0)
    bag = list(range(len(lens)))
    for pos in absent_at:
        bag.insert(pos, -1)
    bag = torch.tensor(bag, dtype=torch.int32)
    return off.to(dev), bag.to(dev), torch.arange(100, 100 + bag.numel(), dtype=torch.int64, device=dev)


def _check_gather(store, off, bag, out, idx):
    present = bag >= 0
    assert bool((idx[~present] == -1).all()) and not bool(out[~present].any())
    src = (off[bag[present].long()].unsqueeze(1) + idx[present].long()).reshape(-1)
    want = store.index_select(0, src).float().view(int(present.sum()), idx.shape[1], store.shape[1])
    assert torch.equal(out[present], want)


def _check_draw(idx, lens, bag, N):
    for r, g in enumerate(bag.tolist()):
        if g < 0:
            continue
        n, row = lens[g], idx[r].tolist()
        assert min(row) >= 0 and max(row) < n, (n, N)
        if n >= N:
            assert len(set(row)) == N, (n, N)               # pairwise distinct
        if n == N:
            assert sorted(row) == list(range(n)), (n, N)    # a permutation of the bag
        if n == 1:
            assert not any(row)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("D", [4, 32, 33, 512])
def test_gather_is_exact_and_draws_are_valid(dev, D, dtype):
    """out[r, t] == store[off[bag] + idx[r, t]] bit for bit (16-bit stores: the upcast of the stored value), absent rows zero with
    idx -1, indices in range, distinct where the bag is long enough, a permutation at n == N, and the store untouched."""
    store = _rows(sum(LENS), D, D).to(dev).to(dtype)
    before = store.clone()
    off, bag, key = _tables(LENS, dev)
    for N in TOKENS:
        out, idx = MF.bag_sample(store, off, bag, key, N, seed=11, counter=N, return_indices=True)
        assert out.shape == (bag.numel(), N, D) and out.dtype == torch.float32 and idx.shape == (bag.numel(), N) and idx.dtype == torch.int32
        _check_gather(store, off, bag, out, idx)
        _check_draw(idx.cpu(), LENS, bag.cpu(), N)
    assert torch.equal(store, before)


@pytest.mark.parametrize("width,D", [(36, 32), (33, 32), (40, 33), (16, 8)])
def test_gather_from_a_strided_store(dev, width, D):
    """A store whose rows are `width` elements apart: 16-byte accesses when D and the stride allow them, element-wise ones otherwise."""
    for dtype in DTYPES:
        base = _rows(sum(LENS), width, width).to(dev).to(dtype)
        store = base[:, :D]
        off, bag, key = _tables(LENS, dev)
        out, idx = MF.bag_sample(store, off, bag, key, 70, seed=5, counter=1, return_indices=True)
        _check_gather(store, off, bag, out, idx)


def test_every_output_element_is_written_and_tables_are_bounded(dev):
    """A NaN-prefilled out / idx_out comes back fully overwritten (tail chunks, absent rows, both access widths), and a bag table that
    points outside the store reads nothing: such rows are written as absent stains."""
    for D in (33, 64):
        store = _rows(sum(LENS), D, 7).to(dev)
        off, bag, key = _tables(LENS, dev)
        bag = torch.cat([bag, torch.tensor([len(LENS), 1 << 20, -7], dtype=torch.int32, device=dev)])      # no such bags
        key = torch.arange(bag.numel(), dtype=torch.int64, device=dev)
        R, N = bag.numel(), 70
        out = torch.full((R, N, D), float("nan"), device=dev)
        idx = torch.full((R, N), -99, dtype=torch.int32, device=dev)
        MF._call("mdl_bag_sample", store, 0, D, store.shape[0], off, len(LENS), bag, key, R, N, D, 3, 4, out, idx, MF._stream())
        assert not bool(torch.isnan(out).any()) and not bool((idx == -99).any())
        assert not bool(out[-3:].any()) and bool((idx[-3:] == -1).all())
        _check_gather(store, off, torch.where(bag < len(LENS), bag, torch.full_like(bag, -1)), out, idx)
        # an offset table that leaves the store (T_total understated): the bags past it are absent, the others unchanged
        short = int(off[-2])
        out2 = torch.full((R, N, D), float("nan"), device=dev)
        MF._call("mdl_bag_sample", store, 0, D, short, off, len(LENS), bag, key, R, N, D, 3, 4, out2, None, MF._stream())
        last = int((bag == len(LENS) - 1).nonzero()[0])
        assert not bool(out2[last].any())
        keep = torch.ones(R, dtype=torch.bool, device=dev)
        keep[last] = False
        assert torch.equal(out2[keep], out[keep])


def _toy_store(dev, dtype=torch.float32, D=32, seed=0):
    g = torch.Generator().manual_seed(seed)
    lens = [[300, None, 40], [5, 700, 64], [1, 2, None], [65, 100, 257], [90, None, None], [128, 33, 500]]
    bags = [[None if n is None else torch.randn(n, D, generator=g) for n in case] for case in lens]
    return DeviceSlideStore(bags, ["c%d" % i for i in range(len(bags))], ["HE", "HER2", "PGR"], dev, dtype=dtype), bags


def test_draws_are_deterministic_and_independent_of_the_batch(dev):
    st, bags = _toy_store(dev)
    assert st.rows.is_cuda and st.off.is_cuda and torch.equal(st.bag_view(1, 1).cpu(), bags[1][1])        # the upload is exact
    cases = [0, 1, 2, 3, 4, 5]
    a, ia = st.sample(cases, 64, counter=9, return_indices=True)
    b, ib = st.sample(cases, 64, counter=9, return_indices=True)
    assert a.shape == (6, 3, 64, 32) and ia.shape == (6, 3, 64) and torch.equal(a, b) and torch.equal(ia, ib)
    c, ic = st.sample(cases, 64, counter=10, return_indices=True)
    d, id_ = st.sample(cases, 64, counter=9, seed=18, return_indices=True)
    e, ie = st.sample(cases, 64, counter=9, seed=0, return_indices=True)        # the default seed, passed explicitly
    assert torch.equal(ie, ia) and torch.equal(e, a)
    for case, m in ((0, 0), (1, 1), (5, 2)):     # bags of 300, 700, 500 rows: another counter / seed moves nearly every position
        assert float((ic[case, m] != ia[case, m]).float().mean()) > 0.9 and float((id_[case, m] != ia[case, m]).float().mean()) > 0.9
    assert not torch.equal(c, a) and not torch.equal(d, a)
    # absent stains: zeros, idx -1
    assert not bool(a[0, 1].any()) and bool((ia[0, 1] == -1).all()) and not bool(a[4, 1:].any())
    # a case draws the same rows whatever its batch mates and its position in the batch
    pair, ipair = st.sample([3, 5], 64, counter=9, return_indices=True)
    solo, isolo = st.sample([5], 64, counter=9, return_indices=True)
    assert torch.equal(pair[1], solo[0]) and torch.equal(ipair[1], isolo[0]) and torch.equal(solo[0], a[5]) and torch.equal(pair[0], a[3])
    swapped = st.sample([5, 3, 5], 64, counter=9)
    assert torch.equal(swapped[0], a[5]) and torch.equal(swapped[1], a[3]) and torch.equal(swapped[2], a[5])
    with pytest.raises(IndexError):
        st.sample([6], 64, counter=0)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_lossy_store_samples_the_rounded_features(dev, dtype):
    st, bags = _toy_store(dev, dtype=dtype)
    out, idx = st.sample([1, 3], 48, counter=2, return_indices=True)
    for b, case in enumerate((1, 3)):
        for m in range(3):
            want = bags[case][m].to(dtype).float().to(dev).index_select(0, idx[b, m].long())
            assert torch.equal(out[b, m], want)


def test_sample_does_not_synchronise_the_host(dev):
    st, _ = _toy_store(dev)
    st.sample([0, 1], 64, counter=0)                      # warm-up: library load, allocator, pinned staging
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = st.sample([2, 3, 4], 64, counter=1)
        out2, idx = st.sample([5], 16, counter=2, return_indices=True)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert out.shape == (3, 3, 64, 32) and out2.shape == (1, 3, 16, 32) and idx.shape == (1, 3, 16)


# ------------------------------------------------------------------------------------------------ statistics
def _bound(df):
    """Upper 1e-6 quantile of chi-square(df) in the Wilson-Hilferty form: a derived bound -- a correct sampler exceeds it once in a
    million statistics, whatever its seed."""
    return df * (1 - 2 / (9 * df) + 4.75 * math.sqrt(2 / (9 * df))) ** 3


def _chi2_uniform(values, cells):
    c = torch.bincount(values.reshape(-1), minlength=cells).double()
    assert c.numel() == cells
    e = c.sum() / cells
    return float(((c - e) ** 2 / e).sum())


def _draw_one_bag(dev, n, N, K):
    """K output rows in one launch, all over one bag of n rows, key_id = arange(K), D = 4 -> idx [K, N] int64."""
    store = torch.arange(n, dtype=torch.float32, device=dev).unsqueeze(1).repeat(1, 4)
    off = torch.tensor([0, n], dtype=torch.int64, device=dev)
    bag = torch.zeros(K, dtype=torch.int32, device=dev)
    out, idx = MF.bag_sample(store, off, bag, torch.arange(K, dtype=torch.int64, device=dev), N, seed=1234, counter=7, return_indices=True)
    assert torch.equal(out[:, :, 0], idx.float()) and torch.equal(out[:, :, 3], idx.float())       # the row that was drawn is the row copied
    idx = idx.long()
    assert int(idx.min()) >= 0 and int(idx.max()) < n
    return idx


@pytest.mark.parametrize("n,N,K", [(5, 3, 200000), (17, 16, 200000), (64, 33, 200000), (65, 64, 20000), (257, 256, 20000),
                                   (1000, 256, 20000), (1025, 64, 40000)])
def test_statistics_without_replacement(dev, n, N, K):
    """Three chi-square statistics of K draws of N out of n, each against the 1e-6 quantile of its distribution under a uniformly
    random ordered N-subset:
      (a) inclusion counts c_i of the n source rows: sum (c_i - K q)^2 / (K q (1 - q)) * (n - 1) / n, q = N / n, df n - 1 (the factor
          (n - 1) / n accounts for the counts of one draw summing to N exactly);
      (b) the row at position 0, uniform over n cells, df n - 1;
      (c) (idx[1] - idx[0]) mod n, uniform over 1 .. n - 1, df n - 2.
    A Feistel network used on a 5-row bag gives 87 and 364 against the bound 35.2 here; four rounds at n = 17 give 72 against 59."""
    idx = _draw_one_bag(dev, n, N, K)
    assert int((idx.sort(dim=1).values.diff(dim=1) == 0).sum()) == 0          # distinct inside every draw
    stats = {}
    if N < n:
        q = N / n
        c = torch.bincount(idx.reshape(-1), minlength=n).double()
        stats["inclusion"] = (float(((c - K * q) ** 2).sum()) / (K * q * (1 - q)) * (n - 1) / n, n - 1)
    stats["position 0"] = (_chi2_uniform(idx[:, 0], n), n - 1)
    stats["difference"] = (_chi2_uniform((idx[:, 1] - idx[:, 0]) % n - 1, n - 1), n - 2)
    for name, (x, df) in stats.items():
        print("n=%d N=%d K=%d %s: %.1f (df %d, bound %.1f)" % (n, N, K, name, x, df, _bound(df)))
    for name, (x, df) in stats.items():
        assert x <= _bound(df), (name, x, df, _bound(df))


def test_statistics_with_replacement(dev):
    """n = 3 < N = 64: single values uniform over 3 cells (df 2), and adjacent pairs (positions 2j, 2j + 1: disjoint pairs, so the
    cells are independent and the statistic is a plain chi-square) uniform over 9 cells (df 8)."""
    n, N, K = 3, 64, 200000
    idx = _draw_one_bag(dev, n, N, K)
    single = _chi2_uniform(idx, n)
    pairs = _chi2_uniform(idx[:, 0::2] * n + idx[:, 1::2], n * n)
    print("with replacement n=3 N=64 K=200000: single %.1f (df 2, bound %.1f), pairs %.1f (df 8, bound %.1f)"
          % (single, _bound(2), pairs, _bound(8)))
    assert single <= _bound(2) and pairs <= _bound(8)


# ------------------------------------------------------------------------------------------------ end to end
E2E_MODS = ["HE", "HER2", "PGR"]
E2E_D = 512
E2E_LENS = [[300, 450, 700], [512, None, 333], [700, 301, 400], [650, 390, 310], [345, 600, 512], [480, 575, 699], [300, 640, None],
            [555, 444, 333]]


@pytest.fixture(scope="module")
def e2e_store(dev):
    bags = [[None if n is None else torch.from_numpy(recipe.uniform((n, E2E_D), "store:%d:%d" % (c, m))) for m, n in enumerate(case)]
            for c, case in enumerate(E2E_LENS)]
    return DeviceSlideStore(bags, ["case%d" % c for c in range(len(bags))], E2E_MODS, dev)


def _model(dev, tag="store", **extra):
    from madeleine_amd import MADELEINE
    cfg = SimpleNamespace(MODALITIES=E2E_MODS, wsi_encoder="abmil", patch_embedding_dim=E2E_D, wsi_encoder_hidden_dim=512,
                          activation="softmax", n_heads=4, **extra)
    m = MADELEINE(cfg)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.state_dict_recipe(shapes, tag).items()}, strict=True)
    return m.to(dev)


def test_batches_are_collate_shaped(dev, e2e_store):
    from madeleine_amd.data import SyntheticSlideDataset, collate
    ds = SyntheticSlideDataset(4, E2E_MODS, 8, 16)
    want = collate([ds[i] for i in range(4)])
    it = e2e_store.batches(4, 256, seed=2)
    assert len(it) == 2
    seen = []
    for _ in range(2):                                                   # re-iterable
        got = list(it)
        assert len(got) == 2
        for data in got:
            assert set(data) == set(want)
            f, lab, ids = data["feats"], data["modality_labels"], data["slide_ids"]
            assert f.shape == (4, 3, 256, E2E_D) and f.dtype == want["feats"].dtype and f.device == dev
            assert lab.shape == (4, 3) and lab.dtype == want["modality_labels"].dtype and lab.device.type == "cpu"
            assert type(ids) is type(want["slide_ids"]) and len(ids) == 4 and all(isinstance(s, str) for s in ids)
            for b, sid in enumerate(ids):
                c = int(sid[4:])
                assert lab[b].tolist() == [0.0 if n is None else 1.0 for n in E2E_LENS[c]]
                assert all(bool(f[b, m].any()) == (n is not None) for m, n in enumerate(E2E_LENS[c]))
        seen.append(got)
    assert sorted(s for d in seen[0] for s in d["slide_ids"]) == sorted(e2e_store.slide_ids)
    assert all(torch.equal(x["feats"], y["feats"]) and x["slide_ids"] == y["slide_ids"] for x, y in zip(*seen))   # same epoch: same batches
    it.set_epoch(1)
    again = list(it)
    assert [d["slide_ids"] for d in again] != [d["slide_ids"] for d in seen[0]]
    # a resumed run: a fresh iterable set to epoch 1 redraws the same batches
    resumed = e2e_store.batches(4, 256, seed=2)
    resumed.set_epoch(1)
    assert all(torch.equal(x["feats"], y["feats"]) and x["slide_ids"] == y["slide_ids"] for x, y in zip(again, resumed))


@pytest.mark.parametrize("skip_absent", [False, True])
def test_model_on_a_store_batch_equals_model_on_the_rebuilt_batch(dev, e2e_store, skip_absent):
    st = e2e_store
    model = _model(dev, skip_absent_stains=skip_absent).eval()
    cases = [1, 4, 6, 2]
    feats, idx = st.sample(cases, 256, counter=3, return_indices=True)
    rebuilt = torch.zeros_like(feats)
    for b, c in enumerate(cases):
        for m in range(3):
            view = st.bag_view(c, m)
            if view is not None:
                rebuilt[b, m] = view.index_select(0, idx[b, m].long())
    assert torch.equal(feats, rebuilt)
    labels = st.modality_labels[cases]
    with torch.no_grad():
        e0, t0 = model({"feats": feats, "modality_labels": labels}, device=dev)
        e1, t1 = model({"feats": rebuilt, "modality_labels": labels}, device=dev)
    for k in E2E_MODS:
        assert torch.isfinite(e0[k]).all() and torch.equal(e0[k], e1[k]) and torch.equal(t0[k], t1[k])


def test_train_loop_epoch_over_the_store(dev, e2e_store):
    from madeleine_amd import GOT, InfoNCE, train_loop
    model = _model(dev)
    for mod in model.modules():
        if isinstance(mod, nn.Dropout):
            mod.p = 0.0
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: 1.0)
    args = SimpleNamespace(precision="float32", warmup_epochs=0, STAINS=E2E_MODS[1:], global_loss="info-nce", symmetric_cl=True,
                           local_loss_weight=0.5)
    np.random.seed(3)
    torch.manual_seed(3)
    loader = e2e_store.batches(4, 256, seed=1)
    loss, rank = train_loop(args, InfoNCE(temperature=0.1), GOT, InfoNCE(temperature=0.1), model, 1, loader, opt, sched, sched)
    assert np.isfinite(loss) and loss > 0 and np.isfinite(rank)
    after = dict(model.named_parameters())
    assert all(torch.isfinite(v).all() for v in after.values())
    assert sum(not torch.equal(before[k], after[k].detach()) for k in before) > len(before) // 2


def test_ragged_batches_feed_forward_ragged_with_views_of_the_store(dev, e2e_store):
    st = e2e_store
    model = _model(dev).eval()
    lo, hi = st.rows.data_ptr(), st.rows.data_ptr() + st.nbytes()
    batches = list(st.ragged_batches(4, shuffle=False))
    assert len(batches) == 2
    for data in batches:
        assert set(data) == {"bags", "modality_labels", "slide_ids"}
        for b, sid in enumerate(data["slide_ids"]):
            c = int(sid[4:])
            for m, n in enumerate(E2E_LENS[c]):
                bag = data["bags"][b][m]
                if n is None:
                    assert bag.shape == (2, E2E_D) and not bool(bag.any()) and bag.device == dev
                else:
                    assert bag.shape == (n, E2E_D) and lo <= bag.data_ptr() < hi and bag.data_ptr() == st.bag_view(c, m).data_ptr()
        with torch.no_grad():
            embs, toks = model(data, device=dev, n_views=1)
        for k in E2E_MODS:
            assert embs[k].shape[0] == 4 and torch.isfinite(embs[k]).all() and torch.isfinite(toks[k]).all()
