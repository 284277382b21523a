"""The two-tier slide store on the GPU.  The whole correctness claim is bit equality with the resident store: the same cohort in a store
built with resident_bytes=None -- the untiered kernels -- is the reference for every dense batch, packed batch, prefetched iteration
and model output below, whatever the split, the width, the dtype and the grid of the host-tier pass."""
from types import SimpleNamespace

import pytest
import torch

from madeleine_amd import functional as MF
from madeleine_amd.store import DeviceSlideStore
from oracle import recipe

pytestmark = pytest.mark.gpu

MODS = ["HE", "HER2", "PGR"]
# one case per length: both sides of N for the with-replacement regime, of the 64-row limit of the in-wave sort and of the 64-token chunk,
# Feistel widths that are odd before rounding (257, 1025) or even (1000)
LENS = [1, 3, 5, 17, 64, 65, 257, 1000, 1025]
ABSENT = {(1, 1), (4, 2), (6, 1), (7, 0)}
CASES = list(range(len(LENS)))
WIDTHS = [512, 8, 6, 772]        # 16-byte rows; 16-byte for fp32, 16-bit stores too; element-wise; 16-byte for fp32 and element-wise for 16 bits
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
DENSE_N = [3, 16, 64, 100]
CAPS = [None, 64, 100]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _bags(D):
    g = torch.Generator().manual_seed(D)
    return [[None if (c, m) in ABSENT else torch.randn(n, D, generator=g) * 3.0 for m in range(3)] for c, n in enumerate(LENS)]


_CACHE = {}


def _reference(dev, D, dtype):
    """The resident store of the cohort and what it yields: computed once per (D, dtype), never modified."""
    key = (D, dtype)
    if key not in _CACHE:
        bags = _bags(D)
        st = DeviceSlideStore(bags, ["c%d" % c for c in CASES], MODS, dev, dtype=dtype)
        assert st.rows_host is None and st.resident_rows == st.rows.shape[0]
        dense = {N: st.sample(CASES, N, counter=7, seed=5, return_indices=True) for N in DENSE_N}
        packed = {cap: st.pack(CASES, cap, counter=7, seed=5, return_indices=True) for cap in CAPS}
        _CACHE[key] = (bags, st, dense, packed)
    return _CACHE[key]


def _splits(st):
    """The budgets of the issue, in bytes: all host; the middle of the cohort; the first 1025-row bag the last resident bag; the same
    bag the first of the host tier."""
    row_bytes = st.dim * st.rows.element_size()
    g = int(st.bag_table[8, 0])
    assert int(st.bag_lens_cpu[g]) == 1025
    off = st.off_cpu.tolist()
    return [0, off[st.n_bags // 2] * row_bytes + 1, off[g + 1] * row_bytes, off[g] * row_bytes]


def _tiered(dev, D, dtype, budget):
    bags, ref = _reference(dev, D, dtype)[:2]
    st = DeviceSlideStore(bags, ref.slide_ids, MODS, dev, dtype=dtype, resident_bytes=budget)
    assert st.rows_host is not None and st.rows_host.is_pinned() and not st.rows_host.is_cuda and st.rows.is_cuda
    assert st.nbytes("device") <= budget and st.resident_rows in ref.off_cpu.tolist() and torch.equal(st.off, ref.off)
    return st


def _same_pack(p, q):
    assert torch.equal(p.tokens, q.tokens) and torch.equal(p.row_bag, q.row_bag) and torch.equal(p.idx, q.idx)
    assert torch.equal(p.cu_seqlens, q.cu_seqlens) and p.lens == q.lens


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("D", WIDTHS)
def test_dense_batches_equal_the_resident_store(dev, D, dtype):
    _, ref, dense, _ = _reference(dev, D, dtype)
    for budget in _splits(ref):
        st = _tiered(dev, D, dtype, budget)
        for N in DENSE_N:
            feats, idx = st.sample(CASES, N, counter=7, seed=5, return_indices=True)
            assert feats.shape == (len(CASES), 3, N, D) and feats.dtype == torch.float32
            assert torch.equal(idx, dense[N][1]), (budget, N)
            assert torch.equal(feats, dense[N][0]), (budget, N)
        assert torch.equal(st.sample(CASES, 64, counter=7, seed=5), dense[64][0])          # without idx_out


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("D", WIDTHS)
def test_packed_batches_equal_the_resident_store(dev, D, dtype):
    _, ref, _, packed = _reference(dev, D, dtype)
    for budget in _splits(ref):
        st = _tiered(dev, D, dtype, budget)
        for cap in CAPS:
            _same_pack(st.pack(CASES, cap, counter=7, seed=5, return_indices=True), packed[cap])
        p = st.pack(CASES, 100, counter=7, seed=5)
        assert p.idx is None and torch.equal(p.tokens, packed[100].tokens)


def test_an_empty_host_tier_is_the_resident_store(dev):
    """A budget of the store's size or more: everything in one device tensor, on the untiered entry points; and the tiered entry points
    with T_dev == T_total (no host tier passed) give the bits of S1 / S2."""
    _, ref, dense, packed = _reference(dev, 8, torch.float32)
    st = DeviceSlideStore(_bags(8), ref.slide_ids, MODS, dev, resident_bytes=ref.nbytes())
    assert st.rows_host is None and st.resident_rows == ref.resident_rows and torch.equal(st.rows, ref.rows)
    assert torch.equal(st.sample(CASES, 16, counter=7, seed=5), dense[16][0])
    assert torch.equal(st.bag_view(8, 1), ref.bag_view(8, 1)) and len(list(st.ragged_batches(4))) == 3
    bag = ref.bag_table.reshape(-1).to(dev)
    feats, idx = MF.bag_sample_tiered(ref.rows, None, ref.off, bag, None, 100, 5, 7, return_indices=True)
    assert torch.equal(feats.view_as(dense[100][0]), dense[100][0]) and torch.equal(idx.view_as(dense[100][1]), dense[100][1])


def _host_items(st, cases, chunks_of):
    """(work items of the host-tier pass, work items of the device pass) of a batch; chunks_of(stored length, None for an absent stain)
    is the number of 64-token chunks of one output bag."""
    host = devc = 0
    for c in cases:
        for m in range(3):
            g = int(st.bag_table[c, m])
            n = chunks_of(None if g < 0 else int(st.bag_lens_cpu[g]))
            if g >= 0 and int(st.off_cpu[g]) >= st.resident_rows:
                host += n
            else:
                devc += n
    return host, devc


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("D", [512, 6])
def test_the_persistent_loop_at_toy_size(dev, D, dtype):
    """host_wgs = 3: a batch with 7 host-tier work items (more than the grid, not a multiple of it), one with 2 (fewer than the grid),
    one with none and one with no resident item; then larger batches, where every workgroup walks many items."""
    _, ref, dense, packed = _reference(dev, D, dtype)
    off = ref.off_cpu.tolist()
    split = off[int(ref.bag_table[5, 0])]                        # cases 0..4 resident, cases 5..8 in the host tier
    st = _tiered(dev, D, dtype, split * D * ref.rows.element_size())
    assert st.resident_rows == split
    dense_chunks = lambda n: 1                                   # noqa: E731  (N = 64: one chunk per output row)
    pack_chunks = lambda n: 1 if n is None else (min(n, 64) + 63) // 64      # noqa: E731  (max_tokens = 64)
    for cases, want in (([5, 6, 7], (7, 2)), ([7], (2, 1)), ([0, 1, 2], (0, 9)), ([8, 5], (6, 0))):
        assert _host_items(st, cases, dense_chunks) == want and _host_items(st, cases, pack_chunks) == want
        f, i = st.sample(cases, 64, counter=7, seed=5, return_indices=True, host_wgs=3)
        assert torch.equal(f, dense[64][0][cases]) and torch.equal(i, dense[64][1][cases]), cases
        _same_pack(st.pack(cases, 64, counter=7, seed=5, return_indices=True, host_wgs=3),
                   ref.pack(cases, 64, counter=7, seed=5, return_indices=True))
    for wgs in (1, 3, 1000):                                     # 1000: more workgroups than items, the grid is cut to the items
        f, i = st.sample(CASES, 100, counter=7, seed=5, return_indices=True, host_wgs=wgs)
        assert torch.equal(f, dense[100][0]) and torch.equal(i, dense[100][1]), wgs
        _same_pack(st.pack(CASES, None, counter=7, seed=5, return_indices=True, host_wgs=wgs), packed[None])


def test_a_bag_index_outside_the_store_is_an_absent_stain(dev):
    """The table-level inconsistency the store tests already use: a `bag` outside [0, n_bags) comes out as zeros / -1, in both passes'
    launches, next to valid bags of both tiers."""
    _, ref, _, _ = _reference(dev, 8, torch.float32)
    st = _tiered(dev, 8, torch.float32, _splits(ref)[1])
    bag = torch.tensor([0, st.n_bags, st.n_bags - 1, -7, 1 << 20], dtype=torch.int32, device=dev)
    for N in (3, 100):
        f, i = MF.bag_sample_tiered(st.rows, st.rows_host, st.off, bag, None, N, 5, 7, return_indices=True, host_wgs=3)
        g, j = MF.bag_sample(ref.rows, ref.off, bag, None, N, 5, 7, return_indices=True)
        assert torch.equal(f, g) and torch.equal(i, j)
        assert not bool(f[[1, 3, 4]].any()) and bool((i[[1, 3, 4]] == -1).all()) and bool((i[[0, 2]] >= 0).all())


def test_an_unpinned_host_tier_is_refused_in_python(dev, monkeypatch):
    _, ref, _, _ = _reference(dev, 8, torch.float32)
    st = _tiered(dev, 8, torch.float32, 0)
    bag = ref.bag_table.reshape(-1).to(dev)
    monkeypatch.setattr(MF, "_call", lambda *a, **k: pytest.fail("the native layer was reached"))
    pageable = st.rows_host.clone()
    assert not pageable.is_pinned()
    with pytest.raises(RuntimeError, match="pinned"):
        MF.bag_sample_tiered(st.rows, pageable, st.off, bag, None, 4, 0, 0)
    with pytest.raises(RuntimeError, match="pinned"):
        MF.bag_pack_tiered(st.rows, pageable, st.off, bag, None, st.off, st.off, 4, 2, 0, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MF.bag_sample(st.rows_host, st.off, bag, None, 4, 0, 0)


def _consume(loader, epochs, key):
    """Every batch of `epochs` epochs, used on the current stream the moment it is yielded: (tensors, sums taken at yield)."""
    seen, sums = [], []
    for e in epochs:
        loader.set_epoch(e)
        for out in loader:
            t = out[key] if key == "feats" else out[key].tokens
            sums.append(t.double().sum() + t[-1].double().sum())                 # no host synchronisation in between
            seen.append(out)
    return seen, sums


def _same_batches(a, b, key):
    assert len(a[0]) == len(b[0]) > 0
    torch.cuda.synchronize()
    for x, y, sx, sy in zip(a[0], b[0], a[1], b[1]):
        assert x["slide_ids"] == y["slide_ids"] and torch.equal(x["modality_labels"], y["modality_labels"])
        if key == "feats":
            assert torch.equal(x["feats"], y["feats"])
        else:
            p, q = x["packed"], y["packed"]
            assert torch.equal(p.tokens, q.tokens) and torch.equal(p.row_bag, q.row_bag) and torch.equal(p.cu_seqlens, q.cu_seqlens)
            assert p.lens == q.lens and p.idx is None and q.idx is None
        assert float(sx) == float(sy)                            # what the consumer read at yield is what the reference read


@pytest.mark.parametrize("budget_no", [0, 1], ids=["all_host", "mixed"])
def test_prefetched_iteration_equals_the_resident_store(dev, budget_no):
    _, ref, _, _ = _reference(dev, 512, torch.float32)
    st = _tiered(dev, 512, torch.float32, _splits(ref)[budget_no])
    makers = {"feats": lambda s, k: s.batches(4, 64, shuffle=True, seed=1, prefetch=k),
              "packed": lambda s, k: s.packed_batches(4, max_tokens=100, shuffle=True, seed=1, prefetch=k)}
    sides = []
    for key, make in makers.items():
        want = _consume(make(ref, 0), (0, 1), key)
        assert len(want[0]) == 6
        loader = make(st, 2)
        _same_batches(_consume(loader, (0, 1), key), want, key)
        _same_batches(_consume(make(st, None), (0, 1), key), want, key)            # the default with a host tier: prefetch = 1
        _same_batches(_consume(make(st, 0), (0, 1), key), want, key)
        _same_batches(_consume(make(ref, 2), (0, 1), key), want, key)              # a resident store may prefetch too
        # an iterator dropped after its first batch: its queued gathers finish into tensors nobody reads, a fresh one starts over
        loader.set_epoch(1)
        first = next(iter(loader))
        again = _consume(loader, (1,), key)
        _same_batches(again, (want[0][3:], want[1][3:]), key)
        t = first[key] if key == "feats" else first[key].tokens
        assert torch.equal(t, again[0][0][key] if key == "feats" else again[0][0][key].tokens)
        sides.append(st._side)
    assert sides[0] is not None and sides[0] is sides[1] is st._side_stream()      # one side stream per store, not one per epoch or iterator


def test_prefetch_does_not_synchronise_the_host(dev):
    _, ref, _, _ = _reference(dev, 8, torch.float32)
    st = _tiered(dev, 8, torch.float32, 0)
    list(st.batches(4, 64, prefetch=1))                          # warm-up: library load, allocator, pinned staging, the side stream
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        n = sum(1 for _ in st.batches(4, 64, prefetch=2)) + sum(1 for _ in st.packed_batches(4, max_tokens=64, prefetch=1))
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert n == 6


# ------------------------------------------------------------------------------------------------ the model on a host-tier batch
SMOKE_D = 64
SMOKE_LENS = [[300, 256, 310], [260, None, 333], [290, 301, 257], [None, 280, 270]]


def test_model_outputs_equal_those_from_the_resident_store(dev):
    from madeleine_amd import MADELEINE
    bags = [[None if n is None else torch.from_numpy(recipe.uniform((n, SMOKE_D), "tier:%d:%d" % (c, m))) for m, n in enumerate(case)]
            for c, case in enumerate(SMOKE_LENS)]
    ids = ["case%d" % c for c in range(4)]
    ref = DeviceSlideStore(bags, ids, MODS, dev)
    st = DeviceSlideStore(bags, ids, MODS, dev, resident_bytes=0)
    assert st.resident_rows == 0 and st.nbytes("device") == 0 and st.nbytes("host") == ref.nbytes()
    cfg = SimpleNamespace(MODALITIES=MODS, wsi_encoder="abmil", patch_embedding_dim=SMOKE_D, wsi_encoder_hidden_dim=512, activation="softmax",
                          n_heads=4)
    model = MADELEINE(cfg)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.state_dict_recipe(shapes, "tier").items()}, strict=True)
    model = model.to(dev).eval()
    cases, labels = [0, 1, 2, 3], ref.modality_labels
    for make in (lambda s: {"feats": s.sample(cases, 64, counter=3, seed=2), "modality_labels": labels},
                 lambda s: {"packed": s.pack(cases, None, counter=3, seed=2), "modality_labels": labels}):
        with torch.no_grad():
            got, want = model(make(st), device=dev), model(make(ref), device=dev)
        for k in MODS:
            assert torch.isfinite(want[0][k]).all() and torch.equal(got[0][k], want[0][k]) and torch.equal(got[1][k], want[1][k]), k
