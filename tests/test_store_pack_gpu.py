"""The packed ragged route of the slide store on the GPU: mdl_bag_pack against the bag views and index_select on its own exported
indices, its draw against mdl_bag_sample's, what it writes with inconsistent tables, and packed batches feeding MADELEINE and train_loop
end to end against the 'bags' route."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from torch import nn

from madeleine_amd import functional as MF
from madeleine_amd.store import DeviceSlideStore, PackedBags
from oracle import recipe

pytestmark = pytest.mark.gpu

# the store tests' lengths: 1, 2, c - 1 / c / c + 1 for the caps 3, 64, 256, both sides of the 64-row limit of the in-wave sort and of the
# 64-row chunk, Feistel widths that are odd before rounding (257, 4097) or even (1000); more than one chunk per bag from 65 rows on
LENS = [1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 1000, 4097]
CAPS = [None, 1, 3, 64, 256]
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
ABSENT_ROWS = 2


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


def _out_lens(bag, lens, cap):
    return [ABSENT_ROWS if g < 0 else (lens[g] if cap is None else min(lens[g], cap)) for g in bag.tolist()]


def _cu(out_lens, dev):
    """cu, chunk_cu on the device and their totals (T_out, n_chunks) for packed bags of `out_lens` rows."""
    L = torch.tensor(out_lens, dtype=torch.int64)
    cu, ch = torch.zeros(L.numel() + 1, dtype=torch.int64), torch.zeros(L.numel() + 1, dtype=torch.int64)
    cu[1:], ch[1:] = torch.cumsum(L, 0), torch.cumsum((L + 63) // 64, 0)
    return cu.to(dev), ch.to(dev), int(cu[-1]), int(ch[-1])


def _check_pack(store, off, bag, lens, out_lens, tok, row_bag, idx):
    """Every property of one packed batch: the bag map, zeros / whole bags / distinct in-range draws per bag, and every row bit-equal
    to the (upcast) stored row its idx names."""
    dev, R = store.device, bag.numel()
    assert tok.dtype == torch.float32 and tok.shape == (sum(out_lens), store.shape[1]) and row_bag.dtype == idx.dtype == torch.int32
    assert torch.equal(row_bag.long(), torch.repeat_interleave(torch.arange(R, device=dev), torch.tensor(out_lens, device=dev)))
    idx_c, start = idx.cpu(), 0
    for r, (g, L) in enumerate(zip(bag.tolist(), out_lens)):
        row = idx_c[start:start + L].tolist()
        if g < 0:
            assert row == [-1] * L, r
        elif L == lens[g]:
            assert row == list(range(L)), (r, L)                 # the bag taken whole, in stored order
        else:
            assert L < lens[g] and min(row) >= 0 and max(row) < lens[g] and len(set(row)) == L, (r, L, lens[g])
        start += L
    present = idx >= 0
    src = off[bag.long().clamp(min=0)][row_bag.long()] + idx.long()
    want = store.index_select(0, src.clamp(min=0)).float() * present.unsqueeze(1)
    assert torch.equal(tok, want)
    assert not bool(tok[~present].any())


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("D", [4, 32, 33, 512])
def test_pack_is_exact(dev, D, dtype):
    """tokens[cu[r]:cu[r + 1]] is the upcast bag view where the bag fits, L distinct in-range rows of it (bit-equal to store[off + idx])
    where it is cut, zeros with idx -1 for an absent stain; row_bag is the bag of every row; the store is untouched."""
    store = _rows(sum(LENS), D, D).to(dev).to(dtype)
    before = store.clone()
    off, bag, key = _tables(LENS, dev)
    for cap in CAPS:
        out_lens = _out_lens(bag, LENS, cap)
        cu, ch, T, n_chunks = _cu(out_lens, dev)
        tok, row_bag, idx = MF.bag_pack(store, off, bag, key, cu, ch, T, n_chunks, seed=11, counter=cap or 0, return_indices=True)
        _check_pack(store, off, bag, LENS, out_lens, tok, row_bag, idx)
        if cap is None:                                          # L == n everywhere: each bag equals its view
            for r, g in enumerate(bag.tolist()):
                if g >= 0:
                    assert torch.equal(tok[int(cu[r]):int(cu[r + 1])], store[int(off[g]):int(off[g + 1])].float())
        tok2, row_bag2 = MF.bag_pack(store, off, bag, key, cu, ch, T, n_chunks, seed=11, counter=cap or 0)      # without idx_out
        assert torch.equal(tok2, tok) and torch.equal(row_bag2, row_bag)
    assert torch.equal(store, before)


@pytest.mark.parametrize("width,D", [(40, 32), (36, 32), (33, 32), (40, 33)])
def test_pack_from_a_strided_store(dev, width, D):
    """A store whose rows are `width` elements apart: 16-byte accesses when D and the stride allow them ((40, 32) for every dtype,
    (36, 32) for fp32 alone), element-wise ones otherwise."""
    for dtype in DTYPES:
        store = _rows(sum(LENS), width, width).to(dev).to(dtype)[:, :D]
        off, bag, key = _tables(LENS, dev)
        for cap in (None, 70):
            out_lens = _out_lens(bag, LENS, cap)
            cu, ch, T, n_chunks = _cu(out_lens, dev)
            tok, row_bag, idx = MF.bag_pack(store, off, bag, key, cu, ch, T, n_chunks, seed=5, counter=1, return_indices=True)
            _check_pack(store, off, bag, LENS, out_lens, tok, row_bag, idx)


def _lens_store(dev, dtype=torch.float32, D=32):
    """A DeviceSlideStore over LENS: 5 cases x 3 stains, three of the 15 bags absent."""
    g = torch.Generator().manual_seed(1)
    lens = [[1, 2, None], [3, 4, 63], [64, None, 65], [255, 256, 257], [None, 1000, 4097]]
    bags = [[None if n is None else torch.randn(n, D, generator=g) for n in case] for case in lens]
    return DeviceSlideStore(bags, ["c%d" % i for i in range(len(bags))], ["HE", "HER2", "PGR"], dev, dtype=dtype), lens


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_pack_draws_what_the_dense_sampler_draws(dev, dtype):
    """A bag longer than the cap c is cut to the rows, in the order, that store.sample(cases, c) draws for it under the same counter
    and seed -- in-wave sort (n <= 64) and Feistel walk alike -- and a bag that fits is its view."""
    st, lens = _lens_store(dev, dtype)
    cases = [0, 1, 2, 3, 4]
    flat = [n for case in lens for n in case]
    cut = 0
    for c in (1, 3, 64, 256):
        p = st.pack(cases, c, counter=7, seed=5, return_indices=True)
        assert isinstance(p, PackedBags) and list(p.lens) == st.pack_lens(cases, c) and p.cu_seqlens.dtype == torch.int64
        assert p.cu_seqlens.device == dev and p.cu_seqlens.tolist() == np.cumsum([0] + list(p.lens)).tolist()
        feats, idx = st.sample(cases, c, counter=7, seed=5, return_indices=True)
        feats, idx, cu = feats.view(len(flat), c, -1), idx.view(len(flat), c), p.cu_seqlens.tolist()
        for r, n in enumerate(flat):
            got, gi = p.tokens[cu[r]:cu[r + 1]], p.idx[cu[r]:cu[r + 1]]
            if n is None:
                assert got.shape[0] == ABSENT_ROWS and not bool(got.any()) and bool((gi == -1).all())
            elif n > c:
                assert torch.equal(got, feats[r]) and torch.equal(gi, idx[r]), (n, c)
                cut += 1
            else:
                assert torch.equal(got, st.bag_view(r // 3, r % 3).float()) and gi.tolist() == list(range(n)), (n, c)
    assert cut == 11 + 9 + 6 + 3
    # another counter or seed moves the draw (bags of 1000 and 4097 rows at c = 256: nearly every position changes)
    a = st.pack([4], 256, counter=7, seed=5, return_indices=True)
    for other in (st.pack([4], 256, counter=8, seed=5, return_indices=True), st.pack([4], 256, counter=7, seed=6, return_indices=True)):
        assert float((other.idx[ABSENT_ROWS:] != a.idx[ABSENT_ROWS:]).float().mean()) > 0.9 and not torch.equal(other.tokens, a.tokens)
    again = st.pack([4], 256, counter=7, seed=5, return_indices=True)
    assert torch.equal(again.tokens, a.tokens) and torch.equal(again.idx, a.idx)
    # a case packs the same rows whatever its batch mates and its position in the batch
    p = st.pack([3, 4, 1], 64, counter=2, return_indices=True)
    cu = p.cu_seqlens.tolist()
    for pos, case in enumerate((3, 4, 1)):
        solo = st.pack([case], 64, counter=2, seed=0, return_indices=True)       # seed None is seed 0
        assert torch.equal(p.tokens[cu[3 * pos]:cu[3 * pos + 3]], solo.tokens) and torch.equal(p.idx[cu[3 * pos]:cu[3 * pos + 3]], solo.idx)
        assert torch.equal(p.row_bag[cu[3 * pos]:cu[3 * pos + 3]] - 3 * pos, solo.row_bag)
    assert st.pack([0, 1], 5).idx is None
    with pytest.raises(IndexError):
        st.pack([5])
    with pytest.raises(ValueError, match="max_tokens"):
        st.pack([0], max_tokens=0)


def test_every_row_below_T_out_is_written_and_none_beyond(dev):
    """Sentinel-prefilled out / row_bag / idx_out longer than T_out: rows < T_out are all overwritten (tail chunks, absent stains, both
    access widths), rows >= T_out keep the sentinel.  A bag table pointing outside the store yields zero rows; an understated T_total
    turns only the bags it cuts off into zeros; a bag asked for more rows than it has is zero past its end; an understated T_out
    clips the writes and changes nothing below it."""
    SLACK = 130
    for D in (33, 64):
        store = _rows(sum(LENS), D, 7).to(dev)
        off, bag, key = _tables(LENS, dev)
        bag = torch.cat([bag, torch.tensor([len(LENS), 1 << 20, -7], dtype=torch.int32, device=dev)])      # no such bags
        key = torch.arange(bag.numel(), dtype=torch.int64, device=dev)
        R = bag.numel()
        out_lens = _out_lens(bag[:-3], LENS, 70) + [5, 70, 3]
        over = int((bag == 3).nonzero()[0])                      # the 4-row bag is asked for 4 + 3 rows: an inconsistent table
        out_lens[over] = 7
        cu, ch, T, n_chunks = _cu(out_lens, dev)

        def run(T_total, T_out, with_maps=True):
            out = torch.full((T + SLACK, D), float("nan"), device=dev)
            rb = torch.full((T + SLACK,), -99, dtype=torch.int32, device=dev)
            idx = torch.full((T + SLACK,), -99, dtype=torch.int32, device=dev)
            MF._call("mdl_bag_pack", store, 0, D, T_total, off, len(LENS), bag, key, cu, ch, R, n_chunks, T_out, D, 3, 4, out,
                     rb if with_maps else None, idx if with_maps else None, MF._stream())
            return out, rb, idx
        out, rb, idx = run(store.shape[0], T)
        assert not bool(torch.isnan(out[:T]).any()) and not bool((rb[:T] == -99).any()) and not bool((idx[:T] == -99).any())
        assert bool(torch.isnan(out[T:]).all()) and bool((rb[T:] == -99).all()) and bool((idx[T:] == -99).all())
        tail = int(cu[-4])
        assert not bool(out[tail:T].any()) and bool((idx[tail:T] == -1).all())                   # the three bags that do not exist
        lo = int(cu[over])
        assert torch.equal(out[lo:lo + 4], store[int(off[3]):int(off[4])]) and idx[lo:lo + 7].tolist() == [0, 1, 2, 3, -1, -1, -1]
        assert not bool(out[lo + 4:lo + 7].any())
        valid = torch.where(bag < len(LENS), bag, torch.full_like(bag, -1))
        present = idx[:T] >= 0
        src = off[valid.long().clamp(min=0)][rb[:T].long()] + idx[:T].long()
        assert torch.equal(out[:T], store.index_select(0, src.clamp(min=0)) * present.unsqueeze(1))
        assert torch.equal(rb[:T].long(), torch.repeat_interleave(torch.arange(R, device=dev), torch.tensor(out_lens, device=dev)))
        # T_total understated: the last stored bag leaves the store and is written as zeros, the others are unchanged
        out2, _, _ = run(int(off[-2]), T, with_maps=False)
        last = int((bag == len(LENS) - 1).nonzero()[0])
        a, b = int(cu[last]), int(cu[last + 1])
        assert not bool(out2[a:b].any()) and torch.equal(out2[:a], out[:a]) and torch.equal(out2[b:T], out[b:T])
        assert bool(torch.isnan(out2[T:]).all())
        # T_out understated (in the middle of a bag, not on a chunk boundary): nothing at or beyond it is written
        short = int(cu[last]) + 37
        out3, rb3, idx3 = run(store.shape[0], short)
        assert torch.equal(out3[:short], out[:short]) and torch.equal(rb3[:short], rb[:short]) and torch.equal(idx3[:short], idx[:short])
        assert bool(torch.isnan(out3[short:]).all()) and bool((rb3[short:] == -99).all()) and bool((idx3[short:] == -99).all())


def test_pack_does_not_synchronise_the_host(dev):
    st, _ = _lens_store(dev)
    st.pack([0, 1], 64, counter=0, return_indices=True)       # warm-up: library load, allocator, pinned staging
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        p = st.pack([2, 3, 4], 64, counter=1)
        q = st.pack([4], None, counter=2, return_indices=True)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert p.tokens.shape == (sum(p.lens), 32) and len(p.lens) == 9 and q.tokens.shape == (2 + 1000 + 4097, 32) and q.idx.shape == (5099,)


# ------------------------------------------------------------------------------------------------ end to end
E2E_MODS = ["HE", "HER2", "PGR"]
E2E_D = 512
E2E_LENS = [[300, 450, 700], [512, None, 333], [700, 301, 400], [650, 390, 310], [345, 600, 512], [480, 575, 699], [300, 640, None],
            [555, 444, 333]]


def _e2e_bags():
    return [[None if n is None else torch.from_numpy(recipe.uniform((n, E2E_D), "store:%d:%d" % (c, m))) for m, n in enumerate(case)]
            for c, case in enumerate(E2E_LENS)]


@pytest.fixture(scope="module")
def e2e_store(dev):
    return DeviceSlideStore(_e2e_bags(), ["case%d" % c for c in range(len(E2E_LENS))], E2E_MODS, dev)


def _model(dev, tag="store", stain_encoding=False):
    from madeleine_amd import MADELEINE
    cfg = SimpleNamespace(MODALITIES=E2E_MODS, wsi_encoder="abmil", patch_embedding_dim=E2E_D, wsi_encoder_hidden_dim=512,
                          activation="softmax", n_heads=4)
    m = MADELEINE(cfg, stain_encoding=stain_encoding)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.state_dict_recipe(shapes, tag).items()}, strict=True)
    return m.to(dev)


def _run(model, data, dev, n_views):
    np.random.seed(5)                     # the intra-modality views are drawn from numpy's generator
    with torch.no_grad():
        return model(data, device=dev, n_views=n_views)


def _same(a, b):
    for k in E2E_MODS:
        assert torch.isfinite(a[0][k]).all() and torch.equal(a[0][k], b[0][k]) and torch.equal(a[1][k], b[1][k]), k


@pytest.mark.parametrize("stain_encoding,n_views", [(False, 1), (False, 3), (True, 1)])
def test_packed_route_equals_the_bags_route(dev, e2e_store, stain_encoding, n_views):
    model = _model(dev, stain_encoding=stain_encoding).eval()
    ragged = list(e2e_store.ragged_batches(4, shuffle=True, seed=3))
    packed = list(e2e_store.packed_batches(4, shuffle=True, seed=3))
    assert len(ragged) == len(packed) == 2
    for rb, pb in zip(ragged, packed):
        assert set(pb) == {"packed", "modality_labels", "slide_ids"} and pb["slide_ids"] == rb["slide_ids"]
        assert torch.equal(pb["modality_labels"], rb["modality_labels"])
        p = pb["packed"]
        assert isinstance(p, PackedBags) and p.idx is None and p.tokens.device == dev
        assert list(p.lens) == [b.shape[0] for case in rb["bags"] for b in case]
        assert torch.equal(p.tokens, torch.cat([b for case in rb["bags"] for b in case]))
        _same(_run(model, pb, dev, n_views), _run(model, rb, dev, n_views))


def test_packed_route_from_a_bf16_store(dev):
    st = DeviceSlideStore(_e2e_bags(), ["case%d" % c for c in range(len(E2E_LENS))], E2E_MODS, dev, dtype=torch.bfloat16)
    model = _model(dev).eval()
    cases = [1, 4, 6, 2]
    labels = st.modality_labels[cases]
    zero = torch.zeros(2, E2E_D, device=dev)
    bags = [[zero if st.bag_view(c, m) is None else st.bag_view(c, m).float() for m in range(3)] for c in cases]
    _same(_run(model, {"packed": st.pack(cases), "modality_labels": labels}, dev, 1),
          _run(model, {"bags": bags, "modality_labels": labels}, dev, 1))


def test_capped_bags_equal_the_bags_route_on_the_rows_idx_names(dev, e2e_store):
    st = e2e_store
    model = _model(dev).eval()
    cases = [0, 1, 6, 3]
    labels = st.modality_labels[cases]
    p = st.pack(cases, max_tokens=300, counter=4, seed=9, return_indices=True)
    assert list(p.lens) == [2 if n is None else 300 for c in cases for n in E2E_LENS[c]]
    cu = p.cu_seqlens.tolist()
    zero = torch.zeros(2, E2E_D, device=dev)
    bags = [[zero if st.bag_view(c, m) is None else st.bag_view(c, m).index_select(0, p.idx[cu[3 * b + m]:cu[3 * b + m + 1]].long())
             for m in range(3)] for b, c in enumerate(cases)]
    assert torch.equal(torch.cat([x for case in bags for x in case]), p.tokens)
    assert p.idx[cu[0]:cu[1]].sort().values.tolist() == list(range(300))             # a 300-row bag at cap 300 is taken whole ...
    assert p.idx[cu[0]:cu[1]].tolist() == list(range(300)) and p.idx[cu[1]:cu[2]].tolist() != list(range(300))   # ... in stored order
    _same(_run(model, {"packed": p, "modality_labels": labels}, dev, 1), _run(model, {"bags": bags, "modality_labels": labels}, dev, 1))
    with pytest.raises(ValueError, match="n_loss_tokens=256"):
        model({"packed": st.pack(cases, max_tokens=200), "modality_labels": labels}, device=dev)


def test_train_loop_epoch_over_packed_batches(dev, e2e_store):
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
    loader = e2e_store.packed_batches(4, max_tokens=400, seed=1)
    loss, rank = train_loop(args, InfoNCE(temperature=0.1), GOT, InfoNCE(temperature=0.1), model, 1, loader, opt, sched, sched)
    assert np.isfinite(loss) and loss > 0 and np.isfinite(rank)
    after = dict(model.named_parameters())
    assert all(torch.isfinite(v).all() for v in after.values())
    assert sum(not torch.equal(before[k], after[k].detach()) for k in before) > len(before) // 2
