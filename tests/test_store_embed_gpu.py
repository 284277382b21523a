"""The cohort-embedding route of the slide store on the GPU: mdl_bag_mean against the fp64 mean of the stored rows under the error bound
of its documented addition depth, its bit contract (stride, order, subset, tier, slicing), the single-stain pack, encode_packed against
encode_he_bags, store.embed against encode_he bag by bag, and mean embeddings feeding the linear probe end to end."""
from types import SimpleNamespace

import pytest
import torch

from madeleine_amd import _native
from madeleine_amd import functional as MF
from madeleine_amd import store as store_mod
from madeleine_amd.store import DeviceSlideStore, PackedBags
from oracle import recipe

pytestmark = pytest.mark.gpu

RN = _native._DEFINES["MDL_BAG_MEAN_ROWS"]
THREADS, COLS = _native._DEFINES["MDL_BAG_MEAN_THREADS"], _native._DEFINES["MDL_BAG_MEAN_COLS"]
# 1, 2, both sides of a wave, both sides of the chunk, and several chunks with a short tail
LENS = [1, 2, 63, 64, 65, RN - 1, RN, RN + 1, 3 * RN + 7]
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
U = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def depth(n, D):
    """h(len) of the header's S5 comment."""
    slots = -(-D // COLS)
    lpr = 1
    while lpr < slots and lpr < THREADS:
        lpr *= 2
    G = THREADS // lpr
    return -(-min(n, RN) // G) + (G - 1) + (-(-n // RN) - 1)


def _rows(T, D, seed):
    """random normal with a per-column offset: mean |x| is not tiny against the mean"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(T, D, generator=g) + torch.linspace(-3.0, 3.0, D).unsqueeze(0)


def _tables(lens, bag, dev):
    """off, bag, chunk_cu on the device and n_chunks, for a store of bags of `lens` rows and the bag list `bag` (-1: absent)"""
    off = torch.zeros(len(lens) + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.tensor(lens), 0)
    n = torch.tensor([0 if g < 0 else lens[g] for g in bag], dtype=torch.int64)
    ch = torch.zeros(len(bag) + 1, dtype=torch.int64)
    ch[1:] = torch.cumsum((n + RN - 1) // RN, 0)
    return off.to(dev), torch.tensor(bag, dtype=torch.int32).to(dev), ch.to(dev), int(ch[-1])


def _mean(store, lens, bag, dev):
    off, bag_d, ch, n_chunks = _tables(lens, bag, dev)
    return MF.bag_mean(store, off, bag_d, ch, n_chunks)


BAG = list(range(len(LENS)))
BAG.insert(4, -1)                         # one absent stain in the middle of the list


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("D", [4, 33, 512])
def test_mean_is_accurate_to_its_addition_depth(dev, D, dtype):
    """|out - fp64 mean of the exactly widened stored rows| <= 2 h(len) 2^-24 mean_i |x_ij| per column: the forward error bound of a
    summation of depth h, the factor 2 covering the final scaling.  The -1 row is exactly zero and every row of out is written."""
    store = _rows(sum(LENS), D, D).to(dev).to(dtype)
    before = store.clone()
    off, bag_d, ch, n_chunks = _tables(LENS, BAG, dev)
    ws = MF._ws_for("mdl_bag_mean_ws_bytes", dev, n_chunks, D)
    out = torch.full((len(BAG), D), float("nan"), device=dev)
    MF._call("mdl_bag_mean", store, MF.STORE_DTYPES[dtype], D, store.shape[0], off, len(LENS), bag_d, ch, len(BAG), n_chunks, D, out, ws,
             MF._stream())
    assert not bool(torch.isnan(out).any())
    assert torch.equal(out, MF.bag_mean(store, off, bag_d, ch, n_chunks))
    check_mean(store, off, out)
    assert torch.equal(store, before)


def check_mean(store, off, out, lens=LENS, bag=BAG):
    """The depth bound of test_mean_is_accurate_to_its_addition_depth on `out`, the means of the bags `bag` of a store of `lens` rows."""
    D, dtype = store.shape[1], store.dtype
    wide, offs = store.double(), off.tolist()
    for r, g in enumerate(bag):
        if g < 0:
            assert not bool(out[r].any()) and not bool(torch.signbit(out[r]).any())
            continue
        x = wide[offs[g]:offs[g + 1]]
        err = (out[r].double() - x.mean(0)).abs()
        bound = 2.0 * depth(lens[g], D) * U * x.abs().mean(0)
        print("D %d %s len %d: h %d, max err / bound %.3f" % (D, dtype, lens[g], depth(lens[g], D), float((err / bound).max())))
        assert bool((err <= bound).all()), (lens[g], float((err / bound).max()))


@pytest.mark.parametrize("width,D", [(40, 32), (36, 32), (33, 32), (40, 33)])
def test_mean_of_a_strided_store_has_the_contiguous_bits(dev, width, D):
    """16-byte loads when D and the stride allow them ((40, 32) for every dtype, (36, 32) for fp32 alone), element-wise ones otherwise:
    the same additions, the same bits."""
    for dtype in DTYPES:
        wide = _rows(sum(LENS), width, width).to(dev).to(dtype)
        strided = wide[:, :D]
        assert strided.stride(0) == width
        assert torch.equal(_mean(strided, LENS, BAG, dev), _mean(strided.contiguous(), LENS, BAG, dev))


@pytest.mark.parametrize("dtype,D", [(torch.float32, 33), (torch.bfloat16, 64)], ids=["fp32-33", "bf16-64"])
def test_bits_depend_on_the_bag_alone(dev, dtype, D):
    store = _rows(sum(LENS), D, 3).to(dev).to(dtype)
    full = _mean(store, LENS, BAG, dev)
    assert torch.equal(_mean(store, LENS, BAG, dev), full)                                  # two calls
    perm = torch.randperm(len(BAG), generator=torch.Generator().manual_seed(1)).tolist()
    assert torch.equal(_mean(store, LENS, [BAG[i] for i in perm], dev), full[perm])           # another order
    sub = [8, 0, 4, 9, 9]
    assert torch.equal(_mean(store, LENS, [BAG[i] for i in sub], dev), full[sub])             # a subset, a bag twice
    for r, g in enumerate(BAG):                                                             # one bag at a time
        assert torch.equal(_mean(store, LENS, [g], dev)[0], full[r]), r


@pytest.mark.parametrize("dtype,D", [(torch.float32, 32), (torch.float32, 33), (torch.float16, 64)], ids=["fp32-32", "fp32-33", "fp16-64"])
def test_tiered_mean_splits_at_any_row(dev, dtype, D):
    """functional.bag_mean_tiered with T_dev inside a bag, inside a chunk, at 0 and at T_total: the bits of the resident store."""
    store = _rows(sum(LENS), D, 5).to(dev).to(dtype)
    off, bag_d, ch, n_chunks = _tables(LENS, BAG, dev)
    want = MF.bag_mean(store, off, bag_d, ch, n_chunks)
    T = store.shape[0]
    for T_dev, wgs in ((0, 0), (1, 3), (200, 1), (int(off[-2]) + RN + 100, 0), (T - 1, 2), (T, 0)):
        host = store[T_dev:].cpu().pin_memory()
        got = MF.bag_mean_tiered(store[:T_dev], host, off, bag_d, ch, n_chunks, host_wgs=wgs)
        assert torch.equal(got, want), T_dev


def _cohort(n_cases, D, seed, lens=None):
    g = torch.Generator().manual_seed(seed)
    lens = lens or [[1 + (37 * c + 11 * m) % 90 + (RN if (c + m) % 5 == 0 else 0) for m in range(2)] for c in range(n_cases)]
    bags = [[None if n is None else torch.randn(n, D, generator=g) + 0.5 for n in case] for case in lens]
    return bags, lens


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_mean_embeddings_of_a_tiered_and_a_sliced_store(dev, dtype, monkeypatch):
    """A store whose resident_bytes put the tier boundary inside the cohort gives the resident store's bits for host_wgs 1 and the
    default, and so does a workspace budget that cuts the cohort into many slices; every row is the mean of its bag."""
    D = 32
    bags, lens = _cohort(12, D, 2)
    lens[7][1], bags[7][1] = None, None
    ids = ["s%d" % c for c in range(len(bags))]
    res = DeviceSlideStore(bags, ids, ["HE", "IHC"], dev, dtype=dtype)
    row_bytes = D * res.rows.element_size()
    tiered = DeviceSlideStore(bags, ids, ["HE", "IHC"], dev, dtype=dtype, resident_bytes=(res.rows.shape[0] // 2) * row_bytes)
    assert tiered.rows_host is not None and 0 < tiered.resident_rows < res.rows.shape[0]
    for m in (0, 1):
        want = res.mean_embeddings(m)
        assert want["embeds"].shape == (12 - m, D) and want["embeds"].dtype == torch.float32 and want["embeds"].device == dev
        assert want["cases"].tolist() == [c for c in range(12) if lens[c][m] is not None] and want["cases"].dtype == torch.int64
        assert want["slide_ids"] == [ids[c] for c in want["cases"].tolist()]
        for i, c in enumerate(want["cases"].tolist()):
            x = res.bag_view(c, m).double()
            assert bool(((want["embeds"][i].double() - x.mean(0)).abs() <= 2.0 * depth(lens[c][m], D) * U * x.abs().mean(0)).all()), (c, m)
        for wgs in (1, 0):
            got = tiered.mean_embeddings(m, host_wgs=wgs)
            assert torch.equal(got["embeds"], want["embeds"]) and torch.equal(got["cases"], want["cases"])
        monkeypatch.setattr(store_mod, "MEAN_WS_BYTES", 3 * D * 4)          # three chunks per slice
        for st in (res, tiered):
            assert torch.equal(st.mean_embeddings(m)["embeds"], want["embeds"])
        monkeypatch.undo()
    some = res.mean_embeddings(1, [9, 2, 9])
    assert some["cases"].tolist() == [9, 2, 9] and torch.equal(some["embeds"], res.mean_embeddings(1)["embeds"][[8, 2, 8]])
    assert res.mean_embeddings(0, [])["embeds"].shape == (0, D)
    with pytest.raises(ValueError, match=r"case 7 \(s7\) has no IHC bag"):
        res.mean_embeddings(1, [0, 7])
    with pytest.raises(IndexError):
        res.mean_embeddings(2)


def test_mean_does_not_synchronise_the_host(dev):
    store = _rows(sum(LENS), 32, 9).to(dev)
    off, bag_d, ch, n_chunks = _tables(LENS, BAG, dev)
    want = MF.bag_mean(store, off, bag_d, ch, n_chunks)          # warm-up: library load, allocator
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = MF.bag_mean(store, off, bag_d, ch, n_chunks)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ packing and the encoder
MODS = ["HE", "HER2"]
ENC_D = 512
ENC_LENS = [[300, 270], [257, 300], [1000, 90], [40, None], [700, 512], [256, 310]]      # case 3 is without the second stain


def _enc_bags():
    return [[None if n is None else torch.from_numpy(recipe.uniform((n, ENC_D), "embed:%d:%d" % (c, m))) for m, n in enumerate(case)]
            for c, case in enumerate(ENC_LENS)]


def _enc_store(dev, **kw):
    return DeviceSlideStore(_enc_bags(), ["case%d" % c for c in range(len(ENC_LENS))], MODS, dev, **kw)


def _model(dev, stain_encoding=False):
    from madeleine_amd import MADELEINE
    cfg = SimpleNamespace(MODALITIES=MODS, wsi_encoder="abmil", patch_embedding_dim=ENC_D, wsi_encoder_hidden_dim=512,
                          activation="softmax", n_heads=4)
    m = MADELEINE(cfg, stain_encoding=stain_encoding)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.state_dict_recipe(shapes, "embed").items()}, strict=True)
    return m.to(dev)


@pytest.fixture(scope="module")
def enc(dev):
    """The fp32 store, the model in eval mode and encode_he of every bag alone (None for the absent stain): computed once."""
    st, model = _enc_store(dev), _model(dev).eval()
    with torch.no_grad():
        alone = [[None if n is None else model.encode_he(st.bag_view(c, m)[None], dev) for m, n in enumerate(case)]
                 for c, case in enumerate(ENC_LENS)]
    return SimpleNamespace(store=st, model=model, alone=alone)


def _alone(enc, m, cases):
    return torch.cat([enc.alone[c][m] for c in cases])


def test_pack_modality_is_the_cat_of_the_bags(dev, enc):
    st = enc.store
    cases = [0, 1, 2, 3, 4, 5]
    p = st.pack_modality(cases, 0)
    assert isinstance(p, PackedBags) and p.idx is None and p.tokens.dtype == torch.float32 and p.tokens.device == dev
    assert list(p.lens) == [n[0] for n in ENC_LENS] and p.cu_seqlens.dtype == torch.int64 and p.cu_seqlens.device == dev
    assert p.cu_seqlens.tolist() == torch.tensor([0] + list(p.lens)).cumsum(0).tolist()
    assert torch.equal(p.tokens, torch.cat([st.bag_view(c, 0) for c in cases]))
    assert torch.equal(p.row_bag.long(), torch.repeat_interleave(torch.arange(6, device=dev), torch.tensor(p.lens, device=dev)))
    q = st.pack_modality([5, 0], 1)
    assert list(q.lens) == [310, 270] and torch.equal(q.tokens, torch.cat([st.bag_view(5, 1), st.bag_view(0, 1)]))
    half = _enc_store(dev, dtype=torch.bfloat16)
    assert torch.equal(half.pack_modality(cases, 0).tokens, torch.cat([half.bag_view(c, 0).float() for c in cases]))
    # capped: the rows sample(..., 128, counter, seed) draws for the bag; a bag that fits is taken whole
    c = st.pack_modality(cases, 0, max_tokens=128, counter=7, seed=5)
    feats = st.sample(cases, 128, counter=7, seed=5)
    cu = c.cu_seqlens.tolist()
    assert list(c.lens) == [128, 128, 128, 40, 128, 128]
    for r in range(6):
        want = st.bag_view(r, 0) if ENC_LENS[r][0] <= 128 else feats[r, 0]
        assert torch.equal(c.tokens[cu[r]:cu[r + 1]], want), r
    with pytest.raises(ValueError, match=r"case 3 \(case3\) has no HER2 bag"):
        st.pack_modality([0, 3], 1)
    with pytest.raises(IndexError):
        st.pack_modality([0], 2)


def test_encode_packed_equals_encode_he_bags(dev, enc):
    st, model = enc.store, enc.model
    for m, cases in ((0, [0, 1, 2, 4]), (1, [4, 1, 5]), (0, [2]), (0, [0, 3, 5])):
        bags = [st.bag_view(c, m) for c in cases]
        p = st.pack_modality(cases, m)
        with torch.no_grad():
            want = model.encode_he_bags(bags, dev)
            got = model.encode_packed(p, dev)
            again = model.encode_packed((p.tokens, p.cu_seqlens, p.lens), dev)
        assert got.shape == (len(cases), 512) and torch.isfinite(got).all()
        assert torch.equal(got, want) and torch.equal(again, want), (m, cases)
    with pytest.raises(ValueError):
        model.encode_packed((p.tokens, p.cu_seqlens, (1, 2)), dev)


def test_embed_equals_encode_he_of_every_bag_alone(dev, enc):
    st, model = enc.store, enc.model
    want = _alone(enc, 0, range(6))
    for bpl in (1, 2, 4, None):
        res = st.embed(model, bags_per_launch=bpl)
        assert set(res) == {"embeds", "cases", "slide_ids"}
        assert res["embeds"].shape == (6, 512) and res["embeds"].dtype == torch.float32 and res["embeds"].device == dev
        assert torch.equal(res["embeds"], want), bpl                     # the 40-row and the 256-row bag included
        assert res["cases"].tolist() == list(range(6)) and res["cases"].dtype == torch.int64 and not res["cases"].is_cuda
        assert res["slide_ids"] == ["case%d" % c for c in range(6)]
    assert not model.training
    model.train()
    try:
        res = st.embed(model, case_indices=[4, 2])
        assert model.training                                            # the flag is restored ...
    finally:
        model.eval()
    assert torch.equal(res["embeds"], want[[4, 2]]) and res["cases"].tolist() == [4, 2] and res["slide_ids"] == ["case4", "case2"]      # ... and was off inside


def test_embed_refusals_and_the_second_stain(dev, enc):
    st, model = enc.store, enc.model
    res = st.embed(model, modality=1)
    assert res["cases"].tolist() == [0, 1, 2, 4, 5] and res["slide_ids"] == ["case0", "case1", "case2", "case4", "case5"]
    assert torch.equal(res["embeds"], _alone(enc, 1, [0, 1, 2, 4, 5]))
    with pytest.raises(ValueError, match=r"case 3 \(case3\) has no HER2 bag"):
        st.embed(model, modality=1, case_indices=[0, 3])
    with pytest.raises(IndexError):
        st.embed(model, modality=2)
    stained = _model(dev, stain_encoding=True).eval()
    with pytest.raises(ValueError, match="stain encoding"):
        st.embed(stained, modality=1)


def test_embed_from_a_bf16_store(dev, enc):
    st = _enc_store(dev, dtype=torch.bfloat16)
    res = st.embed(enc.model)
    with torch.no_grad():
        want = torch.cat([enc.model.encode_he(st.bag_view(c, 0).float()[None], dev) for c in range(6)])
    assert torch.equal(res["embeds"], want)


def test_embed_from_a_tiered_store(dev, enc):
    row_bytes = ENC_D * 4
    st = _enc_store(dev, resident_bytes=1500 * row_bytes)
    assert st.rows_host is not None and 0 < st.resident_rows <= 1500
    assert torch.equal(st.embed(enc.model)["embeds"], _alone(enc, 0, range(6)))
    assert torch.equal(st.embed(enc.model, modality=1, host_wgs=1)["embeds"], _alone(enc, 1, [0, 1, 2, 4, 5]))


def test_embed_under_autocast(dev, enc):
    st, model = enc.store, enc.model
    res = st.embed(model, precision=torch.bfloat16)
    with torch.no_grad(), torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        want = torch.cat([model.encode_he(st.bag_view(c, 0)[None], dev).float() for c in range(6)])
    assert res["embeds"].dtype == torch.float32 and torch.equal(res["embeds"], want)
    assert not torch.equal(res["embeds"], _alone(enc, 0, range(6)))      # (it did run under autocast)


def test_mean_embeddings_feed_the_linear_probe(dev):
    """40 cases in two classes that differ by 8 standard deviations in every column: separable by construction, so exact scores assert
    the plumbing from the store to the probe, not a tolerance."""
    from madeleine_amd import linear_probe
    D, g = 32, torch.Generator().manual_seed(4)
    labels = torch.tensor([c % 2 for c in range(40)])
    bags = [[torch.randn(3 + (7 * c) % 23, D, generator=g) + 8.0 * int(labels[c])] for c in range(40)]
    st = DeviceSlideStore(bags, ["p%d" % c for c in range(40)], ["HE"], dev)
    res = linear_probe(st.mean_embeddings()["embeds"], labels, ks=(1,), folds=2)[("label", 1)]
    assert res["auc"].tolist() == [1.0, 1.0] and res["bacc"].tolist() == [1.0, 1.0]
