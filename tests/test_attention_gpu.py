"""The attention read-out on the GPU: mdl_attn_rank against the integer reference of tests/_attn_ref.py bit for bit (order, percentile
ranks, top-k; any bit pattern), mdl_attn_softmax against the fp64 softmax under the error bound of its documented addition depth, the
bit contracts of both (R, bag order, row stride), MADELEINE.attend_packed and DeviceSlideStore.attention against store.embed, the dense
return_attention branch and the oracle, and the eval branch's stain rule."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from madeleine_amd import functional as MF
from madeleine_amd.abmil import activate
from madeleine_amd.store import DeviceSlideStore
from oracle import recipe
from oracle import restatement as R
from tests import _attn_ref as ref
from tests._util import max_rel, rel_err

pytestmark = pytest.mark.gpu

C = MF.ATTN_SORT_KEYS
ROWS = MF.ATTN_ROWS
# 1, 2, both sides of a wave, of a 256-thread sweep and of the chunk, and several chunks with a short tail (there is no short-segment
# path: every length runs the same kernels)
LENS = [1, 2, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1, 3 * C + 7]
SETS = ["normals", "five", "equal", "bits"]
KMAX = max(LENS) + 5
U = 2.0 ** -24
TOL = 1e-3          # tests/test_model_gpu.py's
# K of the softmax bound: what the device's expf and the division add on top of the addition depth h(n) and the rounding of s - m.
# Measured on the MI355X over the three finite score sets, H in {1, 4}, as the worst
#     |attn - exp(fl32(s - m)) / l| / (2^-24 attn)        (exp and the quotient in fp64, m and l the device's own)
# which is the error of the device's expf and of its one division alone: K_MEASURED units of 2^-24.  K is twice that.  (The excess of
# the whole error over h(n) + |s - m| is printed too; it was negative for every element: a sum of positive terms stays far from the
# worst case of its depth.)
K_MEASURED = 2.047      # normals, H = 4; 1.905 at H = 1, 1.347 on the five values, 0.992 on equal scores
K = 2.0 * K_MEASURED


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def depth(n):
    """h(n) of the header's A-map comment"""
    return (ROWS // 256 - 1) + 6 + 2 + (-(-n // ROWS) - 1)


@functools.lru_cache(maxsize=None)
def scores_of(name, H):
    T = sum(LENS)
    rng = np.random.default_rng(len(name) * 8 + H)
    if name == "normals":       # distinct by construction
        s = (rng.permutation(T * H).astype(np.float32) / np.float32(T * H) * 8 - 4).reshape(T, H)
        assert len(np.unique(s)) == T * H
    elif name == "five":
        s = rng.choice(np.array([-1.5, -0.25, 0.0, 2.0, 3.25], np.float32), (T, H))
    elif name == "equal":
        s = np.full((T, H), 0.625, np.float32)
    else:                       # every digit of every pass, both zeros, infinities, NaNs of both signs, denormals
        s = rng.integers(0, 2 ** 32, (T, H), dtype=np.uint64).astype(np.uint32).view(np.float32)
        s[:8, 0] = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 1e-45, -1e-45], np.float32)[:min(8, T)]
    s.setflags(write=False)
    return s


def cu_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def reference(name, H):
    """computed once per score set, shared and left unchanged"""
    out = ref.readout(scores_of(name, H), cu_of(LENS), KMAX)
    for v in out.values():
        v.setflags(write=False)
    return out


def on_device(s, dev, pad):
    """scores on the device with row stride H + pad"""
    t = torch.from_numpy(np.array(s)).to(dev)
    if pad == 0:
        return t
    wide = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), device=dev)
    wide[:, :t.shape[1]] = t
    view = wide[:, :t.shape[1]]
    assert view.stride(0) == t.shape[1] + pad
    return view


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy() if t.dtype == torch.float32 else t.detach().cpu().numpy()


def permuted(s, lens, perm):
    """the pack with its bags in the order `perm`: (scores, lens, the first row of every new bag in the old pack)"""
    cu = cu_of(lens)
    rows = np.concatenate([np.arange(cu[i], cu[i + 1]) for i in perm])
    return s[rows], [lens[i] for i in perm], rows


# ------------------------------------------------------------------------------------------------ rank
def check_rank(name, H, k, order, pct, ti, tv):
    """The outputs of one attn_rank call on scores_of(name, H) against the reference, exactly."""
    s, want = scores_of(name, H), reference(name, H)
    assert order.shape == (H, len(s)) and order.dtype == torch.int32 and pct.shape == s.shape and pct.dtype == torch.float32
    assert np.array_equal(order.cpu().numpy(), want["order"]), k
    assert np.array_equal(bits(pct), want["pct"].view(np.int32)), k
    if k == 0:
        assert ti is None and tv is None
        return
    assert ti.shape == tv.shape == (len(LENS), H, k) and ti.dtype == torch.int32 and tv.dtype == torch.float32
    assert np.array_equal(ti.cpu().numpy(), want["topk_idx"][:, :, :k]), k
    assert np.array_equal(bits(tv), np.ascontiguousarray(want["topk_val"][:, :, :k]).view(np.int32)), k


@pytest.mark.parametrize("pad", [0, 3], ids=["ld=H", "ld=H+3"])
@pytest.mark.parametrize("H", [1, 4])
@pytest.mark.parametrize("name", SETS)
def test_rank_equals_the_reference_exactly(dev, name, H, pad):
    s, want = scores_of(name, H), reference(name, H)
    cu = torch.from_numpy(cu_of(LENS)).to(dev)
    sd = on_device(s, dev, pad)
    before = sd.clone()
    for k in (0, 1, 16, KMAX):
        order, pct, ti, tv = MF.attn_rank(sd, cu, k=k)
        check_rank(name, H, k, order, pct, ti, tv)
    again = MF.attn_rank(sd, cu, k=KMAX)
    for a, b in zip(again, (order, pct, ti, tv)):
        assert np.array_equal(bits(a), bits(b)), "two calls"
    assert MF.attn_rank(sd, cu, k=3, percentile=False)[1] is None
    assert np.array_equal(bits(sd.contiguous()), bits(before.contiguous())), "the scores are only read"


@pytest.mark.parametrize("name", ["five", "bits"])
def test_rank_does_not_depend_on_the_other_bags(dev, name):
    H = 4
    s, want = scores_of(name, H), reference(name, H)
    cu = cu_of(LENS)
    perm = np.random.default_rng(1).permutation(len(LENS)).tolist()
    sp, lp, rows = permuted(s, LENS, perm)
    cup = cu_of(lp)
    order, pct, ti, tv = MF.attn_rank(on_device(sp, dev, 0), torch.from_numpy(cup).to(dev), k=16)
    order, pct, ti, tv = order.cpu().numpy(), bits(pct), ti.cpu().numpy(), bits(tv)
    assert np.array_equal(pct, want["pct"].view(np.int32)[rows])
    assert np.array_equal(order, want["order"][:, rows])
    assert np.array_equal(ti, want["topk_idx"][perm, :, :16])
    assert np.array_equal(tv, np.ascontiguousarray(want["topk_val"][perm, :, :16]).view(np.int32))
    for i in (0, 7, 11):             # one bag alone: R = 1
        a, b = int(cu[i]), int(cu[i + 1])
        o1, p1, t1, _ = MF.attn_rank(on_device(s[a:b], dev, 0), torch.tensor([0, b - a], device=dev), k=16)
        assert np.array_equal(o1.cpu().numpy(), want["order"][:, a:b]) and np.array_equal(bits(p1), want["pct"].view(np.int32)[a:b])
        assert np.array_equal(t1.cpu().numpy()[0], want["topk_idx"][i, :, :16])


def test_empty_bags_and_an_empty_pack(dev):
    lens = [0, 5, 0, 0, C + 3, 0]
    s = scores_of("five", 4)[:sum(lens)]
    cu = torch.from_numpy(cu_of(lens)).to(dev)
    want = ref.readout(s, cu_of(lens), 4)
    order, pct, ti, tv = MF.attn_rank(on_device(s, dev, 0), cu, k=4)
    assert np.array_equal(order.cpu().numpy(), want["order"]) and np.array_equal(bits(pct), want["pct"].view(np.int32))
    assert np.array_equal(ti.cpu().numpy(), want["topk_idx"]) and np.array_equal(bits(tv), want["topk_val"].view(np.int32))
    attn, m, l = MF.attn_softmax(on_device(s, dev, 0), cu)
    for r, n in enumerate(lens):
        if n == 0:
            assert bool(torch.isneginf(m[r]).all()) and not bool(l[r].any())
    assert abs(float(attn.double().sum()) - 2 * 4) < 1e-4
    zero = torch.zeros(0, 4, device=dev)
    a0, m0, l0 = MF.attn_softmax(zero, torch.zeros(3, dtype=torch.int64, device=dev))
    assert a0.shape == (0, 4) and bool(torch.isneginf(m0).all()) and m0.shape == (2, 4) and not bool(l0.any())
    o0, p0, t0, v0 = MF.attn_rank(zero, torch.zeros(3, dtype=torch.int64, device=dev), k=2)
    assert o0.shape == (4, 0) and p0.shape == (0, 4) and bool((t0 == -1).all()) and bool(torch.isneginf(v0).all())


def test_a_cu_that_is_not_consistent_stays_inside_the_buffers(dev):
    """bags that run backwards or leave [0, T] are served as empty bags; the guard rows around every buffer keep their values: scores,
    cu, every output and both workspaces (at exactly mdl_attn_map_ws_bytes) are carved from one guarded arena (tests/_arena.py), under
    both of its fills, and the outputs do not depend on the fill"""
    from tests._extent_cases import run_case
    H, T, k = 4, 600, 4
    s = scores_of("normals", H)[:T]
    cu_host = torch.tensor([0, 300, 200, 700, -5, 300, 600], dtype=torch.int64)               # valid: [0, 300) and [300, 600)
    R_ = cu_host.numel() - 1
    i32, f32 = torch.int32, torch.float32

    def case(r):
        sd, cu = r.inp("scores", (T, H), f32, torch.from_numpy(s.copy())), r.inp("cu", (R_ + 1,), torch.int64, cu_host)
        order, pct = r.out("order", (H, T), i32), r.out("pct", (T, H))
        ti, tv = r.out("topk_idx", (R_, H, k), i32), r.out("topk_val", (R_, H, k))
        r.call("mdl_attn_rank", sd, H, cu, T, R_, H, k, order, pct, ti, tv, r.ws("ws_rank", "mdl_attn_map_ws_bytes", T, R_, H), r.stream())
        attn, m, l = r.out("attn", (T, H)), r.out("m", (R_, H)), r.out("l", (R_, H))
        r.call("mdl_attn_softmax", sd, H, cu, T, R_, H, attn, m, l, r.ws("ws_softmax", "mdl_attn_map_ws_bytes", T, R_, H), r.stream())
        return dict(order=order, pct=pct, ti=ti, tv=tv, attn=attn, m=m, l=l)

    def check(got):
        ti, m, l = got["ti"], got["m"], got["l"]
        assert ti[:, 0, 0].tolist()[1:5] == [-1, -1, -1, -1] and bool(torch.isneginf(m[1:5]).all()) and not bool(l[1:5].any())
        assert np.array_equal(ti[0].numpy(), ref.readout(s[:300], cu_of([300]), 4)["topk_idx"][0])
        assert np.array_equal(ti[5].numpy(), ref.readout(s[300:600], cu_of([300]), 4)["topk_idx"][0])
    run_case(dev, case, check)


def test_the_read_out_does_not_synchronise_the_host(dev):
    sd = on_device(scores_of("five", 4), dev, 0)
    cu = torch.from_numpy(cu_of(LENS)).to(dev)
    want = MF.attn_rank(sd, cu, k=16) + MF.attn_softmax(sd, cu)          # warm-up: library load, allocator
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = MF.attn_rank(sd, cu, k=16) + MF.attn_softmax(sd, cu)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    for a, b in zip(got, want):
        assert np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ softmax
@pytest.mark.parametrize("H", [1, 4])
@pytest.mark.parametrize("name", ["normals", "five", "equal"])
def test_softmax_is_accurate_to_its_addition_depth(dev, name, H):
    """|attn - a64| <= (h(n) + |s - m| + K) 2^-24 a64 per element, m the exact maximum, l the sum, attn monotone in raw."""
    s = scores_of(name, H)
    attn, m, l = MF.attn_softmax(on_device(s, dev, 0), torch.from_numpy(cu_of(LENS)).to(dev))
    check_softmax(name, H, attn, m, l)


def check_softmax(name, H, attn, m, l):
    """The bound of test_softmax_is_accurate_to_its_addition_depth on the outputs (attn, m, l) of one call on scores_of(name, H)."""
    s = scores_of(name, H)
    cu = cu_of(LENS)
    assert attn.shape == s.shape and m.shape == l.shape == (len(LENS), H)
    attn, m, l = attn.cpu().numpy(), m.cpu().numpy(), l.cpu().numpy()
    worst, k_obs = -np.inf, 0.0
    for r, n in enumerate(LENS):
        for h in range(H):
            seg = s[cu[r]:cu[r + 1], h]
            a64, mx = ref.softmax64(seg)
            assert m[r, h] == mx, (n, h)
            gap = np.abs(seg.astype(np.float64) - float(mx))
            err = np.abs(attn[cu[r]:cu[r + 1], h].astype(np.float64) - a64) / (U * a64)
            worst = max(worst, float((err - depth(n) - gap).max()))
            direct = np.exp((seg - mx).astype(np.float64)) / float(l[r, h])
            k_obs = max(k_obs, float((np.abs(attn[cu[r]:cu[r + 1], h].astype(np.float64) - direct) / (U * direct)).max()))
            assert bool((err <= depth(n) + gap + K).all()), (n, h, float((err - depth(n) - gap).max()))
            l64 = np.exp(seg.astype(np.float64) - float(mx)).sum()
            assert abs(float(l[r, h]) - l64) <= (depth(n) + gap.max() + K) * U * l64, (n, h)
            o = np.argsort(seg, kind="stable")
            assert bool((np.diff(attn[cu[r]:cu[r + 1], h][o]) >= 0).all()), "monotone in raw"
    print("softmax %s H %d: expf and division alone %.3f x 2^-24 (K = %.3f); worst excess over h(n) + |s - m|: %.3f" % (name, H, k_obs, K, worst))


@pytest.mark.parametrize("name", ["normals", "bits"])
def test_softmax_bits_depend_on_the_segment_alone(dev, name):
    H = 4
    s = scores_of(name, H)
    cu = cu_of(LENS)
    full = MF.attn_softmax(on_device(s, dev, 0), torch.from_numpy(cu).to(dev))
    fa, fm, fl = (bits(x) for x in full)
    if name == "bits":          # m passes over NaNs: the maximum of the others
        got_m = full[1].cpu().numpy()
        for r in range(len(LENS)):
            for h in range(H):
                seg = s[cu[r]:cu[r + 1], h]
                assert np.isnan(seg).all() or got_m[r, h] == seg[~np.isnan(seg)].max(), (r, h)
    for x, y in zip(MF.attn_softmax(on_device(s, dev, 0), torch.from_numpy(cu).to(dev)), (fa, fm, fl)):
        assert np.array_equal(bits(x), y), "two calls"
    for x, y in zip(MF.attn_softmax(on_device(s, dev, 3), torch.from_numpy(cu).to(dev)), (fa, fm, fl)):
        assert np.array_equal(bits(x), y), "ld = H + 3"
    perm = np.random.default_rng(2).permutation(len(LENS)).tolist()
    sp, lp, rows = permuted(s, LENS, perm)
    pa, pm, pl = MF.attn_softmax(on_device(sp, dev, 0), torch.from_numpy(cu_of(lp)).to(dev))
    assert np.array_equal(bits(pa), fa[rows]) and np.array_equal(bits(pm), fm[perm]) and np.array_equal(bits(pl), fl[perm])
    for i in (0, 4, 11):        # one bag alone: R = 1
        a, b = int(cu[i]), int(cu[i + 1])
        a1, m1, l1 = MF.attn_softmax(on_device(s[a:b], dev, 0), torch.tensor([0, b - a], device=dev))
        assert np.array_equal(bits(a1), fa[a:b]) and np.array_equal(bits(m1)[0], fm[i]) and np.array_equal(bits(l1)[0], fl[i])


# ------------------------------------------------------------------------------------------------ the model and the store
MODS = ["HE", "HER2"]
ENC_D = 96
ENC_LENS = [[7, 300], [256, 257], [257, None], [300, 7], [1025, 256]]


def _model(dev, mods, d_in, tag, stain_encoding=False, act="softmax"):
    from madeleine_amd import MADELEINE
    cfg = SimpleNamespace(MODALITIES=list(mods), wsi_encoder="abmil", patch_embedding_dim=d_in, wsi_encoder_hidden_dim=512,
                          activation=act, n_heads=4)
    m = MADELEINE(cfg, stain_encoding=stain_encoding)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.state_dict_recipe(shapes, tag).items()}, strict=True)
    return m.to(dev).eval()


def _enc_bags():
    return [[None if n is None else torch.from_numpy(recipe.uniform((n, ENC_D), "attn:%d:%d" % (c, m))) for m, n in enumerate(case)]
            for c, case in enumerate(ENC_LENS)]


def _enc_store(dev, **kw):
    return DeviceSlideStore(_enc_bags(), ["case%d" % c for c in range(len(ENC_LENS))], MODS, dev, **kw)


@pytest.fixture(scope="module")
def enc(dev):
    """The fp32 store, the model, store.attention of the H&E bags and the oracle of every H&E bag alone: computed once."""
    st, model = _enc_store(dev), _model(dev, MODS, ENC_D, "attn")
    res = st.attention(model, topk=16)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    oracle = []
    for c in range(len(ENC_LENS)):
        out = R.abmil_embed(st.bag_view(c, 0).cpu()[None], sd)
        slide = torch.nn.functional.linear(out["slide"].reshape(1, -1), sd["projector.weight"], sd["projector.bias"])
        oracle.append((out["raw"].reshape(-1, 4), slide[0]))
    return SimpleNamespace(store=st, model=model, res=res, oracle=oracle)


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        if torch.is_tensor(a[k]):
            assert a[k].shape == b[k].shape and np.array_equal(bits(a[k]), bits(b[k])), k
        else:
            assert a[k] == b[k], k


def test_attention_of_a_store(dev, enc):
    st, model, res = enc.store, enc.model, enc.res
    n, lens = len(ENC_LENS), [case[0] for case in ENC_LENS]
    T = sum(lens)
    assert set(res) == {"embeds", "cases", "slide_ids", "cu_seqlens", "lens", "raw", "attention", "percentile", "order", "topk_idx",
                        "topk_val"}
    assert res["lens"] == lens and res["cases"].tolist() == list(range(n)) and res["slide_ids"] == ["case%d" % c for c in range(n)]
    assert res["cu_seqlens"].tolist() == cu_of(lens).tolist() and res["cu_seqlens"].dtype == torch.int64 and res["cu_seqlens"].device == dev
    assert res["raw"].shape == res["attention"].shape == res["percentile"].shape == (T, 4) and res["order"].shape == (4, T)
    assert res["topk_idx"].shape == res["topk_val"].shape == (n, 4, 16)
    assert all(res[k].device == dev for k in ("embeds", "raw", "attention", "percentile", "order", "topk_idx", "topk_val"))
    # the embeddings are store.embed's, bit for bit
    assert torch.equal(res["embeds"], st.embed(model)["embeds"])
    # the raw scores are the dense return_attention branch's on every bag alone, bit for bit, and the oracle's within TOL
    cu = cu_of(lens)
    for c in range(n):
        with torch.no_grad():
            he, raw = model({"feats": st.bag_view(c, 0)[None, None]}, dev, train=False, return_attention=True)
        mine = res["raw"][cu[c]:cu[c + 1]]
        assert raw.shape == (1, lens[c], 1, 4)
        assert torch.equal(mine, raw.reshape(lens[c], 4)), c
        assert torch.equal(res["embeds"][c], he.reshape(-1)), c
        o_raw, o_slide = enc.oracle[c]
        assert max_rel(mine, o_raw) < TOL and rel_err(res["embeds"][c], o_slide) < TOL, c
    # the maps are the functional calls on raw
    attn, _, _ = MF.attn_softmax(res["raw"], res["cu_seqlens"])
    order, pct, ti, tv = MF.attn_rank(res["raw"], res["cu_seqlens"], k=16)
    for k, v in (("attention", attn), ("order", order), ("percentile", pct), ("topk_idx", ti), ("topk_val", tv)):
        assert np.array_equal(bits(res[k]), bits(v)), k
    want = ref.readout(res["raw"].cpu().numpy(), cu, 16)
    assert np.array_equal(res["order"].cpu().numpy(), want["order"]) and np.array_equal(bits(res["percentile"]), want["pct"].view(np.int32))
    for c in range(n):
        a = res["attention"][cu[c]:cu[c + 1]].double()
        assert bool(((a.sum(0) - 1).abs() < 1e-5).all())
        assert rel_err(a, torch.softmax(res["raw"][cu[c]:cu[c + 1]].double(), 0)) < 1e-6
    # no dependence on the grouping; k = 0 and percentile=False give None
    for bpl in (1, 4):
        _same(st.attention(model, topk=16, bags_per_launch=bpl), res)
    lean = st.attention(model, percentile=False)
    assert lean["topk_idx"] is None and lean["topk_val"] is None and lean["percentile"] is None
    assert torch.equal(lean["order"], res["order"])
    # a subset in the order asked, the second stain, and the refusals of the plan
    some = st.attention(model, case_indices=[4, 0], topk=16)
    assert some["cases"].tolist() == [4, 0] and torch.equal(some["embeds"], res["embeds"][[4, 0]])
    assert torch.equal(some["raw"], torch.cat([res["raw"][cu[4]:cu[5]], res["raw"][cu[0]:cu[1]]]))
    assert torch.equal(some["topk_idx"], res["topk_idx"][[4, 0]])
    second = st.attention(model, modality=1)
    assert second["cases"].tolist() == [0, 1, 3, 4] and torch.equal(second["embeds"], st.embed(model, modality=1)["embeds"])
    with pytest.raises(ValueError, match=r"case 2 \(case2\) has no HER2 bag"):
        st.attention(model, modality=1, case_indices=[0, 2])
    with pytest.raises(IndexError):
        st.attention(model, modality=2)
    assert not model.training
    model.train()
    try:
        again = st.attention(model, topk=16)
        assert model.training                                            # the flag is restored ...
    finally:
        model.eval()
    _same(again, res)                                                    # ... and was off inside


def test_attend_packed_is_encode_packed_with_the_scores_kept(dev, enc):
    st, model, res = enc.store, enc.model, enc.res
    cu = cu_of([case[0] for case in ENC_LENS])
    for cases in ([2, 3, 4], [4], [0, 3]):          # the packed route, one bag, a 7-row bag in a pack
        p = st.pack_modality(cases, 0)
        with torch.no_grad():
            embeds, raw = model.attend_packed(p, dev)
            again = model.attend_packed((p.tokens, p.cu_seqlens, p.lens), dev, stain_idx=1)      # ignored without stain encoding
            assert torch.equal(embeds, model.encode_packed(p, dev))
        assert torch.equal(again[0], embeds) and torch.equal(again[1], raw)
        assert raw.shape == (sum(p.lens), 4) and embeds.shape == (len(cases), 512)
        if min(p.lens) > 256:                          # (a short bag inside a pack is on another kernel path than alone)
            assert torch.equal(raw, torch.cat([res["raw"][cu[c]:cu[c + 1]] for c in cases]))
            assert torch.equal(embeds, res["embeds"][cases])
    with pytest.raises(ValueError):
        model.attend_packed((p.tokens, p.cu_seqlens, (1, 2)), dev)


def test_attention_from_a_bf16_and_a_tiered_store(dev, enc):
    half = _enc_store(dev, dtype=torch.bfloat16)
    res = half.attention(enc.model, topk=16)
    assert torch.equal(res["embeds"], half.embed(enc.model)["embeds"])
    with torch.no_grad():
        _, raw = enc.model({"feats": half.bag_view(4, 0).float()[None, None]}, dev, train=False, return_attention=True)
    assert torch.equal(res["raw"][-1025:], raw.reshape(1025, 4))
    tiered = _enc_store(dev, resident_bytes=600 * ENC_D * 4)
    assert tiered.rows_host is not None and 0 < tiered.resident_rows <= 600
    _same(tiered.attention(enc.model, topk=16), enc.res)
    _same(tiered.attention(enc.model, topk=16, host_wgs=1), enc.res)


def test_the_relu_activation_fills_attention_element_wise(dev, enc):
    model = _model(dev, MODS, ENC_D, "attn", act="relu")
    res = enc.store.attention(model, topk=16)
    assert torch.equal(res["attention"], activate(res["raw"], "relu")) and bool((res["attention"] >= 0).all())
    assert torch.equal(res["embeds"], enc.store.embed(model)["embeds"])
    order, pct, ti, tv = MF.attn_rank(res["raw"], res["cu_seqlens"], k=16)      # ranks and top-k are of the raw scores
    assert torch.equal(res["order"], order) and torch.equal(res["percentile"], pct) and torch.equal(res["topk_idx"], ti)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    out = R.abmil_embed(enc.store.bag_view(3, 0).cpu()[None], sd, activation="relu")
    cu = cu_of([case[0] for case in ENC_LENS])
    assert max_rel(res["raw"][cu[3]:cu[4]], out["raw"].reshape(-1, 4)) < TOL


# ------------------------------------------------------------------------------------------------ stain encoding
MODS3 = ["HE", "HER2", "PGR"]
ST_D = 64


@pytest.fixture(scope="module")
def stained(dev):
    return _model(dev, MODS3, ST_D, "attnstain", stain_encoding=True)


@pytest.mark.parametrize("m", [0, 1, 2])
def test_attend_packed_applies_the_true_stain_index(dev, stained, m):
    """The eval branch's rule (Model.py:162-203): every bag of the pack gets embedding(stain_idx).  Against the oracle on
    [x | embedding.weight[m]] at TOL, and on equal-length bags against forward(train=False, custom_stain_idx=m) at 1e-5 relative
    (two routes of the same arithmetic: the bound of the ragged-versus-dense activation test)."""
    sd = {k: v.detach().cpu() for k, v in stained.state_dict().items()}
    lens = [300, 257, 410]
    bags = [torch.from_numpy(recipe.uniform((n, ST_D), "attnstain:f%d" % i)) for i, n in enumerate(lens)]
    tokens, cu = torch.cat(bags).to(dev), torch.from_numpy(cu_of(lens)).to(dev)
    with torch.no_grad():
        embeds, raw = stained.attend_packed((tokens, cu, lens), dev, stain_idx=m)
    c = cu_of(lens)
    for i, n in enumerate(lens):
        x = torch.cat([bags[i], sd["embedding.weight"][m].expand(n, -1)], dim=-1).unsqueeze(0)
        out = R.abmil_embed(x, sd)
        slide = torch.nn.functional.linear(out["slide"].reshape(1, -1), sd["projector.weight"], sd["projector.bias"])
        assert rel_err(embeds[i], slide[0]) < TOL and max_rel(raw[c[i]:c[i + 1]], out["raw"].reshape(-1, 4)) < TOL, i
    if m == 0:
        with torch.no_grad():
            default = stained.attend_packed((tokens, cu, lens), dev)
        assert torch.equal(default[0], embeds) and torch.equal(default[1], raw)
    else:
        with torch.no_grad():
            other = stained.attend_packed((tokens, cu, lens), dev, stain_idx=0)
        assert not torch.equal(other[1], raw)                                    # (the index is not ignored)
    same = [torch.from_numpy(recipe.uniform((300, ST_D), "attnstain:e%d" % i)) for i in range(3)]
    with torch.no_grad():
        embeds, _ = stained.attend_packed((torch.cat(same).to(dev), torch.from_numpy(cu_of([300] * 3)).to(dev), [300] * 3), dev, stain_idx=m)
        dense = stained({"feats": torch.stack(same).unsqueeze(1)}, dev, train=False, custom_stain_idx=m)
    assert list(dense) == [MODS3[m]]
    assert rel_err(embeds, dense[MODS3[m]].reshape(3, 512)) < 1e-5
    with pytest.raises(IndexError):
        stained.attend_packed((tokens, cu, lens), dev, stain_idx=3)


def test_attention_of_any_stain_with_stain_encoding(dev, stained):
    g = [[300, 40, 260], [257, None, 300]]
    bags = [[None if n is None else torch.from_numpy(recipe.uniform((n, ST_D), "attnstain:s%d%d" % (c, m))) for m, n in enumerate(case)]
            for c, case in enumerate(g)]
    st = DeviceSlideStore(bags, ["a", "b"], MODS3, dev)
    res = st.attention(stained, modality=2, topk=4)
    assert res["cases"].tolist() == [0, 1] and res["lens"] == [260, 300] and res["raw"].shape == (560, 4)
    with torch.no_grad():
        embeds, raw = stained.attend_packed(st.pack_modality([0, 1], 2), dev, stain_idx=2)
    assert torch.equal(res["embeds"], embeds) and torch.equal(res["raw"], raw)
    sd = {k: v.detach().cpu() for k, v in stained.state_dict().items()}
    x = torch.cat([bags[0][2], sd["embedding.weight"][2].expand(260, -1)], dim=-1).unsqueeze(0)
    assert max_rel(res["raw"][:260], R.abmil_embed(x, sd)["raw"].reshape(-1, 4)) < TOL
    one = st.attention(stained, modality=1)                                      # one 40-row bag: the bag-by-bag route
    x = torch.cat([bags[0][1], sd["embedding.weight"][1].expand(40, -1)], dim=-1).unsqueeze(0)
    assert one["cases"].tolist() == [0] and max_rel(one["raw"], R.abmil_embed(x, sd)["raw"].reshape(-1, 4)) < TOL
    with pytest.raises(ValueError, match="stain encoding"):
        st.embed(stained, modality=2)
