"""DeviceSlideStore.contributions(topk=...) and contribution_maps on a 4-case store with coordinates: the top patches against a numpy
sort of the returned contributions, the signed normalisation of the map values, the images against heatmap.render called directly on
those values, and a zero probe, which renders every covered pixel at the midpoint level."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from madeleine_amd import heatmap as HM
from madeleine_amd.store import DeviceSlideStore
from oracle import restatement as R
from tests import _contrib_ref as ref

pytestmark = pytest.mark.gpu

MODS = ["HE", "HER2"]
D_IN = 32
LENS = [[1, None], [5, 40], [300, 7], [700, 260]]
PS = 64
NC = 3
MID = 32768             # the quantiser's level of 0.5: rint(0.5 * 65535), half to even


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _coords():
    """A jittered grid with half overlap, 25 patches a row."""
    rng = np.random.default_rng(3)
    return [[None if n is None else np.stack([(np.arange(n) % 25) * (PS // 2) + 64, (np.arange(n) // 25) * (PS // 2) + 128], 1)
             + rng.integers(0, 5, (n, 2)) for n in case] for case in LENS]


@pytest.fixture(scope="module")
def env(dev):
    from madeleine_amd import MADELEINE
    g = torch.Generator().manual_seed(23)
    bags = [[None if n is None else torch.rand(n, D_IN, generator=g) * 2 - 1 for n in case] for case in LENS]
    store = DeviceSlideStore(bags, ["case%d" % i for i in range(len(LENS))], MODS, dev, coords=_coords(), patch_size=PS)
    cfg = SimpleNamespace(MODALITIES=list(MODS), wsi_encoder="abmil", patch_embedding_dim=D_IN, wsi_encoder_hidden_dim=512,
                          activation="softmax", n_heads=4)
    model = MADELEINE(cfg)
    model.load_state_dict(R.make_params(len(MODS), D_IN, 4, seed=7), strict=True)
    W, b = torch.randn(NC, 512, generator=g) / 8, torch.randn(NC, generator=g)
    return SimpleNamespace(store=store, model=model.to(dev).eval(), W=W, b=b)


def _same_images(a, b):
    assert a["canvas"] == b["canvas"] and len(a["rgba"]) == len(b["rgba"]) and a["downsample"] == b["downsample"]
    for k in ("level", "covered", "rgba"):
        for x, y in zip(a[k], b[k]):
            assert x.shape == y.shape and torch.equal(x.view(torch.uint8), y.view(torch.uint8)), k


@pytest.mark.parametrize("modality", [0, 1])
def test_topk_is_a_sort_of_the_contributions(dev, env, modality):
    """The k most positive and the k most negative rows per bag and column equal a stable numpy sort of the returned contributions
    (ties: the lower row), with their values; a bag shorter than k is padded with -1 and -inf / +inf."""
    res = env.store.contributions(env.model, env.W, env.b, modality=modality, topk=3)
    n = len(res["lens"])
    cu = res["cu_seqlens"].cpu().numpy()
    c = res["contribution"].cpu().numpy()
    pi, pv, ni, nv = ref.topk(c, cu, 3)
    for k in ("top_pos_idx", "top_neg_idx"):
        assert res[k].shape == (n, NC, 3) and res[k].dtype == torch.int32 and res[k].device == dev
    assert np.array_equal(res["top_pos_idx"].cpu().numpy(), pi) and np.array_equal(res["top_neg_idx"].cpu().numpy(), ni)
    assert np.array_equal(res["top_pos_val"].cpu().numpy(), pv) and np.array_equal(res["top_neg_val"].cpu().numpy(), nv)
    short = res["lens"].index(min(res["lens"]))
    if res["lens"][short] < 3:
        assert res["top_pos_idx"][short, :, res["lens"][short]:].eq(-1).all() and res["top_neg_idx"][short, :, res["lens"][short]:].eq(-1).all()
    for k in (1, 8):                                                   # another k: the head of the same order
        other = env.store.contributions(env.model, env.W, env.b, modality=modality, topk=k)
        pk = ref.topk(c, cu, k)
        assert np.array_equal(other["top_pos_idx"].cpu().numpy(), pk[0]) and np.array_equal(other["top_neg_idx"].cpu().numpy(), pk[2])
    # a zero probe: every contribution is zero, so every row ties and the lower rows win on both sides
    zero = env.store.contributions(env.model, torch.zeros(5, 512), modality=modality, topk=2)      # five columns: blocks of 4 and 1
    assert not bool(zero["contribution"].any()) and not bool(zero["stats"].any()) and not bool(zero["decision"].any())
    zi = ref.topk(zero["contribution"].cpu().numpy(), cu, 2)
    assert np.array_equal(zero["top_pos_idx"].cpu().numpy(), zi[0]) and np.array_equal(zero["top_neg_idx"].cpu().numpy(), zi[2])
    assert zero["top_pos_idx"].shape == (n, 5, 2) and zero["top_pos_idx"][-1, :, :].tolist() == [[0, 1]] * 5


def test_contribution_maps_are_render_of_the_signed_values(dev, env):
    st, model = env.store, env.model
    res = st.contribution_maps(model, env.W, env.b, downsample=16, sigma=2.0, crop=True)
    con = st.contributions(model, env.W, env.b)
    n = len(LENS)
    assert res["cases"].tolist() == list(range(n)) and res["slide_ids"] == ["case%d" % i for i in range(n)]
    for k in ("embeds", "const", "decision", "stats", "cu_seqlens"):
        assert torch.equal(res[k], con[k]), k
    cu = con["cu_seqlens"].cpu().numpy()
    # the values: 0.5 + 0.5 c / max_t |c| per bag and column; one fp32 rounding of the quotient is all the device may differ by
    want = ref.signed_values(con["contribution"].cpu().numpy(), cu)
    values = res["values"]
    assert values.shape == (sum(con["lens"]), NC) and values.dtype == torch.float32
    assert float(np.abs(values.cpu().numpy().astype(np.float64) - want).max()) <= 2.0 ** -23
    for i in range(n):                                                 # the strongest patch of a bag reaches one end of the map
        seg = values[cu[i]:cu[i + 1]]
        assert bool(((seg.min(0).values == 0.0) | (seg.max(0).values == 1.0)).all()) and float(seg.min()) >= 0.0 and float(seg.max()) <= 1.0
    # the images: heatmap.render called directly on those values
    xy = st.coords_of(None, 0)
    by_hand = HM.render(xy, con["cu_seqlens"], values, PS, 16, sigma=2.0, cmap="coolwarm", crop=True)
    _same_images(res, by_hand)
    assert all(r.shape[0] == NC and r.shape[3] == 4 for r in res["rgba"])
    # columns, the second stain, grouping and the byte budget change nothing else
    some = st.contribution_maps(model, env.W, env.b, columns=[2, 0], downsample=16, sigma=2.0, crop=True)
    assert torch.equal(some["values"], values[:, [2, 0]])
    for b in range(n):
        assert torch.equal(some["rgba"][b], res["rgba"][b][[2, 0]])
        assert torch.equal(some["level"][b].to(torch.int32), res["level"][b].to(torch.int32)[[2, 0]])      # (uint16 cannot be indexed)
    _same_images(st.contribution_maps(model, env.W, env.b, downsample=16, sigma=2.0, crop=True, bags_per_launch=1, max_bytes=1 << 16), res)
    second = st.contribution_maps(model, env.W[1], env.b[1], modality=1)
    assert second["cases"].tolist() == [1, 2, 3] and second["values"].shape == (307, 1) and second["downsample"] == PS
    with pytest.raises(IndexError, match="columns"):
        st.contribution_maps(model, env.W, env.b, columns=[3])
    with pytest.raises(RuntimeError, match="no coordinates"):
        DeviceSlideStore([[torch.ones(3, D_IN), None]], ["a"], MODS, dev).contribution_maps(model, env.W)


@pytest.mark.parametrize("sigma", [0.0, 1.5])
def test_a_zero_probe_renders_the_midpoint(dev, env, sigma):
    """W = 0: no patch carries evidence, every value is 0.5 and every covered pixel is at the quantiser's midpoint level."""
    res = env.store.contribution_maps(env.model, torch.zeros(2, 512), sigma=sigma)
    assert bool((res["values"] == 0.5).all()) and res["values"].shape[1] == 2
    covered = 0
    for level, cov in zip(res["level"], res["covered"]):
        level = level.to(torch.int32)                                  # (uint16 tensors cannot be indexed)
        assert bool((level[cov.bool()] == MID).all()) and bool((level[~cov.bool()] == 0).all())
        covered += int(cov.sum())
    assert covered > 0
    by_hand = HM.render(env.store.coords_of(None, 0), res["cu_seqlens"], torch.full_like(res["values"], 0.5), PS, sigma=sigma,
                        cmap="coolwarm")
    _same_images(res, by_hand)
    lut = HM.colormap("coolwarm")
    mid = (MID * 255 + 32767) // 65535
    rgba, cov = res["rgba"][-1][0], res["covered"][-1][0].bool()
    assert torch.equal(rgba[cov][:, :3].cpu(), lut[mid, :3].expand(int(cov.sum()), 3))
