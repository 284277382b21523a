"""The patch contributions through the whole stack (MADELEINE.slide_directions / explain_packed, DeviceSlideStore.contributions) on small
models from oracle.restatement.make_params: the conservation law (contributions plus constant equal the probe's decision value), the
fp64 oracle of the token embeddings and the attention contracted with U in fp64, the embeddings against store.embed's, independence of
bags_per_launch and the per-head split.  Bags of 1, 5, 300 and 700 rows: the bag-by-bag and the packed route both run."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from madeleine_amd import functional as MF
from madeleine_amd.store import DeviceSlideStore
from oracle import restatement as R
from tests import _contrib_ref as ref
from tests._util import rel_err

pytestmark = pytest.mark.gpu

MODS = ["HE", "HER2"]
D_IN = 32
LENS = [1, 5, 300, 700]
NC = 3
TOL = 1e-3              # the project's fp32 parity contract (README)
TOL_BF16 = 2.0 ** -7    # one bf16 rounding of any intermediate costs at most 2^-9 of the denominator
CASES = [(H, act, stain) for H in (1, 4) for act in ("softmax", "sigmoid") for stain in (False, True)]
IDS = ["H%d-%s-%s" % (H, act, "stain" if stain else "plain") for H, act, stain in CASES]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy() if t.dtype == torch.float32 else t.detach().cpu().numpy()


def cu_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def probe():
    g = torch.Generator().manual_seed(5)
    return torch.randn(NC, 512, generator=g) / 8, torch.randn(NC, generator=g)


@functools.lru_cache(maxsize=None)
def bags():
    g = torch.Generator().manual_seed(11)
    return [[torch.rand(n, D_IN, generator=g) * 2 - 1 for _ in MODS] for n in LENS]


@functools.lru_cache(maxsize=None)
def setup(H, act, stain):
    """The model, the store, the stain it is asked for and the fp64 oracle of every bag: computed once per case, left unchanged."""
    from madeleine_amd import MADELEINE
    dev = torch.device("cuda:0")
    sd = R.make_params(len(MODS), D_IN, H, stain_encoding=stain, seed=42 + H)
    cfg = SimpleNamespace(MODALITIES=list(MODS), wsi_encoder="abmil", patch_embedding_dim=D_IN, wsi_encoder_hidden_dim=512,
                          activation=act, n_heads=H)
    model = MADELEINE(cfg, stain_encoding=stain)
    model.load_state_dict(sd, strict=True)
    model = model.to(dev).eval()
    store = DeviceSlideStore(bags(), ["case%d" % i for i in range(len(LENS))], MODS, dev)
    modality = 1 if stain else 0
    sd64 = {k: v.double() for k, v in sd.items()}
    W, b = probe()
    U64, const64 = ref.directions(sd64["projector.weight"].numpy(), sd64["projector.bias"].numpy(), W.double().numpy(), b.double().numpy(), H)
    oracle = []
    for case in bags():
        x = case[modality].double()
        if stain:
            x = torch.cat([x, sd64["embedding.weight"][modality].expand(x.shape[0], -1)], dim=-1)
        e = R.pre_attn(x[None], sd64)                                   # [1, n, 512 H], channel j = e H + h
        eh = e.view(1, -1, R.HIDDEN, H)
        att = []
        for h in range(H):
            p = "wsi_embedders.attn.%d." % h
            raw = R.gate_scores(eh[:, :, :, h], sd64[p + "attention_a.0.weight"], sd64[p + "attention_a.0.bias"],
                                sd64[p + "attention_b.0.weight"], sd64[p + "attention_b.0.bias"], sd64[p + "attention_c.weight"],
                                sd64[p + "attention_c.bias"])
            att.append(R.activate(raw, act)[0, :, 0])
        attn = torch.stack(att, 1).numpy()                              # [n, H]
        per_head, total, _, _ = ref.contrib(ref.head_major(e[0].numpy(), H), attn, U64, H)
        total.setflags(write=False)
        oracle.append(total)
    return SimpleNamespace(model=model, store=store, modality=modality, oracle=oracle, const64=const64, H=H)


def run(s, **kw):
    W, b = probe()
    return s.store.contributions(s.model, W, b, modality=s.modality, **kw)


def completeness(res, tol):
    """max over bags and columns of |decision - (stats.sum + const)| / (sum_t |contribution| + |const|), asserted below tol"""
    cu = res["cu_seqlens"].cpu().numpy()
    c = res["contribution"].double().cpu().numpy()
    dec, st, const = res["decision"].double().cpu().numpy(), res["stats"].double().cpu().numpy(), res["const"].double().cpu().numpy()
    worst = 0.0
    for i in range(len(cu) - 1):
        denom = np.abs(c[cu[i]:cu[i + 1]]).sum(0) + np.abs(const)
        gap = np.abs(dec[i] - (st[i, 0] + const))
        worst = max(worst, float((gap / denom).max()))
        assert bool((gap <= tol * denom).all()), (i, gap / denom)
    return worst


@pytest.mark.parametrize("H,act,stain", CASES, ids=IDS)
def test_contributions_add_up_to_the_decision(dev, H, act, stain):
    """The conservation law in both MADELEINE_GEMM modes at 1e-3 and under bf16 autocast at 2^-7; the result's shapes and keys."""
    s = setup(H, act, stain)
    mode = MF.gemm_mode()
    worst = {}
    try:
        for m in ("split", "fp32"):
            MF.set_gemm_mode(m)
            res = run(s)
            worst[m] = completeness(res, TOL)
        MF.set_gemm_mode(mode)
        res = run(s)
        worst["bf16"] = completeness(run(s, precision=torch.bfloat16), TOL_BF16)
    finally:
        MF.set_gemm_mode(mode)
    print("completeness H %d %s %s: %s" % (H, act, "stain" if stain else "plain", ", ".join("%s %.2e" % kv for kv in worst.items())))
    T, n = sum(LENS), len(LENS)
    assert set(res) == {"embeds", "cases", "slide_ids", "cu_seqlens", "lens", "raw", "attention", "contribution", "per_head", "const",
                        "decision", "stats", "top_pos_idx", "top_pos_val", "top_neg_idx", "top_neg_val"}
    assert res["contribution"].shape == (T, NC) and res["raw"].shape == res["attention"].shape == (T, H) and res["per_head"] is None
    assert res["decision"].shape == (n, NC) and res["stats"].shape == (n, 4, NC) and res["const"].shape == (NC,)
    assert res["lens"] == LENS and res["cu_seqlens"].tolist() == cu_of(LENS).tolist() and res["top_pos_idx"] is None
    assert all(res[k].device == dev for k in ("embeds", "raw", "attention", "contribution", "const", "decision", "stats"))
    # decision is embeds . W^T + b, stats are functional.contrib_stats of the contributions, const is the oracle's
    W, b = probe()
    want = res["embeds"].double().cpu() @ W.double().t() + b.double()
    assert rel_err(res["decision"], want) < 1e-5
    assert np.array_equal(bits(res["stats"]), bits(MF.contrib_stats(res["contribution"], res["cu_seqlens"])))
    assert rel_err(res["const"], s.const64) < 1e-5
    assert not s.model.training


@pytest.mark.parametrize("H,act,stain", CASES, ids=IDS)
def test_contributions_against_the_fp64_oracle(dev, H, act, stain):
    """Token embeddings and attention from oracle.restatement in fp64, mapped to head-major order and contracted with U in fp64: the
    device contributions lie within 1e-3 max_t |ref| per bag and column; the embeddings within the 1e-3 contract of store.embed's."""
    s = setup(H, act, stain)
    res = run(s)
    cu = cu_of(LENS)
    c = res["contribution"].double().cpu().numpy()
    worst = 0.0
    for i, want in enumerate(s.oracle):
        err = np.abs(c[cu[i]:cu[i + 1]] - want).max(0)
        scale = np.abs(want).max(0)
        worst = max(worst, float((err / scale).max()))
        assert bool((err <= TOL * scale).all()), (i, err / scale)
    print("oracle H %d %s %s: worst |c - ref| / max_t |ref| %.2e" % (H, act, "stain" if stain else "plain", worst))
    emb = s.store.embed_modality(s.model, s.modality)["embeds"]
    assert rel_err(res["embeds"], emb) < TOL
    att = s.store.attention(s.model, modality=s.modality)
    assert rel_err(res["raw"], att["raw"]) < TOL and rel_err(res["attention"], att["attention"]) < TOL


@pytest.mark.parametrize("H,act,stain", [(4, "softmax", False), (1, "softmax", True), (4, "sigmoid", False)],
                         ids=["H4-softmax-plain", "H1-softmax-stain", "H4-sigmoid-plain"])
def test_contributions_do_not_depend_on_the_grouping(dev, H, act, stain):
    """bags_per_launch in {1, 2, 4}: every tensor of the result bit for bit; per_head sums to the contribution."""
    s = setup(H, act, stain)
    base = run(s, bags_per_launch=1, per_head=True, topk=3)
    for bpl in (2, 4):
        other = run(s, bags_per_launch=bpl, per_head=True, topk=3)
        assert set(other) == set(base)
        for k, v in base.items():
            if torch.is_tensor(v):
                assert v.shape == other[k].shape and np.array_equal(bits(v), bits(other[k])), (bpl, k)
            else:
                assert v == other[k], (bpl, k)
    ph, c = base["per_head"], base["contribution"]
    assert ph.shape == (sum(LENS), H, NC)
    acc = ph[:, 0]
    for h in range(1, H):
        acc = acc + ph[:, h]
    assert np.array_equal(bits(acc), bits(c)), "the heads added in ascending order"
    gap = (ph.double().sum(1) - c.double()).abs()
    assert bool((gap <= (H * MF.HID + 4) * ref.U23 * ph.double().abs().sum(1)).all())
    lean = run(s)
    assert np.array_equal(bits(lean["contribution"]), bits(c)) and lean["per_head"] is None


def test_explain_packed_routes_and_refusals(dev):
    s = setup(4, "softmax", False)
    W, b = probe()
    U, const = s.model.slide_directions(W, b)
    assert U.shape == (NC, 4 * 512) and const.shape == (NC,) and U.is_contiguous() and U.device == dev
    U1, c1 = s.model.slide_directions(W[1], b[1])                        # a [d] row is one column
    assert U1.shape == (1, 2048) and np.array_equal(bits(U1[0]), bits(U[1])) and np.array_equal(bits(c1), bits(const[1:2]))
    p = s.store.pack_modality([2, 3], 0)
    with torch.no_grad():
        out = s.model.explain_packed(p, dev, U)
        heads = s.model.explain_packed((p.tokens, p.cu_seqlens, p.lens), dev, U, per_head=True)
        one = s.model.explain_packed((p.tokens[:300], None, [300]), dev, U)          # one bag: cu_seqlens is built from the lengths
    assert len(out) == 4 and len(heads) == 5 and heads[4].shape == (1000, 4, NC)
    for x, y in zip(out, heads):
        assert np.array_equal(bits(x), bits(y))
    assert out[0].shape == (2, 512) and out[1].shape == out[2].shape == (1000, 4) and out[3].shape == (1000, NC)
    for x, y in zip(one[1:], out[1:]):
        assert np.array_equal(bits(x), bits(y[:300]))
    with pytest.raises(ValueError, match="cu_seqlens"):
        s.model.explain_packed((p.tokens, None, p.lens), dev, U)
    with pytest.raises(ValueError, match=r"U \[C, 2048\]"):
        s.model.explain_packed(p, dev, U[:, :512])
    with pytest.raises(NotImplementedError, match="decision columns"):
        s.store.contributions(s.model, torch.zeros(9, 512))
    with pytest.raises(ValueError, match="512"):
        s.store.contributions(s.model, torch.zeros(3, 128))
