"""The device smooth rank (R1) on the GPU: every test matrix against the fp64 oracle under the derived tolerances, the shapes at which
the kernels take another path, the bit contract (stride, scale, repetition), no host synchronisation, degenerate values, and the
opt-in wiring of the store, run_inference and train_loop."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from madeleine_amd import functional as MF
from oracle import recipe
from tests import _rank_ref as RR

pytestmark = pytest.mark.gpu

ROWS, TILE, MAX_CHUNKS, TRI_ROWS = MF.RANK_GRAM_ROWS, MF.RANK_GRAM_TILE, MF.RANK_GRAM_MAX_CHUNKS, MF.RANK_TRI_ROWS


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def run(E):
    """(exp(H), H, sigma) on the host from one call on device tensor E."""
    out, sigma = MF._rank_call(E, RR.EPS)
    return float(out[0]), float(out[1]), sigma.cpu().numpy()


def check(E_np, dev, tol, label):
    """One matrix against the oracle: rank to tol relative, sigma^2 to SIGMA_TOL sigma_max^2, sigma descending and >= 0, H = ln rank."""
    rank, H, sigma = run(torch.from_numpy(np.array(E_np)).to(dev))      # a writable, contiguous copy
    return check_result(E_np, rank, H, sigma, tol, label)


def check_result(E_np, rank, H, sigma, tol, label):
    """The bounds of check() on the results (exp(H), H, sigma) of one call on E_np."""
    want, S = RR.oracle(E_np)
    dev_rank = abs(rank - want) / want
    dev_sigma = float(np.abs(sigma ** 2 - S ** 2).max() / S.max() ** 2)
    print("%s: oracle %.6f device %.6f rel. dev. %.2e, sigma^2 dev. %.2e" % (label, want, rank, dev_rank, dev_sigma))
    assert sigma.shape == S.shape and sigma.dtype == np.float64
    assert dev_rank <= tol, (label, dev_rank)
    assert dev_sigma <= RR.SIGMA_TOL, (label, dev_sigma)
    assert bool((sigma[:-1] >= sigma[1:]).all()) and bool((sigma >= 0).all())
    assert abs(H - math.log(rank)) <= 1e-12 * max(1.0, abs(H))
    return rank, sigma


@pytest.mark.parametrize("name", list(RR.CASES))
def test_table_against_the_fp64_oracle(dev, name):
    E, want, S = RR.case(name)
    out, sigma = MF.smooth_rank(torch.from_numpy(E.copy()).to(dev), RR.EPS)
    assert out.dim() == 0 and out.dtype == torch.float64 and out.device == dev and sigma.dtype == torch.float64 and sigma.device == dev
    check(E, dev, RR.RANK_TOL[RR.CASES[name][0]], name)


# n = 1, 2, 3: no, no and one tridiagonalisation step.  d = 64 with n = d - 1, d, d + 1: both sides of the E^T E / E E^T switch.  Rows
# around the Gram chunk (ROWS) and one past MAX_CHUNKS chunks of it (longer chunks), on either side of the switch; k around the Gram tile
# (TILE) and the row block of the tridiagonalisation (TRI_ROWS); d = 77, no multiple of either; k = 1024, the limit.
EDGES = [(1, 64), (2, 64), (3, 64), (64, 1), (64, 3),
         (63, 64), (64, 64), (65, 64),
         (ROWS - 1, 40), (ROWS, 40), (ROWS + 1, 40), (40, ROWS - 1), (40, ROWS), (40, ROWS + 1),
         (MAX_CHUNKS * ROWS, 24), (MAX_CHUNKS * ROWS + 1, 24), (24, MAX_CHUNKS * ROWS + 17),
         (100, TILE - 1), (100, TILE + 1), (TILE + 1, 100), (2 * TILE + 1, 2 * TILE + 1),
         (90, TRI_ROWS + 1), (90, TRI_ROWS + 2), (90, TRI_ROWS + 3),
         (200, 77), (1024, 1030)]


@pytest.mark.parametrize("n,d", EDGES, ids=["%dx%d" % e for e in EDGES])
def test_shape_edges(dev, n, d):
    assert (ROWS, TILE, MAX_CHUNKS, TRI_ROWS) == (512, 64, 16, 16)      # the kernels' constants the list above is built from
    check(RR.gauss(n, d, 100 + n + d), dev, RR.RANK_TOL[RR.FULL], "gauss %dx%d" % (n, d))


@pytest.mark.parametrize("n,d", [(300, 72), (40, 200), (1, 8)])
def test_row_stride_keeps_the_bits(dev, n, d):
    """A column slice of a wider buffer (ldE = d + 24) gives the bits of the contiguous call."""
    wide = torch.from_numpy(RR.gauss(n, d + 24, 7)).to(dev)
    E = wide[:, :d]
    assert not E.is_contiguous() or n == 1
    out_s, sig_s = MF._rank_call(E, RR.EPS)
    out_c, sig_c = MF._rank_call(E.contiguous(), RR.EPS)
    assert torch.equal(out_s, out_c) and torch.equal(sig_s, sig_c)
    check(E.cpu().numpy(), dev, RR.RANK_TOL[RR.FULL], "slice %dx%d" % (n, d))


def test_power_of_two_scale(dev):
    """E 2^12 and E 2^-12: powers of two are exact, so sigma scales exactly and the rank stays to 1e-12."""
    E = torch.from_numpy(RR.gauss(300, 96, 21)).to(dev)
    out, sigma = MF._rank_call(E, RR.EPS)
    for s in (2.0 ** 12, 2.0 ** -12):
        out_s, sigma_s = MF._rank_call(E * s, RR.EPS)
        assert torch.equal(sigma_s, sigma * s)
        assert abs(float(out_s[0]) - float(out[0])) <= 1e-12 * float(out[0])


def test_two_calls_same_bits(dev):
    E = torch.from_numpy(RR.case("gauss_1153x512")[0].copy()).to(dev)
    a, b = MF._rank_call(E, RR.EPS), MF._rank_call(E, RR.EPS)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_no_host_synchronisation(dev):
    E = torch.from_numpy(RR.gauss(300, 96, 22)).to(dev)
    want = MF.smooth_rank(E)                 # warm-up: library load, allocator
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = MF.smooth_rank(E)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_all_zero_matrix_is_nan(dev):
    out, sigma = MF._rank_call(torch.zeros(50, 64, device=dev), RR.EPS)
    assert bool(torch.isnan(out).all()) and not bool(sigma.any())


@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_non_finite_input_returns_nan(dev, value):
    E = RR.case("gauss_512x512")[0].copy()
    E[317, 101] = value
    out, sigma = MF._rank_call(torch.from_numpy(E).to(dev), RR.EPS)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# ------------------------------------------------------------------------------------------------ wiring
MODS = ["HE", "HER2"]
D_IN = 64
STORE_SEED, TRAIN_SEED = 1, 1          # seeds at which the asserted distance holds (rounded_oracle)
DEFICIENT_TOL = RR.RANK_TOL[RR.DEFICIENT]


def _model(dev, mods, tag, projector_bias=0.0):
    """Recipe weights; projector_bias is added to the bias of the last Linear (a common component of every slide embedding)."""
    from madeleine_amd import MADELEINE
    cfg = SimpleNamespace(MODALITIES=mods, wsi_encoder="abmil", patch_embedding_dim=D_IN, wsi_encoder_hidden_dim=512,
                          activation="softmax", n_heads=4)
    m = MADELEINE(cfg)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    sd = {k: torch.from_numpy(v) for k, v in recipe.state_dict_recipe(shapes, tag).items()}
    sd["projector.bias"] = sd["projector.bias"] + projector_bias
    m.load_state_dict(sd, strict=True)
    return m.to(dev)


# The wiring tests compare ROUNDED ranks, after asserting that the oracle lies more than 2.6e-3 * value from a rounding boundary.  A
# boundary is never further than 0.005 away, so that can only hold for a rank below 1.92: every patch is one common vector plus
# SPREAD * noise, which keeps the slide embeddings close to collinear (and is the harder, nearly rank-deficient kind of input).
# In train mode the dropout noise alone spreads the twelve embeddings of an epoch to a rank of 2.5 .. 2.9, so the train_loop test also
# raises the bias of the model's last Linear by TRAIN_BIAS.
SPREAD = 0.2
TRAIN_BIAS = 4.0


def _patches(shape, g, common):
    return common + SPREAD * torch.randn(*shape, D_IN, generator=g)


def _bags(seed):
    """12 H&E bags of 64 .. 300 rows."""
    g = torch.Generator().manual_seed(seed)
    common = torch.randn(D_IN, generator=g)
    lens = torch.randint(64, 301, (12,), generator=g).tolist()
    return [_patches((n,), g, common) for n in lens]


def _train_batches(seed, B=4, M=2, N=64):
    """3 batches of 4 cases x 2 stains x 64 patches."""
    g = torch.Generator().manual_seed(seed)
    common = torch.randn(D_IN, generator=g)
    return [{"feats": _patches((B, M, N), g, common), "modality_labels": torch.ones(B, M),
             "slide_ids": [str(j) for j in range(B)]} for _ in range(3)]


def rounded_oracle(embeds):
    """round(oracle, 2), after asserting that the oracle lies further from a rounding boundary than the widest tolerance of the kernels
    (2.6e-3 relative): the rounded value then cannot depend on which side of the tolerance the device lands."""
    want, _ = RR.oracle(embeds)
    to_boundary = abs((want * 100.0) % 1.0 - 0.5) / 100.0          # boundaries lie at (m + 0.5) / 100
    print("oracle %.6f, distance to a rounding boundary %.2e, needed %.2e" % (want, to_boundary, DEFICIENT_TOL * want))
    assert to_boundary > DEFICIENT_TOL * want, (want, to_boundary)
    return round(want, 2)


def test_store_embed_and_run_inference_rank(dev):
    from madeleine_amd import DeviceSlideStore, run_inference
    import madeleine_amd.utils as U
    bags = _bags(STORE_SEED)
    st = DeviceSlideStore([[b] for b in bags], ["s%d" % i for i in range(12)], ["HE"], dev)
    model = _model(dev, MODS, "rank").eval()
    plain = st.embed(model)
    assert "rank" not in plain
    res = st.embed(model, rank=True)
    assert torch.equal(res["embeds"], plain["embeds"]) and isinstance(res["rank"], float)
    want = rounded_oracle(res["embeds"].cpu().numpy())
    assert res["rank"] == want
    mean = st.mean_embeddings(rank=True)
    assert mean["rank"] == round(float(MF.smooth_rank(mean["embeds"])[0]), 2) and "rank" not in st.mean_embeddings()
    U.DEVICE = dev
    loader = [(b[None], ["s%d" % i]) for i, b in enumerate(bags)]
    out_dev, rank_dev = run_inference(model, loader, config=SimpleNamespace(precision="float32"), device_rank=True)
    out_cpu, rank_cpu = run_inference(model, loader, config=SimpleNamespace(precision="float32"))
    assert np.array_equal(out_dev["embeds"], out_cpu["embeds"]) and np.array_equal(out_dev["embeds"], res["embeds"].cpu().numpy())
    assert rank_dev == want and isinstance(rank_dev, float)
    assert rank_cpu == U.smooth_rank_measure(torch.Tensor(out_cpu["embeds"]))      # the default is the host function, as before


def test_train_loop_device_rank(dev, capsys, monkeypatch):
    """args.device_rank against the default path from the same weights, batches and seeds: the same printed text, a bit-equal epoch
    loss, and the rank = round(oracle of the epoch's embeddings, 2)."""
    import madeleine_amd.trainer as TR
    from madeleine_amd import InfoNCE, train_loop
    monkeypatch.setattr(TR, "DEVICE", dev)
    B = 4
    batches = _train_batches(TRAIN_SEED)
    seen = []
    host_rank = TR.smooth_rank_measure

    def recording(E, *a, **kw):
        seen.append(E.detach().cpu().numpy().copy())
        return host_rank(E, *a, **kw)

    monkeypatch.setattr(TR, "smooth_rank_measure", recording)
    results = []
    for device_rank in (False, True):
        model = _model(dev, MODS, "rank-train", TRAIN_BIAS)
        args = SimpleNamespace(STAINS=MODS[1:], precision="float32", warmup_epochs=0, global_loss="info-nce", symmetric_cl=True,
                               local_loss_weight=1.0)
        if device_rank:
            args.device_rank = True
        opt = torch.optim.AdamW(model.parameters(), lr=1e-4)
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda step: 1.0)
        torch.manual_seed(5)
        capsys.readouterr()
        loss, rank = train_loop(args, InfoNCE(temperature=0.1), None, None, model, 0, batches, opt, sched, sched)
        results.append((loss, rank, capsys.readouterr().out))
    (loss_host, rank_host, text_host), (loss_dev, rank_dev, text_dev) = results
    assert len(seen) == 1 and seen[0].shape == (3 * B, 512)          # the device path never called the host function
    assert text_dev == text_host and "Loss for batch: 0" in text_host
    assert loss_dev == loss_host and math.isfinite(loss_host)
    want = rounded_oracle(seen[0])
    assert rank_dev == want and isinstance(rank_dev, float) and isinstance(rank_host, float)
