"""The encoder's kernels and the model at 1, 2 and 8 attention heads.  n_heads is a run-time option of the reference (--n_heads, default 4)
and every encoder kernel is templated on it: the pooling kernels run H * 128-thread workgroups with an H-wide LDS tile, the gate kernels map
XCD x to head x % H and to the (x / H)-th of 8 / H interleaved shares of that head's token tiles, the third pre-attention block is 512 * H wide
(its own LayerNorm-GELU-Dropout instantiation) and the token projector / projector contract over 512 * H.  The rest of the suite runs at
H = 4; here:
  - kernels against fp64 on the CPU, with the plan-query assertion, NaN-poisoned workspaces and the bounds of
    tests/test_dispatch_edges_gpu.py (gates, split products) and tests/test_hip_kernels.py / tests/test_bf16_gpu.py (pooling, LayerNorm);
  - the model against tests/golden/heads.npz (captured from the reference at n_heads = 1, 2, 8), under bf16 autocast, on ragged bags, and
    a full step at config-1 geometry against the fp64 oracle.
Each gate / product case is named after the branch it targets; tests/test_dispatch_plan_cpu.py checks the same plans without a GPU."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import recipe
from oracle import restatement as R
from tests._util import MODS5, golden, max_rel, rel_err, t
from tests.test_dispatch_edges_gpu import (BF, EPS_BF16, _bf, _chain_check, _check_gate_fp32, _expect_plan, _gate64, _gate_inputs,
                                           _gate_run, _masks, _mm, _poison, _tn, _u, GATE_NAMES)
from tests.test_model_gpu import _oracle_ragged_step, grads_match

pytestmark = pytest.mark.gpu
TOL = 1e-3
HEADS = [1, 2, 8]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------------------------------- pooling
POOL_LENS = [0, 127, 128, 129, 257, 1]      # empty bag; both sides of POOL_CHUNK = POOL_BWD_TOKENS = 128 and of two chunks


def _cu(lens):
    return torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64)


def _pool64(E, s, lens, softmax=True):
    """fp64 pooling of head-major E [T, H*512] with scores / weights s [T, H] over the bags `lens`: (pooled, leaves E64, s64)."""
    H = s.shape[1]
    E64, s64 = E.double().requires_grad_(), s.double().requires_grad_()
    cu, rows = _cu(lens), []
    for b, L in enumerate(lens):
        if L == 0:
            rows.append(torch.zeros(H * 512, dtype=torch.float64))
            continue
        sl = slice(int(cu[b]), int(cu[b + 1]))
        w = torch.softmax(s64[sl], dim=0) if softmax else s64[sl]
        rows.append(torch.einsum("nh,nhe->he", w, E64[sl].view(L, H, 512)).reshape(-1))
    return torch.stack(rows), E64, s64


def _check_dscores(got, ref):
    """tests/test_hip_kernels.py::test_pool_fwd_bwd_dense's score-gradient bound."""
    assert float((got.double().cpu() - ref).abs().max()) <= 1e-4 * float(ref.abs().max()) + 1e-6, "d_scores"


@pytest.mark.parametrize("H", HEADS)
@pytest.mark.parametrize("form,scale,offset", [("ragged", 4.0, 0.0), ("ragged", 80.0, 0.0), ("dense", 80.0, 0.0), ("ragged", 80.0, 60.0)])
def test_softmax_pool_vs_fp64(dev, H, form, scale, offset):
    """mdl_abmil_pool_fwd / _bwd: ragged bags of 0 / 127 / 128 / 129 / 257 / 1 tokens, and dense bags of 129 tokens; scores of +-4 and +-80
    (the softmax must subtract the running max: exp(80) overflows nothing only then).  offset: head c's scores are shifted by
    +-60 (alternating), so neighbouring heads' score ranges lie 120 apart -- each head must subtract its own running max, another
    head's overflows exp."""
    from madeleine_amd import _native
    from madeleine_amd import functional as MF
    lens = POOL_LENS if form == "ragged" else [129] * 3
    T = sum(lens)
    E = _u((T, H * 512), 10 + H)
    s = _u((T, H), 20 + H, scale) + offset * (1 - 2 * (torch.arange(H) % 2))
    g = _u((len(lens), H * 512), 30 + H)
    ref, E64, s64 = _pool64(E, s, lens)
    ref.backward(g.double())
    Ed, sd = E.to(dev).requires_grad_(), s.to(dev).requires_grad_()
    _poison(dev, _native.lib().mdl_abmil_pool_ws_bytes(len(lens), max(lens), H))
    if form == "ragged":
        out = MF.softmax_pool(Ed, sd, _cu(lens).to(dev), max(lens))
    else:
        out = MF.softmax_pool(Ed.view(3, 129, H * 512), sd.view(3, 129, H))
    out.backward(g.to(dev))
    torch.cuda.synchronize()
    ref = ref.detach()
    assert torch.isfinite(out).all()
    if form == "ragged":
        assert float(out[0].abs().max()) == 0.0
    assert rel_err(out, ref) < 1e-5 and max_rel(out, ref) < TOL
    assert rel_err(Ed.grad, E64.grad) < 1e-5 and max_rel(Ed.grad, E64.grad) < TOL
    _check_dscores(sd.grad, s64.grad)


@pytest.mark.parametrize("H", HEADS)
def test_view_pool_vs_fp64(dev, H):
    """mdl_abmil_pool_view_fwd / _bwd (the n_views = 3 branch, Model.py:419-440): each bag pools the softmax of its scores over a token
    subset of 129 of its 300 tokens; both gradients are accumulated into zeroed buffers."""
    from madeleine_amd import _native
    from madeleine_amd import functional as MF
    nb, N = 3, 300
    idx = torch.randperm(N, generator=torch.Generator().manual_seed(H))[:129]
    E = _u((nb * N, H * 512), 40 + H)
    s = _u((nb * N, H), 50 + H, 4.0)
    g = _u((nb, H * 512), 60 + H)
    E64, s64 = E.double().requires_grad_(), s.double().requires_grad_()
    Ev, sv = E64.view(nb, N, H, 512)[:, idx], s64.view(nb, N, H)[:, idx]
    ref = torch.einsum("bnh,bnhe->bhe", torch.softmax(sv, dim=1), Ev).reshape(nb, -1)
    ref.backward(g.double())
    Ed, sd, ti = E.to(dev), s.to(dev), idx.to(torch.int32).to(dev)
    _poison(dev, _native.lib().mdl_abmil_pool_ws_bytes(nb, idx.numel(), H))
    pooled, m, l_ = MF.pool_view_fwd_raw(Ed, sd, nb, N, ti)
    dE, ds = torch.zeros_like(Ed), torch.zeros_like(sd)
    MF.pool_view_bwd_raw(Ed, sd, pooled, m, l_, g.to(dev), dE, ds, nb, N, ti)
    torch.cuda.synchronize()
    ref = ref.detach()
    assert rel_err(pooled, ref) < 1e-5 and max_rel(pooled, ref) < TOL
    assert rel_err(dE, E64.grad) < 1e-5 and max_rel(dE, E64.grad) < TOL
    _check_dscores(ds, s64.grad)


@pytest.mark.parametrize("H", HEADS)
def test_weighted_pool_vs_fp64(dev, H):
    """mdl_abmil_wpool_* (the relu / leaky_relu / sigmoid activations: weights as they are, negative ones included), ragged with an empty
    bag, forward and both gradients (the bounds of tests/test_hip_kernels.py::test_weighted_pool_no_softmax)."""
    from madeleine_amd import functional as MF
    T = sum(POOL_LENS)
    E = _u((T, H * 512), 70 + H)
    w = torch.nn.functional.leaky_relu(_u((T, H), 80 + H, 2.0))
    g = _u((len(POOL_LENS), H * 512), 90 + H)
    ref, E64, w64 = _pool64(E, w, POOL_LENS, softmax=False)
    ref.backward(g.double())
    Ed, wd = E.to(dev).requires_grad_(), w.to(dev).requires_grad_()
    out = MF.weighted_pool(Ed, wd, _cu(POOL_LENS).to(dev), max(POOL_LENS))
    out.backward(g.to(dev))
    ref = ref.detach()
    assert float(out[0].abs().max()) == 0.0
    assert rel_err(out, ref) < 1e-5 and max_rel(out, ref) < TOL
    assert rel_err(Ed.grad, E64.grad) < 1e-5 and max_rel(Ed.grad, E64.grad) < TOL
    assert rel_err(wd.grad, w64.grad) < 1e-5


@pytest.mark.parametrize("H", HEADS)
def test_pool_from_image_vs_fp64(dev, H):
    """mdl_abmil_pool_fwd_img / mdl_abmil_pool_dscores_img (the split GEMM mode pools from the split image of E): the pooled rows and the
    score gradients against fp64, the softmax statistics equal to those of the fp32-E kernel."""
    from madeleine_amd import _native
    from madeleine_amd import functional as MF
    lens = POOL_LENS
    T, nb, mx = sum(lens), len(lens), max(lens)
    E = _u((T, H * 512), 100 + H, 2.0)
    s = _u((T, H), 110 + H, 80.0)
    g = _u((nb, H * 512), 120 + H)
    ref, E64, s64 = _pool64(E, s, lens)
    ref.backward(g.double())
    Ed, sd, cu, gd = E.to(dev), s.to(dev), _cu(lens).to(dev), g.to(dev)
    Ei = MF.split_image(Ed)
    _poison(dev, _native.lib().mdl_abmil_pool_ws_bytes(nb, mx, H))
    p1, m1, l1 = MF.pool_fwd_img_raw(Ei, sd, nb, 0, cu, mx)
    p0, m0, l0 = MF.pool_fwd_raw(Ed, sd, nb, 0, cu, mx)
    ds = torch.full_like(sd, float("nan"))
    MF.pool_dscores_img_raw(Ei, sd, p1, m1, l1, gd, ds, 0, nb, 0, cu, mx)
    torch.cuda.synchronize()
    ref = ref.detach()
    assert torch.equal(m0, m1) and torch.equal(l0, l1)
    assert rel_err(p1, ref) < 1e-5 and max_rel(p1, ref) < TOL
    _check_dscores(ds, s64.grad)


@pytest.mark.parametrize("H", HEADS)
def test_pool_bf16_vs_fp64(dev, H):
    """The bf16 pooling kernels (bf16 E, fp32 scores and accumulation) against fp64 of the same bf16-representable E: the pooled rows and
    score gradients at the fp32 bounds, dE within one bf16 rounding (tests/test_bf16_gpu.py::test_pool_bf16_vs_fp32_kernel)."""
    from madeleine_amd import _native
    from madeleine_amd import functional as MF
    T = sum(POOL_LENS)
    E = _bf(_u((T, H * 512), 130 + H))
    s = _u((T, H), 140 + H, 4.0)
    g = _u((len(POOL_LENS), H * 512), 150 + H)
    ref, E64, s64 = _pool64(E, s, POOL_LENS)
    ref.backward(g.double())
    Ed, sd = E.to(dev).to(BF).requires_grad_(), s.to(dev).requires_grad_()
    _poison(dev, _native.lib().mdl_abmil_pool_ws_bytes(len(POOL_LENS), max(POOL_LENS), H))
    out = MF.softmax_pool(Ed, sd, _cu(POOL_LENS).to(dev), max(POOL_LENS))
    out.backward(g.to(dev))
    ref = ref.detach()
    assert out.dtype == torch.float32 and float(out[0].abs().max()) == 0.0
    assert rel_err(out, ref) < 1e-5 and max_rel(out, ref) < TOL
    assert rel_err(Ed.grad.float(), E64.grad) < EPS_BF16
    _check_dscores(sd.grad, s64.grad)


# --------------------------------------------------------------------------------------------------------------------------------- gates
# (mode, T, H, p, {product: plan fields}).  T = 2305 is 10 token tiles of 256: at H = 1 spread over 8 shares, at H = 2 over 4 -- uneven
# shares.  At H = 8 each XCD owns one whole head.
GATE_CASES = [
    pytest.param("split", 2305, 1, 0.1, {"gate_split_fwd": dict(persist=0), "gate_split_bwd": dict(splits=1, tps=2336)},
                 id="split-H1_10_tiles_over_8_shares-p0.1"),
    pytest.param("split", 2305, 2, 0.25, {"gate_split_fwd": dict(persist=0), "gate_split_bwd": dict(splits=1, tps=2336)},
                 id="split-H2_10_tiles_over_4_shares-p0.25"),
    pytest.param("split", 4097, 8, 0.25, {"gate_split_fwd": dict(persist=0), "gate_split_bwd": dict(splits=4, tps=1056)},
                 id="split-H8_S4-p0.25"),                                   # dW: S=4, tps=1056, last split 929 tokens
    pytest.param("fp32", 2305, 1, 0.25, {"gate_fp32_bwd": dict(splits=1, tps=2320)}, id="fp32-H1_10_tiles-p0.25"),
    pytest.param("fp32", 2305, 2, 0.1, {"gate_fp32_bwd": dict(splits=1, tps=2320)}, id="fp32-H2_10_tiles-p0.1"),
    pytest.param("fp32", 4097, 8, 0.1, {"gate_fp32_bwd": dict(splits=2, tps=2064)}, id="fp32-H8_S2-p0.1"),
    pytest.param("bf16", 2305, 1, 0.1, {"gate_bf16_fwd": dict(variant=128), "gate_bf16_bwd": dict(variant=128, extra=128, splits=1)},
                 id="bf16-H1_fwd128_dx128-p0.1"),
    pytest.param("bf16", 2305, 2, 0.25, {"gate_bf16_fwd": dict(variant=128), "gate_bf16_bwd": dict(variant=128, extra=128, splits=1)},
                 id="bf16-H2_fwd128_dx128-p0.25"),
    pytest.param("bf16", 8192, 8, 0.25, {"gate_bf16_fwd": dict(variant=256, persist=1),
                                         "gate_bf16_bwd": dict(variant=128, extra=256, splits=4, tps=2048)},
                 id="bf16-H8_fwd256_persistent_dw128_S4-p0.25"),
    pytest.param("bf16", 16384, 8, 0.1, {"gate_bf16_fwd": dict(variant=256, persist=1),
                                         "gate_bf16_bwd": dict(variant=256, extra=256, splits=4, tps=4096)},
                 id="bf16-H8_fwd256_persistent_dw256_S4-p0.1"),
]


@pytest.mark.parametrize("mode,T,H,p,plans", GATE_CASES)
def test_gate_vs_fp64(dev, mode, T, H, p, plans):
    """The gate forward and backward in the three engines -- split (the default GEMM mode), exact fp32 (GEMM mode 'fp32') and bf16 -- with
    the in-kernel dropout RNG, against fp64 with the masks exported by mdl_abmil_gate_dropout_mask."""
    from madeleine_amd import _native
    from madeleine_amd import functional as MF
    for product, want in plans.items():
        _expect_plan(product, T, H, 0, want)
    E, w, ds = _gate_inputs(T, H, 1000 + T + H, bf16=(mode == "bf16"))
    seed = 5151 + T + H
    ka, kb = _masks(dev, T, H, p, seed)
    lib = _native.lib()
    ref = _gate64(E, w, ds, p, ka, kb)
    if mode == "bf16":
        got = _gate_run(dev, E, w, ds, p, seed, BF, lib.mdl_abmil_gate_bwd_bf16_ws_bytes(T, H))
        scale = float(ref[0].abs().max())
        assert float((got[0].double() - ref[0]).abs().max()) < 2 * EPS_BF16 * scale, "scores"
        for i in range(1, 8):
            tol = 5e-3 if GATE_NAMES[i] != "dbc" else 1e-5
            assert rel_err(got[i], ref[i]) < tol, GATE_NAMES[i]
        return
    ws = lib.mdl_abmil_gate_bwd_split_ws_bytes(T, H) if mode == "split" else lib.mdl_abmil_gate_bwd_ws_bytes(T, H)
    old = MF.gemm_mode()
    MF.set_gemm_mode(mode)
    try:
        got = _gate_run(dev, E, w, ds, p, seed, torch.float32, ws)
    finally:
        MF.set_gemm_mode(old)
    _check_gate_fp32(got, ref)


# --------------------------------------------------------------------------------------------------------- LayerNorm-GELU-Dropout, 512 * H
LN_ROWS = 3001          # not a multiple of the 4-row block


def _ln64(x, g, b, keep, p, N):
    import torch.nn.functional as F
    leaves = [v.double().requires_grad_() for v in (x, g, b)]
    ref = F.gelu(F.layer_norm(leaves[0], (N,), leaves[1], leaves[2], 1e-5))
    if keep is not None:
        ref = ref * keep.double() / (1 - p)
    return ref, leaves


@pytest.mark.parametrize("H", [1, 8])
@pytest.mark.parametrize("mode", ["eval", "mask"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_ln_gelu_drop_third_block_width_vs_fp64(dev, H, mode, dtype):
    """mdl_ln_gelu_drop_fwd / _bwd (and the _bf16 pair) at the third block's width 512 * H: W = 512 and W = 4096 (NV 4, WPR 4).
    fp32: tests/test_hip_kernels.py::test_ln_gelu_drop_vs_torch's bounds.  bf16 (bf16-representable x and dy): y elementwise within one
    bf16 rounding of y plus the GELU approximation of the bf16 kernels (|error| <= 2.5e-5 times gamma / (1 - p) <= 1.2 / 0.9: 1e-4 covers
    it with margin), dx within one bf16 rounding; dgamma / dbeta: 5e-4 against the fp32 kernel (tests/test_bf16_gpu.py) plus that kernel's
    1e-4 against fp64."""
    from madeleine_amd import functional as MF
    W, rows = 512 * H, LN_ROWS
    x = _u((rows, W), 200 + H, 3.0) + 0.5
    g, b = 1 + _u((W,), 210 + H, 0.2), _u((W,), 220 + H, 0.3)
    dy = _u((rows, W), 230 + H)
    if dtype == "bf16":
        x, dy = _bf(x), _bf(dy)
    keep = torch.from_numpy(recipe.bernoulli((rows, W), f"hln:k{W}", 0.9)) if mode == "mask" else None
    p = 0.1 if keep is not None else 0.0
    ref, leaves = _ln64(x, g, b, keep, p, W)
    ref.backward(dy.double())
    ref = ref.detach()
    xd = x.to(dev).to(BF if dtype == "bf16" else torch.float32).requires_grad_()
    gd, bd = g.to(dev).requires_grad_(), b.to(dev).requires_grad_()
    out = MF.ln_gelu_drop(xd, gd, bd, 1e-5, p, 0, None if keep is None else keep.to(torch.uint8).to(dev))
    out.backward(dy.to(dev).to(out.dtype))
    out, dx = out.detach().double().cpu(), xd.grad.double().cpu()
    if dtype == "fp32":
        assert rel_err(out, ref) < 1e-5 and max_rel(out, ref) < TOL
        assert rel_err(dx, leaves[0].grad) < 1e-4
        assert rel_err(gd.grad, leaves[1].grad) < 1e-4 and rel_err(bd.grad, leaves[2].grad) < 1e-4
    else:
        assert float(((out - ref).abs() - EPS_BF16 * ref.abs()).max()) < 1e-4
        assert rel_err(out, ref) < EPS_BF16
        assert rel_err(dx, leaves[0].grad) < EPS_BF16
        assert rel_err(gd.grad, leaves[1].grad) < 6e-4 and rel_err(bd.grad, leaves[2].grad) < 6e-4


@pytest.mark.parametrize("H", [1, 8])
@pytest.mark.parametrize("mode", ["eval", "mask"])
def test_preattn_third_block_split_vs_fp64(dev, H, mode):
    """The third pre-attention block as the fused split-engine node (mdl_ln_gelu_drop_{fwd,bwd}_split, image scales from the parameter
    bound) at N = 512 * H: as tests/test_split_gpu.py::test_preattn_block_vs_torch_fp64 -- the decoded image, the fp32 copy and the
    x / W / bias / gamma / beta gradients against fp64 -- plus the elementwise bound of the fp32 LayerNorm kernels on the fp32 copy."""
    import torch.nn.functional as F
    from madeleine_amd import functional as MF
    from tests.test_split_gpu import _decode
    T, K, N = LN_ROWS, 512, 512 * H
    x = _u((T, K), 300 + H, 2.0)
    W = _u((N, K), 310 + H, 0.05)
    lb, g, b = _u((N,), 320 + H, 0.3), 1 + _u((N,), 330 + H, 0.2), _u((N,), 340 + H, 0.3)
    dy = _u((T, N), 350 + H) * torch.logspace(0, -2, T).unsqueeze(1)
    keep = torch.from_numpy(recipe.bernoulli((T, N), f"hpb:k{N}", 0.9)) if mode == "mask" else None
    p = 0.1 if keep is not None else 0.0
    leaves = [v.double().requires_grad_() for v in (x, W, lb, g, b)]
    ref = F.gelu(F.layer_norm(leaves[0] @ leaves[1].t() + leaves[2], (N,), leaves[3], leaves[4], 1e-5))
    if keep is not None:
        ref = ref * keep.double() / (1 - p)
    ref.backward(dy.double())
    ref = ref.detach()
    dl = [v.to(dev).requires_grad_() for v in (x, W, lb, g, b)]
    img, sc, out = MF.preattn_block(dl[0], None, dl[1], dl[2], dl[3], dl[4], 1e-5, p, 0,
                                    None if keep is None else keep.to(torch.uint8).to(dev), True)
    dec = _decode(MF.SplitImage(img.detach(), sc, T, N), T, N)
    assert rel_err(dec, ref) < 1e-5
    bound = float(sc[1])
    assert float(ref.abs().max()) <= bound < 2 ** 9 * float(ref.abs().max()) and 2 ** 13 <= bound * float(sc[0]) < 2 ** 14
    assert rel_err(out, ref) < 1e-5 and max_rel(out, ref) < TOL
    out.backward(dy.to(dev))
    for name, a, r in zip(("x", "W", "lin_bias", "gamma", "beta"), dl, leaves):
        assert rel_err(a.grad, r.grad) < 2e-5, name


# ---------------------------------------------------------------------------------------------------- split products at the H = 8 Linears
SPLIT_T = 4097
TN_CASES = [
    pytest.param(SPLIT_T, 4096, 128, dict(splits=2, tps=2080, empty=0), id="token_projector_dW_Mi4096_N128_S2"),
    pytest.param(SPLIT_T, 512, 4096, dict(splits=2, tps=2080, empty=0), id="third_linear_dW_Mi512_N4096_S2"),
]


@pytest.mark.parametrize("M,N,K", [
    pytest.param(SPLIT_T, 128, 4096, id="token_projector_K4096_N128"),      # the 512 x 128 tile
    pytest.param(SPLIT_T, 512, 4096, id="projector_K4096_N512"),
    pytest.param(SPLIT_T, 4096, 512, id="third_linear_N4096_K512"),
])
def test_split_nt_at_h8_linears_vs_fp64(dev, M, N, K):
    """mdl_split_gemm_nt at the H = 8 Linear shapes (the suite's other split-engine tests stop at K = 2048), with the fp32-chain bound:
    elementwise |error| < 4e-7 sum |a b| and 1e-6 relative."""
    from madeleine_amd import functional as MF
    a, b = _u((M, K), 400 + N + K, 3.0), _u((N, K), 410 + N + K, 0.05)
    out = MF.split_gemm_nt(MF.split_image(a.to(dev)), MF.split_image(b.to(dev)))
    _chain_check(out, _mm(a, b.t()), _mm(a.abs(), b.abs().t()), 4e-7, "Y")


@pytest.mark.parametrize("T,Mi,N,want", TN_CASES)
def test_split_tn_at_h8_linears_vs_fp64(dev, T, Mi, N, want):
    """mdl_split_gemm_tn at the H = 8 dW shapes, with the plan assertion, a NaN-poisoned workspace and the fp32-chain bound."""
    from madeleine_amd import _native
    from madeleine_amd import functional as MF
    _expect_plan("split_tn", T, Mi, N, want)
    x, dy = _u((T, Mi), 420 + Mi, 2.0), _u((T, N), 430 + N, 0.5)
    A, B = MF.split_image(x.to(dev)), MF.split_image(dy.to(dev), pad_rows=32)
    _poison(dev, _native.lib().mdl_split_gemm_tn_ws_bytes(T, Mi, N) + N * Mi * 4)
    out = MF.split_gemm_tn(A, B)
    _chain_check(out, _tn(dy, x), _tn(dy.abs(), x.abs()), 4e-7, "dW")


# --------------------------------------------------------------------------------------------------------------------------------- model
def _cfg(mods, d_in, H):
    return SimpleNamespace(MODALITIES=list(mods), wsi_encoder="abmil", patch_embedding_dim=d_in, wsi_encoder_hidden_dim=512,
                           activation="softmax", n_heads=H)


def _build(mods, d_in, tag, dev, H, stain_encoding=False):
    from madeleine_amd import MADELEINE
    m = MADELEINE(_cfg(mods, d_in, H), stain_encoding=stain_encoding)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert shapes == R.param_shapes(len(mods), d_in, H, stain_encoding)
    sd = {k: torch.from_numpy(v) for k, v in recipe.state_dict_recipe(shapes, tag).items()}
    m.load_state_dict(sd, strict=True)
    return m.to(dev), sd


@pytest.mark.parametrize("H,gemm", [(1, "split"), (2, "split"), (8, "split"), (8, "fp32")])
def test_model_vs_reference_golden(dev, H, gemm):
    """MADELEINE(n_heads = H) against the reference (heads.npz): the train forward, the embedder's slide / raw attention / head interleave,
    the eval and encode_he branches, and one full step (InfoNCE + GOT at T = 0.001) with every parameter gradient -- the bounds of
    tests/test_model_gpu.py (test_encoder_eval_and_grads, test_encoder_other_branches, test_full_step_with_got_golden)."""
    from madeleine_amd import GOT, InfoNCE, calculate_losses
    from madeleine_amd import functional as MF
    g = golden("heads")
    B, M, N, D = (int(x) for x in g["shape"])
    mods = MODS5[:M]
    pre = f"h{H}/"
    feats = t((B, M, N, D), f"hd{H}:feats:{int(g[pre + 'trial'])}")
    labels = torch.from_numpy(g["labels"])
    args = SimpleNamespace(global_loss="info-nce", symmetric_cl=True, local_loss_weight=1.0)
    old = MF.gemm_mode()
    MF.set_gemm_mode(gemm)
    try:
        model, _ = _build(mods, D, f"whd{H}", dev, H)
        model.eval()
        with torch.no_grad():
            embs, toks = model({"feats": feats}, device=dev, train=True)
            for k in mods:
                assert tuple(embs[k].shape) == g[f"{pre}emb/{k}"].shape
                assert rel_err(embs[k], g[f"{pre}emb/{k}"]) < TOL
                assert rel_err(toks[k][:, :3], g[f"{pre}tok_head/{k}"]) < TOL
            bags = feats.view(B * M, N, D).to(dev)
            slide, raw = model.wsi_embedders(bags, return_attention=True)
            assert tuple(slide.shape) == g[pre + "slide"].shape and tuple(raw.shape) == g[pre + "raw"].shape
            assert rel_err(slide, g[pre + "slide"]) < TOL and max_rel(raw, g[pre + "raw"]) < TOL
            _, tokens = model.wsi_embedders(bags, return_preattn_feats=True)
            assert rel_err(tokens[:1, :2], g[pre + "tokens_head"]) < TOL
            assert rel_err(model.encode_he(feats[:, 0], dev), g[pre + "encode_he"]) < TOL
            assert rel_err(model({"feats": feats[:, :1]}, device=dev, train=False)["HE"], g[pre + "eval/HE"]) < TOL
            _, raw_att = model({"feats": feats[:, :1]}, device=dev, train=False, return_attention=True)
            assert max_rel(raw_att, g[pre + "att/raw"]) < TOL
        embs, toks = model({"feats": feats}, device=dev, train=True)
        torch.manual_seed(11)
        loss, flag = calculate_losses(mods[1:], InfoNCE(temperature=0.001), GOT, None, embs, toks, labels[:, 1:], args)
        model.zero_grad()
        loss.backward()
        torch.cuda.synchronize()
    finally:
        MF.set_gemm_mode(old)
    # test_full_step_with_got_golden's 4e-5 on the loss is set at H = 4, where the projector contracts over 2048 channels; at H = 8 it
    # contracts over 4096, and the rounding error of an fp32 contraction grows with its length: twice the bound there.
    assert flag and abs(float(loss.detach()) - float(g[pre + "loss"])) < 4e-5 * max(1, H // 4) * abs(float(g[pre + "loss"]))
    grads_match(g, model, prefix=pre, tol=3e-4)


def test_full_step_autocast_h8_parameter_gradients_vs_oracle_under_autocast(dev):
    """tests/test_bf16_gpu.py::test_full_step_autocast_parameter_gradients_vs_oracle_under_autocast at H = 8 (T = 0.1, where the bound
    bites): every parameter gradient of the HIP bf16 mode is within 2x the error of the oracle run under CPU autocast(bf16), floor 2 bf16
    ulps."""
    from madeleine_amd import InfoNCE, calculate_losses
    H, temperature = 8, 0.1
    mods = MODS5[:3]
    B, M, N, D = 6, 3, 128, 512
    BM = B * M
    feats = t((B, M, N, D), "hbf:grad:feats")
    labels = torch.ones(B, M)
    pre = [torch.from_numpy(recipe.bernoulli((BM, N, w), f"hbf:grad:pre{i}", 0.9)) for i, w in enumerate((512, 512, 512 * H))]
    gate = [(torch.from_numpy(recipe.bernoulli((BM, N, 512), f"hbf:grad:g{c}a", 0.75)),
             torch.from_numpy(recipe.bernoulli((BM, N, 512), f"hbf:grad:g{c}b", 0.75))) for c in range(H)]
    model, sd = _build(mods, D, "hbf8", dev, H)
    model.train()
    model.wsi_embedders._injected_keep = {"pre": [p.to(dev) for p in pre], "gate": [(a.to(dev), b.to(dev)) for a, b in gate]}
    args = SimpleNamespace(global_loss="info-nce", symmetric_cl=True, local_loss_weight=1.0)
    with torch.autocast(device_type="cuda", dtype=BF):
        embs, toks = model({"feats": feats}, device=dev, train=True)
        loss, flag = calculate_losses(mods[1:], InfoNCE(temperature=temperature), None, None, embs, toks, labels[:, 1:], args)
    assert flag and torch.isfinite(loss)
    model.zero_grad()
    loss.backward()

    def oracle(autocast):
        leaves = {k: v.clone().requires_grad_() for k, v in sd.items()}
        with torch.autocast(device_type="cpu", dtype=BF, enabled=autocast):
            l, _, _ = R.pretrain_step_loss(feats, labels, leaves, mods, temperature, True, use_got=False, pre_keep=pre, gate_keep=gate,
                                           n_heads=H)
        l.backward()
        return float(l), {k: v.grad.float() for k, v in leaves.items() if v.grad is not None}

    l_ref, g_ref = oracle(False)
    l_ac, g_ac = oracle(True)
    top = max(float(g.norm()) for g in g_ref.values())
    rows = []
    for k, p in model.named_parameters():
        if k not in g_ref or float(g_ref[k].norm()) < 1e-6 * top:
            continue
        ours = float((p.grad.float().cpu() - g_ref[k]).norm() / g_ref[k].norm())
        refe = float((g_ac[k] - g_ref[k]).norm() / g_ref[k].norm())
        rows.append((k, ours, refe))
    assert len(rows) >= 2 + 12 + 5 * H       # projector, pre_attn, every head (attention_c.bias: zero gradient; no token_projector term)
    assert abs(float(loss) - l_ref) <= max(2.0 * abs(l_ac - l_ref), 2 * EPS_BF16 * abs(l_ref))
    bad = [(k, o, r) for k, o, r in rows if o > max(2.0 * r, 2 * EPS_BF16)]
    assert not bad, bad


def test_forward_ragged_h8_backward_vs_oracle(dev):
    """tests/test_model_gpu.py::test_forward_ragged_unequal_backward_vs_oracle (InfoNCE leg) at H = 8: packed bags of unequal lengths with
    stain encoding, loss and every parameter gradient against the oracle run per bag."""
    from madeleine_amd import InfoNCE, calculate_losses
    H, B, M, D = 8, 4, 2, 768
    mods = MODS5[:M]
    lens = [[300, 1100], [257, 256], [1024, 777], [513, 385]]
    model, _ = _build(mods, D, "hrag8", dev, H, stain_encoding=True)
    model.eval()
    bags = [[t((lens[b][m], D), f"hrag:f{b}{m}") for m in range(M)] for b in range(B)]
    labels = torch.ones(B, M)
    args = SimpleNamespace(global_loss="info-nce", symmetric_cl=True, local_loss_weight=0.5)
    T_ = 0.1
    embs, toks = model.forward_ragged(bags, dev)
    loss, flag = calculate_losses(mods[1:], InfoNCE(temperature=T_), None, None, embs, toks, labels[:, 1:], args)
    assert flag
    model.zero_grad()
    loss.backward()
    sd = {k: v.detach().cpu().clone().requires_grad_() for k, v in model.state_dict().items()}
    ref_loss, _ = _oracle_ragged_step(bags, lens, sd, mods, labels, T_, False, 0.5, n_heads=H)
    ref_loss.backward()
    assert abs(float(loss) - float(ref_loss)) < 1e-4 * abs(float(ref_loss)), (float(loss), float(ref_loss))
    top = max(float(v.grad.norm()) for v in sd.values() if v.grad is not None)
    for k, p in model.named_parameters():
        got = p.grad.cpu() if p.grad is not None else torch.zeros(p.shape)
        ref = sd[k].grad if sd[k].grad is not None else torch.zeros_like(got)
        assert float((got - ref).norm()) <= TOL * float(ref.norm()) + 1e-5 * top, k
    assert float(sd["embedding.weight"].grad.norm()) > 1e-4 * top


@pytest.mark.parametrize("H", [1, 2, 4, 8])
def test_config1_full_step_vs_fp64_oracle(dev, H):
    """A full step at config-1 geometry (BASELINE.json configs[0]: 4 slides x 2 stains x 256 patches x 512-d, ABMIL + global InfoNCE) in
    the default GEMM mode against the fp64 oracle: loss, slide embeddings and every parameter gradient (the bounds of
    tests/test_model_gpu.py::test_any_patch_embedding_dim_vs_oracle)."""
    from madeleine_amd import InfoNCE, calculate_losses
    mods = MODS5[:2]
    B, M, N, D = 4, 2, 256, 512
    temperature = 0.01
    model, sd = _build(mods, D, f"c1h{H}", dev, H)
    model.eval()
    feats = t((B, M, N, D), f"c1h{H}:feats")
    labels = torch.ones(B, M)
    args = SimpleNamespace(global_loss="info-nce", symmetric_cl=True, local_loss_weight=1.0)
    embs, toks = model({"feats": feats}, device=dev, train=True)
    loss, flag = calculate_losses(mods[1:], InfoNCE(temperature=temperature), None, None, embs, toks, labels[:, 1:], args)
    model.zero_grad()
    loss.backward()
    sd64 = {k: v.double().requires_grad_() for k, v in sd.items()}
    ref_loss, _, ref_embs = R.pretrain_step_loss(feats.double(), labels, sd64, mods, temperature, True, use_got=False, n_heads=H)
    ref_loss.backward()
    assert flag and abs(float(loss) - float(ref_loss)) < TOL * abs(float(ref_loss))
    for m in mods:
        assert rel_err(embs[m], ref_embs[m]) < TOL
    top = max(float(v.grad.norm()) for v in sd64.values() if v.grad is not None)
    for k, p in model.named_parameters():
        ref = sd64[k].grad
        if ref is None:                  # token_projector: no local loss
            continue
        assert p.grad is not None and p.grad.shape == ref.shape, k
        assert float((p.grad.cpu().double() - ref).norm()) <= TOL * float(ref.norm()) + 1e-5 * top, k
