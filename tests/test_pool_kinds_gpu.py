"""One pooling kernel family, one bag-selection record (csrc/abmil_pool.hip): the same bags named four ways -- dense, packed with
cu_seqlens, a dense token-index view, ragged views -- pool to the same bits, forward and backward; and a packed batch whose lengths
sit on both sides of every chunk boundary (whole bags and their ragged half-bag views) matches the fp64 reference within the bounds of
test_hip_kernels.py::test_pool_fwd_bwd_dense.  E holds bf16-representable values, so that the fp32 and the bf16 kernels share one
reference."""
import functools
import itertools

import pytest
import torch

from tests._util import max_rel, rel_err, t

pytestmark = pytest.mark.gpu
TOL = 1e-3
EPS_BF16 = 2.0 ** -8        # a dE stored as bf16 is the fp32 value rounded once to an 8-bit significand: unit roundoff 2^-8
HID = 512


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _inputs(lens, H, tag):
    T = sum(lens)
    E = t((T, H * HID), "kinds:E" + tag).to(torch.bfloat16).float()
    s = t((T, H), "kinds:s" + tag) * 6
    return E, s


# ------------------------------------------------------------------------------------------------ the four kinds agree
B, N = 3, 137       # one full 128-token chunk and a 9-token tail: one row more than the forward keeps in flight (MDL_POOL_U = 8)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("H", [1, 4])
def test_four_ways_to_name_the_same_bags_pool_to_the_same_bits(dev, H, bf16):
    from madeleine_amd import functional as MF
    E, s = _inputs([N] * B, H, "same%d" % H)
    E, s = E.to(dev, torch.bfloat16 if bf16 else torch.float32), s.to(dev)
    dp = t((B, H * HID), "kinds:dp%d" % H).to(dev)
    cu = torch.arange(B + 1, dtype=torch.int64, device=dev) * N
    idx = torch.arange(N, dtype=torch.int32, device=dev)
    perm = torch.arange(B * N, dtype=torch.int32, device=dev)
    vcu = torch.tensor([0, N, N, 2 * N, 2 * N, 3 * N, 3 * N], dtype=torch.int64, device=dev)    # segment 2k = bag k, segment 2k + 1 is empty

    fwd = {
        "dense": MF.pool_fwd_raw(E, s, B, N, None, N),
        "packed": MF.pool_fwd_raw(E, s, B, 0, cu, N),
        "view": MF.pool_view_fwd_raw(E, s, B, N, idx),
    }
    rp, rm, rl = MF.pool_rview_fwd_raw(E, s, B, perm, vcu, N)
    assert float(rp[:, 1].abs().max()) == 0.0, "an empty segment pools to exact zeros"
    fwd["rview"] = (rp[:, 0].contiguous(), rm[0::2].contiguous(), rl[0::2].contiguous())
    for kind, out in fwd.items():
        for name, a, b in zip(("pooled", "stat_m", "stat_l"), out, fwd["dense"]):
            print("fwd %s %s: max |diff| vs dense %.3e" % (kind, name, float((a - b).abs().max())))
    for kind, out in fwd.items():
        for name, a, b in zip(("pooled", "stat_m", "stat_l"), out, fwd["dense"]):
            assert torch.equal(a, b), (kind, name)

    def grads(fill):
        return torch.full_like(E, fill), torch.full_like(s, fill)
    pooled, m, l = fwd["dense"]
    bwd = {}
    for kind, c in (("dense", None), ("packed", cu)):           # overwrite (accumulate = 0) whatever the outputs held
        dE, ds = grads(float("nan"))
        MF.pool_bwd_raw(E, s, pooled, m, l, dp, dE, 0, ds, 0, B, N if c is None else 0, c, N)
        bwd[kind] = (dE, ds)
    dE, ds = grads(0.0)                                         # the view backwards accumulate
    MF.pool_view_bwd_raw(E, s, pooled, m, l, dp, dE, ds, B, N, idx)
    bwd["view"] = (dE, ds)
    dE, ds = grads(0.0)
    dp2 = torch.stack([dp, t((B, H * HID), "kinds:dp2%d" % H).to(dev)], dim=1).contiguous()     # the empty segments' gradient goes nowhere
    MF.pool_rview_bwd_raw(E, s, rp, rm, rl, dp2, dE, ds, B, perm, vcu, N)
    bwd["rview"] = (dE, ds)
    for kind, out in bwd.items():
        for name, a, b in zip(("dE", "d_scores"), out, bwd["dense"]):
            print("bwd %s %s: max |diff| vs dense %.3e" % (kind, name, float((a.float() - b.float()).abs().max())))
    for kind, out in bwd.items():
        for name, a, b in zip(("dE", "d_scores"), out, bwd["dense"]):
            assert torch.equal(a, b), (kind, name)


# ------------------------------------------------------------------------------------------------ against the fp64 reference
LENS = [1, 7, 128, 129, 1100]       # 1100: 9 chunks, pool_combine's 8-wide loop and its tail; 1: a bag whose first half-view is empty


def _halves(lens):
    """(perm, vcu): every bag's rows shuffled in place; segment 2k is the first len // 2 of them, segment 2k + 1 the rest."""
    g = torch.Generator().manual_seed(7)
    perm, vcu, base = [], [0], 0
    for n in lens:
        perm.append(base + torch.randperm(n, generator=g))
        vcu += [base + n // 2, base + n]
        base += n
    return torch.cat(perm).to(torch.int32), torch.tensor(vcu, dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def _reference(H):
    """fp64: (pooled [5, H*512], views [5, 2, H*512], dE, d_scores of the whole bags, dE, d_scores of the views)."""
    E32, s32 = _inputs(LENS, H, "ref%d" % H)
    perm, vcu = _halves(LENS)
    g = t((len(LENS), 3, H * HID), "kinds:g%d" % H).double()
    out = []
    for which in ("bags", "views"):
        E, s = E32.double().requires_grad_(), s32.double().requires_grad_()
        rows, base = [], 0
        for k, n in enumerate(LENS):
            sets = [torch.arange(base, base + n)] if which == "bags" else [perm[vcu[2 * k + v]:vcu[2 * k + v + 1]].long() for v in (0, 1)]
            for r in sets:
                w = torch.softmax(s[r], dim=0)
                rows.append(torch.einsum("nh,nhe->he", w, E[r].view(len(r), H, HID)).reshape(-1) if len(r) else torch.zeros(H * HID).double())
            base += n
        p = torch.stack(rows).view(len(LENS), -1, H * HID)
        p.backward(g[:, :1] if which == "bags" else g[:, 1:])
        out.append((p.detach(), E.grad, s.grad))
    return out


def _check(tag, pooled, dE, ds, ref, bf16):
    rp, rE, rs = ref
    figures = (rel_err(pooled, rp), max_rel(pooled, rp), rel_err(dE.float(), rE), max_rel(dE.float(), rE),
               float((ds.double().cpu() - rs).abs().max()), float(rs.abs().max()))
    print("%s: pooled rel %.2e max_rel %.2e, dE rel %.2e max_rel %.2e, d_scores max |diff| %.2e of %.2e" % ((tag,) + figures))
    assert figures[0] < 1e-5 and figures[1] < TOL
    # a bf16 dE is the same fp32 value rounded once on its way out: the bounds of the fp32 dE plus that rounding
    assert figures[2] < 1e-5 + (EPS_BF16 if bf16 else 0.0) and figures[3] < TOL + (EPS_BF16 if bf16 else 0.0)
    assert figures[4] <= 1e-4 * figures[5] + 1e-6


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("H", [1, 4])
def test_packed_bags_and_their_half_views_match_fp64(dev, H, bf16):
    from madeleine_amd import functional as MF
    E32, s32 = _inputs(LENS, H, "ref%d" % H)
    E, s = E32.to(dev, torch.bfloat16 if bf16 else torch.float32), s32.to(dev)
    perm, vcu = (x.to(dev) for x in _halves(LENS))
    g = t((len(LENS), 3, H * HID), "kinds:g%d" % H).to(dev)
    cu = torch.tensor([0] + list(itertools.accumulate(LENS)), dtype=torch.int64, device=dev)
    nb, max_len, max_view = len(LENS), max(LENS), max(n - n // 2 for n in LENS)
    ref_bags, ref_views = _reference(H)

    pooled, m, l = MF.pool_fwd_raw(E, s, nb, 0, cu, max_len)
    dE, ds = torch.full_like(E, float("nan")), torch.full_like(s, float("nan"))
    MF.pool_bwd_raw(E, s, pooled, m, l, g[:, 0].contiguous(), dE, 0, ds, 0, nb, 0, cu, max_len)
    _check("bags", pooled.view(nb, 1, -1), dE, ds, ref_bags, bf16)

    vp, vm, vl = MF.pool_rview_fwd_raw(E, s, nb, perm, vcu, max_view)
    assert float(vp[0, 0].abs().max()) == 0.0, "the empty first half of the 1-token bag"
    dE, ds = torch.zeros_like(E), torch.zeros_like(s)
    MF.pool_rview_bwd_raw(E, s, vp, vm, vl, g[:, 1:].contiguous(), dE, ds, nb, perm, vcu, max_view)
    _check("half-views", vp, dE, ds, ref_views, bf16)
