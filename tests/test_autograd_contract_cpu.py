"""The fp64 references of tests/_autograd_ref.py held to torch.autograd.gradcheck and to oracle.restatement at tiny shapes -- a wrong
reference cannot pass a wrong node -- and the node table of tests/test_autograd_contract_gpu.py held to the torch.autograd.Function
classes that exist: a node added later fails here until the table has it.  No GPU."""
import inspect

import torch
import torch.nn.functional as F
from torch.autograd import gradcheck

from oracle import restatement as R
from tests import _autograd_ref as A


def _r(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + 31 * len(shape) + sum(shape))
    return ((torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * scale).requires_grad_()


def _keep(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) < 0.7).to(torch.uint8)


H, W, T = 2, 4, 7


def _gate(seed=0):
    return [_r(H, W, W, seed=seed + 1), _r(H, W, seed=seed + 2), _r(H, W, W, seed=seed + 3), _r(H, W, seed=seed + 4), _r(H, W, seed=seed + 5),
            _r(H, seed=seed + 6)]


def test_gate_scores_is_the_oracle_gate_per_head_and_differentiates():
    E, gate = _r(T, H * W), _gate()
    ka, kb = _keep(T, H, W, seed=1), _keep(T, H, W, seed=2)
    s = A.gate_scores(E, *gate, p=R.GATE_DROPOUT_P, keep_a=ka, keep_b=kb)
    for c in range(H):
        ref = R.gate_scores(E[:, c * W:(c + 1) * W], gate[0][c], gate[1][c], gate[2][c], gate[3][c], gate[4][c:c + 1], gate[5][c:c + 1],
                            ka[:, c].double(), kb[:, c].double())
        assert torch.allclose(s[:, c:c + 1], ref, rtol=1e-13, atol=1e-14)
    assert gradcheck(lambda e, *g: A.gate_scores(e, *g, p=0.25, keep_a=ka, keep_b=kb), [E] + gate)


def test_pools_are_the_oracle_pooling_and_differentiate():
    B, N = 2, 5
    E, s = _r(B, N, H * W), _r(B, N, H, scale=3.0)
    # oracle.restatement.abmil_embed: slide = (e * softmax(raw, dim=1)).sum(dim=1) with e [B, N, W, H] -- head-major here
    e_ref = E.view(B, N, H, W).permute(0, 1, 3, 2)
    slide = (e_ref * torch.softmax(s, dim=1).unsqueeze(2)).sum(dim=1)              # [B, W, H]
    assert torch.allclose(A.softmax_pool(E, s).view(B, H, W), slide.transpose(1, 2), rtol=1e-13, atol=1e-14)
    cu = torch.tensor([0, 1, 4, 10])
    E2, s2 = E.reshape(B * N, -1), s.reshape(B * N, H)
    packed = A.softmax_pool(E2, s2, cu)
    assert torch.allclose(packed[1], A.softmax_pool(E2[1:4].unsqueeze(0), s2[1:4].unsqueeze(0))[0], rtol=1e-13, atol=1e-14)
    assert torch.allclose(A.weighted_pool(E2, torch.softmax(s2[0:1], 0).expand(B * N, H) * 0 + 1, cu)[0], E2[0], rtol=1e-13, atol=1e-14)
    idx = torch.tensor([3, 0, 4])
    assert torch.allclose(A.view_pool(E, s, idx), A.softmax_pool(E[:, idx], s[:, idx]), rtol=1e-13, atol=1e-14)
    perm = torch.tensor([0, 2, 1, 3, 9, 4, 8, 5, 7, 6], dtype=torch.int32)
    vcu = torch.tensor([0, 0, 1, 2, 4, 7, 10])
    rv = A.rview_pool(E2, s2, perm, vcu)
    assert rv.shape == (3, 2, H * W) and float(rv[0, 0].detach().abs().max()) == 0.0          # a one-token bag's first view is empty
    assert torch.allclose(rv[2, 1], A.softmax_pool(E2[[5, 7, 6]].unsqueeze(0), s2[[5, 7, 6]].unsqueeze(0))[0], rtol=1e-13, atol=1e-14)
    assert gradcheck(A.softmax_pool, [E, s]) and gradcheck(lambda e, x: A.softmax_pool(e, x, cu), [E2, s2])
    assert gradcheck(A.weighted_pool, [E, s]) and gradcheck(lambda e, x: A.weighted_pool(e, x, cu), [E2, s2])
    assert gradcheck(lambda e, x: A.view_pool(e, x, idx), [E, s]) and gradcheck(lambda e, x: A.rview_pool(e, x, perm, vcu), [E2, s2])


def test_attn_pool_composes_and_differentiates():
    B, N, P = 2, 5, 3
    E, gate, Wt, bt = _r(B, N, H * W), _gate(), _r(P, H * W, seed=8), _r(P, seed=9)
    views = [torch.tensor([0, 3]), torch.tensor([1, 2, 4])]
    pooled, scores, tok = A.attn_pool(E, gate, tok=(Wt, bt), views=views)
    assert pooled.shape == (B, 3, H * W) and scores.shape == (B * N, H) and tok.shape == (B * N, P)
    s = A.gate_scores(E.reshape(B * N, -1), *gate).view(B, N, H)
    assert torch.equal(pooled[:, 0], A.softmax_pool(E, s)) and torch.equal(pooled[:, 2], A.view_pool(E, s, views[1]))
    assert torch.equal(tok, F.linear(E.reshape(B * N, -1), Wt, bt))
    assert gradcheck(lambda e, wt, b, *g: A.attn_pool(e, g, tok=(wt, b), views=views), [E, Wt, bt] + gate)
    cu = torch.tensor([0, 1, 4, 10])
    perm = torch.tensor([0, 2, 1, 3, 9, 4, 8, 5, 7, 6], dtype=torch.int32)
    vcu = torch.tensor([0, 0, 1, 2, 4, 7, 10])
    E2 = E.reshape(B * N, -1).detach().requires_grad_()
    pooled, _, none = A.attn_pool(E2, gate, cu=cu, rviews=(perm, vcu))
    assert pooled.shape == (3, 3, H * W) and none is None
    assert gradcheck(lambda e, *g: A.attn_pool(e, g, cu=cu, rviews=(perm, vcu))[:2], [E2] + gate)


def test_ln_gelu_drop_and_preattn_block_are_the_oracle_block_and_differentiate():
    rows, Wd, K = 6, 8, 5
    x, g, b, lb = _r(rows, K, scale=2.0), _r(Wd, seed=1), _r(Wd, seed=2), _r(Wd, seed=3)
    Wl = _r(Wd, K, seed=4)
    keep = _keep(rows, Wd, seed=3)
    sd = {"p.0.weight": Wl, "p.0.bias": lb, "p.1.weight": g, "p.1.bias": b}
    for i in (4, 8):      # (the oracle runs three blocks: the second and third are given the identity shape here and not compared)
        sd.update({f"p.{i}.weight": torch.eye(Wd, dtype=torch.float64), f"p.{i}.bias": torch.zeros(Wd, dtype=torch.float64),
                   f"p.{i + 1}.weight": torch.ones(Wd, dtype=torch.float64), f"p.{i + 1}.bias": torch.zeros(Wd, dtype=torch.float64)})
    one = A.preattn_block(x, Wl, lb, g, b, p=R.PRE_DROPOUT_P, keep=keep)
    ref = R._drop(F.gelu(F.layer_norm(F.linear(x, Wl, lb), (Wd,), g, b, 1e-5)), keep.double(), R.PRE_DROPOUT_P)
    assert torch.allclose(one, ref, rtol=1e-13, atol=1e-14)
    three = R.pre_attn(x, sd, prefix="p.")
    two_more = A.preattn_block(A.preattn_block(A.preattn_block(x, Wl, lb, g, b), sd["p.4.weight"], sd["p.4.bias"], sd["p.5.weight"],
                                               sd["p.5.bias"]), sd["p.8.weight"], sd["p.8.bias"], sd["p.9.weight"], sd["p.9.bias"])
    assert torch.allclose(three, two_more, rtol=1e-13, atol=1e-14)
    y = _r(rows, Wd, seed=5)
    assert torch.allclose(A.ln_gelu_drop(y, g, b, lb, p=0.1, keep=keep), R._drop(F.gelu(F.layer_norm(y + lb, (Wd,), g, b, 1e-5)), keep.double(), 0.1),
                          rtol=1e-13, atol=1e-14)
    cu = torch.tensor([0, 1, 1, 6])
    gb = _r(3, Wd, seed=6)
    rows_of = torch.tensor([0, 2, 2, 2, 2, 2])
    assert torch.allclose(A.ln_gelu_drop(y, g, b, gb, cu_groups=cu), A.ln_gelu_drop(y + gb[rows_of], g, b), rtol=1e-13, atol=1e-14)
    assert torch.allclose(A.preattn_block(x, Wl, lb, g, b, gbias=gb, cu_groups=cu),
                          A.ln_gelu_drop(F.linear(x, Wl, lb) + gb[rows_of], g, b), rtol=1e-13, atol=1e-14)
    assert gradcheck(lambda *a: A.ln_gelu_drop(*a, p=0.1, keep=keep), [y, g, b, lb])
    assert gradcheck(lambda *a: A.ln_gelu_drop(*a, p=0.1, keep=keep, cu_groups=cu), [y, g, b, gb])
    assert gradcheck(lambda x_, w_, lb_, g_, b_, gb_: A.preattn_block(x_, w_, lb_, g_, b_, p=0.1, keep=keep, gbias=gb_, cu_groups=cu),
                     [x, Wl, lb, g, b, gb])
    assert gradcheck(A.linear, [x, Wl, lb])


def test_info_nce_references_are_the_oracle_losses_and_differentiate():
    S, K, D, Tm = 2, 5, 6, 0.5
    Q, P = _r(S, K, D), _r(S, K, D, seed=1)
    cnt = torch.tensor([5, 3], dtype=torch.int32)
    for sym in (False, True):
        loss, rows = A.info_nce_batched(Q, P, cnt, Tm, sym)
        for s in range(S):
            k = int(cnt[s])
            assert torch.allclose(loss[s], R.info_nce(Q[s, :k], P[s, :k], Tm, sym), rtol=1e-13, atol=1e-14)
            assert torch.allclose(rows[s, :k].mean(), loss[s], rtol=1e-13, atol=1e-14) and float(rows[s, k:].detach().abs().sum()) == 0.0
        assert gradcheck(lambda q, p: A.info_nce_batched(q, p, cnt, Tm, sym), [Q, P])
    q, p = _r(K, D, seed=2), _r(K, D, seed=3)
    # no negatives beyond the other positives: the explicit-negatives loss with each query's other positives IS the in-batch loss
    neg = torch.stack([torch.cat([p[:i], p[i + 1:]]) for i in range(K)])
    loss, rows = A.info_nce_neg(q, p, neg, Tm, True)
    assert torch.allclose(loss, R.info_nce(q, p, Tm, False), rtol=1e-13, atol=1e-14)
    assert torch.allclose(rows, R.info_nce(q, p, Tm, False, reduction="none"), rtol=1e-13, atol=1e-14)
    bank = _r(4, D, seed=4)
    assert torch.allclose(A.info_nce_neg(q, p, bank, Tm, False)[1], A.info_nce_neg(q, p, bank.unsqueeze(0).expand(K, -1, -1), Tm, True)[1],
                          rtol=1e-13, atol=1e-14)
    assert gradcheck(lambda a, b, c: A.info_nce_neg(a, b, c, Tm, True), [q, p, neg.detach().requires_grad_()])
    assert gradcheck(lambda a, b, c: A.info_nce_neg(a, b, c, Tm, False), [q, p, bank])


def test_got_reference_is_the_oracle_got():
    v, q = _r(2, 4, 6), _r(2, 4, 6, seed=1)
    assert torch.allclose(A.got(v, q).sum(), R.got(v, q), rtol=1e-13, atol=1e-14)
    assert A.got(v, _r(2, 3, 6, seed=2)).shape == (2,)


def _function_classes():
    from madeleine_amd import distributed, functional, model
    found = set()
    for mod in (functional, model, distributed):
        for name, obj in inspect.getmembers(mod, inspect.isclass):
            if issubclass(obj, torch.autograd.Function) and obj.__module__ == mod.__name__:
                found.add(obj.__name__)
    return found


def test_every_autograd_node_is_in_the_gpu_table():
    from tests.test_autograd_contract_gpu import NODE_CLASSES, NODES, NOT_IN_TABLE
    found = _function_classes()
    assert len(found) >= 14, found
    assert not set(NODE_CLASSES) & set(NOT_IN_TABLE)
    assert found - set(NOT_IN_TABLE) == set(NODE_CLASSES), (
        "autograd nodes without an entry in tests/test_autograd_contract_gpu.py::NODES, or entries for classes that no longer exist",
        (found - set(NOT_IN_TABLE)) ^ set(NODE_CLASSES))
    assert set(NOT_IN_TABLE) <= found and all(NOT_IN_TABLE.values())
    assert len({n.name for n in NODES}) == len(NODES)
    for n in NODES:      # every bound names the existing test it was taken from
        assert n.cite and len(n.fwd) >= 1 and n.grad
