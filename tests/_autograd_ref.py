"""Differentiable fp64 CPU references of the operations behind the autograd nodes, for tests/test_autograd_contract_gpu.py.  Each is a
plain torch expression of the operation (layouts as include/madeleine_amd.h: token embeddings head-major [T, H*512], scores [T, H]), so
that torch's own autograd gives the gradient of any loss built from any subset of the outputs with respect to any subset of the
inputs.  tests/test_autograd_contract_cpu.py holds them to torch.autograd.gradcheck and to oracle.restatement at tiny shapes.
Test infrastructure."""
import torch
import torch.nn.functional as F

from oracle import restatement as R


def _drop(x, keep, p):
    """Inverted dropout under a keep mask (None: identity)."""
    return x if keep is None else x * keep.to(x.dtype) / (1.0 - p)


def bags_of(cu, T):
    """[(start, stop)] of the bags: from packed offsets `cu` [n_bags + 1]."""
    cu = [int(c) for c in cu]
    assert cu[-1] == T
    return list(zip(cu[:-1], cu[1:]))


def gate_scores(E, Wa, ba, Wb, bb, wc, bc, p=0.0, keep_a=None, keep_b=None):
    """scores [T, H] of E [T, H*W] (head-major): per head c, oracle.restatement.gate_scores with Wa, Wb [H, W, W], ba, bb, wc [H, W],
    bc [H]; keep_a, keep_b [T, H, W] (1 = keep) under dropout rate p."""
    H, W = Wa.shape[0], Wa.shape[2]
    cols = []
    for c in range(H):
        x = E[:, c * W:(c + 1) * W]
        a = _drop(torch.tanh(x @ Wa[c].t() + ba[c]), None if keep_a is None else keep_a[:, c], p)
        b = _drop(torch.sigmoid(x @ Wb[c].t() + bb[c]), None if keep_b is None else keep_b[:, c], p)
        cols.append((a * b) @ wc[c] + bc[c])
    return torch.stack(cols, dim=1)


def _pool_rows(E, w):
    """sum_t w[t, c] E[t, c, :] -> [H*W] for E [n, H*W] (head-major) and weights w [n, H]."""
    n, H = w.shape
    if n == 0:
        return E.new_zeros(E.shape[1])
    return torch.einsum("nh,nhe->he", w, E.view(n, H, -1)).reshape(-1)


def softmax_pool(E, scores, cu=None):
    """pooled [n_bags, H*W]: dense E [B, N, H*W] with scores [B, N, H], or packed E [T, H*W], scores [T, H] with offsets cu."""
    if cu is None:
        return torch.stack([_pool_rows(E[b], torch.softmax(scores[b], dim=0)) for b in range(E.shape[0])])
    return torch.stack([_pool_rows(E[a:b], torch.softmax(scores[a:b], dim=0)) for a, b in bags_of(cu, E.shape[0])])


def weighted_pool(E, w, cu=None):
    """softmax_pool with the weights taken as they are."""
    if cu is None:
        return torch.stack([_pool_rows(E[b], w[b]) for b in range(E.shape[0])])
    return torch.stack([_pool_rows(E[a:b], w[a:b]) for a, b in bags_of(cu, E.shape[0])])


def view_pool(E, scores, idx):
    """pooled [B, H*W] of the tokens idx (int64 [n]) of every dense bag, the raw scores re-softmaxed over them."""
    return torch.stack([_pool_rows(E[b, idx], torch.softmax(scores[b, idx], dim=0)) for b in range(E.shape[0])])


def rview_pool(E, scores, perm, vcu):
    """pooled [n_bags, 2, H*W]: view v of bag b holds the packed rows perm[vcu[2 b + v] : vcu[2 b + v + 1]]."""
    perm, vcu = perm.long(), [int(x) for x in vcu]
    out = []
    for v in range(len(vcu) - 1):
        rows = perm[vcu[v]:vcu[v + 1]]
        out.append(_pool_rows(E[rows], torch.softmax(scores[rows], dim=0)))
    return torch.stack(out).view((len(vcu) - 1) // 2, 2, -1)


def attn_pool(E, gate, p=0.0, keep_a=None, keep_b=None, cu=None, tok=None, views=(), rviews=None):
    """(pooled, scores, token projections) of functional.attn_pool: gate = (Wa, ba, Wb, bb, wc, bc), tok = (Wtok, btok or None) or
    None (third result None), views = int64 index lists (dense bags; pooled [B, 1 + V, H*W]), rviews = (perm, vcu) (packed bags;
    pooled [n_bags, 3, H*W])."""
    E2d = E.reshape(-1, E.shape[-1])
    scores = gate_scores(E2d, *gate, p=p, keep_a=keep_a, keep_b=keep_b)
    s = scores if cu is not None else scores.view(E.shape[0], E.shape[1], -1)
    pooled = softmax_pool(E, s, cu)
    if views:
        pooled = torch.stack([pooled] + [view_pool(E, s, idx) for idx in views], dim=1)
    elif rviews is not None:
        pooled = torch.cat([pooled.unsqueeze(1), rview_pool(E2d, scores, *rviews)], dim=1)
    t = None
    if tok is not None:
        t = E2d @ tok[0].t() + (tok[1] if tok[1] is not None else 0.0)
    return pooled, scores, t


def ln_gelu_drop(x, gamma, beta, bias=None, eps=1e-5, p=0.0, keep=None, cu_groups=None):
    """Dropout_p(GELU(LayerNorm(x + bias))) over the last axis; with cu_groups, bias is [G, W] and rows cu_groups[g]:cu_groups[g+1]
    take bias[g]."""
    if bias is not None:
        if cu_groups is not None:
            cu = [int(c) for c in cu_groups]
            bias = torch.cat([bias[g:g + 1].expand(b - a, -1) for g, (a, b) in enumerate(zip(cu[:-1], cu[1:]))])
        x = x + bias
    return _drop(F.gelu(F.layer_norm(x, x.shape[-1:], gamma, beta, eps)), keep, p)


def linear(x, W, bias=None):
    return x @ W.t() + (bias if bias is not None else 0.0)


def preattn_block(x, W, lin_bias, gamma, beta, eps=1e-5, p=0.0, keep=None, gbias=None, cu_groups=None):
    """One block of the pre-attention MLP: Linear (+ a bias row per group of rows) -> LayerNorm -> GELU -> Dropout."""
    y = linear(x, W, lin_bias)
    if gbias is not None:
        cu = [int(c) for c in cu_groups]
        y = y + torch.cat([gbias[g:g + 1].expand(b - a, -1) for g, (a, b) in enumerate(zip(cu[:-1], cu[1:]))])
    return ln_gelu_drop(y, gamma, beta, None, eps, p, keep)


def info_nce_batched(Q, P, cnt, temperature, symmetric):
    """(loss [S], rows [S, Kmax]) of S padded problems: problem s is oracle.restatement.info_nce on its first cnt[s] rows; rows holds
    its per-sample losses (reduction 'none'), zero on the padding; loss[s] is their mean."""
    losses, rows = [], []
    for s in range(Q.shape[0]):
        k = int(cnt[s])
        r = R.info_nce(Q[s, :k], P[s, :k], temperature, symmetric, reduction="none")
        losses.append(r.mean())
        rows.append(torch.cat([r, r.new_zeros(Q.shape[1] - k)]))
    return torch.stack(losses), torch.stack(rows)


def info_nce_neg(Q, P, Neg, temperature, paired):
    """(loss [], rows [N]) against explicit negatives: logits [q.p | q.n] / T over normalised rows, target column 0 (the restatement of
    tests/test_infonce_negatives_gpu.py::ref_loss)."""
    qn, pn, nn_ = F.normalize(Q, dim=-1), F.normalize(P, dim=-1), F.normalize(Neg, dim=-1)
    pos = (qn * pn).sum(-1, keepdim=True)
    negl = (qn.unsqueeze(1) @ nn_.transpose(-2, -1)).squeeze(1) if paired else qn @ nn_.transpose(-2, -1)
    logits = torch.cat([pos, negl], dim=1) / temperature
    rows = F.cross_entropy(logits, torch.zeros(len(Q), dtype=torch.long), reduction="none")
    return rows.mean(), rows


def got(V, Q):
    """out [2] = (sum_b WD_b, sum_b GWD_b): oracle.restatement.got_parts with the batch's own extrema (n != m allowed)."""
    return R.got_parts(V, Q)
