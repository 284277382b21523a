"""Losses of the cross-stain pretrain step -- mirrors of the reference's `InfoNCE` and `GOT`
(reference madeleine/utils/loss.py:10-133 and :278-302), computed by libmadeleine_amd.so.
"""
import torch
from torch import nn

from . import functional as MF

__all__ = ['InfoNCE', 'info_nce', 'GOT', 'init_intra_wsi_loss_function']


def _validate(query, positive_key, negative_keys, negative_mode):
    """Argument checks of loss.py:67-89 (same messages)."""
    if query.dim() != 2:
        raise ValueError('<query> must have 2 dimensions.')
    if positive_key.dim() != 2:
        raise ValueError('<positive_key> must have 2 dimensions.')
    if negative_keys is not None:
        if negative_mode == 'unpaired' and negative_keys.dim() != 2:
            raise ValueError("<negative_keys> must have 2 dimensions if <negative_mode> == 'unpaired'.")
        if negative_mode == 'paired' and negative_keys.dim() != 3:
            raise ValueError("<negative_keys> must have 3 dimensions if <negative_mode> == 'paired'.")
    if len(query) != len(positive_key):
        raise ValueError('<query> and <positive_key> must must have the same number of samples.')
    if negative_keys is not None:
        if negative_mode == 'paired' and len(query) != len(negative_keys):
            raise ValueError("If negative_mode == 'paired', then <negative_keys> must have the same number of samples as <query>.")
    if query.shape[-1] != positive_key.shape[-1]:
        raise ValueError('Vectors of <query> and <positive_key> should have the same number of components.')
    if negative_keys is not None:
        if query.shape[-1] != negative_keys.shape[-1]:
            raise ValueError('Vectors of <query> and <negative_keys> should have the same number of components.')


def info_nce(query, positive_key, negative_keys=None, temperature=0.1, reduction='mean', negative_mode='unpaired',
             symmetric=False):
    _validate(query, positive_key, negative_keys, negative_mode)
    if reduction not in ('mean', 'sum', 'none'):
        raise ValueError("reduction must be 'mean', 'sum' or 'none' (F.cross_entropy's values, loss.py:124)")
    if negative_keys is not None:
        return _info_nce_negatives(query, positive_key, negative_keys, temperature, reduction, negative_mode)
    k, d = query.shape
    q, p = query.float().contiguous(), positive_key.float().contiguous()
    if d % 32:   # the similarity kernel works on 32-wide feature blocks: zero columns change neither norms nor cosines
        pad = 32 - d % 32
        q, p = torch.nn.functional.pad(q, (0, pad)), torch.nn.functional.pad(p, (0, pad))
    cnt = torch.full((1,), k, dtype=torch.int32, device=query.device)
    if reduction == 'none':
        return MF.info_nce_rows(q.unsqueeze(0), p.unsqueeze(0), cnt, temperature, symmetric)[0]
    loss = MF.info_nce_batched(q.unsqueeze(0), p.unsqueeze(0), cnt, temperature, symmetric)[0]
    return loss * k if reduction == 'sum' else loss


def _info_nce_negatives(query, positive_key, negative_keys, temperature, reduction, negative_mode):
    """Explicit negatives (loss.py:93-110).  The reference branch builds the logits [q.p | q.n^T] of the normalised rows with the
    target in column 0, then falls off the end of the function and returns None; the loss computed here is the cross entropy its
    in-batch branch applies to such logits, F.cross_entropy(logits / temperature, labels, reduction) (loss.py:125).  `symmetric` is
    not read (neither is it in the reference branch): the result is the same for True and False.  Gradients flow to query,
    positive_key and negative_keys; the negatives' backward runs only when negative_keys requires grad."""
    if negative_mode not in ('paired', 'unpaired'):
        # the reference fails here with an UnboundLocalError (its logits are never formed)
        raise ValueError("negative_mode must be 'paired' or 'unpaired' (got %r)" % (negative_mode,))
    n, d = query.shape
    q, p = query.float().contiguous(), positive_key.float().contiguous()
    neg = negative_keys.float().contiguous()   # read in place, any width: only the small operands are padded
    if d % 32:   # the kernels take Q, P in 32-wide feature blocks: zero columns change neither norms nor cosines
        pad = 32 - d % 32
        q, p = torch.nn.functional.pad(q, (0, pad)), torch.nn.functional.pad(p, (0, pad))
    paired = negative_mode == 'paired'
    if reduction == 'none':
        return MF.info_nce_neg_rows(q, p, neg, temperature, paired)
    loss = MF.info_nce_neg(q, p, neg, temperature, paired)
    return loss * n if reduction == 'sum' else loss


class InfoNCE(nn.Module):
    """Same constructor and call signature as the reference class (loss.py:10-64)."""

    def __init__(self, temperature=0.1, reduction='mean', negative_mode='unpaired'):
        super().__init__()
        self.temperature = temperature
        self.reduction = reduction
        self.negative_mode = negative_mode

    def forward(self, query, positive_key, negative_keys=None, symmetric=False):
        return info_nce(query, positive_key, negative_keys, temperature=self.temperature, reduction=self.reduction,
                        negative_mode=self.negative_mode, symmetric=symmetric)

    def batched(self, Q, P, cnt, symmetric=False):
        """S problems at once: Q,P [S,Kmax,D] padded, cnt int32 [S] -> loss [S] (mean reduction)."""
        return MF.info_nce_batched(Q.float().contiguous(), P.float().contiguous(), cnt, self.temperature, symmetric)


def init_intra_wsi_loss_function(config):
    """loss.py:138-157."""
    if config["intra_modality_mode_wsi"] in ("reconstruct_avg_emb", "reconstruct_masked_emb"):
        return nn.MSELoss()
    return InfoNCE(temperature=config["temperature"])


def GOT(v_, q_, subsample=None):
    """Graph optimal transport token alignment (loss.py:278-302): sum_b GW_b + sum_b WD_b.

    The sub-sample quirk of the reference is kept: indices are torch.randperm(v_.shape[0]) -- the (masked)
    BATCH size k, not the token count -- so the first n = min(k, subsample) tokens of each bag are used, in a
    random order that only changes summation order.

    v_ [k, n, d] and q_ [k, m, d] may hold different token counts (n != m, both <= 4096): the cross cost and the transport plans are
    then n x m, on the tiled size class.  GOT(v, q) != GOT(q, v).  With `subsample` both are indexed with the same indices, as in
    the reference, and an index beyond the shorter one raises IndexError."""
    rect = v_.dim() == 3 and q_.dim() == 3 and v_.shape[1] != q_.shape[1]
    if subsample is not None:
        patch_indices = torch.randperm(v_.shape[0])[:subsample]
        if rect:
            short = min(v_.shape[1], q_.shape[1])
            if patch_indices.numel() and int(patch_indices.max()) >= short:
                # what the reference's v_[:, idx, :] raises; checked on the host so that no device-side bounds assert fires
                raise IndexError("index %d is out of bounds for dimension 1 with size %d" % (int(patch_indices.max()), short))
        patch_indices = patch_indices.to(v_.device)
        v_ = v_.index_select(1, patch_indices)
        q_ = q_.index_select(1, patch_indices)
        rect = False   # equal token counts from here on
    v, q = v_.float().contiguous(), q_.float().contiguous()
    if v.dim() != 3 or (rect and (v.shape[0], v.shape[2]) != (q.shape[0], q.shape[2])):
        # not two [k, ., d] token sets: no size class to ask for; the autograd node's own shape check raises ValueError
        out = MF.got_tiled(v, q) if rect else MF.got(v, q)
        return out[1] + out[0]
    route = got_route(*v.shape, m=q.shape[1] if rect else None)
    if route == "unsupported" and rect:
        raise NotImplementedError("madeleine_amd.GOT supports n <= 4096 and m <= 4096 tokens per bag and d <= 4096 "
                                  "(got n=%d, m=%d, d=%d)" % (v.shape[1], q.shape[1], v.shape[2]))
    if route == "unsupported":
        raise NotImplementedError("madeleine_amd.GOT supports n <= 4096 tokens per bag and d <= 4096 (got n=%d, d=%d)"
                                  % tuple(v.shape[1:]))
    out = MF.got(v, q) if route == "resident" else MF.got_tiled(v, q)
    return out[1] + out[0]


def got_route(k, n, d, m=None):
    """Size class GOT() uses for [k, n, d] after the sub-sampling: 'resident' where mdl_got_ws_bytes accepts the shape (functional.got,
    the training path's class), else 'tiled' where the tiled class accepts it, else 'unsupported'.  With m given and m != n (q_ holds m
    tokens per bag) only the tiled class can take the pair: 'tiled' or 'unsupported'."""
    if m is not None and m != n:
        return "tiled" if MF.got_tiled_supported(k, n, d, m) else "unsupported"
    if MF.got_resident_supported(k, n, d):
        return "resident"
    if MF.got_tiled_supported(k, n, d):
        return "tiled"
    return "unsupported"
