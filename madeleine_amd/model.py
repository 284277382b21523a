"""MADELEINE slide encoder -- MI355X-native mirror of the reference's `MADELEINE`, `ABMILEmbedder`
and `create_model` (reference madeleine/models/Model.py:15-43, :45-216, :314-451).

Same constructor / forward / encode_he contracts, same sub-module names and therefore the same
state_dict keys and shapes (reference and HuggingFace checkpoints load unchanged, with or without a
`module.` prefix).  What differs is where the work happens:

  * pre_attn (3 x Linear + fused LayerNorm-GELU-Dropout), token_projector and projector run in the hand-written
    fp32 matrix-core Linear kernels (functional.linear / ln_gelu_drop) -- in the bf16
    mode (torch.autocast(bfloat16)) in their bf16 siblings (mdl_linear_*_bf16: bf16 activations, fp32 parameters);
  * gated attention scores + softmax-over-patches + weighted pooling, forward and backward, are the
    hand-written HIP kernels behind madeleine_amd.functional.attn_pool.

Head-major trick: the reference interleaves heads as channel j = e*H + c (rearrange
'b t (e c) -> b t e c', Model.py:396).  We permute the ROWS of pre_attn.8 / LayerNorm 9 (and the
COLUMNS of token_projector / projector) by a fixed index vector at forward time, so the encoder emits
the very same numbers with channel order j' = c*512 + e.  Every kernel then reads contiguous 2 KiB
head rows and no activation is ever permuted.  Parameters keep the reference layout.
"""
from collections import OrderedDict
from typing import Dict, Optional, Union

import numpy as np
import os

import torch
import torch.nn.functional as F
from torch import nn

from . import functional as MF
from .abmil import BatchedABMIL, activate

HE_POSITION = 0
PRE_DROPOUT_P = 0.1  # Model.py:354,358,362
SUPPORTED_HEADS = (1, 2, 4, 8)


class _PermuteFn(torch.autograd.Function):
    """w.index_select(dim, perm) for a BIJECTIVE perm: the backward is the gather by the inverse permutation (one kernel)
    instead of autograd's index_put_(accumulate=True), which sorts the indices (~10 small launches per use and step)."""

    @staticmethod
    def forward(ctx, w, perm, inv, dim):
        ctx.save_for_backward(inv)
        ctx.dim = dim
        return w.index_select(dim, perm)

    @staticmethod
    def backward(ctx, g):
        (inv,) = ctx.saved_tensors
        return g.index_select(ctx.dim, inv), None, None, None


def ragged_view_plan(lens):
    """Host side of the intra-modality views on packed bags (Model.py:419-440 applied to each bag on its own): for every bag in packed
    order, `idx = np.arange(N_b); np.random.shuffle(idx); mid = N_b // 2` -- the reference's draw for one bag -- view 1 = idx[:mid],
    view 2 = idx[mid:].  Returns (perm int32 [T]: the absolute packed rows cu[b] + idx, bag after bag; vcu int64 [2*n_bags + 1]:
    positions in perm where each view starts; max_view_len), the inputs of the ragged-view pooling kernels (mdl_abmil_pool_rview_*)."""
    lens = [int(n) for n in lens]
    perm = np.empty(sum(lens), dtype=np.int32)
    vcu = np.empty(2 * len(lens) + 1, dtype=np.int64)
    start, max_view = 0, 0
    for b, n in enumerate(lens):
        idx = np.arange(n)
        np.random.shuffle(idx)
        mid = n // 2
        perm[start:start + n] = start + idx
        vcu[2 * b], vcu[2 * b + 1] = start, start + mid
        max_view = max(max_view, n - mid)
        start += n
    vcu[-1] = start
    return torch.from_numpy(perm), torch.from_numpy(vcu), max_view


def bf16_mode() -> bool:
    """True inside torch.autocast(device_type='cuda', dtype=torch.bfloat16): selects the kernels' bf16 mode."""
    return torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.bfloat16


def _strip_module_prefix(state_dict):
    """Model.py:31-40 / utils.py:112-120: DataParallel checkpoints carry a 'module.' prefix."""
    if not any(k.startswith("module.") for k in state_dict):
        return state_dict
    return OrderedDict((k[7:] if k.startswith("module.") else k, v) for k, v in state_dict.items())


def create_model(model_cfg: Union[str, Dict], device: Union[str, torch.device] = 'cpu',
                 checkpoint_path: Optional[str] = None):
    """Mirror of Model.py:15-43."""
    model = MADELEINE(config=model_cfg, stain_encoding=False).to(device)
    if checkpoint_path:
        state_dict = torch.load(checkpoint_path, weights_only=True, map_location=device)   # a state dict: safe unpickler
        model.load_state_dict(_strip_module_prefix(state_dict), strict=True)
        print("* Loaded weights successfully!")
    return model


class ABMILEmbedder(nn.Module):
    """Multi-head gated-ABMIL patch aggregator (Model.py:314-451)."""

    def __init__(self, pre_attention_params: dict = None, attention_params: dict = None, aggregation: str = 'regular') -> None:
        super().__init__()
        self.pre_attention_params = pre_attention_params
        self.attention_params = attention_params
        self.n_heads = attention_params['params']["n_heads"]
        if self.n_heads not in SUPPORTED_HEADS:
            # every encoder kernel (pooling, gates, the 512*H-wide LayerNorm-GELU-Dropout) is instantiated for these head counts only
            raise ValueError(f"n_heads must be one of {SUPPORTED_HEADS} (got {self.n_heads!r})")
        self._build_pre_attention_params(params=pre_attention_params)
        if attention_params is not None:
            self._build_attention_params(attn_model=attention_params['model'], params=attention_params['params'])
        self.agg_type = aggregation
        H = self.n_heads
        hid = pre_attention_params['hidden_dim']
        # perm[j'] = j with j' = c*hid + e (head-major) and j = e*H + c (reference order)
        jp = torch.arange(hid * H)
        self.register_buffer("_perm", (jp % hid) * H + (jp // hid), persistent=False)
        self.register_buffer("_inv_perm", torch.argsort(self._perm), persistent=False)
        self._injected_keep = None  # dict(pre=[3 masks, reference layout], gate=[(ka,kb) per head]) for parity tests

    def _build_pre_attention_params(self, params):
        H = self.n_heads
        self.pre_attn = nn.Sequential(
            nn.Linear(params['input_dim'], params['hidden_dim']),
            nn.LayerNorm(params['hidden_dim']),
            nn.GELU(),
            nn.Dropout(PRE_DROPOUT_P),
            nn.Linear(params['hidden_dim'], params['hidden_dim']),
            nn.LayerNorm(params['hidden_dim']),
            nn.GELU(),
            nn.Dropout(PRE_DROPOUT_P),
            nn.Linear(params['hidden_dim'], params['hidden_dim'] * H),
            nn.LayerNorm(params['hidden_dim'] * H),
            nn.GELU(),
            nn.Dropout(PRE_DROPOUT_P),
        )

    def _build_attention_params(self, attn_model='ABMIL', params=None):
        if attn_model == 'ABMIL':
            self.attn = nn.ModuleList([BatchedABMIL(**params) for _ in range(self.n_heads)])
        else:
            raise NotImplementedError('Attention model not implemented -- Options are ABMIL')

    # ------------------------------------------------------------------ internals (head-major)
    def permuted(self, w, dim):
        """Parameter `w` with axis `dim` (length H*512) in head-major order."""
        return _PermuteFn.apply(w, self._perm, self._inv_perm, dim)

    def _drop_cfg(self, blk, perm=None):
        """(p, seed, keep) of block `blk`'s dropout for this forward."""
        p, seed, keep = 0.0, 0, None
        if self.training:
            p = float(self.pre_attn[4 * blk + 3].p)   # the nn.Dropout module of this block (0.1 unless the user changed it)
            inj = self._injected_keep
            if p == 0.0:
                pass
            elif inj is not None:
                keep = inj["pre"][blk]
                if perm is not None:
                    keep = keep[..., perm]
                keep = keep.to(torch.uint8).contiguous()
            else:
                seed = MF.new_dropout_seed()
        return p, seed, keep

    def _block_split(self, x, x_scale, blk, perm=None, want_fp32=False, weight=None, group_bias=None):
        """Linear + LayerNorm + GELU + Dropout of block `blk` as one node on the split engine (functional.PreAttnBlockFn)."""
        lin, ln = self.pre_attn[4 * blk], self.pre_attn[4 * blk + 1]
        W, lb, g, b = (lin.weight if weight is None else weight), lin.bias, ln.weight, ln.bias
        if perm is not None:
            W, lb, g, b = self.permuted(W, 0), self.permuted(lb, 0), self.permuted(g, 0), self.permuted(b, 0)
        p, seed, keep = self._drop_cfg(blk, perm)
        if keep is not None:
            keep = keep.reshape(-1, keep.shape[-1])
        gb, rg, cu = group_bias if group_bias is not None else (None, None, None)
        return MF.preattn_block(x, x_scale, W, lb, g, b, ln.eps, p, seed, keep, want_fp32, gb, rg, cu)

    def _act(self, x, ln, blk, perm=None, lin_bias=None):
        """(+ bias of the preceding Linear) -> LayerNorm -> GELU -> Dropout(.1) of block `blk` in ONE fused HIP pass each
        way (functional.ln_gelu_drop); the Linear itself runs bias-free."""
        g, b = (ln.weight, ln.bias) if perm is None else (self.permuted(ln.weight, 0), self.permuted(ln.bias, 0))
        if lin_bias is not None and perm is not None:
            lin_bias = self.permuted(lin_bias, 0)
        p, seed, keep = self._drop_cfg(blk, perm)
        return MF.ln_gelu_drop(x if x.dtype == torch.bfloat16 else x.float(), g, b, ln.eps, p, seed, keep, lin_bias)

    def embed_tokens_headmajor(self, bags: torch.Tensor, return_image: bool = False, want_fp32: bool = True, stain=None):
        """pre_attn(bags) with the 2048 output channels in head-major order: [BM, N, H*512]  (with return_image: (E, image of E or
        None) -- in the split GEMM mode the last block's kernel writes the split image the gate contractions read).  want_fp32 = False
        (with return_image, split GEMM mode only): no fp32 copy of E is written -- the returned "E" IS the image tensor (an opaque
        float32 [BM, N, H*512] tensor that only functional.attn_pool(..., e_only_image=True) can read; `image_only(E, e_img)` tells).

        Under torch.autocast(bfloat16) -- the reference's `precision: bfloat16` runs (trainer.py:101-103) -- the
        activations are kept in bf16 end to end (Linear outputs, the fused LayerNorm-GELU-Dropout input/output and E):
        the bf16 mode of the HIP kernels; LayerNorm statistics, GELU and every reduction stay fp32 inside the kernels."""
        pa = self.pre_attn
        perm = self._perm
        # stain = (e [G, 32], row_group int32 [T], cu_groups int64 [G + 1]): MADELEINE's stain encoding concatenates ONE 32-vector per bag to
        # every patch feature in front of the first Linear (Model.py:125-132, :351).  [x | e_g] W^T = x Wx^T + e_g We^T: on the split engine the
        # concat never exists -- the bag's row e_g We^T ([G, 512], a small HIP Linear with autograd) enters the first product as a per-group
        # bias (mdl_split_gemm_nt_group_bias) and its gradient comes back from the grouped LayerNorm backward.  The other engines (bf16, exact
        # fp32) add the row in a grouped LayerNorm-GELU-Dropout pass (round 6); only more than 2048 bags per call still concatenate.
        group_bias = None
        if stain is not None:
            e_rows, row_group, cu_groups = stain
            d_feat = bags.shape[-1]
            x_flat = bags.reshape(-1, d_feat)
            if (not bf16_mode()) and MF.preattn_split_supported(x_flat, d_feat) and pa[0].weight.shape[0] % 32 == 0 \
                    and e_rows.shape[1] % 4 == 0 and e_rows.shape[0] <= 2048:
                Wfull = pa[0].weight
                img, sc, _ = self._block_split(x_flat.float().contiguous(), None, 0, weight=Wfull[:, :d_feat],
                                               group_bias=(MF.linear(e_rows.float(), Wfull[:, d_feat:].contiguous()), row_group, cu_groups))
                img, sc, _ = self._block_split(img, sc, 1)
                keep_fp32 = want_fp32 or not return_image
                img, sc, E = self._block_split(img, sc, 2, perm, want_fp32=keep_fp32)
                E = (E if keep_fp32 else img).view(*bags.shape[:-1], img.shape[-1])
                return (E, (img, sc)) if return_image else E
            Wfull = pa[0].weight
            if cu_groups is not None and Wfull.shape[0] in (256, 512, 1024) and e_rows.shape[0] <= 2048 \
                    and not os.environ.get("MADELEINE_STAIN_CONCAT"):      # (A/B switch: the round-5 concatenation)
                # bf16 / exact-fp32 engines (round 6): the same fold with the bag's row as a per-group bias of the fused
                # LayerNorm-GELU-Dropout pass (functional.ln_gelu_drop_groups) -- their GEMM epilogues add no bias
                lowp = bf16_mode()          # (read before autocast is switched off for the kernels' own dtype handling)
                with torch.autocast(device_type="cuda", enabled=False):
                    gb = MF.linear(e_rows.float(), Wfull[:, d_feat:].contiguous()) + pa[0].bias          # [G, 512]
                    Wx = Wfull[:, :d_feat]
                    xin = x_flat
                    if d_feat % 32:
                        padc = 32 - d_feat % 32
                        xin, Wx = F.pad(xin, (0, padc)), F.pad(Wx, (0, padc))
                    xin = xin.to(torch.bfloat16) if lowp else xin.float()
                    p, seed, keep = self._drop_cfg(0, None)
                    if keep is not None:
                        keep = keep.reshape(-1, keep.shape[-1])
                    x = MF.ln_gelu_drop_groups(MF.linear(xin, Wx.contiguous()), pa[1].weight, pa[1].bias, pa[1].eps, p, seed, keep, gb,
                                               cu_groups)
                    x = self._act(MF.linear(x, pa[4].weight), pa[5], 1, None, pa[4].bias)
                    E = self._act(MF.linear(x, self.permuted(pa[8].weight, 0)), pa[9], 2, perm, pa[8].bias)
                E = E.view(*bags.shape[:-1], E.shape[-1])
                return (E, None) if return_image else E
            enc = e_rows.index_select(0, row_group.long()).view(*bags.shape[:-1], e_rows.shape[1])
            bags = torch.cat([bags, enc.to(bags.dtype)], dim=-1)
        # Any patch_embedding_dim (Model.py:351 is a plain nn.Linear): the kernels contract over 32-column blocks, so an input width that
        # is not a multiple of 32 is zero-padded -- features and the columns of the first weight alike, which leaves every product
        # unchanged (exact) and costs one padded copy of the bags per forward; autograd slices the weight gradient back.  The usual
        # encoders (512 / 768 / 1024 / 1536 / 2048 / 2560, + 32 stain channels) never take this branch.
        W0 = pa[0].weight
        k_in = bags.shape[-1]
        if k_in % 32:
            padc = 32 - k_in % 32
            bags = F.pad(bags, (0, padc))
            W0 = F.pad(W0, (0, padc))
        if bf16_mode():
            with torch.autocast(device_type="cuda", enabled=False):
                bf = torch.bfloat16
                x = self._act(MF.linear(bags.to(bf), W0), pa[1], 0, None, pa[0].bias)
                x = self._act(MF.linear(x, pa[4].weight), pa[5], 1, None, pa[4].bias)
                E = self._act(MF.linear(x, self.permuted(pa[8].weight, 0)), pa[9], 2, perm, pa[8].bias)
                return (E, None) if return_image else E
        x2d = bags.reshape(-1, bags.shape[-1])
        if MF.preattn_split_supported(x2d, x2d.shape[-1]) and pa[0].weight.shape[0] % 32 == 0:
            # split GEMM mode: three fused blocks; the activations between them exist as split images only
            img, sc, _ = self._block_split(x2d.float().contiguous(), None, 0, weight=W0)
            img, sc, _ = self._block_split(img, sc, 1)
            keep_fp32 = want_fp32 or not return_image
            img, sc, E = self._block_split(img, sc, 2, perm, want_fp32=keep_fp32)
            E = (E if keep_fp32 else img).view(*bags.shape[:-1], img.shape[-1])
            return (E, (img, sc)) if return_image else E
        x = self._act(MF.linear(bags.float(), W0), pa[1], 0, None, pa[0].bias)
        x = self._act(MF.linear(x, pa[4].weight), pa[5], 1, None, pa[4].bias)
        E = self._act(MF.linear(x, self.permuted(pa[8].weight, 0)), pa[9], 2, perm, pa[8].bias)
        return (E, None) if return_image else E

    @staticmethod
    def image_only(E, e_img) -> bool:
        """True when `E` of embed_tokens_headmajor(..., want_fp32=False) is the image tensor itself."""
        return e_img is not None and E.data_ptr() == e_img[0].data_ptr()

    def gate_params_stacked(self):
        ps = [h.gate_params() for h in self.attn]
        return tuple(torch.stack([p[i] for p in ps]) for i in range(5)) + (torch.cat([p[5] for p in ps]),)

    def _gate_dropout(self, shape_bn):
        """(p, seed, keep_a, keep_b) for this forward; masks are uint8 [T,H,512]."""
        p = self.attn[0].dropout_p() if len(self.attn) else 0.0
        if p == 0.0:
            return 0.0, 0, None, None
        inj = self._injected_keep
        if inj is not None:
            ka = torch.stack([g[0] for g in inj["gate"]], dim=2)  # [BM,N,H,512]
            kb = torch.stack([g[1] for g in inj["gate"]], dim=2)
            T = shape_bn[0] * shape_bn[1]
            return p, 0, ka.reshape(T, self.n_heads, MF.HID).to(torch.uint8).contiguous(), \
                kb.reshape(T, self.n_heads, MF.HID).to(torch.uint8).contiguous()
        return p, MF.new_dropout_seed(), None, None

    def pool_headmajor(self, E_hm: torch.Tensor, views=(), tok_proj=None, e_img=None):
        """E_hm [BM,N,H*512] -> (pooled_hm [BM,(1+V,)H*512], raw scores [BM,N,H]) through the fused HIP path; `views` = V int32
        token-index lists pooled in the same autograd node (no index_select copies of E).  tok_proj = (W [P,H*512] head-major
        columns, bias): the token projection [BM,N,P] comes out of the same node (third result), see functional.AttnPoolFn."""
        for h in self.attn:
            h._check_geometry()
        BM, N, _ = E_hm.shape
        wa, ba, wb, bb, wc, bc = self.gate_params_stacked()
        p, seed, ka, kb = self._gate_dropout((BM, N))
        out = MF.attn_pool(E_hm, wa, ba, wb, bb, wc, bc, p, seed, ka, kb, views=views, tok_proj=tok_proj, e_img=e_img,
                           e_only_image=self.image_only(E_hm, e_img))
        if tok_proj is None:
            return out[0], out[1].view(BM, N, self.n_heads)
        return out[0], out[1].view(BM, N, self.n_heads), out[2].view(BM, N, -1)

    def pool_headmajor_ragged(self, E_hm: torch.Tensor, cu_seqlens: torch.Tensor, max_len: int, e_img=None, tok_proj=None, rviews=None):
        """Packed E_hm [T,H*512] + cu_seqlens int64 [n_bags+1] -> (pooled_hm [n_bags,H*512], raw scores [T,H]) (+ the token projections
        [T,P] with tok_proj = (W, bias), see pool_headmajor).  rviews = (perm, vcu, max_view_len) on the device (ragged_view_plan): pooled_hm
        is [n_bags, 3, H*512], the whole bag and its two halves with the raw scores re-softmaxed over each half, whatever the activation."""
        for h in self.attn:
            h._check_geometry()
        wa, ba, wb, bb, wc, bc = self.gate_params_stacked()
        p, seed, ka, kb = self._gate_dropout((E_hm.shape[0], 1))
        act = self.attn[0].activation
        if act != 'softmax':
            # relu / leaky_relu / sigmoid attention (abmil.py:56-61) on ragged bags: element-wise weights, no normalisation over the patch
            # axis -- raw scores from the gate kernel, the activation in torch, un-normalised weighted pooling over cu_seqlens
            # (mdl_abmil_wpool_*), as the dense path does (forward_headmajor_from_tokens)
            if self.image_only(E_hm, e_img) or tok_proj is not None:
                raise ValueError("activation=%r pools the token embeddings themselves: call embed_tokens_headmajor(want_fp32=True) and project "
                                 "the tokens separately" % act)
            scores = MF.gate_scores(E_hm, wa, ba, wb, bb, wc, bc, p, seed, ka, kb)          # [T, H]
            pooled = MF.weighted_pool(E_hm, activate(scores, act), cu_seqlens, max_len)
            if rviews is not None:   # (Model.py:435 re-softmaxes the raw scores over each half for every activation)
                pooled = torch.cat([pooled.unsqueeze(1), MF.ragged_view_pool(E_hm, scores, cu_seqlens, *rviews)], dim=1)
            return pooled, scores
        return MF.attn_pool(E_hm, wa, ba, wb, bb, wc, bc, p, seed, ka, kb, cu_seqlens, max_len, e_img=e_img, tok_proj=tok_proj,
                            e_only_image=self.image_only(E_hm, e_img), rviews=rviews)

    def _scores_only(self, E_hm):
        BM, N, _ = E_hm.shape
        wa, ba, wb, bb, wc, bc = self.gate_params_stacked()
        p, seed, ka, kb = self._gate_dropout((BM, N))
        return MF.gate_scores(E_hm.view(BM * N, -1), wa, ba, wb, bb, wc, bc, p, seed, ka, kb).view(BM, N, self.n_heads)

    def _to_reference_tokens(self, E_hm):
        BM, N, _ = E_hm.shape
        return E_hm.view(BM, N, self.n_heads, -1).permute(0, 1, 3, 2)  # [BM,N,512,H] (strided view)

    def _to_reference_slide(self, pooled_hm):
        lead = pooled_hm.shape[:-1]
        return pooled_hm.view(*lead, self.n_heads, -1).transpose(-1, -2).contiguous()  # [...,512,H]

    def forward_headmajor(self, bags, n_views=1, tok_proj=None, need_tokens=True, stain=None):
        """Fast path used by MADELEINE: returns (pooled_hm [BM,(V,)H*512], E_hm, raw scores [BM,N,H]) and, with tok_proj = (W, bias)
        of a Linear over the head-major token embeddings (MADELEINE's token_projector), its output [BM,N,P] as a fourth result.
        need_tokens = False: the caller does not read E_hm (it is returned as None when the split GEMM mode then keeps E as an image
        only: its LayerNorm kernel writes 4 instead of 8 bytes per element and the pooling kernels read the image)."""
        if self.agg_type != 'regular':
            raise NotImplementedError('Agg type not supported. Options are "regular".')
        act = self.attn[0].activation
        fused = act == 'softmax' and n_views == 1
        tok_on_image = tok_proj is None or MF.split_linear_supported(bags.numel() // bags.shape[-1], tok_proj[0].shape[0],
                                                                     tok_proj[0].shape[1])
        E, e_img = self.embed_tokens_headmajor(bags, return_image=True, want_fp32=need_tokens or not fused or not tok_on_image, stain=stain)
        if self.image_only(E, e_img):
            out = self.pool_headmajor(E, tok_proj=tok_proj, e_img=e_img)
            return (out[0], None, out[1]) + tuple(out[2:])
        if tok_proj is not None:
            if fused:
                pooled, scores, tok = self.pool_headmajor(E, tok_proj=tok_proj, e_img=e_img)   # one autograd node for both consumers of E
                return pooled, E, scores, tok
            with torch.autocast(device_type="cuda", enabled=False):
                tok = MF.linear(E, tok_proj[0], tok_proj[1])
            return self.forward_headmajor_from_tokens(E, n_views, e_img) + (tok,)
        return self.forward_headmajor_from_tokens(E, n_views, e_img)

    def forward_headmajor_from_tokens(self, E, n_views=1, e_img=None):
        act = self.attn[0].activation
        if act == 'softmax' and n_views != 1:
            # intra-modality views (Model.py:419-440): two random halves of the token axis (numpy RNG, as the reference),
            # raw scores re-softmaxed per subset -- pooled by index list inside the fused A2+A3 node
            all_indices = np.arange(E.shape[1])
            np.random.shuffle(all_indices)
            mid = len(all_indices) // 2
            views = tuple(MF.h2d(torch.as_tensor(idx, dtype=torch.int32), E.device) for idx in (all_indices[:mid], all_indices[mid:]))
            pooled, scores = self.pool_headmajor(E, views, e_img=e_img)
            return pooled, E, scores
        if act == 'softmax':
            pooled, scores = self.pool_headmajor(E, e_img=e_img)
        else:
            # non-default activations (abmil.py:56-61): scores from the HIP gate kernel, the elementwise activation in torch,
            # the un-normalised weighted pooling in the HIP pool kernels' linear mode (mdl_abmil_wpool_*)
            scores = self._scores_only(E)
            w = activate(scores.unsqueeze(2), act).squeeze(2)  # elementwise; dim=1 only matters for softmax
            pooled = MF.weighted_pool(E, w)
        if n_views == 1:
            return pooled, E, scores
        # intra-modality views (Model.py:419-440): two random halves, raw scores re-softmaxed per subset
        N = E.shape[1]
        all_indices = np.arange(N)
        np.random.shuffle(all_indices)
        mid = len(all_indices) // 2
        views = [pooled.unsqueeze(1)]
        for idx in (all_indices[:mid], all_indices[mid:]):
            ti = MF.h2d(torch.as_tensor(idx, dtype=torch.long), E.device)
            views.append(MF.softmax_pool(E.index_select(1, ti), scores.index_select(1, ti).contiguous()).unsqueeze(1))
        return torch.cat(views, dim=1), E, scores

    # ------------------------------------------------------------------ reference-shaped API
    def forward(self, bags: torch.Tensor, return_attention: bool = False, return_preattn_feats: bool = False, n_views=1):
        """Model.py:375-451.  slide embeddings [BM,(V,)512,H]; raw attention [BM,N,1,H]; tokens [BM,N,512,H]."""
        pooled, E, scores = self.forward_headmajor(bags, n_views, need_tokens=return_preattn_feats)
        slide = self._to_reference_slide(pooled)
        if return_attention:
            return slide, scores.unsqueeze(2)
        if return_preattn_feats:
            return slide, self._to_reference_tokens(E)
        return slide


class MADELEINE(nn.Module):
    def __init__(self, config, stain_encoding=False):
        super().__init__()
        self.config = config
        self.modalities = config.MODALITIES
        self.stain_encoding = stain_encoding
        # opt-in: encode each distinct all-zero bag of an absent stain once, see _absent_stain_plan
        self.skip_absent_stains = bool(getattr(config, "skip_absent_stains", False))
        if self.stain_encoding:
            self.stain_encoding_dim = 32
            self.embedding = nn.Embedding(len(self.modalities), self.stain_encoding_dim)
        else:
            self.stain_encoding_dim = 0
        if self.config.wsi_encoder == "abmil":
            # (any patch_embedding_dim: widths that are not a multiple of 32 are zero-padded at the encoder's entry, ABMILEmbedder.
            # embed_tokens_headmajor -- round 4 raised here)
            pre_params = {'input_dim': self.config.patch_embedding_dim + self.stain_encoding_dim,
                          'hidden_dim': self.config.wsi_encoder_hidden_dim}
            attention_params = {'model': 'ABMIL',
                                'params': {'input_dim': self.config.wsi_encoder_hidden_dim, 'hidden_dim': 512,
                                           'dropout': True, 'activation': self.config.activation,
                                           'n_heads': self.config.n_heads, 'n_classes': 1}}
            width = attention_params['params']['hidden_dim'] * attention_params['params']['n_heads']
            self.token_projector = nn.Linear(width, 128)
            self.wsi_embedders = ABMILEmbedder(pre_params, attention_params)
            self.projector = nn.Linear(width, attention_params['params']['hidden_dim'])
        else:
            raise ValueError('Unsupported wsi_encoder. Must be "abmil". Now is {}.'.format(self.config.wsi_encoder))

    # ------------------------------------------------------------------ helpers
    def _project_slide(self, pooled_hm):
        """projector Linear(2048, 512) (Model.py:145) on the head-major pooled embeddings (columns permuted to match)."""
        with torch.autocast(device_type="cuda", enabled=False):   # fp32 pooled embeddings: the fp32 kernel in both modes
            return MF.linear(pooled_hm, self.wsi_embedders.permuted(self.projector.weight, 1), self.projector.bias)

    def _project_tokens(self, E_hm):
        """token_projector Linear(2048, 128) (Model.py:140) on the head-major token embeddings."""
        with torch.autocast(device_type="cuda", enabled=False):
            return MF.linear(E_hm, self.wsi_embedders.permuted(self.token_projector.weight, 1), self.token_projector.bias)

    def _stain_groups(self, idx, n_bags, n_tokens, device):
        """(embedding rows [n_bags, 32], row_group int32 [n_bags * n_tokens], cu_groups int64 [n_bags + 1]) for dense bags of n_tokens rows:
        what ABMILEmbedder.embed_tokens_headmajor(stain=...) folds into the first Linear instead of a concatenated copy of the bags."""
        e_rows = self.embedding(MF.h2d(idx, device))
        row_group = torch.arange(n_bags * n_tokens, device=device, dtype=torch.int32).div_(n_tokens, rounding_mode="floor")
        cu = torch.arange(n_bags + 1, device=device, dtype=torch.int64) * n_tokens
        return e_rows, row_group, cu

    @staticmethod
    def _absent_stain_plan(modality_labels, input_key_of_row):
        """the dataset fills a missing stain with an all-zero bag (wsi_dataset.py:66) that the
        reference still pushes through the whole encoder (~27 % of ACROBAT's bags) although the losses never read it.
        All-zero bags with the same stain-encoding index (`input_key_of_row`; one key for all without stain encoding) are
        IDENTICAL inputs, so one representative per key is encoded and its outputs are shared.  Returns (compact, expand): rows of the flattened [B*M] batch to encode, and for
        every original row the position of its source in the compact list; (None, None) when nothing is absent.
        In eval mode every output equals the reference's; in train mode the absent rows share one dropout draw instead of
        having one each -- in outputs that no loss term reads (trainer.py:27-29 gates on the same labels)."""
        present = modality_labels.detach().cpu().reshape(-1).bool()
        if bool(present.all()):
            return None, None
        rows = torch.arange(present.numel())
        compact = rows[present].tolist()
        position = {r: i for i, r in enumerate(compact)}
        representative = {}
        expand = []
        for r in rows.tolist():
            if r in position:
                expand.append(position[r])
                continue
            key = int(input_key_of_row[r])
            if key not in representative:
                representative[key] = len(compact)
                compact.append(r)
            expand.append(representative[key])
        return torch.tensor(compact, dtype=torch.long), torch.tensor(expand, dtype=torch.long)

    @staticmethod
    def _require_single_modality(n_mod):
        # the reference's eval / attention branches reshape with .view(bs*n_mod, d_out*n_heads) on a [bs,512,H]
        # tensor (Model.py:194-196, :210-212): they raise for n_mod != 1.  Same contract here.
        if n_mod != 1:
            raise RuntimeError("MADELEINE.forward(train=False) expects data['feats'] of shape [B, 1, N, D] "
                               "(one modality per call), got n_mod=%d" % n_mod)

    # ------------------------------------------------------------------ public API
    def encode_he(self, feats, device):
        """Model.py:97-107: [B,N,D] -> [B,512]."""
        feats = feats.to(device)
        pooled, _, _ = self.wsi_embedders.forward_headmajor(feats, need_tokens=False)
        return self._project_slide(pooled)

    def encode_he_bags(self, bags, device):
        """encode_he (Model.py:97-107) for SEVERAL bags of different lengths in one launch set: `bags` = list of [N_i, D] (or [1, N_i, D])
        tensors -> [len(bags), 512].  The tokens are packed [sum N_i, D] and pooled through the ragged kernels (cu_seqlens); every kernel
        of the path is row-local and the pooling merges a bag's 128-token chunks in bag order, so each row equals encode_he of that bag
        alone BIT FOR BIT as long as every bag is on the same kernel path alone as in the pack (more than 256 patches: the large-M
        engines; run_inference sends smaller bags one by one).  For the extraction loop (utils.run_inference): one bag per call leaves a
        30,000-patch bag on 235 pooling workgroups and the host bound by ~40 launches per bag.  This is the torch.cat of the bags and
        the upload of cu_seqlens, then encode_packed."""
        flat = [b.reshape(-1, b.shape[-1]) for b in bags]
        lens = tuple(int(x.shape[0]) for x in flat)
        x = flat[0].to(device) if len(flat) == 1 else torch.cat([f.to(device) for f in flat], dim=0)
        cu_d = None
        if not self._encodes_bag_by_bag(len(lens)):
            cu = torch.zeros(len(lens) + 1, dtype=torch.int64)
            cu[1:] = torch.cumsum(torch.tensor(lens, dtype=torch.int64), 0)
            cu_d = MF.h2d(cu, device)
        return self.encode_packed((x, cu_d, lens), device)

    def _encodes_bag_by_bag(self, n_bags):
        """encode_packed's per-bag route: the ragged pooling kernels serve the softmax activation, and one bag is encode_he's own case."""
        return self.wsi_embedders.attn[0].activation != 'softmax' or n_bags == 1

    def encode_packed(self, packed, device):
        """encode_he_bags for tokens that are ALREADY packed: `packed` is a PackedBags (DeviceSlideStore.pack_modality) or (tokens
        [sum N_i, D], cu_seqlens [R + 1] int64 on the device, the host tuple of the R lengths) -> [R, 512].  The kernels and their order
        are encode_he_bags', without the torch.cat and without an upload: nothing is built on the host.  One bag, and the non-softmax
        activations, go bag by bag through encode_he on slices of the tokens (cu_seqlens is then not read and may be None)."""
        tokens, cu_d, lens = (packed.tokens, packed.cu_seqlens, packed.lens) if hasattr(packed, "tokens") else packed
        lens = [int(n) for n in lens]
        if tokens.dim() != 2 or not lens or min(lens) < 1 or tokens.shape[0] != sum(lens):
            raise ValueError("encode_packed needs tokens [sum(lens), D] and at least one bag, every bag of at least one row")
        tokens = tokens.to(device)
        if self._encodes_bag_by_bag(len(lens)):
            ends = np.cumsum(lens).tolist()
            return torch.cat([self.encode_he(tokens[e - n:e].unsqueeze(0), device) for n, e in zip(lens, ends)])
        if cu_d is None or cu_d.numel() != len(lens) + 1:
            raise ValueError("encode_packed needs cu_seqlens [len(lens) + 1] on the device")
        emb = self.wsi_embedders
        E, e_img = emb.embed_tokens_headmajor(tokens, return_image=True, want_fp32=False)
        pooled, _ = emb.pool_headmajor_ragged(E, cu_d.to(device), max(lens), e_img=e_img)
        return self._project_slide(pooled)

    def attend_packed(self, packed, device, stain_idx=None):
        """encode_packed with the attention kept: -> (embeds [R, 512], raw scores [T, H]), row t of `raw` the scores of packed token t in
        every head, before the activation (what forward(..., return_attention=True) returns for a dense H&E batch, Model.py:205-216).
        The kernels and their order are encode_packed's -- the bag-by-bag route for one bag and for the non-softmax activations
        included -- so `embeds` is encode_packed's result.  With stain_encoding=True the eval branch's rule applies (Model.py:162-203):
        every bag of the pack gets embedding(stain_idx), the TRUE stain index (default 0), not the train branch's r // B; it is folded
        in through the per-group route of embed_tokens_headmajor (the engines that cannot fold it concatenate, as in training).
        stain_idx on a model without stain encoding is ignored, as custom_stain_idx is in the reference.  functional.attn_softmax /
        attn_rank turn `raw` into attention maps, percentile ranks and top-k patches."""
        tokens, cu_d, lens = (packed.tokens, packed.cu_seqlens, packed.lens) if hasattr(packed, "tokens") else packed
        lens = [int(n) for n in lens]
        if tokens.dim() != 2 or not lens or min(lens) < 1 or tokens.shape[0] != sum(lens):
            raise ValueError("attend_packed needs tokens [sum(lens), D] and at least one bag, every bag of at least one row")
        tokens = tokens.to(device)
        emb = self.wsi_embedders
        R, H = len(lens), emb.n_heads
        key = 0 if stain_idx is None else int(stain_idx)
        if self.stain_encoding and not 0 <= key < len(self.modalities):
            raise IndexError("attend_packed: stain_idx must be in [0, %d) (got %r)" % (len(self.modalities), stain_idx))
        if self._encodes_bag_by_bag(R):
            embeds, raws = [], []
            for n, e in zip(lens, np.cumsum(lens).tolist()):
                stain = self._stain_groups(torch.full((1,), key, dtype=torch.long), 1, n, device) if self.stain_encoding else None
                pooled, _, scores = emb.forward_headmajor(tokens[e - n:e].unsqueeze(0), need_tokens=False, stain=stain)
                embeds.append(self._project_slide(pooled))
                raws.append(scores.reshape(n, H))
            return torch.cat(embeds), torch.cat(raws)
        if cu_d is None or cu_d.numel() != R + 1:
            raise ValueError("attend_packed needs cu_seqlens [len(lens) + 1] on the device")
        cu_d = cu_d.to(device)
        stain = None
        if self.stain_encoding:
            row_bag = getattr(packed, "row_bag", None)
            if row_bag is None:
                row_bag = MF.h2d(torch.repeat_interleave(torch.arange(R, dtype=torch.int32), torch.tensor(lens)), device)
            stain = (self.embedding(MF.h2d(torch.full((R,), key, dtype=torch.long), device)), row_bag.to(device), cu_d)
        E, e_img = emb.embed_tokens_headmajor(tokens, return_image=True, want_fp32=False, stain=stain)
        pooled, scores = emb.pool_headmajor_ragged(E, cu_d, max(lens), e_img=e_img)
        return self._project_slide(pooled), scores.reshape(tokens.shape[0], H)

    def decision_rows(self, W, b=None):
        """(W [C, d] fp32, b [C] fp32) on the projector's device from what slide_directions accepts.  ValueError for another shape, a
        width other than the projector's output, or a bias that is not one value per row."""
        proj = self.projector
        d, dev = proj.out_features, proj.weight.device
        W = torch.as_tensor(W, dtype=torch.float32, device=dev)
        if W.dim() == 1:
            W = W.unsqueeze(0)
        if W.dim() != 2 or W.shape[0] < 1:
            raise ValueError("slide_directions needs W [d] or [C, d] (got %s)" % (tuple(W.shape),))
        if W.shape[1] != d:
            raise ValueError("slide_directions: W is %d wide, the projector's output is %d" % (W.shape[1], d))
        C = W.shape[0]
        bias = torch.zeros(C, device=dev) if b is None else torch.as_tensor(b, dtype=torch.float32, device=dev).reshape(-1)
        if bias.numel() == 1 and C > 1:
            bias = bias.expand(C)
        if bias.numel() != C:
            raise ValueError("slide_directions: b must hold one value per row of W (%d, got %d)" % (C, bias.numel()))
        return W.contiguous(), bias.contiguous()

    def slide_directions(self, W, b=None):
        """(U [C, H * 512] head-major, const [C]) of the linear decision z = W . slide_embedding + b: U = W . P_hm with P_hm the
        projector's weight with head-major columns, const = W . projector.bias + b, so that z_c = sum_t sum_h a[t, h] <U[c, h], E[t, h]>
        + const_c exactly (include/madeleine_amd_explain.h).  W: [d], [C, d] or a slice of probe.fit_logistic's [P, cols, d] /
        survival.fit_cox's [P, d] weights, d the projector's output width; b: None, a number, [C] or the matching slice of the
        biases.  fp32, without autograd, through functional.linear (no library GEMM).  ValueError for another shape or width."""
        W, bias = self.decision_rows(W, b)
        proj, d = self.projector, self.projector.out_features
        with torch.no_grad(), torch.autocast(device_type="cuda", enabled=False):
            # one product for both: the rows of [P_hm^T ; projector.bias ; 0 0 0] against W (zero rows: a row count in fours)
            p_hm = self.wsi_embedders.permuted(proj.weight, 1)
            rows = torch.cat([p_hm.t(), proj.bias.unsqueeze(0), proj.bias.new_zeros(3, d)]).contiguous()
            out = MF.linear(W.contiguous(), rows)
            n = proj.in_features
            return out[:, :n].contiguous(), out[:, n] + bias

    def explain_packed(self, packed, device, U, stain_idx=None, per_head=False):
        """attend_packed with the token embeddings contracted against the decision directions U [C, H * 512] of slide_directions where
        they are produced: -> (embeds [R, 512], raw scores [T, H], attention [T, H], contribution [T, C][, per_head [T, H, C]]), with
        contribution[t, c] the signed share of packed token t in decision column c (functional.attn_contrib), so that per bag
        sum_t contribution + const = W . embeds + b.  The routes, the stain rule and the argument checks are attend_packed's; E is asked
        for itself (fp32, or bf16 under autocast) and dropped when the call returns.  The attention is formed from the scores of this
        call: functional.attn_softmax over the pack's cu_seqlens (built from the lengths where the bag-by-bag route got none), or
        abmil.activate for the relu, leaky_relu and sigmoid activations.  `embeds` are the embeddings the contributions decompose."""
        tokens, cu_d, lens = (packed.tokens, packed.cu_seqlens, packed.lens) if hasattr(packed, "tokens") else packed
        lens = [int(n) for n in lens]
        if tokens.dim() != 2 or not lens or min(lens) < 1 or tokens.shape[0] != sum(lens):
            raise ValueError("explain_packed needs tokens [sum(lens), D] and at least one bag, every bag of at least one row")
        tokens = tokens.to(device)
        emb = self.wsi_embedders
        R, H = len(lens), emb.n_heads
        if U.dim() != 2 or U.shape[1] != H * MF.HID:
            raise ValueError("explain_packed needs U [C, %d] (slide_directions; got %s)" % (H * MF.HID, tuple(U.shape)))
        key = 0 if stain_idx is None else int(stain_idx)
        if self.stain_encoding and not 0 <= key < len(self.modalities):
            raise IndexError("explain_packed: stain_idx must be in [0, %d) (got %r)" % (len(self.modalities), stain_idx))
        act = emb.attn[0].activation
        by_bag = self._encodes_bag_by_bag(R)
        if cu_d is None and by_bag:
            cu = torch.zeros(R + 1, dtype=torch.int64)
            cu[1:] = torch.cumsum(torch.tensor(lens, dtype=torch.int64), 0)
            cu_d = MF.h2d(cu, device)
        if cu_d is None or cu_d.numel() != R + 1:
            raise ValueError("explain_packed needs cu_seqlens [len(lens) + 1] on the device")
        cu_d = cu_d.to(device)

        def weights(scores, cu):
            return MF.attn_softmax(scores, cu)[0] if act == 'softmax' else activate(scores, act)

        if by_bag:
            embeds, raws, attns, outs = [], [], [], []
            for r, (n, e) in enumerate(zip(lens, np.cumsum(lens).tolist())):
                stain = self._stain_groups(torch.full((1,), key, dtype=torch.long), 1, n, device) if self.stain_encoding else None
                E, e_img = emb.embed_tokens_headmajor(tokens[e - n:e].unsqueeze(0), return_image=True, want_fp32=True, stain=stain)
                pooled, _, scores = emb.forward_headmajor_from_tokens(E, 1, e_img)
                scores = scores.reshape(n, H).float().contiguous()
                attn = weights(scores, cu_d[r:r + 2] - cu_d[r:r + 1])      # a bag's softmax depends on its own scores alone
                embeds.append(self._project_slide(pooled))
                raws.append(scores)
                attns.append(attn)
                outs.append(MF.attn_contrib(E.detach().view(n, -1), attn, U, per_head))
                del E, e_img
            res = (torch.cat(embeds), torch.cat(raws), torch.cat(attns))
            if per_head:
                return res + (torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs]))
            return res + (torch.cat(outs),)
        stain = None
        if self.stain_encoding:
            row_bag = getattr(packed, "row_bag", None)
            if row_bag is None:
                row_bag = MF.h2d(torch.repeat_interleave(torch.arange(R, dtype=torch.int32), torch.tensor(lens)), device)
            stain = (self.embedding(MF.h2d(torch.full((R,), key, dtype=torch.long), device)), row_bag.to(device), cu_d)
        E, e_img = emb.embed_tokens_headmajor(tokens, return_image=True, want_fp32=True, stain=stain)
        pooled, scores = emb.pool_headmajor_ragged(E, cu_d, max(lens), e_img=e_img)
        scores = scores.reshape(tokens.shape[0], H).float().contiguous()
        attn = weights(scores, cu_d)
        out = MF.attn_contrib(E.detach(), attn, U, per_head)
        return (self._project_slide(pooled), scores, attn) + (out if per_head else (out,))

    def forward_ragged(self, bags, device, n_loss_tokens=None, n_views=1, modality_labels=None):
        """Variable-length bags (BASELINE config 5) -- NEW functionality: the reference can only torch.stack equal-N
        bags (wsi_dataset.py:89-92).  `bags` is a list over cases of lists over modalities of [N_bm, D] tensors.
        Semantics = the train branch applied to each bag on its own (incl. the stain-encoding row quirk r // B of
        Model.py:125-131); the pooling kernels take the packed tokens + cu_seqlens, nothing is padded.
        Returns the reference-shaped dicts, with token embeddings restricted to the first `n_loss_tokens` tokens of
        every bag -- all the local loss ever reads (GOT sub-samples randperm(k)[:256]).
        n_views != 1: the intra-modality views of Model.py:419-440 applied to each bag on its own (ragged_view_plan: one numpy shuffle
        per bag, in packed order); slide embeddings are then [B, 3, 512] ([B, 3, 512, M-1] for HE), as on the dense path.
        modality_labels [B, M] (the batch's own tensor): a bag labelled 0 (an absent stain, which the dataset fills with a 2-token zero
        bag and no loss reads) may be shorter than n_loss_tokens; its token rows past its length are zeros."""
        bs, n_mod = len(bags), len(bags[0])
        flat = [bags[b][m] for b in range(bs) for m in range(n_mod)]          # case-major rows, like .view(bs*n_mod,...)
        lens = [int(x.shape[0]) for x in flat]
        n_loss_tokens = self._check_bag_lens(lens, bs, n_mod, n_loss_tokens, modality_labels)
        x = torch.cat([f.to(device) for f in flat], dim=0)                     # packed [T, D]
        return self._forward_packed(x, lens, None, None, bs, n_mod, device, n_loss_tokens, n_views)

    def forward_packed(self, packed, device, n_loss_tokens=None, n_views=1, modality_labels=None):
        """forward_ragged on a batch that is already packed (DeviceSlideStore.pack / packed_batches: `packed` has tokens [T, D],
        cu_seqlens [R + 1] on the device, the host tuple lens and row_bag [T], R = B * M bags, case-major): no list of bags, no
        torch.cat, and the stain-encoding row map is packed.row_bag -- nothing of the size of the tokens is built on the host or
        uploaded.  Same semantics, arguments and outputs as forward_ragged."""
        lens = [int(n) for n in packed.lens]
        n_mod = len(self.modalities)
        if not lens or len(lens) % n_mod:
            raise ValueError("a packed batch needs B * M bags for M = %d modalities (got %d)" % (n_mod, len(lens)))
        bs = len(lens) // n_mod
        n_loss_tokens = self._check_bag_lens(lens, bs, n_mod, n_loss_tokens, modality_labels)
        if packed.tokens.dim() != 2 or packed.tokens.shape[0] != sum(lens) or packed.cu_seqlens.numel() != len(lens) + 1:
            raise ValueError("a packed batch needs tokens [sum(lens), D] and cu_seqlens [len(lens) + 1]")
        return self._forward_packed(packed.tokens.to(device), lens, packed.cu_seqlens.to(device), packed.row_bag.to(device), bs, n_mod,
                                    device, n_loss_tokens, n_views)

    @staticmethod
    def _check_bag_lens(lens, bs, n_mod, n_loss_tokens, modality_labels):
        """The ragged routes' checks of the bag lengths; returns n_loss_tokens (its default when None)."""
        if n_loss_tokens is None:
            # GOT draws token indices randperm(k)[:256] with k = the number of participating CASES (reference quirk, loss.py:282,
            # SURVEY.md section 8(a) G0): indices reach k - 1, so a batch of more than 256 cases needs that many tokens kept
            n_loss_tokens = max(256, bs)
        present = [True] * len(lens)
        if modality_labels is not None:
            present = [bool(v) for v in torch.as_tensor(modality_labels).detach().cpu().reshape(-1).tolist()]
            if len(present) != len(lens):
                raise ValueError("modality_labels must be [B, M] = [%d, %d]" % (bs, n_mod))
        short = [n for n, pr in zip(lens, present) if pr and n < n_loss_tokens]
        if short:
            raise ValueError("every bag needs at least n_loss_tokens=%d tokens (shortest has %d): the local loss reads token "
                             "indices up to min(batch, 256) - 1 of every bag" % (n_loss_tokens, min(short)))
        if min(lens) < 1:
            raise ValueError("every bag needs at least one token (an absent stain's bag included)")
        return n_loss_tokens

    def _forward_packed(self, x, lens, cu_d, row_bag, bs, n_mod, device, n_loss_tokens, n_views):
        """The body shared by forward_ragged and forward_packed: x [T, D] the packed tokens of the bs * n_mod bags of `lens` rows,
        cu_d / row_bag their device tables (None: built from lens and uploaded)."""
        rviews = ragged_view_plan(lens) if n_views != 1 else None     # (numpy's RNG, as the reference's view draw)
        cu = torch.zeros(len(lens) + 1, dtype=torch.int64)
        cu[1:] = torch.cumsum(torch.tensor(lens, dtype=torch.int64), 0)
        stain = None
        if self.stain_encoding:
            row_stain = torch.arange(bs * n_mod) // bs                          # the train-branch quirk
            # one embedding row per BAG; the bag of every packed token as an int32 map (folded into the first Linear on the split engine,
            # gathered + concatenated by the other engines: ABMILEmbedder.embed_tokens_headmajor)
            bag_of_tok = row_bag if row_bag is not None else \
                MF.h2d(torch.repeat_interleave(torch.arange(bs * n_mod, dtype=torch.int32), torch.tensor(lens)), device)
            stain = (self.embedding(MF.h2d(row_stain, device)), bag_of_tok, None)
        emb = self.wsi_embedders
        if cu_d is None:
            cu_d = MF.h2d(cu, device)
        if stain is not None:
            stain = (stain[0], stain[1], cu_d)
        pos = torch.arange(n_loss_tokens).unsqueeze(0)
        lens_t = torch.tensor(lens, dtype=torch.int64).unsqueeze(1)
        pad = None
        if min(lens) < n_loss_tokens:
            # absent bags shorter than n_loss_tokens: their rows past the end repeat the last token and are zeroed after the projection
            pad = MF.h2d((pos < lens_t).reshape(bs, n_mod, n_loss_tokens, 1).float(), device)
            pos = torch.minimum(pos, lens_t - 1)
        head = MF.h2d((cu[:-1].unsqueeze(1) + pos).reshape(-1), device)
        tp = (emb.permuted(self.token_projector.weight, 1), self.token_projector.bias)
        # Split GEMM mode: the token projection is part of the pooling node (every token, on the image of E) and the head tokens are
        # gathered from ITS output -- gathering rows of E instead makes autograd fill a zero [T, 2048] tensor and add it to the node's dE
        # (3 x 11 GB of traffic per config-5 step), and E need not exist in fp32 at all.
        fuse_tok = (not bf16_mode()) and MF.split_linear_supported(x.shape[0], tp[0].shape[0], tp[0].shape[1]) \
            and emb.attn[0].activation == 'softmax' and rviews is None
        # (the other activations pool fp32 tokens through the weighted-pooling kernels; the views read E in fp32 / bf16, as the dense
        # n_views = 3 path does)
        if rviews is not None:
            rviews = (MF.h2d(rviews[0], device), MF.h2d(rviews[1], device), rviews[2])
        E, e_img = emb.embed_tokens_headmajor(x, return_image=True, want_fp32=not fuse_tok, stain=stain)   # [T, H*512]
        if fuse_tok and e_img is not None:
            pooled, _, tok_all = emb.pool_headmajor_ragged(E, cu_d, max(lens), e_img=e_img, tok_proj=tp)
            tok = tok_all.index_select(0, head).view(bs, n_mod, n_loss_tokens, -1)          # [B,M,n,128]
        else:
            pooled, _ = emb.pool_headmajor_ragged(E, cu_d, max(lens), e_img=e_img, rviews=rviews)
            tok = self._project_tokens(E.index_select(0, head)).view(bs, n_mod, n_loss_tokens, -1)
        if pad is not None:
            tok = tok * pad
        slide = self._project_slide(pooled).view(bs, n_mod, -1, self.projector.weight.shape[0])   # [B,M,V,512]
        all_embeddings, all_token_embeddings = {}, {}
        slides, toks = slide.unbind(1), tok.unbind(1)   # (see forward: one stacked gradient instead of per-stain fills and adds)
        for idx, modality in enumerate(self.modalities):
            s, t = slides[idx], toks[idx]
            if modality == "HE":
                s = s.unsqueeze(3).expand(-1, -1, -1, n_mod - 1)
                t = t.unsqueeze(3).expand(-1, -1, -1, n_mod - 1)
            all_embeddings[modality] = s
            all_token_embeddings[modality] = t
        return all_embeddings, all_token_embeddings

    def forward(self, data, device, train=True, n_views=1, custom_stain_idx=None, return_attention=False):
        if 'packed' in data and 'feats' not in data:  # a ragged batch packed on the device (DeviceSlideStore.packed_batches)
            return self.forward_packed(data['packed'], device, n_views=n_views, modality_labels=data.get('modality_labels'))
        if 'bags' in data and 'feats' not in data:   # ragged extension (see forward_ragged); keeps DDP's forward hook path
            return self.forward_ragged(data['bags'], device, n_views=n_views, modality_labels=data.get('modality_labels'))
        all_wsi_feats = data['feats'].to(device)
        all_embeddings, all_token_embeddings = {}, {}
        emb = self.wsi_embedders

        if train:  # Model.py:120-159
            bs, n_mod, n_tokens, d_in = all_wsi_feats.shape
            x = all_wsi_feats.view(bs * n_mod, n_tokens, d_in)
            # reference quirk kept on purpose (Model.py:125-131): the stain-indicator list is stain-major while the
            # flattened rows are case-major, so row r gets embedding index r // bs.
            stain_of_row = torch.arange(bs * n_mod) // bs
            expand = None
            if self.skip_absent_stains and 'modality_labels' in data:
                compact, expand = self._absent_stain_plan(data['modality_labels'],
                                                          stain_of_row if self.stain_encoding else torch.zeros_like(stain_of_row))
                if expand is not None:   # encode every present bag + ONE all-zero bag per distinct input among the absent ones
                    x = x.index_select(0, MF.h2d(compact, device))
                    stain_of_row = stain_of_row[compact]
            stain = self._stain_groups(stain_of_row, x.shape[0], n_tokens, device) if self.stain_encoding else None
            # token_projector (Model.py:140) inside the pooling node: the two gradients of E are accumulated in the gate dX epilogue
            pooled, _, _, tok = emb.forward_headmajor(x, n_views=n_views, need_tokens=False, stain=stain, tok_proj=(
                emb.permuted(self.token_projector.weight, 1), self.token_projector.bias))   # tok [rows,N,128]
            slide = self._project_slide(pooled.view(x.shape[0], -1, pooled.shape[-1]))  # [rows,V,512]
            if expand is not None:       # absent rows take the outputs of their all-zero representative
                expand = MF.h2d(expand, device)
                tok, slide = tok.index_select(0, expand), slide.index_select(0, expand)
            tok = tok.view(bs, n_mod, n_tokens, -1)                                   # [B,M,N,128]
            slide = slide.view(bs, n_mod, -1, slide.shape[-1])
            # unbind, not M selects: its backward stacks the per-stain gradients in ONE pass; M selects make autograd fill a dense
            # [B,M,N,128] zero tensor per stain and add them pairwise (5 fills + 4 adds of 335 MB each at config 3: 1.1 ms per step)
            slides, toks = slide.unbind(1), tok.unbind(1)
            for idx, modality in enumerate(self.modalities):
                s, t = slides[idx], toks[idx]
                if modality == "HE":
                    # reference: .unsqueeze(3).repeat(1,1,1,M-1); expand gives the same values without copies
                    s = s.unsqueeze(3).expand(-1, -1, -1, n_mod - 1)
                    t = t.unsqueeze(3).expand(-1, -1, -1, n_mod - 1)
                all_embeddings[modality] = s
                all_token_embeddings[modality] = t
            return all_embeddings, all_token_embeddings

        elif not train and not return_attention:  # Model.py:162-203
            bs, n_mod, n_tokens, d_in = all_wsi_feats.shape
            self._require_single_modality(n_mod)
            for stain_idx in range(n_mod):
                stain_name = self.modalities[custom_stain_idx] if custom_stain_idx else self.modalities[stain_idx]
                cur = all_wsi_feats[:, stain_idx]
                stain = None
                if self.stain_encoding:
                    key = custom_stain_idx if custom_stain_idx else stain_idx
                    stain = self._stain_groups(torch.full((bs,), key, dtype=torch.long), bs, n_tokens, device)
                pooled, _, _ = emb.forward_headmajor(cur, need_tokens=False, stain=stain)
                # the reference's .view(bs*n_mod, ...) / .view(bs, n_mod, d) only type-checks for n_mod == 1
                all_embeddings[stain_name] = self._project_slide(pooled).view(bs, n_mod, -1)
            return all_embeddings

        else:  # Model.py:206-216
            bs, n_mod, n_tokens, d_in = all_wsi_feats.shape
            self._require_single_modality(n_mod)
            pooled, _, scores = emb.forward_headmajor(all_wsi_feats[:, HE_POSITION], need_tokens=False)
            he = self._project_slide(pooled).view(bs, n_mod, -1)
            return he, scores.unsqueeze(2)
