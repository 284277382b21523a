"""Cross-stain retrieval: the label-free measure of what the contrastive loss optimises.  Given the H&E embedding of a held-out case,
at which rank does the embedding of its own HER2 / PGR / KI67 / ER slide come back among all the others, and the reverse -- a checkpoint
criterion beside the smooth rank, which is blind to whether the stains are aligned at all.  Plus the "most similar slides" query over
one cohort's embeddings.

The similarities, the exact integer rank counts and the top-k lists come from functional.retrieval (mdl_retrieval, csrc/retrieval.hip):
streamed exact-fp32 MFMA tiles, no [n, m] matrix, no library GEMM.  The metrics below are a few reductions over two int32 vectors, done
on the host after ONE read.

Ranks are pessimistic: the partner's rank is 1 + greater + equal, as if every tie were lost.  A collapsed encoder (all embeddings equal)
then scores recall@k = 0 for k < n instead of 1, and an encoder that emits NaN scores worst (a NaN similarity sorts below -inf, a NaN
partner similarity is ranked last).  The optimistic figures are reported beside them; on healthy embeddings the two agree.
"""
import numpy as np
import torch

from . import functional as MF


def retrieval_metrics(greater, equal, ks=(1, 5, 10)) -> dict:
    """{"n", "recall@k", "recall_optimistic@k" for k in ks, "median_rank", "mrr"} as Python numbers from the counts of a paired
    functional.retrieval call (int tensors [n], on any device: one host read).  recall@k is the share of queries with greater + equal
    < k (every tie counted against the partner), recall_optimistic@k with greater < k; median_rank and mrr are over the pessimistic
    rank 1 + greater + equal."""
    if greater.shape != equal.shape or greater.dim() != 1 or greater.numel() < 1:
        raise ValueError("retrieval_metrics needs two count vectors of one length >= 1 (got %s, %s)"
                         % (tuple(greater.shape), tuple(equal.shape)))
    both = torch.stack([greater, equal]).cpu().numpy().astype(np.int64)      # the one host read
    g, rank = both[0], 1 + both[0] + both[1]
    out = {"n": int(g.shape[0])}
    for k in ks:
        out["recall@%d" % k] = float(np.mean(rank <= k))
        out["recall_optimistic@%d" % k] = float(np.mean(g < k))
    out["median_rank"] = float(np.median(rank))
    out["mrr"] = float(np.mean(1.0 / rank))
    return out


def slide_neighbours(embeds, k, metric='cosine'):
    """(idx [n, k] int32, sim [n, k] fp32) on the device: the k most similar OTHER rows of embeds [n, d] for every row, best first (ties
    by the lower index, NaNs last); -1 / -inf past n - 1 neighbours."""
    if int(k) < 1:
        raise ValueError("slide_neighbours needs k >= 1 (got %r)" % (k,))
    res = MF.retrieval(embeds, None, k=k, metric=metric, paired=False, exclude_diag=True)
    return res.topk_idx, res.topk_val


def _stain_indices(store, stains):
    mods = list(store.modalities)
    if stains is None:
        return list(range(1, len(mods)))
    out = []
    for s in stains:
        i = mods.index(s) if isinstance(s, str) and s in mods else s
        if isinstance(i, bool) or not isinstance(i, int) or not 1 <= i < len(mods):
            raise ValueError("cross_stain_retrieval: %r is not a non-H&E stain of %s" % (s, mods))
        out.append(i)
    return out


def cross_stain_retrieval(store, model, case_indices=None, stains=None, ks=(1, 5, 10), precision=None, bags_per_launch=None,
                          max_tokens=None, metric='cosine') -> dict:
    """Retrieval between the H&E slide (modality 0 of store.modalities) and every other stain of a DeviceSlideStore's cases (None: all
    of them; typically a held-out split), in both directions:
        {stain: {"n", "cases", "he_to_stain": retrieval_metrics(...), "stain_to_he": retrieval_metrics(...)}, ..., "mean": {...}}
    For a stain, the cases (of those asked for, in the order asked) that have both bags are embedded on both sides
    (store.embed_modality: eval mode under no_grad, the training flag restored, embed()'s grouping and autocast rule; a model with stain
    encoding gets the true stain index on both sides, H&E = 0), and query i's partner is gallery row i.  A stain with fewer than two such
    cases is reported with "n" and "cases" alone, as calculate_losses skips it.  "mean" is the unweighted mean of every metric over the
    stains that have n >= 2, per direction (empty when there is none).  stains: names or modality indices (None: every non-H&E one).
    One host read per direction and stain."""
    table = store.bag_table
    asked = torch.arange(len(store), dtype=torch.int64) if case_indices is None else store._cases(case_indices)
    with_he = asked[table[asked, 0] >= 0]
    he = None
    out, per_dir = {}, {"he_to_stain": [], "stain_to_he": []}
    for mi in _stain_indices(store, stains):
        name = store.modalities[mi]
        sel = table[with_he, mi] >= 0
        cases = with_he[sel]
        entry = {"n": int(cases.numel()), "cases": cases.tolist()}
        out[name] = entry
        if cases.numel() < 2:
            continue
        if he is None:      # every asked case's H&E slide once, whatever the stain
            he = store.embed_modality(model, 0, with_he, bags_per_launch=bags_per_launch, max_tokens=max_tokens,
                                      precision=precision)["embeds"]
        rows = MF.h2d(sel.nonzero().reshape(-1), store.device)
        E_he = he.index_select(0, rows)
        E_st = store.embed_modality(model, mi, cases, bags_per_launch=bags_per_launch, max_tokens=max_tokens,
                                    precision=precision)["embeds"]
        for direction, (Q, K) in (("he_to_stain", (E_he, E_st)), ("stain_to_he", (E_st, E_he))):
            r = MF.retrieval(Q, K, metric=metric, paired=True)
            entry[direction] = retrieval_metrics(r.greater, r.equal, ks)
            per_dir[direction].append(entry[direction])
    out["mean"] = {d: {k: float(np.mean([m[k] for m in ms])) for k in ms[0] if k != "n"} for d, ms in per_dir.items() if ms}
    return out
