"""Survival probe on the device: do slide embeddings stratify patients?  Ridge-penalised Cox proportional-hazards fits (Breslow ties)
over event-stratified cross-validation folds, Harrell's concordance index and a median-split log-rank test on every fold's held-out
cases -- every (endpoint, repeat, fold) problem of an evaluation in one batch of HIP launches.

    from madeleine_amd import survival_probe
    results = survival_probe(embeds, {"os": os_months, "pfs": pfs_months}, {"os": os_event, "pfs": pfs_event})
    results[("os", 0)]["c_index"]        # [folds]

event: 1 = event, 0 = censored, -1 = no follow-up (such a case is never trained on or tested)."""
import math
import warnings

import numpy as np
import torch

from . import _native
from . import functional as F

__all__ = ["survival_splits", "fit_cox", "survival_probe"]

GTOL = 1e-3      # relative: |gradient|_inf <= GTOL * |gradient at w = 0|_inf; how it was chosen: DESIGN 3.15


def survival_splits(event, folds=5, repeat=0, seed_base=0):
    """The training indices (a list of `folds` int64 vectors, each ascending) of an event-stratified K-fold: the event cases and the
    censored cases are shuffled separately by torch.randperm under torch.Generator().manual_seed(seed_base + 1000 * folds + repeat)
    -- events first -- and dealt to the folds in turn, the censored cases starting at the fold after the last event's; fold f trains on
    every case with follow-up outside its own share.  Cases with event -1 are never drawn.  ValueError with fewer cases with follow-up
    than folds, or when a fold's training part exceeds MDL_COX_MAX_TRAIN."""
    event = torch.as_tensor(np.asarray(event.cpu() if isinstance(event, torch.Tensor) else event)).long()
    folds = int(folds)
    if event.dim() != 1 or folds < 2:
        raise ValueError("survival_splits: event must be a vector and folds >= 2")
    g = torch.Generator().manual_seed(int(seed_base) + 1000 * folds + int(repeat))
    fold_of = torch.full_like(event, -1)
    dealt = 0
    for flag in (1, 0):
        idx = torch.nonzero(event == flag)[:, 0]
        idx = idx[torch.randperm(idx.numel(), generator=g)]
        fold_of[idx] = (torch.arange(idx.numel()) + dealt) % folds
        dealt += idx.numel()
    if dealt < folds:
        raise ValueError("survival_splits: %d cases with follow-up, fewer than %d folds" % (dealt, folds))
    out = [torch.nonzero((fold_of >= 0) & (fold_of != f))[:, 0] for f in range(folds)]
    limit = _native._DEFINES["MDL_COX_MAX_TRAIN"]
    if max(t.numel() for t in out) > limit:
        raise ValueError("survival_splits: a fold trains on %d cases, more than the %d a fit supports" % (
            max(t.numel() for t in out), limit))
    return out


def _problem_table(train_lists, device):
    """(train_idx [P, n_max] int32 padded with -1, n_train [P] int32) on `device`, from a list of 1-D index tensors; queued copies from
    pinned memory, so that the host does not wait for the device."""
    n = [int(t.numel()) for t in train_lists]
    table = torch.full((len(n), max(max(n), 1)), -1, dtype=torch.int32)
    for p, t in enumerate(train_lists):
        table[p, :n[p]] = t.to(torch.int32)
    return F.h2d(table, device), F.h2d(torch.tensor(n, dtype=torch.int32), device)


def fit_cox(X, time, event, train_idx, cost=1.0, gtol=GTOL, max_iter=100):
    """P ridge-penalised Cox fits on the device (scikit-survival's CoxPHSurvivalAnalysis(alpha=1 / cost, ties="breslow")).  X [S, d] fp32
    device tensor; time and event [S] or [P, S]; train_idx a list of P index vectors or a [P, n_max] table padded with -1.  Returns
    (W [P, d], thr [P], info): thr the median training decision value, info = {"iterations", "converged", "residual", "cg_iterations"},
    [P] device tensors.  gtol is relative to the gradient at w = 0.  Nothing is read back: the caller decides when to look."""
    if not isinstance(X, torch.Tensor) or not X.is_cuda:
        raise RuntimeError("madeleine_amd: X must be a tensor on a ROCm device; there is no CPU fallback")
    time = F.h2d(torch.as_tensor(time), X.device, torch.float32).contiguous()
    event = F.h2d(torch.as_tensor(event), X.device, torch.int32).contiguous()
    if isinstance(train_idx, torch.Tensor) and train_idx.dim() == 2:
        table = train_idx.to(device=X.device, dtype=torch.int32).contiguous()
        n_train = (table >= 0).sum(1, dtype=torch.int32)
    else:
        table, n_train = _problem_table([torch.as_tensor(t).reshape(-1) for t in train_idx], X.device)
    W, thr, info = F.cox_fit(X, time, event, table, n_train, cost, gtol, max_iter)
    return W, thr, {"iterations": info[:, 0], "converged": info[:, 1] > 0, "residual": info[:, 2], "cg_iterations": info[:, 3]}


def _host_vector(v, S, what, name):
    v = torch.as_tensor(np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v))
    if v.shape != (S,):
        raise ValueError("survival_probe: endpoint %r has %s %s for %d embeddings" % (name, tuple(v.shape), what, S))
    return v


def survival_probe(embeds, time, event, folds=5, repeats=1, cost=1.0, seed_base=0, gtol=GTOL, max_iter=100):
    """Cross-validated survival probing of embeds [S, d] (tensor or array): for every endpoint (time and event: one [S] vector each --
    endpoint "survival" -- or dicts endpoint -> [S] over the same keys), every repeat and every fold of survival_splits(event, folds,
    repeat, seed_base), fit on the fold's training cases and evaluate on its held-out cases with follow-up.  All problems share ONE fit,
    ONE scoring and ONE metrics launch sequence.  Returns {(endpoint, repeat): {"c_index": [folds], "logrank_chi2": [folds],
    "logrank_p": [folds], "converged": [folds] bool, "threshold": [folds], "counts": [folds, 6]}} as numpy arrays; counts columns:
    concordance numerator, comparable pairs, test cases, high-risk cases (decision value above the training median), events in the low
    group, events in the high group.  Two host reads: the finiteness check of embeds (ValueError) and the results.  time and event are
    host vectors (arrays, lists or CPU tensors: the folds are drawn on the host); a device tensor among them is copied to the host
    first, one more host read each.  Problems that did not converge are flagged in "converged" and announced by one RuntimeWarning."""
    if not torch.cuda.is_available():
        raise RuntimeError("madeleine_amd: survival_probe needs a ROCm device; there is no CPU fallback")
    X = torch.as_tensor(embeds)
    X = X.to(device=X.device if X.is_cuda else "cuda", dtype=torch.float32)
    if X.dim() != 2:
        raise ValueError("survival_probe: embeds must be [S, d]")
    if X.stride(-1) != 1:
        X = X.contiguous()
    if not bool(torch.isfinite(X).all()):
        raise ValueError("survival_probe: embeds holds non-finite values")
    if isinstance(time, dict) != isinstance(event, dict) or (isinstance(time, dict) and set(time) != set(event)):
        raise ValueError("survival_probe: time and event must both be vectors, or dicts over the same endpoints")
    times, events = (time, event) if isinstance(time, dict) else ({"survival": time}, {"survival": event})
    S = X.shape[0]
    probs, t_rows, e_rows = [], [], []              # (endpoint, repeat, fold, training indices)
    for name in times:
        t, e = _host_vector(times[name], S, "times", name).float(), _host_vector(events[name], S, "events", name).long()
        for repeat in range(repeats):
            for fold, idx in enumerate(survival_splits(e, folds, repeat, seed_base)):
                probs.append((name, repeat, fold, idx))
                t_rows.append(t)
                e_rows.append(e)
    P = len(probs)
    table, n_train = _problem_table([p[3] for p in probs], X.device)
    t_dev = F.h2d(torch.stack(t_rows), X.device)
    e_dev = F.h2d(torch.stack(e_rows), X.device, torch.int32)
    W, thr, info = F.cox_fit(X, t_dev, e_dev, table, n_train, cost, gtol, max_iter)
    z = F.probe_scores(X, W.unsqueeze(1), torch.zeros(P, 1, device=X.device), 2).squeeze(2)
    c_index, chi2, counts = F.survival_metrics(z, t_dev, e_dev, table, n_train, thr)
    host = torch.cat([c_index, chi2, info[:, 1].double(), thr.double(), counts.reshape(-1).double()]).cpu().numpy()      # the one read
    c_index, chi2, conv, thr, counts = host[:P], host[P:2 * P], host[2 * P:3 * P] > 0, host[3 * P:4 * P], host[4 * P:].reshape(P, 6)
    out = {}
    for p, (name, repeat, fold, _) in enumerate(probs):
        res = out.setdefault((name, repeat), {"c_index": np.zeros(folds), "logrank_chi2": np.zeros(folds), "logrank_p": np.zeros(folds),
                                              "converged": np.zeros(folds, dtype=bool), "threshold": np.zeros(folds),
                                              "counts": np.zeros((folds, 6), dtype=np.int64)})
        res["c_index"][fold], res["logrank_chi2"][fold], res["converged"][fold] = c_index[p], chi2[p], conv[p]
        res["logrank_p"][fold] = math.erfc(math.sqrt(chi2[p] / 2.0)) if chi2[p] == chi2[p] else float("nan")
        res["threshold"][fold], res["counts"][fold] = thr[p], np.rint(counts[p])
    if not conv.all():
        warnings.warn("survival_probe: %d of %d fits did not reach gtol = %g (relative) in %d Newton steps" % (
            int((~conv).sum()), P, gtol, max_iter), RuntimeWarning)
    return out
