"""Regression probe on the device: do slide embeddings predict continuous targets (Ki-67 index, ER / PR percentages and H-scores, TIL
fraction, bulk expression of a gene panel)?  Ridge regression with an unpenalised intercept over K folds, and Pearson r, Spearman rho,
R^2, MAE and RMSE on every fold's held-out cases -- every (repeat, fold) problem, every penalty and every target of an evaluation in
one batch of HIP launches per availability group (include/madeleine_amd_regress.h).

    from madeleine_amd import regression_probe
    results = regression_probe(embeds, {"ki67": ki67, "er_pct": er_pct}, alphas=(0.1, 1.0, 10.0))
    results[("ki67", 0)]["pearson"]        # [folds, A]

A NaN in a target vector is "no value": such a case is never trained on or tested for that target."""
import warnings

import numpy as np
import torch

from . import _native
from . import functional as F
from .survival import _problem_table

__all__ = ["regression_splits", "fit_ridge", "regression_probe"]

METRICS = F.REG_COLUMNS[1:]      # "pearson", "spearman", "r2", "mae", "rmse"


def regression_splits(available, folds=5, repeat=0, seed_base=0):
    """The training indices (a list of `folds` int64 vectors, each ascending) of a plain K-fold over the cases where `available` is true:
    they are shuffled by torch.randperm under torch.Generator().manual_seed(seed_base + 1000 * folds + repeat) and dealt to the folds in
    turn; fold f trains on every available case outside its own share.  ValueError with fewer available cases than folds, or when a
    fold's training part exceeds MDL_RIDGE_MAX_TRAIN."""
    available = torch.as_tensor(np.asarray(available.cpu() if isinstance(available, torch.Tensor) else available)).bool()
    folds = int(folds)
    if available.dim() != 1 or folds < 2:
        raise ValueError("regression_splits: available must be a vector and folds >= 2")
    g = torch.Generator().manual_seed(int(seed_base) + 1000 * folds + int(repeat))
    idx = torch.nonzero(available)[:, 0]
    if idx.numel() < folds:
        raise ValueError("regression_splits: %d available cases, fewer than %d folds" % (idx.numel(), folds))
    idx = idx[torch.randperm(idx.numel(), generator=g)]
    fold_of = torch.full((available.numel(),), -1, dtype=torch.int64)
    fold_of[idx] = torch.arange(idx.numel()) % folds
    out = [torch.nonzero((fold_of >= 0) & (fold_of != f))[:, 0] for f in range(folds)]
    limit = _native.REGRESS_DEFINES["MDL_RIDGE_MAX_TRAIN"]
    if max(t.numel() for t in out) > limit:
        raise ValueError("regression_splits: a fold trains on %d cases, more than the %d a fit supports" % (
            max(t.numel() for t in out), limit))
    return out


def _device_matrix(X, what):
    if not isinstance(X, torch.Tensor) or not X.is_cuda:
        raise RuntimeError("madeleine_amd: %s must be a tensor on a ROCm device; there is no CPU fallback" % what)
    return X


def fit_ridge(X, Y, train_idx, alphas):
    """P x A x T ridge fits on the device (scikit-learn's Ridge(alpha)): X [S, d] fp32 device tensor, Y [S] or [S, T] targets (NaN: no
    value), train_idx a list of P index vectors or a [P, n_max] table padded with -1, alphas a sequence of A penalties > 0.  Returns
    (W [P, A, T, d], b [P, A, T], info): info = {"ok": [P, A] bool, "pivot_ratio": [P, A]} device tensors -- whether the factorisation
    succeeded and its smallest pivot over its largest diagonal entry.  A fit that failed, that has a NaN among its training targets or
    whose problem is out of range holds NaN.  Nothing is read back: the caller decides when to look."""
    _device_matrix(X, "X")
    Y = F.h2d(torch.as_tensor(Y), X.device, torch.float32)
    Y = (Y[:, None] if Y.dim() == 1 else Y).contiguous()
    if isinstance(train_idx, torch.Tensor) and train_idx.dim() == 2:
        table = train_idx.to(device=X.device, dtype=torch.int32).contiguous()
        n_train = (table >= 0).sum(1, dtype=torch.int32)
    else:
        table, n_train = _problem_table([torch.as_tensor(t).reshape(-1) for t in train_idx], X.device)
    W, b, info = F.ridge_fit(X, Y, table, n_train, alphas)
    return W, b, {"ok": info[..., 0] > 0, "pivot_ratio": info[..., 1]}


def _targets(targets, S):
    """(names, [S, T] float32 host tensor) of a dict name -> [S] vector or a (names, [S, T]) pair."""
    if isinstance(targets, dict):
        names = list(targets)
        cols = []
        for name in names:
            v = targets[name]
            v = torch.as_tensor(np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v)).float()
            if v.shape != (S,):
                raise ValueError("regression_probe: target %r has %s values for %d embeddings" % (name, tuple(v.shape), S))
            cols.append(v)
        if not cols:
            raise ValueError("regression_probe: no targets")
        return names, torch.stack(cols, 1)
    names, Y = targets
    names = list(names)
    Y = torch.as_tensor(np.asarray(Y.cpu() if isinstance(Y, torch.Tensor) else Y)).float()
    if Y.dim() != 2 or Y.shape != (S, len(names)) or not names:
        raise ValueError("regression_probe: targets must be (names, [S, T]) with S = %d and T = len(names)" % S)
    return names, Y


def regression_probe(embeds, targets, folds=5, repeats=1, alphas=(1.0,), seed_base=0):
    """Cross-validated regression probing of embeds [S, d] (tensor or array).  targets: a dict name -> [S] vector, or a
    (names, [S, T]) pair; a NaN is "no value".  The targets are grouped by their availability mask; for every group, every repeat and
    every fold of regression_splits(mask, folds, repeat, seed_base), ridge fits on the fold's training cases for every penalty in
    `alphas` and every target of the group, evaluated on the fold's held-out cases.  Each group makes ONE fit, ONE scoring and ONE
    metrics launch sequence over all its (repeat, fold) problems.  Returns {(name, repeat): {"pearson", "spearman", "r2", "mae", "rmse":
    [folds, A], "n_test": [folds], "ok": [folds, A] bool, "alphas": [A]}} as numpy arrays.  Two host reads: the finiteness check of
    embeds (ValueError) and the results.  The targets are host data (arrays, lists or CPU tensors: the folds are drawn on the host); a
    device tensor among them is copied to the host first, one more host read each.  Factorisations that failed are flagged in "ok" and
    announced by one RuntimeWarning."""
    if not torch.cuda.is_available():
        raise RuntimeError("madeleine_amd: regression_probe needs a ROCm device; there is no CPU fallback")
    X = torch.as_tensor(embeds)
    X = X.to(device=X.device if X.is_cuda else "cuda", dtype=torch.float32)
    if X.dim() != 2:
        raise ValueError("regression_probe: embeds must be [S, d]")
    if X.stride(-1) != 1:
        X = X.contiguous()
    if not bool(torch.isfinite(X).all()):
        raise ValueError("regression_probe: embeds holds non-finite values")
    S = X.shape[0]
    names, Y = _targets(targets, S)
    alphas = [float(a) for a in alphas]
    A = len(alphas)
    Y = torch.where(torch.isfinite(Y), Y, torch.full_like(Y, float("nan")))      # +-inf is no value either
    groups = {}                                                                   # availability mask -> target columns
    for t in range(len(names)):
        groups.setdefault(torch.isfinite(Y[:, t]).numpy().tobytes(), []).append(t)
    pieces, layout = [], []                          # device results; (columns, problems) per group
    for cols in groups.values():
        mask = torch.isfinite(Y[:, cols[0]])
        probs = [(repeat, fold, idx) for repeat in range(repeats)
                 for fold, idx in enumerate(regression_splits(mask, folds, repeat, seed_base))]
        table, n_train = _problem_table([p[2] for p in probs], X.device)
        Yg = F.h2d(Y[:, cols].contiguous(), X.device)
        W, b, info = F.ridge_fit(X, Yg, table, n_train, alphas)
        Z = F.ridge_scores(X, W, b)
        metrics = F.regress_metrics(Z, Yg, table, n_train)                       # [P, A, Tg, 6]
        pieces += [metrics.reshape(-1), info[..., 0].double().reshape(-1)]
        layout.append((cols, probs))
    host = torch.cat(pieces).cpu().numpy()           # the one read
    out, at, failed, total = {}, 0, 0, 0
    for cols, probs in layout:
        P, Tg = len(probs), len(cols)
        metrics = host[at:at + P * A * Tg * 6].reshape(P, A, Tg, 6)
        at += metrics.size
        ok = host[at:at + P * A].reshape(P, A) > 0
        at += ok.size
        failed, total = failed + int((~ok).sum()), total + ok.size
        for k, t in enumerate(cols):
            for p, (repeat, fold, _) in enumerate(probs):
                res = out.setdefault((names[t], repeat), dict(
                    {m: np.zeros((folds, A)) for m in METRICS}, n_test=np.zeros(folds, dtype=np.int64),
                    ok=np.zeros((folds, A), dtype=bool), alphas=np.asarray(alphas)))
                for c, m in enumerate(F.REG_COLUMNS):
                    if c:
                        res[m][fold] = metrics[p, :, k, c]
                res["n_test"][fold] = int(metrics[p, 0, k, 0])
                res["ok"][fold] = ok[p]
    if failed:
        warnings.warn("regression_probe: %d of %d factorisations failed (a pivot that is not positive); their fits hold NaN" % (
            failed, total), RuntimeWarning)
    return out
