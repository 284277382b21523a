"""Few-shot linear probe on the device: the reference's bin/run_linear_probing.py (k training cases per class, 10 folds, L2-regularised
logistic regression, AUC and balanced accuracy) with every (task, k, fold) problem of an evaluation in one batch of HIP launches.

    from madeleine_amd import linear_probe
    results = linear_probe(embeds, {"er": er, "pr": pr, "her2": her2})       # {(task, k): {"auc": [folds], "bacc": [folds], ...}}

`python -m madeleine_amd.probe --slide_embedding_pkl P --label_path CSV` is the reference's command line.

The probe trained on all labels, cross-validated, is linear_probe_cv (stratified K folds by cv_splits, `--cv_folds K` on the command
line): the same objective solved in the primal unknowns, for up to MDL_LOGIT_MAX_TRAIN training cases per fold."""
import warnings

import numpy as np
import torch

from . import _native
from . import functional as F

__all__ = ["probe_splits", "cv_splits", "fit_logistic", "linear_probe", "linear_probe_cv", "balanced_accuracy", "quadratic_kappa"]


def probe_splits(labels, k, fold, seed_base=0):
    """Training indices (int64 [C * k], class 0's first) of the few-shot split (k, fold): k cases of every class 0 .. C-1, C =
    max(labels) + 1, drawn by torch.randperm under torch.Generator().manual_seed(seed_base + 1000 * k + fold), classes in increasing
    order, cases in case order.  Label -1 (unlabeled) is never drawn.  ValueError when a class has no case or fewer than k."""
    labels = torch.as_tensor(np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels)).long()
    if labels.dim() != 1 or int(k) < 1 or not bool((labels >= 0).any()):
        raise ValueError("probe_splits: labels must be a vector with a labeled case, and k >= 1")
    g = torch.Generator().manual_seed(int(seed_base) + 1000 * int(k) + int(fold))
    out = []
    for c in range(int(labels.max()) + 1):
        idx = torch.nonzero(labels == c)[:, 0]
        if idx.numel() == 0:
            raise ValueError("probe_splits: class %d has no case" % c)
        if idx.numel() < k:
            raise ValueError("probe_splits: class %d has %d cases, fewer than k = %d" % (c, idx.numel(), k))
        out.append(idx[torch.randperm(idx.numel(), generator=g)[:k]])
    return torch.cat(out)


def cv_splits(labels, folds=5, repeat=0, seed_base=0):
    """The training indices (a list of `folds` int64 vectors, each ascending) of a class-stratified K-fold: for every class 0 .. C-1 in
    increasing order, C = max(labels) + 1, its cases are shuffled by torch.randperm under ONE torch.Generator().manual_seed(seed_base +
    1000 * folds + repeat) and dealt to the folds in turn, each class starting at the fold after the previous class's last; fold f trains
    on every labeled case outside its own share.  Label -1 (unlabeled) is never drawn.  ValueError without a labeled case, when a class
    has fewer cases than folds, or when a fold's training part exceeds MDL_LOGIT_MAX_TRAIN."""
    labels = torch.as_tensor(np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels)).long()
    folds = int(folds)
    if labels.dim() != 1 or folds < 2 or not bool((labels >= 0).any()):
        raise ValueError("cv_splits: labels must be a vector with a labeled case, and folds >= 2")
    g = torch.Generator().manual_seed(int(seed_base) + 1000 * folds + int(repeat))
    fold_of = torch.full_like(labels, -1)
    dealt = 0
    for c in range(int(labels.max()) + 1):
        idx = torch.nonzero(labels == c)[:, 0]
        if idx.numel() < folds:
            raise ValueError("cv_splits: class %d has %d cases, fewer than %d folds" % (c, idx.numel(), folds))
        idx = idx[torch.randperm(idx.numel(), generator=g)]
        fold_of[idx] = (torch.arange(idx.numel()) + dealt) % folds
        dealt += idx.numel()
    out = [torch.nonzero((fold_of >= 0) & (fold_of != f))[:, 0] for f in range(folds)]
    limit = _native._DEFINES["MDL_LOGIT_MAX_TRAIN"]
    if max(t.numel() for t in out) > limit:
        raise ValueError("cv_splits: a fold trains on %d cases, more than the %d a fit supports" % (max(t.numel() for t in out), limit))
    return out


def balanced_accuracy(confusion):
    """sklearn's balanced_accuracy_score from a confusion matrix (row = truth), fp64: the mean recall of the classes that have a case."""
    cm = np.asarray(confusion, dtype=np.float64)
    support = cm.sum(1)
    have = support > 0
    return float(np.mean(np.diag(cm)[have] / support[have])) if have.any() else float("nan")


def quadratic_kappa(confusion):
    """cohen_kappa_score(weights="quadratic") from a confusion matrix over the grades 0 .. C-1, fp64.  NaN when chance agreement is
    complete (all cases in one cell's row and column)."""
    cm = np.asarray(confusion, dtype=np.float64)
    C = cm.shape[0]
    w = (np.arange(C)[:, None] - np.arange(C)[None, :]) ** 2.0
    expected = np.outer(cm.sum(1), cm.sum(0)) / max(cm.sum(), 1.0)
    den = float((w * expected).sum())
    return 1.0 - float((w * cm).sum()) / den if den > 0 else float("nan")


def _problem_table(train_lists, device):
    """(train_idx [P, n_max] int32 padded with -1, n_train [P] int32) on `device`, from a list of 1-D index tensors -- one copy each."""
    n = [int(t.numel()) for t in train_lists]
    table = torch.full((len(n), max(n)), -1, dtype=torch.int32)
    for p, t in enumerate(train_lists):
        table[p, :n[p]] = t.to(torch.int32)
    return table.to(device), torch.tensor(n, dtype=torch.int32).to(device)


def fit_logistic(X, y, train_idx, n_classes, cost=1.0, gtol=1e-4, max_iter=100):
    """P regularised logistic fits on the device (sklearn's LogisticRegression(C=cost), binary form for two classes, multinomial above).
    X [S, d] fp32 device tensor; y [S] or [P, S] integer labels (-1: unlabeled); train_idx a list of P index vectors or a [P, n_max]
    table padded with -1.  Returns (W [P, cols, d], b [P, cols], info) with info = {"iterations", "converged", "residual",
    "cg_iterations"}, [P] device tensors.  Nothing is read back: the caller decides when to look at `converged`.  A table of at most
    MDL_PROBE_MAX_TRAIN columns goes to the few-shot solver (probe_fit, in the span of the training rows), a wider one to the primal
    solver (logit_fit, up to MDL_LOGIT_MAX_TRAIN columns)."""
    if not isinstance(X, torch.Tensor) or not X.is_cuda:
        raise RuntimeError("madeleine_amd: X must be a tensor on a ROCm device; there is no CPU fallback")
    y = torch.as_tensor(y).to(device=X.device, dtype=torch.int32).contiguous()
    if isinstance(train_idx, torch.Tensor) and train_idx.dim() == 2:
        table = train_idx.to(device=X.device, dtype=torch.int32).contiguous()
        n_train = (table >= 0).sum(1, dtype=torch.int32)
    else:
        table, n_train = _problem_table([torch.as_tensor(t).reshape(-1) for t in train_idx], X.device)
    fit = F.probe_fit if table.shape[1] <= _native._DEFINES["MDL_PROBE_MAX_TRAIN"] else F.logit_fit
    W, b, info = fit(X, y, table, n_train, n_classes, cost, gtol, max_iter)
    return W, b, {"iterations": info[:, 0], "converged": info[:, 1] > 0, "residual": info[:, 2], "cg_iterations": info[:, 3]}


def linear_probe(embeds, labels, ks=(1, 10, 25), folds=10, cost=1.0, seed_base=0, kappa=False, gtol=1e-4, max_iter=100):
    """The reference's linear-probing protocol over embeds [S, d] (tensor or array): for every task (labels: one [S] vector -- task
    "label" -- or a dict task -> [S]; -1 = unlabeled), every k of ks and every fold, fit on probe_splits(labels, k, fold, seed_base) and
    score on all other labeled cases.  All problems of equal class count share ONE fit, ONE scoring and ONE metrics launch sequence.
    Returns {(task, k): {"auc": [folds], "bacc": [folds], "converged": [folds] bool, "confusion": [folds, C, C] (+ "q_kappa": [folds]
    with kappa=True)}} as numpy arrays.  Two host reads: the finiteness check of embeds (ValueError) and the results.  Problems that
    did not converge are flagged in "converged" and announced by one RuntimeWarning."""
    if not torch.cuda.is_available():
        raise RuntimeError("madeleine_amd: linear_probe needs a ROCm device; there is no CPU fallback")
    X = torch.as_tensor(embeds)
    X = X.to(device=X.device if X.is_cuda else "cuda", dtype=torch.float32)
    if X.dim() != 2:
        raise ValueError("linear_probe: embeds must be [S, d]")
    if X.stride(-1) != 1:
        X = X.contiguous()
    if not bool(torch.isfinite(X).all()):
        raise ValueError("linear_probe: embeds holds non-finite values")
    tasks = labels if isinstance(labels, dict) else {"label": labels}
    groups = {}                                     # C -> [(task, k, fold, y, train indices)]
    for task, y in tasks.items():
        y = torch.as_tensor(np.asarray(y.cpu() if isinstance(y, torch.Tensor) else y)).long()
        if y.shape != (X.shape[0],):
            raise ValueError("linear_probe: task %r has %s labels for %d embeddings" % (task, tuple(y.shape), X.shape[0]))
        for k in ks:
            for fold in range(folds):
                groups.setdefault(int(y.max()) + 1, []).append((task, k, fold, y, probe_splits(y, k, fold, seed_base)))
    parts = []
    for C, probs in groups.items():
        table, n_train = _problem_table([p[4] for p in probs], X.device)
        y_dev = torch.stack([p[3] for p in probs]).to(torch.int32).to(X.device)
        W, b, info = F.probe_fit(X, y_dev, table, n_train, C, cost, gtol, max_iter)
        confusion, auc = F.probe_metrics(F.probe_scores(X, W, b, C), y_dev, table, n_train, C)
        parts += [auc.double(), info[:, 1].double(), confusion.reshape(-1).double()]
    host = torch.cat(parts).cpu().numpy()           # the one read of the results
    out, at, failed = {}, 0, 0
    for C, probs in groups.items():
        P = len(probs)
        auc, conv, cm = host[at:at + P], host[at + P:at + 2 * P] > 0, host[at + 2 * P:at + 2 * P + P * C * C].reshape(P, C, C)
        at += 2 * P + P * C * C
        failed += int((~conv).sum())
        for p, (task, k, fold, _, _) in enumerate(probs):
            res = out.setdefault((task, k), {"auc": np.zeros(folds), "bacc": np.zeros(folds), "converged": np.zeros(folds, dtype=bool),
                                             "confusion": np.zeros((folds, C, C), dtype=np.int64)})
            res["auc"][fold], res["converged"][fold], res["confusion"][fold] = auc[p], conv[p], np.rint(cm[p])
            res["bacc"][fold] = balanced_accuracy(cm[p])
            if kappa:
                res.setdefault("q_kappa", np.zeros(folds))[fold] = quadratic_kappa(cm[p])
    if failed:
        warnings.warn("linear_probe: %d of %d fits did not reach gtol = %g in %d Newton steps" % (failed, sum(map(len, groups.values())),
                                                                                                   gtol, max_iter), RuntimeWarning)
    return out


def linear_probe_cv(embeds, labels, folds=5, repeats=1, cost=1.0, seed_base=0, kappa=False, gtol=1e-4, max_iter=100):
    """The linear probe trained on all labels, cross-validated, over embeds [S, d] (tensor or array): for every task (labels: one [S]
    vector -- task "label" -- or a dict task -> [S]; -1 = unlabeled), every repeat and every fold of cv_splits(labels, folds, repeat,
    seed_base), fit on the fold's training cases and score on its held-out labeled cases.  All problems of equal class count share ONE
    fit, ONE scoring and ONE metrics launch sequence.  Returns {(task, repeat): {"auc": [folds], "bacc": [folds], "converged": [folds]
    bool, "confusion": [folds, C, C] (+ "q_kappa": [folds] with kappa=True)}} as numpy arrays.  Two host reads: the finiteness check of
    embeds (ValueError) and the results.  Problems that did not converge are flagged in "converged" and announced by one
    RuntimeWarning."""
    if not torch.cuda.is_available():
        raise RuntimeError("madeleine_amd: linear_probe_cv needs a ROCm device; there is no CPU fallback")
    X = torch.as_tensor(embeds)
    X = X.to(device=X.device if X.is_cuda else "cuda", dtype=torch.float32)
    if X.dim() != 2:
        raise ValueError("linear_probe_cv: embeds must be [S, d]")
    if X.stride(-1) != 1:
        X = X.contiguous()
    if not bool(torch.isfinite(X).all()):
        raise ValueError("linear_probe_cv: embeds holds non-finite values")
    tasks = labels if isinstance(labels, dict) else {"label": labels}
    groups = {}                                     # C -> [(task, repeat, fold, y, train indices)]
    for task, y in tasks.items():
        y = torch.as_tensor(np.asarray(y.cpu() if isinstance(y, torch.Tensor) else y)).long()
        if y.shape != (X.shape[0],):
            raise ValueError("linear_probe_cv: task %r has %s labels for %d embeddings" % (task, tuple(y.shape), X.shape[0]))
        for repeat in range(repeats):
            for fold, idx in enumerate(cv_splits(y, folds, repeat, seed_base)):
                groups.setdefault(int(y.max()) + 1, []).append((task, repeat, fold, y, idx))
    parts = []
    for C, probs in groups.items():
        table, n_train = _problem_table([p[4] for p in probs], X.device)
        y_dev = torch.stack([p[3] for p in probs]).to(torch.int32).to(X.device)
        W, b, info = F.logit_fit(X, y_dev, table, n_train, C, cost, gtol, max_iter)
        confusion, auc = F.logit_metrics(F.probe_scores(X, W, b, C), y_dev, table, n_train, C)
        parts += [auc.double(), info[:, 1].double(), confusion.reshape(-1).double()]
    host = torch.cat(parts).cpu().numpy()           # the one read of the results
    out, at, failed = {}, 0, 0
    for C, probs in groups.items():
        P = len(probs)
        auc, conv, cm = host[at:at + P], host[at + P:at + 2 * P] > 0, host[at + 2 * P:at + 2 * P + P * C * C].reshape(P, C, C)
        at += 2 * P + P * C * C
        failed += int((~conv).sum())
        for p, (task, repeat, fold, _, _) in enumerate(probs):
            res = out.setdefault((task, repeat), {"auc": np.zeros(folds), "bacc": np.zeros(folds), "converged": np.zeros(folds, dtype=bool),
                                                  "confusion": np.zeros((folds, C, C), dtype=np.int64)})
            res["auc"][fold], res["converged"][fold], res["confusion"][fold] = auc[p], conv[p], np.rint(cm[p])
            res["bacc"][fold] = balanced_accuracy(cm[p])
            if kappa:
                res.setdefault("q_kappa", np.zeros(folds))[fold] = quadratic_kappa(cm[p])
    if failed:
        warnings.warn("linear_probe_cv: %d of %d fits did not reach gtol = %g in %d Newton steps" % (
            failed, sum(map(len, groups.values())), gtol, max_iter), RuntimeWarning)
    return out


def _parser():
    import argparse
    ap = argparse.ArgumentParser(description="few-shot linear probing of slide embeddings (the reference's bin/run_linear_probing.py)")
    ap.add_argument("--slide_embedding_pkl", required=True)
    ap.add_argument("--label_path", required=True)
    ap.add_argument("--tasks", nargs="+", default=["er", "pr", "her2"])
    ap.add_argument("--cv_folds", type=int, default=0, help="train on all labels, cross-validated in this many stratified folds, "
                                                            "instead of the few-shot protocol")
    ap.add_argument("--cv_repeats", type=int, default=1)
    ap.add_argument("--bootstrap", type=int, default=0, metavar="R",
                    help="also resample the cohort R times: one more line per task with the percentile interval of the metric")
    ap.add_argument("--versus", default=None, metavar="OTHER.pkl",
                    help="with --bootstrap: a second embedding pickle over the same slides; the lines add the paired difference and its p")
    ap.add_argument("--level", type=float, default=0.95, help="with --bootstrap: the level of the intervals")
    ap.add_argument("--seed", type=int, default=0, help="with --bootstrap: the seed of the resamples")
    ap.add_argument("--regress", nargs="+", default=None, metavar="COL",
                    help="instead of the class tasks: read these columns as floats (empty or non-numeric: no value) and print the "
                         "cross-validated ridge regression metrics (--cv_folds, default 5; --cv_repeats)")
    ap.add_argument("--alphas", nargs="+", type=float, default=None, help="with --regress: the ridge penalties (default 1.0)")
    return ap


def _parse(argv=None):
    ap = _parser()
    args = ap.parse_args(argv)
    if args.bootstrap < 0 or not 0.0 < args.level < 1.0:
        ap.error("--bootstrap needs R >= 0 and --level a value inside (0, 1)")
    if not args.bootstrap and (args.versus is not None or args.level != 0.95 or args.seed != 0):
        ap.error("--versus, --level and --seed belong to --bootstrap R")
    if args.alphas is not None and (args.regress is None or any(not 0.0 < a < float("inf") for a in args.alphas)):
        ap.error("--alphas belongs to --regress and takes finite penalties > 0")
    if args.regress is not None and args.bootstrap:
        ap.error("--bootstrap does not cover --regress")
    return args


def _float_or_nan(text):
    try:
        return float(text)
    except (TypeError, ValueError):
        return float("nan")


def _regress_lines(results, names, repeats, alphas):
    """One line per (column, penalty): mean +/- std of every metric over every fold of every repeat."""
    lines = []
    for name in names:
        for a, alpha in enumerate(alphas):
            parts = []
            for m in ("pearson", "spearman", "r2", "mae", "rmse"):
                v = np.concatenate([results[(name, r)][m][:, a] for r in range(repeats)])
                parts.append("{}={} +/- {}".format(m, round(float(np.nanmean(v)), 3), round(float(np.nanstd(v)), 3)))
            n_test = int(sum(results[(name, r)]["n_test"].sum() for r in range(repeats)) // repeats)
            lines.append("regress={}, alpha={:g}, cases={}, {}".format(name, alpha, n_test, ", ".join(parts)))
    return lines


def _bootstrap_lines(results, unit_name, level):
    """One line per (task, k or cv repeat) of a linear_probe_ci result: the interval of the task's metric and, with a second arm, the
    paired difference and its p-value."""
    lines = []
    for (task, unit), res in results.items():
        metric = "q_kappa" if task == "isup_grade" else "auc"
        arms = list(res["arms"])
        a = res["arms"][arms[0]][metric]
        line = "{}={}, task={}, bootstrap {} {:g}% interval=[{}, {}] (point {}, {} valid replicates)".format(
            unit_name, unit, task, "quadratic kappa" if metric == "q_kappa" else "auc", 100 * level, round(a["lo"], 3), round(a["hi"], 3),
            round(a["point"], 3), a["n_valid"])
        if len(arms) > 1:
            d = res["pairs"][(arms[0], arms[1])][metric]
            line += ", difference to {}={} [{}, {}], p={}".format(arms[1], round(d["diff"], 3), round(d["lo"], 3), round(d["hi"], 3),
                                                                   round(d["p"], 4))
        lines.append(line)
    return lines


def _main(argv=None):
    import csv
    import os
    import pickle
    args = _parse(argv)
    with open(args.slide_embedding_pkl, "rb") as f:
        obj = pickle.load(f)
    with open(args.label_path, newline="") as f:
        rows = {str(r["slide_id"]): r for r in csv.DictReader(f)}
    keep = [i for i, s in enumerate(obj["slide_ids"]) if str(s) in rows]      # the reference's intersection of labels and embeddings
    embeds = np.asarray(obj["embeds"], dtype=np.float32)[keep]
    if args.regress is not None:                    # continuous targets: the regression probe, and nothing of the class tasks
        from .regress import regression_probe
        targets = {c: np.array([_float_or_nan(rows[str(obj["slide_ids"][i])].get(c)) for i in keep], dtype=np.float32) for c in args.regress}
        alphas = tuple(args.alphas or (1.0,))
        results = regression_probe(embeds, targets, folds=args.cv_folds or 5, repeats=args.cv_repeats, alphas=alphas)
        print("\n".join(_regress_lines(results, args.regress, args.cv_repeats, alphas)))
        return
    labels = {t: np.array([int(float(rows[str(obj["slide_ids"][i])][t])) for i in keep]) for t in args.tasks}
    if args.bootstrap:                              # printed after the usual lines; the pickles below hold what they always held
        from .resample import linear_probe_ci
        arms = {"embeds": embeds}
        if args.versus is not None:
            with open(args.versus, "rb") as f:
                other = pickle.load(f)
            where = {str(s): i for i, s in enumerate(other["slide_ids"])}
            missing = [str(obj["slide_ids"][i]) for i in keep if str(obj["slide_ids"][i]) not in where]
            if missing:
                raise SystemExit("--versus: %d slides of %s are absent from %s (first: %s)" % (
                    len(missing), args.slide_embedding_pkl, args.versus, missing[0]))
            arms[os.path.splitext(os.path.basename(args.versus))[0]] = np.asarray(other["embeds"], dtype=np.float32)[
                [where[str(obj["slide_ids"][i])] for i in keep]]
        ci = dict(replicates=args.bootstrap, level=args.level, seed=args.seed, kappa="isup_grade" in args.tasks)
    if args.cv_folds:
        results = linear_probe_cv(embeds, labels, folds=args.cv_folds, repeats=args.cv_repeats, kappa="isup_grade" in args.tasks)
        for task in args.tasks:                     # mean +/- std over every fold of every repeat
            metric = "q_kappa" if task == "isup_grade" else "auc"
            v = np.concatenate([results[(task, r)][metric] for r in range(args.cv_repeats)])
            print("cv_folds={}, task={}, {}={} +/- {}".format(args.cv_folds, task, "quadratic kappa" if metric == "q_kappa" else "auc",
                                                              round(float(v.mean()), 3), round(float(v.std()), 3)))
        if args.bootstrap:
            print("\n".join(_bootstrap_lines(linear_probe_ci(arms, labels, protocol="cv", folds=args.cv_folds, repeats=args.cv_repeats, **ci),
                                             "cv_repeat", args.level)))
        return
    results = linear_probe(embeds, labels, kappa="isup_grade" in args.tasks)
    name = os.path.splitext(os.path.basename(args.slide_embedding_pkl))[0]
    save = os.path.join(os.path.dirname(args.slide_embedding_pkl), "res_linear_probing", name)
    os.makedirs(save, exist_ok=True)
    for (task, k), res in results.items():
        if task == "isup_grade":
            print("k={}, task={}, quadratic kappa={}".format(k, task, round(float(res["q_kappa"].mean()), 3)))
        else:
            print("k={}, task={}, auc={} +/- {}".format(k, task, round(float(res["auc"].mean()), 3), round(float(res["auc"].std()), 3)))
        store = {m: res[m].tolist() for m in ("auc", "bacc", "q_kappa") if m in res}
        with open(os.path.join(save, "k=%d_probing_%s.pickle" % (k, task.replace("/", ""))), "wb") as f:
            pickle.dump({"tangle": store}, f, protocol=pickle.HIGHEST_PROTOCOL)
    if args.bootstrap:
        print("\n".join(_bootstrap_lines(linear_probe_ci(arms, labels, **ci), "k", args.level)))


if __name__ == "__main__":
    _main()
