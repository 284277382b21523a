"""Bootstrap intervals and paired comparisons for the probes: is one slide encoder better than another on this cohort, and with what
uncertainty?  The cohort's cases are resampled with replacement `replicates` times; every fold's metric of every arm is recomputed
under the same resample on the device (exact integer counts: include/madeleine_amd_stats.h), and the percentile interval of each arm
and of the paired difference is read on the host.

    from madeleine_amd import linear_probe_ci
    res = linear_probe_ci({"madeleine": E, "mean": E_mean}, {"er": er}, ks=(10,), replicates=1000)
    res[("er", 10)]["arms"]["madeleine"]["auc"]              # {"point", "lo", "hi", "n_valid"}
    res[("er", 10)]["pairs"][("madeleine", "mean")]["auc"]   # {"diff", "lo", "hi", "p", "n_valid"}: diff = first arm - second arm

Only the test sets are resampled: the fits are those of the sample (the splits of probe_splits / cv_splits / survival_splits, shared by
all arms).  The standard deviation over the few-shot folds is no substitute: their test sets overlap almost completely."""
import warnings

import numpy as np
import torch

from . import functional as F
from . import probe as _probe
from . import survival as _survival

__all__ = ["bootstrap_summary", "paired_difference", "auc_from_counts", "c_index_from_counts", "linear_probe_ci", "survival_probe_ci"]


def _level(level):
    level = float(level)
    if not 0.0 < level < 1.0:
        raise ValueError("bootstrap: level must lie inside (0, 1) (got %r)" % level)
    return level


def bootstrap_summary(values, level=0.95):
    """{"point", "lo", "hi", "n_valid"} of values [R + 1, ...] (row 0: the sample; rows 1 .. R: the replicates), in fp64: the point value
    and the percentile interval -- np.quantile, linear, at (1 - level) / 2 and 1 - (1 - level) / 2 -- over the finite replicates of every
    column, with their number.  Replicates that are not finite are counted out, never silently: n_valid says how many remain (0: NaN
    bounds).  Floats / an int for a vector, arrays of the trailing shape otherwise."""
    level = _level(level)
    v = np.asarray(values, dtype=np.float64)
    if v.ndim < 1 or v.shape[0] < 1:
        raise ValueError("bootstrap_summary: values must be [R + 1, ...]")
    flat = v.reshape(v.shape[0], -1)
    lo, hi = np.full(flat.shape[1], np.nan), np.full(flat.shape[1], np.nan)
    n_valid = np.zeros(flat.shape[1], dtype=np.int64)
    for c in range(flat.shape[1]):
        rep = flat[1:, c]
        rep = rep[np.isfinite(rep)]
        n_valid[c] = rep.size
        if rep.size:
            lo[c], hi[c] = np.quantile(rep, [(1.0 - level) / 2.0, 1.0 - (1.0 - level) / 2.0])
    if v.ndim == 1:
        return {"point": float(v[0]), "lo": float(lo[0]), "hi": float(hi[0]), "n_valid": int(n_valid[0])}
    shape = v.shape[1:]
    return {"point": v[0].copy(), "lo": lo.reshape(shape), "hi": hi.reshape(shape), "n_valid": n_valid.reshape(shape)}


def paired_difference(a, b, level=0.95):
    """{"diff", "lo", "hi", "p", "n_valid"} of two arms' replicate vectors [R + 1] under the SAME resamples: the difference a - b of the
    sample, its percentile interval over the n replicates in which both are finite, and the two-sided bootstrap p-value
    p = min(1, 2 min((#{d* <= 0} + 1) / (n + 1), (#{d* >= 0} + 1) / (n + 1)))."""
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    if d.ndim != 1 or d.shape[0] < 1:
        raise ValueError("paired_difference: the arms must be vectors [R + 1] of one length")
    s = bootstrap_summary(d, level)
    rep = d[1:][np.isfinite(d[1:])]
    n = rep.size
    p = min(1.0, 2.0 * min((int((rep <= 0).sum()) + 1) / (n + 1), (int((rep >= 0).sum()) + 1) / (n + 1)))
    return {"diff": s["point"], "lo": s["lo"], "hi": s["hi"], "p": float(p), "n_valid": s["n_valid"]}


def auc_from_counts(confusion, auc_num):
    """fp64 [...] from confusion [..., C, C] and auc_num [..., cols] (boot_class_counts): per class column num / (2 pos neg) with pos
    the weight of the class (its row sum) and neg the rest, macro-averaged.  NaN where a class or its complement has no weight in the
    resample, or where the numerator is -1 (a NaN score)."""
    conf, num = np.asarray(confusion, dtype=np.float64), np.asarray(auc_num, dtype=np.float64)
    C, cols = conf.shape[-1], num.shape[-1]
    rows = conf.sum(-1)
    total = rows.sum(-1)
    out = np.zeros(num.shape[:-1])
    with np.errstate(all="ignore"):
        for ci in range(cols):
            pos = rows[..., 1 if C == 2 else ci]
            neg = total - pos
            term = num[..., ci] / (2.0 * pos * neg)
            out = out + np.where((pos > 0) & (neg > 0) & (num[..., ci] >= 0), term, np.nan)
    return out / cols


def c_index_from_counts(counts):
    """fp64 [...] from counts [..., 2] (boot_surv_counts): numerator / (2 comparable), NaN without a comparable pair."""
    counts = np.asarray(counts, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(counts[..., 1] > 0, counts[..., 0] / (2.0 * counts[..., 1]), np.nan)


def _arms(embeds, who):
    """{arm: X [S, d] fp32 on the device} of one matrix (arm "embeds") or a dict of matrices over the same cases."""
    if not torch.cuda.is_available():
        raise RuntimeError("madeleine_amd: %s needs a ROCm device; there is no CPU fallback" % who)
    arms = embeds if isinstance(embeds, dict) else {"embeds": embeds}
    if not arms:
        raise ValueError("%s: no embeddings" % who)
    out = {}
    for name, E in arms.items():
        X = torch.as_tensor(E)
        X = X.to(device=X.device if X.is_cuda else "cuda", dtype=torch.float32)
        if X.dim() != 2:
            raise ValueError("%s: embeds of arm %r must be [S, d]" % (who, name))
        if X.stride(-1) != 1:
            X = X.contiguous()
        out[name] = X
    if len({X.shape[0] for X in out.values()}) != 1:
        raise ValueError("%s: the arms must hold the same cases (got %s rows)" % (who, sorted(X.shape[0] for X in out.values())))
    if not bool(torch.stack([torch.isfinite(X).all() for X in out.values()]).all()):
        raise ValueError("%s: embeds holds non-finite values" % who)
    return out


def _pairs(arm_values, metrics, level):
    """{(a, b): {metric: paired_difference}} over the arm pairs in the order given, a before b."""
    names = list(arm_values)
    return {(a, b): {m: paired_difference(arm_values[a][m], arm_values[b][m], level) for m in metrics}
            for i, a in enumerate(names) for b in names[i + 1:]}


def linear_probe_ci(embeds, labels, protocol="few_shot", ks=(1, 10, 25), folds=None, repeats=1, cost=1.0, replicates=1000, level=0.95,
                    seed=0, seed_base=0, kappa=False, gtol=1e-4, max_iter=100):
    """Bootstrap intervals of the linear probe, and paired differences between arms.  embeds: one [S, d] matrix or a dict arm -> [S, d]
    over the same cases; labels: one [S] vector (task "label") or a dict task -> [S], -1 = unlabeled.  protocol "few_shot": the
    problems of linear_probe (probe_splits over ks x folds, folds = 10 by default); "cv": those of linear_probe_cv (cv_splits over
    repeats x folds, folds = 5 by default).  The splits are shared by all arms, the fits and scores are those of the probes, and every
    problem of a task carries the task's index as its group: replicate r resamples the cohort ONCE for all folds and arms.  The statistic
    of a replicate is the mean over the folds of the fold's AUC / balanced accuracy (q_kappa too with kappa=True), in fp64 from the
    integer counts; a fold without a value (a class lost by the resample) makes that replicate invalid for that metric: n_valid counts
    the others.  Returns {(task, k or repeat): {"arms": {arm: {"auc": {"point", "lo", "hi", "n_valid"}, "bacc": ..., "replicates":
    {"auc": [R + 1], "bacc": [R + 1]}, "converged": [folds] bool}}, "pairs": {(arm a, arm b): {"auc": {"diff", "lo", "hi", "p",
    "n_valid"}, "bacc": ...}}}}; diff is a - b, a the arm given first.  Two host reads: the finiteness check and the results."""
    if protocol not in ("few_shot", "cv"):
        raise ValueError("linear_probe_ci: protocol must be 'few_shot' or 'cv' (got %r)" % (protocol,))
    level, R = _level(level), int(replicates)
    if R < 1:
        raise ValueError("linear_probe_ci: replicates must be >= 1")
    arms = _arms(embeds, "linear_probe_ci")
    dev = next(iter(arms.values())).device
    S = next(iter(arms.values())).shape[0]
    folds = int(folds) if folds is not None else (10 if protocol == "few_shot" else 5)
    tasks = labels if isinstance(labels, dict) else {"label": labels}
    groups = {}                                     # C -> [(task, k or repeat, fold, y, train indices, task index)]
    for g, (task, y) in enumerate(tasks.items()):
        y = torch.as_tensor(np.asarray(y.cpu() if isinstance(y, torch.Tensor) else y)).long()
        if y.shape != (S,):
            raise ValueError("linear_probe_ci: task %r has %s labels for %d embeddings" % (task, tuple(y.shape), S))
        C = int(y.max()) + 1
        if protocol == "few_shot":
            for k in ks:
                for fold in range(folds):
                    groups.setdefault(C, []).append((task, k, fold, y, _probe.probe_splits(y, k, fold, seed_base), g))
        else:
            for repeat in range(repeats):
                for fold, idx in enumerate(_probe.cv_splits(y, folds, repeat, seed_base)):
                    groups.setdefault(C, []).append((task, repeat, fold, y, idx, g))
    fit = F.probe_fit if protocol == "few_shot" else F.logit_fit
    parts, layout = [], []
    for C, probs in groups.items():
        table, n_train = _probe._problem_table([p[4] for p in probs], dev)
        y_dev = torch.stack([p[3] for p in probs]).to(torch.int32).to(dev)
        group = torch.tensor([p[5] for p in probs], dtype=torch.int32).to(dev)
        for arm, X in arms.items():
            W, b, info = fit(X, y_dev, table, n_train, C, cost, gtol, max_iter)
            confusion, auc_num = F.boot_class_counts(F.probe_scores(X, W, b, C), y_dev, table, n_train, C, group, seed, R)
            parts += [info[:, 1].long(), confusion.reshape(-1).long(), auc_num.reshape(-1)]
            layout.append((C, arm, probs))
    host = torch.cat(parts).cpu().numpy()           # the one read of the results
    metrics = ("auc", "bacc") + (("q_kappa",) if kappa else ())
    folded, conv_of, at, failed, total = {}, {}, 0, 0, 0      # (unit, arm) -> {metric: [folds, R + 1]}
    for C, arm, probs in layout:
        P, cols = len(probs), 1 if C == 2 else C
        conv = host[at:at + P] > 0
        cm = host[at + P:at + P + P * (R + 1) * C * C].reshape(P, R + 1, C, C)
        num = host[at + P + cm.size:at + P + cm.size + P * (R + 1) * cols].reshape(P, R + 1, cols)
        at += P + cm.size + num.size
        failed, total = failed + int((~conv).sum()), total + P
        auc = auc_from_counts(cm, num)
        for p, (task, unit, fold, _, _, _) in enumerate(probs):
            res = folded.setdefault(((task, unit), arm), {m: np.zeros((folds, R + 1)) for m in metrics})
            res["auc"][fold] = auc[p]
            res["bacc"][fold] = [_probe.balanced_accuracy(cm[p, r]) for r in range(R + 1)]
            if kappa:
                res["q_kappa"][fold] = [_probe.quadratic_kappa(cm[p, r]) for r in range(R + 1)]
            conv_of.setdefault(((task, unit), arm), np.zeros(folds, dtype=bool))[fold] = conv[p]
    out = {}
    for (key, arm), res in folded.items():
        reps = {m: res[m].mean(0) for m in metrics}      # [folds, R + 1] -> [R + 1]; a fold without a value: NaN, invalid
        entry = {m: bootstrap_summary(reps[m], level) for m in metrics}
        entry["replicates"], entry["converged"] = reps, conv_of[(key, arm)]
        out.setdefault(key, {"arms": {}, "pairs": {}})["arms"][arm] = entry
    for key, res in out.items():
        res["pairs"] = _pairs({arm: e["replicates"] for arm, e in res["arms"].items()}, metrics, level)
    if failed:
        warnings.warn("linear_probe_ci: %d of %d fits did not reach gtol = %g in %d Newton steps" % (failed, total, gtol, max_iter),
                      RuntimeWarning)
    return out


def survival_probe_ci(embeds, time, event, folds=5, repeats=1, cost=1.0, replicates=1000, level=0.95, seed=0, seed_base=0,
                      gtol=_survival.GTOL, max_iter=100):
    """Bootstrap intervals of the survival probe's C-index, and paired differences between arms.  embeds: one [S, d] matrix or a dict
    arm -> [S, d] over the same cases; time and event as for survival_probe (vectors, or dicts over the same endpoints).  The splits are
    survival_splits', shared by all arms; every problem of an endpoint carries the endpoint's index as its group.  The statistic of a
    replicate is the mean over the folds of the fold's C-index; a fold without a comparable pair makes the replicate invalid.  Returns
    {(endpoint, repeat): {"arms": {arm: {"c_index": {"point", "lo", "hi", "n_valid"}, "replicates": {"c_index": [R + 1]}, "converged":
    [folds] bool}}, "pairs": {(arm a, arm b): {"c_index": {"diff", "lo", "hi", "p", "n_valid"}}}}}.  S <= BOOT_SURV_MAX_TEST.  Two host
    reads: the finiteness check and the results."""
    level, R = _level(level), int(replicates)
    if R < 1:
        raise ValueError("survival_probe_ci: replicates must be >= 1")
    arms = _arms(embeds, "survival_probe_ci")
    dev = next(iter(arms.values())).device
    S = next(iter(arms.values())).shape[0]
    if isinstance(time, dict) != isinstance(event, dict) or (isinstance(time, dict) and set(time) != set(event)):
        raise ValueError("survival_probe_ci: time and event must both be vectors, or dicts over the same endpoints")
    times, events = (time, event) if isinstance(time, dict) else ({"survival": time}, {"survival": event})
    probs, t_rows, e_rows = [], [], []              # (endpoint, repeat, fold, training indices, endpoint index)
    for g, name in enumerate(times):
        t = _survival._host_vector(times[name], S, "times", name).float()
        e = _survival._host_vector(events[name], S, "events", name).long()
        for repeat in range(repeats):
            for fold, idx in enumerate(_survival.survival_splits(e, folds, repeat, seed_base)):
                probs.append((name, repeat, fold, idx, g))
                t_rows.append(t)
                e_rows.append(e)
    P = len(probs)
    table, n_train = _survival._problem_table([p[3] for p in probs], dev)
    t_dev = F.h2d(torch.stack(t_rows), dev)
    e_dev = F.h2d(torch.stack(e_rows), dev, torch.int32)
    group = F.h2d(torch.tensor([p[4] for p in probs], dtype=torch.int32), dev)
    parts = []
    for arm, X in arms.items():
        W, thr, info = F.cox_fit(X, t_dev, e_dev, table, n_train, cost, gtol, max_iter)
        z = F.probe_scores(X, W.unsqueeze(1), torch.zeros(P, 1, device=dev), 2).squeeze(2)
        parts += [info[:, 1].long(), F.boot_surv_counts(z, t_dev, e_dev, table, n_train, group, seed, R).reshape(-1)]
    host = torch.cat(parts).cpu().numpy()           # the one read of the results
    out, at, failed = {}, 0, 0
    for arm in arms:
        conv = host[at:at + P] > 0
        c = c_index_from_counts(host[at + P:at + P + P * (R + 1) * 2].reshape(P, R + 1, 2))
        at += P + P * (R + 1) * 2
        failed += int((~conv).sum())
        folded, conv_of = {}, {}
        for p, (name, repeat, fold, _, _) in enumerate(probs):
            folded.setdefault((name, repeat), np.zeros((folds, R + 1)))[fold] = c[p]
            conv_of.setdefault((name, repeat), np.zeros(folds, dtype=bool))[fold] = conv[p]
        for key, per_fold in folded.items():
            reps = per_fold.mean(0)                     # a fold without a comparable pair: NaN, the replicate is invalid
            out.setdefault(key, {"arms": {}, "pairs": {}})["arms"][arm] = {
                "c_index": bootstrap_summary(reps, level), "replicates": {"c_index": reps}, "converged": conv_of[key]}
    for key, res in out.items():
        res["pairs"] = _pairs({arm: e["replicates"] for arm, e in res["arms"].items()}, ("c_index",), level)
    if failed:
        warnings.warn("survival_probe_ci: %d of %d fits did not reach gtol = %g (relative) in %d Newton steps" % (
            failed, P * len(arms), gtol, max_iter), RuntimeWarning)
    return out
