"""Measures the bootstrap counts of the probes on an MI355X against two restatements of the same counting, at the
two shapes a user runs:

  few_shot   S = 1153 cases (ACROBAT's cohort), 90 binary problems (3 tasks x 3 k x 10 folds, k training cases per class), R = 1000
             replicates, two arms: two calls of functional.boot_class_counts;
  cv         5 cross-validation folds at S = 16384, binary, R = 1000, one arm.

Per shape, after one warm-up call of each leg and with the legs alternated inside one process:

  1. functional.boot_class_counts by device events (prepare + rank + replicate kernels, the draws included);
  2. a torch-on-device restatement by device events: per problem one sort of the test scores, then for ALL replicates at once the
     cumulative outside weight along the order, read by searchsorted at every case of the class -- given the weight vectors ready-made
     (functional.boot_weights, not timed), and checked to give the same integers;
  3. (few_shot only) a numpy loop on the CPU over problems and replicates by a host clock, on the same ready-made weights, with the
     thread count -- without the copies between device and host that this path also pays.

The comparison is against these restatements, never against this code itself.

       python tools/exp_resample.py [--steps 3] [--replicates 1000] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from madeleine_amd import functional as MF  # noqa: E402


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def few_shot_shape(arm):
    """(z [90, 1153, 1], y [90, 1153], table, n_train, group): gaussian scores shifted by the label, k = 1, 10, 25 cases per class."""
    rng = np.random.default_rng(100 + arm)
    S, rows, ys, groups = 1153, [], [], []
    for task in range(3):
        y = np.random.default_rng(task).integers(0, 2, S)
        for k in (1, 10, 25):
            for fold in range(10):
                pick = np.random.default_rng(1000 * k + fold + task)
                rows.append(np.concatenate([pick.choice(np.nonzero(y == c)[0], k, replace=False) for c in (0, 1)]))
                ys.append(y)
                groups.append(task)
    table = np.full((len(rows), 50), -1, dtype=np.int32)
    for p, r in enumerate(rows):
        table[p, :len(r)] = r
    y = np.stack(ys)
    z = (rng.standard_normal(y.shape) + 0.8 * (2 * y - 1)).astype(np.float32)[:, :, None]
    return z, y, table, np.array([len(r) for r in rows], dtype=np.int32), np.array(groups, dtype=np.int32)


def cv_shape():
    rng = np.random.default_rng(7)
    S, folds = 16384, 5
    y = rng.integers(0, 2, S)
    fold_of = rng.permutation(S) % folds
    rows = [np.nonzero(fold_of != f)[0] for f in range(folds)]
    table = np.full((folds, max(map(len, rows))), -1, dtype=np.int32)
    for p, r in enumerate(rows):
        table[p, :len(r)] = r
    z = (rng.standard_normal((folds, S)) + 0.8 * (2 * y - 1)).astype(np.float32)[:, :, None]
    return z, np.stack([y] * folds), table, np.array([len(r) for r in rows], dtype=np.int32), np.zeros(folds, dtype=np.int32)


def test_sets(y, table, n_train):
    out = []
    for p in range(y.shape[0]):
        test = y[p] >= 0
        test[table[p, :n_train[p]]] = False
        out.append(np.nonzero(test)[0])
    return out


def torch_restatement(z, y, tests, w, group):
    """(confusion [P, R + 1, 2, 2], num [P, R + 1]) int64 on the device: a sort per problem, searchsorted for all replicates at once."""
    conf, num = [], []
    for p, idx in enumerate(tests):
        s, t, W = z[p, idx, 0], y[p, idx], w[group[p]][:, idx].to(torch.int64)
        pos, neg = t == 1, t == 0
        order = torch.argsort(s[neg])
        neg_sorted = s[neg][order]
        cum = torch.nn.functional.pad(torch.cumsum(W[:, neg][:, order], 1), (1, 0))
        lt = torch.searchsorted(neg_sorted, s[pos], right=False)
        le = torch.searchsorted(neg_sorted, s[pos], right=True)
        num.append((W[:, pos] * (cum[:, lt] + cum[:, le])).sum(1))                       # 2 below + tied = below + (below + tied)
        cell = (2 * t + (s > 0)).to(torch.int64)
        conf.append((W.double() @ torch.nn.functional.one_hot(cell, 4).double()).to(torch.int64).view(-1, 2, 2))
    return torch.stack(conf), torch.stack(num)


def numpy_loop(z, y, tests, w, group):
    P, reps = len(tests), w.shape[1]
    conf, num = np.zeros((P, reps, 2, 2), dtype=np.int64), np.zeros((P, reps), dtype=np.int64)
    for p, idx in enumerate(tests):
        s, t = z[p, idx, 0], y[p, idx]
        pos, neg = t == 1, t == 0
        order = np.argsort(s[neg], kind="stable")
        neg_sorted = s[neg][order]
        lt, le = np.searchsorted(neg_sorted, s[pos], "left"), np.searchsorted(neg_sorted, s[pos], "right")
        cell = 2 * t + (s > 0)
        for r in range(reps):
            W = w[group[p], r, idx].astype(np.int64)
            cum = np.concatenate([[0], np.cumsum(W[neg][order])])
            num[p, r] = (W[pos] * (cum[lt] + cum[le])).sum()
            conf[p, r] = np.bincount(cell, weights=W, minlength=4).reshape(2, 2)
    return conf, num


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--replicates", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("exp_resample.py measures on a GPU; none is visible")
    dev, R, seed = torch.device("cuda:0"), a.replicates, 0
    report = {"device": torch.cuda.get_device_name(0), "cpu_threads": torch.get_num_threads(), "steps": a.steps, "replicates": R,
              "shapes": {}}
    for name, arms in (("few_shot", [few_shot_shape(0), few_shot_shape(1)]), ("cv", [cv_shape()])):
        host = arms
        devs = [tuple(torch.from_numpy(x).to(dev) for x in arm) for arm in arms]
        devs = [(z, y.to(torch.int32), tb, n, g) for z, y, tb, n, g in devs]
        tests = [test_sets(arm[1], arm[2], arm[3]) for arm in host]
        tests_dev = [[torch.from_numpy(i).to(dev) for i in ts] for ts in tests]
        n_groups = int(max(arm[4].max() for arm in host)) + 1
        S = host[0][0].shape[1]
        w = MF.boot_weights(seed, torch.arange(n_groups, dtype=torch.int32, device=dev), R, S)
        w = w.view(torch.int16).to(torch.int32) & 0xFFFF                                 # uint16 -> int32
        y_long = [arm[1].long() for arm in devs]

        def kernel():
            return [MF.boot_class_counts(z, y, tb, n, 2, g, seed, R) for z, y, tb, n, g in devs]

        def restated():
            return [torch_restatement(d[0], y, ts, w, arm[4]) for d, y, ts, arm in zip(devs, y_long, tests_dev, host)]

        got, ref = kernel(), restated()                                                  # warm-up, and the check
        for (conf, num), (conf_r, num_r) in zip(got, ref):
            assert torch.equal(conf.long(), conf_r) and torch.equal(num[:, :, 0], num_r), "the restatement disagrees with the kernels"
        ms = {"kernels": [], "torch_restatement": []}
        for _ in range(a.steps):
            ms["kernels"].append(event_ms(kernel)[0])
            ms["torch_restatement"].append(event_ms(restated)[0])
        entry = {"S": S, "problems_per_arm": int(host[0][1].shape[0]), "arms": len(host),
                 "test_cases_per_problem": int(statistics.median(len(t) for t in tests[0])),
                 "device_ms": {k: stats(v) for k, v in ms.items()}}
        if name == "few_shot":
            w_host = w.cpu().numpy()
            t0 = time.perf_counter()
            cpu = [numpy_loop(arm[0], arm[1], ts, w_host, arm[4]) for arm, ts in zip(host, tests)]
            entry["numpy_loop_s"] = time.perf_counter() - t0
            for (conf, num), (conf_c, num_c) in zip(got, cpu):
                assert np.array_equal(conf.cpu().numpy(), conf_c) and np.array_equal(num.cpu().numpy()[:, :, 0], num_c)
        report["shapes"][name] = entry
        print(name, json.dumps(entry))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
