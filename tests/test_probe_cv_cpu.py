"""Host side of the full-label linear probe, no GPU: the entry points and their argument validation (every refusal returns before a
launch), the workspace sizes the header documents, the stratified K-fold rule and the command line's --cv_folds switch."""
import csv
import pickle

import numpy as np
import pytest
import torch

ENTRY_POINTS = ["mdl_logit_fit_ws_bytes", "mdl_logit_fit", "mdl_logit_metrics_ws_bytes", "mdl_logit_metrics"]


def test_entry_points_declared_bound_and_exported():
    import madeleine_amd
    from madeleine_amd import _native, functional as F, probe
    assert _native.ABI_VERSION == 26 and _native.lib().mdl_abi_version() == 26
    for name in ENTRY_POINTS:
        assert name in _native.SIGNATURES and getattr(_native.lib(), name).argtypes == _native.SIGNATURES[name][1], name
    assert len(_native.SIGNATURES["mdl_logit_fit"][1]) == 19 and len(_native.SIGNATURES["mdl_logit_metrics"][1]) == 13
    assert len(_native.SIGNATURES["mdl_logit_fit_ws_bytes"][1]) == 4 and len(_native.SIGNATURES["mdl_logit_metrics_ws_bytes"][1]) == 3
    d = _native._DEFINES
    assert d["MDL_LOGIT_MAX_TRAIN"] == 16384 == d["MDL_PROBE_MAX_CASES"] and d["MDL_LOGIT_MAX_DIM"] == 1024
    assert d["MDL_LOGIT_CG_MAX"] == 400 and d["MDL_LOGIT_LS_MAX"] == 24
    for name in ("logit_fit", "logit_metrics"):
        assert callable(getattr(F, name))
    for name in ("cv_splits", "linear_probe_cv"):
        assert getattr(madeleine_amd, name) is getattr(probe, name) and name in madeleine_amd.__all__


def test_workspace_sizes():
    """mdl_logit_fit_ws_bytes = P (3 n4 cols + d nc) 4 with n4 = n_max rounded up to 4 and nc = 1 / 4 / 8; the metrics workspace is that
    of mdl_probe_metrics."""
    from madeleine_amd import _native
    lib, d = _native.lib(), _native._DEFINES
    ARG, UNS = d["MDL_E_ARG"], d["MDL_E_UNSUPPORTED"]
    assert lib.mdl_logit_fit_ws_bytes(15, 923, 512, 2) == 15 * (3 * 924 * 1 + 512 * 1) * 4
    assert lib.mdl_logit_fit_ws_bytes(5, 720, 512, 4) == 5 * (3 * 720 * 4 + 512 * 4) * 4
    assert lib.mdl_logit_fit_ws_bytes(2, 1, 7, 3) == 2 * (3 * 4 * 3 + 7 * 4) * 4
    assert lib.mdl_logit_fit_ws_bytes(1, 16384, 1024, 8) == (3 * 16384 * 8 + 1024 * 8) * 4
    assert lib.mdl_logit_fit_ws_bytes(1, 16385, 8, 2) == UNS and lib.mdl_logit_fit_ws_bytes(1, 8, 1025, 2) == UNS
    assert lib.mdl_logit_fit_ws_bytes(1, 8, 8, 9) == UNS and lib.mdl_logit_fit_ws_bytes(1, 8, 8, 1) == UNS
    assert lib.mdl_logit_fit_ws_bytes(0, 8, 8, 2) == ARG and lib.mdl_logit_fit_ws_bytes(1, 0, 8, 2) == ARG
    for P, S, C in ((2, 100, 2), (2, 100, 3), (25, 16384, 8)):
        assert lib.mdl_logit_metrics_ws_bytes(P, S, C) == lib.mdl_probe_metrics_ws_bytes(P, S, C) > 0
    assert lib.mdl_logit_metrics_ws_bytes(2, 100, 3) == 2 * 112 + 2 * 8 * 8 + 2 * 3 * 100 * 8
    assert lib.mdl_logit_metrics_ws_bytes(1, 16385, 2) == UNS and lib.mdl_logit_metrics_ws_bytes(1, 100, 9) == UNS
    assert lib.mdl_logit_metrics_ws_bytes(0, 100, 2) == ARG


def test_argument_validation_return_codes():
    """test_probe_cpu's cases with the limits moved.  Every refusal is decided on the host before anything is launched: the pointers are
    never dereferenced."""
    from madeleine_amd import _native
    lib, d = _native.lib(), _native._DEFINES
    ARG, UNS, ALIGN = d["MDL_E_ARG"], d["MDL_E_UNSUPPORTED"], d["MDL_E_ALIGN"]
    q = 4096      # a non-null, 16-byte aligned address

    def fit(X=q, ldX=8, S=100, dd=8, y=q, ldy=0, ti=q, nt=q, P=4, n_max=10, C=2, cost=1.0, gtol=1e-4, it=10, W=q, b=q, info=q, ws=q):
        return lib.mdl_logit_fit(X, ldX, S, dd, y, ldy, ti, nt, P, n_max, C, cost, gtol, it, W, b, info, ws, None)

    for null in ("X", "y", "ti", "nt", "W", "b", "info", "ws"):
        assert fit(**{null: None}) == ARG, null
    assert fit(ldX=7) == ARG and fit(dd=0, ldX=0) == ARG and fit(P=0) == ARG and fit(S=0) == ARG and fit(it=-1) == ARG
    assert fit(ldy=50) == ARG and fit(cost=0.0) == ARG and fit(n_max=0) == ARG
    assert fit(n_max=16385) == UNS and fit(dd=1025, ldX=1025) == UNS
    assert fit(C=9) == UNS and fit(C=1) == UNS and fit(S=2 ** 31) == UNS and fit(P=2 ** 31) == UNS
    assert fit(P=2 ** 20, n_max=4096) == UNS      # the problem table leaves int32
    assert fit(ws=q + 4) == ALIGN

    def metrics(z=q, y=q, ldy=0, ti=q, nt=q, P=4, n_max=10, S=100, C=2, conf=q, auc=q, ws=q):
        return lib.mdl_logit_metrics(z, y, ldy, ti, nt, P, n_max, S, C, conf, auc, ws, None)

    for null in ("z", "y", "ti", "nt", "conf", "auc", "ws"):
        assert metrics(**{null: None}) == ARG, null
    assert metrics(S=16385) == UNS and metrics(C=9) == UNS and metrics(n_max=16385) == UNS and metrics(ldy=99) == ARG
    assert metrics(ws=q + 8) == ALIGN
    # the few-shot launcher keeps its own limit
    assert lib.mdl_probe_metrics(q, q, 0, q, q, 4, 257, 100, 2, q, q, q, None) == UNS


def test_cv_splits():
    from madeleine_amd import cv_splits
    g = torch.Generator().manual_seed(5)
    y = torch.randint(0, 3, (211,), generator=g)
    y[::9] = -1
    labeled = torch.nonzero(y >= 0)[:, 0]
    for folds in (2, 5, 7):
        train = cv_splits(y, folds, repeat=1, seed_base=3)
        assert len(train) == folds and all(t.dtype == torch.int64 for t in train)
        held = []
        for t in train:
            assert torch.equal(t, t.sort().values) and t.unique().numel() == t.numel()      # ascending, no repeats
            assert bool((y[t] >= 0).all())                                                  # -1 is never drawn
            mask = y >= 0
            mask[t] = False
            held.append(torch.nonzero(mask)[:, 0])
        assert torch.equal(torch.cat(held).sort().values, labeled)                          # the held-out shares partition the labeled cases
        for c in range(3):
            sizes = [int((y[h] == c).sum()) for h in held]
            assert max(sizes) - min(sizes) <= 1, (folds, c, sizes)
        sizes = [h.numel() for h in held]
        assert max(sizes) - min(sizes) <= 1                                                 # the deal runs on across the classes
        again = cv_splits(y.numpy(), folds, repeat=1, seed_base=3)
        assert all(torch.equal(a, b) for a, b in zip(train, again))
    assert all(torch.equal(a, b) for a, b in zip(cv_splits(y), cv_splits(y.tolist(), 5, 0, 0)))
    draws = {tuple(cv_splits(y, 5, r, s)[0].tolist()) for r in range(3) for s in (0, 7)}
    assert len(draws) == 6                           # repeat and seed_base move the draw
    # the documented rule, restated
    gen = torch.Generator().manual_seed(11 + 1000 * 4 + 2)
    fold_of, dealt = torch.full_like(y, -1), 0
    for c in range(3):
        idx = (y == c).nonzero()[:, 0]
        idx = idx[torch.randperm(idx.numel(), generator=gen)]
        fold_of[idx] = (torch.arange(idx.numel()) + dealt) % 4
        dealt += idx.numel()
    for f, t in enumerate(cv_splits(y, 4, repeat=2, seed_base=11)):
        assert torch.equal(t, ((fold_of >= 0) & (fold_of != f)).nonzero()[:, 0])
    with pytest.raises(ValueError):
        cv_splits(torch.tensor([0, 1, 0, 1, 0, 1, 0, 0, 0, -1]), 5)        # class 1 has three cases, five folds
    with pytest.raises(ValueError):
        cv_splits(torch.tensor([-1, -1, -1]), 2)                          # no labeled case
    with pytest.raises(ValueError):
        cv_splits(torch.arange(20600) % 2, 5)                             # 16480 training cases per fold: above the limit
    assert max(t.numel() for t in cv_splits(torch.arange(20480) % 2, 5)) == 16384


def test_no_cpu_fallback(monkeypatch):
    from madeleine_amd import fit_logistic, functional as F, linear_probe_cv
    X, y = torch.zeros(300, 4), torch.zeros(300, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fit_logistic(X, y, [torch.arange(257)], 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.logit_fit(X, y, torch.zeros(1, 257, dtype=torch.int32), torch.ones(1, dtype=torch.int32), 2)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="needs a ROCm device"):
        linear_probe_cv(np.zeros((20, 4), dtype=np.float32), np.arange(20) % 2, folds=2)


def test_cli_cv_folds(tmp_path, monkeypatch, capsys):
    """--cv_folds runs linear_probe_cv and prints mean +/- std per task; without it the few-shot protocol runs as before."""
    from madeleine_amd import probe
    ids = ["s%d" % i for i in range(6)]
    pkl = tmp_path / "emb.pkl"
    with open(pkl, "wb") as f:
        pickle.dump({"embeds": np.arange(24, dtype=np.float32).reshape(6, 4), "slide_ids": ids}, f)
    with open(tmp_path / "labels.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["slide_id", "er", "pr"])
        for i in range(6):
            w.writerow(["s%d" % i, i % 2, 1])
    seen = {}

    def fake_cv(e, labels, **kw):
        seen.update(kw=kw, tasks=list(labels))
        return {(t, r): {"auc": np.array([0.5, 0.75]) + 0.1 * r, "bacc": np.array([0.25, 0.5]), "converged": np.array([True, True]),
                         "confusion": np.zeros((2, 2, 2), dtype=np.int64)} for t in labels for r in range(kw["repeats"])}

    def few_shot(*a, **kw):
        raise AssertionError("the few-shot protocol must not run under --cv_folds")

    monkeypatch.setattr(probe, "linear_probe_cv", fake_cv)
    monkeypatch.setattr(probe, "linear_probe", few_shot)
    probe._main(["--slide_embedding_pkl", str(pkl), "--label_path", str(tmp_path / "labels.csv"), "--tasks", "er", "pr", "--cv_folds", "2",
                 "--cv_repeats", "2"])
    assert seen["kw"] == {"folds": 2, "repeats": 2, "kappa": False} and seen["tasks"] == ["er", "pr"]
    v = np.array([0.5, 0.75, 0.6, 0.85])
    assert capsys.readouterr().out.splitlines() == ["cv_folds=2, task=%s, auc=%s +/- %s" % (t, round(float(v.mean()), 3),
                                                                                            round(float(v.std()), 3)) for t in ("er", "pr")]
