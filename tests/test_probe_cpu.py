"""Host side of the linear probe, no GPU: the entry points and their argument validation (every refusal returns before a launch), the
split rule, the host formulae for balanced accuracy and quadratic kappa, and the command line's CSV / pickle handling."""
import csv
import os
import pickle

import numpy as np
import pytest
import torch

ENTRY_POINTS = ["mdl_probe_fit_ws_bytes", "mdl_probe_fit", "mdl_probe_scores", "mdl_probe_metrics_ws_bytes", "mdl_probe_metrics"]


def test_entry_points_declared_bound_and_exported():
    import madeleine_amd
    from madeleine_amd import _native, functional as F, probe
    assert _native.ABI_VERSION == 26 and _native.lib().mdl_abi_version() == 26
    for name in ENTRY_POINTS:
        assert name in _native.SIGNATURES and getattr(_native.lib(), name).argtypes == _native.SIGNATURES[name][1], name
    assert len(_native.SIGNATURES["mdl_probe_fit"][1]) == 19 and len(_native.SIGNATURES["mdl_probe_metrics"][1]) == 13
    for name in ("probe_fit", "probe_scores", "probe_metrics"):
        assert callable(getattr(F, name))
    for name in ("probe_splits", "fit_logistic", "linear_probe"):
        assert getattr(madeleine_amd, name) is getattr(probe, name) and name in madeleine_amd.__all__


def test_argument_validation_return_codes():
    """Every refusal below is decided on the host before anything is launched: the pointers are never dereferenced."""
    from madeleine_amd import _native
    lib, d = _native.lib(), _native._DEFINES
    ARG, UNS, ALIGN = d["MDL_E_ARG"], d["MDL_E_UNSUPPORTED"], d["MDL_E_ALIGN"]
    q = 4096      # a non-null, 16-byte aligned address
    assert lib.mdl_probe_fit_ws_bytes(90, 50, 512, 2) == 90 * 64 * 64 * 4
    assert lib.mdl_probe_fit_ws_bytes(1, 256, 1, 8) == 256 * 256 * 4
    assert lib.mdl_probe_fit_ws_bytes(1, 257, 8, 2) == UNS and lib.mdl_probe_fit_ws_bytes(1, 8, 8, 9) == UNS
    assert lib.mdl_probe_fit_ws_bytes(1, 8, 8, 1) == UNS and lib.mdl_probe_fit_ws_bytes(0, 8, 8, 2) == ARG
    assert lib.mdl_probe_metrics_ws_bytes(2, 100, 2) == 2 * 112 + 2 * 8 * 8
    assert lib.mdl_probe_metrics_ws_bytes(2, 100, 3) == 2 * 112 + 2 * 8 * 8 + 2 * 3 * 100 * 8
    assert lib.mdl_probe_metrics_ws_bytes(1, 16385, 2) == UNS and lib.mdl_probe_metrics_ws_bytes(1, 16384, 2) > 0

    def fit(X=q, ldX=8, S=100, dd=8, y=q, ldy=0, ti=q, nt=q, P=4, n_max=10, C=2, cost=1.0, gtol=1e-4, it=10, W=q, b=q, info=q, ws=q):
        return lib.mdl_probe_fit(X, ldX, S, dd, y, ldy, ti, nt, P, n_max, C, cost, gtol, it, W, b, info, ws, None)

    for null in ("X", "y", "ti", "nt", "W", "b", "info", "ws"):
        assert fit(**{null: None}) == ARG, null
    assert fit(ldX=7) == ARG and fit(dd=0, ldX=0) == ARG and fit(P=0) == ARG and fit(S=0) == ARG and fit(it=-1) == ARG
    assert fit(ldy=50) == ARG and fit(cost=0.0) == ARG
    assert fit(n_max=257) == UNS and fit(C=9) == UNS and fit(C=1) == UNS and fit(S=2 ** 31) == UNS and fit(P=2 ** 31) == UNS
    assert fit(ws=q + 4) == ALIGN

    def scores(X=q, ldX=8, S=100, dd=8, W=q, b=q, P=4, C=2, z=q):
        return lib.mdl_probe_scores(X, ldX, S, dd, W, b, P, C, z, None)

    for null in ("X", "W", "b", "z"):
        assert scores(**{null: None}) == ARG, null
    assert scores(ldX=7) == ARG and scores(P=0) == ARG and scores(C=9) == UNS and scores(S=2 ** 31) == UNS
    assert scores(P=2 ** 28, S=2 ** 10) == UNS      # the launch grid leaves int32

    def metrics(z=q, y=q, ldy=0, ti=q, nt=q, P=4, n_max=10, S=100, C=2, conf=q, auc=q, ws=q):
        return lib.mdl_probe_metrics(z, y, ldy, ti, nt, P, n_max, S, C, conf, auc, ws, None)

    for null in ("z", "y", "ti", "nt", "conf", "auc", "ws"):
        assert metrics(**{null: None}) == ARG, null
    assert metrics(S=16385) == UNS and metrics(C=9) == UNS and metrics(n_max=257) == UNS and metrics(ldy=99) == ARG
    assert metrics(ws=q + 8) == ALIGN


def test_probe_splits():
    from madeleine_amd import probe_splits
    y = torch.tensor([0, 1, 2, -1, 0, 1, 2, 0, 1, -1, 0, 1, 2, 0, 1, 0, 0, 2, -1, 1])
    for k in (1, 2, 4):
        idx = probe_splits(y, k, 3)
        assert idx.dtype == torch.int64 and idx.numel() == 3 * k and idx.unique().numel() == 3 * k
        assert y[idx].tolist() == [c for c in range(3) for _ in range(k)]      # k per class, classes in increasing order; never -1
        test = (y >= 0)
        test[idx] = False
        assert int(test.sum()) == int((y >= 0).sum()) - 3 * k
        assert torch.equal(idx, probe_splits(y.numpy(), k, 3)) and torch.equal(idx, probe_splits(y.tolist(), k, 3, seed_base=0))
    draws = {tuple(probe_splits(y, 2, fold, seed).tolist()) for fold in range(6) for seed in (0, 7)}
    assert len(draws) > 6                            # fold and seed_base move the draw
    assert torch.equal(probe_splits(y, 2, 5, seed_base=1000), probe_splits(y, 3, 5, seed_base=0)[[0, 1, 3, 4, 6, 7]])   # one seed, one permutation
    # the documented rule, restated
    g = torch.Generator().manual_seed(11 + 1000 * 2 + 4)
    want = torch.cat([(y == c).nonzero()[:, 0][torch.randperm(int((y == c).sum()), generator=g)[:2]] for c in range(3)])
    assert torch.equal(probe_splits(y, 2, 4, seed_base=11), want)
    with pytest.raises(ValueError):
        probe_splits(y, 5, 0)                        # class 2 has 4 cases
    with pytest.raises(ValueError):
        probe_splits(torch.tensor([0, 2, 2, 0, -1]), 1, 0)      # class 1 has no case


def test_host_metrics_on_hand_computed_matrices():
    from madeleine_amd.probe import balanced_accuracy, quadratic_kappa
    # recalls 8/10 and 3/5; po = 11/15, pe = (10 * 10 + 5 * 5) / 225 = 5/9: kappa = (11/15 - 5/9) / (4/9) = 0.4
    cm = [[8, 2], [2, 3]]
    assert abs(balanced_accuracy(cm) - 0.7) < 1e-15 and abs(quadratic_kappa(cm) - 0.4) < 1e-15
    # three grades: disagreement sum w * cm = 1 * (1 + 1 + 1 + 1) + 4 * (1 + 0) = 8; expected, rows (4, 4, 4), columns (4, 4, 4), N 12:
    # sum w * 16 / 12 = (4 * 1 + 2 * 4) * 16 / 12 = 16: kappa = 1 - 8 / 16 = 0.5; recalls 2/4, 2/4, 3/4
    cm = [[2, 1, 1], [1, 2, 1], [0, 1, 3]]
    assert abs(balanced_accuracy(cm) - 7 / 12) < 1e-15 and abs(quadratic_kappa(cm) - 0.5) < 1e-15
    # a class without a case is left out of the balanced accuracy (sklearn); perfect agreement is kappa 1
    cm = [[5, 0, 0], [0, 0, 0], [0, 0, 2]]
    assert balanced_accuracy(cm) == 1.0 and quadratic_kappa(cm) == 1.0
    assert np.isnan(quadratic_kappa([[3, 0], [0, 0]])) and np.isnan(balanced_accuracy([[0, 0], [0, 0]]))


def test_cli_reads_csv_and_writes_pickles(tmp_path, monkeypatch, capsys):
    from madeleine_amd import probe
    ids = ["s%d" % i for i in range(6)]
    embeds = np.arange(24, dtype=np.float32).reshape(6, 4)
    pkl = tmp_path / "madeleine_slide_embeddings.pkl"
    with open(pkl, "wb") as f:
        pickle.dump({"embeds": embeds, "slide_ids": ids}, f)
    with open(tmp_path / "BCNB.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["slide_id", "er", "pr", "her2"])
        for i in (5, 0, 2, 3, 9):                    # s1, s4 have no label row; s9 has no embedding; CSV order is not pickle order
            w.writerow(["s%d" % i, i % 2, -1 if i == 2 else 1, 0])
    seen = {}

    def fake(e, labels, **kw):
        seen.update(embeds=e, labels=labels, kw=kw)
        return {(t, k): {"auc": np.array([0.5, 0.75]), "bacc": np.array([0.25, 0.5]), "converged": np.array([True, True]),
                         "confusion": np.zeros((2, 2, 2), dtype=np.int64)} for t in labels for k in (1, 10)}

    monkeypatch.setattr(probe, "linear_probe", fake)
    probe._main(["--slide_embedding_pkl", str(pkl), "--label_path", str(tmp_path / "BCNB.csv"), "--tasks", "er", "pr"])
    assert np.array_equal(seen["embeds"], embeds[[0, 2, 3, 5]])
    assert seen["labels"]["er"].tolist() == [0, 0, 1, 1] and seen["labels"]["pr"].tolist() == [1, -1, 1, 1] and set(seen["labels"]) == {"er", "pr"}
    out = capsys.readouterr().out.splitlines()
    assert out == ["k=%d, task=%s, auc=0.625 +/- 0.125" % (k, t) for t in ("er", "pr") for k in (1, 10)]
    folder = tmp_path / "res_linear_probing" / "madeleine_slide_embeddings"
    assert sorted(os.listdir(folder)) == sorted("k=%d_probing_%s.pickle" % (k, t) for t in ("er", "pr") for k in (1, 10))
    with open(folder / "k=10_probing_pr.pickle", "rb") as f:
        assert pickle.load(f) == {"tangle": {"auc": [0.5, 0.75], "bacc": [0.25, 0.5]}}
