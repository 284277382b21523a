"""Host side of the test-set bootstrap (B1-B3, include/madeleine_amd_stats.h): the third header and its binding, the refusals that come
before any launch, the properties of the resampling weights in the host model (tests/_resample_ref.py), bootstrap_summary and the paired
p-value on fixed arrays, the command line's new options and the lazy names.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

from madeleine_amd import _build, _native
from tests import _resample_ref as M

P, I32, I64, U64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64
FAKE = 1 << 20          # a 16-byte aligned address nothing dereferences: every refusal below comes before the first launch
ARG, UNSUP, ALIGN = (_native._DEFINES[k] for k in ("MDL_E_ARG", "MDL_E_UNSUPPORTED", "MDL_E_ALIGN"))
NAMES = {"mdl_boot_weights", "mdl_boot_class_ws_bytes", "mdl_boot_class_counts", "mdl_boot_surv_counts"}


# ---- header and ABI ------------------------------------------------------------------------------------------------------------------
def test_the_third_header_parses_and_is_bound_beside_the_other_two():
    with open(_build.STATS_HEADER) as f:
        sigs, defines = _native._parse_header(f.read())
    assert sigs == _native.STATS_SIGNATURES and set(sigs) == NAMES and defines == _native.STATS_DEFINES
    assert sigs["mdl_boot_weights"] == (I32, [U64, P, I64, I64, I64, P, P])
    assert sigs["mdl_boot_class_ws_bytes"] == (I64, [I64, I64, I32])
    assert sigs["mdl_boot_class_counts"] == (I32, [P, P, I64, P, P, I64, I32, I64, I32, P, U64, I64, P, P, P, P])
    assert sigs["mdl_boot_surv_counts"] == (I32, [P, P, I64, P, I64, P, P, I64, I32, I64, P, U64, I64, P, P])
    assert defines == {"MDL_BOOT_REP_BLOCK": 8, "MDL_BOOT_SURV_MAX_TEST": 4096, "MDL_BOOT_LDS_RAISE_FROM": 12288}
    lib = _native.lib()
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)                          # exported by the built library
        assert fn.restype is res and fn.argtypes == args, name
    assert not NAMES & (set(_native.SIGNATURES) | set(_native.VIEW_SIGNATURES))      # the other two tables are what they were
    assert set(_native.VIEW_SIGNATURES) == {"mdl_heat_ws_bytes", "mdl_heat_render", "mdl_heat_render_marked"}
    assert not set(defines) & (set(_native._DEFINES) | set(_native.VIEW_DEFINES))
    assert _native.ABI_VERSION == 26 and lib.mdl_abi_version() == 26
    assert _build.STATS_HEADER in _build._deps() and _build.HEADER in _build._deps() and _build.VIEW_HEADER in _build._deps()


def test_a_header_that_repeats_a_name_is_refused():
    with open(_build.STATS_HEADER) as f:
        text = f.read()
    sigs, _ = _native._parse_header(text.replace("mdl_boot_weights(", "mdl_heat_render("))
    assert set(sigs) & set(_native.VIEW_SIGNATURES)      # what the import-time check of _native looks for


def test_the_python_surface_is_exported():
    import madeleine_amd
    from madeleine_amd import functional as F, resample
    for name in ("bootstrap_summary", "paired_difference", "linear_probe_ci", "survival_probe_ci"):
        assert name in madeleine_amd.__all__ and getattr(madeleine_amd, name) is getattr(resample, name)
    assert callable(F.boot_weights) and callable(F.boot_class_counts) and callable(F.boot_surv_counts)
    assert F.BOOT_SURV_MAX_TEST == 4096 and F.BOOT_REP_BLOCK == 8


def test_workspace_query():
    ws = _native.lib().mdl_boot_class_ws_bytes
    for Pn, S, C in ((90, 1153, 2), (1, 1, 2), (5, 16384, 8), (3, 97, 3)):
        ncls = 1 if C == 2 else C
        need = 8 * Pn * ncls * S + Pn * S + 8 * Pn + (8 * Pn * C * S if C > 2 else 0)
        assert need <= ws(Pn, S, C) <= need + 16 * 6 + 15 * Pn and ws(Pn, S, C) % 16 == 0
    assert ws(0, 5, 2) == ARG and ws(5, 0, 2) == ARG
    assert ws(5, 16385, 2) == UNSUP and ws(5, 10, 1) == UNSUP and ws(5, 10, 9) == UNSUP and ws(1 << 31, 10, 2) == UNSUP


# ---- refusals before any launch ------------------------------------------------------------------------------------------------------
def _weights(seed=1, G=2, R=3, S=10, null=None, misalign=None):
    ptr = {"group": FAKE, "w_out": FAKE}
    if null:
        ptr[null] = None
    if misalign:
        ptr[misalign[0]] += misalign[1]
    return _native.lib().mdl_boot_weights(seed, ptr["group"], G, R, S, ptr["w_out"], None)


def _class(Pn=3, n_max=4, S=10, C=3, ldy=0, R=5, null=None, misalign=None):
    ptr = {k: FAKE for k in ("z", "y", "train_idx", "n_train", "group", "confusion_out", "auc_num_out", "ws")}
    if null:
        ptr[null] = None
    if misalign:
        ptr[misalign[0]] += misalign[1]
    return _native.lib().mdl_boot_class_counts(ptr["z"], ptr["y"], ldy, ptr["train_idx"], ptr["n_train"], Pn, n_max, S, C, ptr["group"], 7, R,
                                               ptr["confusion_out"], ptr["auc_num_out"], ptr["ws"], None)


def _surv(Pn=3, n_max=4, S=10, ldt=0, lde=10, R=5, null=None, misalign=None):
    ptr = {k: FAKE for k in ("z", "time", "event", "train_idx", "n_train", "group", "counts_out")}
    if null:
        ptr[null] = None
    if misalign:
        ptr[misalign[0]] += misalign[1]
    return _native.lib().mdl_boot_surv_counts(ptr["z"], ptr["time"], ldt, ptr["event"], lde, ptr["train_idx"], ptr["n_train"], Pn, n_max, S,
                                              ptr["group"], 7, R, ptr["counts_out"], None)


@pytest.mark.parametrize("call,null", [(_weights, n) for n in ("group", "w_out")] +
                         [(_class, n) for n in ("z", "y", "train_idx", "n_train", "group", "confusion_out", "auc_num_out", "ws")] +
                         [(_surv, n) for n in ("z", "time", "event", "train_idx", "n_train", "group", "counts_out")])
def test_null_pointers_are_refused(call, null):
    assert call(null=null) == ARG


@pytest.mark.parametrize("call,kw,code", [
    (_weights, dict(G=0), ARG), (_weights, dict(S=0), ARG), (_weights, dict(R=-1), ARG),
    (_weights, dict(S=16385), UNSUP), (_weights, dict(R=(1 << 31) - 1), UNSUP), (_weights, dict(G=1 << 31), UNSUP),
    (_weights, dict(G=1 << 16, R=1 << 16), UNSUP),                                     # the grid G (R + 1)
    (_weights, dict(misalign=("group", 2)), ALIGN), (_weights, dict(misalign=("w_out", 1)), ALIGN),
    (_class, dict(Pn=0), ARG), (_class, dict(n_max=0), ARG), (_class, dict(S=0), ARG), (_class, dict(R=-1), ARG),
    (_class, dict(ldy=9), ARG), (_class, dict(ldy=-1), ARG),
    (_class, dict(S=16385), UNSUP), (_class, dict(n_max=16385), UNSUP), (_class, dict(C=1), UNSUP), (_class, dict(C=9), UNSUP),
    (_class, dict(R=(1 << 31) - 1), UNSUP), (_class, dict(Pn=1 << 31), UNSUP), (_class, dict(Pn=1 << 20, n_max=1 << 12), UNSUP),
    (_class, dict(Pn=1 << 24, C=8, S=16384), UNSUP),                                   # the grid P ncls ceil(S / 256)
    (_class, dict(Pn=1 << 20, R=(1 << 15) - 1), UNSUP),                                # the grid P ceil((R + 1) / 8)
    (_class, dict(misalign=("ws", 8)), ALIGN), (_class, dict(misalign=("auc_num_out", 4)), ALIGN), (_class, dict(misalign=("z", 2)), ALIGN),
    (_class, dict(misalign=("y", 2)), ALIGN), (_class, dict(misalign=("group", 1)), ALIGN), (_class, dict(misalign=("confusion_out", 2)), ALIGN),
    (_surv, dict(Pn=0), ARG), (_surv, dict(n_max=0), ARG), (_surv, dict(S=0), ARG), (_surv, dict(R=-1), ARG),
    (_surv, dict(ldt=9), ARG), (_surv, dict(lde=9), ARG),
    (_surv, dict(S=4097, lde=0), UNSUP), (_surv, dict(n_max=1025), UNSUP), (_surv, dict(R=(1 << 31) - 1), UNSUP),
    (_surv, dict(Pn=1 << 31), UNSUP), (_surv, dict(Pn=1 << 20, R=(1 << 15) - 1), UNSUP),
    (_surv, dict(misalign=("counts_out", 4)), ALIGN), (_surv, dict(misalign=("time", 2)), ALIGN), (_surv, dict(misalign=("event", 1)), ALIGN),
])
def test_refusals_before_any_launch(call, kw, code):
    assert call(**kw) == code


def test_the_order_of_the_refusals():
    """(1) MDL_E_ARG before (2) MDL_E_UNSUPPORTED before (3) MDL_E_ALIGN, as in P1-P3."""
    assert _weights(S=16385, R=-1) == ARG and _weights(S=16385, misalign=("w_out", 1)) == UNSUP
    assert _class(C=9, ldy=5) == ARG and _class(S=16385, ldy=5) == ARG
    assert _class(C=9, misalign=("ws", 8)) == UNSUP and _class(Pn=1 << 24, C=8, S=16384, misalign=("z", 2)) == UNSUP
    assert _surv(S=4097, lde=10) == ARG and _surv(S=4097, lde=0, misalign=("counts_out", 4)) == UNSUP


def test_wrapper_refusals_on_cpu_tensors():
    from madeleine_amd import functional as F
    with pytest.raises(RuntimeError, match="ROCm device"):
        F.boot_weights(0, torch.zeros(2, dtype=torch.int32), 3, 10)
    with pytest.raises(RuntimeError, match="ROCm device"):
        F.boot_class_counts(torch.zeros(1, 4, 1), torch.zeros(4, dtype=torch.int32), torch.zeros(1, 2, dtype=torch.int32),
                            torch.ones(1, dtype=torch.int32), 2, torch.zeros(1, dtype=torch.int32), 0, 3)
    with pytest.raises(RuntimeError, match="ROCm device"):
        F.boot_surv_counts(torch.zeros(1, 4), torch.zeros(4), torch.zeros(4, dtype=torch.int32), torch.zeros(1, 2, dtype=torch.int32),
                           torch.ones(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), 0, 3)


# ---- the weights of the host model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2 ** 63 + 5])
def test_weights_sum_to_the_cohort_and_are_dispersed_like_a_multinomial(seed):
    """Every replicate sums to S, replicate 0 is the sample, and the variance of the counts at S = 1100, R = 1000 lies within 1 % of 1
    (1 - 1/S = 0.9991 is expected; one round of mix32 per draw gives 0.992-0.993)."""
    w = M.weights(seed, 3, 1000, 1100)
    assert w.shape == (1001, 1100) and (w.sum(1) == 1100).all() and (w[0] == 1).all() and w.min() >= 0
    assert 0.99 <= float(w[1:].var()) <= 1.01, float(w[1:].var())
    assert abs(float(w[1:].mean()) - 1.0) < 1e-12


def test_weights_follow_the_formula_written_out():
    from tests._drop_ref import key, mix32
    seed, g, r, n = 2 ** 63 + 5, -3, 4, 65
    a = int(mix32(int(key(seed)) ^ (((g & 0xFFFFFFFF) * 0x9E3779B9) & 0xFFFFFFFF)))
    b = int(mix32((a + r) & 0xFFFFFFFF))
    counts = [0] * n
    for j in range(n):
        h = int(mix32((int(mix32(b ^ j)) + j * 0x9E3779B9) & 0xFFFFFFFF))
        counts[(h * n) >> 32] += 1
    assert M.weights(seed, g, r, n)[r].tolist() == counts and M.draws(seed, g, r, n).tolist() == [
        (int(mix32((int(mix32(b ^ j)) + j * 0x9E3779B9) & 0xFFFFFFFF)) * n) >> 32 for j in range(n)]


def test_groups_and_seeds_draw_independently():
    """Draw j of two groups, or of two seeds, agrees as often as two independent draws do: 1 / S within 20 % (1.1e6 draws: the standard
    deviation of the count is 3.2 %)."""
    n, reps = 1100, 1000
    base = np.stack([M.draws(0, 0, r, n) for r in range(1, reps + 1)])
    for seed, g in ((0, 1), (1, 0), (0, 2 ** 31 - 1)):
        other = np.stack([M.draws(seed, g, r, n) for r in range(1, reps + 1)])
        rate = float((base == other).mean()) * n
        assert 0.8 <= rate <= 1.2, (seed, g, rate)
    assert not np.array_equal(M.draws(0, 0, 1, n), M.draws(0, 0, 2, n))


def test_the_model_counts_a_case_by_hand():
    """Two positives and three negatives with a tie, weights by hand: the weighted Mann-Whitney numerator and the confusion matrix."""
    z = np.array([[[1.0], [0.0], [-0.0], [2.0], [1.0], [5.0]]], dtype=np.float32)
    y = np.array([1, 0, 1, 0, 0, 1])
    conf, num = M.class_counts(z, y, np.array([[5, -1]]), np.array([1]), 2, [0], 0, 0)
    # test cases 0 .. 4; positives {0: 1.0, 2: -0.0}, negatives {1: 0.0, 3: 2.0, 4: 1.0}: (0 > 1) 2 + (0 == 4) 1 + (2 == 1) 1 = 4
    assert num.tolist() == [[[4]]] and conf[0, 0].tolist() == [[1, 2], [1, 1]]
    assert M.auc_from_counts(conf, num)[0, 0] == 4 / (2.0 * 2 * 3)
    counts = M.surv_counts(np.array([[3.0, 1.0, 1.0, 0.0]], dtype=np.float32), [1.0, 2.0, 2.0, 3.0], [1, 1, 0, -1], np.array([[-1]]), [0], [0], 0, 0)
    # comparable: (0, 1), (0, 2), (1, 2: equal times, censored); case 3 has no follow-up.  points 2 + 2 + 1
    assert counts.tolist() == [[[5, 3]]] and M.c_index_from_counts(counts)[0, 0] == 5 / 6.0


# ---- host-side functions -------------------------------------------------------------------------------------------------------------
def test_bootstrap_summary_on_fixed_arrays():
    from madeleine_amd.resample import bootstrap_summary
    v = np.array([0.7, 0.5, 0.9, np.nan, 0.6, 0.8, np.inf])
    s = bootstrap_summary(v, level=0.5)
    assert s == {"point": 0.7, "lo": float(np.quantile([0.5, 0.9, 0.6, 0.8], 0.25)), "hi": float(np.quantile([0.5, 0.9, 0.6, 0.8], 0.75)),
                 "n_valid": 4}
    assert abs(s["lo"] - 0.575) < 1e-15 and abs(s["hi"] - 0.825) < 1e-15      # linear: 0.5 + 0.75 (0.6 - 0.5), 0.8 + 0.25 (0.9 - 0.8)
    assert M.summary(v, 0.5) == (0.7, s["lo"], s["hi"], 4)
    s = bootstrap_summary(np.array([[1.0, 2.0], [0.0, np.nan], [4.0, np.nan]]))
    assert s["point"].tolist() == [1.0, 2.0] and s["n_valid"].tolist() == [2, 0] and np.isnan(s["lo"][1]) and np.isnan(s["hi"][1])
    q = (1 - 0.95) / 2                                    # the probabilities as the functions form them
    assert s["lo"][0] == np.quantile([0.0, 4.0], q) and s["hi"][0] == np.quantile([0.0, 4.0], 1 - q)
    empty = bootstrap_summary([0.3])
    assert empty["point"] == 0.3 and empty["n_valid"] == 0 and np.isnan(empty["lo"])
    for bad in (0.0, 1.0, 1.5):
        with pytest.raises(ValueError):
            bootstrap_summary(v, level=bad)


def test_the_paired_p_value_on_fixed_arrays():
    from madeleine_amd.resample import paired_difference
    a = np.array([0.8, 0.7, 0.9, 0.8, 0.6, np.nan])
    b = np.array([0.6, 0.6, 0.6, 0.8, 0.7, 0.5])
    d = paired_difference(a, b)                          # d* = 0.1, 0.3, 0, -0.1, NaN: n = 4, #{<= 0} = 2, #{>= 0} = 3
    assert d["n_valid"] == 4 and abs(d["diff"] - 0.2) < 1e-15 and d["p"] == min(1.0, 2 * min(3 / 5, 4 / 5)) == 1.0
    assert d["p"] == M.p_value((a - b)[1:])
    up = paired_difference(np.full(20, 0.9), np.full(20, 0.5))
    assert up["p"] == 2 * (0 + 1) / (19 + 1) and up["lo"] == up["hi"] == up["diff"] == 0.4
    same = paired_difference(a[:5], a[:5])
    assert same["diff"] == 0 and same["lo"] == 0 and same["hi"] == 0 and same["p"] == 1.0
    none = paired_difference([0.5, np.nan], [0.4, 0.1])
    assert none["n_valid"] == 0 and none["p"] == 1.0


def test_the_metrics_from_counts():
    from madeleine_amd.resample import auc_from_counts, c_index_from_counts
    conf = np.array([[[3, 1], [0, 2]], [[4, 0], [0, 0]]])
    num = np.array([[10], [0]])
    assert auc_from_counts(conf, num).tolist()[0] == 10 / (2.0 * 2 * 4) and np.isnan(auc_from_counts(conf, num)[1])
    assert np.isnan(auc_from_counts(conf[:1], np.array([[-1]]))[0])
    conf3 = np.array([[2, 0, 0], [0, 1, 1], [1, 0, 1]])
    got = auc_from_counts(conf3, np.array([12, 8, 6]))
    assert got == (12 / (2.0 * 2 * 4) + 8 / (2.0 * 2 * 4) + 6 / (2.0 * 2 * 4)) / 3 and got == M.auc_from_counts(conf3, np.array([12, 8, 6]))
    assert c_index_from_counts(np.array([[5, 3], [0, 0]])).tolist()[0] == 5 / 6.0 and np.isnan(c_index_from_counts(np.array([[5, 3], [0, 0]]))[1])


def test_the_bootstrap_options_of_the_command_line():
    from madeleine_amd import probe
    base = ["--slide_embedding_pkl", "a.pkl", "--label_path", "l.csv"]
    plain = probe._parse(base)
    assert (plain.bootstrap, plain.versus, plain.level, plain.seed) == (0, None, 0.95, 0)
    args = probe._parse(base + ["--bootstrap", "1000", "--versus", "mean.pkl", "--level", "0.9", "--seed", "7", "--cv_folds", "5"])
    assert (args.bootstrap, args.versus, args.level, args.seed, args.cv_folds) == (1000, "mean.pkl", 0.9, 7, 5)
    for bad in (["--versus", "mean.pkl"], ["--seed", "3"], ["--level", "0.9"], ["--bootstrap", "-1"], ["--bootstrap", "10", "--level", "1.0"]):
        with pytest.raises(SystemExit):
            probe._parse(base + bad)
    res = {("er", 10): {"arms": {"embeds": {"auc": {"point": 0.81234, "lo": 0.7004, "hi": 0.9, "n_valid": 99}}, "mean": {"auc": {}}},
                        "pairs": {("embeds", "mean"): {"auc": {"diff": 0.1, "lo": 0.01, "hi": 0.2, "p": 0.0198}}}}}
    assert probe._bootstrap_lines(res, "k", 0.9) == [
        "k=10, task=er, bootstrap auc 90% interval=[0.7, 0.9] (point 0.812, 99 valid replicates), difference to mean=0.1 [0.01, 0.2], p=0.0198"]
    del res[("er", 10)]["arms"]["mean"]
    assert probe._bootstrap_lines(res, "k", 0.95) == ["k=10, task=er, bootstrap auc 95% interval=[0.7, 0.9] (point 0.812, 99 valid replicates)"]


def test_cli_bootstrap_adds_lines_and_aligns_the_second_pickle(tmp_path, monkeypatch, capsys):
    """--bootstrap prints the usual lines and pickles first, then one line per (task, k); --versus is matched by slide id."""
    import csv
    import pickle
    from madeleine_amd import probe, resample
    ids = ["s%d" % i for i in range(6)]
    embeds = np.arange(24, dtype=np.float32).reshape(6, 4)
    pkl, other = tmp_path / "enc.pkl", tmp_path / "mean.pkl"
    with open(pkl, "wb") as f:
        pickle.dump({"embeds": embeds, "slide_ids": ids}, f)
    with open(other, "wb") as f:                        # the same slides in reverse order, and one more
        pickle.dump({"embeds": np.concatenate([100 + embeds[::-1], np.zeros((1, 4), np.float32)]), "slide_ids": ids[::-1] + ["s7"]}, f)
    with open(tmp_path / "labels.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["slide_id", "er"])
        for i in (5, 0, 2, 3):
            w.writerow(["s%d" % i, i % 2])
    seen = {}

    def fake(e, labels, **kw):
        return {("er", k): {"auc": np.array([0.5, 0.75]), "bacc": np.array([0.25, 0.5]), "converged": np.array([True, True]),
                            "confusion": np.zeros((2, 2, 2), dtype=np.int64)} for k in (1, 10)}

    def fake_ci(arms, labels, **kw):
        seen.update(arms=arms, labels=labels, kw=kw)
        s = {"point": 0.7, "lo": 0.6, "hi": 0.8, "n_valid": 5}
        return {("er", k): {"arms": {a: {"auc": s} for a in arms},
                            "pairs": {tuple(arms): {"auc": {"diff": 0.1, "lo": -0.05, "hi": 0.2, "p": 0.3333, "n_valid": 5}}}} for k in (1, 10)}

    monkeypatch.setattr(probe, "linear_probe", fake)
    monkeypatch.setattr(resample, "linear_probe_ci", fake_ci)
    base = ["--slide_embedding_pkl", str(pkl), "--label_path", str(tmp_path / "labels.csv"), "--tasks", "er"]
    probe._main(base)
    plain = capsys.readouterr().out
    assert plain.splitlines() == ["k=%d, task=er, auc=0.625 +/- 0.125" % k for k in (1, 10)] and not seen
    probe._main(base + ["--bootstrap", "5", "--versus", str(other), "--level", "0.9", "--seed", "3"])
    out = capsys.readouterr().out
    assert out.startswith(plain) and out[len(plain):].splitlines() == [
        "k=%d, task=er, bootstrap auc 90%% interval=[0.6, 0.8] (point 0.7, 5 valid replicates), difference to mean=0.1 [-0.05, 0.2], p=0.3333"
        % k for k in (1, 10)]
    assert list(seen["arms"]) == ["embeds", "mean"] and seen["kw"] == {"replicates": 5, "level": 0.9, "seed": 3, "kappa": False}
    assert np.array_equal(seen["arms"]["embeds"], embeds[[0, 2, 3, 5]]) and np.array_equal(seen["arms"]["mean"], 100 + embeds[[0, 2, 3, 5]])
    with open(other, "wb") as f:
        pickle.dump({"embeds": embeds[:3], "slide_ids": ids[:3]}, f)
    with pytest.raises(SystemExit, match="absent"):
        probe._main(base + ["--bootstrap", "5", "--versus", str(other)])
