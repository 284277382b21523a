"""The test-set bootstrap on the GPU (B1-B3, include/madeleine_amd_stats.h): mdl_boot_weights, mdl_boot_class_counts and
mdl_boot_surv_counts against the numpy model of tests/_resample_ref.py BIT FOR BIT, replicate 0 against the metrics kernels of the
probes, the independence of a problem's bits from its neighbours, n_max and R, the stated buffer extents in the guarded arena of
tests/_arena.py, and linear_probe_ci / survival_probe_ci against np.quantile over the model's replicate values.

Shapes: S = 97 cases, 5 problems, 33 replicates for the counts (odd, no multiple of anything, several replicate blocks of 8); the sizes
at which the class kernel takes another path on top: one position per thread against two (256 / 257 test cases), the default dynamic
LDS limit against the raised one (S = 12287 / 12288 / 12289), and the largest cohort (16384).  Scores are small integers, so that ties
are everywhere; for C > 2 the rows come from a pool in which two different rows never have nearly equal log-softmax scores, so that no
tie hangs on the last bit of exp and log."""
import numpy as np
import pytest
import torch

from madeleine_amd import _native
from madeleine_amd import functional as F
from tests import _resample_ref as M
from tests._arena import FILLS, Arena

pytestmark = pytest.mark.gpu

S, P, R, N_MAX = 97, 5, 33, 12
SEED = 0x9E3779B97F4A7C15            # above 2^63
N_TRAIN = (1, 5, 12, 7, 3)
GROUP = (0, 0, 1, 2, 1)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _t(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(dev)


# ======================================================================================================================== weights
@pytest.mark.parametrize("n_cases", [1, 2, 63, 64, 65, 1153, 16384])
def test_boot_weights_equal_the_host_model(dev, n_cases):
    for seed, groups in ((0, (0, 1)), (SEED, (7, -3)), (2 ** 64 - 1, (2 ** 31 - 1,))):
        w = F.boot_weights(seed, torch.tensor(groups, dtype=torch.int32, device=dev), 7, n_cases).cpu().numpy()
        assert w.shape == (len(groups), 8, n_cases) and w.dtype == np.uint16
        for i, g in enumerate(groups):
            ref = M.weights(seed, g, 7, n_cases)
            assert np.array_equal(w[i].astype(np.int64), ref), (seed, g)
            assert (ref.sum(1) == n_cases).all() and (ref[0] == 1).all()


# ================================================================================================================= classification
def _pool(C, rng, size=14):
    """`size` integer rows [C] in -2 .. 2 whose log-softmax scores differ, class by class, by more than 1e-9 between any two rows."""
    rows, scores = [], []
    while len(rows) < size:
        cand = rng.integers(-2, 3, C).astype(np.float32)
        sc = M.predict(cand[None], C)[1][0]
        if all(np.abs(sc - s).min() > 1e-9 for s in scores):
            rows.append(cand)
            scores.append(sc)
    return np.stack(rows)


def class_case(C, per_problem_y, seed=5):
    """z float32 [P, S, cols], y [S] or [P, S], train_idx [P, N_MAX] (-1 padded), n_train, group: tie-heavy integer scores with both
    zeros, unlabeled cases, training lists of different lengths, and class C - 1 with two cases only (never trained on)."""
    rng = np.random.default_rng(seed + C)
    cols = 1 if C == 2 else C
    if C == 2:
        z = rng.integers(-2, 3, (P, S, 1)).astype(np.float32)
    else:
        z = _pool(C, rng)[rng.integers(0, 14, (P, S))]
    z = np.where((z == 0) & (rng.random(z.shape) < 0.5), np.float32(-0.0), z).astype(np.float32)
    y = rng.integers(0, C - 1, S)
    y[rng.choice(S, 10, replace=False)] = -1
    rare = rng.choice(np.nonzero(y >= 0)[0], 2, replace=False)
    y[rare] = C - 1
    ys = np.stack([y] * P)
    if per_problem_y:
        for p in range(1, P):
            move = rng.choice(np.setdiff1d(np.arange(S), rare), 6, replace=False)
            ys[p, move] = rng.integers(-1, C - 1, 6)
    table = np.full((P, N_MAX), -1, dtype=np.int32)
    for p in range(P):
        table[p, :N_TRAIN[p]] = rng.choice(np.nonzero((ys[p] >= 0) & (ys[p] < C - 1))[0], N_TRAIN[p], replace=False)
    return dict(C=C, cols=cols, z=z, y=ys if per_problem_y else y, table=table, n_train=np.array(N_TRAIN, dtype=np.int32),
                group=np.array(GROUP, dtype=np.int32))


def device_counts(dev, c, seed=SEED, replicates=R, rows=slice(None), table=None):
    y = c["y"] if c["y"].ndim == 1 else c["y"][rows]
    table = c["table"] if table is None else table
    conf, num = F.boot_class_counts(_t(c["z"][rows], dev), _t(y, dev, torch.int32), _t(table[rows], dev), _t(c["n_train"][rows], dev),
                                    c["C"], _t(c["group"][rows], dev), seed, replicates)
    return conf.cpu().numpy().astype(np.int64), num.cpu().numpy()


_MODEL = {}


def model_counts(C, per_problem_y):
    """The case and the model's counts, computed once and shared (read-only)."""
    key = (C, per_problem_y)
    if key not in _MODEL:
        c = class_case(C, per_problem_y)
        conf, num = M.class_counts(c["z"], c["y"], c["table"], c["n_train"], C, c["group"], SEED, R)
        conf.setflags(write=False)
        num.setflags(write=False)
        _MODEL[key] = (c, conf, num)
    return _MODEL[key]


@pytest.mark.parametrize("per_problem_y", [False, True], ids=["ldy0", "ldyS"])
@pytest.mark.parametrize("C", [2, 3, 8])
def test_class_counts_equal_the_host_model(dev, C, per_problem_y):
    c, conf_ref, num_ref = model_counts(C, per_problem_y)
    auc = M.auc_from_counts(conf_ref, num_ref)
    lost = np.isnan(auc[0, 1:])
    assert lost.any() and not lost.all(), "the rare class must be lost by some replicates of problem 0 and kept by others"
    conf, num = device_counts(dev, c)
    assert num.dtype == np.int64 and conf.shape == (P, R + 1, C, C) and num.shape == (P, R + 1, c["cols"])
    assert np.array_equal(conf, conf_ref)
    assert np.array_equal(num, num_ref)


@pytest.mark.parametrize("C", [2, 3, 8])
def test_replicate_zero_is_the_metrics_kernel(dev, C):
    """Confusion exactly; AUC: num / (2 pos neg) in double, macro-averaged, rounded to fp32, within one fp32 ulp of auc_out."""
    c, _, _ = model_counts(C, True)
    conf, num = device_counts(dev, c, replicates=0)
    assert conf.shape == (P, 1, C, C)
    args = (_t(c["z"], dev), _t(c["y"], dev, torch.int32), _t(c["table"], dev), _t(c["n_train"], dev), C)
    for metrics in (F.probe_metrics, F.logit_metrics):
        cm, auc = metrics(*args)
        assert np.array_equal(cm.cpu().numpy().astype(np.int64), conf[:, 0])
        auc = auc.cpu().numpy()
        mine = M.auc_from_counts(conf[:, 0], num[:, 0]).astype(np.float32)
        assert np.array_equal(np.isnan(auc), np.isnan(mine))
        ok = ~np.isnan(auc)
        assert ok.any() and (np.abs(auc[ok] - mine[ok]) <= np.spacing(np.abs(mine[ok]))).all(), (auc, mine)


@pytest.mark.parametrize("C", [2, 3])
def test_a_nan_score_marks_its_problem_alone(dev, C):
    c, conf_ref, num_ref = model_counts(C, False)
    bad = dict(c, z=c["z"].copy())
    victim = int(np.nonzero(M.test_mask(c["y"], c["table"][2], c["n_train"][2], C))[0][3])
    bad["z"][2, victim, c["cols"] - 1] = np.nan
    conf_m, num_m = M.class_counts(bad["z"], bad["y"], bad["table"], bad["n_train"], C, bad["group"], SEED, R)
    assert (num_m[2] == -1).all()
    conf, num = device_counts(dev, bad)
    assert (num[2] == -1).all() and np.array_equal(conf, conf_m)
    others = [0, 1, 3, 4]
    assert np.array_equal(num[others], num_ref[others]) and np.array_equal(conf[others], conf_ref[others])


@pytest.mark.parametrize("n_cases,replicates", [(1, 3), (2, 3), (266, 9), (267, 9), (12287, 2), (12288, 2), (12289, 2), (16384, 2)])
def test_class_counts_at_the_size_edges(dev, n_cases, replicates):
    """One problem.  266 / 267 cases with 10 training cases: 256 / 257 test cases, one against two positions per thread; 12288: the first
    size whose dynamic LDS exceeds the default limit (MDL_BOOT_LDS_RAISE_FROM); 16384: MDL_PROBE_MAX_CASES."""
    assert _native.STATS_DEFINES["MDL_BOOT_LDS_RAISE_FROM"] == 12288 and _native._DEFINES["MDL_PROBE_MAX_CASES"] == 16384
    rng = np.random.default_rng(n_cases)
    z = rng.integers(-40, 41, (1, n_cases, 1)).astype(np.float32)
    y = rng.integers(0, 2, n_cases)
    n_train = min(10, n_cases - 1)
    table = np.full((1, 10), -1, dtype=np.int32)
    table[0, :n_train] = np.arange(n_train)
    c = dict(C=2, z=z, y=y, table=table, n_train=np.array([n_train], dtype=np.int32), group=np.array([3], dtype=np.int32))
    assert n_cases not in (266, 267) or int(M.test_mask(y, table[0], n_train, 2).sum()) == n_cases - 10
    conf_ref, num_ref = M.class_counts(z, y, table, c["n_train"], 2, c["group"], 11, replicates)
    conf, num = device_counts(dev, c, seed=11, replicates=replicates)
    assert np.array_equal(conf, conf_ref) and np.array_equal(num, num_ref)


def test_a_problem_does_not_depend_on_its_neighbours_n_max_or_the_replicate_count(dev):
    for C in (2, 3):
        c, conf_ref, num_ref = model_counts(C, True)
        conf, num = device_counts(dev, c, rows=slice(3, 4))                       # alone
        assert np.array_equal(conf[0], conf_ref[3]) and np.array_equal(num[0], num_ref[3])
        wide = np.full((P, 20), -1, dtype=np.int32)                               # at another n_max
        wide[:, :N_MAX] = c["table"]
        conf, num = device_counts(dev, c, table=wide)
        assert np.array_equal(conf, conf_ref) and np.array_equal(num, num_ref)
        for replicates in (5, 50):                                                # the first six rows at another R
            conf, num = device_counts(dev, c, replicates=replicates)
            assert np.array_equal(conf[:, :6], conf_ref[:, :6]) and np.array_equal(num[:, :6], num_ref[:, :6])


def test_problems_of_one_group_share_their_weights(dev):
    """Equal test sets and groups, different scores: the weight of every true class (the confusion row sums) is the same in every
    replicate; under another group it is not."""
    c, _, _ = model_counts(2, False)
    z = np.stack([c["z"][0], c["z"][1], c["z"][0]])
    two = dict(C=2, z=z, y=c["y"], table=np.stack([c["table"][1]] * 3), n_train=np.array([N_TRAIN[1]] * 3, dtype=np.int32),
               group=np.array([4, 4, 5], dtype=np.int32))
    conf, _ = device_counts(dev, two)
    assert not np.array_equal(conf[0], conf[1])
    assert np.array_equal(conf[0].sum(-1), conf[1].sum(-1))
    assert not np.array_equal(conf[0, 1:].sum(-1), conf[2, 1:].sum(-1)) and np.array_equal(conf[0, 0], conf[2, 0])


# ======================================================================================================================= survival
SURV_S, SURV_P = 61, 4


def surv_case(per_problem, seed=9):
    rng = np.random.default_rng(seed)
    z = rng.integers(-3, 4, (SURV_P, SURV_S)).astype(np.float32)
    z = np.where((z == 0) & (rng.random(z.shape) < 0.5), np.float32(-0.0), z).astype(np.float32)
    time = rng.integers(1, 9, SURV_S).astype(np.float32)
    event = rng.choice([1, 1, 0, 0, -1], SURV_S)
    times, events = np.stack([time] * SURV_P), np.stack([event] * SURV_P)
    if per_problem:
        for p in range(1, SURV_P):
            times[p] = rng.permutation(time)
            events[p] = rng.permutation(event)
    n_train = np.array([0, 5, 9, 0], dtype=np.int32)
    table = np.full((SURV_P, 9), -1, dtype=np.int32)
    for p in range(SURV_P):
        table[p, :n_train[p]] = rng.choice(np.nonzero(events[p] >= 0)[0], n_train[p], replace=False)
    return dict(z=z, time=times if per_problem else time, event=events if per_problem else event, table=table, n_train=n_train,
                group=np.array([0, 1, 1, 0], dtype=np.int32))


def device_surv(dev, c, seed=SEED, replicates=R):
    return F.boot_surv_counts(_t(c["z"], dev), _t(c["time"], dev), _t(c["event"], dev, torch.int32), _t(c["table"], dev),
                              _t(c["n_train"], dev), _t(c["group"], dev), seed, replicates).cpu().numpy()


@pytest.mark.parametrize("per_problem", [False, True], ids=["shared", "per_problem"])
def test_surv_counts_equal_the_host_model_and_replicate_zero_the_metrics_kernel(dev, per_problem):
    c = surv_case(per_problem)
    ref = M.surv_counts(c["z"], c["time"], c["event"], c["table"], c["n_train"], c["group"], SEED, R)
    assert (ref[:, :, 1] > 0).all() and len({tuple(r) for r in ref[0, :, 1:].tolist()}) > 1
    got = device_surv(dev, c)
    assert got.dtype == np.int64 and np.array_equal(got, ref)
    _, _, counts = F.survival_metrics(_t(c["z"], dev), _t(c["time"], dev), _t(c["event"], dev, torch.int32), _t(c["table"], dev),
                                      _t(c["n_train"], dev), torch.zeros(SURV_P, device=dev))
    assert np.array_equal(counts[:, :2].cpu().numpy().astype(np.int64), got[:, 0])
    assert np.array_equal(device_surv(dev, c, replicates=0), ref[:, :1])


def test_surv_counts_at_the_cap_and_past_it(dev):
    cap = _native.STATS_DEFINES["MDL_BOOT_SURV_MAX_TEST"]
    rng = np.random.default_rng(2)
    c = dict(z=rng.integers(-5, 6, (1, cap)).astype(np.float32), time=rng.integers(1, 40, cap).astype(np.float32),
             event=rng.choice([1, 0, 0, -1], cap), table=np.arange(7, dtype=np.int32)[None], n_train=np.array([7], dtype=np.int32),
             group=np.array([1], dtype=np.int32))
    ref = M.surv_counts(c["z"], c["time"], c["event"], c["table"], c["n_train"], c["group"], 3, 1)
    assert np.array_equal(device_surv(dev, c, seed=3, replicates=1), ref)
    big = dict(c, z=np.zeros((1, cap + 1), dtype=np.float32), time=np.ones(cap + 1, dtype=np.float32), event=np.ones(cap + 1, dtype=np.int64))
    with pytest.raises(NotImplementedError, match="bootstrap counts support"):
        device_surv(dev, big, replicates=1)


# ================================================================================================================== guarded arena
@pytest.mark.parametrize("fill", FILLS)
def test_every_buffer_at_the_headers_size_in_the_guarded_arena(dev, fill):
    lib = _native.lib()
    stream = torch.cuda.current_stream().cuda_stream
    c, conf_ref, num_ref = model_counts(3, True)
    sc = surv_case(True)
    sref = M.surv_counts(sc["z"], sc["time"], sc["event"], sc["table"], sc["n_train"], sc["group"], SEED, R)
    C, cols = 3, 3
    ws_bytes = lib.mdl_boot_class_ws_bytes(P, S, C)
    assert ws_bytes > 0
    bufs = [("w_group", (2,), torch.int32, "in"), ("w_out", (2, R + 1, S), torch.uint16, "out"),
            ("z", (P, S, cols), torch.float32, "in"), ("y", (P, S), torch.int32, "in"), ("table", (P, N_MAX), torch.int32, "in"),
            ("n_train", (P,), torch.int32, "in"), ("group", (P,), torch.int32, "in"), ("conf", (P, R + 1, C, C), torch.int32, "out"),
            ("num", (P, R + 1, cols), torch.int64, "out"), ("ws", (ws_bytes,), torch.uint8, "ws"),
            ("s_z", (SURV_P, SURV_S), torch.float32, "in"), ("s_time", (SURV_P, SURV_S), torch.float32, "in"),
            ("s_event", (SURV_P, SURV_S), torch.int32, "in"), ("s_table", (SURV_P, 9), torch.int32, "in"),
            ("s_n", (SURV_P,), torch.int32, "in"), ("s_group", (SURV_P,), torch.int32, "in"),
            ("s_counts", (SURV_P, R + 1, 2), torch.int64, "out")]
    a = Arena(dev, fill)
    for name, shape, dtype, role in bufs:
        a.reserve(name, shape, dtype, role)
    a.allocate()
    for name, shape, dtype, role in bufs:
        a.take(name, shape, dtype, role)
    a["w_group"].copy_(torch.tensor([5, 6], dtype=torch.int32))
    for name, src in (("z", c["z"]), ("y", c["y"]), ("table", c["table"]), ("n_train", c["n_train"]), ("group", c["group"]),
                      ("s_z", sc["z"]), ("s_time", sc["time"]), ("s_event", sc["event"]), ("s_table", sc["table"]),
                      ("s_n", sc["n_train"]), ("s_group", sc["group"])):
        a[name].copy_(torch.from_numpy(np.ascontiguousarray(src)).to(a[name].dtype))
    a.seal()
    F._call("mdl_boot_weights", SEED, a["w_group"], 2, R, S, a["w_out"], stream)
    F._call("mdl_boot_class_counts", a["z"], a["y"], S, a["table"], a["n_train"], P, N_MAX, S, C, a["group"], SEED, R, a["conf"], a["num"],
            a["ws"], stream)
    F._call("mdl_boot_surv_counts", a["s_z"], a["s_time"], SURV_S, a["s_event"], SURV_S, a["s_table"], a["s_n"], SURV_P, 9, SURV_S,
            a["s_group"], SEED, R, a["s_counts"], stream)
    torch.cuda.synchronize()
    a.check()
    assert np.array_equal(a["w_out"].cpu().numpy()[1].astype(np.int64), M.weights(SEED, 6, R, S))
    assert np.array_equal(a["conf"].cpu().numpy(), conf_ref) and np.array_equal(a["num"].cpu().numpy(), num_ref)
    assert np.array_equal(a["s_counts"].cpu().numpy(), sref)


# ============================================================================================================= the probes' intervals
CI_S, CI_D, CI_FOLDS, CI_R, CI_SEED = 120, 16, 3, 64, 17


def ci_cohort():
    """Two binary tasks carried by the first two columns of arm "signal"; arm "noise" knows nothing.  numpy seed 4."""
    rng = np.random.default_rng(4)
    labels = {"a": rng.integers(0, 2, CI_S), "b": rng.integers(0, 2, CI_S)}
    labels["b"][rng.choice(CI_S, 8, replace=False)] = -1
    X = rng.standard_normal((CI_S, CI_D)).astype(np.float32)
    X[:, 0] += 3.0 * (2 * labels["a"] - 1)
    X[:, 1] += 3.0 * (2 * np.maximum(labels["b"], 0) - 1)
    return X, rng.standard_normal((CI_S, CI_D)).astype(np.float32), labels


def model_probe_replicates(dev, X, labels, k, seed):
    """{task: {"auc": [R + 1], "bacc": [R + 1]}} from the model's counts of the device's own decision values."""
    from madeleine_amd import probe
    out = {}
    Xd = _t(X, dev)
    for g, (task, y) in enumerate(labels.items()):
        lists = [probe.probe_splits(y, k, fold, 0) for fold in range(CI_FOLDS)]
        table, n_train = probe._problem_table(lists, dev)
        yd = _t(np.stack([y] * CI_FOLDS), dev, torch.int32)
        W, b, _ = F.probe_fit(Xd, yd, table, n_train, 2)
        z = F.probe_scores(Xd, W, b, 2).cpu().numpy()
        conf, num = M.class_counts(z, y, table.cpu().numpy(), n_train.cpu().numpy(), 2, [g] * CI_FOLDS, seed, CI_R)
        bacc = np.array([[probe.balanced_accuracy(conf[f, r]) for r in range(CI_R + 1)] for f in range(CI_FOLDS)])
        out[task] = {"auc": M.auc_from_counts(conf, num).mean(0), "bacc": bacc.mean(0)}
    return out


def test_linear_probe_ci(dev):
    from madeleine_amd import linear_probe_ci
    X, noise, labels = ci_cohort()
    kw = dict(ks=(2,), folds=CI_FOLDS, replicates=CI_R, seed=CI_SEED)
    res = linear_probe_ci({"signal": X, "twin": X.copy(), "noise": noise}, labels, **kw)
    assert set(res) == {("a", 2), ("b", 2)}
    ref = {arm: model_probe_replicates(dev, E, labels, 2, CI_SEED) for arm, E in (("signal", X), ("noise", noise))}
    for task in labels:
        r = res[(task, 2)]
        assert list(r["arms"]) == ["signal", "twin", "noise"] and list(r["pairs"]) == [("signal", "twin"), ("signal", "noise"), ("twin", "noise")]
        for arm in ("signal", "noise"):
            for metric in ("auc", "bacc"):
                got, values = r["arms"][arm][metric], ref[arm][task][metric]
                assert np.array_equal(r["arms"][arm]["replicates"][metric], values, equal_nan=True)
                point, lo, hi, n_valid = M.summary(values)
                assert (got["point"], got["lo"], got["hi"], got["n_valid"]) == (point, lo, hi, n_valid)
                assert (got["lo"] <= got["point"] <= got["hi"]) == (lo <= point <= hi)
        for metric in ("auc", "bacc"):
            twin = r["pairs"][("signal", "twin")][metric]               # an identical arm: no difference in any replicate
            assert twin["diff"] == 0 and twin["lo"] == 0 and twin["hi"] == 0 and twin["p"] == 1.0
            assert np.array_equal(r["arms"]["signal"]["replicates"][metric], r["arms"]["twin"]["replicates"][metric], equal_nan=True)
        d = ref["signal"][task]["auc"] - ref["noise"][task]["auc"]      # a noise arm: the interval of the difference excludes 0
        point, lo, hi, n_valid = M.summary(d)
        assert n_valid > 0 and lo > 0, "the fixture (numpy seed 4, bootstrap seed %d) must separate the arms in the model: %r" % (CI_SEED, (lo, hi))
        got = r["pairs"][("signal", "noise")]["auc"]
        assert (got["diff"], got["lo"], got["hi"], got["n_valid"]) == (point, lo, hi, n_valid) and got["p"] == M.p_value(d[1:])
        assert got["lo"] > 0 and got["p"] <= 2.0 / (n_valid + 1)
    again = linear_probe_ci({"signal": X}, labels, **kw)
    other = linear_probe_ci({"signal": X}, labels, **dict(kw, seed=CI_SEED + 1))
    for task in labels:
        mine = res[(task, 2)]["arms"]["signal"]["replicates"]["auc"]
        assert np.array_equal(again[(task, 2)]["arms"]["signal"]["replicates"]["auc"], mine, equal_nan=True)
        theirs = other[(task, 2)]["arms"]["signal"]["replicates"]["bacc"]
        assert theirs[0] == res[(task, 2)]["arms"]["signal"]["replicates"]["bacc"][0]
        assert not np.array_equal(theirs[1:], res[(task, 2)]["arms"]["signal"]["replicates"]["bacc"][1:], equal_nan=True)


def test_linear_probe_ci_cross_validated(dev):
    """The cv protocol: the problems of linear_probe_cv, and a point value that is linear_probe_cv's own mean over the folds."""
    from madeleine_amd import linear_probe_ci, linear_probe_cv
    X, _, labels = ci_cohort()
    res = linear_probe_ci(X, labels, protocol="cv", folds=CI_FOLDS, replicates=8, seed=CI_SEED, kappa=True)
    plain = linear_probe_cv(X, labels, folds=CI_FOLDS, kappa=True)
    for task in labels:
        arm = res[(task, 0)]["arms"]["embeds"]
        assert abs(arm["auc"]["point"] - plain[(task, 0)]["auc"].mean()) <= 1e-6
        assert arm["bacc"]["point"] == plain[(task, 0)]["bacc"].mean() and arm["converged"].all()
        assert arm["q_kappa"]["point"] == plain[(task, 0)]["q_kappa"].mean() and arm["replicates"]["q_kappa"].shape == (9,)
        assert res[(task, 0)]["pairs"] == {}


def test_survival_probe_ci(dev):
    from madeleine_amd import survival, survival_probe, survival_probe_ci
    rng = np.random.default_rng(6)
    n, folds = 90, 3
    X = rng.standard_normal((n, 8)).astype(np.float32)
    time = np.ceil(np.exp(1.5 - 1.2 * X[:, 0] + 0.3 * rng.standard_normal(n)) * 4).astype(np.float32)      # tied, risk in column 0
    event = rng.choice([1, 1, 1, 0, -1], n)
    noise = rng.standard_normal((n, 8)).astype(np.float32)
    kw = dict(folds=folds, replicates=CI_R, seed=CI_SEED)
    res = survival_probe_ci({"signal": X, "twin": X.copy(), "noise": noise}, time, event, **kw)[("survival", 0)]
    ref = {}
    for arm, E in (("signal", X), ("noise", noise)):
        Xd = _t(E, dev)
        lists = survival.survival_splits(event, folds, 0, 0)
        table, n_train = survival._problem_table(lists, dev)
        t_dev, e_dev = _t(np.stack([time] * folds), dev), _t(np.stack([event] * folds), dev, torch.int32)
        W, _, _ = F.cox_fit(Xd, t_dev, e_dev, table, n_train, 1.0, survival.GTOL, 100)
        z = F.probe_scores(Xd, W.unsqueeze(1), torch.zeros(folds, 1, device=dev), 2).squeeze(2).cpu().numpy()
        counts = M.surv_counts(z, time, event, table.cpu().numpy(), n_train.cpu().numpy(), [0] * folds, CI_SEED, CI_R)
        ref[arm] = M.c_index_from_counts(counts).mean(0)
        got = res["arms"][arm]
        assert np.array_equal(got["replicates"]["c_index"], ref[arm], equal_nan=True)
        point, lo, hi, n_valid = M.summary(ref[arm])
        assert (got["c_index"]["point"], got["c_index"]["lo"], got["c_index"]["hi"], got["c_index"]["n_valid"]) == (point, lo, hi, n_valid)
        assert (got["c_index"]["lo"] <= point <= got["c_index"]["hi"]) == (lo <= point <= hi)
    assert res["arms"]["signal"]["c_index"]["point"] == survival_probe(X, time, event, folds=folds)[("survival", 0)]["c_index"].mean()
    twin = res["pairs"][("signal", "twin")]["c_index"]
    assert twin["diff"] == 0 and twin["lo"] == 0 and twin["hi"] == 0 and twin["p"] == 1.0
    d = ref["signal"] - ref["noise"]
    point, lo, hi, n_valid = M.summary(d)
    assert lo > 0, "the fixture (numpy seed 6, bootstrap seed %d) must separate the arms in the model: %r" % (CI_SEED, (lo, hi))
    got = res["pairs"][("signal", "noise")]["c_index"]
    assert (got["diff"], got["lo"], got["hi"], got["n_valid"], got["p"]) == (point, lo, hi, n_valid, M.p_value(d[1:]))
    again = survival_probe_ci({"signal": X}, time, event, **kw)[("survival", 0)]["arms"]["signal"]["replicates"]["c_index"]
    other = survival_probe_ci({"signal": X}, time, event, **dict(kw, seed=CI_SEED + 1))[("survival", 0)]["arms"]["signal"]["replicates"]["c_index"]
    assert np.array_equal(again, ref["signal"], equal_nan=True) and other[0] == ref["signal"][0] and not np.array_equal(other[1:], ref["signal"][1:])
