"""Host side of the survival probe, no GPU: the entry points and their argument validation (every refusal returns before a launch), the
event-stratified split rule, the fp64 reference of tests/_survival_ref.py against a partial likelihood worked by hand, and the
properties the closed-form cohorts of the GPU tests must have."""
import math

import numpy as np
import pytest
import torch

from tests import _survival_ref as R

ENTRY_POINTS = ["mdl_cox_order_fit_ws_bytes", "mdl_cox_fit", "mdl_surv_metrics_ws_bytes", "mdl_surv_metrics"]


def test_entry_points_declared_bound_and_exported():
    import madeleine_amd
    from madeleine_amd import _native, functional as F, survival
    assert _native.ABI_VERSION == 26 and _native.lib().mdl_abi_version() == 26      # additive entries: the revision stays
    for name in ENTRY_POINTS:
        assert name in _native.SIGNATURES and getattr(_native.lib(), name).argtypes == _native.SIGNATURES[name][1], name
    assert len(_native.SIGNATURES["mdl_cox_fit"][1]) == 20 and len(_native.SIGNATURES["mdl_surv_metrics"][1]) == 16
    assert _native._DEFINES["MDL_COX_MAX_TRAIN"] == 1024
    for name in ("cox_fit", "survival_metrics"):
        assert callable(getattr(F, name))
    for name in ("survival_splits", "fit_cox", "survival_probe"):
        assert getattr(madeleine_amd, name) is getattr(survival, name) and name in madeleine_amd.__all__


def test_argument_validation_return_codes():
    """Every refusal below is decided on the host before anything is launched: the pointers are never dereferenced."""
    from madeleine_amd import _native
    lib, d = _native.lib(), _native._DEFINES
    ARG, UNS, ALIGN = d["MDL_E_ARG"], d["MDL_E_UNSUPPORTED"], d["MDL_E_ALIGN"]
    q = 4096      # a non-null, 16-byte aligned address
    assert lib.mdl_cox_order_fit_ws_bytes(10, 922, 512) == 48 + 10 * 922 * 4 + 10 * 960 * 960 * 4      # status, order, Gram (ld 960)
    assert lib.mdl_cox_order_fit_ws_bytes(1, 1024, 1) == 16 + 4096 + 1024 * 1024 * 4
    assert lib.mdl_cox_order_fit_ws_bytes(1, 1025, 8) == UNS and lib.mdl_cox_order_fit_ws_bytes(0, 8, 8) == ARG
    assert lib.mdl_cox_order_fit_ws_bytes(1, 8, 0) == ARG and lib.mdl_cox_order_fit_ws_bytes(2 ** 31, 8, 8) == UNS
    assert lib.mdl_surv_metrics_ws_bytes(2, 100) == 16 + 2400 + 2 * 112
    assert lib.mdl_surv_metrics_ws_bytes(1, 16385) == UNS and lib.mdl_surv_metrics_ws_bytes(1, 16384) > 0
    assert lib.mdl_surv_metrics_ws_bytes(0, 10) == ARG

    def fit(X=q, ldX=8, S=100, dd=8, t=q, ldt=0, e=q, lde=0, ti=q, nt=q, P=4, n_max=10, cost=1.0, gtol=1e-3, it=10, W=q, thr=q, info=q,
            ws=q):
        return lib.mdl_cox_fit(X, ldX, S, dd, t, ldt, e, lde, ti, nt, P, n_max, cost, gtol, it, W, thr, info, ws, None)

    for null in ("X", "t", "e", "ti", "nt", "W", "thr", "info", "ws"):
        assert fit(**{null: None}) == ARG, null
    assert fit(ldX=7) == ARG and fit(dd=0, ldX=0) == ARG and fit(P=0) == ARG and fit(S=0) == ARG and fit(it=-1) == ARG
    assert fit(ldt=50) == ARG and fit(lde=99) == ARG and fit(cost=0.0) == ARG and fit(gtol=-1.0) == ARG
    assert fit(n_max=1025) == UNS and fit(S=2 ** 31) == UNS and fit(P=2 ** 31) == UNS
    assert fit(P=2 ** 24, n_max=1024) == UNS         # P * n_max leaves int32
    assert fit(ws=q + 4) == ALIGN

    def metrics(z=q, t=q, ldt=0, e=q, lde=0, ti=q, nt=q, P=4, n_max=10, S=100, thr=q, c=q, chi=q, cnt=q, ws=q):
        return lib.mdl_surv_metrics(z, t, ldt, e, lde, ti, nt, P, n_max, S, thr, c, chi, cnt, ws, None)

    for null in ("z", "t", "e", "ti", "nt", "thr", "c", "chi", "cnt", "ws"):
        assert metrics(**{null: None}) == ARG, null
    assert metrics(S=16385) == UNS and metrics(n_max=1025) == UNS and metrics(ldt=99) == ARG and metrics(lde=1) == ARG
    assert metrics(ws=q + 8) == ALIGN and metrics(c=q + 4) == ALIGN and metrics(chi=q + 4) == ALIGN


def test_survival_splits():
    from madeleine_amd import survival_splits
    n = torch.arange(103)
    event = torch.where(n % 3 == 0, 0, 1)
    event[n % 10 == 7] = -1
    labeled = set(torch.nonzero(event >= 0)[:, 0].tolist())
    for folds in (2, 5):
        train = survival_splits(event, folds, repeat=1, seed_base=3)
        assert len(train) == folds and all(t.dtype == torch.int64 for t in train)
        held = [labeled - set(t.tolist()) for t in train]
        assert all(set(t.tolist()) <= labeled for t in train)                     # -1 is never drawn
        assert set().union(*held) == labeled and sum(map(len, held)) == len(labeled)      # the held-out parts partition the labeled cases
        ev = [sum(int(event[i]) for i in h) for h in held]
        assert max(ev) - min(ev) <= 1 and max(map(len, held)) - min(map(len, held)) <= 1      # events, and cases, balanced to within one
        again = survival_splits(event.numpy(), folds, repeat=1, seed_base=3)
        assert all(torch.equal(a, b) for a, b in zip(train, again))
    draws = {tuple(survival_splits(event, 5, r, s)[0].tolist()) for r in range(3) for s in (0, 7)}
    assert len(draws) == 6                                                       # repeat and seed_base move the draw
    with pytest.raises(ValueError):
        survival_splits(torch.tensor([1, 0, -1, -1, 1, -1]), 5)                   # three cases with follow-up, five folds
    with pytest.raises(ValueError):
        survival_splits(torch.ones(1400, dtype=torch.int64), 5)                   # 1120 training cases per fold: above the limit
    assert max(t.numel() for t in survival_splits(torch.ones(1153, dtype=torch.int64), 5)) == 923


def test_reference_against_a_partial_likelihood_worked_by_hand():
    """Five cases, one feature.  (time, event, x): (5, 1, 1), (3, 1, -1), (3, 1, 2), (3, 0, 0.5), (1, 1, 0).  Risk sets: the event at 5 has
    {1}; BOTH tied events at 3 have {1, 2, 3, 4} (Breslow: the whole tie group stays in each denominator; Efron would thin the second);
    the event at 1 has everybody.  With q_k = exp(w x_k):
        loss = [log q1 - w] + [log(q1 + q2 + q3 + q4) + w] + [log(q1 + q2 + q3 + q4) - 2 w] + log(q1 + q2 + q3 + q4 + q5)."""
    time = torch.tensor([5.0, 3.0, 3.0, 3.0, 1.0], dtype=torch.float64)
    event = torch.tensor([1, 1, 1, 0, 1])
    x = [1.0, -1.0, 2.0, 0.5, 0.0]
    w, cost = 0.3, 2.0
    q = [math.exp(w * v) for v in x]
    s4, s5 = sum(q[:4]), sum(q)
    loss = (math.log(q[0]) - w) + (math.log(s4) + w) + (math.log(s4) - 2 * w) + math.log(s5)
    m4, m5 = sum(v * k for v, k in zip(x[:4], q[:4])) / s4, sum(v * k for v, k in zip(x, q)) / s5      # risk-set means of x
    grad = (1.0 - 1.0) + (m4 + 1.0) + (m4 - 2.0) + (m5 - 0.0)
    X = torch.tensor(x, dtype=torch.float64)[:, None]
    obj, g = R.cox_objective(X, time, event, torch.tensor([w], dtype=torch.float64), cost)
    assert abs(float(obj) - (cost * loss + 0.5 * w * w)) < 1e-14
    assert abs(float(g[0]) - (cost * grad + w)) < 1e-14
    # the optimum: the gradient vanishes there, and the objective is no larger than at its neighbours
    wo, res, _ = R.newton_fit(X, time, event, cost)
    assert res < 1e-12
    f = lambda v: float(R.cox_objective(X, time, event, torch.tensor([v], dtype=torch.float64), cost)[0])
    assert f(float(wo)) <= min(f(float(wo) - 1e-4), f(float(wo) + 1e-4))


def test_reference_metrics_on_hand_counts():
    """Four test cases (time, event, z): a (1, 1, 0.9), b (2, 1, 0.1), c (2, 0, 0.5), d (3, 0, 0.1).  Comparable: (a, b), (a, c), (a, d) by
    time; (b, c) by the event / censored tie; (b, d) by time: five pairs.  a ranks above all three (2 each), b below c (0), b ties d (1):
    numerator 7, C = 0.7.  Split at 0.3: high = {a, c}.  a: n 4, h 2, d 1: O - E = 1 - 1/2, V = 1/4 * 3/3.  b: n 3, h 1, d 1:
    O - E += 0 - 1/3, V += 2/9 * 2/2."""
    time, event, z = np.array([1.0, 2.0, 2.0, 3.0]), np.array([1, 1, 0, 0]), np.array([0.9, 0.1, 0.5, 0.1])
    test = np.ones(4, dtype=bool)
    assert R.concordance(z, time, event, test) == (7, 5)
    lr = R.logrank(z, 0.3, time, event, test)
    assert abs(lr["O_E"] - (0.5 - 1.0 / 3.0)) < 1e-15 and abs(lr["V"] - (0.25 + 2.0 / 9.0)) < 1e-15
    assert (lr["n_test"], lr["n_high"], lr["events_low"], lr["events_high"]) == (4, 2, 1, 1)
    assert R.test_mask(np.array([1, 0, -1, 1, 0]), np.array([3])).tolist() == [True, True, False, False, True]


@pytest.mark.parametrize("name", list(R.COHORTS))
def test_cohorts_have_ties_censoring_and_signal(name):
    """What the GPU tests rely on: tie groups that hold an event and a censored case, about 30 % censored, and a held-out fp64 C-index of
    at least 0.65 for every fit on 63 or more cases -- at 0.5 a sign error in the fit would be invisible."""
    co = R.cohort(name)
    tm, ev = co["time"].numpy(), co["event"].numpy()
    assert bool((ev == -1).any())
    assert 0.25 <= float((ev == 0).sum()) / float((ev >= 0).sum()) <= 0.35
    assert any(((tm == tm[i]) & (ev == 0)).any() for i in np.nonzero(ev == 1)[0])
    assert any((((tm == tm[i]) & (ev == 1)).sum() > 1) for i in np.nonzero(ev == 1)[0])
    for pr in co["problems"]:
        idx = pr["idx"].numpy()
        assert bool((ev[idx] >= 0).all())
        if idx.size >= 63:
            tt, te = tm[idx], ev[idx]
            assert any(((tt == tt[i]) & (te == 0)).any() for i in np.nonzero(te == 1)[0])      # inside the training list too
            c = R.c_index(*R.concordance(pr["z64"].numpy(), tm, ev, R.test_mask(ev, idx)))
            print("%s n=%d: held-out fp64 C-index %.4f, fp32 floor %.2e of g0" % (name, idx.size, c, pr["r32"] / pr["g0"]))
            assert c >= 0.65, (name, idx.size, c)


def test_no_device_is_an_error(monkeypatch):
    from madeleine_amd import fit_cox, functional as F, survival_probe
    X, t, e = torch.zeros(8, 4), torch.ones(8), torch.ones(8, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fit_cox(X, t, e, [torch.tensor([0, 1, 2])])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.cox_fit(X, t, e, torch.zeros(1, 3, dtype=torch.int32), torch.ones(1, dtype=torch.int32))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="needs a ROCm device"):
        survival_probe(X.numpy(), t.numpy(), e.numpy(), folds=2)
