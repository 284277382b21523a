"""Argument checks of the probe family without a GPU (csrc/probe_host.hpp: probe_check, the only place that refuses a call that takes a
problem table).  One order for the few-shot probe, the full-label probe, the survival probe and their bootstrap:
  1. MDL_E_ARG: a NULL pointer; P, n_max or S (G) < 1; d < 1 or ldX < d; max_iter < 0, cost not > 0, gtol not >= 0; R < 0; a column
     stride (ldy, ldt, lde) neither 0 nor >= S
  2. MDL_E_UNSUPPORTED: n_max, d or S beyond the entry point's limits, C outside 2 .. MDL_PROBE_MAX_CLASSES; R + 1 beyond int32; S, P,
     P * n_max, P * cols * d or a launch grid beyond int32
  3. MDL_E_ALIGN: ws off 16 bytes, and the 8 / 4 / 2-byte alignments an entry point states.
All pointers are fake host addresses, so no call here may reach a launch: every call carries a fault (`_model` below says so before the
library is asked), and "accepted up to step k" is read off a later step's code -- a launch grid beyond int32 together with ws + 4 gives
MDL_E_UNSUPPORTED, ws + 4 alone MDL_E_ALIGN.  The one code that differs from the library before probe_check (that pair, for the fits and
metrics whose grids used to be checked behind the alignment): DESIGN.md section 3.18.1."""
import ctypes

import pytest

from madeleine_amd import _native

OK, E_ARG, E_ALIGN, E_UNSUP = 0, -1, -2, -3
D = dict(_native._DEFINES, **_native.STATS_DEFINES)
CMAX, CASES = D["MDL_PROBE_MAX_CLASSES"], D["MDL_PROBE_MAX_CASES"]
I32 = 0x7FFFFFFF

_RAW = ctypes.create_string_buffer(8192)
_P0 = (ctypes.addressof(_RAW) + 15) & ~15
POINTERS = ["X", "y", "time", "event", "train_idx", "n_train", "z", "thr", "group", "W_out", "b_out", "thr_out", "info_out",
            "confusion_out", "auc_out", "auc_num_out", "c_index_out", "chi2_out", "counts_out", "ws", "W", "b", "z_out", "w_out"]
PTRS = {name: _P0 + 64 * i for i, name in enumerate(POINTERS)}      # host memory, 16-byte aligned, never dereferenced before a launch
BASE = dict(PTRS, ldX=8, S=40, d=8, ldy=0, ldt=0, lde=0, P=3, n_max=5, C=3, cost=1.0, gtol=1e-4, max_iter=10, seed=7, R=4, G=2, stream=None)

_FIT = "X ldX S d y ldy train_idx n_train P n_max C cost gtol max_iter W_out b_out info_out ws stream"
_METRICS = "z y ldy train_idx n_train P n_max S C confusion_out auc_out ws stream"


def _ceil(a, b):
    return -(-a // b)


def _cols(v):
    return 1 if v["C"] == 2 else v["C"]


class Entry:
    """An entry point that takes a problem table: its arguments in the header's order, its limits, what else must fit int32 (beside S, P
    and P * n_max) and what must be aligned beside ws."""

    def __init__(self, name, args, n_max, grids, d=None, S=None, align=(), columns=("ldy",)):
        self.name, self.args = name, args.split()
        self.limits = {k: v for k, v in (("n_max", n_max), ("d", d), ("S", S)) if v is not None}
        self.grids, self.align, self.columns = grids, {p: a for p, a in align if p in self.args}, columns
        self.pointers = [a for a in self.args if a in PTRS]
        self.fit, self.classes, self.reps, self.ws = "ldX" in self.args, "C" in self.args, "R" in self.args, "ws" in self.args
        self.changed = name in ("mdl_probe_fit", "mdl_probe_metrics", "mdl_logit_metrics", "mdl_cox_fit", "mdl_surv_metrics")


def _gram(v):
    return v["P"] * _ceil(v["n_max"], 64) ** 2


def _pairs(v):
    return v["P"] * _cols(v) * _ceil(v["S"], 256)


def _blocks(v):
    return v["P"] * (v["R"] // D["MDL_BOOT_REP_BLOCK"] + 1)


_FOUR = [(a, 4) for a in ("z", "y", "time", "event", "train_idx", "n_train", "group", "confusion_out")]
ENTRIES = [
    Entry("mdl_probe_fit", _FIT, D["MDL_PROBE_MAX_TRAIN"], [_gram, lambda v: v["P"] * _cols(v) * v["d"]]),
    Entry("mdl_probe_metrics", _METRICS, D["MDL_PROBE_MAX_TRAIN"], [_pairs], S=CASES),
    Entry("mdl_logit_fit", _FIT, D["MDL_LOGIT_MAX_TRAIN"], [lambda v: v["P"] * _cols(v) * v["d"]], d=D["MDL_LOGIT_MAX_DIM"]),
    Entry("mdl_logit_metrics", _METRICS, D["MDL_LOGIT_MAX_TRAIN"], [_pairs], S=CASES),
    Entry("mdl_cox_fit", "X ldX S d time ldt event lde train_idx n_train P n_max cost gtol max_iter W_out thr_out info_out ws stream",
          D["MDL_COX_MAX_TRAIN"], [_gram, lambda v: v["P"] * v["d"]], columns=("ldt", "lde")),
    Entry("mdl_surv_metrics", "z time ldt event lde train_idx n_train P n_max S thr c_index_out chi2_out counts_out ws stream",
          D["MDL_COX_MAX_TRAIN"], [lambda v: v["P"] * _ceil(v["S"], 256)], S=CASES, align=[("c_index_out", 8), ("chi2_out", 8)],
          columns=("ldt", "lde")),
    Entry("mdl_boot_class_counts", "z y ldy train_idx n_train P n_max S C group seed R confusion_out auc_num_out ws stream",
          D["MDL_LOGIT_MAX_TRAIN"], [_pairs, _blocks], S=CASES, align=[("auc_num_out", 8)] + _FOUR),
    Entry("mdl_boot_surv_counts", "z time ldt event lde train_idx n_train P n_max S group seed R counts_out stream",
          D["MDL_COX_MAX_TRAIN"], [_blocks], S=D["MDL_BOOT_SURV_MAX_TEST"], align=[("counts_out", 8)] + _FOUR, columns=("ldt", "lde")),
]
IDS = [e.name for e in ENTRIES]
# name -> (arguments, limits, classes): the *_ws_bytes queries read the rows of their entry points
WS_QUERIES = {
    "mdl_probe_fit_ws_bytes": ("P n_max d C", dict(n_max=D["MDL_PROBE_MAX_TRAIN"])),
    "mdl_probe_metrics_ws_bytes": ("P S C", dict(S=CASES)),
    "mdl_logit_fit_ws_bytes": ("P n_max d C", dict(n_max=D["MDL_LOGIT_MAX_TRAIN"], d=D["MDL_LOGIT_MAX_DIM"])),
    "mdl_logit_metrics_ws_bytes": ("P S C", dict(S=CASES)),
    "mdl_cox_order_fit_ws_bytes": ("P n_max d", dict(n_max=D["MDL_COX_MAX_TRAIN"])),
    "mdl_surv_metrics_ws_bytes": ("P S", dict(S=CASES)),
    "mdl_boot_class_ws_bytes": ("P S C", dict(S=CASES)),
}


@pytest.fixture(scope="module")
def lib():
    return _native.lib()


def _model(e, v):
    """The code the three steps give the call with the values v."""
    if any(v[p] is None for p in e.pointers) or min(v["P"], v["n_max"], v["S"]) < 1:
        return E_ARG
    if e.fit and (v["d"] < 1 or v["ldX"] < v["d"] or v["max_iter"] < 0 or not v["cost"] > 0 or not v["gtol"] >= 0):
        return E_ARG
    if (e.reps and v["R"] < 0) or any(v[ld] != 0 and v[ld] < v["S"] for ld in e.columns):
        return E_ARG
    if any(v[k] > lim for k, lim in e.limits.items()) or (e.classes and not 2 <= v["C"] <= CMAX) or (e.reps and v["R"] > I32 - 1):
        return E_UNSUP
    if max(v["S"], v["P"], v["P"] * v["n_max"], *[g(v) for g in e.grids]) > I32:
        return E_UNSUP
    if (e.ws and v["ws"] % 16) or any(v[p] % a for p, a in e.align.items()):
        return E_ALIGN
    return OK


def _caller(lib, e):
    fn = getattr(lib, e.name)

    def call(**kw):
        assert set(kw) <= set(e.args), kw
        v = dict(BASE, **kw)
        want = _model(e, v)
        assert want != OK, ("a call without a fault would launch", kw)
        got = fn(*[v[a] for a in e.args])
        assert got == want, (kw, "the library and the three steps disagree", got, want)
        return got
    return call


def _mis(e):
    """The fault of step 3: behind it a call is accepted."""
    return {"ws": PTRS["ws"] + 4} if e.ws else {"counts_out": PTRS["counts_out"] + 4}


def _grid_faults(e):
    """Calls whose fault is a launch grid or an element count beyond int32; in all but the Gram case every limit and P * n_max hold."""
    out = []
    if e.fit:
        out.append(dict(P=2 ** 22 // (8 if e.classes else 1), C=8, n_max=1, d=1024, ldX=1024) if e.classes else
                   dict(P=2 ** 22, n_max=1, d=1024, ldX=1024))
    if "mdl_probe_fit" == e.name or "mdl_cox_fit" == e.name:
        out.append(dict(P=2 ** 27, n_max=e.limits["n_max"]))      # the Gram tiles; P * n_max = 2^35 / 2^37 is beyond int32 as well
    if not e.fit and not e.reps:
        out.append(dict(P=2 ** 25, n_max=1, S=CASES))
    if e.reps:
        out.append(dict(P=8, R=I32 - 1))
        if e.classes:
            out.append(dict(P=2 ** 25, n_max=1, S=CASES, R=0))
    return out


@pytest.mark.parametrize("e", ENTRIES, ids=IDS)
def test_probe_argument_checks(lib, e):
    call, mis = _caller(lib, e), _mis(e)
    # 1. pointers, sizes, solver arguments, strides
    for p in e.pointers:
        assert call(**{p: None}) == E_ARG, p
    for s in ("P", "n_max", "S"):
        assert call(**{s: 0}) == E_ARG and call(**{s: -1}) == E_ARG, s
    for ld in e.columns:
        assert call(**{ld: BASE["S"] - 1}) == E_ARG and call(**{ld: -1}) == E_ARG and call(**{ld: 1}) == E_ARG, ld
        assert call(**{ld: BASE["S"]}, **mis) == E_ALIGN and call(**{ld: BASE["S"] + 3}, **mis) == E_ALIGN, (ld, "a stride >= S")
    if e.fit:
        assert call(d=0) == E_ARG and call(ldX=BASE["d"] - 1) == E_ARG and call(max_iter=-1) == E_ARG
        assert call(cost=0.0) == E_ARG and call(cost=-1.0) == E_ARG and call(cost=float("nan")) == E_ARG
        assert call(gtol=-1e-3) == E_ARG and call(gtol=float("nan")) == E_ARG
        assert call(gtol=0.0, max_iter=0, ldX=BASE["d"], **mis) == E_ALIGN, "the smallest legal solver arguments"
    if e.reps:
        assert call(R=-1) == E_ARG and call(R=0, **mis) == E_ALIGN
    # 2. the limits on both sides, the classes, the replicates, int32
    for k, lim in e.limits.items():
        ok = {k: lim, **({"ldX": lim} if k == "d" else {})}
        over = {k: lim + 1, **({"ldX": lim + 1} if k == "d" else {})}
        assert call(**ok, **mis) == E_ALIGN, (k, lim, "within the limit")
        assert call(**over) == E_UNSUP, (k, lim + 1)
    if e.classes:
        assert call(C=1) == E_UNSUP and call(C=0) == E_UNSUP and call(C=CMAX + 1) == E_UNSUP
        assert call(C=2, **mis) == E_ALIGN and call(C=CMAX, **mis) == E_ALIGN
    if e.reps:
        assert call(R=I32) == E_UNSUP and call(R=2 ** 40) == E_UNSUP, "R + 1 beyond int32"
        assert call(R=I32 - 1, P=1, **mis) == E_ALIGN, "the largest replicate count"
    assert call(P=2 ** 31) == E_UNSUP and call(P=2 ** 40) == E_UNSUP
    assert call(P=2 ** 29, n_max=4) == E_UNSUP, "P * n_max beyond int32"
    if "S" not in e.limits:
        assert call(S=2 ** 31) == E_UNSUP and call(S=2 ** 40) == E_UNSUP
    for fault in _grid_faults(e):
        assert call(**fault) == E_UNSUP, fault
    # 3. alignment
    if e.ws:
        assert call(ws=PTRS["ws"] + 4) == E_ALIGN and call(ws=PTRS["ws"] + 8) == E_ALIGN and call(ws=PTRS["ws"] + 1) == E_ALIGN
    for p, a in e.align.items():
        assert call(**{p: PTRS[p] + a // 2}) == E_ALIGN, (p, a)
        if a == 4 and e.ws:
            assert call(**{p: PTRS[p] + 4}, **mis) == E_ALIGN, (p, "4-byte aligned is enough")


@pytest.mark.parametrize("e", ENTRIES, ids=IDS)
def test_probe_check_order(lib, e):
    """One pair of faults per pair of steps."""
    call, mis = _caller(lib, e), _mis(e)
    arg = [{p: None} for p in e.pointers] + [{"P": 0}, {"n_max": 0}, {"S": 0}] + [{ld: 1} for ld in e.columns]
    arg += [{"d": 0}, {"ldX": 1}, {"max_iter": -1}, {"cost": 0.0}, {"gtol": -1.0}] if e.fit else []
    arg += [{"R": -1}] if e.reps else []
    unsup = [{"n_max": e.limits["n_max"] + 1}] + ([{"C": CMAX + 1}] if e.classes else []) + ([{"R": I32}] if e.reps else [])
    unsup += [{"S": e.limits["S"] + 1}] if "S" in e.limits else [{"S": 2 ** 31}]
    unsup += [{"d": e.limits["d"] + 1, "ldX": e.limits["d"] + 1}] if "d" in e.limits else []
    unsup += [{"P": 2 ** 31}] + _grid_faults(e)
    for a in arg:
        for u in unsup:
            if not set(a) & set(u):
                assert call(**a, **u) == E_ARG, (a, u, "1 before 2")
        if not set(a) & set(mis):
            assert call(**a, **mis) == E_ARG, (a, "1 before 3")
    for u in unsup:
        assert call(**u, **mis) == E_UNSUP, (u, "2 before 3")
        for p, al in e.align.items():
            assert call(**u, **{p: PTRS[p] + al // 2}) == E_UNSUP, (u, p, "2 before 3")


@pytest.mark.parametrize("e", [e for e in ENTRIES if e.changed], ids=[e.name for e in ENTRIES if e.changed])
def test_a_grid_beyond_int32_is_refused_before_a_misaligned_workspace(lib, e):
    """The one pair of faults whose code differs from the library before probe_check: these five checked the alignment of ws (and of the
    8-byte outputs) before the int32 bounds of their launch grids and answered MDL_E_ALIGN."""
    call = _caller(lib, e)
    for fault in _grid_faults(e):
        assert call(**fault, ws=PTRS["ws"] + 4) == E_UNSUP, fault
        for p, a in e.align.items():
            assert call(**fault, **{p: PTRS[p] + a // 2}) == E_UNSUP, (fault, p)
    assert call(ws=PTRS["ws"] + 4) == E_ALIGN, "each fault alone gives what it gave"


def test_probe_scores_checks(lib):
    args = "X ldX S d W b P C z_out stream".split()

    def call(**kw):
        return lib.mdl_probe_scores(*[dict(BASE, **kw)[a] for a in args])
    for p in ("X", "W", "b", "z_out"):
        assert call(**{p: None}) == E_ARG, p
    assert call(d=0) == E_ARG and call(ldX=BASE["d"] - 1) == E_ARG and call(P=0) == E_ARG and call(S=0) == E_ARG
    assert call(C=1) == E_UNSUP and call(C=CMAX + 1) == E_UNSUP
    assert call(S=2 ** 31) == E_UNSUP and call(P=2 ** 31) == E_UNSUP
    assert call(P=2 ** 28, S=256) == E_UNSUP, "the launch grid: P * ceil(S / 16)"
    assert call(P=2 ** 22, C=2, d=1024, ldX=1024, S=1) == E_UNSUP, "P * cols * d"
    assert call(C=1, S=0) == E_ARG and call(P=2 ** 31, X=None) == E_ARG, "1 before 2"


def test_boot_weights_checks(lib):
    args = "seed group G R S w_out stream".split()

    def call(**kw):
        return lib.mdl_boot_weights(*[dict(BASE, **kw)[a] for a in args])
    assert call(group=None) == E_ARG and call(w_out=None) == E_ARG
    assert call(G=0) == E_ARG and call(S=0) == E_ARG and call(R=-1) == E_ARG
    assert call(R=I32) == E_UNSUP and call(S=CASES + 1) == E_UNSUP and call(G=2 ** 31) == E_UNSUP
    assert call(G=2 ** 16, R=2 ** 15) == E_UNSUP, "the launch grid: G * (R + 1)"
    assert call(group=PTRS["group"] + 2) == E_ALIGN and call(w_out=PTRS["w_out"] + 1) == E_ALIGN
    assert call(S=CASES, R=I32 - 1, G=1, w_out=PTRS["w_out"] + 1) == E_ALIGN, "the limits themselves are accepted"
    assert call(S=CASES + 1, G=0) == E_ARG and call(R=I32, group=None) == E_ARG, "1 before 2"
    assert call(S=CASES + 1, w_out=PTRS["w_out"] + 1) == E_UNSUP and call(G=2 ** 31, group=PTRS["group"] + 2) == E_UNSUP, "2 before 3"


@pytest.mark.parametrize("name", list(WS_QUERIES))
def test_probe_ws_queries_read_the_same_limits(lib, name):
    names, limits = WS_QUERIES[name]
    names = names.split()

    def ask(**kw):
        return getattr(lib, name)(*[dict(BASE, **kw)[a] for a in names])
    assert ask() > 0
    for s in names:
        if s != "C":
            assert ask(**{s: 0}) == E_ARG and ask(**{s: -1}) == E_ARG, s
    for k, lim in limits.items():
        assert ask(**{k: lim}) > 0 and ask(**{k: lim + 1}) == E_UNSUP, (k, lim)
        assert ask(**{k: lim + 1}, P=0) == E_ARG, "the sizes before the limits"
    if "C" in names:
        assert ask(C=1) == E_UNSUP and ask(C=CMAX + 1) == E_UNSUP and ask(C=2) > 0 and ask(C=CMAX) > 0
        assert ask(C=1, P=0) == E_ARG
    assert ask(P=2 ** 31) == E_UNSUP and ask(P=I32, **{k: 1 for k in names if k in ("n_max", "S", "d")}, **({"C": 2} if "C" in names else {})) > 0


def test_every_entry_point_of_the_family_is_in_the_tables():
    sigs = dict(_native.SIGNATURES, **_native.STATS_SIGNATURES)
    family = {n for n in sigs if n.split("_")[1] in ("probe", "logit", "cox", "surv", "boot")}
    tested = {e.name for e in ENTRIES} | set(WS_QUERIES) | {"mdl_probe_scores", "mdl_boot_weights"}
    assert family == tested
    for e in ENTRIES:
        assert len(sigs[e.name][1]) == len(e.args), e.name
    for name, (names, _) in WS_QUERIES.items():
        assert len(sigs[name][1]) == len(names.split()), name
