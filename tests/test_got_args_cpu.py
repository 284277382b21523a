"""Argument checks of the 22 GOT entry points without a GPU (csrc/got_host.hpp: got_check, the only place that refuses a GOT call).  One
order for the four families (mdl_got_*, mdl_got_*_multi, mdl_got_tiled_*, mdl_got_tiled_rect_*), each step over all problems of a call
before the next step begins:
  1. MDL_E_ARG: np outside [1, MDL_GOT_MAX_BATCH] or a NULL array of a _multi form; k, n, m < 0, d < 1; an empty problem of a _multi form
  2. MDL_E_UNSUPPORTED: a size beyond the engine's limits (resident n <= 512, d <= 128; a _multi problem n <= 256; tiled n, m, d <= 4096)
  3. MDL_E_ARG: ws NULL; out (forward), minmax_out (extrema), d_out (backward begin) NULL; extrema of an empty problem; V, Q, dV, dQ NULL
     while the tensor has elements (k n d, for Q and dQ k m d)
  4. MDL_E_ALIGN: ws off 16 bytes
  5. the empty problem: MDL_OK, nothing launched.
All pointers are fake host addresses, so no call here may reach a launch or a memset: every call carries a fault (which the library
before got_check refused before its first HIP call as well), and "is accepted" is read off a later step's code -- a NULL V of an empty
problem together with a misaligned ws gives MDL_E_ALIGN, not MDL_E_ARG.  Codes that differ from the library before got_check:
DESIGN.md section 3.5."""
import ctypes

import pytest

from madeleine_amd import _native

OK, E_ARG, E_ALIGN, E_UNSUP = 0, -1, -2, -3
MAX_BATCH = _native._DEFINES["MDL_GOT_MAX_BATCH"]

_RAW = ctypes.create_string_buffer(4096)
_P0 = (ctypes.addressof(_RAW) + 15) & ~15


def P(i):
    """The i-th fake pointer: host memory, 16-byte aligned, never dereferenced before a launch."""
    return _P0 + 64 * i


K0, N0, M0, D0 = 2, 8, 9, 8
NP0 = 2      # problems of the valid _multi call
PTRS = {name: P(i) for i, name in enumerate(
    ["V", "Q", "out", "minmax_out", "minmax_in", "d_out", "d_minmax", "dV", "dQ", "d_minmax_total", "ws"])}
TOKENS = {"V": "n", "Q": "m", "dV": "n", "dQ": "m"}     # may be NULL while k * (that size) * d == 0

# stage -> (pointer arguments in the header's order, those that are refused when NULL, those that may always be NULL)
STAGES = {
    "fwd": (["V", "Q", "out", "minmax_out", "minmax_in"], ["out"], ["minmax_out", "minmax_in"]),
    "extrema": (["V", "Q", "minmax_out"], ["minmax_out"], []),
    "bwd_begin": (["d_out", "d_minmax"], ["d_out"], ["d_minmax"]),
    "bwd_finish": (["V", "Q", "dV", "dQ", "d_minmax_total"], [], ["d_minmax_total"]),
    "bwd": (["V", "Q", "d_out", "dV", "dQ"], ["d_out"], []),
}
MULTI_STAGES = {      # the _multi forms take minmax_in alone in the forward
    "fwd": (["V", "Q", "out", "minmax_in"], ["out"], ["minmax_in"]),
    "extrema": STAGES["extrema"], "bwd_begin": STAGES["bwd_begin"], "bwd_finish": STAGES["bwd_finish"],
}
LIMITS = {"resident": dict(n=512, d=128), "multi": dict(n=256, d=128), "tiled": dict(n=4096, d=4096), "rect": dict(n=4096, m=4096, d=4096)}


class Entry:
    def __init__(self, name, family, stage):
        self.name, self.family, self.stage = name, family, stage
        self.multi, self.rect = family == "multi", family == "rect"
        self.ptrs, self.required, self.optional = (MULTI_STAGES if self.multi else STAGES)[stage]
        self.tokens = [p for p in self.ptrs if p in TOKENS]
        self.limits = LIMITS[family]
        self.sizes = ["k", "n"] + (["m"] if self.rect else []) + ["d"]


ENTRIES = ([Entry("mdl_got_" + s, "resident", s) for s in STAGES] + [Entry("mdl_got_%s_multi" % s, "multi", s) for s in MULTI_STAGES] +
           [Entry("mdl_got_tiled_" + s, "tiled", s) for s in STAGES] + [Entry("mdl_got_tiled_rect_" + s, "rect", s) for s in STAGES])
WS_QUERIES = [("mdl_got_ws_bytes", "resident"), ("mdl_got_tiled_ws_bytes", "tiled"), ("mdl_got_tiled_rect_ws_bytes", "rect")]
assert len(ENTRIES) + len(WS_QUERIES) == 22
IDS = [e.name for e in ENTRIES]
MIS = {"ws": PTRS["ws"] + 4}      # the fault of step 4: behind it a call is accepted


@pytest.fixture(scope="module")
def lib():
    return _native.lib()


def _has_fault(e, kw):
    """A fault that the library refuses before any HIP call -- by got_check, and by the checks it replaced."""
    if "ws" in kw or "np" in kw or "null_array" in kw:
        return True
    per = [dict((k, v[p] if isinstance(v, tuple) else v) for k, v in kw.items()) for p in range(NP0 if e.multi else 1)]
    for q in per:
        size = dict(k=q.get("k", K0), n=q.get("n", N0), d=q.get("d", D0))
        size["m"] = q.get("m", M0) if e.rect else size["n"]
        if min(size["k"], size["n"], size["m"]) < 0 or size["d"] < 1 or any(size[s] > lim for s, lim in e.limits.items()):
            return True
        empty = 0 in (size["k"], size["n"], size["m"])
        if empty and (e.multi or e.stage == "extrema"):
            return True
        for name in e.ptrs:
            if name in q and q[name] is None and name not in e.optional:
                if name not in TOKENS or size["k"] * size[TOKENS[name]] != 0:
                    return True
    return False


def _caller(lib, e):
    fn = getattr(lib, e.name)

    def single(**kw):
        assert set(kw) <= set(e.ptrs) | set(e.sizes) | {"ws"}, kw
        assert _has_fault(e, kw), ("a call without a fault would launch", kw)
        base = dict(PTRS, k=K0, n=N0, m=M0, d=D0)
        return fn(*[kw.get(a, base[a]) for a in e.ptrs + e.sizes + ["ws"]], None)

    def multi(np=NP0, null_array=None, **kw):
        """A value is that of every problem, or a tuple with one per problem.  null_array: that array argument is NULL."""
        given = dict(kw, **({"np": np} if np != NP0 else {}), **({"null_array": null_array} if null_array else {}))
        assert set(kw) <= set(e.ptrs) | {"k", "n", "d", "ws"}, kw
        assert _has_fault(e, given), ("a call without a fault would launch", given)
        at = lambda name, p, base: (lambda v: v[p] if isinstance(v, tuple) else v)(kw.get(name, base))      # noqa: E731

        def array(name, ctype, base):
            if null_array == name:
                return None
            return (ctype * NP0)(*[at(name, p, base if ctype is ctypes.c_int else base + 1024 * p) for p in range(NP0)])
        args = [np] + [array(a, ctypes.c_void_p, PTRS[a]) for a in e.ptrs]
        args += [array("k", ctypes.c_int, K0), array("n", ctypes.c_int, N0), kw.get("d", D0), array("ws", ctypes.c_void_p, PTRS["ws"]), None]
        return fn(*args)
    return multi if e.multi else single


def _mis(e):
    """ws off 16 bytes: of every problem but the first one of a _multi call, so that the last problem decides."""
    return {"ws": (PTRS["ws"], PTRS["ws"] + 1024 + 4)} if e.multi else MIS


def _empties(e):
    """The ways of a single problem to be empty, with the token pointers that then have no elements."""
    ways = [(dict(k=0), e.tokens), (dict(n=0), [t for t in e.tokens if TOKENS[t] == "n" or not e.rect])]
    if e.rect:
        ways.append((dict(m=0), [t for t in e.tokens if TOKENS[t] == "m"]))
    return ways


@pytest.mark.parametrize("e", ENTRIES, ids=IDS)
def test_got_argument_checks(lib, e):
    call, mis = _caller(lib, e), _mis(e)
    assert set(e.ptrs) == set(e.required) | set(e.optional) | set(e.tokens), "every pointer is classified"
    # 1. the sizes, and the arrays of a _multi form
    for s in e.sizes:
        assert call(**{s: 0 if s == "d" else -1}) == E_ARG, s
    assert call(d=-3) == E_ARG
    if e.multi:
        for np in (0, -1, MAX_BATCH + 1):
            assert call(np=np) == E_ARG, np
        for a in ["k", "n", "ws"] + e.required + e.tokens:
            assert call(null_array=a) == E_ARG, (a, "a NULL array")
        for a in e.optional:
            assert call(null_array=a, **mis) == E_ALIGN, (a, "this array may be NULL")
        assert call(k=(K0, 0)) == E_ARG and call(n=(0, N0)) == E_ARG, "the caller filters empty problems"
        assert call(k=(K0, -1)) == E_ARG and call(n=(N0, -1)) == E_ARG
    # 2. the limits, on both sides
    for s, lim in e.limits.items():
        assert call(**{s: lim}, **mis) == E_ALIGN, (s, lim, "within the class")
        assert call(**{s: lim + 1}) == E_UNSUP, (s, lim + 1)
        if e.multi:
            assert call(**{s: (1, lim + 1) if s != "d" else lim + 1}) == E_UNSUP
    # 3. the pointers
    assert call(ws=None) == E_ARG
    for name in e.required:
        assert call(**{name: None}) == E_ARG, (name, "required")
    for name in e.optional:
        assert call(**{name: None}, **mis) == E_ALIGN, (name, "may be NULL")
    for name in e.tokens:
        assert call(**{name: None}) == E_ARG, (name, "NULL with elements")
    if e.multi:
        assert call(ws=(PTRS["ws"], None)) == E_ARG
        for name in e.required + e.tokens:
            assert call(**{name: (PTRS[name], None)}) == E_ARG, (name, "of the second problem")
    else:
        for size, free in _empties(e):
            if e.stage == "extrema":
                assert call(**size) == E_ARG, (size, "extrema of an empty problem")
                continue
            assert call(**size, **MIS) == E_ALIGN, (size, "the empty problem is served")
            assert call(**size, **{t: None for t in free}, **MIS) == E_ALIGN, (size, free, "no elements: may be NULL")
            for t in set(e.tokens) - set(free):
                assert call(**size, **{t: None}) == E_ARG, (size, t, "the other side's tensor has elements")
            for name in e.required:
                assert call(**size, **{name: None}) == E_ARG, (size, name, "required of an empty problem too")
    # 4. alignment of ws
    assert call(**mis) == E_ALIGN
    assert call(ws=PTRS["ws"] + 8) == E_ALIGN and call(ws=PTRS["ws"] + 1) == E_ALIGN


@pytest.mark.parametrize("e", ENTRIES, ids=IDS)
def test_got_check_order(lib, e):
    """One pair of faults per pair of steps."""
    call, mis = _caller(lib, e), _mis(e)
    over = {s: lim + 1 for s, lim in e.limits.items()}
    nulls = ["ws"] + e.required + e.tokens
    for s in e.sizes:
        bad = {s: 0 if s == "d" else -1}
        for t, v in over.items():
            if t != s:
                assert call(**bad, **{t: v}) == E_ARG, (s, t, "1 before 2")
        assert call(**bad, **mis) == E_ARG, (s, "1 before 4")
    for t, v in over.items():
        for name in nulls:
            assert call(**{t: v}, **{name: None}) == E_UNSUP, (t, name, "2 before 3")
        assert call(**{t: v}, **mis) == E_UNSUP, (t, "2 before 4")
    for name in nulls:
        if name != "ws":
            assert call(**{name: None}, **mis) == E_ARG, (name, "3 before 4")
    if e.multi:      # a step runs over all problems before the next one begins
        assert call(n=(LIMITS["multi"]["n"] + 1, N0), k=(K0, -1)) == E_ARG, "1 of the second problem before 2 of the first"
        assert call(n=(LIMITS["multi"]["n"] + 1, N0), k=(K0, 0)) == E_ARG
        assert call(ws=(PTRS["ws"] + 4, PTRS["ws"] + 1024), n=(N0, LIMITS["multi"]["n"] + 1)) == E_UNSUP, "2 of the second before 4 of the first"
        for name in nulls:
            if name != "ws":
                assert call(ws=(PTRS["ws"] + 4, PTRS["ws"] + 1024), **{name: (PTRS[name], None)}) == E_ARG, (name, "3 of the second before 4")
        assert call(ws=(PTRS["ws"] + 4, None)) == E_ARG
        assert call(np=MAX_BATCH + 1, n=LIMITS["multi"]["n"] + 1) == E_ARG and call(null_array=nulls[1], d=LIMITS["multi"]["d"] + 1) == E_ARG
    elif e.stage == "extrema":
        assert call(k=0, **MIS) == E_ARG and call(n=0, **MIS) == E_ARG, "3 (extrema of an empty problem) before 4"
    else:
        assert call(k=0, **MIS) == E_ALIGN, "4 before 5"
        assert call(k=0, ws=None) == E_ARG and call(k=0, n=e.limits["n"] + 1) == E_UNSUP and call(k=0, d=0) == E_ARG, "1, 2, 3 before 5"
    if e.stage == "bwd":      # both stages are checked before the first one runs
        for name in ("dV", "dQ", "V", "Q"):
            assert call(**{name: None}, **MIS) == E_ARG, (name, "a fault of the second stage before the first stage's alignment")


@pytest.mark.parametrize("name,family", WS_QUERIES, ids=[q[0] for q in WS_QUERIES])
def test_got_ws_queries_read_the_same_limits(lib, name, family):
    fn, sizes = getattr(lib, name), ["k", "n"] + (["m"] if family == "rect" else []) + ["d"]
    base = dict(k=K0, n=N0, m=M0, d=D0)
    ask = lambda **kw: fn(*[kw.get(s, base[s]) for s in sizes])      # noqa: E731
    assert ask() > 0 and ask(k=0) > 0 and ask(n=0) > 0
    for s in sizes:
        assert ask(**{s: 0 if s == "d" else -1}) == E_ARG, s
    for s, lim in LIMITS[family].items():
        assert ask(**{s: lim}, k=1) > 0 and ask(**{s: lim + 1}) == E_UNSUP, (s, lim)
        assert ask(**{s: lim + 1}, k=-1) == E_ARG, "the sizes before the limits"


def test_every_launching_got_entry_point_is_in_the_table():
    launching = {n for n, (_res, args) in _native.SIGNATURES.items() if n.startswith("mdl_got_") and args and args[-1] is ctypes.c_void_p}
    assert launching == {e.name for e in ENTRIES} and len(launching) == 19
    assert {n for n in _native.SIGNATURES if n.startswith("mdl_got_")} - launching == {q[0] for q in WS_QUERIES}
