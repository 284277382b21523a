"""Argument checks of the 11 launching gated-attention entry points without a GPU (csrc/gate_host.hpp: gate_check_fwd, gate_check_bwd,
and the mask export): one order for the three engines and both directions -- pointers, pairs, the pooling term and ranges (MDL_E_ARG),
then alignment (MDL_E_ALIGN), then the head count and the 32-bit stride limits (MDL_E_UNSUPPORTED), then the empty forward (MDL_OK),
then the grids (MDL_E_UNSUPPORTED).  All pointers are fake host addresses, so no call here may reach a launch: only the three forwards
(and the mask export, which launches nothing for no elements) are ever called without a fault, at T == 0; every backward call carries a
fault, and "is not refused" is read off a later step's code (a NULL optional pointer together with H = 3 gives MDL_E_UNSUPPORTED, not
MDL_E_ARG; a pointer that is not on the aligned list, offset by 4 bytes together with H = 3, gives MDL_E_UNSUPPORTED, not MDL_E_ALIGN).
The row strides have tests/test_strides_cpu.py.
Codes that differ from the library before gate_check_*: DESIGN.md section 3.3 -- (a) a forward with T == 0 and H in {3,5,6,7} is
MDL_E_UNSUPPORTED (was MDL_OK); (b) a backward with such an H and a bad p_drop is MDL_E_ARG, with a misaligned pointer MDL_E_ALIGN (both
were MDL_E_UNSUPPORTED); (c) wc, act_a and act_b of the forwards and dE of the fp32 backward are on the aligned list; (d) the fp32
backward (mdl_abmil_gate_bwd, mdl_abmil_attnpool_bwd, _phases with bit 0) refuses a grid above 2^31 - 1 (T = 2^40 here) before any HIP
call: it used to zero the pad rows of dz first and then return MDL_E_UNSUPPORTED, so that without a device the call came back with that
memset's HIP error.  The bf16 and split backwards and the forwards refused it up front already."""
import ctypes
import math

import pytest

from madeleine_amd import _native

OK, E_ARG, E_ALIGN, E_UNSUP = 0, -1, -2, -3
MAX_HEADS = 8

_RAW = ctypes.create_string_buffer(4096)
_P0 = (ctypes.addressof(_RAW) + 15) & ~15


def P(i):
    """The i-th fake pointer: host memory, 16-byte aligned, never dereferenced before a launch."""
    return _P0 + 64 * i


T0, H0 = 5, 2
_PAR_F = [("Wa", P(1)), ("ba", P(2)), ("Wb", P(3)), ("bb", P(4)), ("wc", P(5)), ("bc", P(6))]
_OUT_F = [("scores", P(7)), ("act_a", P(8)), ("act_b", P(9))]
_SHAPE = [("T", T0), ("H", H0), ("p_drop", 0.1), ("seed", 7), ("keep_a", P(10)), ("keep_b", P(11))]
_END = [("ws", P(12)), ("stream", None)]
_TENSOR = [("E", P(0)), ("ldE", MAX_HEADS * 512)]      # strides wide enough for any head count: H = 3 is a fault of its own
_IMAGE = [("E", P(0)), ("e_rsb", MAX_HEADS * 2048), ("e_scale", P(13))]
_BWD_IN = [("Wa", P(1)), ("Wb", P(3)), ("wc", P(5)), ("act_a", P(8)), ("act_b", P(9)), ("d_scores", P(14)), ("dE", P(15))]
_GRADS = [("accumulate", 0), ("dWa", P(16)), ("dWb", P(17)), ("dba", P(18)), ("dbb", P(19)), ("dwc", P(20)), ("dbc", P(21))]
_POOL = [("scores", P(7)), ("stat_m", P(22)), ("stat_l", P(23)), ("d_pooled", P(24)), ("row_bag", P(25)), ("N", T0)]


class Fam:
    """args: (name, valid value) in the header's order.  required: NULL is refused.  optional: groups of pointers that may be NULL
    together.  pairs: both or neither.  aligned: 16-byte alignment is checked.  pool: 'must' (the entry point needs the pooling term),
    'may' (only when scores is given) or None.  phases: the largest mask, or None."""

    def __init__(self, args, required, optional, pairs, aligned, forward=False, pool=None, phases=None, terms=False):
        self.args, self.required, self.optional, self.pairs, self.aligned = args, required, optional, pairs, aligned
        self.forward, self.pool, self.phases, self.terms = forward, pool, phases, terms


_FWD_REQ = ["E", "Wa", "ba", "Wb", "bb", "wc", "bc", "scores", "ws"]
_FWD_AL = ["E", "Wa", "Wb", "wc", "act_a", "act_b", "ws"]
_BWD_REQ = ["E", "Wa", "Wb", "wc", "act_a", "act_b", "d_scores", "dE", "dWa", "dWb", "dba", "dbb", "dwc", "ws"]
_BWD_AL = ["E", "dE", "Wa", "Wb", "act_a", "act_b", "wc", "ws"]
_KEEP = ("keep_a", "keep_b")
_POOL_PTRS = ["scores", "stat_m", "stat_l", "d_pooled"]
FAMILIES = {
    "fwd": Fam(_TENSOR + _PAR_F + _OUT_F + _SHAPE + _END, _FWD_REQ, [("act_a", "act_b"), _KEEP], [("act_a", "act_b"), _KEEP], _FWD_AL,
               forward=True),
    "fwd_split": Fam(_IMAGE + _PAR_F + _OUT_F + _SHAPE + _END, _FWD_REQ + ["e_scale"], [("act_a", "act_b"), _KEEP],
                     [("act_a", "act_b"), _KEEP], _FWD_AL, forward=True),
    "bwd": Fam(_TENSOR + _BWD_IN + _GRADS + _SHAPE + _END, _BWD_REQ, [("dbc",), _KEEP], [_KEEP], _BWD_AL),
    "attnpool": Fam(_TENSOR + _BWD_IN + _GRADS + _SHAPE + _POOL + _END, _BWD_REQ + _POOL_PTRS, [("dbc",), _KEEP, ("row_bag",)], [_KEEP],
                    _BWD_AL, pool="must"),
    "attnpool_phases": Fam(_TENSOR + _BWD_IN + _GRADS + _SHAPE + _POOL + _END + [("phases", 3)], _BWD_REQ + _POOL_PTRS,
                           [("dbc",), _KEEP, ("row_bag",)], [_KEEP], _BWD_AL, pool="must", phases=3),
    "attnpool_split": Fam(_IMAGE + _BWD_IN + [("ldE", MAX_HEADS * 512)] + _GRADS + _SHAPE + _POOL + [("dE_absmax", P(26))] + _END +
                          [("phases", 3), ("terms", 3)], _BWD_REQ + ["e_scale"],
                          [("dbc",), _KEEP, ("row_bag",), ("dE_absmax",), ("scores",), tuple(_POOL_PTRS) + ("row_bag",)], [_KEEP], _BWD_AL,
                          pool="may", phases=15, terms=True),
}
ENTRIES = ([("mdl_abmil_gate_fwd" + s, "fwd") for s in ("", "_bf16")] + [("mdl_abmil_gate_fwd_split", "fwd_split")] +
           [("mdl_abmil_gate_bwd" + s, "bwd") for s in ("", "_bf16")] + [("mdl_abmil_attnpool_bwd" + s, "attnpool") for s in ("", "_bf16")] +
           [("mdl_abmil_attnpool_bwd_phases" + s, "attnpool_phases") for s in ("", "_bf16")] +
           [("mdl_abmil_attnpool_bwd_split", "attnpool_split")])
assert len(ENTRIES) == 10      # + mdl_abmil_gate_dropout_mask below: every launching entry point of the three gate files
IDS = [e[0] for e in ENTRIES]
BAD_H = dict(H=3)
HUGE_T = 1 << 40   # the widest grid of any engine and direction is above 2^31 - 1


@pytest.fixture(scope="module")
def lib():
    return _native.lib()


def _caller(lib, name, fam, min_faults):
    base = dict(fam.args)
    fn = getattr(lib, name)

    def call(**kw):
        assert set(kw) <= set(base), kw
        if min_faults > 1:
            assert len(kw) >= 2, kw
        elif set(kw) <= {"T"} and kw.get("T", T0) >= 0 and kw.get("T", T0) < HUGE_T:
            assert kw.get("T") == 0 and fam.forward, "a call without a fault would launch"
        return fn(*[kw.get(k, v) for k, v in fam.args])
    return base, call


def _stride_key(base):
    return "e_rsb" if "e_rsb" in base else "ldE"


@pytest.mark.parametrize("name,family", ENTRIES, ids=IDS)
def test_gate_argument_checks(lib, name, family):
    fam = FAMILIES[family]
    base, call = _caller(lib, name, fam, 1)
    pointers = [k for k, v in fam.args if isinstance(v, int) and v >= _P0]
    optional = {k for grp in fam.optional for k in grp}
    assert set(pointers) == set(fam.required) | optional, "every pointer is classified"
    assert set(fam.aligned) <= set(pointers)
    if fam.forward:
        assert call(T=0) == OK, "the valid empty call"
    # 1. pointers, pairs, the pooling term and ranges
    for k in fam.required:
        if fam.pool == "may" and k in _POOL_PTRS:
            continue
        assert call(**{k: None}) == E_ARG, (k, "required")
    for grp in fam.optional:
        null = {k: None for k in grp}
        assert call(**null, **BAD_H) == E_UNSUP, (grp, "may be NULL: the head count is looked at")
        if fam.forward:
            assert call(**null, T=0) == OK, (grp, "may be NULL")
    for a, b in fam.pairs:
        assert call(**{a: None}) == E_ARG and call(**{b: None}) == E_ARG, (a, b, "both or neither")
    if fam.pool:
        for k in _POOL_PTRS[1:]:
            assert call(**{k: None}) == E_ARG, (k, "the pooling term is incomplete")
        assert call(row_bag=None, N=0) == E_ARG and call(row_bag=None, N=-1) == E_ARG, "dense bags need N >= 1"
        assert call(row_bag=None, N=1, **BAD_H) == E_UNSUP and call(N=0, **BAD_H) == E_UNSUP, "N is not read with row_bag"
    if fam.pool == "may":
        assert call(scores=None, row_bag=None, N=0, **BAD_H) == E_UNSUP, "no pooling term: the rest of it is not looked at"
    if fam.phases:
        assert call(phases=0) == E_ARG and call(phases=fam.phases + 1) == E_ARG and call(phases=-1) == E_ARG
        for ph in range(1, fam.phases + 1):
            assert call(phases=ph, **BAD_H) == E_UNSUP, ph
    if fam.terms:
        assert call(terms=1) == E_ARG and call(terms=4) == E_ARG and call(terms=2, **BAD_H) == E_UNSUP
    assert call(T=-1) == E_ARG
    assert call(H=0) == E_ARG and call(H=MAX_HEADS + 1) == E_ARG and call(H=-2) == E_ARG
    assert call(p_drop=-0.1) == E_ARG and call(p_drop=1.0) == E_ARG and call(p_drop=math.nan) == E_ARG
    assert call(p_drop=0.0, **BAD_H) == E_UNSUP
    # 2. alignment: the pointers addressed in 16-byte units, and only they
    for k in pointers:
        if k in fam.aligned:
            assert call(**{k: base[k] + 4}) == E_ALIGN, (k, "offset by 4 bytes")
        else:
            assert call(**{k: base[k] + 4}, **BAD_H) == E_UNSUP, (k, "offset by 4 bytes: not checked, the head count is looked at")
            if fam.forward:
                assert call(**{k: base[k] + 4}, T=0) == OK, (k, "offset by 4 bytes: not checked")
    # 3. the head count
    for H in (3, 5, 6, 7):
        assert call(H=H) == E_UNSUP, H
    # 5. the grids
    assert call(T=HUGE_T) == E_UNSUP


@pytest.mark.parametrize("name,family", ENTRIES, ids=IDS)
def test_gate_check_order(lib, name, family):
    """One pair of faults per step of the order."""
    fam = FAMILIES[family]
    base, call = _caller(lib, name, fam, 2)
    sk = _stride_key(base)
    wide = {sk: 1 << 30}        # above every 32-bit limit, on every alignment
    bad = fam.aligned[0]
    off = {bad: base[bad] + 4}
    # 1 before 2, 3, 4 and 5
    for k in fam.required:
        if fam.pool == "may" and k in _POOL_PTRS:
            continue
        assert call(**{k: None}, **BAD_H) == E_ARG, (k, "NULL before the head count")
        assert call(**{k: None}, **wide) == E_ARG, (k, "NULL before the stride limit")
        assert call(**{k: None}, T=HUGE_T) == E_ARG, (k, "NULL before the grids")
        if k != bad:
            assert call(**{k: None}, **off) == E_ARG, (k, "NULL before misaligned")
        if fam.forward:
            assert call(**{k: None}, T=0) == E_ARG, (k, "NULL before the empty problem")
    for a, _b in fam.pairs:
        assert call(**{a: None}, **BAD_H) == E_ARG and call(**{a: None}, **off) == E_ARG
    for fault in (dict(T=-1), dict(H=0), dict(H=MAX_HEADS + 1), dict(p_drop=1.0), {sk: 512}, {sk: base[sk] + 1}):
        assert call(**fault, **off) == E_ARG, (fault, "range before misaligned")
        if "H" not in fault:
            assert call(**fault, **BAD_H) == E_ARG, (fault, "range before the head count")   # (b) for p_drop on a backward
        if sk not in fault:
            assert call(**fault, **wide) == E_ARG, (fault, "range before the stride limit")
    if fam.pool:
        assert call(stat_m=None, **BAD_H) == E_ARG and call(row_bag=None, N=0, **off) == E_ARG
    if fam.phases:
        assert call(phases=0, **BAD_H) == E_ARG and call(phases=fam.phases + 1, **off) == E_ARG
    if fam.terms:
        assert call(terms=4, **BAD_H) == E_ARG and call(terms=0, **off) == E_ARG
    # 2 before 3, 4 and 5
    for k in fam.aligned:
        o = {k: base[k] + 4}
        assert call(**o, **BAD_H) == E_ALIGN, (k, "misaligned before the head count")                # (b) on a backward
        assert call(**o, **wide) == E_ALIGN, (k, "misaligned before the stride limit")
        assert call(**o, T=HUGE_T) == E_ALIGN, (k, "misaligned before the grids")
        if fam.forward:
            assert call(**o, T=0) == E_ALIGN, (k, "misaligned before the empty problem")
    # 3 before 4 and 5
    assert call(T=HUGE_T, **BAD_H) == E_UNSUP and call(T=HUGE_T, **wide) == E_UNSUP
    if fam.forward:
        assert call(T=0, **BAD_H) == E_UNSUP, "the head count before the empty problem"                # (a)
        assert call(T=0, **wide) == E_UNSUP, "the stride limit before the empty problem"
        assert call(T=0, H=1) == OK and call(T=0, p_drop=0.0) == OK, "4: the empty problem is served"


def test_dropout_mask_checks(lib):
    """The mask export launches one elementwise kernel: no workspace, no alignment rule, no head-count rule."""
    args = [("keep", P(0)), ("T", T0), ("H", H0), ("which", 0), ("p_drop", 0.25), ("seed", 7), ("stream", None)]

    def call(**kw):
        assert kw and (kw.get("T", T0) <= 0 or not set(kw) <= {"T"}), "a call without a fault would launch"
        return lib.mdl_abmil_gate_dropout_mask(*[kw.get(k, v) for k, v in args])

    assert call(T=0) == OK
    assert call(keep=None) == E_ARG and call(keep=None, T=0) == E_ARG
    assert call(T=-1) == E_ARG and call(H=0) == E_ARG and call(H=MAX_HEADS + 1) == E_ARG
    assert call(which=2) == E_ARG and call(which=-1) == E_ARG and call(which=1, T=0) == OK
    assert call(p_drop=1.0) == E_ARG and call(p_drop=-0.5) == E_ARG and call(p_drop=math.nan) == E_ARG and call(p_drop=0.0, T=0) == OK
    assert call(H=3, T=0) == OK and call(keep=P(0) + 1, T=0) == OK
    assert call(H=0, T=0) == E_ARG and call(which=2, T=0) == E_ARG and call(p_drop=1.0, T=0) == E_ARG, "ranges before the empty problem"


# ---- the workspace layouts, restated ----
def _splits_for(T, tiles, slots=768):
    """Token splits of a dW-type contraction (csrc/gate_common.hpp splits_for)."""
    quantum = _native.switch_get("MADELEINE_SPLIT_TOKENS")
    s = min(max(-(-T // 4096), 1), 64)
    if quantum > 4096:
        fill, sq = -(-slots // tiles), -(-T // quantum)
        s = min(max(sq, min(s, fill)), 64)
    if s * tiles >= slots // 2:
        rounds = -(-s * tiles // slots)
        want = -(-rounds * slots // tiles)
        if want <= 192 and T // want >= 1024:
            s = want
    return s


def _fwd_bytes(T, H, w_elem, scale_bytes):
    """weight image [H][1024][512] | score partials [T][H][4] fp32 | scale floats | 64"""
    return H * 1024 * 512 * w_elem + T * H * 4 * 4 + scale_bytes + 64


def _bwd_bytes(T, H, S, wn_elem, dz_elem, pad, dz_rows, scale_bytes):
    """weight image | dz [T + pad][H][1024] | slabW [S][H][512][1024] fp32 | slabV [row blocks][H][4][512] fp32 | scale floats | 64"""
    return (H * 512 * 1024 * wn_elem + (T + pad) * H * 1024 * dz_elem + S * H * 512 * 1024 * 4 + -(-T // dz_rows) * H * 4 * 512 * 4 +
            scale_bytes + 64)


def _layouts(T, H):
    wide = T >= 16384 and _native.switch_get("MADELEINE_BF16_TN256") != 0   # the bf16 dW kernel on 256 x 256 tiles
    return {
        "mdl_abmil_gate_fwd_ws_bytes": _fwd_bytes(T, H, 4, 0),
        "mdl_abmil_gate_fwd_bf16_ws_bytes": _fwd_bytes(T, H, 2, 0),
        "mdl_abmil_gate_fwd_split_ws_bytes": _fwd_bytes(T, H, 4, 64),
        "mdl_abmil_gate_bwd_ws_bytes": _bwd_bytes(T, H, _splits_for(T, 16 * H), 0, 4, 16, 256, 0),
        "mdl_abmil_gate_bwd_bf16_ws_bytes": _bwd_bytes(T, H, _splits_for(T, 8 * H, 256) if wide else _splits_for(T, 16 * H, 512), 2, 2, 64, 256, 0),
        "mdl_abmil_gate_bwd_split_ws_bytes": _bwd_bytes(T, H, _splits_for(T, 8 * H, 256), 4, 4, 32, 256 if T >= 131072 else 64 if T >= 16384 else 16,
                                                        64),
    }


def test_ws_bytes_match_the_layouts(lib):
    for T in (0, 1, 4095, 4096, 16383, 16384, 131071, 131072, 300000):
        for H in (1, 4):
            for name, want in _layouts(T, H).items():
                assert getattr(lib, name)(T, H) == want, (name, T, H)
    for name in _layouts(1, 1):
        fn = getattr(lib, name)
        assert fn(-1, 1) == E_ARG and fn(5, 0) == E_ARG and fn(5, MAX_HEADS + 1) == E_ARG, name
