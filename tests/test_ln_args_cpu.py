"""Argument checks of the 11 launching LayerNorm-GELU-Dropout entry points without a GPU (csrc/preattn_act.hip, ln_check): required
pointers and ranges (MDL_E_ARG), then the width (MDL_E_UNSUPPORTED), then alignment (MDL_E_ALIGN), then the empty problem -- one order
for plain, grouped, split and split-grouped calls, fp32 and bf16.  All pointers are fake host addresses, so no call here may reach a
launch: only the four forwards that return MDL_OK for rows == 0 before any launch are ever called without a fault (the split forward
writes its scale and every backward zeroes its sums even then); every other entry is called with a fault, and "is not refused" is read
off a later step's code (a NULL optional pointer with a bad width gives MDL_E_UNSUPPORTED, not MDL_E_ARG).  For those entries nothing
follows the alignment step, so that a pointer is NOT alignment-checked is asserted on the four forwards only.
The one single-fault code that differs from the library before ln_check: rows == 0 with a bad width is MDL_E_UNSUPPORTED on the four
non-split forwards (it was MDL_OK); DESIGN.md section 3.3 lists it with the pairs of faults whose code changed."""
import ctypes

import pytest

from madeleine_amd import _native

OK, E_ARG, E_ALIGN, E_UNSUP = 0, -1, -2, -3

_RAW = ctypes.create_string_buffer(4096)
_P0 = (ctypes.addressof(_RAW) + 15) & ~15


def P(i):
    """The i-th fake pointer: host memory, 16-byte aligned, never dereferenced before a launch."""
    return _P0 + 64 * i


_PAR = [("x", P(0)), ("bias", P(1)), ("gamma", P(2)), ("beta", P(3))]
_SHAPE_F = [("rows", 5), ("W", 512), ("eps", 1e-5), ("p_drop", 0.1), ("seed", 7), ("keep", P(9))]
_SHAPE_B = [("rows", 5), ("W", 512), ("p_drop", 0.1), ("seed", 7), ("keep", P(9))]
_STATS = [("mean", P(5)), ("rstd", P(6))]
_GROUPS = [("cu_groups", P(10)), ("G", 3)]
_IMG_END = [("row_mul", P(11)), ("rstd_max", P(12))]
_BWD_SPLIT = (_PAR + _STATS + [("dy", P(4)), ("dy_absmax", P(13)), ("dx_img", P(7)), ("dx_scale", P(8)), ("dgamma", P(14)), ("dbeta", P(15)),
                               ("dbias", P(16))] + _SHAPE_B + _IMG_END)


class Fam:
    """args: (name, valid value) in the header's order; required: NULL is refused; optional: NULL is accepted; aligned: 16-byte
    alignment is checked; wide: 2048 columns are supported."""

    def __init__(self, args, required, optional, aligned, wide=True):
        self.args, self.required, self.optional, self.aligned, self.wide = args, required, optional, aligned, wide


_BWD_REQ = ["x", "gamma", "beta", "mean", "rstd", "dy", "dgamma", "dbeta", "ws"]
FAMILIES = {
    "fwd": Fam(_PAR + [("y", P(4))] + _STATS + _SHAPE_F + [("stream", None)],
               ["x", "gamma", "beta", "y", "mean", "rstd"], ["bias", "keep"], ["x", "bias", "gamma", "beta", "y"]),
    "bwd": Fam(_PAR + _STATS + [("dy", P(4)), ("dx", P(7)), ("dgamma", P(14)), ("dbeta", P(15)), ("dbias", P(16))] + _SHAPE_B +
               [("ws", P(17)), ("stream", None)], _BWD_REQ + ["dx"], ["bias", "dbias", "keep"], ["x", "bias", "gamma", "beta", "dy", "dx"]),
    "fwd_groups": Fam(_PAR + [("y", P(4))] + _STATS + _SHAPE_F + _GROUPS + [("stream", None)],
                      ["x", "bias", "gamma", "beta", "y", "mean", "rstd", "cu_groups"], ["keep"], ["x", "bias", "gamma", "beta", "y"], False),
    "bwd_groups": Fam(_PAR + _STATS + [("dy", P(4)), ("dx", P(7)), ("dgamma", P(14)), ("dbeta", P(15)), ("dgroup_bias", P(16))] + _SHAPE_B +
                      _GROUPS + [("ws", P(17)), ("stream", None)], _BWD_REQ + ["dx", "bias", "cu_groups", "dgroup_bias"], ["keep"],
                      ["x", "bias", "gamma", "beta", "dy", "dx"], False),
    "fwd_split": Fam(_PAR + [("y", P(4)), ("img", P(7)), ("scale", P(8))] + _STATS + _SHAPE_F + _IMG_END + [("stream", None)],
                     ["x", "gamma", "beta", "img", "scale", "mean", "rstd"], ["bias", "y", "keep", "row_mul", "rstd_max"],
                     ["x", "bias", "gamma", "beta", "y", "img"]),
    "bwd_split": Fam(_BWD_SPLIT + [("ws", P(17)), ("stream", None)], _BWD_REQ + ["dx_img", "dx_scale"],
                     ["bias", "dy_absmax", "dbias", "keep", "row_mul", "rstd_max"], ["x", "bias", "gamma", "beta", "dy", "dx_img", "ws"]),
    "bwd_split_groups": Fam(_BWD_SPLIT + _GROUPS + [("dgroup_bias", P(18)), ("ws", P(17)), ("stream", None)],
                            _BWD_REQ + ["dx_img", "dx_scale", "cu_groups", "dgroup_bias"],
                            ["bias", "dy_absmax", "dbias", "keep", "row_mul", "rstd_max"], ["x", "bias", "gamma", "beta", "dy", "dx_img", "ws"]),
}
ENTRIES = ([("mdl_ln_gelu_drop_%s%s" % (k, s), k) for k in ("fwd", "bwd") for s in ("", "_bf16")] +
           [("mdl_ln_gelu_drop_%s_groups%s" % (k, s), k + "_groups") for k in ("fwd", "bwd") for s in ("", "_bf16")] +
           [("mdl_ln_gelu_drop_" + k, k) for k in ("fwd_split", "bwd_split", "bwd_split_groups")])
assert len(ENTRIES) == 11
RETURNS_EMPTY = ("fwd", "fwd_groups")      # MDL_OK for rows == 0 before any launch


@pytest.fixture(scope="module")
def lib():
    return _native.lib()


@pytest.mark.parametrize("name,family", ENTRIES, ids=[e[0] for e in ENTRIES])
def test_ln_argument_checks(lib, name, family):
    fam = FAMILIES[family]
    base = dict(fam.args)
    fn = getattr(lib, name)
    forward, grouped = "eps" in base, "G" in base
    pointers = [k for k, v in fam.args if isinstance(v, int) and v >= _P0]
    bad_w = dict(W=300)

    def call(**kw):
        assert set(kw) <= set(base), kw
        faultless = set(kw) <= {"rows"} and kw.get("rows", 5) >= 0
        assert not faultless or (kw.get("rows") == 0 and family in RETURNS_EMPTY), "a call without a fault would launch"
        return fn(*[kw.get(k, v) for k, v in fam.args])

    assert set(pointers) == set(fam.required) | set(fam.optional), "every pointer is classified"
    assert set(fam.aligned) <= set(pointers)
    if family in RETURNS_EMPTY:
        assert call(rows=0) == OK, "the valid empty call"
    # 1. pointers and ranges
    for k in fam.required:
        assert call(**{k: None}) == E_ARG, (k, "required")
    for k in fam.optional:
        assert call(**{k: None}, **bad_w) == E_UNSUP, (k, "may be NULL: the width is looked at")
        if family in RETURNS_EMPTY:
            assert call(**{k: None}, rows=0) == OK, (k, "may be NULL")
    assert call(rows=-1) == E_ARG
    assert call(p_drop=-0.1) == E_ARG and call(p_drop=1.0) == E_ARG
    if forward:
        assert call(eps=0.0) == E_ARG
    if grouped:
        assert call(G=0) == E_ARG and call(G=2049) == E_ARG
    # 2. the width
    assert call(W=300) == E_UNSUP and call(W=8192) == E_UNSUP
    if not fam.wide:
        assert call(W=2048) == E_UNSUP, "grouped rows are at most 1024 wide"
    # 3. alignment: the pointers addressed in 16-byte units, and only they
    for k in pointers:
        if k in fam.aligned:
            assert call(**{k: base[k] + 4}) == E_ALIGN, (k, "offset by 4 bytes")
        elif family in RETURNS_EMPTY:
            assert call(**{k: base[k] + 4}, rows=0) == OK, (k, "offset by 4 bytes: not checked")


@pytest.mark.parametrize("name,family", ENTRIES, ids=[e[0] for e in ENTRIES])
def test_ln_check_order(lib, name, family):
    """One pair of faults per step of the order, and the empty problem last."""
    fam = FAMILIES[family]
    base = dict(fam.args)
    fn = getattr(lib, name)

    def call(**kw):
        assert len(kw) >= 2 and set(kw) <= set(base), kw
        return fn(*[kw.get(k, v) for k, v in fam.args])

    bad = fam.aligned[0]
    off = {bad: base[bad] + 4}
    for k in fam.required:
        assert call(**{k: None}, W=300) == E_ARG, (k, "NULL before the width")
        if k != bad:
            assert call(**{k: None}, **off) == E_ARG, (k, "NULL before misaligned")
    assert call(rows=-1, W=300) == E_ARG and call(rows=-1, **off) == E_ARG, "range before the width and before misaligned"
    assert call(p_drop=1.0, W=8192) == E_ARG
    if "G" in base:
        assert call(G=0, W=300) == E_ARG and call(G=2049, **off) == E_ARG
        assert call(cu_groups=None, W=2048) == E_ARG, "NULL before the width, the grouped limit included"
    if not fam.wide:
        assert call(W=2048, **off) == E_UNSUP and call(W=2048, rows=0) == E_UNSUP
    for k in fam.aligned:
        assert call(W=300, **{k: base[k] + 4}) == E_UNSUP, (k, "the width before misaligned")
        assert call(rows=0, **{k: base[k] + 4}) == E_ALIGN, (k, "misaligned before the empty problem")
    assert call(rows=0, W=300) == E_UNSUP and call(rows=0, W=8192) == E_UNSUP, "the width before the empty problem"


def _ws_bytes(rows, W, G=0):
    """[slots][dgamma W | dbeta W | dbias W] fp32 + 128: a slot per workgroup of the widest launch -- row blocks of 4 / 4 / 2 / 1 / 1 rows
    at 256 / 512 / 1024 / 2048 / 4096 columns, at most 2048 and at least one; with groups, no fewer than G times the workgroups per group."""
    rpb = {256: 4, 512: 4, 1024: 2, 2048: 1, 4096: 1}[W]
    slots = min(max(-(-rows // rpb), 1), 2048)
    if G:
        slots = max(slots, G * max(1, min(2048 // G, -(-(rows // G) // rpb))))
    return slots * 3 * W * 4 + 128


def test_ws_bytes_match_the_layout(lib):
    plain, groups = lib.mdl_ln_gelu_drop_bwd_ws_bytes, lib.mdl_ln_gelu_drop_bwd_groups_ws_bytes
    for rows, W in ((0, 512), (1, 256), (7, 512), (8197, 256), (4099, 2048), (5, 2048), (3000, 1024), (9000, 4096)):
        assert plain(rows, W) == _ws_bytes(rows, W), (rows, W)
    for rows, W, G in ((0, 512, 3), (19, 512, 3), (10, 512, 7), (5, 2048, 4), (4099, 2048, 3), (100000, 1024, 2048), (9000, 256, 1),
                       (70000, 4096, 5)):
        assert groups(rows, W, G) == _ws_bytes(rows, W, G), (rows, W, G)
    assert _ws_bytes(10, 512, 7) > _ws_bytes(10, 512), "G * nbx above the un-grouped slot count"
    assert plain(-1, 512) == E_ARG and groups(-1, 512, 3) == E_ARG
    assert groups(5, 512, 0) == E_ARG and groups(5, 512, 2049) == E_ARG
    assert plain(5, 300) == E_UNSUP and plain(5, 8192) == E_UNSUP and groups(5, 300, 3) == E_UNSUP
