"""Argument checks of the 18 launching pooling entry points without a GPU (csrc/abmil_pool.hip): required pointers and ranges
(MDL_E_ARG), then alignment (MDL_E_ALIGN), then the empty problem (MDL_OK), then the grid limit (MDL_E_UNSUPPORTED) -- one order for
every bag kind (dense, packed, dense view, ragged views), element type (fp32, bf16, split image) and pooling (softmax, weighted).
Every call either is a zero-bag problem or is refused, on fake host pointers: nothing here reaches a launch."""
import ctypes

import pytest

from madeleine_amd import _native

OK, E_ARG, E_ALIGN, E_UNSUP = 0, -1, -2, -3
HID, H = 512, 4

_RAW = ctypes.create_string_buffer(4096)
_P0 = (ctypes.addressof(_RAW) + 15) & ~15


def P(i):
    """The i-th fake pointer: host memory, 16-byte aligned, never dereferenced before a launch."""
    return _P0 + 64 * i


# One argument list per family, in the header's order: (name, value of the valid zero-bag call).  Pointers are P(i); the packed
# families pass cu_seqlens and N != max_len, which only cu_seqlens makes valid.
_SRC = [("E", P(0)), ("ldE", H * HID + 4), ("scores", P(1))]
_IMG = [("E", P(0)), ("e_rsb", 4 * H * HID + 16), ("e_scale", P(20)), ("scores", P(1))]
_STATS = [("pooled", P(2)), ("stat_m", P(3)), ("stat_l", P(4))]
_BAGS = [("n_bags", 0), ("N", 7), ("cu_seqlens", P(10)), ("max_len", 5), ("H", H)]
_VIEW = [("n_bags", 0), ("N", 7), ("token_idx", P(11)), ("n_idx", 5), ("H", H)]
_RVIEW = [("n_bags", 0), ("perm", P(11)), ("vcu", P(10)), ("max_view_len", 5), ("H", H)]
_FWD_END = [("ws", P(5)), ("stream", None)]
_VIEW_GRADS = [("d_pooled", P(6)), ("dE", P(7)), ("d_scores", P(8))]


class Fam:
    """required: NULL is refused; optional: NULL is accepted; aligned: 16-byte alignment is checked; the scalar that bounds the tokens
    of a bag (`length`); ragged: two grid rows per bag."""

    def __init__(self, args, required, optional, aligned, length="max_len", ragged=False):
        self.args, self.required, self.optional, self.aligned, self.length, self.ragged = args, required, optional, aligned, length, ragged


_FWD_REQ, _BWD_REQ = ["E", "scores", "pooled", "stat_m", "stat_l", "ws"], ["E", "scores", "pooled", "stat_m", "stat_l", "d_pooled"]
_FWD_AL, _BWD_AL = ["E", "pooled", "ws"], ["E", "dE", "pooled", "d_pooled"]
FAMILIES = {
    "fwd": Fam(_SRC + _STATS + _BAGS + _FWD_END, _FWD_REQ, ["stream"], _FWD_AL),
    "fwd_img": Fam(_IMG + _STATS + _BAGS + _FWD_END, _FWD_REQ + ["e_scale"], ["stream"], _FWD_AL),
    "bwd": Fam(_SRC + _STATS + [("d_pooled", P(6)), ("dE", P(7)), ("accumulate", 0), ("d_scores", P(8)), ("accumulate_scores", 0)] + _BAGS +
               [("stream", None)], _BWD_REQ + ["d_scores"], ["dE", "stream"], _BWD_AL),
    "dscores_img": Fam(_IMG + _STATS + [("d_pooled", P(6)), ("d_scores", P(8)), ("accumulate_scores", 0)] + _BAGS + [("stream", None)],
                       _BWD_REQ + ["d_scores", "e_scale"], ["stream"], ["E", "pooled", "d_pooled"]),
    "wbwd": Fam(_SRC + [("d_pooled", P(6)), ("dE", P(7)), ("accumulate", 0), ("d_scores", P(8))] + _BAGS + [("stream", None)],
                ["E", "scores", "d_pooled", "d_scores"], ["dE", "stream"], ["E", "dE", "d_pooled"]),
    "vfwd": Fam(_SRC + _STATS + _VIEW + _FWD_END, _FWD_REQ + ["token_idx"], ["stream"], _FWD_AL, "n_idx"),
    "vbwd": Fam(_SRC + _STATS + _VIEW_GRADS + _VIEW + [("stream", None)], _BWD_REQ + ["token_idx"], ["dE", "d_scores", "stream"], _BWD_AL,
                "n_idx"),
    "rfwd": Fam(_SRC + _STATS + _RVIEW + _FWD_END, _FWD_REQ + ["perm", "vcu"], ["stream"], _FWD_AL, "max_view_len", True),
    "rbwd": Fam(_SRC + _STATS + _VIEW_GRADS + _RVIEW + [("stream", None)], _BWD_REQ + ["perm", "vcu"], ["dE", "d_scores", "stream"], _BWD_AL,
                "max_view_len", True),
}
ENTRIES = ([("mdl_abmil_pool_fwd" + s, "fwd") for s in ("", "_bf16")] + [("mdl_abmil_pool_fwd_img", "fwd_img")] +
           [("mdl_abmil_pool_bwd" + s, "bwd") for s in ("", "_bf16")] + [("mdl_abmil_pool_dscores_img", "dscores_img")] +
           [("mdl_abmil_wpool_fwd" + s, "fwd") for s in ("", "_bf16")] + [("mdl_abmil_wpool_bwd" + s, "wbwd") for s in ("", "_bf16")] +
           [("mdl_abmil_pool_%s%s" % (k, s), f) for k, f in (("view_fwd", "vfwd"), ("view_bwd", "vbwd"), ("rview_fwd", "rfwd"),
                                                               ("rview_bwd", "rbwd")) for s in ("", "_bf16")])
assert len(ENTRIES) == 18


@pytest.fixture(scope="module")
def lib():
    return _native.lib()


@pytest.mark.parametrize("name,family", ENTRIES, ids=[e[0] for e in ENTRIES])
def test_pool_argument_checks(lib, name, family):
    fam = FAMILIES[family]
    base = dict(fam.args)
    fn = getattr(lib, name)
    backward, view, image = "ws" not in base, family in ("vfwd", "vbwd"), "e_rsb" in base
    whole = "cu_seqlens" in base
    stride = "e_rsb" if image else "ldE"
    unit = 4 if image else 1             # e_rsb is in bytes, 4 per channel
    too_many = 32768 if fam.ragged else 65536
    pointers = [k for k, v in fam.args if isinstance(v, int) and v >= _P0]

    def call(**kw):
        assert set(kw) <= set(base), kw
        return fn(*[kw.get(k, v) for k, v in fam.args])

    assert call() == OK, "the valid zero-bag call"
    # 1. pointers
    assert set(pointers) - {"cu_seqlens"} == set(fam.required) | (set(fam.optional) - {"stream"}), "every pointer is classified"
    for k in fam.required:
        assert call(**{k: None}) == E_ARG, (k, "required")
    for k in fam.optional:
        assert call(**{k: None}) == OK, (k, "may be NULL")
    if family in ("vbwd", "rbwd"):
        assert call(dE=None, d_scores=None) == E_ARG, "a view backward with neither output"
    if whole:
        assert call(cu_seqlens=None) == E_ARG, "N != max_len without cu_seqlens"
        assert call(cu_seqlens=None, N=base["max_len"]) == OK, "dense bags"
    # 2. ranges
    assert call(n_bags=-1) == E_ARG
    assert call(**{fam.length: -1}) == E_ARG
    assert call(**{stride: unit * (H * HID - 4)}) == E_ARG and call(**{stride: unit * (H * HID + 2)}) == E_ARG
    assert call(**{stride: unit * H * HID}) == OK, "contiguous rows"
    if view:
        assert call(n_idx=base["N"] + 1) == E_ARG and call(n_idx=base["N"]) == OK
        assert call(N=-1, n_idx=0) == E_ARG
    if image:
        assert call(e_rsb=base["e_rsb"] + 4) == E_ARG and call(e_rsb=base["e_rsb"] + 12) == E_ARG, "e_rsb % 16"
    # 3. alignment: the pointers addressed in 16-byte units, and only they
    for k in pointers:
        assert call(**{k: base[k] + 4}) == (E_ALIGN if k in fam.aligned else OK), (k, "offset by 4 bytes")
    # 4. / 5. the empty problem, the grid limit
    assert call(n_bags=too_many) == E_UNSUP
    assert call(n_bags=1 << 40) == E_UNSUP
    assert call(**{"n_bags": too_many, fam.length: 0}) == (OK if backward else E_UNSUP), "a backward over zero tokens has nothing to do"
    # the order of the steps, one pair per step
    bad = fam.aligned[0]
    for k in fam.required:
        if k != bad:
            assert call(**{k: None, bad: base[bad] + 4}) == E_ARG, (k, "NULL before misaligned")
    assert call(**{"n_bags": -1, bad: base[bad] + 4}) == E_ARG, "range before misaligned"
    assert call(**{stride: unit * (H * HID + 2), bad: base[bad] + 4}) == E_ARG, "stride before misaligned"
    for k in fam.aligned:
        assert call(**{k: base[k] + 4, "n_bags": too_many}) == E_ALIGN, (k, "misaligned before the grid limit")
    assert call(**{bad: base[bad] + 4, "n_bags": too_many, fam.length: 0}) == E_ALIGN, "misaligned before the empty problem"
    if image:
        assert call(e_scale=None, E=base["E"] + 4) == E_ARG and call(e_rsb=base["e_rsb"] + 8, n_bags=too_many) == E_ARG


def test_ws_bytes_matches_the_layout(lib):
    """mdl_abmil_pool_ws_bytes: acc [rows][chunks][H*512] fp32, then m and l [rows][chunks][H] fp32 each rounded up to 16 bytes, + 64."""
    for rows, max_len, heads in ((0, 0, 1), (3, 137, 1), (3, 137, 4), (5, 1100, 2), (6, 128, 8), (1, 129, 1), (7, 1, 1)):
        mc = (max_len + 127) // 128
        st = (rows * mc * heads * 4 + 15) // 16 * 16
        assert lib.mdl_abmil_pool_ws_bytes(rows, max_len, heads) == rows * mc * heads * HID * 4 + 2 * st + 64
    assert lib.mdl_abmil_pool_ws_bytes(-1, 5, 1) == E_ARG and lib.mdl_abmil_pool_ws_bytes(1, -1, 1) == E_ARG
    assert lib.mdl_abmil_pool_ws_bytes(1, 5, 0) == E_ARG and lib.mdl_abmil_pool_ws_bytes(1, 5, 9) == E_ARG
