"""Row strides of the C ABI without a GPU: every entry point that takes a leading dimension or an image row stride refuses, before any
launch, a stride below the row width, a stride that breaks the documented alignment and a stride above the limit its 32-bit offsets
allow (include/madeleine_amd.h states each limit as rows * stride bytes + column bytes <= 2^31 - 1; the table below carries the same
rows / column terms).  Every call is an EMPTY problem (T = 0, rows = 0, M = 0 or n_bags = 0) on fake host pointers: a missing refusal
returns MDL_OK instead of launching a kernel on host memory (one exception, marked below: the narrow-output tile of mdl_split_gemm_nt).  Entry points that return MDL_OK on an empty problem without touching
their pointers (`empty_ok`) are also called with valid strides -- the padded ones, and the largest aligned stride within the limit --
so that a refusal is known to come from the stride and from nothing else in the argument list."""
import ctypes

import pytest

from madeleine_amd import _native

E_ARG, E_ALIGN, E_UNSUP = -1, -2, -3
LIM = 0x7FFFFFFF
HID = 512


@pytest.fixture(scope="module")
def lib():
    return _native.lib()


_RAW = ctypes.create_string_buffer(4096)
_P0 = (ctypes.addressof(_RAW) + 15) & ~15


def P(i):
    """The i-th fake pointer: host memory, 16-byte aligned, never dereferenced by a launcher."""
    return _P0 + 64 * i


class S:
    """One stride argument: row `width` and `align` in the argument's own unit (elements, or bytes for images), `elem` bytes per unit,
    the limit rows * stride * elem + col <= 2^31 - 1 (rows = None: no limit), and the codes for too narrow / misaligned."""

    def __init__(self, name, width, align, elem=1, rows=None, col=0, below=E_ARG, misaligned=E_ARG):
        self.name, self.width, self.align, self.elem, self.rows, self.col = name, width, align, elem, rows, col
        self.below, self.misaligned = below, misaligned

    def limit(self):
        return None if self.rows is None else (LIM - self.col) // (self.rows * self.elem)


GATE_W = ("Wa", "ba", "Wb", "bb", "wc", "bc")


def _gate_fwd(sfx, H):
    def args(s):
        return [P(0), s["ldE"]] + [P(1 + i) for i in range(6)] + [P(7), P(8), P(9), 0, H, 0.0, 1, None, None, P(10), None]
    return args


def _gate_bwd(H, pool, phases):
    def args(s):
        a = [P(0), s["ldE"], P(1), P(2), P(3), P(4), P(5), P(6), P(7), 0] + [P(8 + i) for i in range(6)] + [0, H, 0.0, 1, None, None]
        if pool:
            a += [P(14), P(15), P(16), P(17), None, 4]
        a += [P(18), None]
        if phases:
            a += [3]
        return a
    return args


def _gate_fwd_split(H):
    def args(s):
        return [P(0), s["e_rsb"], P(1)] + [P(2 + i) for i in range(6)] + [P(8), P(9), P(10), 0, H, 0.0, 1, None, None, P(11), None]
    return args


def _bwd_split(H):
    def args(s):
        return ([P(0), s["e_rsb"], P(1), P(2), P(3), P(4), P(5), P(6), P(7), P(8), s["ldE"], 0] + [P(9 + i) for i in range(6)] +
                [0, H, 0.0, 1, None, None, P(15), P(16), P(17), P(18), None, 4, None, P(19), None, 3, 3])
    return args


def _pool(kind, H, key="ldE"):
    """Argument lists of the pooling family on zero bags."""
    img = [P(20)] if key == "e_rsb" else []          # e_scale follows the stride of the image entry points
    def args(s):
        head = [P(0), s[key]] + img
        return {
            "fwd": head + [P(1), P(2), P(3), P(4), 0, 5, None, 5, H, P(5), None],
            "bwd": head + [P(1), P(2), P(3), P(4), P(5), P(6), 0, P(7), 0, 0, 5, None, 5, H, None],
            "dscores": head + [P(1), P(2), P(3), P(4), P(5), P(7), 0, 0, 5, None, 5, H, None],
            "wfwd": head + [P(1), P(2), P(3), P(4), 0, 5, None, 5, H, P(5), None],
            "wbwd": head + [P(1), P(5), P(6), 0, P(7), 0, 5, None, 5, H, None],
            "vfwd": head + [P(1), P(2), P(3), P(4), 0, 5, P(8), 3, H, P(5), None],
            "vbwd": head + [P(1), P(2), P(3), P(4), P(5), P(6), P(7), 0, 5, P(8), 3, H, None],
            "rfwd": head + [P(1), P(2), P(3), P(4), 0, P(8), P(9), 3, H, P(5), None],
            "rbwd": head + [P(1), P(2), P(3), P(4), P(5), P(6), P(7), 0, P(8), P(9), 3, H, None],
        }[kind]
    return args


def _lin_fwd(N, K):
    return lambda s: [P(0), s["ldx"], P(1), P(2), P(3), s["ldy"], 0, N, K, P(4), None]


def _lin_bwd(N, K, ldy="ldy"):
    return lambda s: [P(0), s["ldx"], P(1), P(2), s[ldy], P(3), s["lddx"], P(4), P(5), 0, N, K, P(6), None]


def _nt(N, K, group, M=0):
    def args(s):
        a = [P(0), s["a_rsb"], P(1), P(2), s["b_rsb"], P(3), P(4), s["ldc"], M, N, K, P(5)]
        a += [None, None, P(6), P(7), 3, None] if group else [0, None, None, None, None, 3, None]
        return a
    return args


def _entries():
    out = []

    def add(name, args, strides, empty_ok, tag=""):
        out.append(pytest.param(name, args, strides, empty_ok, id=name + tag))
    for H in (1, 4):
        W, t = H * HID, "-H%d" % H
        add("mdl_abmil_gate_fwd", _gate_fwd("", H), [S("ldE", W, 4, 4, 127, 48)], True, t)
        add("mdl_abmil_gate_fwd_bf16", _gate_fwd("_bf16", H), [S("ldE", W, 8, 2, 255, 112)], True, t)
        add("mdl_abmil_gate_fwd_split", _gate_fwd_split(H), [S("e_rsb", 4 * W, 16, 1, 256)], True, t)
        for sfx, st in (("", S("ldE", W, 4, 4, 15, 1020)), ("_bf16", S("ldE", W, 8, 2, 63, 496))):
            add("mdl_abmil_gate_bwd" + sfx, _gate_bwd(H, False, False), [st], False, t)
            add("mdl_abmil_attnpool_bwd" + sfx, _gate_bwd(H, True, False), [st], False, t)
            add("mdl_abmil_attnpool_bwd_phases" + sfx, _gate_bwd(H, True, True), [st], False, t)
        add("mdl_abmil_attnpool_bwd_split", _bwd_split(H), [S("e_rsb", 4 * W, 16, 1, 32), S("ldE", W, 4, 4, 1)], False, t)
        for sfx, elem in (("", 4), ("_bf16", 2)):     # one alignment rule for fp32 and bf16 E: a multiple of 4 elements, no upper limit
            st = [S("ldE", W, 4, elem)]
            for kind, fn in (("fwd", "pool_fwd"), ("bwd", "pool_bwd"), ("wfwd", "wpool_fwd"), ("wbwd", "wpool_bwd"), ("vfwd", "pool_view_fwd"),
                             ("vbwd", "pool_view_bwd"), ("rfwd", "pool_rview_fwd"), ("rbwd", "pool_rview_bwd")):
                add("mdl_abmil_%s%s" % (fn, sfx), _pool(kind, H), st, True, t)
        add("mdl_abmil_pool_fwd_img", _pool("fwd", H, "e_rsb"), [S("e_rsb", 4 * W, 16)], True, t)
        add("mdl_abmil_pool_dscores_img", _pool("dscores", H, "e_rsb"), [S("e_rsb", 4 * W, 16)], True, t)
    # fp32 Linears: the wide tile (N % 256 == 0) and the tall one (N % 256 == 128) have different limits on ldx
    add("mdl_linear_fwd", _lin_fwd(256, 96), [S("ldx", 96, 4, 4, 127, 48), S("ldy", 256, 4, 4, 3, 1020)], True, "-wide")
    add("mdl_linear_fwd", _lin_fwd(128, 256), [S("ldx", 256, 4, 4, 255, 48), S("ldy", 128, 4, 4, 3, 1020)], True, "-tall")
    for N, K, t in ((256, 96, "-wide"), (128, 256, "-tall")):
        add("mdl_linear_bwd", _lin_bwd(N, K), [S("ldx", K, 4, 4, 15, 4 * K), S("ldy", N, 4, 4, 127, 48), S("lddx", K, 4, 4, 3, 1020)], False, t)
    U = E_UNSUP   # the bf16 Linears report a stride that is no multiple of 8 as an unsupported geometry
    add("mdl_linear_fwd_bf16", _lin_fwd(256, 512), [S("ldx", 512, 8, 2, 255, 112, misaligned=U), S("ldy", 256, 8, 2, 7, 510, misaligned=U)], True)
    add("mdl_linear_bwd_bf16", _lin_bwd(256, 512, "lddy"),
        [S("ldx", 512, 8, 2, 63, 496, misaligned=U), S("lddy", 256, 8, 2, 255, 112, misaligned=U), S("lddx", 512, 8, 2, 7, 510, misaligned=U)], False)
    # split images
    add("mdl_split_image", lambda s: [P(0), s["ldx"], 0, 64, P(1), s["rsb"], 0, P(2), None], [S("ldx", 64, 4, 4), S("rsb", 256, 16)], False)
    add("mdl_split_image_rows", lambda s: [P(0), s["ldx"], 0, 64, P(1), s["rsb"], 0, P(2), None, None], [S("ldx", 64, 4, 4), S("rsb", 256, 16)],
        True)
    add("mdl_split_tile_absmax", lambda s: [P(0), s["ldx"], 0, 64, P(1), P(2), None], [S("ldx", 64, 4, 4)], True)
    nt = [S("a_rsb", 256, 16, 1, 256), S("b_rsb", 256, 16, 1, 256), S("ldc", 256, 4, 4, 1)]
    add("mdl_split_gemm_nt", _nt(256, 64, False), nt, True)
    add("mdl_split_gemm_nt_group_bias", _nt(256, 64, True), nt, True)
    # the narrow-output tile (N <= 128, M > 256, no row_gate, no group_bias) has limits of its own; the launcher picks it by M, so
    # this one entry is not an empty problem: every call made for it (empty_ok = False) is one the launcher refuses
    add("mdl_split_gemm_nt", _nt(128, 64, False, M=257), [S("a_rsb", 256, 16, 1, 512), S("b_rsb", 256, 16, 1, 128), S("ldc", 128, 4, 4, 1)],
        False, "-narrow")
    add("mdl_split_gemm_tn", lambda s: [P(0), s["a_rsb"], P(1), 64, P(2), s["b_rsb"], P(3), 128, P(4), 0, None, P(5), 3, None],
        [S("a_rsb", 256, 16, 1, 32), S("b_rsb", 512, 16, 1, 32)], False)
    return out


@pytest.mark.parametrize("name,args,strides,empty_ok", _entries())
def test_stride_refusals_before_any_launch(lib, name, args, strides, empty_ok):
    fn = getattr(lib, name)
    # every stride argument of a call gets a different pad, so that a check applied to the wrong argument shows
    good = {st.name: st.width + (i + 1) * st.align for i, st in enumerate(strides)}

    def call(**kw):
        return fn(*args(dict(good, **kw)))
    if empty_ok:
        assert call() == 0, "padded strides"
        assert call(**{st.name: st.width for st in strides}) == 0, "contiguous"
    for st in strides:
        assert call(**{st.name: st.width - st.align}) == st.below, (st.name, "below the row width")
        assert call(**{st.name: 0}) == st.below and call(**{st.name: -st.align}) == st.below, (st.name, "zero / negative")
        assert call(**{st.name: st.width + st.align // 2}) == st.misaligned, (st.name, "misaligned")
        lim = st.limit()
        if lim is None:
            if empty_ok:    # no 32-bit offset: a stride of 2^40 units is as good as any
                assert call(**{st.name: 1 << 40}) == 0, (st.name, "no upper limit")
            continue
        inside = lim // st.align * st.align
        assert st.rows * inside * st.elem + st.col <= LIM < st.rows * (inside + st.align) * st.elem + st.col
        assert call(**{st.name: inside + st.align}) == E_UNSUP, (st.name, "first aligned stride above the limit")
        assert call(**{st.name: 1 << 40}) == E_UNSUP and call(**{st.name: 1 << 62}) == E_UNSUP, (st.name, "far above the limit")
        if empty_ok:
            assert call(**{st.name: inside}) == 0, (st.name, "largest aligned stride within the limit")


def test_bf16_pooling_takes_strides_that_are_multiples_of_4(lib):
    """The pooling kernels load 4 bf16 per lane (8 bytes): ldE % 4 == 0 is the rule for them, while the bf16 gates, whose LDS-DMA moves
    16-byte granules, keep ldE % 8 == 0."""
    H, W = 1, HID
    assert lib.mdl_abmil_pool_fwd_bf16(*_pool("fwd", H)({"ldE": W + 4})) == 0
    assert lib.mdl_abmil_pool_bwd_bf16(*_pool("bwd", H)({"ldE": W + 4})) == 0
    assert lib.mdl_abmil_pool_fwd_bf16(*_pool("fwd", H)({"ldE": W + 2})) == E_ARG
    assert lib.mdl_abmil_gate_fwd_bf16(*_gate_fwd("_bf16", H)({"ldE": W + 4})) == E_ARG
    assert lib.mdl_abmil_gate_fwd_bf16(*_gate_fwd("_bf16", H)({"ldE": W + 8})) == 0
    assert lib.mdl_abmil_gate_bwd_bf16(*_gate_bwd(H, False, False)({"ldE": W + 4})) == E_ARG


def test_header_states_the_stride_rules():
    from madeleine_amd import _build
    with open(_build.HEADER) as f:
        header = f.read()
    assert "requires ldE == H*512" not in header            # the bf16 gate backward reads E in place, at any stride
    for text in ("127 * 4 ldE + 48 <= 2^31 - 1", "63 * 2 ldE + 496 <= 2^31 - 1", "256 a_rsb and 256 b_rsb <= 2^31 - 1", "512 a_rsb and 128 b_rsb on the narrow-output tile",
                 "of 4 on the pooling entry points"):
        assert text in header, text
