"""Host side of the patch contributions (X1-X2, include/madeleine_amd_explain.h): the fourth header and its binding, every refusal in
its stated order from the loaded library, the argument checks of the wrappers and of MADELEINE.slide_directions, and the fp64 reference
(tests/_contrib_ref.py) on a two-token case worked by hand.  No GPU."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from madeleine_amd import _build, _native
from tests import _contrib_ref as ref

P, I32, I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
FAKE = 1 << 20          # a 16-byte aligned address nothing dereferences: every refusal below comes before the first launch
OK = 0
ARG, UNSUP, ALIGN = (_native._DEFINES[k] for k in ("MDL_E_ARG", "MDL_E_UNSUPPORTED", "MDL_E_ALIGN"))
NAMES = {"mdl_attn_contrib", "mdl_contrib_stats_ws_bytes", "mdl_contrib_stats"}
VIEW_NAMES = {"mdl_heat_ws_bytes", "mdl_heat_render", "mdl_heat_render_marked"}
STATS_NAMES = {"mdl_boot_weights", "mdl_boot_class_ws_bytes", "mdl_boot_class_counts", "mdl_boot_surv_counts"}


# ---- header and ABI ------------------------------------------------------------------------------------------------------------------
def test_the_fourth_header_parses_and_is_bound_beside_the_other_three():
    with open(_build.EXPLAIN_HEADER) as f:
        sigs, defines = _native._parse_header(f.read())
    assert sigs == _native.EXPLAIN_SIGNATURES and set(sigs) == NAMES and defines == _native.EXPLAIN_DEFINES
    assert sigs["mdl_attn_contrib"] == (I32, [P, I64, I32, P, I64, P, I64, I32, I32, I32, P, P, I64, P])
    assert sigs["mdl_contrib_stats_ws_bytes"] == (I64, [I64, I64, I32])
    assert sigs["mdl_contrib_stats"] == (I32, [P, I64, P, I64, I64, I32, P, P, P])
    assert defines == {"MDL_CONTRIB_MAX_C": 8, "MDL_CONTRIB_E_F32": 0, "MDL_CONTRIB_E_BF16": 1, "MDL_CONTRIB_ROWS": 1024,
                       "MDL_CONTRIB_SUM": 0, "MDL_CONTRIB_POS": 1, "MDL_CONTRIB_NEG": 2, "MDL_CONTRIB_ABSMAX": 3}
    lib = _native.lib()
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)                          # exported by the built library
        assert fn.restype is res and fn.argtypes == args, name
    # disjoint from the other three tables, whose sets are what they were
    others = set(_native.SIGNATURES) | set(_native.VIEW_SIGNATURES) | set(_native.STATS_SIGNATURES)
    assert not NAMES & others
    assert set(_native.VIEW_SIGNATURES) == VIEW_NAMES and set(_native.STATS_SIGNATURES) == STATS_NAMES
    assert not set(defines) & (set(_native._DEFINES) | set(_native.VIEW_DEFINES) | set(_native.STATS_DEFINES))
    assert _native.ABI_VERSION == 26 and lib.mdl_abi_version() == 26
    assert all(h in _build._deps() for h in (_build.EXPLAIN_HEADER, _build.HEADER, _build.VIEW_HEADER, _build.STATS_HEADER))


def test_a_header_that_repeats_a_name_is_refused():
    with open(_build.EXPLAIN_HEADER) as f:
        text = f.read()
    sigs, _ = _native._parse_header(text.replace("mdl_contrib_stats(", "mdl_boot_weights("))
    assert set(sigs) & set(_native.STATS_SIGNATURES)     # what the import-time check of _native looks for


def test_the_python_surface_is_exported():
    import madeleine_amd
    from madeleine_amd import functional as F
    for name in ("attn_contrib", "contrib_stats"):
        assert name in madeleine_amd.__all__ and getattr(madeleine_amd, name) is getattr(F, name)
    assert F.CONTRIB_MAX_C == 8 and F.CONTRIB_ROWS == 1024 and F.CONTRIB_STATS == ("sum", "pos", "neg", "absmax")
    for name in ("contributions", "contribution_maps"):
        assert callable(getattr(madeleine_amd.DeviceSlideStore, name))
    for name in ("slide_directions", "explain_packed"):
        assert callable(getattr(madeleine_amd.MADELEINE, name))


def test_workspace_query():
    ws = _native.lib().mdl_contrib_stats_ws_bytes
    for T, R, C in ((0, 1, 1), (5000, 3, 8), (1024, 1, 3), (1 << 20, 48, 5)):
        need = 4 * R + 4 * R + 4 * (R + 1) + 16 * C * (T // 1024 + R)
        assert need <= ws(T, R, C) <= need + 16 * 4 and ws(T, R, C) % 16 == 0
    assert ws(-1, 1, 1) == ARG and ws(1, -1, 1) == ARG and ws(1, 1, 0) == ARG
    assert ws(1, 1, 9) == UNSUP and ws(1 << 31, 1, 1) == UNSUP and ws(1, 1 << 31, 1) == UNSUP and ws((1 << 31) - 1, (1 << 31) - 1, 1) == UNSUP
    assert ws(-1, 1, 9) == ARG                           # (1) before (2)


# ---- refusals before any launch ------------------------------------------------------------------------------------------------------
def _contrib(T=10, H=4, W=512, C=3, ldE=None, ldA=None, ldO=None, e_dtype=0, null=(), misalign=None):
    ptr = {k: FAKE for k in ("E", "attn", "U", "per_head", "total")}
    for k in ([null] if isinstance(null, str) else null):
        ptr[k] = None
    if misalign:
        ptr[misalign[0]] += misalign[1]
    return _native.lib().mdl_attn_contrib(ptr["E"], H * W if ldE is None else ldE, e_dtype, ptr["attn"], H if ldA is None else ldA,
                                          ptr["U"], T, H, W, C, ptr["per_head"], ptr["total"], C if ldO is None else ldO, None)


def _stats(T=10, R=2, C=3, ld=None, null=(), misalign=None):
    ptr = {k: FAKE for k in ("contrib", "cu", "stats", "ws")}
    for k in ([null] if isinstance(null, str) else null):
        ptr[k] = None
    if misalign:
        ptr[misalign[0]] += misalign[1]
    return _native.lib().mdl_contrib_stats(ptr["contrib"], C if ld is None else ld, ptr["cu"], T, R, C, ptr["stats"], ptr["ws"], None)


@pytest.mark.parametrize("call,null", [(_contrib, n) for n in ("E", "attn", "U", "total")] +
                         [(_stats, n) for n in ("contrib", "cu", "stats", "ws")])
def test_null_pointers_are_refused(call, null):
    assert call(null=null) == ARG


@pytest.mark.parametrize("call,kw,code", [
    (_contrib, dict(T=-1), ARG), (_contrib, dict(H=0), ARG), (_contrib, dict(H=-4), ARG), (_contrib, dict(W=0), ARG),
    (_contrib, dict(C=0), ARG), (_contrib, dict(C=-1), ARG),
    (_contrib, dict(ldE=2047), ARG), (_contrib, dict(ldA=3), ARG), (_contrib, dict(ldO=2), ARG),
    (_contrib, dict(e_dtype=2), ARG), (_contrib, dict(e_dtype=-1), ARG),
    (_contrib, dict(H=3), UNSUP), (_contrib, dict(H=16), UNSUP), (_contrib, dict(W=256), UNSUP), (_contrib, dict(W=1024), UNSUP),
    (_contrib, dict(C=9), UNSUP), (_contrib, dict(T=1 << 31), UNSUP),
    (_contrib, dict(misalign=("E", 8)), ALIGN), (_contrib, dict(misalign=("E", 4)), ALIGN), (_contrib, dict(misalign=("U", 8)), ALIGN),
    (_contrib, dict(ldE=2050), ALIGN), (_contrib, dict(ldE=2052, e_dtype=1), ALIGN),
    (_contrib, dict(misalign=("attn", 2)), ALIGN), (_contrib, dict(misalign=("total", 1)), ALIGN),
    (_contrib, dict(misalign=("per_head", 2)), ALIGN),
    (_stats, dict(T=-1), ARG), (_stats, dict(R=-1), ARG), (_stats, dict(C=0), ARG), (_stats, dict(ld=2), ARG),
    (_stats, dict(C=9), UNSUP), (_stats, dict(T=1 << 31), UNSUP), (_stats, dict(R=1 << 31), UNSUP),
    (_stats, dict(T=(1 << 31) - 1, R=(1 << 31) - 1), UNSUP),                       # the chunk grid
    (_stats, dict(R=1 << 27, C=8), UNSUP),                                          # the grid R 4 C
    (_stats, dict(misalign=("cu", 4)), ALIGN), (_stats, dict(misalign=("ws", 8)), ALIGN), (_stats, dict(misalign=("contrib", 2)), ALIGN),
    (_stats, dict(misalign=("stats", 1)), ALIGN),
])
def test_refusals_before_any_launch(call, kw, code):
    assert call(**kw) == code


def test_accepted_strides_and_the_empty_calls():
    """ldE a multiple of 4 (fp32) / 8 (bf16) passes the checks; T == 0 and R == 0 return MDL_OK with nothing launched (there is no
    device here), and T == 0 takes NULL for E, attn and total, per_head NULL in every call."""
    assert _contrib(T=0, ldE=2052) == OK and _contrib(T=0, ldE=2056, e_dtype=1) == OK and _contrib(T=0, ldA=7, ldO=4) == OK
    assert _contrib(T=0, null=("E", "attn", "total", "per_head")) == OK
    assert _contrib(T=0, null="U") == ARG
    for H in (1, 2, 4, 8):
        for C in range(1, 9):
            assert _contrib(T=0, H=H, C=C) == OK
    assert _stats(R=0) == OK and _stats(T=0) == OK and _stats(T=0, null="contrib") == OK and _stats(T=0, R=0) == OK


def test_the_order_of_the_refusals():
    """(1) MDL_E_ARG before (2) MDL_E_UNSUPPORTED before (3) MDL_E_ALIGN."""
    assert _contrib(H=3, ldA=2) == ARG and _contrib(C=9, ldO=8) == ARG and _contrib(W=256, e_dtype=5) == ARG
    assert _contrib(T=1 << 31, null="total") == ARG and _contrib(H=16, C=0) == ARG
    assert _contrib(H=3, misalign=("E", 8)) == UNSUP and _contrib(C=9, ldE=2050) == UNSUP and _contrib(T=1 << 31, misalign=("U", 4)) == UNSUP
    assert _contrib(misalign=("E", 8), T=0) == ALIGN      # the alignment is checked before the empty call returns
    assert _stats(C=9, ld=2) == ARG and _stats(T=1 << 31, null="cu") == ARG
    assert _stats(C=9, misalign=("ws", 8)) == UNSUP and _stats(R=1 << 31, misalign=("cu", 4)) == UNSUP
    assert _stats(R=0, misalign=("cu", 4)) == ALIGN


def test_wrapper_refusals_on_cpu_tensors():
    from madeleine_amd import functional as F
    E, a, U = torch.zeros(3, 2048), torch.zeros(3, 4), torch.zeros(2, 2048)
    with pytest.raises(RuntimeError, match="ROCm device"):
        F.attn_contrib(E, a, U)
    with pytest.raises(RuntimeError, match="float32 or bfloat16"):
        F.attn_contrib(E.double(), a, U)
    with pytest.raises(RuntimeError, match="ROCm device"):
        F.contrib_stats(torch.zeros(3, 2), torch.zeros(2, dtype=torch.int64))


# ---- slide_directions ----------------------------------------------------------------------------------------------------------------
def _cpu_model(H=4):
    from madeleine_amd import MADELEINE
    cfg = SimpleNamespace(MODALITIES=["HE"], wsi_encoder="abmil", patch_embedding_dim=32, wsi_encoder_hidden_dim=512,
                          activation="softmax", n_heads=H)
    return MADELEINE(cfg)


def test_slide_directions_shape_and_width_errors():
    m = _cpu_model()
    for W, b, C in ((torch.zeros(512), None, 1), (torch.zeros(3, 512), torch.zeros(3), 3), (torch.zeros(2, 512), 0.5, 2),
                    (np.zeros((5, 3, 512), np.float32)[2], np.zeros((5, 3), np.float32)[2], 3),       # a slice of fit_logistic's
                    (torch.zeros(6, 512)[4], None, 1)):                                                # a slice of fit_cox's
        rows, bias = m.decision_rows(W, b)
        assert rows.shape == (C, 512) and bias.shape == (C,) and rows.dtype == bias.dtype == torch.float32
    with pytest.raises(ValueError, match="512"):
        m.slide_directions(torch.zeros(3, 2048))
    with pytest.raises(ValueError, match="512"):
        m.slide_directions(torch.zeros(128))
    with pytest.raises(ValueError, match=r"\[d\] or \[C, d\]"):
        m.slide_directions(torch.zeros(2, 3, 512))
    with pytest.raises(ValueError, match=r"\[d\] or \[C, d\]"):
        m.slide_directions(torch.zeros(0, 512))
    with pytest.raises(ValueError, match="one value per row"):
        m.slide_directions(torch.zeros(3, 512), torch.zeros(2))
    with pytest.raises(ValueError, match=r"U \[C, 2048\]"):
        m.explain_packed((torch.zeros(5, 32), None, [5]), "cpu", torch.zeros(3, 512))
    with pytest.raises(ValueError, match="at least one bag"):
        m.explain_packed((torch.zeros(5, 32), None, [4]), "cpu", torch.zeros(3, 2048))


# ---- the reference by hand -----------------------------------------------------------------------------------------------------------
def test_the_reference_on_two_tokens_by_hand():
    """H = 2 heads of W = 2 channels, C = 2 columns.  Head-major E rows: [h0e0 h0e1 | h1e0 h1e1]."""
    E = np.array([[1.0, 2.0, 3.0, 4.0], [-1.0, 0.5, 2.0, -2.0]])
    attn = np.array([[0.25, 0.5], [0.75, 0.5]])
    U = np.array([[1.0, 1.0, 1.0, 1.0], [2.0, -1.0, 0.0, 3.0]])
    per_head, total, abs_head, abs_total = ref.contrib(E, attn, U, 2)
    # token 0: head 0 dots (3, 0), head 1 dots (7, 12); token 1: head 0 (-0.5, -2.5), head 1 (0, -6)
    assert per_head.tolist() == [[[0.75, 0.0], [3.5, 6.0]], [[-0.375, -1.875], [0.0, -3.0]]]
    assert total.tolist() == [[4.25, 6.0], [-0.375, -4.875]]
    assert abs_head[0].tolist() == [[0.75, 1.0], [3.5, 6.0]] and abs_total[1].tolist() == [1.125 + 2.0, 1.875 + 3.0]
    pi, ti = ref.contrib_int(E * 2, attn, U, 2)
    assert np.array_equal(pi, 2 * per_head) and np.array_equal(ti, 2 * total)
    # the statistics of the two tokens as one bag, an empty bag and token 1 alone
    st, scale = ref.stats(total, [0, 2, 2, 1])
    assert st[0].tolist() == [[3.875, 1.125], [4.25, 6.0], [-0.375, -4.875], [4.25, 6.0]] and scale[0].tolist() == [4.625, 10.875]
    assert not st[1].any() and not st[2].any()
    st1, _ = ref.stats(total, [1, 2])
    assert st1[0].tolist() == [[-0.375, -4.875], [0.0, 0.0], [-0.375, -4.875], [0.375, 4.875]]
    nan = ref.stats(np.array([[1.0], [-np.nan], [-2.0]]), [0, 3])[0][0, :, 0]
    assert np.isnan(nan[0]) and nan[1] == 1.0 and np.isnan(nan[2]) and np.isnan(nan[3])
    # the identity: pooled = sum_t a E in the reference's channel order e H + h, one Linear on top, one linear probe on top of that
    rng = np.random.default_rng(0)
    Pw, bP, Wp, bp = rng.normal(size=(3, 4)), rng.normal(size=3), rng.normal(size=(2, 3)), rng.normal(size=2)
    E_ref = np.stack([E[:, [0, 2]], E[:, [1, 3]]], 1).reshape(2, 4)                  # [t, e, h] flattened: j = e H + h
    assert np.array_equal(ref.head_major(E_ref, 2), E)
    pooled = (E_ref.reshape(2, 2, 2) * attn[:, None, :]).sum(0).reshape(4)
    z = Wp @ (Pw @ pooled + bP) + bp
    Ud, const = ref.directions(Pw, bP, Wp, bp, 2)
    assert np.allclose(ref.contrib(E, attn, Ud, 2)[1].sum(0) + const, z, rtol=1e-12, atol=1e-12)
    # the signed map values and the top patches
    v = ref.signed_values(np.array([[2.0, 0.0], [-4.0, 0.0], [1.0, 0.0]], np.float32), [0, 2, 3, 3])
    assert v.tolist() == [[0.75, 0.5], [0.0, 0.5], [1.0, 0.5]]
    pi_, pv, ni, nv = ref.topk(np.array([[1.0], [3.0], [1.0], [-2.0]], np.float32), [0, 4, 4], 3)
    assert pi_[0, 0].tolist() == [1, 0, 2] and ni[0, 0].tolist() == [3, 0, 2] and pv[0, 0].tolist() == [3.0, 1.0, 1.0]
    assert pi_[1, 0].tolist() == [-1] * 3 and np.isneginf(pv[1]).all() and np.isposinf(nv[1]).all()
