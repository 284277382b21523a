"""Host side of the device heatmaps (V1, include/madeleine_amd_view.h): the second header and its binding, the refusals that come before
any launch, the integer taps, the colour maps, the PNG writer, set_coords on a CPU-built store, and the numpy reference itself on a
case computed by hand.  No GPU."""
import ctypes
import struct
import zlib

import numpy as np
import pytest
import torch

from madeleine_amd import _build, _native
from tests import _heat_ref as HR

P, I32, I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
FAKE = 1 << 20          # a 16-byte aligned address nothing dereferences: every refusal below comes before the first launch
ARG, UNSUP, ALIGN = (_native._DEFINES[k] for k in ("MDL_E_ARG", "MDL_E_UNSUPPORTED", "MDL_E_ALIGN"))


# ---- header and ABI ------------------------------------------------------------------------------------------------------------------
def test_the_second_header_parses_and_is_bound_beside_the_first():
    with open(_build.VIEW_HEADER) as f:
        sigs, defines = _native._parse_header(f.read())
    assert sigs == _native.VIEW_SIGNATURES and set(sigs) == {"mdl_heat_ws_bytes", "mdl_heat_render", "mdl_heat_render_marked"}
    assert sigs["mdl_heat_ws_bytes"] == (I64, [I64, I64, I32])
    assert sigs["mdl_heat_render"] == (I32, [P, P, P, I64, I64, I64, I32, P, P, I64, I32, P, I32, P, P, I32, P, P, P, P, P])
    assert sigs["mdl_heat_render_marked"] == (I32, sigs["mdl_heat_render"][1][:-1] + [P, P])      # the same arguments + marks_host
    assert defines["MDL_HEAT_MARKS"] == 5
    assert defines["MDL_HEAT_REC"] == 6 and defines["MDL_HEAT_MAX_R"] == 32 and defines["MDL_HEAT_MAX_SIDE"] == 32768
    assert defines["MDL_HEAT_TAP_SUM"] == 4096
    assert "MDL_ABI_VERSION" not in defines
    lib = _native.lib()
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)                          # exported by the built library
        assert fn.restype is res and fn.argtypes == args, name
        assert name not in _native.SIGNATURES            # the main header's table is the main header's set
    assert _native.ABI_VERSION == 26 and lib.mdl_abi_version() == 26
    assert _build.VIEW_HEADER in _build._deps()


def test_the_python_surface_is_exported():
    import madeleine_amd
    from madeleine_amd import functional as MF, heatmap
    for name in ("heatmap", "render_heatmaps", "gaussian_taps", "colormap", "save_png"):
        assert name in madeleine_amd.__all__ and getattr(madeleine_amd, name) is not None
    assert madeleine_amd.render_heatmaps is heatmap.render and madeleine_amd.heatmap is heatmap
    assert callable(MF.heat_render) and callable(madeleine_amd.DeviceSlideStore.heatmaps)


def test_workspace_query():
    ws = _native.lib().mdl_heat_ws_bytes
    for Pn, R, C in ((1000, 3, 4), (1, 1, 1), (30000, 7, 5)):
        assert ws(Pn, R, C) >= 24 * Pn * C + 4 * (R + 1) and ws(Pn, R, C) % 16 == 0
    assert ws(0, 0, 1) >= 0
    assert ws(-1, 1, 1) == ARG and ws(1, -1, 1) == ARG and ws(1, 1, 0) == ARG
    assert ws(1 << 31, 1, 1) == UNSUP and ws(1 << 30, 1, 2) == UNSUP and ws(10, 1, 65536) == UNSUP


# ---- refusals before any launch ------------------------------------------------------------------------------------------------------
def _call(T=100, R=2, C=3, ld=3, Pn=40, ds=4, taps=(4096,), alpha=255, recs=None, null=None, misalign=None, base=None):
    """mdl_heat_render with addresses that nothing may dereference for every device pointer, host arrays for bag_host and taps_host."""
    recs = [[16, 0, 0, 5, 4, 0], [16, 0, 0, 5, 4, 20]] if recs is None else recs
    rec = (ctypes.c_int64 * (6 * max(1, len(recs))))(*[v for r in recs for v in r])
    tp = (ctypes.c_int32 * len(taps))(*taps)
    ptr = {k: FAKE for k in ("xy", "cu", "values", "bag", "lut", "level", "covered", "rgba", "ws")}
    ptr["bag_host"], ptr["taps_host"] = ctypes.addressof(rec), ctypes.addressof(tp)
    if null:
        ptr[null] = None
    if misalign:
        ptr[misalign[0]] += misalign[1]
    return _native.lib().mdl_heat_render(ptr["xy"], ptr["cu"], ptr["values"], ld, T, R, C, ptr["bag_host"], ptr["bag"], Pn, ds,
                                         ptr["taps_host"], len(taps) // 2, ptr["lut"], base, alpha, ptr["level"], ptr["covered"],
                                         ptr["rgba"], ptr["ws"], None)


@pytest.mark.parametrize("null", ["xy", "cu", "values", "bag_host", "bag", "taps_host", "lut", "level", "covered", "rgba", "ws"])
def test_null_pointers_are_refused(null):
    assert _call(null=null) == ARG


@pytest.mark.parametrize("kw, code", [
    (dict(taps=(0,) * 33 + (4096,) + (0,) * 33), UNSUP),            # r = 33
    (dict(taps=(1024, 2048, 1023)), ARG),                           # asymmetric, sum 4095
    (dict(taps=(1024, 2047, 1024)), ARG),                           # symmetric, sum 4095
    (dict(taps=(2048, 0, 2048)), ARG),                              # centre 0
    (dict(taps=(-1, 4098, -1)), ARG),                               # negative taps
    (dict(ds=0), ARG), (dict(ds=-3), ARG),
    (dict(ld=2), ARG),                                              # ld < C
    (dict(alpha=256), ARG), (dict(alpha=-1), ARG),
    (dict(T=-1), ARG), (dict(R=-1), ARG), (dict(C=0), ARG), (dict(Pn=-1), ARG),
    (dict(T=1 << 24), UNSUP), (dict(C=65536, ld=65536), UNSUP),
    (dict(recs=[[16, 0, 0, 32769, 1, 0]], R=1, Pn=40000), UNSUP),   # W > 32768
    (dict(recs=[[16, 0, 0, 1, 32769, 0]], R=1, Pn=40000), UNSUP),   # H > 32768
    (dict(recs=[[0, 0, 0, 5, 4, 0]], R=1), ARG),                    # ps < 1
    (dict(recs=[[16, 0, 0, 0, 4, 0]], R=1), ARG),                   # W < 1
    (dict(recs=[[16, 0, 0, 5, 4, 21]], R=1), ARG),                  # the canvas leaves the planes
    (dict(recs=[[16, 0, 0, 5, 4, -1]], R=1), ARG),
    (dict(recs=[[(1 << 24) + 1, 0, 0, 5, 4, 0]], R=1), UNSUP),
    (dict(recs=[[16, 1 << 31, 0, 5, 4, 0]], R=1), UNSUP),
    (dict(misalign=("ws", 8)), ALIGN), (dict(misalign=("cu", 4)), ALIGN), (dict(misalign=("xy", 2)), ALIGN),
    (dict(misalign=("values", 2)), ALIGN), (dict(misalign=("rgba", 2)), ALIGN), (dict(misalign=("level", 1)), ALIGN),
])
def test_refusals_before_any_launch(kw, code):
    assert _call(**kw) == code


def test_the_order_of_the_refusals_and_the_empty_call():
    assert _call(ds=0, taps=(0,) * 33 + (4096,) + (0,) * 33) == ARG                     # (1) before (2)
    assert _call(T=1 << 24, taps=(1, 1, 1)) == UNSUP                                    # (2) before (3)
    assert _call(taps=(1, 1, 1), recs=[[0, 0, 0, 5, 4, 0]], R=1) == ARG                 # (3) ...
    assert _call(recs=[[16, 0, 0, 5, 4, 0], [16, 0, 0, 40000, 4, 0]]) == UNSUP          # (4) the records in bag order
    assert _call(recs=[[16, 0, 0, 40000, 4, 0]], R=1, misalign=("ws", 8)) == UNSUP      # (4) before (5)
    assert _call(R=0, recs=[]) == 0 and _call(Pn=0, R=0, recs=[]) == 0                  # nothing to do: MDL_OK, nothing launched


def test_the_marked_call_needs_every_event_and_refuses_like_the_plain_one():
    call = _native.lib().mdl_heat_render_marked
    rec = (ctypes.c_int64 * 6)(16, 0, 0, 5, 4, 0)
    tp = (ctypes.c_int32 * 1)(4096)
    args = [FAKE, FAKE, FAKE, 3, 100, 1, 3, ctypes.addressof(rec), FAKE, 40, 4, ctypes.addressof(tp), 0, FAKE, None, 255, FAKE, FAKE, FAKE,
            FAKE]
    assert call(*args, None, None) == ARG
    marks = (ctypes.c_void_p * 5)(FAKE, FAKE, None, FAKE, FAKE)
    assert call(*args, ctypes.addressof(marks), None) == ARG
    marks = (ctypes.c_void_p * 5)(*[FAKE] * 5)
    args[3] = 2                                                                         # ld < C: the plain call's refusal, nothing recorded
    assert call(*args, ctypes.addressof(marks), None) == ARG
    args[3], args[12] = 3, 33
    assert call(*args, ctypes.addressof(marks), None) == UNSUP


def test_the_declared_bytes_of_the_tile_passes_follow_the_kernels():
    """memset 8; rows: read acc 8, write S1 and N1 16; columns: read acc, S1, N1 24, write level 2, covered 1, rgba 4."""
    from madeleine_amd import functional as MF
    assert MF.HEAT_PLANE_BYTES == {"clear": 8, "blur_rows": 24, "blur_cols_colour": 31} and sum(MF.HEAT_PLANE_BYTES.values()) == 63
    assert MF.HEAT_STAGES == ("clear", "accumulate", "blur_rows", "blur_cols_colour") and MF.HEAT_MARKS == len(MF.HEAT_STAGES) + 1


def test_wrapper_refusals_on_cpu_tensors():
    from madeleine_amd import functional as MF, heatmap
    xy, cu, v = torch.zeros(4, 2, dtype=torch.int32), torch.tensor([0, 4]), torch.zeros(4, 1)
    rec, taps, lut = torch.tensor([[16, 0, 0, 2, 2, 0]]), heatmap.gaussian_taps(0), heatmap.colormap("gray")
    with pytest.raises(RuntimeError, match="ROCm device"):
        MF.heat_render(xy, cu, v, rec, 4, 16, taps, lut)
    with pytest.raises(RuntimeError, match=r"xy \[T, 2\]"):
        MF.heat_render(torch.zeros(4, 3, dtype=torch.int32), cu, v, rec, 4, 16, taps, lut)


# ---- gaussian_taps -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.25, 0.5, 1.0, 2.0, 3.3, 7.0, 10.7, 40.0])
@pytest.mark.parametrize("radius", [None, 1, 5, 32])
def test_gaussian_taps(sigma, radius):
    from madeleine_amd.heatmap import gaussian_taps
    t = gaussian_taps(sigma, radius)
    assert t.dtype == torch.int32 and t.device.type == "cpu"
    r = min(32, int(np.ceil(3 * sigma))) if radius is None else radius
    t = t.tolist()
    assert len(t) == 2 * r + 1 and sum(t) == 4096 and t == t[::-1] and min(t) >= 0 and t[r] > 0
    half = t[r:]
    assert all(a >= b for a, b in zip(half, half[1:]))                                 # monotone from the centre
    w = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    err = np.array(t) - 4096 * w / w.sum()              # a tap is its floor or its floor + 1; the centre may also take the odd last unit
    err[r] = err[r] / 2
    assert err.min() > -1.0 - 1e-9 and err.max() < 1.0 + 1e-9


def test_gaussian_taps_edges():
    from madeleine_amd.heatmap import gaussian_taps
    assert gaussian_taps(0).tolist() == [4096] and gaussian_taps(0.0, 2).tolist() == [0, 0, 4096, 0, 0]
    assert gaussian_taps(5.0, 0).tolist() == [4096]
    assert gaussian_taps(2.0).numel() == 13 and gaussian_taps(100.0).numel() == 65      # radius follows sigma, capped at 32
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            gaussian_taps(bad)
    with pytest.raises(ValueError):
        gaussian_taps(1.0, 33)


# ---- colormap and save_png -----------------------------------------------------------------------------------------------------------
def test_colormap():
    from madeleine_amd.heatmap import colormap
    ends = {"jet": ([0, 0, 128, 255], [128, 0, 0, 255]), "coolwarm": ([59, 76, 192, 255], [180, 4, 38, 255]),
            "gray": ([0, 0, 0, 255], [255, 255, 255, 255])}
    for name, (lo, hi) in ends.items():
        lut = colormap(name)
        assert lut.dtype == torch.uint8 and tuple(lut.shape) == (256, 4) and lut.device.type == "cpu"
        assert lut[0].tolist() == lo and lut[255].tolist() == hi and bool((lut[:, 3] == 255).all())
    assert colormap("gray")[:, 0].tolist() == list(range(256))
    assert colormap("jet")[128, 1] == 255 and colormap("coolwarm")[127, :3].min() >= 215      # green plateau | the white middle
    own = torch.arange(1024, dtype=torch.int64).remainder(256).to(torch.uint8).view(256, 4)
    assert colormap(own) is own
    with pytest.raises(ValueError):
        colormap("viridis")
    with pytest.raises(ValueError):
        colormap(torch.zeros(256, 3, dtype=torch.uint8))


def _decode_png(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF
        chunks.append((tag, body))
        pos += 12 + n
    assert [c[0] for c in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    W, H, depth, kind, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, filt, lace) == (8, 0, 0, 0)
    ch = {6: 4, 2: 3}[kind]
    raw = np.frombuffer(zlib.decompress(chunks[1][1]), dtype=np.uint8).reshape(H, 1 + W * ch)
    assert not raw[:, 0].any()                                                         # filter type 0 on every row
    return raw[:, 1:].reshape(H, W, ch)


@pytest.mark.parametrize("shape", [(5, 7, 4), (1, 1, 4), (3, 2, 3)])
def test_save_png_round_trip(tmp_path, shape):
    from madeleine_amd.heatmap import save_png
    img = torch.from_numpy(np.random.default_rng(0).integers(0, 256, shape, dtype=np.uint8))
    save_png(str(tmp_path / "a.png"), img)
    assert np.array_equal(_decode_png((tmp_path / "a.png").read_bytes()), img.numpy())
    with pytest.raises(ValueError):
        save_png(str(tmp_path / "b.png"), img.float())


# ---- set_coords on a CPU-built store -------------------------------------------------------------------------------------------------
def _store(**kw):
    from madeleine_amd import DeviceSlideStore
    bags = [[torch.ones(3, 8), None], [torch.ones(2, 8), torch.ones(4, 8)]]
    return DeviceSlideStore(bags, ["a", "b"], ["HE", "ER"], "cpu", **kw)


def _coords():
    return [[np.array([[0, 0], [256, 0], [0, 512]]), None], [np.array([[10, 20], [30, 40]]), np.arange(8).reshape(4, 2) * 100]]


def test_set_coords_holds_them_in_store_row_order():
    st = _store(coords=_coords(), patch_size=256)
    assert st.coords.dtype == torch.int32 and tuple(st.coords.shape) == (9, 2)
    assert st.coords.tolist() == [[0, 0], [256, 0], [0, 512], [10, 20], [30, 40], [0, 100], [200, 300], [400, 500], [600, 700]]
    assert st.coord_extents.tolist() == [[0, 0, 256, 512], [10, 20, 30, 40], [0, 100, 600, 700]]
    assert st.patch_sizes.tolist() == [256, 256, 256]
    assert st.coords_of([1, 0], 0).tolist() == [[10, 20], [30, 40], [0, 0], [256, 0], [0, 512]]
    assert st.coords_of(None, 1).tolist() == [[0, 100], [200, 300], [400, 500], [600, 700]]
    st2 = _store()
    assert st2.coords is None
    with pytest.raises(RuntimeError, match="no coordinates"):
        st2.coords_of([0], 0)
    st2.set_coords([[c.astype(np.float32) if c is not None else None for c in case] for case in _coords()], [[224, None], [256, 512]])
    assert torch.equal(st2.coords, st.coords) and st2.patch_sizes.tolist() == [224, 256, 512]
    st2.set_coords([[np.array([[0, 0], [0, 0], [(1 << 24) - 1, 5]]), None], _coords()[1]], 1)      # the last value of the range
    assert int(st2.coords.max()) == (1 << 24) - 1


@pytest.mark.parametrize("edit, match", [
    (lambda c: c[0].__setitem__(0, np.zeros((4, 2), dtype=np.int64)), "has 3 rows"),                   # wrong length
    (lambda c: c[1].__setitem__(1, np.zeros((4, 3), dtype=np.int64)), "has 4 rows"),                   # not [n, 2]
    (lambda c: c[1].__setitem__(0, np.array([[10, 20], [-1, 40]])), "span -1"),                         # negative
    (lambda c: c[1].__setitem__(0, np.array([[10, 20], [1 << 24, 40]])), "2\\^24"),                    # >= 2^24
    (lambda c: c[1].__setitem__(0, np.array([[10, 20.5], [30, 40]])), "not integral"),                 # non-integral
    (lambda c: c[1].__setitem__(0, np.array([[10, np.nan], [30, 40]])), "not integral"),
    (lambda c: c[1].__setitem__(1, None), "present and has no coordinates"),                           # present bag without
    (lambda c: c[0].__setitem__(1, np.zeros((2, 2), dtype=np.int64)), "absent"),                       # absent bag with
    (lambda c: c.pop(), "coordinate lists"),
])
def test_set_coords_refusals(edit, match):
    c = _coords()
    edit(c)
    with pytest.raises(ValueError, match=match):
        _store(coords=c, patch_size=256)


def test_set_coords_patch_size_refusals_and_cpu_heatmaps():
    for bad in (0, -4, 2.5, (1 << 24) + 1, None, [[256, None]]):
        with pytest.raises(ValueError):
            _store(coords=_coords(), patch_size=bad)
    with pytest.raises(ValueError, match="without coords"):
        _store(patch_size=256)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _store(coords=_coords(), patch_size=256).heatmaps(None)


def test_from_dataset_reads_the_coords_beside_the_features(tmp_path):
    """from_dataset(coords=True) reads `coords` from the h5 files SlideDataset reads `features` from: the same names, the split suffix
    included, so that a change of one path rule without the other fails here."""
    import pandas as pd
    from madeleine_amd import DeviceSlideStore, h5io
    from madeleine_amd.data import SlideDataset
    rng = np.random.default_rng(0)
    files = {("c0", "HE", ""): 5, ("c0", "ER", ""): 3, ("c1", "HE", "_val"): 4}
    feats = {k: rng.standard_normal((n, 8)).astype(np.float32) for k, n in files.items()}
    xy = {k: rng.integers(0, 1 << 24, (n, 2)) for k, n in files.items()}
    xy[("c0", "HE", "")][0] = [(1 << 24) - 1, 0]
    for (cid, m, special), a in feats.items():
        h5io.write_datasets(str(tmp_path / ("%s_%s%s.h5" % (cid, m, special))), {"features": a, "coords": xy[(cid, m, special)].astype(np.float32)})
    df = pd.DataFrame({"slide_id": ["c0", "c1"], "HE": [1, 1], "ER": [1, 0], "split": ["train", "val"]})
    ds = SlideDataset("toy", None, str(tmp_path), ["HE", "ER"], embedding_size=8, sample=-1, train=True, dataframe=df)
    st = DeviceSlideStore.from_dataset(ds, "cpu", coords=True, patch_size=224)
    want = np.concatenate([xy[("c0", "HE", "")], xy[("c0", "ER", "")], xy[("c1", "HE", "_val")]])
    assert st.coords.dtype == torch.int32 and np.array_equal(st.coords.numpy(), want)
    assert torch.equal(st.rows, torch.from_numpy(np.concatenate([feats[k] for k in files])))
    assert st.patch_sizes.tolist() == [224, 224, 224] and st.coords_of([1], 0).tolist() == xy[("c1", "HE", "_val")].tolist()
    with pytest.raises(ValueError, match="patch_size"):
        DeviceSlideStore.from_dataset(ds, "cpu", coords=True)
    assert DeviceSlideStore.from_dataset(ds, "cpu").coords is None


def test_plan_canvases():
    from madeleine_amd.heatmap import plan_canvases
    ext = [[512, 256, 1024, 768], [0, 0, -1, -1], [100, 50, 100, 50]]
    assert plan_canvases(ext, 256, 64).tolist() == [[256, 0, 0, 20, 16], [256, 0, 0, 1, 1], [256, 0, 0, 6, 5]]
    assert plan_canvases(ext, [256, 256, 7], 64, crop=True).tolist() == [[256, 512, 256, 12, 12], [256, 0, 0, 1, 1], [7, 100, 50, 1, 1]]
    with pytest.raises(ValueError):
        plan_canvases(ext, 256, 0)


# ---- the reference on a case computed by hand ----------------------------------------------------------------------------------------
def test_the_reference_on_three_patches_by_hand():
    """W = 4, H = 3, ds = 2, ps = 4, origin 0.  A at (0, 0), v = 1: q = 65535 on x 0..1, y 0..1.  B at (2, 0), v = 0.5: 32767.5 rounds to
    the even 32768, on x 1..2, y 0..1.  C at (5, 3), v = 0: q = 0 on x 2..4 -> 2..3, y 1..3 -> 1..2 (clipped)."""
    xy = [[0, 0], [2, 0], [5, 3]]
    gray = np.stack([np.arange(256)] * 3 + [np.full(256, 255)], 1).astype(np.uint8)
    res = HR.render_bag(xy, [[1.0], [0.5], [0.0]], 4, 0, 0, 4, 3, 2, [4096], gray, 255)
    assert res["S"].tolist() == [[[65535, 98303, 32768, 0], [65535, 98303, 32768, 0], [0, 0, 0, 0]]]
    assert res["N"].tolist() == [[[1, 2, 1, 0], [1, 2, 2, 1], [0, 0, 1, 1]]]
    assert res["level"].tolist() == [[[65535, 49151, 32768, 0], [65535, 49151, 16384, 0], [0, 0, 0, 0]]]
    assert res["covered"].tolist() == [[[1, 1, 1, 0], [1, 1, 1, 1], [0, 0, 1, 1]]]
    idx = [[255, 191, 128, -1], [255, 191, 64, 0], [-1, -1, 0, 0]]      # (m * 255 + 32767) // 65535; -1: uncovered
    want = [[[0, 0, 0, 0] if i < 0 else [i, i, i, 255] for i in row] for row in idx]
    assert res["rgba"].tolist() == [want]
    # alpha 128 over a constant thumbnail of 100: a = (255 * 128 + 127) // 255 = 128, rgb = (i * 128 + 100 * 127 + 127) // 255
    base = np.full((3, 4, 3), 100, dtype=np.uint8)
    mixed = HR.render_bag(xy, [[1.0], [0.5], [0.0]], 4, 0, 0, 4, 3, 2, [4096], gray, 128, base)["rgba"]
    want = [[[100, 100, 100, 255] if i < 0 else [(i * 128 + 12827) // 255] * 3 + [255] for i in row] for row in idx]
    assert mixed.tolist() == [want] and want[0][0] == [178, 178, 178, 255] and want[1][3] == [50, 50, 50, 255]
    # a [1, 2, 1] / 4 blur of one row: S = [65535, 0, 0], N = [1, 1, 1] -> S1 = [2048, 1024, 0] * 65535, N1 = [3072, 4096, 3072]
    row = HR.render_bag([[0, 0], [1, 0], [2, 0]], [[1.0], [0.0], [0.0]], 1, 0, 0, 3, 1, 1, [1024, 2048, 1024], gray, 255)
    assert row["level"].tolist() == [[[(2048 * 65535) // 3072, (1024 * 65535) // 4096, 0]]] == [[[43690, 16383, 0]]]


def test_the_reference_quantiser():
    v = np.array([np.nan, -np.inf, -1.0, -0.0, 0.0, 1e-30, 0.5 / 65535, 1.5 / 65535, 2.5 / 65535, 0.5, 1.0 - 2 ** -24, 1.0, 7.0, np.inf],
                 dtype=np.float32)
    q, keep = HR.quantise(v)
    assert keep.tolist() == [False] + [True] * 13
    assert q[1:].tolist() == [0, 0, 0, 0, 0, int(np.rint(np.float32(0.5 / 65535) * np.float32(65535))),
                              int(np.rint(np.float32(1.5 / 65535) * np.float32(65535))),
                              int(np.rint(np.float32(2.5 / 65535) * np.float32(65535))), 32768, 65535, 65535, 65535, 65535]
