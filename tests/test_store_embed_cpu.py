"""The cohort-embedding route of the slide store without a GPU: the mdl_bag_mean entry points (declared, bound, exported, argument
refusals before any launch), the ABI revision, the single-stain pack plan on a store built on the CPU, and the refusal to embed there."""
import ctypes

import pytest
import torch

from madeleine_amd import _build, _native
from madeleine_amd import functional as MF
from madeleine_amd.store import DeviceSlideStore

E_ARG, E_ALIGN, E_UNSUP = -1, -2, -3
MODS = ["HE", "HER2", "PGR"]


@pytest.fixture(scope="module")
def lib():
    return _native.lib()


def test_entry_points_are_declared_bound_and_exported(lib):
    with open(_build.HEADER) as f:
        header = f.read()
    assert " * S5 -- " in header
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    want = {"mdl_bag_mean_ws_bytes": (L, [L, I]),
            #                store dtype stride T_total off n_bags bag chunk_cu R n_chunks D out ws stream
            "mdl_bag_mean": (I, [P, I, L, L, P, L, P, P, L, L, I, P, P, P]),
            #                       store host dtype stride T_total T_dev off n_bags bag chunk_cu R n_chunks D out ws host_wgs stream
            "mdl_bag_mean_tiered": (I, [P, P, I, L, L, L, P, L, P, P, L, L, I, P, P, I, P])}
    handle = ctypes.CDLL(_native.lib_path())
    for name, (res, args) in want.items():
        assert name + "(" in header
        assert _native.SIGNATURES[name] == (res, args), name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
        assert hasattr(handle, name)
    assert callable(MF.bag_mean) and callable(MF.bag_mean_tiered)


def test_abi_version_is_still_26_and_the_chunk_is_parsed(lib):
    assert _native.ABI_VERSION == 26 and lib.mdl_abi_version() == 26
    d = _native._DEFINES
    assert d["MDL_BAG_MEAN_ROWS"] == MF.BAG_MEAN_ROWS >= 64 and d["MDL_BAG_MEAN_THREADS"] == 256 and d["MDL_BAG_MEAN_COLS"] == 8
    assert (58_000_000 // d["MDL_BAG_MEAN_ROWS"] + 1) * 512 * 4 < 128e6      # the partials of a 58 M-row cohort at D = 512


def test_workspace_query(lib):
    assert lib.mdl_bag_mean_ws_bytes(0, 8) == 0 and lib.mdl_bag_mean_ws_bytes(3, 512) == 3 * 512 * 4
    assert lib.mdl_bag_mean_ws_bytes(2 ** 31 - 1, 4096) == (2 ** 31 - 1) * 4096 * 4
    assert lib.mdl_bag_mean_ws_bytes(-1, 8) == E_ARG and lib.mdl_bag_mean_ws_bytes(1, 0) == E_ARG
    assert lib.mdl_bag_mean_ws_bytes(2 ** 31, 8) == E_UNSUP


def _good():
    raw = ctypes.create_string_buffer(1024)
    p = (ctypes.addressof(raw) + 15) & ~15          # host memory: a launch on it would fault, so every case below must refuse first
    return raw, p, dict(store=p, host=None, dtype=0, stride=8, T=4, T_dev=4, off=p + 64, n_bags=1, bag=p + 96, chunk=p + 256, R=2,
                        chunks=2, D=8, out=p + 16, ws=p + 320, wgs=0)


def _check_refusals(call, p):
    for name in ("off", "bag", "chunk", "out", "ws"):
        assert call(**{name: None}) == E_ARG, name
    assert call(R=-1) == E_ARG and call(chunks=-1) == E_ARG and call(D=0) == E_ARG and call(D=-1) == E_ARG
    assert call(dtype=3) == E_ARG and call(dtype=-1) == E_ARG
    assert call(T=-1) == E_ARG and call(n_bags=-1) == E_ARG and call(stride=7) == E_ARG
    assert call(out=p + 20) == E_ALIGN and call(out=p + 8) == E_ALIGN and call(store=p + 4) == E_ALIGN
    assert call(ws=p + 324) == E_ALIGN and call(ws=p + 328) == E_ALIGN
    assert call(off=p + 68) == E_ALIGN and call(bag=p + 98) == E_ALIGN and call(chunk=p + 260) == E_ALIGN
    # the misaligned vector case: with D and the stride multiples of the 16-byte access, a base that is not
    for dtype, D in ((0, 4), (1, 8), (2, 8)):
        assert call(dtype=dtype, D=D, stride=D, store=p + 8) == E_ALIGN
    assert call(chunks=2 ** 31) == E_UNSUP and call(R=2 ** 31) == E_UNSUP and call(R=2 ** 40, chunks=2 ** 34) == E_UNSUP
    # the order of the refusals: argument, then alignment, then geometry
    assert call(D=0, out=p + 8, R=2 ** 31) == E_ARG and call(ws=p + 324, R=2 ** 31) == E_ALIGN
    # nothing to reduce: no launch
    assert call(R=0) == 0 and call(chunks=0) == 0 and call(R=0, chunks=0) == 0
    assert call(R=0, out=p + 8) == E_ALIGN and call(R=0, ws=None) == E_ARG       # ... and the checks still hold


def test_mean_refuses_bad_arguments_before_any_launch(lib):
    raw, p, good = _good()

    def call(**kw):
        a = dict(good, **kw)
        return lib.mdl_bag_mean(a["store"], a["dtype"], a["stride"], a["T"], a["off"], a["n_bags"], a["bag"], a["chunk"], a["R"], a["chunks"],
                                a["D"], a["out"], a["ws"], None)
    assert call(store=None) == E_ARG
    _check_refusals(call, p)


def test_tiered_mean_refuses_bad_arguments_before_any_query_or_launch(lib):
    """store_host is NULL throughout (T_dev == T_total needs none): the runtime is never asked about a pointer and pageable memory never
    stands in for a host tier."""
    raw, p, good = _good()

    def call(**kw):
        a = dict(good, **kw)
        return lib.mdl_bag_mean_tiered(a["store"], a["host"], a["dtype"], a["stride"], a["T"], a["T_dev"], a["off"], a["n_bags"], a["bag"],
                                       a["chunk"], a["R"], a["chunks"], a["D"], a["out"], a["ws"], a["wgs"], None)
    _check_refusals(call, p)
    assert call(T_dev=-1) == E_ARG and call(T_dev=5) == E_ARG and call(wgs=-1) == E_ARG
    assert call(store=None) == E_ARG                                              # a tier with rows needs its base ...
    assert call(T_dev=3) == E_ARG and call(T_dev=0) == E_ARG                      # (rows in a host tier, and no host tier given)
    assert call(R=0, store=None, T=0, T_dev=0) == 0                               # ... an empty store needs no tier
    assert call(host=p + 516) == E_ALIGN                                          # a misaligned store_host, even with no row in it


def _bags():
    g = torch.Generator().manual_seed(0)
    r = lambda n: torch.randn(n, 6, generator=g)      # noqa: E731
    return [[r(5), None, r(3)], [r(2), r(7), None], [r(1), None, None], [r(4), r(4), r(9)]]


def _store(**kw):
    return DeviceSlideStore(_bags(), ["a", "b", "c", "d"], MODS, "cpu", **kw)


def test_the_plan_of_pack_modality_on_a_cpu_store():
    st = _store()
    plan = lambda *a, **k: tuple(t.tolist() for t in st._modality_plan(*a, **k))      # noqa: E731
    # stored bags are numbered case-major: a -> 0, 1; b -> 2, 3; c -> 4; d -> 5, 6, 7
    assert plan(None, 0) == ([0, 1, 2, 3], [0, 2, 4, 5], [5, 2, 1, 4])               # None: every case that has the stain, in case order
    assert plan(None, 1) == ([1, 3], [3, 6], [7, 4]) and plan(None, 2) == ([0, 3], [1, 7], [3, 9])
    assert plan([3, 0], 2) == ([3, 0], [7, 1], [9, 3])                                 # in the order asked
    assert plan([3, 0, 3], 0, max_tokens=3) == ([3, 0, 3], [5, 0, 5], [3, 3, 3]) and plan([2], 0, max_tokens=3)[2] == [1]
    assert plan(torch.tensor([1]), 1) == ([1], [3], [7]) and plan([], 1) == ([], [], [])
    cases, bag, lens = st._modality_plan(None, 0)
    assert cases.dtype == torch.int64 and bag.dtype == torch.int32 and lens.dtype == torch.int64
    with pytest.raises(ValueError, match=r"case 2 \(c\) has no HER2 bag"):
        st._modality_plan([3, 2, 0], 1)
    with pytest.raises(ValueError, match=r"case 1 \(b\) has no PGR bag"):
        st._modality_plan([0, 1, 2], 2)
    for bad in (3, -1, 1.0, True, None):
        with pytest.raises(IndexError, match="modality"):
            st._modality_plan([0], bad)
    with pytest.raises(IndexError):
        st._modality_plan([4], 0)
    with pytest.raises(ValueError, match="max_tokens"):
        st._modality_plan([0], 0, max_tokens=0)


def test_embedding_a_cpu_store_raises():
    st = _store()
    for call in (lambda: st.mean_embeddings(), lambda: st.mean_embeddings(1, [1, 3], host_wgs=2), lambda: st.embed(None),
                 lambda: st.embed(None, 1, [1], bags_per_launch=2, max_tokens=4, precision=torch.bfloat16),
                 lambda: st.pack_modality([0, 1], 0), lambda: st.pack_modality([1], 1, max_tokens=3, counter=1, seed=2)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    z = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MF.bag_mean(st.rows, st.off, torch.zeros(1, dtype=torch.int32), z, 1)


def test_pack_lens_and_the_plan_of_pack_are_unchanged():
    st = _store()
    assert st.pack_lens([0, 1, 2, 3]) == [5, 2, 3, 2, 7, 2, 1, 2, 2, 4, 4, 9]
    assert st.pack_lens([0, 1, 2, 3], max_tokens=4) == [4, 2, 3, 2, 4, 2, 1, 2, 2, 4, 4, 4]
    assert st.pack_lens([3, 0]) == [4, 4, 9, 5, 2, 3]
    bag, lens = st._pack_plan([3, 0], 6)
    assert bag.tolist() == [5, 6, 7, 0, -1, 1] and lens.tolist() == [4, 4, 6, 5, 2, 3] and bag.dtype == torch.int32
    half = _store(dtype=torch.bfloat16)
    assert half.pack_lens([3, 0], 6) == [4, 4, 6, 5, 2, 3] and half._modality_plan(None, 1)[2].tolist() == [7, 4]
    assert callable(st._pack_bags)
