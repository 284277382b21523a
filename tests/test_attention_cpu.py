"""The attention read-out without a GPU: the A-map entry points (declared, bound, exported), every refusal of the header in its order
on fake host pointers -- nothing here reaches a launch --, the workspace query, the refusal of a store built on the CPU, and the numpy
reference of the GPU tests against scipy (or the O(n^2) count of the definition)."""
import ctypes

import numpy as np
import pytest
import torch

from madeleine_amd import _build, _native
from madeleine_amd import functional as MF
from madeleine_amd.store import DeviceSlideStore
from tests import _attn_ref as ref

OK, E_ARG, E_ALIGN, E_UNSUP = 0, -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    return _native.lib()


def test_entry_points_are_declared_bound_and_exported(lib):
    with open(_build.HEADER) as f:
        header = f.read()
    assert " * A-map -- " in header
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    want = {"mdl_attn_map_ws_bytes": (L, [L, L, I]),
            #                    scores ld cu T R H attn m l ws stream
            "mdl_attn_softmax": (I, [P, L, P, L, L, I, P, P, P, P, P]),
            #                 scores ld cu T R H k order pct topk_idx topk_val ws stream
            "mdl_attn_rank": (I, [P, L, P, L, L, I, L, P, P, P, P, P, P])}
    handle = ctypes.CDLL(_native.lib_path())
    for name, (res, args) in want.items():
        assert name + "(" in header
        assert _native.SIGNATURES[name] == (res, args), name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
        assert hasattr(handle, name)
    assert _native.ABI_VERSION == 26 and lib.mdl_abi_version() == 26          # additive: the revision stays
    d = _native._DEFINES
    assert d["MDL_ATTN_ROWS"] == MF.ATTN_ROWS >= 256 and d["MDL_ATTN_SORT_KEYS"] == MF.ATTN_SORT_KEYS >= 256
    assert callable(MF.attn_softmax) and callable(MF.attn_rank)


def test_workspace_query(lib):
    C = MF.ATTN_SORT_KEYS
    q = lib.mdl_attn_map_ws_bytes
    assert q(-1, 1, 4) == E_ARG and q(1, -1, 4) == E_ARG
    for H in (0, 3, 5, 16, -1):
        assert q(10, 1, H) == E_UNSUP, H
    assert q(2 ** 31, 1, 1) == E_UNSUP and q(1, 2 ** 31, 1) == E_UNSUP and q(2 ** 31 - 1, 2 ** 31 - 1, 1) == E_UNSUP
    assert q(-1, 1, 3) == E_ARG                                               # argument before geometry
    for T, R, H in ((0, 0, 1), (1, 1, 1), (7114, 12, 4), (30000 * 48, 48, 4), (5 * C, 3, 8)):
        n = q(T, R, H)
        chunks = T // C + R
        # keys twice, one row-index buffer, 256 counters per chunk, two partials per chunk (all per head), three per-bag tables
        assert n >= 3 * 4 * H * T + H * chunks * (256 * 4 + 8) + 4 * (3 * R + 1) and n % 16 == 0, (T, R, H)
        assert n <= 3 * 4 * H * T + H * chunks * (256 * 4 + 8) + 4 * (3 * R + 1) + 16 * 9


def _good():
    raw = ctypes.create_string_buffer(2048)
    p = (ctypes.addressof(raw) + 15) & ~15          # host memory: a launch on it would fault, so every case below must refuse first
    return raw, p, dict(scores=p, ld=4, cu=p + 64, T=0, R=3, H=4, k=2, attn=p + 128, m=p + 192, l=p + 256, order=p + 320, pct=p + 384,
                        topk_idx=p + 448, topk_val=p + 512, ws=p + 1024)


def _softmax(lib, good):
    def call(**kw):
        a = dict(good, **kw)
        return lib.mdl_attn_softmax(a["scores"], a["ld"], a["cu"], a["T"], a["R"], a["H"], a["attn"], a["m"], a["l"], a["ws"], None)
    return call, ("scores", "cu", "attn", "m", "l", "ws"), (), ("scores", "attn", "m", "l")


def _rank(lib, good):
    def call(**kw):
        a = dict(good, **kw)
        return lib.mdl_attn_rank(a["scores"], a["ld"], a["cu"], a["T"], a["R"], a["H"], a["k"], a["order"], a["pct"], a["topk_idx"],
                                 a["topk_val"], a["ws"], None)
    return call, ("scores", "cu", "order", "topk_idx", "topk_val", "ws"), ("pct",), ("scores", "order", "pct", "topk_idx", "topk_val")


@pytest.mark.parametrize("entry", [_softmax, _rank], ids=["softmax", "rank"])
def test_every_refusal_in_the_headers_order(lib, entry):
    raw, p, good = _good()
    call, required, optional, four_byte = entry(lib, good)
    assert call() == OK, "the valid call over no rows"
    # 1. MDL_E_ARG: a NULL required pointer, negative sizes, ld < H, k < 0
    for name in required:
        assert call(**{name: None}) == E_ARG, name
    for name in optional:
        assert call(**{name: None}) == OK, name
    assert call(T=-1) == E_ARG and call(R=-1) == E_ARG and call(ld=3) == E_ARG and call(ld=0) == E_ARG and call(ld=-4) == E_ARG
    assert call(ld=4) == OK and call(ld=7) == OK
    if entry is _rank:
        assert call(k=-1) == E_ARG
        assert call(k=0, topk_idx=None, topk_val=None) == OK, "no top-k buffers without a top-k"
    # 2. MDL_E_UNSUPPORTED: H outside {1, 2, 4, 8}, T or R beyond int32
    for H in (3, 5, 6, 7):
        assert call(H=H, ld=8) == E_UNSUP, H
    assert call(H=16, ld=16) == E_UNSUP and call(H=0) == E_UNSUP
    for H in (1, 2, 4, 8):
        assert call(H=H, ld=8) == OK, H
    assert call(T=2 ** 31) == E_UNSUP and call(R=2 ** 31) == E_UNSUP and call(T=2 ** 40, R=2 ** 40) == E_UNSUP
    if entry is _rank:
        assert call(k=2 ** 31) == E_UNSUP and call(R=2 ** 30, k=2 ** 20) == E_UNSUP
    # 3. MDL_E_ALIGN: the workspace in 16-byte units, cu as int64, every float / int32 buffer in 4-byte units
    assert call(ws=good["ws"] + 4) == E_ALIGN and call(ws=good["ws"] + 8) == E_ALIGN
    assert call(cu=good["cu"] + 4) == E_ALIGN and call(cu=good["cu"] + 8) == OK
    for name in four_byte:
        assert call(**{name: good[name] + 2}) == E_ALIGN and call(**{name: good[name] + 4}) == OK, name
    # 4. R == 0 or T == 0: MDL_OK and no launch (these pointers are host memory)
    assert call(R=0, T=5) == OK and call(R=3, T=0) == OK and call(R=0, T=0) == OK
    # the order of the steps, one pair per step
    assert call(scores=None, H=3, ws=good["ws"] + 4) == E_ARG and call(ld=3, T=2 ** 31) == E_ARG, "argument first"
    assert call(H=3, ws=good["ws"] + 4) == E_UNSUP and call(R=2 ** 31, cu=good["cu"] + 4) == E_UNSUP, "geometry before alignment"
    assert call(R=0, ws=good["ws"] + 4) == E_ALIGN and call(R=0, ws=None) == E_ARG and call(R=0, H=3) == E_UNSUP, "the checks hold for no rows"


def _bags():
    g = torch.Generator().manual_seed(0)
    r = lambda n: torch.randn(n, 6, generator=g)      # noqa: E731
    return [[r(5), None, r(3)], [r(2), r(7), None], [r(1), None, None], [r(4), r(4), r(9)]]


def test_attention_on_a_cpu_store_raises_as_embed_does():
    st = DeviceSlideStore(_bags(), ["a", "b", "c", "d"], ["HE", "HER2", "PGR"], "cpu")
    for call in (lambda: st.attention(None), lambda: st.attention(None, 1, [1], topk=4, percentile=False, bags_per_launch=2,
                                                                  precision=torch.bfloat16, host_wgs=1)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        st.embed(None)
    z = torch.zeros(2, dtype=torch.int64)
    for fn in (MF.attn_softmax, MF.attn_rank):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(torch.zeros(3, 4), z)


def _segments():
    rng = np.random.default_rng(7)
    yield np.array([0.5], np.float32)
    yield rng.standard_normal(257).astype(np.float32)
    yield rng.choice(np.array([-1.5, -0.0, 0.0, 2.0, 3.25], np.float32), 300)          # heavy ties, both zeros
    yield np.full(65, 1.25, np.float32)
    yield rng.integers(0, 2 ** 32, 400, dtype=np.uint64).astype(np.uint32).view(np.float32)      # any bit pattern
    yield np.array([np.nan, np.inf, -np.inf, -np.nan, 0.0, -0.0, 1e-45, -1e-45, 3.0, 3.0], np.float32)


def test_the_reference_agrees_with_scipy_or_the_count():
    try:
        from scipy.stats import rankdata
    except ImportError:
        rankdata = None
    for s in _segments():
        n = len(s)
        pct = ref.percentile(s)
        assert pct.dtype == np.float32 and np.array_equal(pct, ref.percentile_by_counting(s))
        order = ref.order_desc(s)
        key = ref.rank_key(s)
        assert sorted(order.tolist()) == list(range(n))
        assert all(key[order[j]] > key[order[j + 1]] or (key[order[j]] == key[order[j + 1]] and order[j] < order[j + 1]) for j in range(n - 1))
        if rankdata is not None and np.isfinite(s).all():      # scipy has its own rule for NaN; the finite sets are its ground
            want = rankdata(s.astype(np.float64), "average") / n * 100
            assert np.allclose(pct.astype(np.float64), want, rtol=2.0 ** -23, atol=0), n
        idx, val = ref.topk(s, n + 5)
        assert idx[:n].tolist() == order.tolist() and (idx[n:] == -1).all() and np.isneginf(val[n:]).all()
        assert np.array_equal(val[:n].view(np.uint32), s[order].view(np.uint32))
    k = ref.rank_key(np.array([np.nan, -np.nan, np.inf, 1.0, 0.0, -0.0, -1.0, -np.inf], np.float32))
    assert k[0] == k[1] > k[2] > k[3] > k[4] == k[5] > k[6] > k[7]
    a64, m = ref.softmax64(np.array([0.0, 1.0, 1.0], np.float32))
    assert m == 1.0 and abs(a64.sum() - 1.0) < 1e-15 and a64[1] == a64[2] > a64[0]
