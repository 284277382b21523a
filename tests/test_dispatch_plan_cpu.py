"""mdl_dispatch_plan (include/madeleine_amd.h): the host-only query of what each launcher chooses for a shape -- kernel / tile variant,
persistence, token splits of the dW-type contractions, GOT size class and split sweeps.  No GPU: these run with -m "not gpu" and catch a
retune of a split rule or a tile threshold that breaks an invariant of the kernels before any GPU run.  tests/test_dispatch_edges_gpu.py
uses the same query to assert that each of its shapes reaches the branch it is named after."""
import pytest

from tests import _switches


@pytest.fixture
def _default_switches():
    """The pinned values are those of the default switches (the invariants hold for any of their values)."""
    changed = _switches.non_default()
    if changed:
        pytest.skip("pinned values are those of the default switches; the library sees %r" % changed)


defaults_only = pytest.mark.usefixtures("_default_switches")

# (product, a, b) of the token-split products: heads for the gates, (Mi, N) / (N, K) for the products
SPLIT_PRODUCTS = [("gate_fp32_bwd", 4, 0), ("gate_fp32_bwd", 1, 0), ("gate_split_bwd", 4, 0), ("gate_split_bwd", 8, 0),
                  ("gate_bf16_bwd", 4, 0), ("gate_bf16_bwd", 1, 0), ("split_tn", 512, 512), ("split_tn", 768, 256),
                  ("split_tn", 32, 32), ("split_tn", 512, 256), ("linear_fp32_bwd", 512, 512), ("linear_fp32_bwd", 128, 512),
                  ("linear_bf16_bwd", 256, 512), ("linear_bf16_bwd", 512, 1024), ("linear_bf16_bwd", 384, 256)]
SWEEP_T = sorted(set(list(range(1, 300)) + [2 ** e + d for e in range(8, 19) for d in (-1, 0, 1)] +
                 list(range(4000, 70000, 1013)) + [61441, 126977, 131073, 172039, 192514, 258055, 262144, 270000, 400000, 1000003]))


def _plan(*args, **kw):
    from madeleine_amd import _native
    return _native.dispatch_plan(*args, **kw)


@defaults_only
def test_pinned_plans():
    """Hand-computed from splits_for (gate_common.hpp): S = max(ceil(T / 32768), min(ceil(T / 4096), ceil(slots / tiles))), then
    rounded up to whole rounds of `slots` workgroups when it fills half of them; tps = ceil(T / S) rounded up to whole chunks."""
    # config 2 (B = 32, M = 2, N = 4096 -> T = 262144, H = 4), split gate dW: 32 tiles per split on 256 slots -> fill 8 = ceil(T / 32768);
    # 8 x 32 = 256 tiles = one round
    p = _plan("gate_split_bwd", 262144, 4)
    assert (p["splits"], p["tps"], p["empty"], p["chunk"]) == (8, 32768, 0, 32)
    # S > 64: split TN 768 x 256 (3 tiles): ceil(T / 4096) = 43, 129 tiles >= 128 -> one round of 256 slots = 86 splits, tps 2001 -> 2016
    p = _plan("split_tn", 172039, 768, 256)
    assert (p["splits"], p["tps"], p["empty"]) == (86, 2016, 0)
    # empty trailing split: split TN 512 x 512 (4 tiles): 32 -> 64 splits, tps 1985 -> 2016, 63 x 2016 = 127008 >= T
    p = _plan("split_tn", 126977, 512, 512)
    assert (p["splits"], p["tps"], p["empty"]) == (64, 2016, 1)
    # the same on the bf16 gate dW 256 kernel (H = 1: 8 tiles, 64-token chunks): 16 -> 32 splits, tps 1921 -> 1984, 31 x 1984 >= T
    p = _plan("gate_bf16_bwd", 61441, 1)
    assert (p["variant"], p["splits"], p["tps"], p["empty"], p["chunk"]) == (256, 32, 1984, 1, 64)
    # the bf16 Linear recomputes S from tps instead: 127 splits, none empty
    p = _plan("linear_bf16_bwd", 258055, 256, 512)
    assert (p["splits"], p["tps"], p["empty"]) == (127, 2048, 0)


@defaults_only
def test_pinned_thresholds():
    """The tile / class thresholds the GPU edge tests are written around, one shape on each side."""
    assert [_plan("gate_bf16_fwd", T, 4)["variant"] for T in (4095, 4096)] == [128, 256]
    assert [_plan("gate_bf16_fwd", T, 4)["persist"] for T in (16384, 20000)] == [1, 0]
    assert [_plan("gate_bf16_bwd", T, 4)["extra"] for T in (4095, 4096)] == [128, 256]
    assert [_plan("gate_bf16_bwd", T, 4)["variant"] for T in (16383, 16384)] == [128, 256]
    assert [_plan("linear_bf16_bwd", T, 256, 512)["variant"] for T in (16383, 16384)] == [128, 256]
    assert _plan("linear_bf16_bwd", 16384, 384, 256)["variant"] == 128                     # N % 256 != 0
    assert [_plan("linear_bf16_fwd", T, 256, 1024)["variant"] for T in (4095, 4096)] == [4, 256]
    assert [_plan("linear_bf16_fwd", 4096, N, 512)["variant"] for N in (1024, 768)] == [256, 4]   # 4 vs 3 column tiles at Kc = 512
    assert _plan("linear_bf16_fwd", 4096, 1024, 512)["persist"] == 4
    assert _plan("linear_bf16_fwd", 4096, 256, 1056)["variant"] == 4                      # Kc % 64 != 0
    assert [_plan("linear_fp32_bwd", 4097, N, 512)["variant"] for N in (256, 128)] == [1, 2]
    assert [_plan("got", 2, n)["variant"] for n in (64, 65, 128, 129, 192, 193, 256, 257)] == [64, 128, 128, 192, 192, 256, 256, 512]
    assert [_plan("got", k, 193, cus=256)["extra"] for k in (64, 65, 128, 129)] == [2, 1, 1, 0]
    assert [_plan("got", k, 193, cus=256)["persist"] for k in (128, 129)] == [1, 0]
    assert _plan("got", 64, 193, cus=128)["extra"] == 1                                    # the answer follows `cus`
    assert _plan("got", 2, 100, cus=256)["extra"] == 0                                     # no split sweeps in the fused classes


@pytest.mark.parametrize("product,a,b", SPLIT_PRODUCTS)
def test_split_invariants(product, a, b):
    """What the split kernels and the slab reductions rely on, for any retune: 1 <= S <= 192; tps a positive whole number of chunks;
    the S splits cover all T tokens; EMPTY counts exactly the splits s with s * tps >= T; the bf16 Linear (which recomputes S from tps)
    has no empty split."""
    for T in SWEEP_T:
        p = _plan(product, T, a, b)
        S, tps, chunk, empty = p["splits"], p["tps"], p["chunk"], p["empty"]
        if product == "linear_fp32_bwd" and T <= 256:    # the FMA kernel of few rows: no token splits
            assert p["variant"] == 0 and (S, tps, chunk, empty) == (1, 0, 0, 0), (T, p)
            continue
        assert 1 <= S <= 192, (T, p)
        assert chunk > 0 and tps >= chunk and tps % chunk == 0, (T, p)
        assert S * tps >= T, (T, p)
        assert empty == sum(1 for s in range(S) if s * tps >= T), (T, p)
        if product == "linear_bf16_bwd":
            assert (S - 1) * tps < T and empty == 0, (T, p)


def test_forward_products_have_no_splits():
    for product, a, b in [("gate_split_fwd", 4, 0), ("gate_bf16_fwd", 4, 0), ("linear_bf16_fwd", 256, 512), ("got", 193, 0)]:
        for T in (1, 300, 4096, 20000):
            p = _plan(product, T, a, b)
            assert (p["splits"], p["tps"], p["empty"], p["chunk"]) == (1, 0, 0, 0), (product, T, p)


def test_plan_rejects_what_the_launchers_reject():
    import ctypes

    from madeleine_amd import _native
    lib = _native.lib()
    out = (ctypes.c_int64 * 7)()
    call = lambda prod, T, a, b, n=7: lib.mdl_dispatch_plan(prod, T, a, b, 256, ctypes.addressof(out), n)   # noqa: E731
    assert call(99, 100, 4, 0) == -1                        # unknown product
    assert call(3, -1, 4, 0) == -1 and call(3, 100, 9, 0) == -1 and call(3, 100, 3, 0) == -3   # T < 0, H > 8, H = 3
    assert call(6, 100, 48, 32) == -1                       # split TN: Mi % 32 != 0
    assert call(7, 1000, 200, 512) == -3                    # fp32 Linear: N % 128 != 0
    assert call(9, 1000, 100, 512) == -3                    # bf16 Linear: N % 128 != 0
    assert call(10, 2, 513, 0) == -3 and call(10, 0, 64, 0) == -1    # GOT: n > 512, no case
    assert call(3, 100, 4, 0, n=0) == -1
    out[3] = -7
    assert call(3, 5000, 4, 0, n=3) == 0 and out[2] == 2 and out[3] == -7   # n_out caps what is written
    assert lib.mdl_dispatch_plan(3, 100, 4, 0, 256, None, 7) == -1


@defaults_only
def test_head_count_cases_take_their_branches():
    """The gate and split-TN cases of tests/test_heads_gpu.py (1, 2 and 8 heads) reach the branches they are named after on a 256-CU
    device; the GPU tests assert the same with the device's own CU count."""
    from tests.test_heads_gpu import GATE_CASES, TN_CASES
    for case in GATE_CASES:
        _mode, T, H, _p, plans = case.values
        for product, want in plans.items():
            p = _plan(product, T, H)
            assert {k: p[k] for k in want} == want, (case.id, product, p)
    for case in TN_CASES:
        T, Mi, N, want = case.values
        p = _plan("split_tn", T, Mi, N)
        assert {k: p[k] for k in want} == want, (case.id, p)
