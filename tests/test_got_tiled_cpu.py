"""The tiled GOT class without a GPU: argument validation of its six entry points, the workspace size, plan product 12, the routing
predicate of GOT(), and the fp64 restatement of tests/test_got_tiled_gpu.py against the oracle."""
import ctypes

import pytest
import torch

from madeleine_amd import _native
from oracle import restatement as R
from tests._util import t

E_ARG, E_ALIGN, E_UNSUP = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    return _native.lib()


def _buf():
    raw = ctypes.create_string_buffer(64)
    base = ctypes.addressof(raw)
    return raw, (base + 15) & ~15


def test_tiled_entry_points_validate_arguments(lib):
    raw, p = _buf()
    mis = p + 4
    # limits: n, d in [1, 4096]
    assert lib.mdl_got_tiled_ws_bytes(1, 4096, 128) > 0 and lib.mdl_got_tiled_ws_bytes(1, 64, 4096) > 0
    assert lib.mdl_got_tiled_ws_bytes(1, 4097, 128) == E_UNSUP and lib.mdl_got_tiled_ws_bytes(1, 64, 4097) == E_UNSUP
    assert lib.mdl_got_tiled_ws_bytes(-1, 8, 8) == E_ARG and lib.mdl_got_tiled_ws_bytes(1, -1, 8) == E_ARG
    assert lib.mdl_got_tiled_ws_bytes(1, 8, 0) == E_ARG
    for n, d, rc in ((4097, 8, E_UNSUP), (8, 4097, E_UNSUP)):
        assert lib.mdl_got_tiled_fwd(p, p, p, None, None, 1, n, d, p, None) == rc
        assert lib.mdl_got_tiled_extrema(p, p, p, 1, n, d, p, None) == rc
        assert lib.mdl_got_tiled_bwd_begin(p, None, 1, n, d, p, None) == rc
        assert lib.mdl_got_tiled_bwd_finish(p, p, p, p, None, 1, n, d, p, None) == rc
        assert lib.mdl_got_tiled_bwd(p, p, p, p, p, 1, n, d, p, None) == rc
    # null pointers
    assert lib.mdl_got_tiled_fwd(None, p, p, None, None, 1, 8, 8, p, None) == E_ARG
    assert lib.mdl_got_tiled_fwd(p, p, None, None, None, 1, 8, 8, p, None) == E_ARG
    assert lib.mdl_got_tiled_fwd(p, p, p, None, None, 1, 8, 8, None, None) == E_ARG
    assert lib.mdl_got_tiled_extrema(p, p, None, 1, 8, 8, p, None) == E_ARG
    assert lib.mdl_got_tiled_extrema(p, p, p, 0, 8, 8, p, None) == E_ARG   # extrema of an empty batch
    assert lib.mdl_got_tiled_bwd_begin(None, None, 1, 8, 8, p, None) == E_ARG
    assert lib.mdl_got_tiled_bwd_finish(p, p, None, p, None, 1, 8, 8, p, None) == E_ARG
    assert lib.mdl_got_tiled_bwd(p, p, None, p, p, 1, 8, 8, p, None) == E_ARG
    # misaligned workspace
    assert lib.mdl_got_tiled_fwd(p, p, p, None, None, 1, 8, 8, mis, None) == E_ALIGN
    assert lib.mdl_got_tiled_extrema(p, p, p, 1, 8, 8, mis, None) == E_ALIGN
    assert lib.mdl_got_tiled_bwd_begin(p, None, 1, 8, 8, mis, None) == E_ALIGN
    assert lib.mdl_got_tiled_bwd_finish(p, p, p, p, None, 1, 8, 8, mis, None) == E_ALIGN
    assert lib.mdl_got_tiled_bwd(p, p, p, p, p, 1, 8, 8, mis, None) == E_ALIGN
    # the resident classes keep their refusals
    assert lib.mdl_got_ws_bytes(1, 513, 128) == E_UNSUP and lib.mdl_got_ws_bytes(1, 64, 129) == E_UNSUP


def test_tiled_ws_bytes_monotone_and_covers_the_tape(lib):
    ws = lambda k, n, d: lib.mdl_got_tiled_ws_bytes(k, n, d)  # noqa: E731
    for k in (1, 2, 7):
        for n in (1, 15, 16, 17, 128, 129, 512, 1000, 4096):
            for d in (1, 128, 129, 4096):
                b = ws(k, n, d)
                assert b > 0
                assert ws(k + 1, n, d) > b
                if n < 4096:
                    assert ws(k, n + 1, d) > b
                if d < 4096:
                    assert ws(k, n, d + 1) >= b
                # tape: 30 WD plans + 5 x 20 GW plans + 5 C_gamma, one n x n matrix each, per case
                assert b >= 4 * k * 135 * n * n
    assert ws(1, 4096, 128) < 11 * 2 ** 30                     # ~151 n^2 floats per case
    assert ws(0, 700, 8) > 0 and ws(1, 0, 8) > 0               # empty batches are accepted (zero outputs)


def test_plan_got_tiled_thresholds():
    plan = lambda k, n, d: _native.dispatch_plan("got_tiled", k, n, d)  # noqa: E731
    assert _native.PLAN_PRODUCTS["got_tiled"] == 12
    p = plan(1, 16, 128)
    assert p["variant"] == 16 and p["splits"] == 1 and p["tps"] == 128 and p["empty"] == 1 and p["chunk"] == 256 and p["extra"] == 2
    assert plan(1, 17, 128)["splits"] == 2
    assert plan(1, 128, 128)["empty"] == 1 and plan(1, 129, 128)["empty"] == 4
    assert plan(3, 4096, 128)["splits"] == 256 and plan(3, 4096, 128)["empty"] == 1024
    assert plan(1, 4096, 4096)["splits"] == 256
    lib = _native.lib()
    out = (ctypes.c_int64 * 7)()
    assert lib.mdl_dispatch_plan(12, 1, 4097, 128, 256, ctypes.addressof(out), 7) == E_UNSUP
    assert lib.mdl_dispatch_plan(12, 1, 64, 4097, 256, ctypes.addressof(out), 7) == E_UNSUP
    assert lib.mdl_dispatch_plan(12, 0, 64, 128, 256, ctypes.addressof(out), 7) == E_ARG
    assert lib.mdl_dispatch_plan(12, 1, 0, 128, 256, ctypes.addressof(out), 7) == E_ARG
    assert lib.mdl_dispatch_plan(12, 1, 64, 0, 256, ctypes.addressof(out), 7) == E_ARG
    # product 10 keeps its refusal
    assert lib.mdl_dispatch_plan(10, 1, 513, 0, 256, ctypes.addressof(out), 7) == E_UNSUP


def test_got_route_predicate():
    from madeleine_amd.loss import got_route
    assert got_route(2, 256, 128) == "resident"
    assert got_route(2, 512, 128) == "resident"
    assert got_route(0, 512, 128) == "resident"
    assert got_route(2, 513, 128) == "tiled"
    assert got_route(2, 40, 129) == "tiled"
    assert got_route(1, 4096, 4096) == "tiled"
    assert got_route(0, 700, 8) == "tiled"
    assert got_route(1, 4097, 128) == "unsupported"
    assert got_route(1, 64, 4097) == "unsupported"


def test_restatement_matches_oracle_on_cpu():
    from tests.test_got_tiled_gpu import got_parts64
    v = t((2, 24, 16), "got_tiled:cpu:v").double()
    q = t((2, 24, 16), "got_tiled:cpu:q").double() + 0.7 * v
    a, b = got_parts64(v, q), R.got_parts(v, q)
    assert torch.allclose(a, b, rtol=1e-12, atol=0)
    ex = R.got_extrema(v, q) * 1.01
    assert torch.allclose(got_parts64(v, q, ex), R.got_parts(v, q, ex), rtol=1e-12, atol=0)
    c = got_parts64(v, q, ckpt=True)
    assert torch.allclose(a, c, rtol=1e-12, atol=0)
