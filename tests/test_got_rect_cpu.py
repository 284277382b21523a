"""GOT between token sets of different sizes (v [k, n, d], q [k, m, d]) without a GPU: argument validation of the six
mdl_got_tiled_rect_* entry points, the workspace size, plan product 13, the routing predicate and the host-side IndexError of GOT(),
the fp64 restatement of the GPU file against the oracle, and the golden file against the oracle."""
import ctypes

import pytest
import torch

from madeleine_amd import _native
from oracle import restatement as R
from tests._util import golden, rel_err, t

E_ARG, E_ALIGN, E_UNSUP = -1, -2, -3
GOLDEN_SHAPES = [(2, 40, 56, 128), (3, 70, 33, 128), (1, 1, 9, 32), (2, 17, 1, 64)]


def inputs(k, n, m, d):
    v = t((k, n, d), f"got_rect:{k}x{n}x{m}x{d}:v")
    q = t((k, m, d), f"got_rect:{k}x{n}x{m}x{d}:q") + 0.7 * v[:, torch.arange(m) % n]
    return v, q


@pytest.fixture(scope="module")
def lib():
    return _native.lib()


def _buf():
    raw = ctypes.create_string_buffer(64)
    base = ctypes.addressof(raw)
    return raw, (base + 15) & ~15


def test_rect_entry_points_validate_arguments(lib):
    raw, p = _buf()
    mis = p + 4
    ws = lib.mdl_got_tiled_rect_ws_bytes
    # limits: n, m, d in [1, 4096], each on its own
    assert ws(1, 4096, 8, 128) > 0 and ws(1, 8, 4096, 128) > 0 and ws(1, 64, 32, 4096) > 0
    assert ws(1, 4097, 8, 128) == E_UNSUP and ws(1, 8, 4097, 128) == E_UNSUP and ws(1, 64, 32, 4097) == E_UNSUP
    assert ws(-1, 8, 9, 8) == E_ARG and ws(1, -1, 9, 8) == E_ARG and ws(1, 8, -1, 8) == E_ARG and ws(1, 8, 9, 0) == E_ARG
    for n, m, d, rc in ((4097, 8, 8, E_UNSUP), (8, 4097, 8, E_UNSUP), (8, 9, 4097, E_UNSUP), (8, -1, 8, E_ARG)):
        assert lib.mdl_got_tiled_rect_fwd(p, p, p, None, None, 1, n, m, d, p, None) == rc
        assert lib.mdl_got_tiled_rect_extrema(p, p, p, 1, n, m, d, p, None) == rc
        assert lib.mdl_got_tiled_rect_bwd_begin(p, None, 1, n, m, d, p, None) == rc
        assert lib.mdl_got_tiled_rect_bwd_finish(p, p, p, p, None, 1, n, m, d, p, None) == rc
        assert lib.mdl_got_tiled_rect_bwd(p, p, p, p, p, 1, n, m, d, p, None) == rc
    # null pointers
    assert lib.mdl_got_tiled_rect_fwd(None, p, p, None, None, 1, 8, 9, 8, p, None) == E_ARG
    assert lib.mdl_got_tiled_rect_fwd(p, None, p, None, None, 1, 8, 9, 8, p, None) == E_ARG
    assert lib.mdl_got_tiled_rect_fwd(p, p, None, None, None, 1, 8, 9, 8, p, None) == E_ARG
    assert lib.mdl_got_tiled_rect_fwd(p, p, p, None, None, 1, 8, 9, 8, None, None) == E_ARG
    assert lib.mdl_got_tiled_rect_extrema(p, p, None, 1, 8, 9, 8, p, None) == E_ARG
    for k, n, m in ((0, 8, 9), (1, 0, 9), (1, 8, 0)):   # extrema of an empty batch
        assert lib.mdl_got_tiled_rect_extrema(p, p, p, k, n, m, 8, p, None) == E_ARG
    assert lib.mdl_got_tiled_rect_bwd_begin(None, None, 1, 8, 9, 8, p, None) == E_ARG
    assert lib.mdl_got_tiled_rect_bwd_finish(p, p, None, p, None, 1, 8, 9, 8, p, None) == E_ARG
    assert lib.mdl_got_tiled_rect_bwd_finish(p, p, p, None, None, 1, 8, 9, 8, p, None) == E_ARG
    assert lib.mdl_got_tiled_rect_bwd(p, p, None, p, p, 1, 8, 9, 8, p, None) == E_ARG
    # misaligned workspace
    assert lib.mdl_got_tiled_rect_fwd(p, p, p, None, None, 1, 8, 9, 8, mis, None) == E_ALIGN
    assert lib.mdl_got_tiled_rect_extrema(p, p, p, 1, 8, 9, 8, mis, None) == E_ALIGN
    assert lib.mdl_got_tiled_rect_bwd_begin(p, None, 1, 8, 9, 8, mis, None) == E_ALIGN
    assert lib.mdl_got_tiled_rect_bwd_finish(p, p, p, p, None, 1, 8, 9, 8, mis, None) == E_ALIGN
    assert lib.mdl_got_tiled_rect_bwd(p, p, p, p, p, 1, 8, 9, 8, mis, None) == E_ALIGN
    # the square entry points keep their refusals
    assert lib.mdl_got_tiled_ws_bytes(1, 4097, 128) == E_UNSUP and lib.mdl_got_tiled_ws_bytes(1, 8, 0) == E_ARG


def test_rect_ws_bytes(lib):
    ws = lambda k, n, m, d: lib.mdl_got_tiled_rect_ws_bytes(k, n, m, d)  # noqa: E731
    sq = lambda k, n, d: lib.mdl_got_tiled_ws_bytes(k, n, d)  # noqa: E731
    up4 = lambda x: (x + 3) & ~3  # noqa: E731
    sizes = (1, 15, 16, 17, 128, 129, 512, 1000, 4096)
    for k in (1, 2, 7):
        for n in sizes:
            for d in (1, 128, 129, 4096):
                assert ws(k, n, n, d) == sq(k, n, d)
    for k in (1, 2, 7):
        for n in sizes:
            for m in sizes:
                b = ws(k, n, m, 128)
                assert b > 0
                assert ws(k + 1, n, m, 128) > b
                if n < 4096:
                    assert ws(k, n + 1, m, 128) > b
                if m < 4096:
                    assert ws(k, n, m + 1, 128) > b
                # tape: 30 WD plans + 5 x 20 GW plans + 5 C_gamma, one n x up4(m) matrix each, per case
                assert b >= 4 * k * 135 * n * up4(m)
    # the tape scales with n m, only the Cs- / Ct-like matrices with n^2 / m^2
    assert ws(1, 4096, 512, 128) < sq(1, 4096, 128) // 4
    assert ws(1, 512, 4096, 128) < sq(1, 4096, 128) // 4
    assert ws(0, 700, 30, 8) > 0 and ws(1, 0, 30, 8) > 0 and ws(1, 700, 0, 8) > 0   # empty batches are accepted (zero outputs)


def test_plan_got_tiled_rect_thresholds():
    plan = lambda k, n, m: _native.dispatch_plan("got_tiled_rect", k, n, m)  # noqa: E731
    assert _native.PLAN_PRODUCTS["got_tiled_rect"] == 13
    p = plan(1, 16, 128)
    assert p["variant"] == 16 and p["splits"] == 1 and p["tps"] == 128 and p["empty"] == 1 and p["chunk"] == 256 and p["extra"] == 2
    assert p["persist"] == 0
    assert plan(1, 17, 128)["splits"] == 2 and plan(1, 16, 4096)["splits"] == 1    # splits follow n alone
    assert plan(1, 128, 128)["empty"] == 1 and plan(1, 129, 128)["empty"] == 2 and plan(1, 128, 129)["empty"] == 2
    assert plan(1, 129, 129)["empty"] == 4
    assert plan(3, 4096, 512)["splits"] == 256 and plan(3, 4096, 512)["empty"] == 128
    assert plan(3, 512, 4096)["splits"] == 32 and plan(3, 512, 4096)["empty"] == 128
    lib = _native.lib()
    out = (ctypes.c_int64 * 7)()
    assert lib.mdl_dispatch_plan(13, 1, 4097, 128, 256, ctypes.addressof(out), 7) == E_UNSUP
    assert lib.mdl_dispatch_plan(13, 1, 64, 4097, 256, ctypes.addressof(out), 7) == E_UNSUP
    assert lib.mdl_dispatch_plan(13, 0, 64, 128, 256, ctypes.addressof(out), 7) == E_ARG
    assert lib.mdl_dispatch_plan(13, 1, 0, 128, 256, ctypes.addressof(out), 7) == E_ARG
    assert lib.mdl_dispatch_plan(13, 1, 64, 0, 256, ctypes.addressof(out), 7) == E_ARG
    # product 12 is unchanged: a = n, b = d
    p12 = _native.dispatch_plan("got_tiled", 1, 129, 4096)
    assert p12["splits"] == 9 and p12["empty"] == 4
    assert lib.mdl_dispatch_plan(12, 1, 64, 4097, 256, ctypes.addressof(out), 7) == E_UNSUP
    assert _native.dispatch_plan("got_tiled", 3, 4096, 128) == dict(plan(3, 4096, 4096))


def test_got_route_with_m():
    from madeleine_amd.loss import got_route
    assert got_route(2, 256, 128, m=256) == "resident" and got_route(2, 256, 128, m=None) == "resident"
    assert got_route(2, 513, 128, m=513) == "tiled"
    assert got_route(2, 256, 128, m=255) == "tiled"       # never "resident" when the token counts differ
    assert got_route(2, 40, 128, 56) == "tiled"
    assert got_route(1, 4096, 4096, m=1) == "tiled" and got_route(1, 1, 8, m=4096) == "tiled"
    assert got_route(0, 40, 8, m=30) == "tiled"
    assert got_route(1, 4097, 128, m=8) == "unsupported"
    assert got_route(1, 8, 128, m=4097) == "unsupported"
    assert got_route(1, 8, 4097, m=9) == "unsupported"


def test_got_subsample_index_error_on_the_host():
    """With n != m the reference indexes both tensors with randperm(k)[:subsample]; an index beyond the shorter one is an IndexError,
    raised before any device work (CPU tensors get that far)."""
    from madeleine_amd import GOT
    v, q = torch.zeros(12, 20, 8), torch.zeros(12, 5, 8)      # k = 12 > min(n, m) = 5: randperm(12)[:12] holds 11
    with pytest.raises(IndexError):
        GOT(v, q, subsample=256)
    with pytest.raises(IndexError):
        GOT(q, v, subsample=12)


def test_restatement_matches_oracle_on_cpu_rect():
    from tests.test_got_tiled_gpu import got_parts64
    k, n, m, d = 2, 24, 37, 16
    v = t((k, n, d), "got_rect:cpu:v").double()
    q = t((k, m, d), "got_rect:cpu:q").double() + 0.7 * v[:, torch.arange(m) % n]
    a, b = got_parts64(v, q), R.got_parts(v, q)
    assert torch.allclose(a, b, rtol=1e-12, atol=0)
    ex = R.got_extrema(v, q) * 1.01
    assert torch.allclose(got_parts64(v, q, ex), R.got_parts(v, q, ex), rtol=1e-12, atol=0)
    assert torch.allclose(got_parts64(v, q, ckpt=True), a, rtol=1e-12, atol=0)


@pytest.mark.parametrize("k,n,m,d", GOLDEN_SHAPES)
def test_golden_got_rect_is_reproduced_by_the_oracle(k, n, m, d):
    """tests/golden/got_rect.npz (the reference's fp32 GOT value, dV, dQ; tools/gen_golden_got_rect.py) against oracle.restatement.got
    in fp32 on the CPU, at the bar of tests/test_oracle_golden.py."""
    g = golden("got_rect")
    tag = f"{k}x{n}x{m}x{d}"
    v, q = inputs(k, n, m, d)
    v.requires_grad_()
    q.requires_grad_()
    loss = R.got(v, q)
    loss.backward()
    assert g[tag + "/dv"].shape == (k, n, d) and g[tag + "/dq"].shape == (k, m, d)
    ref = float(g[tag + "/loss"])
    assert abs(float(loss.detach()) - ref) <= 1e-5 * abs(ref)
    assert rel_err(v.grad, g[tag + "/dv"]) < 1e-5 and rel_err(q.grad, g[tag + "/dq"]) < 1e-5
