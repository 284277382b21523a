"""The contribution kernels on the GPU (X1-X2, include/madeleine_amd_explain.h) against the fp64 references of tests/_contrib_ref.py:
mdl_attn_contrib under the per-element any-order fp32 summation bound, bit for bit on integer data, row-local (a row alone, at another
offset and stride, beside a NaN), inside its stated extents; mdl_contrib_stats on bags around the chunk size, exact on integer data,
under the summation bound on random data, with the bits of a bag depending on the bag alone."""
import functools

import numpy as np
import pytest
import torch

from madeleine_amd import functional as MF
from tests import _contrib_ref as ref
from tests._arena import FILLS, Arena

pytestmark = pytest.mark.gpu

W = MF.HID
TS = [1, 63, 64, 65, 255, 256, 257, 1025]      # one row, both sides of a wave / of a 256-thread sweep, several rounds of every tile shape
TMAX = max(TS)
HS = [1, 2, 4, 8]
CS = [1, 2, 3, 5, 8]
DTYPES = [torch.float32, torch.bfloat16]
U23 = ref.U23


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


@functools.lru_cache(maxsize=None)
def inputs(H, dtype, kind):
    """(E [TMAX, H W] in `dtype`, attn [TMAX, H] fp32, U [8, H W] fp32) on the host, computed once and left unchanged.  'random':
    normals, attention weights in (0, 1); 'integer': E and U in [-3, 3], attn a power of two in [2^-6, 1]: every product and every
    partial sum is an integer below 512 * 9 * 8 < 2^24 times a power of two, so any summation order is exact."""
    g = torch.Generator().manual_seed(1000 * H + (1 if dtype == torch.bfloat16 else 0) + (17 if kind == "integer" else 0))
    if kind == "random":
        E = torch.randn(TMAX, H * W, generator=g)
        attn = torch.rand(TMAX, H, generator=g)
        U = torch.randn(8, H * W, generator=g)
    else:
        E = torch.randint(-3, 4, (TMAX, H * W), generator=g).float()
        attn = torch.pow(2.0, -torch.randint(0, 7, (TMAX, H), generator=g).float())
        U = torch.randint(-3, 4, (8, H * W), generator=g).float()
    return E.to(dtype), attn, U


@functools.lru_cache(maxsize=None)
def reference(H, dtype, kind, C):
    """the fp64 reference of the first C columns on exactly the values the device reads (bf16 E widened exactly)"""
    E, attn, U = inputs(H, dtype, kind)
    if kind == "integer":
        out = ref.contrib_int(E.float().numpy(), attn.numpy(), U[:C].numpy(), H)
    else:
        out = ref.contrib(E.float().numpy(), attn.numpy(), U[:C].numpy(), H)
    for v in out:
        v.setflags(write=False)
    return out


def strided(x, pad, dev, fill=float("nan")):
    """x [T, n] on the device as a view of row stride n + pad, the padding holding `fill`"""
    wide = torch.full((x.shape[0], x.shape[1] + pad), fill, dtype=x.dtype, device=dev)
    wide[:, :x.shape[1]] = x.to(dev)
    return wide[:, :x.shape[1]]


def launch(E, attn, U, T, H, C, per_head, ldO, dev):
    """mdl_attn_contrib on the first T rows of the (strided) views E and attn -> (total view [T, C] of a [T, ldO] buffer, the buffer,
    per_head or None).  The buffer is pre-filled with a sentinel."""
    buf = torch.full((T, ldO), -77.0, device=dev)
    heads = torch.full((T, H, C), -77.0, device=dev) if per_head else None
    MF._call("mdl_attn_contrib", E, E.stride(0), 1 if E.dtype == torch.bfloat16 else 0, attn, attn.stride(0), U, T, H, W, C, heads, buf,
             ldO, MF._stream())
    return buf[:, :C], buf, heads


@functools.lru_cache(maxsize=None)
def device_inputs(H, dtype, kind):
    dev = torch.device("cuda:0")
    E, attn, U = inputs(H, dtype, kind)
    return strided(E, 8, dev), strided(attn, 3, dev), U.to(dev)


# ------------------------------------------------------------------------------------------------ X1: bounds and exactness
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("H", HS)
def test_contrib_within_the_summation_bound(dev, H, C, dtype):
    """|per_head - ref| <= (W + 4) 2^-23 sum_e |a u_e E_e| and |total - ref| <= (H W + 4) 2^-23 sum_{h, e} |...| per element: the
    any-order fp32 summation bound with a factor 2 of slack.  ldE = H W + 8, ldA = H + 3, ldO = C + 1; per_head NULL and given."""
    E, attn, U = device_inputs(H, dtype, "random")
    assert E.stride(0) == H * W + 8 and attn.stride(0) == H + 3
    ph64, tot64, aph, atot = reference(H, dtype, "random", C)
    Uc = U[:C].contiguous()
    worst = [0.0, 0.0]
    for T in TS:
        total, buf, heads = launch(E, attn, Uc, T, H, C, True, C + 1, dev)
        lean, lbuf, none = launch(E, attn, Uc, T, H, C, False, C + 1, dev)
        assert none is None and np.array_equal(bits(lean), bits(total)), "per_head NULL changes nothing"
        assert bool((buf[:, C] == -77.0).all()) and bool((lbuf[:, C] == -77.0).all()), "the padding column is not written"
        eh = np.abs(heads.cpu().numpy().astype(np.float64) - ph64[:T])
        et = np.abs(total.cpu().numpy().astype(np.float64) - tot64[:T])
        bh, bt = (W + 4) * U23 * aph[:T], (H * W + 4) * U23 * atot[:T]
        worst = [max(worst[0], float((eh / bh).max())), max(worst[1], float((et / bt).max()))]
        assert bool((eh <= bh).all()), (T, float((eh / bh).max()))
        assert bool((et <= bt).all()), (T, float((et / bt).max()))
        # heads added in ascending order: total is that fp32 sum exactly
        acc = heads[:, 0]
        for h in range(1, H):
            acc = acc + heads[:, h]
        assert np.array_equal(bits(acc), bits(total)), T
    print("contrib H %d C %d %s: worst error / bound per_head %.4f, total %.4f" % (H, C, dtype, worst[0], worst[1]))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("H", HS)
def test_contrib_is_exact_on_integers(dev, H, C, dtype):
    """E and U small integers, attn powers of two, every partial sum below 2^24: the device equals int64 numpy bit for bit at every T."""
    E, attn, U = device_inputs(H, dtype, "integer")
    ph, tot = reference(H, dtype, "integer", C)
    assert float(np.abs(tot).max()) < 2.0 ** 24
    ph32, tot32 = ph.astype(np.float32), tot.astype(np.float32)
    assert np.array_equal(ph32.astype(np.float64), ph) and np.array_equal(tot32.astype(np.float64), tot)
    Uc = U[:C].contiguous()
    for T in TS:
        total, _, heads = launch(E, attn, Uc, T, H, C, True, C + 1, dev)
        assert np.array_equal(bits(heads), ph32[:T].view(np.int32)), T
        assert np.array_equal(bits(total), tot32[:T].view(np.int32)), T


# ------------------------------------------------------------------------------------------------ X1: row locality
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("H,C", [(1, 8), (2, 3), (4, 5), (8, 1), (4, 8)])
def test_contrib_rows_are_local(dev, H, C, dtype):
    """Row t alone, at another offset, with another ld, and inside the big call: identical bits.  A NaN and an Inf planted in rows of
    E change those rows only."""
    E, attn, U = device_inputs(H, dtype, "random")
    Uc = U[:C].contiguous()
    big_t, _, big_h = launch(E, attn, Uc, TMAX, H, C, True, C + 1, dev)
    for T in (1, 65, 257):                                              # the same rows in a shorter call
        t, _, h = launch(E, attn, Uc, T, H, C, True, C + 4, dev)
        assert np.array_equal(bits(t), bits(big_t[:T])) and np.array_equal(bits(h), bits(big_h[:T])), T
    rows = [1024, 0, 100, 63, 64, 511, 1000]
    for k, r in enumerate(rows):                                        # one row alone (T = 1), from a base 16 (k + 1) elements in
        ebuf = torch.zeros(16 * (k + 1) + H * W, dtype=E.dtype, device=dev)
        ebuf[16 * (k + 1):] = E[r]
        abuf = torch.zeros(5 + H, device=dev)
        abuf[5:] = attn[r]
        e1, a1 = ebuf[16 * (k + 1):].view(1, H * W), abuf[5:].view(1, H)
        buf = torch.full((1, C), -77.0, device=dev)
        heads = torch.full((1, H, C), -77.0, device=dev)
        MF._call("mdl_attn_contrib", e1, H * W, 1 if E.dtype == torch.bfloat16 else 0, a1, H, Uc, 1, H, W, C, heads, buf, C, MF._stream())
        assert np.array_equal(bits(buf[0]), bits(big_t[r])) and np.array_equal(bits(heads[0]), bits(big_h[r])), r
    sel = torch.tensor(rows, device=dev)                                 # the rows together, in another order, ld = H W + 16 / H + 1
    t, _, h = launch(strided(E[sel].cpu(), 16, dev), strided(attn[sel].cpu(), 1, dev), Uc, len(rows), H, C, True, C, dev)
    assert np.array_equal(bits(t), bits(big_t[sel])) and np.array_equal(bits(h), bits(big_h[sel]))
    bad = strided(E.cpu(), 8, dev)
    bad[5, 7] = float("nan")
    bad[300, H * W - 1] = float("inf")
    bad_a = strided(attn.cpu(), 3, dev)
    bad_a[700, 0] = float("nan")
    t, _, h = launch(bad, bad_a, Uc, TMAX, H, C, True, C + 1, dev)
    keep = torch.ones(TMAX, dtype=torch.bool, device=dev)
    keep[[5, 300, 700]] = False
    assert np.array_equal(bits(t[keep]), bits(big_t[keep])) and np.array_equal(bits(h[keep]), bits(big_h[keep]))
    assert bool(torch.isnan(t[5]).all()) and bool(torch.isnan(h[5, 0]).all()) and bool(torch.isnan(t[700]).all())
    assert bool(torch.isinf(h[300, H - 1]).all()) and not bool(torch.isfinite(t[300]).any())
    if H > 1:                                                           # inside the row the other heads are untouched
        assert np.array_equal(bits(h[5, 1:]), bits(big_h[5, 1:])) and np.array_equal(bits(h[300, :H - 1]), bits(big_h[300, :H - 1]))


def test_the_wrapper_is_the_call(dev):
    """functional.attn_contrib on strided views: the same bits, contiguous outputs, no host synchronisation."""
    H, C = 4, 3
    E, attn, U = device_inputs(H, torch.float32, "random")
    Uc = U[:C].contiguous()
    want_t, _, want_h = launch(E, attn, Uc, TMAX, H, C, True, C, dev)
    cu = torch.tensor([0, 10, TMAX], device=dev)
    MF.contrib_stats(want_t, cu)                                        # warm-up: the allocator
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        total, heads = MF.attn_contrib(E, attn, Uc, per_head=True)
        lean = MF.attn_contrib(E, attn, Uc)
        st = MF.contrib_stats(total, cu)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert total.shape == (TMAX, C) and heads.shape == (TMAX, H, C) and total.is_contiguous() and st.shape == (2, 4, C)
    assert np.array_equal(bits(total), bits(want_t)) and np.array_equal(bits(heads), bits(want_h)) and np.array_equal(bits(lean), bits(want_t))
    empty = MF.attn_contrib(E[:0], attn[:0], Uc, per_head=True)
    assert empty[0].shape == (0, C) and empty[1].shape == (0, H, C)
    with pytest.raises(NotImplementedError, match="1..8 decision columns"):
        MF.attn_contrib(E, attn, torch.zeros(9, H * W, device=dev))
    with pytest.raises(RuntimeError, match="attn_contrib needs"):
        MF.attn_contrib(E, attn[:, :2], Uc)


# ------------------------------------------------------------------------------------------------ extents
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("H,C,T", [(4, 3, 257), (1, 8, 65), (8, 5, 63), (2, 1, 1025)])
def test_the_calls_stay_inside_their_stated_extents(dev, H, C, T, dtype):
    """Every buffer at exactly the extent the header states, carved from one guarded arena, under both fills: no byte outside changes
    (the padding columns of total included), the inputs are only read, and the outputs do not depend on the fill."""
    E, attn, U = inputs(H, dtype, "random")
    ldE, ldA, ldO = H * W + 8, H + 3, C + 1
    lens = [0, T // 3, T - T // 3]
    cu_host = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64)
    R = len(lens)
    n_ws = int(MF._entry("mdl_contrib_stats_ws_bytes")(T, R, C))
    assert n_ws > 0
    spec = [("E", ((T - 1) * ldE + H * W,), dtype, "in"), ("attn", ((T - 1) * ldA + H,), torch.float32, "in"),
            ("U", (C, H * W), torch.float32, "in"), ("cu", (R + 1,), torch.int64, "in"), ("per_head", (T, H, C), torch.float32, "out"),
            ("total", ((T - 1) * ldO + C,), torch.float32, "out"), ("stats", (R, 4, C), torch.float32, "out"),
            ("ws", (n_ws,), torch.uint8, "ws")]
    got = {}
    for fill in FILLS:
        ar = Arena(dev, fill)
        for name, shape, dt, role in spec:
            ar.reserve(name, shape, dt, role)
        ar.allocate()
        b = {name: ar.take(name, shape, dt, role) for name, shape, dt, role in spec}
        # rows of the inputs at their strides; the bytes between the rows keep the fill
        torch.as_strided(b["E"], (T, H * W), (ldE, 1)).copy_(E[:T])
        torch.as_strided(b["attn"], (T, H), (ldA, 1)).copy_(attn[:T])
        b["U"].copy_(U[:C])
        b["cu"].copy_(cu_host)
        ar.seal()
        before = b["total"].clone()
        MF._call("mdl_attn_contrib", b["E"], ldE, 1 if dtype == torch.bfloat16 else 0, b["attn"], ldA, b["U"], T, H, W, C, b["per_head"],
                 b["total"], ldO, MF._stream())
        MF._call("mdl_contrib_stats", b["total"], ldO, b["cu"], T, R, C, b["stats"], b["ws"], MF._stream())
        torch.cuda.synchronize()
        ar.check()
        pad, pad0 = (x[:(T - 1) * ldO].view(T - 1, ldO)[:, C:].contiguous().cpu().view(torch.uint8) for x in (b["total"], before))
        assert pad.numel() == 4 * (T - 1) * (ldO - C) and torch.equal(pad, pad0), "the padding columns of total keep the fill"
        got[fill] = (torch.as_strided(b["total"], (T, C), (ldO, 1)).clone(), b["per_head"].clone(), b["stats"].clone())
        assert not any(bool(torch.isnan(x).any()) for x in got[fill])
    for x, y in zip(got[FILLS[0]], got[FILLS[1]]):
        assert np.array_equal(bits(x), bits(y))
    ph64, tot64, aph, atot = reference(H, dtype, "random", C)
    assert bool((np.abs(got[FILLS[0]][0].cpu().numpy() - tot64[:T]) <= (H * W + 4) * U23 * atot[:T]).all())
    assert not bool(got[FILLS[0]][2][0].any())                          # the empty bag


# ------------------------------------------------------------------------------------------------ X2
LENS = [0, 1, 1023, 1024, 1025, 3000]
ROWS = MF.CONTRIB_ROWS


def cu_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def stat_inputs(kind, C):
    g = torch.Generator().manual_seed(7 + C + (100 if kind == "integer" else 0))
    n = sum(LENS)
    c = torch.randint(-8, 9, (n, C), generator=g).float() if kind == "integer" else torch.randn(n, C, generator=g) * 3
    return c


@pytest.mark.parametrize("C", [1, 3, 8])
def test_stats_are_exact_on_integers(dev, C):
    """Bags of 0, 1, 1023, 1024, 1025 and 3000 rows in one call, ld = C + 1, terms in [-8, 8]: every statistic equals fp64 numpy."""
    assert ROWS == 1024
    c = stat_inputs("integer", C)
    want, _ = ref.stats(c.numpy(), cu_of(LENS))
    st = MF.contrib_stats(strided(c, 1, dev), torch.from_numpy(cu_of(LENS)).to(dev))
    assert st.shape == (len(LENS), 4, C) and st.dtype == torch.float32
    assert np.array_equal(st.cpu().numpy().astype(np.float64), want)
    assert not bool(st[0].any()), "an empty bag gives zeros"


@pytest.mark.parametrize("C", [1, 3, 8])
def test_stats_within_the_summation_bound_and_bag_local(dev, C):
    """Random data: the three sums within (n + 4) 2^-23 sum |c| of fp64, max |.| exact; the bits of a bag are the same alone, in the
    pack, in another order and at another stride."""
    c = stat_inputs("random", C)
    cu = cu_of(LENS)
    want, scale = ref.stats(c.numpy(), cu)
    cd = c.to(dev)
    st = MF.contrib_stats(cd, torch.from_numpy(cu).to(dev))
    got = st.cpu().numpy().astype(np.float64)
    worst = 0.0
    for r, n in enumerate(LENS):
        bound = (n + 4) * U23 * scale[r]
        for s in range(3):
            err = np.abs(got[r, s] - want[r, s])
            assert bool((err <= bound).all()), (n, s, err, bound)
            if n:
                worst = max(worst, float((err / bound).max()))
        assert np.array_equal(got[r, 3], want[r, 3]), n
    print("contrib_stats C %d: worst error / bound %.4f" % (C, worst))
    for r, n in enumerate(LENS):                                        # every bag alone: R = 1
        alone = MF.contrib_stats(cd[cu[r]:cu[r + 1]], torch.tensor([0, n], device=dev))
        assert np.array_equal(bits(alone[0]), bits(st[r])), n
    perm = [4, 0, 5, 2, 1, 3]
    rows = np.concatenate([np.arange(cu[i], cu[i + 1]) for i in perm])
    again = MF.contrib_stats(strided(c[rows], 3, dev), torch.from_numpy(cu_of([LENS[i] for i in perm])).to(dev))
    assert np.array_equal(bits(again), bits(st[perm]))


def test_stats_nan_rule_and_bags_outside_the_pack(dev):
    """A NaN reaches the sum, max |.| and the signed sum its sign bit names; an Inf is an ordinary term; a bag that runs backwards or
    leaves [0, T] is an empty bag."""
    c = torch.tensor([[1.0, 2.0], [float("nan"), -3.0], [-2.0, float("inf")], [4.0, -1.0], [-float("nan"), 5.0]])
    c[4, 0] = torch.tensor(np.array([0xFFC00000], np.uint32).view(np.float32))[0]      # a NaN with its sign bit set
    cu = torch.tensor([0, 3, 2, 9, 3, 5], dtype=torch.int64)              # valid: [0, 3) and [3, 5)
    st = MF.contrib_stats(c.to(dev), cu.to(dev)).cpu()
    assert not bool(st[[1, 2, 3]].any())
    a, b = st[0], st[4]
    assert torch.isnan(a[0, 0]) and torch.isnan(a[1, 0]) and a[2, 0] == -2.0 and torch.isnan(a[3, 0])
    assert torch.isinf(a[0, 1]) and a[1, 1] == float("inf") and a[2, 1] == -3.0 and a[3, 1] == float("inf")
    assert torch.isnan(b[0, 0]) and b[1, 0] == 4.0 and torch.isnan(b[2, 0]) and torch.isnan(b[3, 0])
    assert b[:, 1].tolist() == [4.0, 5.0, -1.0, 5.0]
    zero = MF.contrib_stats(torch.zeros(0, 2, device=dev), torch.zeros(4, dtype=torch.int64, device=dev))
    assert zero.shape == (3, 4, 2) and not bool(zero.any())
