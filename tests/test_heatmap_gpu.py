"""The heatmap renderer on the GPU (V1, include/madeleine_amd_view.h): mdl_heat_render against the numpy int64 / uint64 restatement of
tests/_heat_ref.py BIT FOR BIT (level, covered, rgba) -- footprints, contention, bags, canvases and blur radii, channels and strides,
every class of value, the colour step -- its stated buffer extents in the guarded arena of tests/_arena.py, and
DeviceSlideStore.heatmaps against heatmap.render fed from store.attention + store.coords_of.  The shapes are the smallest at which each
mechanism can go wrong: both sides of the 32-pixel tile and of the 64-lane wave, canvases narrower than the blur radius, several tiles."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from madeleine_amd import functional as MF
from madeleine_amd import heatmap as HM
from madeleine_amd.store import DeviceSlideStore
from oracle import recipe
from tests import _heat_ref as HR
from tests._arena import FILLS, Arena

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def distinct_lut(seed=0):
    """[256, 4] uint8 with 256 distinct entries in every column."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(256) for _ in range(4)], 1).astype(np.uint8)


GRAY = np.stack([np.arange(256)] * 3 + [np.full(256, 255)], 1).astype(np.uint8)


def box_taps(r):
    """A box of 2 r + 1 equal taps, the remainder of 4096 on the centre: nothing like a Gaussian, so a wrong halo or tap order shows."""
    n = 2 * r + 1
    t = [4096 // n] * n
    t[r] += 4096 - sum(t)
    return t


def tent_taps(r):
    """Symmetric, rising towards the centre by uneven steps."""
    half = [1 + k * k // 8 for k in range(r)]             # r = 32: 2 * 1,328 beside a centre of 1,440
    return half + [4096 - 2 * sum(half)] + half[::-1]


def records_of(canvases):
    """[R, 6] int64 from per-bag (ps, ox, oy, W, H): the canvases back to back."""
    rec = torch.zeros(len(canvases), 6, dtype=torch.int64)
    off = 0
    for b, (ps, ox, oy, W, H) in enumerate(canvases):
        rec[b] = torch.tensor([ps, ox, oy, W, H, off])
        off += W * H
    return rec, off


def device_render(dev, xy, cu, values, canvases, ds, taps, lut, alpha, bases=None, ld=None):
    """mdl_heat_render through functional.heat_render; per bag (level, covered, rgba) as device tensors."""
    rec, P = records_of(canvases)
    v = values if torch.is_tensor(values) else torch.from_numpy(np.asarray(values, dtype=np.float32))
    T, C = v.shape
    if torch.is_tensor(values):                               # the caller's own view of the values on the device, at its row stride
        assert ld is None and v.is_cuda
    elif ld is not None:                                      # a wider row, NaN between the rows
        wide = torch.full((T, ld), float("nan"))
        wide[:, :C] = v
        v = wide.to(dev)[:, :C]
    else:
        v = v.to(dev)
    under = None
    if bases is not None:
        under = torch.cat([torch.from_numpy(b).reshape(-1, 3) for b in bases]).to(dev)
    level, covered, rgba = MF.heat_render(torch.from_numpy(np.asarray(xy, dtype=np.int32).reshape(-1, 2)).to(dev),
                                          torch.tensor(cu, dtype=torch.int64, device=dev), v, rec, P, ds,
                                          torch.tensor(taps, dtype=torch.int32), torch.from_numpy(lut).to(dev), alpha, under)
    out = []
    for ps, ox, oy, W, H, off in rec.tolist():
        n = W * H
        out.append((level[C * off:C * (off + n)].view(C, H, W), covered[C * off:C * (off + n)].view(C, H, W),
                    rgba[C * off:C * (off + n)].view(C, H, W, 4)))
    return out


def same_bits(got, want, what=""):
    """(level, covered, rgba) of the device against a _heat_ref.render_bag result, bit for bit."""
    level, covered, rgba = got
    dev = level.device
    assert torch.equal(level.view(torch.int16), torch.from_numpy(want["level"].view(np.int16)).to(dev)), "level " + what
    assert torch.equal(covered, torch.from_numpy(want["covered"]).to(dev)), "covered " + what
    assert torch.equal(rgba, torch.from_numpy(want["rgba"]).to(dev)), "rgba " + what


def check(dev, xy, cu, values, canvases, ds, taps, lut=GRAY, alpha=255, bases=None, ld=None):
    got = device_render(dev, xy, cu, values, canvases, ds, taps, lut, alpha, bases, ld)
    want = HR.render(xy, cu, values, canvases, ds, taps, lut, alpha, bases)
    assert len(got) == len(want) == len(canvases)
    for b, (g, w) in enumerate(zip(got, want)):
        same_bits(g, w, "of bag %d" % b)
    return got, want


# ---- footprints ------------------------------------------------------------------------------------------------------------------------
def test_one_pixel_per_patch_on_an_aligned_grid(dev):
    gx, gy = np.meshgrid(np.arange(40), np.arange(33))
    xy = np.stack([gx.ravel(), gy.ravel()], 1) * 16
    v = np.random.default_rng(1).random((xy.shape[0], 1), dtype=np.float32)
    _, want = check(dev, xy, [0, xy.shape[0]], v, [(16, 0, 0, 40, 33)], 16, [4096])
    assert int(want[0]["N"].max()) == 1 and int(want[0]["N"].min()) == 1          # exactly one patch per pixel


def test_half_overlap_with_ds_dividing_nothing(dev):
    gx, gy = np.meshgrid(np.arange(30), np.arange(21))
    xy = np.stack([gx.ravel(), gy.ravel()], 1) * 8 + 3        # stride ps / 2, coordinates no multiple of ds
    v = np.random.default_rng(2).random((xy.shape[0], 2), dtype=np.float32)
    W, H = (3 + 29 * 8 + 15) // 5 + 1, (3 + 20 * 8 + 15) // 5 + 1
    _, want = check(dev, xy, [0, xy.shape[0]], v, [(16, 0, 0, W, H)], 5, [4096])
    assert int(want[0]["N"].max()) >= 4 and int(want[0]["N"].min()) >= 1      # overlapping footprints, every pixel under one at least


def test_patches_smaller_than_a_pixel(dev):
    rng = np.random.default_rng(3)
    xy = rng.integers(0, 700, (900, 2))
    check(dev, xy, [0, 900], rng.random((900, 1), dtype=np.float32), [(3, 0, 0, 101, 101)], 7, [4096])


def test_patches_across_and_beyond_every_edge_of_a_shifted_canvas(dev):
    """Origin (100, 90), canvas 13 x 9 at ds = 8: level-0 window [100, 204) x [90, 162).  Patches of 20 pixels straddle every edge and
    corner, lie wholly outside on every side (negative numerators: floor, not truncation, decides) and just touch / just miss."""
    edge_x = [60, 79, 80, 81, 85, 99, 100, 150, 190, 203, 204, 230]
    edge_y = [50, 69, 70, 71, 89, 90, 120, 150, 161, 162, 190]
    xy = np.array([(x, y) for x in edge_x for y in edge_y])
    v = np.random.default_rng(4).random((xy.shape[0], 1), dtype=np.float32)
    _, want = check(dev, xy, [0, xy.shape[0]], v, [(20, 100, 90, 13, 9)], 8, [4096])
    # x = 80 (reaches 99) misses, x = 81 touches pixel 0; truncation instead of floor would put x = 79 .. 80 on pixel 0 as well
    lone = HR.render_bag([[80, 120], [204, 120], [150, 70], [150, 162]], np.ones((4, 1), np.float32), 20, 100, 90, 13, 9, 8, [4096], GRAY, 255)
    assert int(lone["N"].sum()) == 0
    check(dev, [[80, 120], [204, 120], [150, 70], [150, 162], [81, 161]], [0, 5], np.ones((5, 1), np.float32), [(20, 100, 90, 13, 9)], 8,
          box_taps(1))


# ---- contention ------------------------------------------------------------------------------------------------------------------------
def test_hundreds_of_patches_on_one_pixel_and_heavy_random_overlap(dev):
    rng = np.random.default_rng(5)
    pile = np.tile(np.array([[77, 45]]), (400, 1))             # 400 patches on one place
    xy = np.concatenate([pile, rng.integers(0, 250, (5600, 2))])
    v = rng.random((6000, 2), dtype=np.float32)
    _, want = check(dev, xy, [0, 6000], v, [(64, 0, 0, 40, 40)], 8, HM.gaussian_taps(1.0).tolist())
    assert int(want[0]["N"].max()) >= 400


# ---- bags ------------------------------------------------------------------------------------------------------------------------------
BAG_LENS = [1, 0, 63, 64, 65, 3000, 200]
BAG_PS = [16, 16, 24, 7, 16, 32, 40]


def _bags(seed=6):
    rng = np.random.default_rng(seed)
    xy = np.concatenate([rng.integers(0, 600, (n, 2)) for n in BAG_LENS])
    v = rng.random((sum(BAG_LENS), 2), dtype=np.float32)
    canv = [(ps, 0, 0, 70 + 3 * b, 66 - b) for b, ps in enumerate(BAG_PS)]
    return xy, v, np.concatenate([[0], np.cumsum(BAG_LENS)]).tolist(), canv


def test_seven_bags_in_one_call_and_each_alone(dev):
    xy, v, cu, canv = _bags()
    taps = tent_taps(3)
    got, _ = check(dev, xy, cu, v, canv, 9, taps)              # an empty bag between two others, a patch size per bag
    for b in (0, 1, 5):                                        # R = 1: the same bag alone, as rows 0 .. n - 1 of its own arrays
        a, e = cu[b], cu[b + 1]
        alone, _ = check(dev, xy[a:e], [0, e - a], v[a:e], [canv[b]], 9, taps)
        for x, y in zip(alone[0], got[b]):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), b
    assert int(got[1][1].sum()) == 0 and int(got[1][2].sum()) == 0      # the empty bag: nothing covered, transparent


# ---- canvas and blur -------------------------------------------------------------------------------------------------------------------
CANVASES = [(1, 1), (3, 3), (1, 65), (63, 64), (64, 65), (65, 63), (200, 150), (3, 1)]


@pytest.mark.parametrize("r, kind", [(0, "box"), (1, "box"), (8, "box"), (32, "box"), (8, "tent"), (32, "tent"), (5, "gauss")])
def test_canvas_sizes_and_blur_radii(dev, r, kind):
    """Every canvas as one bag of the same call: W < r, H < r, both sides of the 32-pixel tile, several tiles each way."""
    rng = np.random.default_rng(7)
    taps = {"box": box_taps, "tent": tent_taps}[kind](r) if kind != "gauss" else HM.gaussian_taps(1.7, r).tolist()
    assert len(taps) == 2 * r + 1 and sum(taps) == 4096
    xy, lens = [], []
    for W, H in CANVASES:
        n = max(1, min(600, W * H // 3))                       # sparse enough that uncovered pixels remain beside covered ones
        xy.append(np.stack([rng.integers(0, W * 4, n), rng.integers(0, H * 4, n)], 1))
        lens.append(n)
    xy = np.concatenate(xy)
    v = rng.random((xy.shape[0], 1), dtype=np.float32)
    canv = [(6 if W > 3 else 4, 0, 0, W, H) for W, H in CANVASES]
    _, want = check(dev, xy, np.concatenate([[0], np.cumsum(lens)]).tolist(), v, canv, 4, taps, lut=distinct_lut(1))
    assert any(0 < int(w["covered"].sum()) < w["covered"].size for w in want)


# ---- channels and stride ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 4, 5])
@pytest.mark.parametrize("pad", [0, 3])
def test_channels_and_row_stride(dev, C, pad):
    rng = np.random.default_rng(8 + C)
    xy = rng.integers(0, 500, (700, 2))
    v = rng.random((700, C), dtype=np.float32)
    check(dev, xy, [0, 300, 700], v, [(32, 0, 0, 67, 67), (32, 10, 10, 33, 70)], 8, box_taps(2), ld=C + pad if pad else None)


# ---- values ----------------------------------------------------------------------------------------------------------------------------
def test_every_class_of_value(dev):
    """One pixel per patch, so that level is the quantiser itself: NaN, both infinities, both zeros, negatives, above one, denormals,
    exact half-way points of rint (k + 0.5) / 65535 where the fp32 product is exact, and the last number below one.  Channel 1 is all
    NaN: nothing of it is covered."""
    half = [np.float32(k + 0.5) / np.float32(65535) for k in (0, 1, 2, 3, 100, 101, 32767, 65533, 65534)]
    special = [np.nan, -np.inf, np.inf, -0.0, 0.0, -1.0, -1e-30, 1e-45, 1e-30, 7.6e-6, 7.7e-6, 0.25, 0.5, 0.75, 1.0 - 2.0 ** -24, 1.0,
               1.0 + 2.0 ** -23, 3.0, 1e30] + half
    rng = np.random.default_rng(9)
    col = np.concatenate([np.array(special, dtype=np.float32), rng.random(256 - len(special), dtype=np.float32)])
    v = np.stack([col, np.full(256, np.nan, dtype=np.float32), col[::-1]], 1)
    gx, gy = np.meshgrid(np.arange(16), np.arange(16))
    xy = np.stack([gx.ravel(), gy.ravel()], 1) * 10
    got, want = check(dev, xy, [0, 256], v, [(10, 0, 0, 16, 16)], 10, [4096], lut=distinct_lut(2))
    q, keep = HR.quantise(col)
    assert np.array_equal(want[0]["level"][0].ravel(), q.astype(np.uint16)) and not keep[0] and want[0]["covered"][0].ravel()[0] == 0
    level, covered, rgba = got[0]
    assert not bool(covered[1].any()) and not bool(level.view(torch.int16)[1].any()) and not bool(rgba[1].any())      # the NaN channel
    check(dev, xy, [0, 256], v, [(10, 0, 0, 16, 16)], 10, box_taps(2), lut=distinct_lut(2))                   # ... and blurred


# ---- colour ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [0, 1, 128, 255])
@pytest.mark.parametrize("with_base", [False, True])
def test_colour(dev, alpha, with_base):
    """1,024 one-pixel patches whose levels run through all 65,536 / 64 steps: every index of a LUT with 256 distinct entries a column."""
    gx, gy = np.meshgrid(np.arange(40), np.arange(30))
    xy = np.stack([gx.ravel(), gy.ravel()], 1)[:1100] * 4     # the last 100 pixels stay uncovered
    v = (np.arange(1100, dtype=np.float32) / np.float32(1099)).reshape(-1, 1)
    rng = np.random.default_rng(10)
    bases = [rng.integers(0, 256, (30, 40, 3), dtype=np.uint8)] if with_base else None
    _, want = check(dev, xy, [0, 1100], v, [(4, 0, 0, 40, 30)], 4, [4096], lut=distinct_lut(3), alpha=alpha, bases=bases)
    idx = (want[0]["level"].astype(np.int64) * 255 + 32767) // 65535
    assert set(idx[want[0]["covered"] > 0].tolist()) == set(range(256))
    assert int((want[0]["covered"] == 0).sum()) == 100


# ---- extents ---------------------------------------------------------------------------------------------------------------------------
def _arena_render(dev, fill, with_base, tamper=None):
    """mdl_heat_render twice on buffers of a guarded arena at exactly the sizes the header states; the arena is checked after each run.
    tamper(rec) -> the DEVICE copy of the records, where it shall differ from bag_host.  Returns the outputs of both runs and what
    the reference needs."""
    xy, v, cu, canv = _bags(11)
    rec, P = records_of(canv)
    T, C, R, ld, ds = xy.shape[0], 2, len(canv), 5, 9
    taps = torch.tensor(tent_taps(8), dtype=torch.int32)
    lut = distinct_lut(4)
    base = np.random.default_rng(12).integers(0, 256, (P, 3), dtype=np.uint8)
    lib = MF._native.lib()
    ws_bytes = lib.mdl_heat_ws_bytes(P, R, C)
    assert ws_bytes > 0
    spec = [("xy", (T, 2), torch.int32, "in"), ("cu", (R + 1,), torch.int64, "in"), ("values", ((T - 1) * ld + C,), torch.float32, "in"),
            ("bag", (R, 6), torch.int64, "in"), ("lut", (256, 4), torch.uint8, "in"), ("level", (C * P,), torch.int16, "out"),
            ("covered", (C * P,), torch.uint8, "out"), ("rgba", (C * P, 4), torch.uint8, "out"), ("ws", (ws_bytes,), torch.uint8, "ws")]
    if with_base:
        spec.append(("base", (P, 3), torch.uint8, "in"))
    arena = Arena(dev, fill)
    for name, shape, dtype, role in spec:
        arena.reserve(name, shape, dtype, role, pitch=C * 200 * 8 if role == "ws" else None)
    arena.allocate()
    buf = {name: arena.take(name, shape, dtype, role) for name, shape, dtype, role in spec}
    buf["xy"].copy_(torch.from_numpy(xy.astype(np.int32)))
    buf["cu"].copy_(torch.tensor(cu))
    rows = torch.full((T, ld), float("nan"))
    rows[:, :C] = torch.from_numpy(v)
    buf["values"].copy_(rows.reshape(-1)[:(T - 1) * ld + C])
    buf["bag"].copy_(rec if tamper is None else tamper(rec.clone()))
    buf["lut"].copy_(torch.from_numpy(lut))
    if with_base:
        buf["base"].copy_(torch.from_numpy(base))
    arena.seal()
    stream = torch.cuda.current_stream().cuda_stream
    runs = []
    for _ in range(2):
        rc = lib.mdl_heat_render(buf["xy"].data_ptr(), buf["cu"].data_ptr(), buf["values"].data_ptr(), ld, T, R, C, rec.data_ptr(),
                                 buf["bag"].data_ptr(), P, ds, taps.data_ptr(), 8, buf["lut"].data_ptr(),
                                 buf["base"].data_ptr() if with_base else None, 200, buf["level"].data_ptr(), buf["covered"].data_ptr(),
                                 buf["rgba"].data_ptr(), buf["ws"].data_ptr(), stream)
        assert rc == 0
        torch.cuda.synchronize()
        arena.check()
        runs.append([buf[k].clone() for k in ("level", "covered", "rgba")])
    for x, y in zip(*runs):
        assert torch.equal(x, y)
    want = HR.render(xy, cu, v, canv, ds, taps.tolist(), lut, 200,
                     [base[o:o + W * H].reshape(H, W, 3) for _, _, _, W, H, o in rec.tolist()] if with_base else None)
    return runs[0], rec, want, C


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("with_base", [False, True])
def test_the_render_stays_inside_the_extents_the_header_states(dev, fill, with_base):
    """Every buffer at exactly the size include/madeleine_amd_view.h gives, carved from one guarded arena: the guards stay intact, the
    inputs unchanged, the workspace needs no initialisation (it holds the fill), and two runs agree bit for bit."""
    run, rec, want, C = _arena_render(dev, fill, with_base)
    for (ps, ox, oy, W, H, off), w in zip(rec.tolist(), want):
        n = W * H
        same_bits((run[0][C * off:C * (off + n)].view(C, H, W).view(torch.uint16), run[1][C * off:C * (off + n)].view(C, H, W),
                   run[2][C * off:C * (off + n)].view(C, H, W, 4)), w)


@pytest.mark.parametrize("fill", FILLS)
def test_a_device_record_that_differs_from_the_host_record_touches_nothing_outside(dev, fill):
    """The header's promise for a device copy of the records that is not the host's: bag 3's canvas would leave the planes (served as an
    empty canvas: its blocks keep the fill), bag 5 claims a taller canvas than the grids were sized for (the tile table saturates),
    bag 6 a record that does not hold at all.  The call returns MDL_OK, every guard stays intact and every input unchanged
    (_arena_render checks the arena after both runs); the bags before the first difference are still the reference's."""
    def tamper(rec):
        P = int(rec[-1, 5] + rec[-1, 3] * rec[-1, 4])
        rec[3, 5] = P - int(rec[3, 3] * rec[3, 4]) + 1        # off + W * H = P + 1
        rec[5, 4] += 40                                       # H: more tiles than the host counted, still inside the planes
        rec[6, 0] = 0                                         # ps < 1
        return rec
    run, rec, want, C = _arena_render(dev, fill, False, tamper)
    for b in range(3):
        ps, ox, oy, W, H, off = rec[b].tolist()
        n = W * H
        same_bits((run[0][C * off:C * (off + n)].view(C, H, W).view(torch.uint16), run[1][C * off:C * (off + n)].view(C, H, W),
                   run[2][C * off:C * (off + n)].view(C, H, W, 4)), want[b])
    _, _, _, W, H, off = rec[3].tolist()
    assert bool((run[1][C * off:C * (off + W * H)] == fill).all()) and bool((run[2][C * off:C * (off + W * H)] == fill).all())


def test_three_hundred_canvases_cross_the_slices_of_the_tile_table_scan(dev):
    """R = 300 > the 256 records a slice of hv_plan's scan holds: the carry between slices.  Mostly 1 x 1 canvases, every 37th of more
    than one tile, every 5th bag empty."""
    rng = np.random.default_rng(16)
    canv = [(8, 0, 0, 70, 35) if b % 37 == 36 else (8, 0, 0, 1, 1) for b in range(300)]
    lens = [0 if b % 5 == 4 else (40 if b % 37 == 36 else 2) for b in range(300)]
    xy = np.concatenate([rng.integers(0, 8 * W, (n, 2)) for n, (_, _, _, W, _) in zip(lens, canv)])
    v = rng.random((xy.shape[0], 1), dtype=np.float32)
    check(dev, xy, np.concatenate([[0], np.cumsum(lens)]).tolist(), v, canv, 8, box_taps(1))


def test_the_marked_call_gives_the_same_images_and_four_stage_times(dev):
    xy, v, cu, canv = _bags(17)
    rec, P = records_of(canv)
    args = (torch.from_numpy(xy.astype(np.int32)).to(dev), torch.tensor(cu, device=dev), torch.from_numpy(v).to(dev), rec, P, 9,
            torch.tensor(tent_taps(4), dtype=torch.int32), torch.from_numpy(GRAY).to(dev), 255)
    plain = MF.heat_render(*args)
    level, covered, rgba, ms = MF.heat_render_stages(*args)
    assert torch.equal(level.view(torch.int16), plain[0].view(torch.int16)) and torch.equal(covered, plain[1]) and torch.equal(rgba, plain[2])
    assert tuple(ms) == MF.HEAT_STAGES and all(0.0 <= t < 1e3 for t in ms.values())


# ---- the Python planner ----------------------------------------------------------------------------------------------------------------
def test_render_plans_the_canvases_and_does_not_depend_on_the_grouping(dev):
    xy, v, cu, _ = _bags(13)
    xy_d = torch.from_numpy(xy.astype(np.int32)).to(dev)
    cu_d, v_d = torch.tensor(cu, device=dev), torch.from_numpy(v).to(dev)
    ext = HM.coord_extents(xy_d, cu_d)
    for b, n in enumerate(BAG_LENS):
        seg = xy[cu[b]:cu[b + 1]]
        assert ext[b].tolist() == ([0, 0, -1, -1] if n == 0 else [seg[:, 0].min(), seg[:, 1].min(), seg[:, 0].max(), seg[:, 1].max()])
    for crop in (False, True):
        out = HM.render(xy_d, cu_d, v_d, BAG_PS, 11, sigma=1.5, cmap="coolwarm", alpha=180, crop=crop)
        plan = HM.plan_canvases(ext, BAG_PS, 11, crop).tolist()
        assert out["canvas"] == [(W, H, ox, oy) for _, ox, oy, W, H in plan] and out["downsample"] == 11
        want = HR.render(xy, cu, v, plan, 11, HM.gaussian_taps(1.5).tolist(), HM.colormap("coolwarm").numpy(), 180)
        for b, w in enumerate(want):
            same_bits((out["level"][b], out["covered"][b], out["rgba"][b]), w, "of bag %d" % b)
            if BAG_LENS[b]:                                   # the canvas ends with the last pixel a footprint touches
                assert w["covered"][0, :, -1].any() and w["covered"][0, -1, :].any()
        for budget in (1, 700_000, 1 << 21):                  # every bag alone | pairs of bags | one group: ~290 KB a canvas
            again = HM.render(xy_d, cu_d, v_d, BAG_PS, 11, sigma=1.5, cmap="coolwarm", alpha=180, crop=crop, extents=ext, max_bytes=budget)
            assert again["canvas"] == out["canvas"]
            for k in ("level", "covered", "rgba"):
                assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(again[k], out[k])), (k, budget)
    with pytest.raises(NotImplementedError):
        HM.render(xy_d, cu_d, v_d, BAG_PS, 11, taps=[0] * 33 + [4096] + [0] * 33)


# ---- the store path --------------------------------------------------------------------------------------------------------------------
MODS = ["HE", "HER2"]
ENC_D = 96
ENC_LENS = [[7, 300], [256, 257], [257, None], [300, 7], [1025, 256]]
ENC_PS = 64


def _model(dev, tag="heat"):
    from madeleine_amd import MADELEINE
    cfg = SimpleNamespace(MODALITIES=list(MODS), wsi_encoder="abmil", patch_embedding_dim=ENC_D, wsi_encoder_hidden_dim=512,
                          activation="softmax", n_heads=4)
    m = MADELEINE(cfg, stain_encoding=False)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.state_dict_recipe(shapes, tag).items()}, strict=True)
    return m.to(dev).eval()


def _enc_coords():
    """A jittered grid with half overlap: stride ps / 2 plus up to 5 pixels, 40 patches a row."""
    rng = np.random.default_rng(14)
    out = []
    for case in ENC_LENS:
        out.append([None if n is None else
                    np.stack([(np.arange(n) % 40) * (ENC_PS // 2) + 200, (np.arange(n) // 40) * (ENC_PS // 2) + 100], 1)
                    + rng.integers(0, 6, (n, 2)) for n in case])
    return out


def _enc_store(dev, **kw):
    bags = [[None if n is None else torch.from_numpy(recipe.uniform((n, ENC_D), "heat:%d:%d" % (c, m))) for m, n in enumerate(case)]
            for c, case in enumerate(ENC_LENS)]
    return DeviceSlideStore(bags, ["case%d" % c for c in range(len(ENC_LENS))], MODS, dev, coords=_enc_coords(), patch_size=ENC_PS, **kw)


@pytest.fixture(scope="module")
def enc(dev):
    stores = {"fp32": _enc_store(dev), "bf16": _enc_store(dev, dtype=torch.bfloat16), "tiered": _enc_store(dev, resident_bytes=600 * ENC_D * 4)}
    assert stores["tiered"].rows_host is not None and 0 < stores["tiered"].resident_rows <= 600
    return SimpleNamespace(store=stores["fp32"], stores=stores, model=_model(dev))


def _same_images(a, b):
    assert a["canvas"] == b["canvas"] and len(a["rgba"]) == len(b["rgba"])
    for k in ("level", "covered", "rgba"):
        for x, y in zip(a[k], b[k]):
            assert x.shape == y.shape and torch.equal(x.view(torch.uint8), y.view(torch.uint8)), k


@pytest.mark.parametrize("kind", ["fp32", "bf16", "tiered"])
@pytest.mark.parametrize("source", ["percentile", "attention", "raw"])
@pytest.mark.parametrize("heads", ["mean", "all", 2])
def test_store_heatmaps_are_render_of_the_attention_read_out(dev, enc, source, heads, kind):
    st, model = enc.stores[kind], enc.model
    res = st.heatmaps(model, source=source, heads=heads, downsample=16, sigma=2.0, crop=True)
    att = st.attention(model)
    n = len(ENC_LENS)
    assert res["cases"].tolist() == list(range(n)) and res["slide_ids"] == ["case%d" % c for c in range(n)]
    assert torch.equal(res["embeds"], st.embed(model)["embeds"])
    values = HM.heat_values(att, source, heads)
    C = 4 if heads == "all" else 1
    assert values.shape == (att["raw"].shape[0], C) and torch.equal(values, res["values"])
    xy = st.coords_of(None, 0)
    coords = _enc_coords()
    assert torch.equal(xy.cpu(), torch.from_numpy(np.concatenate([coords[c][0] for c in range(n)]).astype(np.int32)))
    by_hand = HM.render(xy, att["cu_seqlens"], values, ENC_PS, 16, sigma=2.0, crop=True)      # its own host read of the extents
    _same_images(res, by_hand)
    assert all(r.shape[0] == C and r.shape[3] == 4 for r in res["rgba"])
    if source == "percentile":
        src = att["percentile"] / 100.0
        assert torch.equal(values, src.mean(1, keepdim=True) if heads == "mean" else src if heads == "all" else src[:, 2:3])
    else:                                                      # min-max per bag and channel: 0 and 1 are reached in every bag > 1 row
        cu = att["cu_seqlens"].tolist()
        for b in range(n):
            seg = values[cu[b]:cu[b + 1]]
            assert float(seg.min()) == 0.0 and float(seg.max()) == 1.0
    # against the numpy restatement, from the device's values
    cu = att["cu_seqlens"].tolist()
    plan = [(ENC_PS, ox, oy, W, H) for W, H, ox, oy in res["canvas"]]
    want = HR.render(xy.cpu().numpy(), cu, values.cpu().numpy(), plan, 16, HM.gaussian_taps(2.0).tolist(), HM.colormap("jet").numpy(), 255)
    for b, w in enumerate(want):
        same_bits((res["level"][b], res["covered"][b], res["rgba"][b]), w, "of bag %d" % b)


def test_store_heatmaps_options_and_other_stores(dev, enc):
    st, model = enc.store, enc.model
    res = st.heatmaps(model, sigma=1.0)                        # downsample None: the patch size; crop False: origin 0
    assert res["downsample"] == ENC_PS and all(c[2:] == (0, 0) for c in res["canvas"])
    ext = st.coord_extents
    for b, (W, H, _, _) in enumerate(res["canvas"]):
        g = int(st.bag_table[b, 0])
        assert (W, H) == ((int(ext[g, 2]) + ENC_PS - 1) // ENC_PS + 1, (int(ext[g, 3]) + ENC_PS - 1) // ENC_PS + 1)
    for budget in (1, 300_000):                                # the grouping and the byte budget do not show
        _same_images(st.heatmaps(model, sigma=1.0, max_bytes=budget), res)
    _same_images(st.heatmaps(model, sigma=1.0, bags_per_launch=1), res)
    some = st.heatmaps(model, case_indices=[4, 0], sigma=1.0)
    assert some["cases"].tolist() == [4, 0]
    for i, b in enumerate((4, 0)):
        assert torch.equal(some["rgba"][i], res["rgba"][b]) and some["canvas"][i] == res["canvas"][b]
    # thumbnails: blended under the colours, kept where nothing is covered
    thumbs = [torch.from_numpy(np.random.default_rng(15 + b).integers(0, 256, (H, W, 3), dtype=np.uint8)) for b, (W, H, _, _) in
              enumerate(res["canvas"])]
    over = st.heatmaps(model, sigma=1.0, alpha=100, thumbnails=thumbs)
    for b in range(len(thumbs)):
        unc = (over["covered"][b][0] == 0).cpu()
        assert torch.equal(over["rgba"][b][0].cpu()[unc][:, :3], thumbs[b][unc]) and bool((over["rgba"][b][..., 3] == 255).all())
        assert torch.equal(over["level"][b].view(torch.int16), res["level"][b].view(torch.int16))
    second = st.heatmaps(model, modality=1, source="raw", heads="all", downsample=32)
    assert second["cases"].tolist() == [0, 1, 3, 4] and torch.equal(second["embeds"], st.embed(model, modality=1)["embeds"])
    # a bf16 store and a tiered store: heatmaps is render of ITS attention; the tiered store's bits are the resident store's
    half = _enc_store(dev, dtype=torch.bfloat16)
    got = half.heatmaps(model, source="attention", heads="all", downsample=16, sigma=2.0)
    att = half.attention(model)
    assert torch.equal(got["embeds"], half.embed(model)["embeds"])
    _same_images(got, HM.render(half.coords_of(None, 0), att["cu_seqlens"], HM.heat_values(att, "attention", "all"), ENC_PS, 16, sigma=2.0,
                                extents=half.coord_extents.index_select(0, half.bag_table[:, 0].long())))
    tiered = _enc_store(dev, resident_bytes=600 * ENC_D * 4)
    assert tiered.rows_host is not None and tiered.coords.is_cuda and tiered.coords.shape[0] == int(tiered.off_cpu[-1])
    t = tiered.heatmaps(model, sigma=1.0)
    _same_images(t, res)
    assert torch.equal(t["embeds"], res["embeds"]) and torch.equal(t["embeds"], tiered.embed(model)["embeds"])
    with pytest.raises(RuntimeError, match="no coordinates"):
        DeviceSlideStore([[torch.ones(3, ENC_D), None]], ["a"], MODS, dev).heatmaps(model)
    with pytest.raises(ValueError, match="source"):
        st.heatmaps(model, source="softmax")
