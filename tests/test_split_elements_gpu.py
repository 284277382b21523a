"""The split-fp16 engine's images and products, element by element (tests/_split_bounds.py states the contract, the references and every
bound; tests/test_split_bounds_cpu.py holds the checkers to a CPU emulation and to seeded faults).

An image is a decodable object, element = (hi + lo) / scale, and every product a documented expression of the planes.  Each case builds
its images with the kernels under test, holds them to the definition (the scale rule exactly, the element bound at every element, the
planes bit for bit), reads the planes back and references the product in fp64 on the planes the kernel read: only the fp32 accumulation
is left to the bound.  Input kinds: uniform, row_scaled (rows times 2^[-12, 12]), cancelling (the exact result is 0 against a mag of
order 1) and integer (operands of [-7, 7]: bit for bit).  Every 2-D operand and output has a row stride wider than its rows; outputs,
workspaces and the gaps between rows start as NaN (0xFF bytes in an image) and the gaps are asserted untouched.  Shapes that reach a
dispatch path assert it through mdl_dispatch_plan.  No assertion here is a norm.  (The LayerNorm entry points take no row stride: their
images are rows of 4 W bytes, with a guard row behind them.)  379 cases, 15.6 s on an MI355X.

Entry points and the tests that call them:
  mdl_split_image, mdl_split_image_rows                 test_images, and every product test
  mdl_split_tile_absmax                                 test_tile_absmax, test_nt_row_gate, test_tn_chunk_gate
  mdl_split_gemm_nt                                     test_nt, test_nt_row_gate
  mdl_split_gemm_nt_group_bias                          test_nt (the 'group' variants)
  mdl_split_gemm_tn                                     test_tn, test_tn_chunk_gate, test_tn_row_factors_cancel
  mdl_abmil_pool_fwd_img, mdl_abmil_pool_dscores_img    test_pool_img
  mdl_abmil_gate_fwd_split, mdl_abmil_attnpool_bwd_split test_gate, test_gate_two_token_splits, test_gate_fused_pooling_term
  mdl_ln_gelu_drop_fwd_split, mdl_ln_gelu_drop_bwd_split test_ln_images
  mdl_ln_gelu_drop_bwd_split_groups                     test_ln_images_groups
  sp_nt_kernel<*, 2>, sp_tn_kernel<*, 2>                test_two_stage_rings (a fresh child process with MADELEINE_SP_*_STAGES=2)
"""
import os
import subprocess
import sys

import pytest
import torch

from tests import _bf16_bounds as B
from tests import _split_bounds as S
from tests.test_dispatch_edges_gpu import _expect_plan, _poison

pytestmark = pytest.mark.gpu
NAN = float("nan")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _call(name, *args):
    from madeleine_amd import functional as MF
    MF._call(name, *args)


def _nan(dev, *shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=dev)


def _wide(dev, rows, width, pad=4, x=None):
    """An fp32 [rows, width] view of a NaN buffer `pad` floats wider, holding x where given; (view, whole buffer)."""
    buf = _nan(dev, max(rows, 1), width + pad)
    v = buf[:rows, :width]
    if x is not None:
        v.copy_(x.to(dev))
    return v, buf


def _gap_is_nan(buf, width):
    return bool(torch.isnan(buf[:, width:]).all())


class Img:
    """An image the kernels wrote into a 0xFF-filled buffer of row stride 4 K + 32 bytes, with what the host read back of it."""

    def __init__(self, dev, x, rows_scaled=False, pad_rows=0, with_scale=True, what=""):
        rows, K = x.shape
        self.rows, self.K, self.rsb = rows, K, 4 * K + 32
        self.raw = torch.full((rows + pad_rows + 1, self.rsb), 0xFF, dtype=torch.uint8, device=dev)      # (+ 1: a guard row)
        X, xbuf = _wide(dev, rows, K, 4, x)
        self.row_inv = None
        if rows_scaled:
            self.row_inv = _nan(dev, max(rows, 1))[:rows]
            self.scale = _nan(dev, 2) if with_scale else torch.tensor([1.0, 0.0], device=dev)
            _call("mdl_split_image_rows", X, X.stride(0), rows, K, self.raw, self.rsb, pad_rows, self.row_inv, self.scale if with_scale else None,
                  _stream())
        else:
            self.scale = _nan(dev, 2)
            _call("mdl_split_image", X, X.stride(0), rows, K, self.raw, self.rsb, pad_rows, self.scale, _stream())
        torch.cuda.synchronize()
        raw = self.raw.cpu()
        assert bool((raw[:, 4 * K:] == 0xFF).all()) and bool((raw[rows + pad_rows:] == 0xFF).all()), what + ": bytes outside the image rows written"
        assert bool((raw[rows:rows + pad_rows, :4 * K] == 0).all()), what + ": pad rows not zero"
        self.hi, self.lo = S.unpack(raw[:rows], K)
        self.s = float(self.scale[0])
        self.inv_cpu = None if self.row_inv is None else self.row_inv.cpu()

    def check(self, x, what):
        """The scale rule exactly, the element bound, the planes bit for bit."""
        sc = self.scale.cpu()
        if self.row_inv is None:
            S.check_scale(what, sc[0], sc[1], x)
            S.check_image(what, self.hi, self.lo, x, self.s)
        else:
            assert float(sc[0]) == 1.0, what
            S.check_row_inv(what, self.inv_cpu, x)
            zero = x.abs().amax(1) == 0
            assert float(self.inv_cpu[zero].abs().sum()) == 0.0 and float(self.hi[zero].float().abs().sum() + self.lo[zero].float().abs().sum()) == 0.0
            S.check_image(what, self.hi, self.lo, x, S.row_scale_rule(x)[0])

    def planes(self):
        return self.hi, self.lo


# =============================================================================================================================== images
IMG_ROWS = (1, 3, 4, 5, 15, 16, 17, 33)          # the tails of 4 and 2 rows per wave, of 16 and 8 rows per workgroup iteration
IMG_K = (32, 480, 512, 544, 1024, 1056)          # both sides of the limits of the three row-scaled kernels (K <= 512, <= 1024, above)


@pytest.mark.parametrize("kind", S.KINDS4)
@pytest.mark.parametrize("K", IMG_K)
def test_images(dev, K, kind):
    """mdl_split_image and mdl_split_image_rows at every row count of IMG_ROWS: scale rule, element bound, exact planes, zero pad rows,
    untouched gaps; zero rows (row_inv == 0, a zero image); scale == NULL; the absmax in scale[1] exact."""
    for rows in IMG_ROWS:
        x = S.operand((rows, K), 100 + rows + K, kind)
        if rows >= 3:
            x[rows // 2] = 0.0                     # a zero row inside
        if rows in (4, 17):
            x[rows - 1] = 0.0                      # and as the last row of a wave's group
        what = "image[%dx%d,%s]." % (rows, K, kind)
        Img(dev, x, False, 32, what=what).check(x, what + "common.")
        im = Img(dev, x, True, 32, what=what)
        im.check(x, what + "rows.")
        assert float(im.scale[1]) == float(x.abs().max()), what + "rows.absmax"
        im0 = Img(dev, x, True, 0, with_scale=False, what=what)
        assert torch.equal(im0.hi, im.hi) and torch.equal(im0.lo, im.lo) and torch.equal(im0.inv_cpu, im.inv_cpu), what + "scale == NULL"
    z = torch.zeros(5, K)
    im = Img(dev, z, False, 0)
    assert im.scale.cpu().tolist() == [1.0, 0.0] and float(im.hi.float().abs().sum() + im.lo.float().abs().sum()) == 0.0


@pytest.mark.parametrize("rows", [1, 31, 32, 33, 255, 256, 257])
def test_tile_absmax(dev, rows):
    """mdl_split_tile_absmax: the per-256-row and per-32-row maxima, exactly, with whole zero chunks and a row stride wider than K."""
    K = 36
    x = S.operand((rows, K), 200 + rows, "row_scaled")
    x[40:70] = 0.0
    X, _ = _wide(dev, rows, K, 4, x)
    gate, cm = _nan(dev, (rows + 255) // 256), _nan(dev, (rows + 31) // 32)
    _call("mdl_split_tile_absmax", X, X.stride(0), rows, K, gate, cm, _stream())
    only = _nan(dev, (rows + 255) // 256)
    _call("mdl_split_tile_absmax", X, X.stride(0), rows, K, only, None, _stream())
    pad = lambda n: torch.cat([x, torch.zeros(-rows % n, K)]).view(-1, n * K).abs().amax(1)      # noqa: E731
    S.check_exact("tile_absmax.gate", gate.cpu(), pad(256))
    S.check_exact("tile_absmax.chunks", cm.cpu(), pad(32))
    S.check_exact("tile_absmax.gate (chunk_max NULL)", only.cpu(), pad(256))


# ================================================================================================================================== NT
# every M of {1, 255, 256, 257, 513}, N of {4, 128, 132, 256, 260}, K of {32, 64, 96, 512}; M > 256 with N <= 128: the 512 x 128 tile
NT_SHAPES = ((1, 4, 32), (1, 256, 96), (255, 128, 64), (255, 260, 512), (256, 132, 96), (256, 128, 32), (257, 256, 512), (257, 4, 96),
             (257, 132, 64), (513, 260, 32), (513, 128, 512), (513, 4, 64))
# (A row-scaled, B row-scaled, options): each epilogue argument on its own, then all that the launcher takes together
NT_VARIANTS = ((0, 0, ()), (0, 0, ("bias",)), (0, 0, ("acc",)), (0, 0, ("absmax",)), (1, 0, ()), (0, 1, ()), (0, 0, ("group",)),
               (1, 1, ("bias", "acc", "absmax")), (1, 1, ("bias", "group")))


def _nt_call(dev, A, Bm, case, opts, terms, a_mul=None, gate=None):
    """One mdl_split_gemm_nt / _group_bias call on the images A, Bm -> (C on the host, absmax or None)."""
    M, N, K = A.rows, Bm.rows, A.K
    C, cbuf = _wide(dev, M, N, 4, case["c0"] if "acc" in opts else None)
    bias = case["bias"].to(dev) if "bias" in opts else None
    amax = torch.zeros(1, device=dev) if "absmax" in opts else None
    arm = A.row_inv if a_mul is None else a_mul
    if "group" in opts:
        _call("mdl_split_gemm_nt_group_bias", A.raw, A.rsb, A.scale, Bm.raw, Bm.rsb, Bm.scale, C, C.stride(0), M, N, K, bias, arm, Bm.row_inv,
              case["gb"].to(dev), case["row_group"].to(dev), terms, _stream())
    else:
        _call("mdl_split_gemm_nt", A.raw, A.rsb, A.scale, Bm.raw, Bm.rsb, Bm.scale, C, C.stride(0), M, N, K, bias, int("acc" in opts), amax, gate,
              arm, Bm.row_inv, terms, _stream())
    torch.cuda.synchronize()
    assert _gap_is_nan(cbuf, N), "the gap between the rows of C was written"
    return C.cpu(), (None if amax is None else float(amax))


def _nt_kwargs(A, Bm, case, opts, a_mul=None):
    kw = dict(inv=1.0 / (A.s * Bm.s), a_row_mul=A.inv_cpu if a_mul is None else a_mul, b_col_mul=Bm.inv_cpu)
    if "bias" in opts:
        kw["bias"] = case["bias"]
    if "group" in opts:
        kw["gb_rows"] = case["gb"][case["row_group"].long()]
    if "acc" in opts:
        kw["c0"] = case["c0"]
    return kw


def _nt(dev, M, N, K, kind, variants=NT_VARIANTS, terms_list=(3, 2)):
    case = S.nt_case(M, N, K, 300 + M + N + K, kind)
    if M >= 3:
        case["a"][M // 2] = 0.0                                            # a zero row: row_inv == 0 as a_row_mul
    imgs = {}
    raws = {}
    for a_rows, b_rows, opts in variants:
        for key, x, rows in (("a", case["a"], a_rows), ("b", case["b"], b_rows)):
            if (key, rows) not in imgs:
                imgs[key, rows] = Img(dev, x, bool(rows), what="nt.%s" % key)
        A, Bm = imgs["a", a_rows], imgs["b", b_rows]
        for terms in terms_list:
            if (a_rows, b_rows, terms) not in raws:
                raws[a_rows, b_rows, terms] = S.nt_raw(*A.planes(), *Bm.planes(), terms)
            got, amax = _nt_call(dev, A, Bm, case, opts, terms)
            ref, b1, b2 = S.nt_finish(raws[a_rows, b_rows, terms], terms * K, **_nt_kwargs(A, Bm, case, opts))
            what = "nt[%dx%dx%d,%s,A%dB%d,%s,terms%d]" % (M, N, K, kind, a_rows, b_rows, "+".join(opts) or "plain", terms)
            if kind == "integer":
                S.check_exact(what, got, ref)
            else:
                S.check(what, got, ref, b1, b2)
            if amax is not None:
                assert amax == float(got.abs().max()), what + ": absmax_out is not max |C| as stored"


@pytest.mark.parametrize("kind", S.KINDS4)
@pytest.mark.parametrize("M,N,K", NT_SHAPES)
def test_nt(dev, M, N, K, kind):
    """mdl_split_gemm_nt and mdl_split_gemm_nt_group_bias on the 256 x 256 and the 512 x 128 tile: row and column tails, 1, 2, 3 and 16
    k-blocks (the ring's prologue and drain), bias, accumulate, absmax_out, a_row_mul with a zero row, b_col_mul, a group bias whose
    groups change inside the tiles, 3 and 2 terms."""
    _nt(dev, M, N, K, kind)


@pytest.mark.parametrize("kind", S.KINDS4)
@pytest.mark.parametrize("M,N,K,zero", [(513, 132, 64, (200, 512)), (257, 260, 96, (0, 256)), (513, 128, 32, (0, 300))])
def test_nt_row_gate(dev, M, N, K, zero, kind):
    """row_gate from mdl_split_tile_absmax with all-zero 256-row tiles (a gated call stays on the 256 x 256 tile at N <= 128 too): the
    skipped tiles keep their contents to the bit, the others meet the bound; plain, and with a_row_mul, b_col_mul and absmax_out."""
    case = S.nt_case(M, N, K, 400 + M + N + K, kind)
    case["a"][zero[0]:zero[1]] = 0.0
    X, _ = _wide(dev, M, K, 4, case["a"])
    gate = _nan(dev, (M + 255) // 256)
    _call("mdl_split_tile_absmax", X, X.stride(0), M, K, gate, None, _stream())
    assert int((gate == 0).sum()) == 1
    for rows, opts in ((0, ("acc",)), (1, ("acc", "absmax"))):
        A, Bm = Img(dev, case["a"], bool(rows)), Img(dev, case["b"], bool(rows))
        for terms in (3, 2):
            got, amax = _nt_call(dev, A, Bm, case, opts, terms, gate=gate)
            ref, b1, b2 = S.nt_ref(*A.planes(), *Bm.planes(), terms=terms, **_nt_kwargs(A, Bm, case, opts))
            what = "nt_gate[%dx%dx%d,%s,rows%d,terms%d]" % (M, N, K, kind, rows, terms)
            if kind == "integer":
                S.check_exact(what, got, ref)
            else:
                S.check(what, got, ref, b1, b2)
            skipped = torch.repeat_interleave(gate.cpu() == 0, 256)[:M]
            assert torch.equal(got[skipped], case["c0"][skipped]), what + ": a skipped tile changed"
            if amax is not None:
                assert amax == float(got[~skipped].abs().max()), what + ": absmax_out over the tiles that ran"


# ================================================================================================================================== TN
TN_SHAPES = ((1, 32, 32), (31, 288, 256), (32, 256, 288), (33, 32, 288), (64, 288, 32), (65, 256, 256), (97, 288, 288), (4097, 32, 288),
             (4097, 288, 256))


def _tn_call(dev, A, Bm, chunk_max=None, terms=3):
    from madeleine_amd import _native
    T, Mi, N = A.rows, A.K, Bm.K
    nbytes = _native.lib().mdl_split_gemm_tn_ws_bytes(T, Mi, N)
    assert nbytes >= 0
    _poison(dev, 2 * nbytes + N * Mi * 4 + 4096)
    ws = torch.empty(nbytes // 4 + 16, device=dev)
    out = _nan(dev, N, Mi)
    _call("mdl_split_gemm_tn", A.raw, A.rsb, A.scale, Mi, Bm.raw, Bm.rsb, Bm.scale, N, out, T, chunk_max, ws, terms, _stream())
    torch.cuda.synchronize()
    return out.cpu()


def _tn_check(what, got, A, Bm, terms, kind):
    ref, b1, b2 = S.tn_ref(*A.planes(), *Bm.planes(), 1.0 / (A.s * Bm.s), terms, scaled=kind in ("row_scaled", "decaying"))
    if kind == "integer":
        S.check_exact(what, got, ref)
    else:
        S.check(what, got, ref, b1, b2)


def _tn_plan(T, Mi, N):
    S_ = 2 if T == 4097 else 1
    tps = -(-(-(-T // S_)) // 32) * 32
    _expect_plan("split_tn", T, Mi, N, dict(splits=S_, tps=tps, empty=0, chunk=32))


def _tn(dev, T, Mi, N, kind, terms_list=(3, 2)):
    case = S.tn_case(T, Mi, N, 500 + T + Mi + N, kind)
    A, Bm = Img(dev, case["x"]), Img(dev, case["dy"], pad_rows=32)
    for terms in terms_list:
        _tn_check("tn[T%d,%dx%d,%s,terms%d]" % (T, Mi, N, kind, terms), _tn_call(dev, A, Bm, None, terms), A, Bm, terms, kind)


@pytest.mark.parametrize("kind", S.KINDS4)
@pytest.mark.parametrize("T,Mi,N", TN_SHAPES)
def test_tn(dev, T, Mi, N, kind):
    """mdl_split_gemm_tn: one token, a partial first chunk, one, two and three chunks with partial last ones, two token splits with a
    short last one (T = 4097: 2080 + 2017) and their slab reduction; column tiles of 32, 256 and 288 on either side; 3 and 2 terms."""
    _tn_plan(T, Mi, N)
    _tn(dev, T, Mi, N, kind)


@pytest.mark.parametrize("kind", ["uniform", "integer"])
@pytest.mark.parametrize("T,zero_chunks", [(97, (0, 2, 3)), (97, (0, 1, 2, 3)), (4097, (0, 30, 64, 65, 100, 128)), (4097, tuple(range(129)))],
                         ids=["T97", "T97_all_zero", "T4097", "T4097_all_zero"])
def test_tn_chunk_gate(dev, T, zero_chunks, kind):
    """b_chunk_max from mdl_split_tile_absmax with all-zero 32-token chunks at the start, in the middle and at the end of a split (T = 4097:
    of both splits), and with every chunk zero: the product from the planes, unchanged by the skipping."""
    Mi, N = 288, 32
    _tn_plan(T, Mi, N)
    case = S.tn_case(T, Mi, N, 600 + T, kind)
    for c in zero_chunks:
        case["dy"][32 * c:32 * c + 32] = 0.0
    X, _ = _wide(dev, T, N, 4, case["dy"])
    gate, cm = _nan(dev, (T + 255) // 256), _nan(dev, (T + 31) // 32)
    _call("mdl_split_tile_absmax", X, X.stride(0), T, N, gate, cm, _stream())
    assert sorted(torch.nonzero(cm.cpu() == 0).flatten().tolist()) == sorted(zero_chunks)
    A, Bm = Img(dev, case["x"]), Img(dev, case["dy"], pad_rows=32)
    for terms in (3, 2):
        got = _tn_call(dev, A, Bm, cm, terms)
        _tn_check("tn_chunks[T%d,%d zero,%s,terms%d]" % (T, len(zero_chunks), kind, terms), got, A, Bm, terms, kind)
        if len(zero_chunks) == (T + 31) // 32:
            assert float(got.abs().max()) == 0.0


@pytest.mark.parametrize("kind", ["uniform", "row_scaled", "integer"])
@pytest.mark.parametrize("T", [33, 97])
def test_tn_row_factors_cancel(dev, T, kind):
    """A row-scaled A image (s_r x_r) paired with a gradient image of row_inv[r] dy[r] (what mdl_ln_gelu_drop_bwd_split writes with
    row_mul = row_inv): the row factors cancel inside the contraction -- the product from the planes is dy^T x, and a zero row of x
    (row_inv = 0) contributes nothing and does not set the gradient image's scale."""
    Mi, N = 256, 32
    case = S.tn_case(T, Mi, N, 700 + T, kind)
    case["x"][T // 2] = 0.0
    A = Img(dev, case["x"], True)
    g = case["dy"] * A.inv_cpu[:, None]
    if kind == "integer":
        g = g * 2.0 ** 14                                                   # (back to integers: exact either way, the scale is a power of two)
    Bm = Img(dev, g, pad_rows=32)
    Bm.check(g, "tn_rows.gradient image.")
    assert float(Bm.scale[1]) == float(g.abs().max())
    for terms in (3, 2):
        got = _tn_call(dev, A, Bm, None, terms)
        # (the scaled rows of A are all of one magnitude; dy's own row scales remain: the proven ceiling for row_scaled)
        _tn_check("tn_rows[T%d,%s,terms%d]" % (T, kind, terms), got, A, Bm, terms, kind)
        if kind == "integer":
            S.check_exact("tn_rows: dy^T x", got, (g.double().t() @ (case["x"].double() / A.inv_cpu.double().clamp_min(1e-300)[:, None])))


# ================================================================================================================== pooling on the image
@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("lens,dense", [pytest.param(*c, id="dense" if c[1] else "ragged") for c in S.POOL_BAGS])
@pytest.mark.parametrize("H", S.POOL_HEADS)
def test_pool_img(dev, H, lens, dense, kind):
    """mdl_abmil_pool_fwd_img and mdl_abmil_pool_dscores_img (written and accumulated) on the image of E, against fp64 of the decoded
    image; the score gradients from the forward results the kernel stored."""
    from madeleine_amd import _native
    case = S.pool_img_case(lens, H, kind)
    T, C, n = sum(lens), H * B.HID, len(lens)
    Ei = Img(dev, case["E32"], what="pool.E")
    Ei.check(case["E32"], "pool_img[H%d,%s,%s].E." % (H, "dense" if dense else "ragged", kind))
    case["E"] = S.decode(Ei.hi, Ei.lo, Ei.s)
    cu = None if dense else torch.tensor(B.bag_rows(lens), dtype=torch.int64, device=dev)
    geom = (n, lens[0] if dense else 0, cu, max(lens), H)
    sd, dpd = case["s"].to(dev), case["dp"].to(dev)
    nbytes = _native.lib().mdl_abmil_pool_ws_bytes(n, max(lens), H)
    _poison(dev, 2 * nbytes + 4096)
    ws = torch.empty(nbytes // 4 + 16, device=dev)
    pooled, m, l_ = _nan(dev, n, C), _nan(dev, n, H), _nan(dev, n, H)
    _call("mdl_abmil_pool_fwd_img", Ei.raw, Ei.rsb, Ei.scale, sd, pooled, m, l_, *geom, ws, _stream())
    ds, ds_acc = _nan(dev, T, H), case["ds0"].to(dev).clone()
    _call("mdl_abmil_pool_dscores_img", Ei.raw, Ei.rsb, Ei.scale, sd, pooled, m, l_, dpd, ds, 0, *geom, _stream())
    _call("mdl_abmil_pool_dscores_img", Ei.raw, Ei.rsb, Ei.scale, sd, pooled, m, l_, dpd, ds_acc, 1, *geom, _stream())
    torch.cuda.synchronize()
    fwd = dict(pooled=pooled.cpu(), m=m.cpu(), l=l_.cpu())
    bounds, ratios = S.pool_img_bounds(case, fwd)
    what = "pool_img[H%d,%s,%s]." % (H, "dense" if dense else "ragged", kind)
    print("SPLITERR %storch fp32 ratios of this case %s (constants %s, x %g allowed)" % (what, {k: round(v, 2) for k, v in ratios.items()},
                                                                                      S.SOFTMAX_RATIO, S.SOFTMAX_FACTOR))
    S.check_exact(what + "stat_m", fwd["m"], bounds["stat_m"][0])
    S.check(what + "stat_l", fwd["l"], *bounds["stat_l"])
    S.check(what + "pooled", fwd["pooled"], *bounds["pooled"])
    for name, got in (("d_scores", ds.cpu()), ("d_scores_acc", ds_acc.cpu())):
        ref, bound, rows = bounds[name]
        S.check(what + name, got[rows], ref[rows], bound[rows])


# ================================================================================================================================= gate
def _gate_fwd(dev, case, seed):
    """mdl_abmil_gate_fwd_split on the image of E (checked): (image, device parameters, scores, act_a, act_b)."""
    from madeleine_amd import _native
    T, H, p = case["T"], case["H"], case["p"]
    Ei = Img(dev, case["E32"], what="gate.E")
    ps = {k: case[k].to(dev) for k in ("Wa", "ba", "Wb", "bb", "wc", "bc")}
    sc, a, b = _nan(dev, T, H), _nan(dev, T, H, B.HID), _nan(dev, T, H, B.HID)
    nbytes = _native.lib().mdl_abmil_gate_fwd_split_ws_bytes(T, H)
    assert nbytes >= 0
    _poison(dev, 2 * nbytes + 4096)
    ws = torch.empty(nbytes // 4 + 16, device=dev)
    _call("mdl_abmil_gate_fwd_split", Ei.raw, Ei.rsb, Ei.scale, ps["Wa"], ps["ba"], ps["Wb"], ps["bb"], ps["wc"], ps["bc"], sc, a, b, T, H, float(p),
          seed, None, None, ws, _stream())
    torch.cuda.synchronize()
    return Ei, ps, sc, a, b


def _gate_bwd(dev, case, Ei, ps, a, b, seed, acc, phases=(3,), terms=3, pool=()):
    """mdl_abmil_attnpool_bwd_split, one call per entry of `phases` on one workspace -> the gradients on the host, and dE_absmax."""
    from madeleine_amd import _native
    T, H, p = case["T"], case["H"], case["p"]
    dE, dbuf = _wide(dev, T, H * B.HID, 4, case["dE0"] if acc else None)
    grads = [_nan(dev, H, B.HID, B.HID), _nan(dev, H, B.HID, B.HID), _nan(dev, H, B.HID), _nan(dev, H, B.HID), _nan(dev, H, B.HID), _nan(dev, H)]
    amax = torch.zeros(1, device=dev)
    nbytes = _native.lib().mdl_abmil_gate_bwd_split_ws_bytes(T, H)
    assert nbytes >= 0
    _poison(dev, 2 * nbytes + 4096)
    ws = torch.empty(nbytes // 4 + 16, device=dev)
    pool = list(pool) if pool else [None] * 5 + [0]
    for ph in phases:
        _call("mdl_abmil_attnpool_bwd_split", Ei.raw, Ei.rsb, Ei.scale, ps["Wa"], ps["Wb"], ps["wc"], a, b, case["ds"].to(dev), dE, dE.stride(0), acc,
              *grads, T, H, float(p), seed, None, None, *pool, amax, ws, _stream(), ph, terms)
    torch.cuda.synchronize()
    assert _gap_is_nan(dbuf, H * B.HID), "the gap between the rows of dE was written"
    got = dict(zip(("dE", "dWa", "dWb", "dba", "dbb", "dwc", "dbc"), [dE.cpu()] + [g.cpu() for g in grads]))
    assert float(amax) == float(got["dE"].abs().max()), "dE_absmax is not max |dE| as stored"
    return got


def _gate_check_fwd(case, Ei, sc, a, b, ka, kb, what, ref_device):
    a, b = a.cpu(), b.cpu()
    E_dec = S.decode(Ei.hi, Ei.lo, Ei.s)
    fwd = S.gate_fwd_ref(case, E_dec, ref_device)
    S.check(what + "act_a", a, *fwd["act_a"])
    S.check(what + "act_b", b, *fwd["act_b"])
    S.check(what + "scores", sc.cpu(), *B.gate_scores_ref(case, a, b, ka, kb))
    return E_dec, Ei.hi.double() / Ei.s, a, b


# (accumulate, phases, terms): the one-call form, the sequence dz | dX | dW on one workspace, and the hi-plane products of terms = 2
GATE_BWD = ((0, (3,), 3), (1, (1, 4, 8), 3), (0, (3,), 2))


def _gate(dev, T, H, p, kind, ref_device, lens=None):
    from tests.test_bf16_elements_gpu import _gate_masks
    S_ = 2 if T == 4097 else 1
    _expect_plan("gate_split_fwd", T, H, 0, dict(persist=0))
    _expect_plan("gate_split_bwd", T, H, 0, dict(splits=S_, tps=-(-(-(-T // S_)) // 32) * 32, chunk=32))
    case = S.gate_case(T, H, 4000 + T + H, kind, p)
    seed = 777 + T
    ka, kb = _gate_masks(dev, T, H, p, seed)
    what = "gate[T%d,H%d,p%g,%s]." % (T, H, p, kind)
    Ei, ps, sc, a, b = _gate_fwd(dev, case, seed)
    E_dec, E_hi, a32, b32 = _gate_check_fwd(case, Ei, sc, a, b, ka, kb, what, ref_device)
    pool, term = (), None
    if lens is not None:      # the pooling term's inputs are arguments of the call: the kernel's own scores, their statistics formed here
        s = sc.cpu()
        row_bag, m, l_ = S.gate_pool_inputs(s, lens)
        dp = S.operand((len(lens), H * B.HID), 4600 + H, kind)
        term, _ = S.gate_pool_term(s, m, l_, dp, row_bag, H, what)
        pool = [x.to(dev) for x in (s, m, l_, dp, row_bag)] + [0]
    for acc, phases, terms in GATE_BWD:
        got = _gate_bwd(dev, case, Ei, ps, a, b, seed, acc, phases, terms, pool)
        tag = "%sacc%d.phases%s.terms%d." % (what, acc, "".join(map(str, phases)), terms)
        for k, v in S.gate_bwd_ref(case, E_dec, E_hi, a32, b32, ka, kb, acc, terms, term, ref_device).items():
            S.check(tag + k, got[k].reshape(v[0].shape), *v)


@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("H", [1, 2, 4])
@pytest.mark.parametrize("T", [1, 33, 257])
def test_gate(dev, T, H, p, kind):
    """mdl_abmil_gate_fwd_split and mdl_abmil_attnpool_bwd_split (no pooling term) at one token, a partial second 32-token chunk and a
    one-row second 256-tile: scores, act_a, act_b; dE written and accumulated with dE_absmax; dWa, dWb, dba, dbb, dwc, dbc; the dropout
    replayed in fp64 from the exported masks."""
    _gate(dev, T, H, p, kind, dev if T >= 257 else "cpu")


@pytest.mark.parametrize("H,p,kind", [(1, 0.25, "row_scaled"), (2, 0.0, "uniform"), (4, 0.25, "cancelling")])
def test_gate_two_token_splits(dev, H, p, kind):
    """T = 4097: two token splits of the dW contraction (2080 + 2017 tokens) with their slab reduction, 17 token tiles with a one-row last."""
    _gate(dev, 4097, H, p, kind, dev)


@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("H", [1, 4])
def test_gate_fused_pooling_term(dev, H, kind):
    """The pooling term w d_pooled in the dX epilogue, on two ragged bags of 70 and 59 tokens (the bag boundary inside the tile)."""
    _gate(dev, 129, H, 0.25, kind, "cpu", lens=(70, 59))


# =============================================================================================================== LayerNorm-GELU-Dropout
LN_WIDTHS = (256, 512, 1024, 2048, 4096)          # 512 and the other widths of tests/test_ln_kinds_gpu.py


def _ln_image(dev, rows, W):
    """A dense image buffer of `rows` rows of 4 W bytes (these entry points take no row stride) and a guard row, all 0xFF."""
    return torch.full((rows + 1, 4 * W), 0xFF, dtype=torch.uint8, device=dev)


def _ln_planes(raw, rows, W):
    host = raw.cpu()
    assert bool((host[rows:] == 0xFF).all()), "bytes behind the image written"
    return S.unpack(host[:rows], W)


def _ln_fwd(dev, case, d, want_y, row_mul, want_rstd_max):
    rows, W = case["x"].shape
    raw, scale = _ln_image(dev, rows, W), _nan(dev, 2)
    y = _nan(dev, rows, W) if want_y else None
    mean, rstd = _nan(dev, rows), _nan(dev, rows)
    rmax = _nan(dev, 1) if want_rstd_max else None
    _call("mdl_ln_gelu_drop_fwd_split", d["x"], d["bias"], d["gamma"], d["beta"], y, raw, scale, mean, rstd, rows, W, case["eps"], float(case["p"]), 5,
          d["keep"], row_mul, rmax, _stream())
    torch.cuda.synchronize()
    hi, lo = _ln_planes(raw, rows, W)
    return dict(hi=hi, lo=lo, scale=scale.cpu(), y=None if y is None else y.cpu(), mean=mean.cpu(), rstd=rstd.cpu(), rstd_dev=(mean, rstd),
                rstd_max=rmax)


def _ln_bwd(dev, case, d, st, dy_absmax, row_mul, rstd_max, groups=None):
    from madeleine_amd import _native
    rows, W = case["x"].shape
    raw, scale = _ln_image(dev, rows + 32, W), _nan(dev, 2)
    dg, db, dbias = _nan(dev, W), _nan(dev, W), _nan(dev, W)
    out = dict(dgamma=dg, dbeta=db, dbias=dbias)
    extra = ()
    if groups is not None:
        G = len(groups)
        out["dgroup_bias"] = _nan(dev, G, W)
        extra = (torch.tensor(B.bag_rows(groups), dtype=torch.int64, device=dev), G, out["dgroup_bias"])
        nbytes = _native.lib().mdl_ln_gelu_drop_bwd_groups_ws_bytes(rows, W, G)
    else:
        nbytes = _native.lib().mdl_ln_gelu_drop_bwd_ws_bytes(rows, W)
    assert nbytes >= 0
    _poison(dev, 2 * nbytes + 4096)
    ws = torch.empty(nbytes // 4 + 16, device=dev)
    mean, rstd = st["rstd_dev"]
    _call("mdl_ln_gelu_drop_bwd_split" + ("_groups" if groups is not None else ""), d["x"], d["bias"], d["gamma"], d["beta"], mean, rstd, d["dy"],
          dy_absmax, raw, scale, dg, db, dbias, rows, W, float(case["p"]), 5, d["keep"], row_mul, rstd_max, *extra, ws, _stream())
    torch.cuda.synchronize()
    hi, lo = _ln_planes(raw, rows + 32, W)
    assert float(hi[rows:].float().abs().sum() + lo[rows:].float().abs().sum()) == 0.0, "the dx image is not followed by 32 zero rows"
    out = {k: v.cpu() for k, v in out.items()}
    out.update(hi=hi[:rows], lo=lo[:rows], scale=scale.cpu())
    return out


def _ln(dev, rows, W, p, kind, groups=None):
    case = S.ln_case(rows, W, 6000 + rows + W, kind, p, groups)
    d = {k: case[k].to(dev).contiguous() for k in ("x", "dy", "gamma", "beta", "bias")}
    d["keep"] = case["keep"].to(dev) if case["keep"] is not None else None
    rm = case["row_mul"].to(dev)
    what = "ln[%dx%d,p%g,%s%s]." % (rows, W, p, kind, "" if groups is None else ",G%d" % len(groups))
    # ---- forward: y and the image; the image alone with row_mul and rstd_max; rstd_max without row_mul
    f1 = _ln_fwd(dev, case, d, True, None, False)
    f2 = _ln_fwd(dev, case, d, False, rm, True)
    f3 = _ln_fwd(dev, case, d, False, None, True)
    mean_ref, rstd_ref = S.ln_stats_ref(case)
    S.check(what + "mean", f1["mean"], *mean_ref)
    S.check(what + "rstd", f1["rstd"], *rstd_ref)
    ref, slack = S.ln_y_ref(case, f1["mean"], f1["rstd"])
    S.check(what + "y", f1["y"], ref, slack + S.U24 * ref.abs())
    S.check_ln_scale(what + "fwd.", f1["scale"], S.ln_fwd_bound(case, W), f1["y"])
    S.check_ln_image(what + "y.", f1["hi"], f1["lo"], float(f1["scale"][0]), ref, slack, y32=f1["y"])
    for f in (f2, f3):
        assert torch.equal(f["hi"], f1["hi"]) and torch.equal(f["lo"], f1["lo"]) and torch.equal(f["scale"], f1["scale"]), what + "y == NULL"
        assert torch.equal(f["rstd"], f1["rstd"]) and torch.equal(f["mean"], f1["mean"])
    assert float(f2["rstd_max"]) == float((f1["rstd"] * case["row_mul"]).max()), what + "rstd_max with row_mul"
    assert float(f3["rstd_max"]) == float(f1["rstd"].max()), what + "rstd_max"
    # ---- backward: everything taken by passes over the data; then dy_absmax, row_mul and the forward's rstd_max handed in
    dy_max = case["dy"].abs().max().reshape(1).to(dev)
    for tag, args, row_mul in (("plain.", (None, None, None), None), ("given.", (dy_max, rm, f2["rstd_max"]), case["row_mul"]),
                               ("row_mul.", (None, rm, None), case["row_mul"])):
        got = _ln_bwd(dev, case, d, f1, *args, groups=groups)
        bref = S.ln_bwd_ref(case, f1["mean"], f1["rstd"], row_mul)
        for k in ("dgamma", "dbeta", "dbias") + (("dgroup_bias",) if groups is not None else ()):
            S.check(what + tag + k, got[k], *bref[k])
        if groups is not None:
            for g, n in enumerate(groups):
                if n == 0:
                    assert float(got["dgroup_bias"][g].abs().max()) == 0.0, "the empty group"
        dx, e_dx = bref["dx"]
        S.check_ln_scale(what + tag + "bwd.", got["scale"], S.ln_bwd_bound(case, W, f1["rstd"], row_mul), S.decode(got["hi"], got["lo"], float(got["scale"][0])))
        S.check_ln_image(what + tag + "dx.", got["hi"], got["lo"], float(got["scale"][0]), dx, e_dx)


@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("rows", [1, 33, 257])
@pytest.mark.parametrize("W", LN_WIDTHS)
def test_ln_images(dev, W, rows, p, kind):
    """mdl_ln_gelu_drop_fwd_split and mdl_ln_gelu_drop_bwd_split: the scales (a power of two by the rule from the stored bound, the bound
    by the documented formula, every value below it), the decoded images of y and of row_mul dx against fp64 from the stored mean / rstd,
    the image within the element bound of the fp32 y, rstd_max exact, 32 zero rows behind dx, dgamma / dbeta / dbias; row_mul, rstd_max
    and dy_absmax given and NULL."""
    _ln(dev, rows, W, p, kind)


@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("rows", [1, 33, 257])
@pytest.mark.parametrize("W", [512, 1024])
def test_ln_images_groups(dev, W, rows, G, p, kind):
    """mdl_ln_gelu_drop_bwd_split_groups: one group, and three with a group of one row in the middle (at rows = 1 the outer two are
    empty): dgroup_bias per element beside everything test_ln_images checks."""
    _ln(dev, rows, W, p, kind, [rows] if G == 1 else [rows - 1 - (rows - 1) // 2, 1, (rows - 1) // 2])


# ======================================================================================================================= two-stage rings
def _stages_child():
    """Runs in the child of test_two_stage_rings: the NT and TN element and integer cases at one tail shape each, on the two-stage rings."""
    assert os.environ.get("MADELEINE_SP_NT_STAGES") == "2" and os.environ.get("MADELEINE_SP_TN_STAGES") == "2"
    dev = torch.device("cuda:0")
    for kind in S.KINDS4:
        _nt(dev, 257, 132, 96, kind)              # (N > 128: the 256 x 256 tile -- the 512 x 128 tile has a loop of its own)
        _nt(dev, 513, 260, 512, kind, variants=((1, 1, ("bias", "acc", "absmax")),))
        _tn(dev, 97, 288, 288, kind)
        _tn(dev, 4097, 288, 32, kind)
    print("SPLITERR two-stage rings: done")


def test_two_stage_rings(dev):
    """sp_nt_kernel<*, 2> and sp_tn_kernel<*, 2> are compiled and selectable (MADELEINE_SP_NT_STAGES / _TN_STAGES = 2, read once per
    process): a fresh child process with both set reruns NT and TN cases of this file, row-, column- and token-tailed."""
    env = dict(os.environ, MADELEINE_SP_NT_STAGES="2", MADELEINE_SP_TN_STAGES="2")
    code = "from tests import test_split_elements_gpu as G; G._stages_child()"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout[-6000:])
    assert r.returncode == 0, "the two-stage child failed with status %d" % r.returncode
    assert "SPLITERR two-stage rings: done" in r.stdout
