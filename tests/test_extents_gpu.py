"""Every launching entry point of include/madeleine_amd.h inside a guarded arena (tests/_arena.py): every device buffer of a call
sequence is exactly the byte extent the header states -- outputs at their stated shapes, workspaces at exactly the bytes their
*_ws_bytes query returns, the documented zero padding at exactly its documented count -- between guard bands of a known byte, once
per fill (0xFF: every float a NaN, every integer -1; 0x3F: finite non-zero floats).  Each case asserts
  (a) every guard byte, every operand the header declares const and every documented zero padding is untouched;
  (b) every output is bit-identical between the two fills (nothing depends on bytes outside the stated extents) and free of NaN;
  (c) the valid region agrees with a plain fp64 CPU reference within the bound the suite already states for that kernel; each case
      cites the test it takes the bound from.
A case is a function of tests/_extent_cases.Run; FAMILIES registers all of them so that tests/test_extents_cpu.py can run their
planning passes (no GPU) and hold the set of entry points they issue against the header's export list.

Findings (entry point, shape, offset, cause, fix) are recorded in the docstring of the case that found them; see FINDINGS below."""
import functools

import numpy as np
import pytest
import torch

from tests._extent_cases import BF, F32, run_case
from tests._util import max_rel, rel_err

pytestmark = pytest.mark.gpu
EPS_BF16 = 2.0 ** -8
TOL = 1e-3
U8, I32, I64, F64 = torch.uint8, torch.int32, torch.int64, torch.float64

FINDINGS = """No kernel, launcher or workspace query was found outside its stated extents.  One gap in the header itself: mdl_infonce_fwd / _bwd and
mdl_infonce_ws_bytes refuse D % 32 != 0 (and D < 8) with MDL_E_ARG, which the header did not state; it does now (no ABI change).
One bound that fits no case: d_scores of one-token dense bags (see _pool_factory)."""

FAMILIES = {}      # family -> {case id: factory() -> (case(r), check(got) or None, plans [(product, T, a, b, want)], run_case keywords)}


def _register(family, cid):
    def deco(factory):
        FAMILIES.setdefault(family, {})[cid] = factory
        return factory
    return deco


def _ids(family):
    return sorted(FAMILIES[family])


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _go(dev, family, cid):
    from tests.test_dispatch_edges_gpu import _expect_plan
    case, check, plans, kw = FAMILIES[family][cid]()
    for product, T, a, b, want in plans:
        _expect_plan(product, T, a, b, want)
    try:
        return run_case(dev, case, check, **kw)
    except RuntimeError as e:      # a device fault poisons the process: nothing more is started on the GPU after it
        if "HIP error" in str(e) or "illegal memory access" in str(e) or "hipError" in str(e):
            pytest.exit("device fault in %s:%s: %s" % (family, cid, e), returncode=3)
        raise


def _S():
    import tests.test_strides_gpu as S
    return S


def _D():
    import tests.test_dispatch_edges_gpu as D
    return D


# ============================================================================================================================ Linears
LINEAR_SHAPES = [(19, 12, 20), (300, 256, 96), (300, 128, 256), (257, 256, 512), (4097, 256, 512)]
LINEAR_PLAN_FP32 = {(19, 12, 20): dict(variant=0, splits=1), (300, 256, 96): dict(variant=1, splits=1), (300, 128, 256): dict(variant=2, splits=1),
                    (257, 256, 512): dict(variant=1, splits=1), (4097, 256, 512): dict(variant=1, splits=2)}
LINEAR_PLAN_BF16 = {(300, 256, 96): (dict(variant=4), dict(variant=128, extra=4, splits=1)), (300, 128, 256): (dict(variant=2), dict(variant=128, extra=4)),
                    (257, 256, 512): (dict(variant=4), dict(variant=128, splits=1)), (4097, 256, 512): (dict(variant=4), dict(variant=128, splits=2))}


def _linear_factory(T, N, K, bf16):
    """mdl_linear_fwd / _bwd (fp32: bounds of tests/test_strides_gpu.py::test_linear_fp32 = the exact-fp32 contract of
    tests/test_dispatch_edges_gpu.py; bf16: tests/test_strides_gpu.py::test_linear_bf16 = the output-rounding bounds of
    tests/test_bf16_gpu.py), with dX and dbias present and absent."""
    dtype, sfx = (BF, "_bf16") if bf16 else (F32, "")

    def case(r):
        d = r.data(lambda: _S()._lin_case(T, N, K, bf16))
        x, W, b, dy = d[:4] if d else (None,) * 4
        st = r.stream()
        X, Wd, bd, dY = r.inp("X", (T, K), dtype, x), r.inp("W", (N, K), F32, W), r.inp("bias", (N,), F32, b), r.inp("dY", (T, N), dtype, dy)
        Y = r.out("Y", (T, N), dtype)
        r.call("mdl_linear_fwd" + sfx, X, K, Wd, bd, Y, N, T, N, K, r.ws("ws_fwd", "mdl_linear_fwd%s_ws_bytes" % sfx, T, N, K), st)
        dX, dW, db, dW2 = r.out("dX", (T, K), dtype), r.out("dW", (N, K)), r.out("dbias", (N,)), r.out("dW_only", (N, K))
        r.call("mdl_linear_bwd" + sfx, X, K, Wd, dY, N, dX, K, dW, db, T, N, K, r.ws("ws_bwd", "mdl_linear_bwd%s_ws_bytes" % sfx, T, N, K), st)
        r.call("mdl_linear_bwd" + sfx, X, K, Wd, dY, N, None, K, dW2, None, T, N, K, r.ws("ws_bwd2", "mdl_linear_bwd%s_ws_bytes" % sfx, T, N, K), st)
        return dict(Y=Y, dX=dX, dW=dW, db=db, dW_only=dW2)

    def check(got):
        D = _D()
        x, W, b, dy, y64, dx64, dw64, db64 = _S()._lin_case(T, N, K, bf16)
        if bf16:
            assert float((got["Y"].double() - y64).abs().max()) <= EPS_BF16 * float(y64.abs().max())
            assert rel_err(got["Y"], y64) < EPS_BF16 and rel_err(got["dX"], dx64) < EPS_BF16
            assert rel_err(got["dW"], dw64) < 1e-5 and rel_err(got["dW_only"], dw64) < 1e-5 and rel_err(got["db"], db64) < 1e-5
        else:
            D._chain_check(got["Y"], y64, D._mm(x.abs(), W.abs().t()) + b.double().abs(), 1e-6, "Y")
            D._chain_check(got["dX"], dx64, D._mm(dy.abs(), W.abs()), 1e-6, "dX")
            for k in ("dW", "dW_only"):
                D._chain_check(got[k], dw64, D._tn(dy.abs(), x.abs()), 1e-6, k)
            D._chain_check(got["db"], db64, dy.double().abs().sum(0), 1e-6, "dbias")
    if bf16:
        pf, pb = LINEAR_PLAN_BF16[(T, N, K)]
        plans = [("linear_bf16_fwd", T, N, K, pf), ("linear_bf16_bwd", T, N, K, pb)]
    else:
        plans = [("linear_fp32_bwd", T, N, K, LINEAR_PLAN_FP32[(T, N, K)])]
    return case, check, plans, {}


for _T, _N, _K in LINEAR_SHAPES:
    _register("linear", "fp32-T%d-N%d-K%d" % (_T, _N, _K))(functools.partial(_linear_factory, _T, _N, _K, False))
    if (_T, _N, _K) in LINEAR_PLAN_BF16:      # (19, 12, 20) is MDL_E_UNSUPPORTED in the bf16 mode: N % 128 == 0 and K % 32 == 0 only
        _register("linear", "bf16-T%d-N%d-K%d" % (_T, _N, _K))(functools.partial(_linear_factory, _T, _N, _K, True))


@pytest.mark.parametrize("cid", _ids("linear"))
def test_linear(dev, cid):
    _go(dev, "linear", cid)


# ======================================================================================================================= split engine
def _image_factory(K, pad):
    """mdl_split_image, mdl_split_image_rows and mdl_split_tile_absmax at rows = 300 (bounds: tests/test_strides_gpu.py::test_split_image):
    the image buffers are exactly (rows + pad_rows) x 4 K bytes and hold the fill where the pad rows will be."""
    rows = 300

    def x_of():
        x = _D()._u((rows, K), 9500 + K)
        x[7] = 0.0
        x[40:80] *= 2.0 ** -12
        return x

    def case(r):
        x, st = r.data(x_of), r.stream()
        X = r.inp("X", (rows, K), F32, x)
        img, sc1 = r.out("img", (rows + pad, K)), r.out("scale", (2,))
        r.call("mdl_split_image", X, K, rows, K, img, 4 * K, pad, sc1, st)
        img2, rinv, sc2 = r.out("img_rows", (rows + pad, K)), r.out("row_inv", (rows,)), r.out("scale_rows", (2,))
        r.call("mdl_split_image_rows", X, K, rows, K, img2, 4 * K, pad, rinv, sc2, st)
        img3, rinv3 = r.out("img_rows_noscale", (rows + pad, K)), r.out("row_inv_noscale", (rows,))
        r.call("mdl_split_image_rows", X, K, rows, K, img3, 4 * K, pad, rinv3, None, st)
        gate, cm, gate2 = r.out("gate", ((rows + 255) // 256,)), r.out("chunk_max", ((rows + 31) // 32,)), r.out("gate_alone", ((rows + 255) // 256,))
        r.call("mdl_split_tile_absmax", X, K, rows, K, gate, cm, st)
        r.call("mdl_split_tile_absmax", X, K, rows, K, gate2, None, st)
        return dict(img=img, scale=sc1, img_rows=img2, row_inv=rinv, scale_rows=sc2, gate=gate, chunk_max=cm, gate_alone=gate2,
                    img_rows_noscale=img3, row_inv_noscale=rinv3)

    def check(got):
        S, x = _S(), x_of()
        ax = x.abs().double()
        assert float(got["scale"][1]) == float(ax.max()) and float(got["scale_rows"][1]) == float(ax.max())
        S._check_image(got["img"][:rows], got["scale"][0], x, K)
        assert not got["img"][rows:].any() and not got["img_rows"][rows:].any() and not got["img_rows_noscale"][rows:].any()
        assert torch.equal(got["img_rows"].view(I32), got["img_rows_noscale"].view(I32)) and torch.equal(got["row_inv"], got["row_inv_noscale"])
        rinv = got["row_inv"].double()
        keep = torch.arange(rows) != 7
        assert float(rinv[7]) == 0.0 and bool((rinv[keep] > 0).all())
        s_r = torch.where(rinv > 0, 1.0 / rinv, torch.zeros_like(rinv))
        top = (ax * s_r[:, None]).max(1).values
        assert bool(((top >= 2.0 ** 13) & (top < 2.0 ** 14))[keep].all())
        S._check_image(got["img_rows"][:rows], s_r[:, None], x, K)
        want_gate = torch.stack([ax[i:i + 256].max() for i in range(0, rows, 256)])
        assert torch.equal(got["gate"].double(), want_gate) and torch.equal(got["gate_alone"].double(), want_gate)
        assert torch.equal(got["chunk_max"].double(), torch.stack([ax[i:i + 32].max() for i in range(0, rows, 32)]))
    return case, check, [], {}


for _K in (64, 1024, 2048):
    for _pad in (0, 32):
        _register("split", "image-K%d-pad%d" % (_K, _pad))(functools.partial(_image_factory, _K, _pad))


def _pow2(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return 2.0 ** torch.randint(-3, 4, shape, generator=g).float()


def _image_in(r, name, rows, K, x, pad_rows=0):
    """The split image of x [rows, K] built in the arena by mdl_split_image into exactly (rows + pad_rows) x 4 K bytes and frozen:
    an operand from here on.  pad_rows > 0: the header's trailing zero rows, provided and zeroed by the test (zero_tail), not by
    the kernel -- mdl_split_image is called with pad_rows = 0."""
    X = r.inp(name + ".x", (rows, K), F32, x)
    img = r.out(name, (rows + pad_rows, K), zero_tail=pad_rows * K * 4)
    sc = r.out(name + ".scale", (2,))
    r.call("mdl_split_image", X, K, rows, K, img, 4 * K, 0, sc, r.stream())
    r.freeze(name, name + ".scale")
    return img, sc


def _nt_factory(M, N, K):
    """mdl_split_gemm_nt on both kernels (N <= 128 with M > 256: the 512 x 128 narrow-output tile) with bias + absmax_out, with
    accumulate + row_gate, with a_row_mul + b_col_mul (powers of two, as the row scales are: exact), and mdl_split_gemm_nt_group_bias.
    Bounds: the fp32-fmaf-chain contract of tests/test_split_gpu.py as tests/test_strides_gpu.py::test_split_gemm_nt applies it."""
    def data():
        D = _D()
        a, bw = D._u((M, K), 9600 + M + N), D._u((N, K), 9700 + N, K ** -0.5)
        a[256:] = 0.0
        return dict(a=a, bw=bw, bias=D._u((N,), 9800, 0.1), c0=D._u((M, N), 9900), gb=D._u((3, N), 9950, 0.1),
                    rg=(torch.arange(M) % 3).to(I32), rm=_pow2((M,), 1), cm=_pow2((N,), 2))

    def case(r):
        d = r.data(data) or {}
        st = r.stream()
        A, asc = _image_in(r, "A", M, K, d.get("a"))
        B, bsc = _image_in(r, "B", N, K, d.get("bw"))
        geo = (A, 4 * K, asc, B, 4 * K, bsc)
        bias = r.inp("bias", (N,), F32, d.get("bias"))
        C1, amax = r.out("C_bias", (M, N)), r.inout("absmax", (1,), F32, torch.zeros(1))
        r.call("mdl_split_gemm_nt", *geo, C1, N, M, N, K, bias, 0, amax, None, None, None, 3, st)
        a32 = r.inp("a_fp32", (M, K), F32, d.get("a"))
        gate = r.out("row_gate", ((M + 255) // 256,))
        r.call("mdl_split_tile_absmax", a32, K, M, K, gate, None, st)
        r.freeze("row_gate")
        C2 = r.inout("C_acc_gate", (M, N), F32, d.get("c0"))
        r.call("mdl_split_gemm_nt", *geo, C2, N, M, N, K, None, 1, None, gate, None, None, 3, st)
        C3 = r.out("C_group", (M, N))
        r.call("mdl_split_gemm_nt_group_bias", *geo, C3, N, M, N, K, bias, None, None, r.inp("group_bias", (3, N), F32, d.get("gb")),
               r.inp("row_group", (M,), I32, d.get("rg")), 3, st)
        C4 = r.out("C_mul", (M, N))
        r.call("mdl_split_gemm_nt", *geo, C4, N, M, N, K, bias, 0, None, None, r.inp("a_row_mul", (M,), F32, d.get("rm")),
               r.inp("b_col_mul", (N,), F32, d.get("cm")), 3, st)
        return dict(bias=C1, absmax=amax, acc_gate=C2, group=C3, mul=C4)

    def check(got):
        D, d = _D(), data()
        p64, mag = D._mm(d["a"], d["bw"].t()), D._mm(d["a"].abs(), d["bw"].abs().t())
        bias, c0, gb, rg = d["bias"].double(), d["c0"].double(), d["gb"].double(), d["rg"].long()
        want = p64 + bias
        D._chain_check(got["bias"], want, mag + bias.abs(), 4e-7, "bias")
        assert abs(float(got["absmax"]) - float(want.abs().max())) <= 1e-6 * float(want.abs().max())
        D._chain_check(got["acc_gate"], p64 + c0, mag + c0.abs(), 4e-7, "accumulate + row_gate")
        assert torch.equal(got["acc_gate"][256:], d["c0"][256:])
        D._chain_check(got["group"], want + gb[rg], mag + bias.abs() + gb.abs()[rg], 4e-7, "group_bias")
        f = d["rm"].double()[:, None] * d["cm"].double()[None, :]
        D._chain_check(got["mul"], p64 * f + bias, mag * f + bias.abs(), 4e-7, "a_row_mul, b_col_mul")
    return case, check, [], {}


_register("split", "nt-M300-N256-K96-tile256")(functools.partial(_nt_factory, 300, 256, 96))
_register("split", "nt-M300-N128-K64-narrow_tile512x128")(functools.partial(_nt_factory, 300, 128, 64))


def _tn_factory(T, want):
    """mdl_split_gemm_tn (dW = dY^T X) with B followed by exactly the 32 zero rows the header asks for and nothing else, and with
    b_chunk_max.  Bound: tests/test_strides_gpu.py::test_split_gemm_tn (4e-7 sum |a b|, 1e-6 relative)."""
    Mi, N = 256, 128

    def data():
        D = _D()
        return D._u((T, Mi), 9960 + T), D._u((T, N), 9970 + T, 0.5)

    def case(r):
        x, dy = r.data(data) or (None, None)
        st = r.stream()
        A, asc = _image_in(r, "A", T, Mi, x)
        B, bsc = _image_in(r, "B", T, N, dy, pad_rows=32)
        out = r.out("dW", (N, Mi))
        r.call("mdl_split_gemm_tn", A, 4 * Mi, asc, Mi, B, 4 * N, bsc, N, out, T, None, r.ws("ws", "mdl_split_gemm_tn_ws_bytes", T, Mi, N), 3, st)
        dy32, cm = r.inp("dy_fp32", (T, N), F32, dy), r.out("chunk_max", ((T + 31) // 32,))
        r.call("mdl_split_tile_absmax", dy32, N, T, N, r.out("gate", ((T + 255) // 256,)), cm, st)
        r.freeze("chunk_max")
        out2 = r.out("dW_chunk_max", (N, Mi))
        r.call("mdl_split_gemm_tn", A, 4 * Mi, asc, Mi, B, 4 * N, bsc, N, out2, T, cm, r.ws("ws2", "mdl_split_gemm_tn_ws_bytes", T, Mi, N), 3, st)
        return dict(dW=out, dW_chunk_max=out2)

    def check(got):
        D = _D()
        x, dy = data()
        for k in ("dW", "dW_chunk_max"):
            D._chain_check(got[k], D._tn(dy, x), D._tn(dy.abs(), x.abs()), 4e-7, k)
    return case, check, [("split_tn", T, Mi, N, want)], {}


_register("split", "tn-T33")(functools.partial(_tn_factory, 33, dict(splits=1, tps=64)))
_register("split", "tn-T4097-S2")(functools.partial(_tn_factory, 4097, dict(splits=2)))


@pytest.mark.parametrize("cid", _ids("split"))
def test_split_engine(dev, cid):
    _go(dev, "split", cid)


# ============================================================================================================================== gates
GATE_QUERIES = {"fp32": ("mdl_abmil_gate_fwd_ws_bytes", "mdl_abmil_gate_bwd_ws_bytes"),
                "bf16": ("mdl_abmil_gate_fwd_bf16_ws_bytes", "mdl_abmil_gate_bwd_bf16_ws_bytes"),
                "split": ("mdl_abmil_gate_fwd_split_ws_bytes", "mdl_abmil_gate_bwd_split_ws_bytes")}
SPLIT_VARIANTS = [("plain", 0, None, (3,)), ("plain_acc_1_2", 1, None, (1, 2)), ("ragged_acc", 1, True, (3,)), ("ragged_1_2", 0, True, (1, 2)),
                  ("plain_1_4_8", 0, None, (1, 4, 8))]
GRAD_NAMES = ("dWa", "dWb", "dba", "dbb", "dwc", "dbc")      # the order of the backward's arguments


@functools.lru_cache(maxsize=None)
def _gate_base(T, H, p, bf16):
    """tests/test_strides_gpu.py::_gate_case; below four tokens (its bag splits need four) the same tuple with one bag of T tokens as
    the ragged pooling term and no dense one."""
    S, D = _S(), _D()
    if T >= 4:
        return S._gate_case(T, H, p, bf16)
    assert p == 0
    E, w, ds = D._gate_inputs(T, H, 7000 + T + H, bf16=bf16)
    ds = (ds.double() + ((T / 3.0) ** 0.5 - ds.double().sum(0)) / T).float()
    ref = D._gate64(E, w, ds, 0.0, None, None)
    dE0 = D._u((T, H * 512), 7100 + T)
    if bf16:
        dE0 = dE0.to(BF).float()
    row_bag, dp, sc = torch.zeros(T, dtype=I32), D._u((1, H * 512), 7201 + T), ref[0].float()
    m = sc.max(0, keepdim=True).values
    l_ = (sc - m).double().exp().sum(0, keepdim=True).float()
    wgt = (sc.double() - m.double()).exp() / l_.double()
    term = (wgt[:, :, None] * dp.double().view(1, H, 512)).reshape(T, H * 512)
    return E, w, ds, None, None, ref, dE0, {True: dict(lens=[T], row_bag=row_bag, dp=dp, scores=sc, m=m, l=l_, term=term)}


def _gate_factory(engine, T, H, p, drop, forward=True):
    """Forward and every backward form of one gate engine at (T, H): mdl_abmil_gate_fwd, _gate_bwd, _attnpool_bwd, _attnpool_bwd_phases
    (fp32, bf16) or mdl_abmil_gate_fwd_split and mdl_abmil_attnpool_bwd_split in phases 3, 1 + 2 and 1 + 4 + 8.  drop: None (p = 0),
    'keep' (explicit keep_a / keep_b) or 'hash' (the counter hash; the masks mdl_abmil_gate_dropout_mask exports, into arena buffers
    of their own, are replayed in fp64).  The dz region [T + 16, H, 1024] and every slab live in a workspace of exactly the query's
    bytes.  Bounds: tests/test_hip_kernels.py::test_gate_eval through tests/test_dispatch_edges_gpu.py::_check_gate_fp32 (fp32, split);
    tests/test_strides_gpu.py::test_gate_bf16 = the gate bounds of tests/test_bf16_gpu.py (bf16)."""
    dtype = BF if engine == "bf16" else F32
    sfx = {"fp32": "", "bf16": "_bf16", "split": "_split"}[engine]
    C = H * 512
    qf, qb = GATE_QUERIES[engine]
    explicit = p if drop == "keep" else 0.0

    def base():
        return _gate_base(T, H, explicit, engine == "bf16")

    def case(r):
        d = r.data(base)
        E, w, ds, ka, kb, _, dE0, pool = d if d else (None, (None,) * 6, None, None, None, None, None, None)
        st = r.stream()
        Wa, ba, Wb, bb, wc, bc = [r.inp(n, s, F32, x) for n, s, x in zip(("Wa", "ba", "Wb", "bb", "wc", "bc"),
                                                                            ((H, 512, 512), (H, 512), (H, 512, 512), (H, 512), (H, 512), (H,)), w)]
        if engine == "split":
            img, esc = _image_in(r, "E_img", T, C, E)
            e_args = (img, 4 * C, esc)
        else:
            e_args = (r.inp("E", (T, C), dtype, E), C)
        out, kad, kbd = {}, None, None
        if drop == "keep":
            kad, kbd = r.inp("keep_a", (T, H, 512), U8, ka), r.inp("keep_b", (T, H, 512), U8, kb)
        elif drop == "hash":
            for which, n in ((0, "mask_a"), (1, "mask_b")):
                out[n] = r.out(n, (T, H, 512), U8)
                r.call("mdl_abmil_gate_dropout_mask", out[n], T, H, which, float(p), 11, st)
        sc, a, b = r.out("scores", (T, H)), r.out("act_a", (T, H, 512), dtype), r.out("act_b", (T, H, 512), dtype)
        r.call("mdl_abmil_gate_fwd" + sfx, *e_args, Wa, ba, Wb, bb, wc, bc, sc, a, b, T, H, float(p), 11, kad, kbd, r.ws("ws_fwd", qf, T, H), st)
        r.freeze("act_a", "act_b")
        out.update(scores=sc, act_a=a, act_b=b)
        dsd = r.inp("d_scores", (T, H), F32, ds)
        terms = {}
        for ragged in (False, True):
            q = pool[ragged] if pool is not None and ragged in pool else None
            if ragged or (T % 4 == 0 and T >= 4):
                nb = (3 if T >= 4 else 1) if ragged else 4
                terms[ragged] = [r.inp("pt%d.%s" % (ragged, n), s, t, q and q[n]) for n, s, t in
                                 (("scores", (T, H), F32), ("m", (nb, H), F32), ("l", (nb, H), F32), ("dp", (nb, C), F32), ("row_bag", (T,), I32))]
        variants = SPLIT_VARIANTS if engine == "split" else [(n, acc, pt, e) for n, acc, pt, e in _S()._gate_variants(T)]
        for name, acc, pterm, how in variants:
            dE = r.inout(name + ".dE", (T, C), dtype, dE0) if acc else r.out(name + ".dE", (T, C), dtype)
            grads = [r.out(name + "." + n, s) for n, s in zip(GRAD_NAMES, ((H, 512, 512), (H, 512, 512), (H, 512), (H, 512), (H, 512), (H,)))]
            ws = r.ws(name + ".ws", qb, T, H)
            if pterm is None:
                pt = [None] * 5 + [0]
            else:
                pt = terms[pterm][:4] + [terms[pterm][4] if pterm else None, 0 if pterm else T // 4]
            if engine == "split":
                for ph in how:
                    r.call("mdl_abmil_attnpool_bwd_split", *e_args, Wa, Wb, wc, a, b, dsd, dE, C, acc, *grads, T, H, float(p), 11, kad, kbd, *pt,
                           None, ws, st, ph, 3)
            else:
                args = [*e_args, Wa, Wb, wc, a, b, dsd, dE, acc, *grads, T, H, float(p), 11, kad, kbd] + (pt if pterm is not None else []) + [ws, st]
                if how == "attnpool_bwd_phases":
                    r.call("mdl_abmil_" + how + sfx, *args, 1)
                    r.call("mdl_abmil_" + how + sfx, *args, 2)
                else:
                    r.call("mdl_abmil_" + how + sfx, *args)
            out[name + ".dE"] = dE
            out.update({name + "." + n: g for n, g in zip(GRAD_NAMES, grads)})
        return out

    def check(got):
        S, D = _S(), _D()
        case_ = base()
        E, w, ds, ka, kb, ref, dE0, pool = case_
        if drop == "hash":
            ref = D._gate64(E, w, ds, p, got["mask_a"], got["mask_b"])
            keep = float(got["mask_a"].float().mean())
            assert abs(keep - (1 - p)) < 0.1 if T * H > 8 else 0 < keep < 1, keep
        variants = SPLIT_VARIANTS if engine == "split" else S._gate_variants(T)
        if forward:
            if engine == "bf16":
                assert float((got["scores"].double() - ref[0]).abs().max()) < 2 * EPS_BF16 * float(ref[0].abs().max()), "scores"
            else:
                assert rel_err(got["scores"], ref[0]) < 1e-5 and max_rel(got["scores"], ref[0]) < TOL, "scores"
        for name, acc, pterm, _ in variants:
            want = ref[1].clone()
            if pterm is not None:
                want = want + pool[pterm]["term"]
            if acc:
                want = want + dE0.double()
            g = {n: got[name + "." + n] for n in GRAD_NAMES}
            if engine == "bf16":
                assert rel_err(got[name + ".dE"].float(), want) < 5e-3, name + ".dE"
                for n, rr in zip(S.GRAD_ORDER, ref[2:]):
                    assert rel_err(g[n].reshape(rr.shape), rr) < (1e-5 if n == "dbc" else 5e-3), name + "." + n
            else:
                res = [got["scores"], got[name + ".dE"]] + [g[n].reshape(rr.shape) for n, rr in zip(S.GRAD_ORDER, ref[2:])]
                D._check_gate_fp32(res, [ref[0], want] + list(ref[2:]))
    return case, check, [], {}


GATE_SHAPES = [(1, 1, 0.25, "hash"), (300, 4, 0.25, "keep"), (4097, 1, 0.0, None)]
GATE_PLANS = {
    ("fp32", 1): [("gate_fp32_bwd", dict(splits=1, tps=16))], ("fp32", 300): [("gate_fp32_bwd", dict(splits=1))], ("fp32", 4097): [("gate_fp32_bwd", dict(splits=2))],
    ("split", 1): [("gate_split_bwd", dict(splits=1, tps=32))], ("split", 300): [("gate_split_bwd", dict(splits=1))], ("split", 4097): [("gate_split_bwd", dict(splits=2))],
    ("bf16", 1): [("gate_bf16_fwd", dict(variant=128)), ("gate_bf16_bwd", dict(variant=128, extra=128))],
    ("bf16", 300): [("gate_bf16_fwd", dict(variant=128)), ("gate_bf16_bwd", dict(variant=128, extra=128))],
    ("bf16", 4097): [("gate_bf16_fwd", dict(variant=256)), ("gate_bf16_bwd", dict(variant=128, extra=256, splits=2))],
    ("bf16", 16385): [("gate_bf16_fwd", dict(variant=256)), ("gate_bf16_bwd", dict(variant=256, extra=256))],
}


def _gate_entry(engine, T, H, p, drop, forward=True):
    case, check, _, kw = _gate_factory(engine, T, H, p, drop, forward)
    return case, check, [(prod, T, H, 0, want) for prod, want in GATE_PLANS[(engine, T)]], kw


for _eng in ("fp32", "split", "bf16"):
    for _T, _H, _p, _drop in GATE_SHAPES:
        _register("gate", "%s-T%d-H%d-%s" % (_eng, _T, _H, _drop or "p0"))(functools.partial(_gate_entry, _eng, _T, _H, _p, _drop))
_register("gate", "bf16-T16385-H1-dw256-bwd_only")(functools.partial(_gate_entry, "bf16", 16385, 1, 0.0, None, False))


@pytest.mark.parametrize("cid", _ids("gate"))
def test_gate(dev, cid):
    _go(dev, "gate", cid)


# ============================================================================================================================== pools
POOL_LENS = {"ragged": (0, 1, 129, 300), "dense300": (300, 300, 300), "dense129": (129, 129), "dense1": (1, 1, 1)}


def _pool_factory(H, bf16, lens_id):
    """mdl_abmil_pool_fwd / _bwd and mdl_abmil_wpool_fwd / _bwd (fp32 and bf16 E): dE and d_scores written, then accumulated onto
    finite contents.  Bounds: tests/test_hip_kernels.py::test_pool_fwd_bwd_dense through tests/test_strides_gpu.py::_check_pool."""
    lens = POOL_LENS[lens_id]
    T, n, C = sum(lens), len(lens), H * 512
    dtype, sfx = (BF, "_bf16") if bf16 else (F32, "")
    dense = lens_id != "ragged"

    def base():
        return _S()._pool_case(H, bf16, lens)

    def case(r):
        E, s, dp, dE0, ds0, cu, _ = r.data(base) or (None,) * 7
        st = r.stream()
        Ev, sd, dpd = r.inp("E", (T, C), dtype, E), r.inp("scores", (T, H), F32, s), r.inp("d_pooled", (n, C), F32, dp)
        cud = None if dense else r.inp("cu_seqlens", (n + 1,), I64, cu)
        geom = (n, lens[0] if dense else 0, cud, max(lens), H)
        out = {}
        for lin, pre in ((False, "pool"), (True, "wpool")):
            pooled, m, l_ = r.out(pre + ".pooled", (n, C)), r.out(pre + ".m", (n, H)), r.out(pre + ".l", (n, H))
            r.call("mdl_abmil_%s_fwd%s" % (pre, sfx), Ev, C, sd, pooled, m, l_, *geom, r.ws(pre + ".ws", "mdl_abmil_pool_ws_bytes", n, max(lens), H), st)
            r.freeze(pre + ".pooled", pre + ".m", pre + ".l")
            out[pre + ".pooled"] = pooled
            for acc in (0, 1):
                k = "%s.acc%d" % (pre, acc)
                dE = r.inout(k + ".dE", (T, C), dtype, dE0) if acc else r.out(k + ".dE", (T, C), dtype)
                dsc = r.inout(k + ".ds", (T, H), F32, ds0) if (acc and not lin) else r.out(k + ".ds", (T, H))
                if lin:
                    r.call("mdl_abmil_wpool_bwd" + sfx, Ev, C, sd, dpd, dE, acc, dsc, *geom, st)
                else:
                    r.call("mdl_abmil_pool_bwd" + sfx, Ev, C, sd, pooled, m, l_, dpd, dE, acc, dsc, acc, *geom, st)
                out[k + ".dE"], out[k + ".ds"] = dE, dsc
        return out

    def check(got):
        S = _S()
        E, s, dp, dE0, ds0, cu, res = base()
        for lin, pre in ((False, "pool"), (True, "wpool")):
            for acc in (0, 1):
                k = "%s.acc%d" % (pre, acc)
                g = {"pooled": got[pre + ".pooled"], "dE": got[k + ".dE"].float(), "ds": got[k + ".ds"]}
                if lin and acc:          # the weighted pooling accumulates into dE only: d_weights is always written
                    assert rel_err(g["dE"], res[lin][1] + dE0.double()) < (EPS_BF16 if bf16 else 1e-5), k
                    dsc = res[lin][2]
                    assert float((g["ds"].double() - dsc).abs().max()) <= 1e-4 * float(dsc.abs().max()) + 1e-6, k
                elif max(lens) == 1 and not lin:
                    # One-token bags: the softmax is 1 and the true d_scores is identically 0, so the suite's bound on it
                    # (1e-4 max |d_scores| + 1e-6, tests/test_hip_kernels.py::test_pool_fwd_bwd_dense) has no scale to work with: the
                    # kernel's <E, d_pooled> - <pooled, d_pooled> leaves 1.9e-6 of fp32 cancellation noise on terms of size ~10.
                    # No existing bound fits; none is invented: pooled and dE are held to theirs, d_scores to (a) and (b) only.
                    S._check_pool(dict(g, ds=(ds0 if acc else torch.zeros_like(ds0))), "", res[lin], dE0, ds0, bf16, acc)
                else:
                    S._check_pool(g, "", res[lin], dE0, ds0, bf16, acc)
    return case, check, [], {}


for _H in (1, 4):
    for _bf in (False, True):
        for _lid in POOL_LENS:
            _register("pool", "H%d-%s-%s" % (_H, "bf16" if _bf else "fp32", _lid))(functools.partial(_pool_factory, _H, _bf, _lid))


def _views_factory(H, bf16):
    """mdl_abmil_pool_view_fwd / _bwd on a 129-index view of dense bags and mdl_abmil_pool_rview_fwd / _bwd on the two half-bag views of
    ragged bags (an empty bag, a one-token bag whose first view is empty); the backward accumulates.  Bounds: as the pools above
    (tests/test_strides_gpu.py::test_pool_views)."""
    dtype, sfx = (BF, "_bf16") if bf16 else (F32, "")
    C = H * 512
    S = _S()
    shapes = {False: (S.DENSE, len(S.DENSE)), True: (S.RAGGED, 2 * len(S.RAGGED))}

    def case(r):
        cases = r.data(lambda: S._view_case(H, bf16))
        st, out = r.stream(), {}
        for ragged, pre in ((False, "view"), (True, "rview")):
            lens, nseg = shapes[ragged]
            T, n = sum(lens), len(lens)
            if cases:
                _, plan, dp, _ = cases[ragged]
                E, s, _, dE0, ds0, _, _ = S._pool_case(H, bf16, lens)
            else:
                plan, dp, E, s, dE0, ds0 = (None, None, None), None, None, None, None, None
            Ev, sd, dpd = r.inp(pre + ".E", (T, C), dtype, E), r.inp(pre + ".scores", (T, H), F32, s), r.inp(pre + ".d_pooled", (nseg, C), F32, dp)
            pooled, m, l_ = r.out(pre + ".pooled", (nseg, C)), r.out(pre + ".m", (nseg, H)), r.out(pre + ".l", (nseg, H))
            dE, dsc = r.inout(pre + ".dE", (T, C), dtype, dE0), r.inout(pre + ".ds", (T, H), F32, ds0)
            if ragged:
                max_view = max((L + 1) // 2 for L in lens)
                assert plan[2] is None or plan[2] == max_view
                perm, vcu = r.inp("perm", (T,), I32, plan[0]), r.inp("vcu", (2 * n + 1,), I64, plan[1])
                r.call("mdl_abmil_pool_rview_fwd" + sfx, Ev, C, sd, pooled, m, l_, n, perm, vcu, max_view, H,
                       r.ws(pre + ".ws", "mdl_abmil_pool_ws_bytes", nseg, max_view, H), st)
                r.freeze(pre + ".pooled", pre + ".m", pre + ".l")
                r.call("mdl_abmil_pool_rview_bwd" + sfx, Ev, C, sd, pooled, m, l_, dpd, dE, dsc, n, perm, vcu, max_view, H, st)
            else:
                idx = r.inp("token_idx", (129,), I32, plan[0])
                r.call("mdl_abmil_pool_view_fwd" + sfx, Ev, C, sd, pooled, m, l_, n, lens[0], idx, 129, H,
                       r.ws(pre + ".ws", "mdl_abmil_pool_ws_bytes", n, 129, H), st)
                r.freeze(pre + ".pooled", pre + ".m", pre + ".l")
                r.call("mdl_abmil_pool_view_bwd" + sfx, Ev, C, sd, pooled, m, l_, dpd, dE, dsc, n, lens[0], idx, 129, H, st)
            out[pre + ".pooled"], out[pre + ".dE"], out[pre + ".ds"] = pooled, dE, dsc
        return out

    def check(got):
        cases = S._view_case(H, bf16)
        for ragged, pre in ((False, "view."), (True, "rview.")):
            lens, _, _, ref = cases[ragged]
            _, _, _, dE0, ds0, _, _ = S._pool_case(H, bf16, lens)
            S._check_pool({k: v.float() for k, v in got.items()}, pre, ref, dE0, ds0, bf16, 1)
    return case, check, [], {}


for _H in (1, 4):
    for _bf in (False, True):
        _register("pool", "views-H%d-%s" % (_H, "bf16" if _bf else "fp32"))(functools.partial(_views_factory, _H, _bf))


def _pool_img_factory(H, lens_id):
    """mdl_abmil_pool_fwd_img / mdl_abmil_pool_dscores_img on the split image of E; d_scores written and accumulated.  Bounds:
    tests/test_strides_gpu.py::test_pool_img."""
    lens = POOL_LENS[lens_id]
    T, n, C = sum(lens), len(lens), H * 512
    dense = lens_id != "ragged"

    def base():
        return _S()._pool_case(H, False, lens)

    def case(r):
        E, s, dp, _, ds0, cu, _ = r.data(base) or (None,) * 7
        st = r.stream()
        Ei, esc = _image_in(r, "E_img", T, C, E)
        sd, dpd = r.inp("scores", (T, H), F32, s), r.inp("d_pooled", (n, C), F32, dp)
        cud = None if dense else r.inp("cu_seqlens", (n + 1,), I64, cu)
        geom = (n, lens[0] if dense else 0, cud, max(lens), H)
        pooled, m, l_ = r.out("pooled", (n, C)), r.out("m", (n, H)), r.out("l", (n, H))
        r.call("mdl_abmil_pool_fwd_img", Ei, 4 * C, esc, sd, pooled, m, l_, *geom, r.ws("ws", "mdl_abmil_pool_ws_bytes", n, max(lens), H), st)
        r.freeze("pooled", "m", "l")
        ds_w, ds_a = r.out("ds0", (T, H)), r.inout("ds1", (T, H), F32, ds0)
        r.call("mdl_abmil_pool_dscores_img", Ei, 4 * C, esc, sd, pooled, m, l_, dpd, ds_w, 0, *geom, st)
        r.call("mdl_abmil_pool_dscores_img", Ei, 4 * C, esc, sd, pooled, m, l_, dpd, ds_a, 1, *geom, st)
        return dict(pooled=pooled, ds0=ds_w, ds1=ds_a)

    def check(got):
        _, _, _, _, ds0, _, res = base()
        pooled, _, dsc = res[False]
        assert rel_err(got["pooled"], pooled) < 1e-5 and max_rel(got["pooled"], pooled) < TOL
        for acc in (0, 1):
            diff = got["ds%d" % acc].double() - (ds0.double() if acc else 0.0)
            assert float((diff - dsc).abs().max()) <= 1e-4 * float(dsc.abs().max()) + 1e-6, acc
    return case, check, [], {}


for _H in (1, 4):
    for _lid in ("ragged", "dense300"):
        _register("pool", "img-H%d-%s" % (_H, _lid))(functools.partial(_pool_img_factory, _H, _lid))


@pytest.mark.parametrize("cid", _ids("pool"))
def test_pool(dev, cid):
    _go(dev, "pool", cid)


# ============================================================================================================ LayerNorm-GELU-Dropout
LN_SHAPES = [(256, 13), (512, 1), (512, 300), (1024, 51), (4096, 9)]
LN_GROUPS = {13: (0, 5, 5, 6, 13), 1: (0, 0, 1), 300: (0, 100, 100, 101, 300), 51: (0, 20, 20, 21, 51)}      # an empty and a one-row group


@functools.lru_cache(maxsize=None)
def _ln_base(W, rows, bf16, grouped):
    """Inputs as tests/test_heads_gpu.py::test_ln_gelu_drop_third_block_width_vs_fp64 draws them, a keep mask at p = 0.1, and the fp64
    y = drop(gelu(LN(x + bias))) with its gradients; grouped: a bias row per group of rows instead of the common one."""
    import torch.nn.functional as F
    D = _D()
    x, dy = D._u((rows, W), 200 + W + rows, 3.0) + 0.5, D._u((rows, W), 230 + W + rows)
    if bf16:
        x, dy = D._bf(x), D._bf(dy)
    g, b = 1 + D._u((W,), 210 + W, 0.2), D._u((W,), 220 + W, 0.3)
    keep = (torch.rand((rows, W), generator=torch.Generator().manual_seed(W + rows)) < 0.9).to(U8)
    cu = torch.tensor(LN_GROUPS[rows], dtype=I64) if grouped else None
    G = len(LN_GROUPS[rows]) - 1 if grouped else 1
    bias = D._u((G, W), 240 + W, 0.7) if grouped else D._u((W,), 240 + W, 0.7)
    leaves = [v.double().requires_grad_() for v in (x, g, b, bias)]
    rows_bias = leaves[3][torch.repeat_interleave(torch.arange(G), cu[1:] - cu[:-1])] if grouped else leaves[3]
    y = F.gelu(F.layer_norm(leaves[0] + rows_bias, (W,), leaves[1], leaves[2], 1e-5)) * keep.double() / 0.9
    y.backward(dy.double())
    return dict(x=x, dy=dy, gamma=g, beta=b, bias=bias, keep=keep, cu=cu, G=G, y=y.detach(), dx=leaves[0].grad, dgamma=leaves[1].grad,
                dbeta=leaves[2].grad, dbias=leaves[3].grad)


def _ln_factory(W, rows, kind, grouped):
    """One LayerNorm-GELU-Dropout pair: kind 'fp32' / 'bf16' (mdl_ln_gelu_drop_fwd / _bwd, _groups) or 'split'
    (mdl_ln_gelu_drop_fwd_split with y, image, rstd_max; mdl_ln_gelu_drop_bwd_split(_groups) with the dx image in exactly rows + 32
    rows: the 32 trailing zero rows are the kernel's to write, over the fill).  Explicit keep mask, p = 0.1.
    Bounds: fp32 tests/test_hip_kernels.py::test_ln_gelu_drop_vs_torch as tests/test_heads_gpu.py restates them (y 1e-5 / 1e-3
    elementwise, dx, dgamma, dbeta 1e-4; dbias / dgroup_bias 1e-4, tests/test_ln_kinds_gpu.py); bf16 tests/test_heads_gpu.py::
    test_ln_gelu_drop_third_block_width_vs_fp64 (dbias / dgroup_bias 1e-2, tests/test_hip_kernels.py::test_ln_gelu_drop_groups_vs_torch);
    split: the plain fp32 kernel's bounds on y, the image quantum of tests/test_strides_gpu.py::_check_image on the image of y, and for
    the dx image the quantum of tests/test_ln_kinds_gpu.py::test_split_backward_equals_plain_backward against the fp64 dx plus the
    plain kernel's 1e-4.  mean and rstd have no bound of their own in the suite: held to (a), (b) and NaN-freedom."""
    bf16 = kind == "bf16"
    dtype = BF if bf16 else F32
    sfx = "_bf16" if bf16 else ""
    g_ = "_groups" if grouped else ""
    G = len(LN_GROUPS[rows]) - 1 if grouped else 1

    def base():
        return _ln_base(W, rows, bf16, grouped)

    def case(r):
        d = r.data(base) or {}
        st = r.stream()
        x, dy = r.inp("x", (rows, W), dtype, d.get("x")), r.inp("dy", (rows, W), dtype, d.get("dy"))
        gamma, beta, keep = r.inp("gamma", (W,), F32, d.get("gamma")), r.inp("beta", (W,), F32, d.get("beta")), r.inp("keep", (rows, W), U8, d.get("keep"))
        bias = r.inp("bias", (G, W) if grouped else (W,), F32, d.get("bias"))
        cu = r.inp("cu_groups", (G + 1,), I64, d.get("cu")) if grouped else None
        groups = (cu, G) if grouped else ()
        mean, rstd = r.out("mean", (rows,)), r.out("rstd", (rows,))
        dgamma, dbeta, dbias = r.out("dgamma", (W,)), r.out("dbeta", (W,)), r.out("dbias", (G, W) if grouped else (W,))
        wsq = "mdl_ln_gelu_drop_bwd%s_ws_bytes" % g_
        out = dict(mean=mean, rstd=rstd, dgamma=dgamma, dbeta=dbeta, dbias=dbias)
        if kind != "split":
            y, dx = r.out("y", (rows, W), dtype), r.out("dx", (rows, W), dtype)
            r.call("mdl_ln_gelu_drop_fwd" + g_ + sfx, x, bias, gamma, beta, y, mean, rstd, rows, W, 1e-5, 0.1, 7, keep, *groups, st)
            r.freeze("mean", "rstd")
            r.call("mdl_ln_gelu_drop_bwd" + g_ + sfx, x, bias, gamma, beta, mean, rstd, dy, dx, dgamma, dbeta, dbias, rows, W, 0.1, 7, keep, *groups,
                   r.ws("ws", wsq, rows, W, *groups[1:]), st)
            out.update(y=y, dx=dx)
            return out
        # split: the grouped entry takes x with the group rows already added (tests/test_ln_kinds_gpu.py::ln_bwd_split) and a common bias
        y, img, scale, rmax = r.out("y", (rows, W)), r.out("img", (rows, W)), r.out("scale", (2,)), r.out("rstd_max", (1,))
        img_only, scale2 = r.out("img_only", (rows, W)), r.out("scale_only", (2,))
        mean2, rstd2 = r.out("mean_only", (rows,)), r.out("rstd_only", (rows,))
        xs = x
        if grouped:
            xg = None if d.get("x") is None else d["x"] + d["bias"][torch.repeat_interleave(torch.arange(G), d["cu"][1:] - d["cu"][:-1])]
            xs, bias = r.inp("x_plus_group_rows", (rows, W), F32, xg), None
        r.call("mdl_ln_gelu_drop_fwd_split", xs, bias, gamma, beta, y, img, scale, mean, rstd, rows, W, 1e-5, 0.1, 7, keep, None, rmax, st)
        r.call("mdl_ln_gelu_drop_fwd_split", xs, bias, gamma, beta, None, img_only, scale2, mean2, rstd2, rows, W, 1e-5, 0.1, 7, keep, None, None, st)
        r.freeze("mean", "rstd", "rstd_max")
        dx_img, dx_scale = r.out("dx_img", (rows + 32, W)), r.out("dx_scale", (2,))
        tail = (cu, G, dbias) if grouped else ()
        r.call("mdl_ln_gelu_drop_bwd_split" + g_, xs, bias, gamma, beta, mean, rstd, dy, None, dx_img, dx_scale, dgamma, dbeta,
               None if grouped else dbias, rows, W, 0.1, 7, keep, None, rmax, *tail, r.ws("ws", wsq, rows, W, *groups[1:]), st)
        out.update(y=y, img=img, scale=scale, dx_img=dx_img, dx_scale=dx_scale, rstd_max=rmax, img_only=img_only, scale_only=scale2,
                   mean_only=mean2, rstd_only=rstd2)
        return out

    def check(got):
        S, d = _S(), base()
        y, dx = d["y"], d["dx"]
        if kind == "bf16":
            out = got["y"].double()
            assert float(((out - y).abs() - EPS_BF16 * y.abs()).max()) < 1e-4 and rel_err(out, y) < EPS_BF16, "y"
            assert rel_err(got["dx"].float(), dx) < EPS_BF16, "dx"
            assert rel_err(got["dgamma"], d["dgamma"]) < 6e-4 and rel_err(got["dbeta"], d["dbeta"]) < 6e-4
            assert rel_err(got["dbias"], d["dbias"]) < 1e-2
            return
        assert rel_err(got["y"], y) < 1e-5 and max_rel(got["y"], y) < TOL, "y"
        assert rel_err(got["dgamma"], d["dgamma"]) < 1e-4 and rel_err(got["dbeta"], d["dbeta"]) < 1e-4 and rel_err(got["dbias"], d["dbias"]) < 1e-4
        if grouped:
            empty = [i for i in range(G) if LN_GROUPS[rows][i] == LN_GROUPS[rows][i + 1]]
            assert empty and all(float(got["dbias"][i].abs().max()) == 0.0 for i in empty), "the empty group"
        if kind == "fp32":
            assert rel_err(got["dx"], dx) < 1e-4, "dx"
            return
        S._check_image(got["img"], got["scale"][0], got["y"], W)
        for a, b in (("img", "img_only"), ("scale", "scale_only"), ("mean", "mean_only"), ("rstd", "rstd_only")):
            assert torch.equal(got[a].view(I32), got[b].view(I32)), b          # tests/test_ln_kinds_gpu.py::test_split_forward_equals_plain_forward
        assert float(got["rstd_max"]) == float(got["rstd"].max())
        s0 = float(got["dx_scale"][0])
        dec = S._decode(got["dx_img"][:rows], W) / s0
        assert rel_err(dec, dx) < 1e-4, "dx image"
        assert not got["dx_img"][rows:].any(), "the 32 zero rows behind the dx image"
    return case, check, [], {}


for _W, _rows in LN_SHAPES:
    for _kind in ("fp32", "bf16", "split"):
        _register("ln", "%s-W%d-rows%d" % (_kind, _W, _rows))(functools.partial(_ln_factory, _W, _rows, _kind, False))
        if _W <= 1024:      # the grouped forms: W in {256, 512, 1024}
            _register("ln", "%s-groups-W%d-rows%d" % (_kind, _W, _rows))(functools.partial(_ln_factory, _W, _rows, _kind, True))


@pytest.mark.parametrize("cid", _ids("ln"))
def test_ln_gelu_drop(dev, cid):
    _go(dev, "ln", cid)


# ============================================================================================================================ InfoNCE
def _nce_factory(S_, Kmax, D, cnts, sym):
    """mdl_infonce_fwd / _bwd: S problems of cnts rows in [S, Kmax, D] blocks, mean losses and per-row losses, gradients of the mean
    (d_loss) and of the rows (d_row_loss).  Bounds: tests/test_hip_kernels.py::test_infonce_reduction_none_sum_and_odd_width and
    ::test_infonce_staged_path (loss 1e-5, gradients 1e-4 relative).
    D = 37 goes in as the Python mirror passes it: zero-padded to 64 columns (the entry points refuse D % 32 != 0 with MDL_E_ARG,
    which the header did not say before this test was written; it does now)."""
    T = 0.07
    Dp = (D + 31) // 32 * 32      # the C entry points take D % 32 == 0: a narrower embedding arrives with zero columns behind it

    def data():
        D_ = _D()
        Q, P = D_._u((S_, Kmax, D), 500 + Kmax + D), D_._u((S_, Kmax, D), 501 + Kmax + D)
        P = P + 0.3 * Q
        return Q, P, torch.tensor(cnts, dtype=I32), D_._u((S_,), 502).abs() + 0.5, D_._u((S_, Kmax), 503).abs() + 0.1

    def ref():
        import torch.nn.functional as F
        Q, P, cnt, dl, dr = data()
        q, p = Q.double().requires_grad_(), P.double().requires_grad_()
        rows = torch.zeros(S_, Kmax, dtype=F64)
        means = []
        for s, k in enumerate(cnts):
            if k == 0:
                means.append(torch.zeros((), dtype=F64))
                continue
            lg = F.normalize(q[s, :k], dim=-1) @ F.normalize(p[s, :k], dim=-1).t() / T
            ce = F.cross_entropy(lg, torch.arange(k), reduction="none")
            if sym:
                ce = 0.5 * ce + 0.5 * F.cross_entropy(lg.t(), torch.arange(k), reduction="none")
            rows = rows + F.pad(ce, (0, Kmax - k))[None, :] * F.one_hot(torch.tensor(s), S_).double()[:, None]
            means.append(ce.mean())
        means = torch.stack(means)
        g_mean = torch.autograd.grad((means * dl.double()).sum(), (q, p), retain_graph=True)
        g_rows = torch.autograd.grad((rows * dr.double()).sum(), (q, p))
        return means.detach(), rows.detach(), g_mean, g_rows

    def case(r):
        Q, P, cnt, dl, dr = r.data(data) or (None,) * 5
        st = r.stream()
        pad = (lambda x: None if x is None else torch.nn.functional.pad(x, (0, Dp - D)))
        Qd, Pd, cd = r.inp("Q", (S_, Kmax, Dp), F32, pad(Q)), r.inp("P", (S_, Kmax, Dp), F32, pad(P)), r.inp("cnt", (S_,), I32, cnt)
        dld, drd = r.inp("d_loss", (S_,), F32, dl), r.inp("d_row_loss", (S_, Kmax), F32, dr)
        out = {}
        for tag, want_rows in (("mean", False), ("rows", True)):
            loss, rows = r.out(tag + ".loss", (S_,)), (r.out(tag + ".row_loss", (S_, Kmax)) if want_rows else None)
            ws = r.ws(tag + ".ws", "mdl_infonce_ws_bytes", S_, Kmax, Dp)
            r.call("mdl_infonce_fwd", Qd, Pd, cd, loss, rows, S_, Kmax, Dp, T, int(sym), ws, st)
            dQ, dP = r.out(tag + ".dQ", (S_, Kmax, Dp)), r.out(tag + ".dP", (S_, Kmax, Dp))
            r.call("mdl_infonce_bwd", Qd, Pd, None if want_rows else dld, drd if want_rows else None, cd, dQ, dP, S_, Kmax, Dp, T, int(sym), ws, st)
            out.update({tag + ".loss": loss, tag + ".dQ": dQ, tag + ".dP": dP})
            if want_rows:
                out[tag + ".row_loss"] = rows
        return out

    def check(got):
        means, rows, g_mean, g_rows = ref()
        for tag in ("mean", "rows"):
            assert float((got[tag + ".loss"].double() - means).abs().max()) <= 1e-5 * float(means.abs().max()), tag
        assert rel_err(got["rows.row_loss"], rows) < 1e-5
        for tag, g in (("mean", g_mean), ("rows", g_rows)):
            assert rel_err(got[tag + ".dQ"][..., :D], g[0]) < 1e-4 and rel_err(got[tag + ".dP"][..., :D], g[1]) < 1e-4, tag
            assert not got[tag + ".dQ"][..., D:].any() and not got[tag + ".dP"][..., D:].any(), "the zero columns"
            for s, k in enumerate(cnts):      # rows >= cnt[s] are zeroed
                assert not got[tag + ".dQ"][s, k:].any() and not got[tag + ".dP"][s, k:].any()
    return case, check, [], {}


for _k in (2, 33):
    for _Dn in (37, 64):
        _register("infonce", "S1-k%d-D%d" % (_k, _Dn))(functools.partial(_nce_factory, 1, _k, _Dn, (_k,), _k == 33))
_register("infonce", "S3-unequal-counts")(functools.partial(_nce_factory, 3, 33, 37, (33, 7, 0), True))
_register("infonce", "staged-k300-D64")(functools.partial(_nce_factory, 1, 300, 64, (300,), True))


def _nce_neg_factory(N, M, D, paired):
    """mdl_infonce_neg_fwd / _bwd, paired and unpaired, M = 0 included; Q and P are [N, Dq] with Dq = D rounded up to 32 and zero
    padding columns.  Bounds: tests/test_infonce_negatives_gpu.py::check_against_fp64 (loss 1e-3 relative + 1e-5; gradients 1e-3)."""
    T = 0.05
    Dq = (D + 31) // 32 * 32

    def data():
        D_ = _D()
        q, p = D_._u((N, D), 600 + N + D), D_._u((N, D), 601 + N + D)
        p = p + 0.3 * q
        neg = D_._u((N, M, D) if paired else (M, D), 602 + N + M)
        return q, p, neg, D_._u((N,), 603).abs() + 0.1

    def ref():
        import torch.nn.functional as F
        q, p, neg, dr = data()
        q64, p64, n64 = q.double().requires_grad_(), p.double().requires_grad_(), neg.double().requires_grad_()
        qh, ph = (x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12) for x in (q64, p64))
        nh = n64 / n64.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        pos = (qh * ph).sum(-1, keepdim=True)
        ng = torch.einsum("nd,nmd->nm", qh, nh) if paired else qh @ nh.t()
        rows = F.cross_entropy(torch.cat([pos, ng], 1) / T, torch.zeros(N, dtype=torch.long), reduction="none")
        g_mean = torch.autograd.grad(rows.mean(), (q64, p64, n64), retain_graph=True, allow_unused=True)
        g_rows = torch.autograd.grad((rows * dr.double()).sum(), (q64, p64, n64), allow_unused=True)
        return rows.detach(), g_mean, g_rows

    def case(r):
        q, p, neg, dr = r.data(data) or (None,) * 4
        st = r.stream()
        pad = (lambda x: None if x is None else torch.nn.functional.pad(x, (0, Dq - D)))
        Qd, Pd = r.inp("Q", (N, Dq), F32, pad(q)), r.inp("P", (N, Dq), F32, pad(p))
        nshape = (N, M, D) if paired else (M, D)
        Nd = r.inp("Neg", nshape, F32, neg) if M else None
        one, drd = r.inp("d_loss", (1,), F32, torch.ones(1)), r.inp("d_row_loss", (N,), F32, dr)
        out = {}
        for tag, want_rows in (("mean", False), ("rows", True)):
            loss, rows = (None if want_rows else r.out(tag + ".loss", (1,))), (r.out(tag + ".row_loss", (N,)) if want_rows else None)
            ws = r.ws(tag + ".ws", "mdl_infonce_neg_ws_bytes", N, M, D, int(paired))
            r.call("mdl_infonce_neg_fwd", Qd, Pd, Nd, loss, rows, N, M, D, int(paired), T, ws, st)
            dQ, dP = r.out(tag + ".dQ", (N, Dq)), r.out(tag + ".dP", (N, Dq))
            dN = r.out(tag + ".dNeg", nshape) if (M and want_rows) else None          # (mean: dNeg = NULL, skipped entirely)
            r.call("mdl_infonce_neg_bwd", Nd, None if want_rows else one, drd if want_rows else None, dQ, dP, dN, N, M, D, int(paired), T, ws, st)
            out.update({tag + ".dQ": dQ, tag + ".dP": dP})
            out[tag + (".row_loss" if want_rows else ".loss")] = rows if want_rows else loss
            if dN is not None:
                out[tag + ".dNeg"] = dN
        return out

    def check(got):
        rows, g_mean, g_rows = ref()
        r64 = float(rows.mean())
        assert abs(float(got["mean.loss"]) - r64) <= TOL * abs(r64) + 1e-5
        assert float((got["rows.row_loss"].double() - rows).abs().max()) <= TOL * float(rows.abs().max()) + 1e-5
        for tag, g in (("mean", g_mean), ("rows", g_rows)):
            for n, i in (("dQ", 0), ("dP", 1)):
                if M == 0:
                    assert not got["%s.%s" % (tag, n)].any(), "M = 0: zero gradients"
                else:
                    assert rel_err(got["%s.%s" % (tag, n)][:, :D], g[i]) < TOL, (tag, n)
                    assert float(got["%s.%s" % (tag, n)][:, D:].abs().max() if Dq > D else 0.0) <= 1e-6 * float(g[i].abs().max()), "padding columns"
        if M:
            assert rel_err(got["rows.dNeg"], g_rows[2]) < TOL
    plans = [("infonce_neg", N, M, D, dict(variant=int(D % 4 == 0)))] if (M and not paired) else []
    return case, check, plans, {}


for _N, _M, _Dn in ((5, 7, 37), (33, 65, 64), (5, 0, 37)):
    for _pr in (False, True):
        _register("infonce", "neg-%s-N%d-M%d-D%d" % ("paired" if _pr else "unpaired", _N, _M, _Dn))(functools.partial(_nce_neg_factory, _N, _M, _Dn, _pr))


@pytest.mark.parametrize("cid", _ids("infonce"))
def test_infonce(dev, cid):
    _go(dev, "infonce", cid)


# ================================================================================================================================ GOT
# Never a shape in the split-sweep class: 128 < n <= 256 on the RESIDENT entry points with 2 k <= compute units.  Those sweeps run as
# two workgroups per case that spin-wait on each other through 8-byte granules in the workspace; a mis-carved workspace there is a
# one-second stall per sweep, not a failed assertion.  The resident cases below stay at n <= 128 or n > 256 and assert the plan;
# n = 130 runs on the tiled entry points only, whose workgroups meet at kernel boundaries.
GOT_PREFIX = {"resident": "mdl_got", "tiled": "mdl_got_tiled", "rect": "mdl_got_tiled_rect"}


@functools.lru_cache(maxsize=None)
def _got_base(k, n, m, d):
    """Token sets as tests/test_hip_kernels.py::test_got_large_n_vs_fp64_oracle draws them and the fp64 oracle (oracle.restatement.
    got_parts): (WD sum, GWD sum), their extrema, and the gradients of WD + GWD."""
    from oracle import restatement as R
    from tests._util import t
    v = t((k, n, d), "extents:got:v:%d:%d:%d" % (k, n, d))
    q = t((k, m, d), "extents:got:q:%d:%d:%d" % (k, m, d))
    q = q + 0.7 * (v if n == m else v[:, torch.arange(m) % n])
    v64, q64 = v.double().requires_grad_(), q.double().requires_grad_()
    parts = R.got_parts(v64, q64)
    parts.sum().backward()
    return v, q, parts.detach(), R.got_extrema(v.double(), q.double()), v64.grad, q64.grad


def _got_bounds(cls):
    """(value, gradient): tests/test_hip_kernels.py::test_got_large_n_vs_fp64_oracle for the resident classes, VAL_TOL / GRAD_TOL of
    tests/test_got_tiled_gpu.py (tests/test_got_rect_gpu.py uses them unchanged) for the tiled ones."""
    if cls == "resident":
        return TOL, TOL
    from tests.test_got_tiled_gpu import GRAD_TOL, VAL_TOL
    return VAL_TOL, GRAD_TOL


def _got_factory(cls, k, n, m, d, want):
    """The six entry points of one GOT class: extrema alone; fwd (minmax_out) + bwd; fwd + bwd_begin (d_minmax NULL) + bwd_finish
    (d_minmax_total NULL), whose dV, dQ equal the one-call backward bit for bit; fwd with minmax_in (this batch's own extrema, so the
    result is the local one) + bwd_begin (d_minmax) + bwd_finish (d_minmax_total = that d_minmax).  Every sequence has a workspace of
    its own at exactly the query's bytes."""
    assert cls != "resident" or not 128 < n <= 256, "the split-sweep class is out of scope (see above)"
    pre = GOT_PREFIX[cls]
    sizes = (k, n, m, d) if cls == "rect" else (k, n, d)
    wsq = pre + "_ws_bytes"

    def case(r):
        b = r.data(lambda: _got_base(k, n, m, d))
        v, q = (b[0], b[1]) if b else (None, None)
        st = r.stream()
        V, Q, one = r.inp("V", (k, n, d), F32, v), r.inp("Q", (k, m, d), F32, q), r.inp("d_out", (2,), F32, torch.ones(2))
        mm0 = r.out("ext.minmax", (6,))
        r.call(pre + "_extrema", V, Q, mm0, *sizes, r.ws("ext.ws", wsq, *sizes), st)
        out = {"ext.minmax": mm0}
        # one-call backward
        o, mm, dV, dQ, ws = r.out("a.out", (2,)), r.out("a.minmax", (6,)), r.out("a.dV", (k, n, d)), r.out("a.dQ", (k, m, d)), r.ws("a.ws", wsq, *sizes)
        r.call(pre + "_fwd", V, Q, o, mm, None, *sizes, ws, st)
        r.call(pre + "_bwd", V, Q, one, dV, dQ, *sizes, ws, st)
        out.update({"a.out": o, "a.minmax": mm, "a.dV": dV, "a.dQ": dQ})
        r.freeze("a.minmax")
        # two steps, nothing exchanged
        o, dV, dQ, ws = r.out("b.out", (2,)), r.out("b.dV", (k, n, d)), r.out("b.dQ", (k, m, d)), r.ws("b.ws", wsq, *sizes)
        r.call(pre + "_fwd", V, Q, o, None, None, *sizes, ws, st)
        r.call(pre + "_bwd_begin", one, None, *sizes, ws, st)
        r.call(pre + "_bwd_finish", V, Q, dV, dQ, None, *sizes, ws, st)
        out.update({"b.out": o, "b.dV": dV, "b.dQ": dQ})
        # the data-parallel form: extrema in, d_minmax out and back in
        o, dmm, dV, dQ, ws = r.out("c.out", (2,)), r.out("c.d_minmax", (6,)), r.out("c.dV", (k, n, d)), r.out("c.dQ", (k, m, d)), r.ws("c.ws", wsq, *sizes)
        r.call(pre + "_fwd", V, Q, o, None, mm, *sizes, ws, st)
        r.call(pre + "_bwd_begin", one, dmm, *sizes, ws, st)
        r.freeze("c.d_minmax")
        r.call(pre + "_bwd_finish", V, Q, dV, dQ, dmm, *sizes, ws, st)
        out.update({"c.out": o, "c.d_minmax": dmm, "c.dV": dV, "c.dQ": dQ})
        return out

    def check(got):
        _, _, parts, ext, gv, gq = _got_base(k, n, m, d)
        vt, gt = _got_bounds(cls)
        ref = float(parts.sum())
        assert torch.equal(got["ext.minmax"], got["a.minmax"]) and rel_err(got["a.minmax"], ext) < 1e-5      # (1e-5: fp32 costs 1 - cos)
        for s_ in "abc":
            assert abs(float(got[s_ + ".out"].double().sum()) - ref) < vt * abs(ref), s_
            assert rel_err(got[s_ + ".dV"], gv) < gt and rel_err(got[s_ + ".dQ"], gq) < gt, s_
        assert torch.equal(got["a.out"], got["b.out"]) and torch.equal(got["a.dV"], got["b.dV"]) and torch.equal(got["a.dQ"], got["b.dQ"])
    plans = [("got", k, n, 0, want)] if cls == "resident" else [("got_tiled" if cls == "tiled" else "got_tiled_rect", k, n, d if cls == "tiled" else m, want)]
    return case, check, plans, {}


_register("got", "resident-k2-n65-d100")(functools.partial(_got_factory, "resident", 2, 65, 65, 100, dict(variant=128, extra=0)))
_register("got", "resident-k1-n257-d128-whole_sweeps")(functools.partial(_got_factory, "resident", 1, 257, 257, 128, dict(variant=512, extra=0)))
_register("got", "tiled-k2-n130-d20")(functools.partial(_got_factory, "tiled", 2, 130, 130, 20, dict(variant=16, extra=2)))
_register("got", "rect-k2-n130-m33-d20")(functools.partial(_got_factory, "rect", 2, 130, 33, 20, dict(variant=16, splits=9)))
_register("got", "rect-k2-n33-m130-d20")(functools.partial(_got_factory, "rect", 2, 33, 130, 20, dict(variant=16, splits=3)))


def _got_multi_factory():
    """The four _multi entry points on np = 2 problems of different k, (2, 65, 100) and (1, 65, 100): every V, Q, out, gradient,
    extrema row and workspace is an arena buffer, handed over through host arrays of device addresses.  Bound: as the resident class."""
    import ctypes
    ks, n, d = (2, 1), 65, 100

    def case(r):
        st = r.stream()
        bases = [r.data(lambda k=k: _got_base(k, n, n, d)) for k in ks]
        V = [r.inp("V%d" % i, (k, n, d), F32, b and b[0]) for i, (k, b) in enumerate(zip(ks, bases))]
        Q = [r.inp("Q%d" % i, (k, n, d), F32, b and b[1]) for i, (k, b) in enumerate(zip(ks, bases))]
        ws = [r.ws("ws%d" % i, "mdl_got_ws_bytes", k, n, d) for i, k in enumerate(ks)]
        d_out = r.inp("d_out", (2, 2), F32, torch.ones(2, 2))
        mm, out, dmm = r.out("minmax", (2, 6)), r.out("out", (2, 2)), r.out("d_minmax", (2, 6))
        dV = [r.out("dV%d" % i, (k, n, d)) for i, k in enumerate(ks)]
        dQ = [r.out("dQ%d" % i, (k, n, d)) for i, k in enumerate(ks)]
        ka, na = (ctypes.c_int * 2)(*ks), (ctypes.c_int * 2)(n, n)
        r.call("mdl_got_extrema_multi", 2, r.ptrs(V), r.ptrs(Q), r.ptrs(mm, rows=True), ka, na, d, r.ptrs(ws), st)
        r.freeze("minmax")
        r.call("mdl_got_fwd_multi", 2, r.ptrs(V), r.ptrs(Q), r.ptrs(out, rows=True), r.ptrs(mm, rows=True), ka, na, d, r.ptrs(ws), st)
        r.call("mdl_got_bwd_begin_multi", 2, r.ptrs(d_out, rows=True), r.ptrs(dmm, rows=True), ka, na, d, r.ptrs(ws), st)
        r.freeze("d_minmax")
        r.call("mdl_got_bwd_finish_multi", 2, r.ptrs(V), r.ptrs(Q), r.ptrs(dV), r.ptrs(dQ), r.ptrs(dmm, rows=True), ka, na, d, r.ptrs(ws), st)
        res = dict(minmax=mm, out=out)
        res.update({"dV%d" % i: x for i, x in enumerate(dV)})
        res.update({"dQ%d" % i: x for i, x in enumerate(dQ)})
        return res

    def check(got):
        for i, k in enumerate(ks):
            _, _, parts, ext, gv, gq = _got_base(k, n, n, d)
            assert rel_err(got["minmax"][i], ext) < 1e-5
            assert abs(float(got["out"][i].double().sum()) - float(parts.sum())) < TOL * abs(float(parts.sum()))
            assert rel_err(got["dV%d" % i], gv) < TOL and rel_err(got["dQ%d" % i], gq) < TOL
    return case, check, [("got", 3, 65, 0, dict(variant=128, extra=0))], {}


_register("got", "multi-np2-k2_k1-n65-d100")(_got_multi_factory)


@pytest.mark.parametrize("cid", _ids("got"))
def test_got(dev, cid):
    _go(dev, "got", cid)


# ============================================================================================================================== AdamW
ADAMW_NUMEL = (1, 4097, 12289)


def _adamw_factory():
    """mdl_adamw_grad_stats, _update, _commit over three tensors of 1, 4097 and 12289 elements with CLIP and GUARD on: one step from
    zero moments.  The gradients are views at odd 4-byte offsets (1, 2, 4099 floats) inside one `in` buffer, so a 16-byte access that
    ignored the offset would read its neighbours; parameters, moments and steps are inout buffers of exactly numel floats.
    Bar: tests/test_adamw_gpu.py::check_parity, E(ours) <= 2 E(torch fp32) against torch's fp64 run; the norm to 1e-6
    (::test_parity_with_torch_adamw)."""
    from madeleine_amd import functional as MF
    lr, b1, b2, eps, wd, clip = 1e-3, 0.9, 0.999, 1e-8, 1e-2, 0.5
    offs = [1, 2, 4099]
    total = offs[-1] + ADAMW_NUMEL[-1] + 2

    def data():
        p = [torch.sin(torch.arange(n, dtype=F64) * 0.37 + i) * 0.05 for i, n in enumerate(ADAMW_NUMEL)]
        g = [torch.sin(torch.arange(n, dtype=F64) * 0.11 + 1.3 * i) * 10.0 ** (i - 3) for i, n in enumerate(ADAMW_NUMEL)]
        gbuf = torch.full((total,), 7.0)                    # finite neighbours: a load past a tensor's end would change the norm
        for o, x in zip(offs, g):
            gbuf[o:o + x.numel()] = x.float()
        return p, g, gbuf

    def ref(dtype):
        p, g, _ = data()
        params = [torch.nn.Parameter(x.float().to(dtype)) for x in p]
        opt = torch.optim.AdamW(params, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False, fused=False)
        for x, gg in zip(params, g):
            x.grad = gg.float().to(dtype)
        torch.nn.utils.clip_grad_norm_(params, clip, foreach=False)
        opt.step()
        return [x.detach() for x in params], [opt.state[x]["exp_avg"] for x in params], [opt.state[x]["exp_avg_sq"] for x in params]

    def case(r):
        d = r.data(data)
        st = r.stream()
        gbuf = r.inp("grads", (total,), F32, d and d[2])
        P = [r.inout("p%d" % i, (n,), F32, d and d[0][i]) for i, n in enumerate(ADAMW_NUMEL)]
        M = [r.inout("m%d" % i, (n,), F32, torch.zeros(n)) for i, n in enumerate(ADAMW_NUMEL)]
        Vv = [r.inout("v%d" % i, (n,), F32, torch.zeros(n)) for i, n in enumerate(ADAMW_NUMEL)]
        St = [r.inout("step%d" % i, (1,), F32, torch.zeros(1)) for i in range(3)]
        norm, skipped = r.out("grad_norm", (1,)), r.inout("skipped", (1,), I64, torch.zeros(1, dtype=I64))
        ws = r.ws("ws", "mdl_adamw_ws_bytes", 1)
        G = [gbuf[o:o + n] for o, n in zip(offs, ADAMW_NUMEL)]
        assert r.planning or all(x.data_ptr() % 16 for x in G)
        numel = MF.adamw_sizes(P)
        flags = MF.ADAMW_GUARD | MF.ADAMW_CLIP
        bits = [MF._f64_bits(x) for x in (lr, b1, b2, eps, wd, clip)]
        r.call("mdl_adamw_grad_stats", 3, r.ptrs(G), numel, ws, 0, 1, st)
        r.call("mdl_adamw_update", 3, r.ptrs(P), r.ptrs(G), r.ptrs(M), r.ptrs(Vv), r.ptrs(St), numel, *bits, flags, ws, 1, st)
        r.call("mdl_adamw_commit", 3, r.ptrs(St), flags | MF.ADAMW_FINAL, ws, 1, norm, skipped, st)
        res = dict(grad_norm=norm, skipped=skipped)
        for i in range(3):
            res.update({"p%d" % i: P[i], "m%d" % i: M[i], "v%d" % i: Vv[i], "step%d" % i: St[i]})
        return res

    def check(got):
        from tests.test_adamw_gpu import E
        r64, r32 = ref(F64), ref(torch.float32)
        for j, k in enumerate("pmv"):
            ours, torchs = E([got["%s%d" % (k, i)] for i in range(3)], r64[j]), E(r32[j], r64[j])
            assert ours <= 2.0 * torchs, (k, ours, torchs)
        assert all(float(got["step%d" % i]) == 1.0 for i in range(3)) and int(got["skipped"]) == 0
        nrm = float(torch.sqrt(sum((x.float().double() ** 2).sum() for x in data()[1])))
        assert abs(float(got["grad_norm"]) - nrm) <= 1e-6 * nrm
    return case, check, [], {}


_register("adamw", "three-tensors-odd-offsets-clip-guard")(_adamw_factory)


@pytest.mark.parametrize("cid", _ids("adamw"))
def test_adamw(dev, cid):
    _go(dev, "adamw", cid)


# ================================================================================================================ evaluation kernels
def _table(idx_lists):
    """(train_idx [P, n_max] int32 padded with -1, n_train [P] int32): madeleine_amd.probe._problem_table on the CPU."""
    n = [int(t.numel()) for t in idx_lists]
    table = torch.full((len(n), max(n)), -1, dtype=I32)
    for p_, t in enumerate(idx_lists):
        table[p_, :n[p_]] = t.to(I32)
    return table, torch.tensor(n, dtype=I32)


def _fit_factory(kind, name, dims):
    """mdl_probe_fit / mdl_logit_fit, mdl_probe_scores and mdl_probe_metrics / mdl_logit_metrics over a cohort of the suite's
    references (tests/_probe_ref.py: A = (160, 64, C 2), B = (160, 48, C 3); tests/_probe_cv_ref.py: FA = (400, 24, C 2), FB = (400, 70,
    C 3): d = 70 is no multiple of 4, C = 3 takes the multinomial kernels), all problems in one launch sequence, ld = d.
    Bounds: every problem converges and E_p = max |z - z64| / max |z64| <= 1e-3 (tests/test_probe_gpu.py::test_decision_values,
    tests/test_probe_cv_gpu.py::test_decision_values); the metrics against the recount from the device's own scores: the confusion
    matrix exactly, the AUC to 1e-6 (tests/test_probe_cv_gpu.py::test_metrics_consistent_with_device_scores)."""
    S, d, C, P, n_max = dims
    cols = 1 if C == 2 else C
    fit, metr = ("mdl_probe_fit", "mdl_probe_metrics") if kind == "probe" else ("mdl_logit_fit", "mdl_logit_metrics")

    def cohort():
        from tests import _probe_cv_ref, _probe_ref
        co = (_probe_ref if kind == "probe" else _probe_cv_ref).cohort(name)
        assert (co["X"].shape, co["C"], len(co["problems"])) == ((S, d), C, P)
        return co

    def case(r):
        co = r.data(cohort)
        tb = _table([p_["idx"] for p_ in co["problems"]]) if co else (None, None)
        assert co is None or tb[0].shape == (P, n_max)
        st = r.stream()
        X, y = r.inp("X", (S, d), F32, co and co["X"].float()), r.inp("y", (S,), I32, co and co["y"])
        ti, nt = r.inp("train_idx", (P, n_max), I32, tb[0]), r.inp("n_train", (P,), I32, tb[1])
        W, b, info = r.out("W", (P, cols, d)), r.out("b", (P, cols)), r.out("info", (P, 4))
        r.call(fit, X, d, S, d, y, 0, ti, nt, P, n_max, C, 1.0, 1e-4, 100, W, b, info, r.ws("ws_fit", fit + "_ws_bytes", P, n_max, d, C), st)
        r.freeze("W", "b")
        z = r.out("z", (P, S, cols))
        r.call("mdl_probe_scores", X, d, S, d, W, b, P, C, z, st)
        r.freeze("z")
        conf, auc = r.out("confusion", (P, C, C), I32), r.out("auc", (P,))
        r.call(metr, z, y, 0, ti, nt, P, n_max, S, C, conf, auc, r.ws("ws_metrics", metr + "_ws_bytes", P, S, C), st)
        return dict(W=W, b=b, info=info, z=z, conf=conf, auc=auc)

    def check(got):
        from tests import _probe_ref as R_
        co = cohort()
        for p_, pr in enumerate(co["problems"]):
            assert got["info"][p_, 1] == 1, (p_, got["info"][p_])
            E = float((got["z"][p_].double() - pr["z64"]).abs().max() / pr["z64"].abs().max())
            assert E <= 1e-3, (p_, E)
            test = R_.test_mask(co["y"].clone(), pr["idx"])
            assert torch.equal(got["conf"][p_].long(), R_.confusion(got["z"][p_].double(), co["y"], test, C)), p_
            assert abs(float(got["auc"][p_]) - R_.auc(got["z"][p_].double(), co["y"], test, C)) <= 1e-6, p_
    return case, check, [], {}


def _fit_entry(kind, name):
    def factory():
        from tests import _probe_cv_ref, _probe_ref
        if kind == "probe":
            from madeleine_amd.probe import probe_splits
            S, d, C, sep, _ = _probe_ref.COHORTS[name]
            y = _probe_ref.recipe(S, d, C, sep)[1]
            lists = [probe_splits(y, k, f) for k in _probe_ref.KS for f in _probe_ref.FOLDS]
        else:
            from madeleine_amd.probe import cv_splits
            S, d, C, sep, _ = _probe_cv_ref.COHORTS[name]
            lists = list(cv_splits(_probe_cv_ref.recipe(S, d, C, sep)[1]))
        return _fit_factory(kind, name, (S, d, C, len(lists), max(int(t.numel()) for t in lists)))
    return factory


for _kind, _name in (("probe", "A"), ("probe", "B"), ("logit", "FA"), ("logit", "FB")):
    _register("eval", "%s-%s" % (_kind, _name))(_fit_entry(_kind, _name))


def _cox_factory():
    """mdl_cox_fit, mdl_probe_scores (C = 2, zero intercept) and mdl_surv_metrics over cohort A of tests/_survival_ref.py (S 330, d 4,
    training lists of 1 .. 257 rows: S, and all sizes but two, are no multiples of 4).  Bounds: tests/test_survival_gpu.py::
    test_decision_values (E_p <= 1e-3, thr the median of the device's own scores bit for bit) and ::test_metrics_equal_the_host_recount
    (the six counts exactly, the two doubles to 1e-12)."""
    from tests import _survival_ref as R_
    S, d, _, _, _, cost, sizes = R_.COHORTS["A"]
    P, n_max = len(sizes), max(sizes)

    def case(r):
        co = r.data(lambda: R_.cohort("A"))
        tb = _table([p_["idx"] for p_ in co["problems"]]) if co else (None, None)
        st = r.stream()
        X = r.inp("X", (S, d), F32, co and co["X"].float())
        tm, ev = r.inp("time", (S,), F32, co and co["time"]), r.inp("event", (S,), I32, co and co["event"])
        ti, nt = r.inp("train_idx", (P, n_max), I32, tb[0]), r.inp("n_train", (P,), I32, tb[1])
        W, thr, info = r.out("W", (P, d)), r.out("thr", (P,)), r.out("info", (P, 4))
        r.call("mdl_cox_fit", X, d, S, d, tm, 0, ev, 0, ti, nt, P, n_max, float(cost), 1e-3, 100, W, thr, info,
               r.ws("ws_fit", "mdl_cox_order_fit_ws_bytes", P, n_max, d), st)
        r.freeze("W", "thr")
        z, zero = r.out("z", (P, S)), r.inp("zero_intercept", (P, 1), F32, torch.zeros(P, 1))
        r.call("mdl_probe_scores", X, d, S, d, W, zero, P, 2, z, st)
        r.freeze("z")
        c, chi2, counts = r.out("c_index", (P,), F64), r.out("chi2", (P,), F64), r.out("counts", (P, 6), I32)
        r.call("mdl_surv_metrics", z, tm, 0, ev, 0, ti, nt, P, n_max, S, thr, c, chi2, counts, r.ws("ws_metrics", "mdl_surv_metrics_ws_bytes", P, S), st)
        return dict(W=W, thr=thr, info=info, z=z, c=c, chi2=chi2, counts=counts)

    def check(got):
        from tests.test_survival_gpu import _same
        co = R_.cohort("A")
        tm, ev = co["time"].numpy(), co["event"].numpy()
        for p_, pr in enumerate(co["problems"]):
            z, z64 = got["z"][p_].double(), pr["z64"]
            assert got["info"][p_, 1] == 1, p_
            if float(z64.abs().max()) == 0.0:
                assert not bool(z.any()) and float(got["thr"][p_]) == 0.0
            else:
                assert float((z - z64).abs().max() / z64.abs().max()) <= 1e-3, p_
                assert float(got["thr"][p_]) == float(np.median(got["z"][p_][pr["idx"]].numpy())), p_
            counts, c, chi2 = R_.counts_row(got["z"][p_].numpy(), float(got["thr"][p_]), tm, ev, R_.test_mask(ev, pr["idx"].numpy()))
            assert got["counts"][p_].tolist() == counts and _same(float(got["c"][p_]), c) and _same(float(got["chi2"][p_]), chi2), p_
    return case, check, [], dict(nan_ok=("chi2", "c"))      # (NaN is a documented value of both: no comparable pair, V = 0)


_register("eval", "cox-survival-A")(_cox_factory)


def _attn_factory(H, k):
    """mdl_attn_softmax and mdl_attn_rank over bags of 1 .. 1025 rows with an empty bag in the middle; k = 0 passes NULL for topk_*.
    Bounds: mdl_attn_rank equals tests/_attn_ref.py bit for bit (tests/test_attention_gpu.py::test_rank_equals_the_reference); the
    softmax within (h(n) + |s - m| + K) 2^-24 of fp64 (::test_softmax_is_accurate_to_its_addition_depth)."""
    lens = [1, 2, 63, 65, 0, 257, 1025]
    T, R_ = sum(lens), len(lens)
    cu_np = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)

    def scores():
        rng = np.random.default_rng(40 + H)
        return (rng.permutation(T * H).astype(np.float32) / np.float32(T * H) * 8 - 4).reshape(T, H)

    def case(r):
        s = r.data(scores)
        st = r.stream()
        sd, cu = r.inp("scores", (T, H), F32, None if s is None else torch.from_numpy(s)), r.inp("cu", (R_ + 1,), I64, torch.from_numpy(cu_np))
        attn, m, l_ = r.out("attn", (T, H)), r.out("m", (R_, H)), r.out("l", (R_, H))
        r.call("mdl_attn_softmax", sd, H, cu, T, R_, H, attn, m, l_, r.ws("ws_softmax", "mdl_attn_map_ws_bytes", T, R_, H), st)
        order, pct = r.out("order", (H, T), I32), r.out("pct", (T, H))
        ti, tv = (r.out("topk_idx", (R_, H, k), I32), r.out("topk_val", (R_, H, k))) if k else (None, None)
        r.call("mdl_attn_rank", sd, H, cu, T, R_, H, k, order, pct, ti, tv, r.ws("ws_rank", "mdl_attn_map_ws_bytes", T, R_, H), st)
        out = dict(attn=attn, m=m, l=l_, order=order, pct=pct)
        if k:
            out.update(topk_idx=ti, topk_val=tv)
        return out

    def check(got):
        from tests import _attn_ref
        from tests.test_attention_gpu import K, U, depth
        s = scores()
        want = _attn_ref.readout(s, cu_np, k)
        assert np.array_equal(got["order"].numpy(), want["order"]) and np.array_equal(got["pct"].numpy().view(np.int32), want["pct"].view(np.int32))
        if k:
            assert np.array_equal(got["topk_idx"].numpy(), want["topk_idx"])
            assert np.array_equal(got["topk_val"].numpy().view(np.int32), np.ascontiguousarray(want["topk_val"]).view(np.int32))
        attn, m, l_ = got["attn"].numpy(), got["m"].numpy(), got["l"].numpy()
        for b_, n in enumerate(lens):
            for h in range(H):
                if n == 0:
                    assert m[b_, h] == -np.inf and l_[b_, h] == 0
                    continue
                seg = s[cu_np[b_]:cu_np[b_ + 1], h]
                a64, mx = _attn_ref.softmax64(seg)
                gap = np.abs(seg.astype(np.float64) - float(mx))
                err = np.abs(attn[cu_np[b_]:cu_np[b_ + 1], h].astype(np.float64) - a64) / (U * a64)
                assert m[b_, h] == mx and bool((err <= depth(n) + gap + K).all()), (n, h)
                l64 = np.exp(seg.astype(np.float64) - float(mx)).sum()
                assert abs(float(l_[b_, h]) - l64) <= (depth(n) + gap.max() + K) * U * l64, (n, h)
    return case, check, [], dict(nan_ok=())


_register("eval", "attn-H4-k5")(functools.partial(_attn_factory, 4, 5))
_register("eval", "attn-H1-k0")(functools.partial(_attn_factory, 1, 0))


def _rank_factory(name, marked):
    """mdl_smooth_rank / mdl_smooth_rank_marked (four caller-created events) on the two smallest matrices of tests/_rank_ref.py and on
    a 13 x 30 one (neither size a multiple of 4).  Bounds: RANK_TOL and SIGMA_TOL of tests/_rank_ref.py as tests/test_rank_gpu.py
    applies them."""
    import ctypes
    from tests import _rank_ref as RR

    def base():
        if name in RR.CASES:
            E, rank, sig = RR.case(name)
            return np.asarray(E), rank, np.asarray(sig)
        E = RR.gauss(13, 30, 99)
        rank, sig = RR.oracle(E)
        return np.asarray(E), rank, np.asarray(sig)
    n, d = {"two_rows_2x512": (2, 512), "gauss_37x512": (37, 512), "gauss_13x30": (13, 30)}[name]
    kk = min(n, d)

    def case(r):
        b = r.data(base)
        st = r.stream()
        E = r.inp("E", (n, d), F32, None if b is None else torch.from_numpy(b[0].copy()))
        sigma, out = r.out("sigma", (kk,), F64), r.out("out", (2,), F64)
        ws = r.ws("ws", "mdl_smooth_rank_ws_bytes", n, d)
        from madeleine_amd import functional as MF
        bits = MF._f64_bits(RR.EPS)
        if marked:
            marks = None
            if not r.planning:
                events = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                for ev in events:
                    ev.record()          # (creates the handle)
                marks = (ctypes.c_void_p * 4)(*[ev.cuda_event for ev in events])
            r.call("mdl_smooth_rank_marked", E, d, n, d, bits, sigma, out, ws, marks, st)
        else:
            r.call("mdl_smooth_rank", E, d, n, d, bits, sigma, out, ws, st)
        return dict(sigma=sigma, out=out)

    def check(got):
        _, rank, sig = base()
        assert abs(float(got["out"][0]) - rank) <= RR.RANK_TOL[RR.FULL] * rank
        s2 = got["sigma"].numpy() ** 2
        assert np.abs(s2 - sig ** 2).max() <= RR.SIGMA_TOL * sig.max() ** 2
    return case, check, [], {}


_register("eval", "smooth_rank-2x512")(functools.partial(_rank_factory, "two_rows_2x512", False))
_register("eval", "smooth_rank-13x30")(functools.partial(_rank_factory, "gauss_13x30", False))
_register("eval", "smooth_rank_marked-37x512")(functools.partial(_rank_factory, "gauss_37x512", True))


def _retrieval_factory(n, m, d):
    """mdl_retrieval on integer data (dot metric: every similarity exact in fp32, ties everywhere): paired with k = 5 and col_chunks = 2,
    paired with k = 0 (topk_* NULL), unpaired with k = 5 (greater / equal / pair_sim NULL), exclude_diag on a square gallery.
    Bound: bit for bit tests/_retrieval_ref.py::exact, as tests/test_retrieval_gpu.py::test_exact_on_integer_data."""
    from tests import _retrieval_ref as RR
    DOT = 1

    def data():
        from tests.test_retrieval_gpu import integer_case
        return integer_case(n, m, d)

    modes = [("paired_k5_c2", 1, 0, 5, 2), ("paired_k0", 1, 0, 0, 0), ("unpaired_k5", 0, 0, 5, 3), ("exclude_diag_k5", 0, 1, 5, 0)]

    def case(r):
        b = r.data(data)
        st = r.stream()
        Q = r.inp("Q", (n, d), F32, None if b is None else torch.from_numpy(b[0]))
        K_ = r.inp("K", (m, d), F32, None if b is None else torch.from_numpy(b[1]))
        out = {}
        for tag, paired, excl, k, chunks in modes:
            Kd, mm = (K_, m) if not excl else (Q, n)
            g, e, ps = (r.out(tag + ".greater", (n,), I32), r.out(tag + ".equal", (n,), I32), r.out(tag + ".pair_sim", (n,))) if paired else (None,) * 3
            ti, tv = (r.out(tag + ".topk_idx", (n, k), I32), r.out(tag + ".topk_val", (n, k))) if k else (None, None)
            r.call("mdl_retrieval", Q, d, Kd, d, n, mm, d, DOT, paired, excl, k, chunks, g, e, ps, ti, tv,
                   r.ws(tag + ".ws", "mdl_retrieval_ws_bytes", n, mm, d, k, chunks), st)
            for nm, x in (("greater", g), ("equal", e), ("pair_sim", ps), ("topk_idx", ti), ("topk_val", tv)):
                if x is not None:
                    out[tag + "." + nm] = x
        return out

    def check(got):
        from tests.test_retrieval_gpu import same_bits
        Qn, Kn, S = data()
        for tag, paired, excl, k, _ in modes:
            S_ = (Qn.astype(np.int64) @ Qn.astype(np.int64).T).astype(np.float32) if excl else S
            want = RR.exact(S_, bool(paired), bool(excl), k)
            have = tuple(got[tag + "." + nm].numpy() if (tag + "." + nm) in got else None for nm in ("greater", "equal", "pair_sim", "topk_idx", "topk_val"))
            same_bits(have, want)
    return case, check, [], {}


_register("eval", "retrieval-33x40-d7")(functools.partial(_retrieval_factory, 33, 40, 7))
_register("eval", "retrieval-129x257-d9")(functools.partial(_retrieval_factory, 129, 257, 9))


@pytest.mark.parametrize("cid", _ids("eval"))
def test_evaluation(dev, cid):
    _go(dev, "eval", cid)


# ========================================================================================================================= slide store
STORE_LENS = [5, 70, 130, 1]          # two bags shorter than n_tokens = 64, two longer
STORE_BAG = [0, 1, -1, 2, 3]          # an absent stain in the middle
STORE_TDEV = 75                       # tiered: bags 0 and 1 in the device tier, 2 and 3 in pinned host memory


def _store_factory(D, dtype):
    """mdl_bag_sample, mdl_bag_pack, mdl_bag_mean and their _tiered forms on one store (fp32 / bf16, D = 36 and 512: 16-byte and
    element-wise accesses).  Device buffers are arena buffers: the resident store is exactly T x D elements, the device tier exactly
    T_dev x D; the host tier is a pinned tensor of exactly its rows between two 4-KiB guards of the fill byte, checked after the run.
    Bounds: gathers exact (tests/test_store_gpu.py::_check_gather, ::_check_draw; tests/test_store_pack_gpu.py::_check_pack), the tiered
    forms bit-equal to the resident ones (tests/test_store_tiered_gpu.py), the mean within 2 h(len) 2^-24 mean |x| per column
    (tests/test_store_embed_gpu.py::test_mean_is_accurate_to_its_addition_depth)."""
    N, R_, T = 64, len(STORE_BAG), sum(STORE_LENS)
    code = {F32: 0, torch.float16: 1, BF: 2}[dtype]
    out_lens = [2 if g < 0 else min(STORE_LENS[g], N) for g in STORE_BAG]
    T_out = sum(out_lens)
    HG = 4096

    def data():
        from tests.test_store_embed_gpu import _rows
        rows = _rows(T, D, D).to(dtype)
        off = torch.zeros(len(STORE_LENS) + 1, dtype=I64)
        off[1:] = torch.cumsum(torch.tensor(STORE_LENS), 0)
        L = torch.tensor(out_lens, dtype=I64)
        cu, ch = torch.zeros(R_ + 1, dtype=I64), torch.zeros(R_ + 1, dtype=I64)
        cu[1:], ch[1:] = torch.cumsum(L, 0), torch.cumsum((L + 63) // 64, 0)
        nrows = torch.tensor([0 if g < 0 else STORE_LENS[g] for g in STORE_BAG], dtype=I64)
        mch = torch.zeros(R_ + 1, dtype=I64)
        mch[1:] = torch.cumsum((nrows + 1023) // 1024, 0)
        return dict(rows=rows, off=off, bag=torch.tensor(STORE_BAG, dtype=I32), key=torch.arange(100, 100 + R_, dtype=I64), cu=cu, ch=ch, mch=mch)

    n_chunks = sum((L + 63) // 64 for L in out_lens)
    m_chunks = sum(0 if g < 0 else (STORE_LENS[g] + 1023) // 1024 for g in STORE_BAG)

    def case(r):
        d_ = r.data(data) or {}
        st = r.stream()
        rows = d_.get("rows")
        store = r.inp("store", (T, D), dtype, rows)
        tier = r.inp("device_tier", (STORE_TDEV, D), dtype, None if rows is None else rows[:STORE_TDEV])
        off, bag, key = r.inp("off", (len(STORE_LENS) + 1,), I64, d_.get("off")), r.inp("bag", (R_,), I32, d_.get("bag")), r.inp("key_id", (R_,), I64, d_.get("key"))
        cu, ch, mch = r.inp("cu", (R_ + 1,), I64, d_.get("cu")), r.inp("chunk_cu", (R_ + 1,), I64, d_.get("ch")), r.inp("mean_chunk_cu", (R_ + 1,), I64, d_.get("mch"))
        host = hbuf = None
        if not r.planning:
            nb = (T - STORE_TDEV) * D * rows.element_size()
            hbuf = torch.full((HG + nb + HG,), r.arena.fill, dtype=U8).pin_memory()
            host = hbuf[HG:HG + nb].view(dtype).view(T - STORE_TDEV, D)
            host.copy_(rows[STORE_TDEV:])
            assert host.data_ptr() % 16 == 0
        out = {}
        for tag, tiered in (("res", False), ("tier", True)):
            src = (tier, host, code, D, T, STORE_TDEV) if tiered else (store, code, D, T)
            tail = (0,) if tiered else ()
            sfx = "_tiered" if tiered else ""
            so, si = r.out(tag + ".sample", (R_, N, D)), r.out(tag + ".sample_idx", (R_, N), I32)
            r.call("mdl_bag_sample" + sfx, *src, off, len(STORE_LENS), bag, key, R_, N, D, 7, 3, so, si, *tail, st)
            po, pb, pi = r.out(tag + ".pack", (T_out, D)), r.out(tag + ".row_bag", (T_out,), I32), r.out(tag + ".pack_idx", (T_out,), I32)
            r.call("mdl_bag_pack" + sfx, *src, off, len(STORE_LENS), bag, key, cu, ch, R_, n_chunks, T_out, D, 7, 3, po, pb, pi, *tail, st)
            mo = r.out(tag + ".mean", (R_, D))
            r.call("mdl_bag_mean" + sfx, *src, off, len(STORE_LENS), bag, mch, R_, m_chunks, D, mo, r.ws(tag + ".ws_mean", "mdl_bag_mean_ws_bytes", m_chunks, D),
                   *tail, st)
            out.update({tag + ".sample": so, tag + ".sample_idx": si, tag + ".pack": po, tag + ".row_bag": pb, tag + ".pack_idx": pi, tag + ".mean": mo})
        if not r.planning:
            torch.cuda.synchronize()
            assert bool((hbuf[:HG] == r.arena.fill).all()) and bool((hbuf[-HG:] == r.arena.fill).all()), "a write beside the host tier"
            assert torch.equal(host, rows[STORE_TDEV:]), "the host tier was written"
        return out

    def check(got):
        from tests.test_store_embed_gpu import U, depth
        from tests.test_store_gpu import _check_draw, _check_gather
        from tests.test_store_pack_gpu import _check_pack
        d_ = data()
        rows, off, bag = d_["rows"], d_["off"], d_["bag"]
        for k_ in ("sample", "sample_idx", "pack", "row_bag", "pack_idx", "mean"):
            assert torch.equal(got["tier." + k_].view(I32), got["res." + k_].view(I32)), "tiered " + k_
        _check_gather(rows, off, bag, got["res.sample"], got["res.sample_idx"])
        _check_draw(got["res.sample_idx"], STORE_LENS, bag, N)
        _check_pack(rows, off, bag, STORE_LENS, out_lens, got["res.pack"], got["res.row_bag"], got["res.pack_idx"])
        wide, offs = rows.double(), off.tolist()
        for r_, g in enumerate(STORE_BAG):
            if g < 0:
                assert not bool(got["res.mean"][r_].any())
                continue
            x = wide[offs[g]:offs[g + 1]]
            assert bool(((got["res.mean"][r_].double() - x.mean(0)).abs() <= 2.0 * depth(STORE_LENS[g], D) * U * x.abs().mean(0)).all()), g
    return case, check, [], {}


for _Dn in (36, 512):
    for _dt, _dn in ((F32, "fp32"), (BF, "bf16")):
        _register("store", "%s-D%d" % (_dn, _Dn))(functools.partial(_store_factory, _Dn, _dt))


@pytest.mark.parametrize("cid", _ids("store"))
def test_slide_store(dev, cid):
    _go(dev, "store", cid)


# =================================================================================================== the Python layer, same contract
@pytest.mark.parametrize("mode", ["split", "fp32", "bf16"])
def test_python_layer_asks_for_the_workspace_it_launches_with(dev, mode, monkeypatch):
    """Forward, backward and one AdamW step (clip and guard on) of the smallest model the ragged tests build (tests/
    test_ragged_views_gpu.py::_build, three stains at D = 64 with stain tokens; ragged bags with two absent stains, n_views = 3) under
    the global and intra InfoNCE and the local GOT -- whose token count is the number of participating cases (at most 3: far below the
    split-sweep class, see the GOT cases) -- with functional._ws replaced by an allocator that serves every workspace at exactly the
    bytes its *_ws_bytes query returned, between guards.  Every `_ws_for(query, sizes...)` sits beside a `_call(...)` whose sizes
    are written separately: here a query that asks for less than its launch uses shows as a changed guard, and a launch that reads
    beyond what it wrote as a loss, gradient or parameter that differs from the same step on stock allocations (0xFF fill: NaN)."""
    from types import SimpleNamespace

    import madeleine_amd
    from madeleine_amd import GOT, InfoNCE, calculate_losses
    from madeleine_amd import functional as MF
    from tests._arena import Arena
    from tests._util import MODS5
    from tests.test_ragged_views_gpu import _absent_batch, _build
    D, mods = 64, MODS5[:3]
    bags, labels = _absent_batch(D, long_absent=False)
    args = SimpleNamespace(global_loss="info-nce", symmetric_cl=True, local_loss_weight=0.5)

    def step():
        model = _build(mods, D, "extents", dev, stain_encoding=True).eval()
        opt = madeleine_amd.AdamW(model.parameters(), lr=1e-3, max_grad_norm=1.0)
        np.random.seed(3)
        torch.manual_seed(3)
        with torch.amp.autocast(device_type="cuda", dtype=torch.bfloat16, enabled=mode == "bf16"):
            embs, toks = model({"bags": bags, "modality_labels": labels}, dev, n_views=3)
            loss, flag = calculate_losses(mods[1:], InfoNCE(temperature=0.1), GOT, InfoNCE(temperature=0.1), embs, toks, labels[:, 1:], args)
        assert flag
        loss.backward()
        grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
        opt.step()
        torch.cuda.synchronize()
        assert opt.skipped_steps() == 0 and len(grads) >= 20
        return loss.detach().clone(), grads, {k: p.detach().clone() for k, p in model.named_parameters()}

    old = MF.gemm_mode()
    MF.set_gemm_mode("fp32" if mode == "fp32" else "split")
    try:
        want = step()
        arenas, stock = [], MF._ws

        def guarded(nbytes, device):
            if nbytes < 0:
                return stock(nbytes, device)          # (raises the query's refusal)
            n = max(int(nbytes), 16)
            a = Arena(device, 0xFF)
            a.reserve("ws%d" % len(arenas), (n,), torch.uint8, "ws", nbytes=n)
            a.allocate()
            v = a.take("ws%d" % len(arenas), (n,), torch.uint8, "ws", nbytes=n)
            a.seal()
            arenas.append(a)
            return v
        monkeypatch.setattr(MF, "_ws", guarded)
        got = step()
        monkeypatch.setattr(MF, "_ws", stock)
    finally:
        MF.set_gemm_mode(old)
    assert len(arenas) >= 10, len(arenas)
    for a in arenas:
        a.check()
    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)), (float(got[0]), float(want[0]))
    for have, ref in ((got[1], want[1]), (got[2], want[2])):
        assert set(have) == set(ref)
        for k_ in ref:
            assert torch.equal(have[k_], ref[k_]) and bool(torch.isfinite(have[k_]).all()), k_
