"""The ways of describing the same rows to the LayerNorm-GELU-Dropout kernels agree (csrc/preattn_act.hip): a grouped call against a plain
call with the common bias row, the split forward against the plain fp32 forward, the split backward's decoded image against the plain
backward's dx -- at every width, at fewer rows than a block iteration (1), a ragged last one (7) and a grid-stride loop that takes a
second trip (8197 rows at 256 and 2048 columns: past 2048 workgroups of 4, 4 and 2 rows), with dropout off, by the counter hash and by a
keep mask (every DM).  Through the C ABI, so that every output of an entry point is looked at.

Levels (measured on the library before the records, and the same after; the figures are the largest seen over all cases):
- equal to the bit: grouped against plain y, mean, rstd, dx (the same kernel walks the same rows; only the partition differs), fp32 and
  bf16; split forward (y requested) against plain forward y, mean, rstd; image-only forward against the y-requested one: image bytes,
  scale, mean, rstd; split backward against plain backward dgamma, dbeta, dbias (the same grid, the same order of the partial sums).
- grouped against plain dgamma, dbeta and sum_g dgroup_bias[g] against dbias: the partial sums are cut at other rows, so the order of the
  additions differs -- rel_err < 1e-4 for fp32 (tests/test_hip_kernels.py::test_ln_gelu_drop_vs_torch) and < 1e-2 for bf16
  (::test_ln_gelu_drop_groups_vs_torch); measured 9.4e-8 and 9.2e-8.
- split backward image against plain dx: |decoded - dx| <= 2^-22 |dx| + 2^-25 / dx_scale[0], the image's quantum (hi = fp16(v s), lo =
  fp16(v s - hi): the error is lo's rounding, half an ulp of a value no larger than half an ulp of hi, or half the subnormal step 2^-24);
  measured 0.999 of it (the worst rounding of lo among 16.8 M elements): nothing is left for a difference between the two kernels' dx."""
import pytest
import torch

from tests._util import rel_err
from tests.test_split_gpu import _decode

pytestmark = pytest.mark.gpu

WIDTHS = (256, 512, 1024, 2048, 4096)
SHAPES = [(W, rows) for W in WIDTHS for rows in (1, 7)] + [(256, 8197), (2048, 8197)]
MODES = ("off", "hash", "mask")
SEED = 1234


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def make_inputs(dev, W, rows, dtype=torch.float32):
    """x, dy [rows, W] in `dtype`; gamma, beta, bias [W] fp32; a uint8 keep mask."""
    gen = torch.Generator(device=dev).manual_seed(1000 * W + rows)
    rnd = lambda *shape: torch.randn(*shape, device=dev, generator=gen)      # noqa: E731
    x, dy = (rnd(rows, W) * 3 + 0.5).to(dtype), rnd(rows, W).to(dtype)
    gamma, beta, bias = 1 + 0.2 * rnd(W), 0.3 * rnd(W), 0.7 * rnd(W)
    keep = (torch.rand(rows, W, device=dev, generator=gen) < 0.9).to(torch.uint8)
    return dict(x=x, dy=dy, gamma=gamma, beta=beta, bias=bias, keep=keep)


def drop_args(inp, mode):
    return (0.0 if mode == "off" else 0.1, SEED, inp["keep"] if mode == "mask" else None)


def ln_fwd(inp, mode, cu=None):
    from madeleine_amd import functional as MF
    x = inp["x"]
    rows, W = x.shape
    y, mean = torch.empty_like(x), torch.empty(rows, device=x.device)
    rstd = torch.empty_like(mean)
    groups = () if cu is None else (cu, cu.numel() - 1)
    MF._call("mdl_ln_gelu_drop_fwd" + ("_groups" if groups else "") + MF._sfx(x), x, inp["bias"], inp["gamma"], inp["beta"], y, mean, rstd, rows,
             W, 1e-5, *drop_args(inp, mode), *groups, MF._stream())
    return dict(y=y, mean=mean, rstd=rstd)


def ln_bwd(inp, st, mode, cu=None):
    from madeleine_amd import functional as MF
    x = inp["x"]
    rows, W = x.shape
    dx, dg, db, dbias = torch.empty_like(x), torch.empty_like(inp["gamma"]), torch.empty_like(inp["beta"]), torch.empty_like(inp["bias"])
    groups = () if cu is None else (cu, cu.numel() - 1)
    ws = MF._ws_for("mdl_ln_gelu_drop_bwd%s_ws_bytes" % ("_groups" if groups else ""), x.device, rows, W, *groups[1:])
    MF._call("mdl_ln_gelu_drop_bwd" + ("_groups" if groups else "") + MF._sfx(x), x, inp["bias"], inp["gamma"], inp["beta"], st["mean"],
             st["rstd"], inp["dy"], dx, dg, db, dbias, rows, W, *drop_args(inp, mode), *groups, ws, MF._stream())
    return {"dx": dx, "dgamma": dg, "dbeta": db, "dgroup_bias" if groups else "dbias": dbias}


def ln_fwd_split(inp, mode, want_y, row_mul=None, want_rstd_max=False):
    from madeleine_amd import functional as MF
    x = inp["x"]
    rows, W = x.shape
    y = torch.empty_like(x) if want_y else None
    img, scale, mean = torch.empty_like(x), torch.empty(2, device=x.device), torch.empty(rows, device=x.device)
    rstd = torch.empty_like(mean)
    rstd_max = torch.empty(1, device=x.device) if want_rstd_max else None
    MF._call("mdl_ln_gelu_drop_fwd_split", x, inp["bias"], inp["gamma"], inp["beta"], y, img, scale, mean, rstd, rows, W, 1e-5,
             *drop_args(inp, mode), row_mul, rstd_max, MF._stream())
    out = dict(img=img, scale=scale, mean=mean, rstd=rstd)
    if want_y:
        out["y"] = y
    if want_rstd_max:
        out["rstd_max"] = rstd_max
    return out


def ln_bwd_split(inp, st, mode, dy_absmax=None, row_mul=None, rstd_max=None, cu=None, bias=None):
    """bias: the common row when inp["bias"] is the grouped one (the split-grouped entry takes x with the group rows already added)."""
    from madeleine_amd import functional as MF
    x = inp["x"]
    rows, W = x.shape
    bias = inp["bias"] if bias is None else bias
    dximg, dxscale = torch.empty(rows + 32, W, device=x.device), torch.empty(2, device=x.device)
    dg, db, dbias = torch.empty_like(inp["gamma"]), torch.empty_like(inp["beta"]), torch.empty_like(bias)
    out = dict(dx_img=dximg, dx_scale=dxscale, dgamma=dg, dbeta=db, dbias=dbias)
    groups = ()
    if cu is not None:
        out["dgroup_bias"] = torch.empty(cu.numel() - 1, W, device=x.device)
        groups = (cu, cu.numel() - 1, out["dgroup_bias"])
    ws = MF._ws_for("mdl_ln_gelu_drop_bwd%s_ws_bytes" % ("_groups" if groups else ""), x.device, rows, W, *groups[1:2])
    MF._call("mdl_ln_gelu_drop_bwd_split" + ("_groups" if groups else ""), x, bias, inp["gamma"], inp["beta"], st["mean"], st["rstd"], inp["dy"],
             dy_absmax, dximg, dxscale, dg, db, dbias, rows, W, *drop_args(inp, mode), row_mul, rstd_max, *groups, ws, MF._stream())
    return out


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("W", [256, 512, 1024])
def test_grouped_call_equals_plain_call_with_the_bias(dev, W, dtype):
    cu = torch.tensor([0, 5, 5, 19], dtype=torch.int64, device=dev)          # an empty group
    tol = 1e-4 if dtype == torch.float32 else 1e-2
    plain = make_inputs(dev, W, 19, dtype)
    grouped = dict(plain, bias=plain["bias"].repeat(3, 1))
    for mode in MODES:
        fp, fg = ln_fwd(plain, mode), ln_fwd(grouped, mode, cu)
        bp, bg = ln_bwd(plain, fp, mode), ln_bwd(grouped, fg, mode, cu)
        for k in ("y", "mean", "rstd"):
            assert same_bits(fp[k], fg[k]), (mode, k)
        assert same_bits(bp["dx"], bg["dx"]), mode
        errs = [rel_err(bg["dgamma"], bp["dgamma"]), rel_err(bg["dbeta"], bp["dbeta"]), rel_err(bg["dgroup_bias"].sum(0), bp["dbias"])]
        print("grouped vs plain W=%d %s %s: dgamma %.2e dbeta %.2e dbias %.2e" % (W, dtype, mode, *errs))
        assert max(errs) < tol, (mode, errs)
        assert float(bg["dgroup_bias"][1].abs().max()) == 0.0, "the empty group"


@pytest.mark.parametrize("W,rows", SHAPES)
def test_split_forward_equals_plain_forward(dev, W, rows):
    inp = make_inputs(dev, W, rows)
    for mode in MODES:
        plain, both, image = ln_fwd(inp, mode), ln_fwd_split(inp, mode, True), ln_fwd_split(inp, mode, False)
        for k in ("y", "mean", "rstd"):
            assert same_bits(plain[k], both[k]), (mode, k, "y requested")
        for k in ("img", "scale", "mean", "rstd"):
            assert same_bits(both[k], image[k]), (mode, k, "image only")


@pytest.mark.parametrize("W,rows", SHAPES)
def test_split_backward_equals_plain_backward(dev, W, rows):
    from madeleine_amd import functional as MF
    inp = make_inputs(dev, W, rows)
    for mode in MODES:
        st = ln_fwd(inp, mode)
        plain, split = ln_bwd(inp, st, mode), ln_bwd_split(inp, st, mode)
        for k in ("dgamma", "dbeta", "dbias"):
            assert same_bits(plain[k], split[k]), (mode, k)
        dec = _decode(MF.SplitImage(split["dx_img"], split["dx_scale"], rows, W), rows, W)
        dx = plain["dx"].double()
        quantum = 2.0 ** -22 * dx.abs() + 2.0 ** -25 / float(split["dx_scale"][0])
        worst = float(((dec - dx).abs() / quantum).max())
        print("split vs plain backward W=%d rows=%d %s: |decoded - dx| / quantum = %.3f" % (W, rows, mode, worst))
        assert worst <= 1.0, mode
        assert float(split["dx_img"][rows:].abs().max()) == 0.0, "the 32 zero rows"
