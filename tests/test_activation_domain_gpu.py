"""The kernels' hand-rolled activations against fp64, point by point over their whole domain (tests/_act_ref.py holds the references and
the grids): every bound below is asserted on the maximum over all grid points, never on a norm.

GELU and GELU' (csrc/preattn_act.hip) are driven through the LayerNorm-GELU-Dropout entry points with gamma = 0, beta = grid, p = 0: the
LayerNorm output is then beta[c] exactly, y[r, c] = GELU(grid[c]) in every row, and with dy = 1 in one row dbeta[c] = GELU'(grid[c]) (fp32 in
bf16 mode too).  tanh and sigmoid (csrc/common.hpp gate_tanh_pre / gate_sigmoid_pre) are driven through the gate entry points of all three
engines: sweep A feeds the argument through the bias alone (E = 0), sweep B through the accumulator and the bias with cancellation
(z = x_t + bias_j, exact on every engine), which is where the rounding of the folded bias shows.

The references are the fp64 functions, never another kernel.  The bounds are the source comments' figures at about twice the error of the
same formulas in numpy fp32 with an exact exp2 and reciprocal (the hardware's are good to 1 ulp).  Each check prints
    ACTERR <entry point> <quantity> max <error> at t = <argument>
(for a bound that varies with the argument: the error at the point that comes closest to it).

Measured on an MI355X (largest over the grids; the bound in brackets):
- erfc GELU, fp32 storage (plain, split y, grouped): absolute 3.6e-7 at t = 5.06 [8e-7, |t| <= 40]; relative 1.5e-5 at t = -11.8 [5e-5,
  2^-100 <= |t| <= 12.5] and 1.8e-6 on |t| <= 4; GELU' through dbeta 1.8e-7 [5e-7].
- polynomial GELU, bf16 storage: 0.99 of tol + half a bf16 ulp (7.85e-3 at t = 2.45: the rounding of y), tol = 8e-5 on |t| <= 4 and
  6e-5 |t| beyond; GELU' through the fp32 dbeta 2.66e-4 at t = +-4 [4e-4].
- tanh / sigmoid through the bias, fp32 and split engines: 1.9e-7 / 9.2e-8 [4e-7 / 2e-7]; dba, dbb, dwc 3.8e-7, 8.7e-8, 2.2e-7 [2e-6];
  bf16 engine: within 2e-7 of half a bf16 ulp; 3.9e-3, 1.9e-3, 3.3e-3 [6e-3].
- tanh / sigmoid with cancellation (|bias| <= 8): 4.3e-7 / 6.3e-8, 0.39 / 0.27 of 4e-7 / 2e-7 + 2^-23 (|bias| + |z|) -- above the
  bias-only figure, as the rounding of the folded bias predicts.

Three things differ from the first statement of these checks, each for a reason the runs showed:
- Half a bf16 ulp is 2^(e-8) for a value in [2^e, 2^(e+1)): between 2^-9 and 2^-8 of the value (8 significant bits), not 2^-9 of it.  A
  correctly rounded y = 2.05 is up to 7.8e-3 off, which 2^-9 |y| = 4.0e-3 does not allow.  The bf16 bounds add bf16_half_ulp() instead:
  the exact rounding error of the format, nothing wider (measured: 0.99 and 1.00 of it).
- At beta = -0 the argument is h 0 + -0, whose sign follows the row's h: the rows are compared to the bit everywhere else, and are
  zero of either sign there.
- The zero dx image of the split backward holds -0 halves; it is decoded, not compared as bytes.
The polynomial forms used to hold their value at the clamp (GELU(-1e30) = -4.1e25, GELU'(+-1e30) = 1.00024 / -0.00024): the exact
requirements at +-1e30 failed in bf16 mode until act_gelu4 / act_gelu_grad4 saturated past +-4 (csrc/preattn_act.hip).
"""
import pytest
import torch

from tests import _act_ref as R
from tests._bf16_bounds import bf16_half_ulp
from tests.test_ln_kinds_gpu import ln_bwd, ln_bwd_split, ln_fwd, ln_fwd_split, same_bits
from tests.test_split_gpu import _decode

pytestmark = pytest.mark.gpu

HID = 512
LN_KINDS = {   # kind -> (entry points, storage type, W, calls, lim, huge)
    "fp32": ("mdl_ln_gelu_drop", torch.float32, 2048, 8, 40, True),
    "bf16": ("mdl_ln_gelu_drop_bf16", torch.bfloat16, 2048, 8, 40, True),
    "split": ("mdl_ln_gelu_drop_split", torch.float32, 2048, 8, 40, False),     # the image scale is derived from max |beta|
    "groups": ("mdl_ln_gelu_drop_groups", torch.float32, 512, 4, 40, False),
    "groups_bf16": ("mdl_ln_gelu_drop_groups_bf16", torch.bfloat16, 512, 4, 40, False),
}
LN_ROWS, DY_ROW = 3, 1
ENGINES = {"fp32": "mdl_abmil_gate", "split": "mdl_abmil_gate_split", "bf16": "mdl_abmil_gate_bf16"}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def check(entry, quantity, got, ref, bound, t):
    """Prints the ACTERR line of |got - ref| and asserts it pointwise against `bound` (a number or a tensor); a NaN fails."""
    assert got.shape == ref.shape == t.shape
    err = (got.double() - ref.double()).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err).flatten()
    err, t = err.flatten(), t.double().flatten()
    ratio = torch.nan_to_num(err / bound.clamp_min(1e-300), nan=float("inf"))
    i = int(ratio.argmax())
    print("ACTERR %s %s max %.3e at t = %r (%.2f of the bound %.3e)" % (entry, quantity, float(err[i]), float(t[i]), float(ratio[i]),
                                                                       float(bound[i])))
    assert bool((err <= bound).all()), (entry, quantity, float(err[i]), float(t[i]), float(bound[i]))
    return float(err[i])


def at(values, grid, point):
    """The entries of `values` (last dimension along the grid) where the fp32 grid holds `point`."""
    sel = grid == torch.tensor(point, dtype=torch.float32)
    assert bool(sel.any()), point
    return values[..., sel]


# ------------------------------------------------------------------------------------------------------------- GELU through LayerNorm
_LN_RUNS = {}


def ln_run(dev, kind):
    """(grid [N], y [rows, N], backward outputs) of all calls of one kind, run once per module: N = calls x W."""
    if kind in _LN_RUNS:
        return _LN_RUNS[kind]
    _, dtype, W, calls, lim, huge = LN_KINDS[kind]
    if W == 2048:
        grids = [R.act_grid(W, lim, huge, k / calls) for k in range(calls)]
    else:   # one 2048-point grid over the calls: 512 columns cannot hold the ladder
        grids = list(R.act_grid(W * calls, lim, huge).view(calls, W))
    ys, backs = [], []
    for k, grid in enumerate(grids):
        gen = torch.Generator(device=dev).manual_seed(77 + k)
        x = (torch.randn(LN_ROWS, W, device=dev, generator=gen) * 3 + 0.5).to(dtype)
        dy = torch.zeros(LN_ROWS, W, device=dev, dtype=dtype)
        dy[DY_ROW] = 1.0
        grouped = kind.startswith("groups")
        bias = torch.zeros(1, W, device=dev) if grouped else 0.7 * torch.randn(W, device=dev, generator=gen)
        inp = dict(x=x, dy=dy, gamma=torch.zeros(W, device=dev), beta=grid.to(dev), bias=bias)
        cu = torch.tensor([0, LN_ROWS], dtype=torch.int64, device=dev) if grouped else None
        if kind == "split":
            st = ln_fwd_split(inp, "off", True)
            bw = ln_bwd_split(inp, st, "off")
        else:
            st = ln_fwd(inp, "off", cu)
            bw = ln_bwd(inp, st, "off", cu)
        torch.cuda.synchronize()
        ys.append(st["y"].float().cpu())
        backs.append({k2: v.float().cpu() for k2, v in bw.items()})
    out = (torch.cat(grids), torch.cat(ys, dim=1), backs)
    _LN_RUNS[kind] = out
    return out


@pytest.mark.parametrize("kind", list(LN_KINDS))
def test_gelu_forward_over_the_domain(dev, kind):
    entry, dtype, _, _, _, huge = LN_KINDS[kind]
    entry = entry.replace("drop", "drop_fwd")
    grid, y, _ = ln_run(dev, kind)
    assert bool(torch.isfinite(y).all()), "finite at every finite argument"
    # at beta = -0 the argument is h 0 + -0: +0 or -0 with the sign of the row's h, and GELU keeps the sign -- zero in every row, of either sign
    neg0 = grid.view(torch.int32) == torch.tensor(-0.0).view(torch.int32)
    assert bool((y[:, neg0] == 0).all()), "y(-0)"
    for r in range(1, LN_ROWS):
        differ = y[0].view(torch.int32) != y[r].view(torch.int32)
        assert not bool((differ & ~neg0).any()), ("rows differ: row %d at t =" % r, grid[differ & ~neg0][:8].tolist())
    ref, t = R.gelu64(grid), grid.double().abs()
    if dtype == torch.float32:
        m = t <= 40
        check(entry, "gelu_abs", y[0][m], ref[m], 8e-7, grid[m])
        m = (t >= 2.0 ** -100) & (t <= 12.5)
        check(entry, "gelu_rel_tail", y[0][m] / ref[m], torch.ones_like(ref[m]), 5e-5, grid[m])
        m = (t >= 2.0 ** -100) & (t <= 4)             # (inside the tail claim: printed for the figure the source comment quotes)
        check(entry, "gelu_rel_core", y[0][m] / ref[m], torch.ones_like(ref[m]), 5e-5, grid[m])
    else:
        tol = torch.where(t <= 4, torch.full_like(t, 8e-5), 6e-5 * t)
        check(entry, "gelu_abs", y[0], ref, tol + bf16_half_ulp(ref, tol), grid)
    if huge:
        big = torch.tensor(1e30, dtype=torch.float32).to(dtype).float()     # 1e30 as the storage type holds it
        assert bool((at(y, grid, 1e30) == big).all()), ("y(1e30)", at(y, grid, 1e30))
        assert bool((at(y, grid, -1e30) == 0).all()), ("y(-1e30)", at(y, grid, -1e30))


@pytest.mark.parametrize("kind", list(LN_KINDS))
def test_gelu_derivative_over_the_domain(dev, kind):
    from madeleine_amd.functional import SplitImage
    entry, dtype, W, _, _, huge = LN_KINDS[kind]
    entry = entry.replace("drop", "drop_bwd")
    grid, _, backs = ln_run(dev, kind)
    for bw in backs:
        for name, v in bw.items():
            if name not in ("dx_img", "dx_scale"):
                assert bool(torch.isfinite(v).all()), name
    dbeta = torch.cat([bw["dbeta"] for bw in backs])
    ref, t = R.gelu_grad64(grid), grid.double().abs()
    if dtype == torch.float32:
        check(entry, "gelu_grad_abs", dbeta, ref, 5e-7, grid)
    else:
        m = t <= 40
        check(entry, "gelu_grad_abs", dbeta[m], ref[m], 4e-4, grid[m])
    if huge:
        assert bool((at(dbeta, grid, 1e30) == 1).all()), ("dbeta(1e30)", at(dbeta, grid, 1e30))
        assert bool((at(dbeta, grid, -1e30) == 0).all()), ("dbeta(-1e30)", at(dbeta, grid, -1e30))
    if kind == "split":   # gamma = 0: the dx bound, and with it every dx, is 0
        for bw in backs:
            assert bool(torch.isfinite(bw["dx_scale"]).all())
            image = SplitImage(bw["dx_img"], bw["dx_scale"], LN_ROWS + 32, W)           # zero halves of either sign
            assert float(_decode(image, LN_ROWS + 32, W).abs().max()) == 0.0, "the dx image"
    else:
        for bw in backs:
            assert float(bw["dx"].abs().max()) == 0.0, "dx at gamma = 0"


# ------------------------------------------------------------------------------------------------------ tanh, sigmoid through the gate
def gate_forward(dev, engine, E, Wa, ba, Wb, bb):
    """act_a, act_b [T, H, 512] of the engine's forward entry point (wc = 1, bc = 0, no dropout), as fp32 on the CPU."""
    from madeleine_amd import functional as MF
    H = Wa.shape[0]
    E = E.to(dev)
    src = E.bfloat16() if engine == "bf16" else MF.split_image(E) if engine == "split" else E
    wc, bc = torch.ones(H, HID, device=dev), torch.zeros(H, device=dev)
    scores, a, b = MF.gate_fwd_raw(src, Wa.to(dev), ba.to(dev), Wb.to(dev), bb.to(dev), wc, bc, 0.0, 0, None, None, True)
    torch.cuda.synchronize()
    assert a.dtype == (torch.bfloat16 if engine == "bf16" else torch.float32)
    assert bool(torch.isfinite(scores).all())
    return a.float().cpu(), b.float().cpu()


def gate_backward(dev, engine, E, Wa, ba, Wb, bb, ds):
    """dba, dbb, dwc [H, 512] of gate_scores(...).backward(ds) at wc = 1 under the engine's GEMM mode."""
    from madeleine_amd import functional as MF
    H = Wa.shape[0]
    old = MF.gemm_mode()
    MF.set_gemm_mode("fp32" if engine == "fp32" else "split")
    try:
        Ed = E.to(dev).to(torch.bfloat16 if engine == "bf16" else torch.float32).requires_grad_()
        ps = [p.to(dev).requires_grad_() for p in (Wa, ba, Wb, bb, torch.ones(H, HID), torch.zeros(H))]
        MF.gate_scores(Ed, *ps, p_drop=0.0, seed=0).backward(ds.to(dev))
        torch.cuda.synchronize()
    finally:
        MF.set_gemm_mode(old)
    return ps[1].grad.cpu(), ps[3].grad.cpu(), ps[4].grad.cpu()


def check_ranges(a, b):
    assert not bool(torch.isnan(a).any()) and not bool(torch.isnan(b).any()), "NaN"
    assert float(a.min()) >= -1.0 and float(a.max()) <= 1.0, "tanh leaves [-1, 1]"
    assert float(b.min()) >= 0.0 and float(b.max()) <= 1.0, "sigmoid leaves [0, 1]"


def check_saturation(a, b, za, zb):
    m = za.abs() >= 20
    assert torch.equal(a[m].double(), torch.sign(za[m])), "tanh is not exactly +-1 from |z| = 20 on"
    assert bool((b[zb >= 20] == 1).all()), "sigmoid is not exactly 1 from z = 20 on"
    assert bool((b[zb <= -100] == 0).all()), "sigmoid is not exactly 0 from z = -100 down"


@pytest.mark.parametrize("engine", list(ENGINES))
def test_gate_activations_bias_sweep(dev, engine):
    H, T, bf16 = 8, 2, engine == "bf16"
    ba = R.act_grid(H * HID, 100, True, 0.0).view(H, HID)
    bb = R.act_grid(H * HID, 100, True, 0.5).flip(0).view(H, HID)
    E, W0 = torch.zeros(T, H * HID), torch.zeros(H, HID, HID)
    a, b = gate_forward(dev, engine, E, W0, ba, W0, bb)
    assert same_bits(a[0], a[1]) and same_bits(b[0], b[1]), "the two token rows differ"
    check_ranges(a, b)
    check_saturation(a[0], b[0], ba.double(), bb.double())
    ra, rb = R.tanh64(ba), R.sigmoid64(bb)
    check(ENGINES[engine] + "_fwd", "tanh_abs", a[0], ra, 4e-7 + (bf16_half_ulp(ra, 4e-7) if bf16 else 0.0), ba)
    check(ENGINES[engine] + "_fwd", "sigmoid_abs", b[0], rb, 2e-7 + (bf16_half_ulp(rb, 2e-7) if bf16 else 0.0), bb)

    ds = torch.zeros(T, H)
    ds[0] = 1.0
    grads = gate_backward(dev, engine, E, W0, ba, W0, bb, ds)
    tol = 6e-3 if bf16 else 2e-6
    for name, got, ref, arg in zip(("dba", "dbb", "dwc"), grads, R.gate_grads64(ba, bb), (ba, bb, ba)):
        assert not bool(torch.isnan(got).any()), name
        check(ENGINES[engine] + "_bwd", name + "_abs", got, ref, tol, arg)


@pytest.mark.parametrize("H", [1, 8])
@pytest.mark.parametrize("engine", list(ENGINES))
def test_gate_activations_accumulator_and_bias_sweep(dev, engine, H):
    T, bf16 = 257, engine == "bf16"
    x = -8.0 + torch.arange(T, dtype=torch.float32) / 16            # bf16-representable; hi + lo fp16 holds it exactly at the scale 2^10
    E, W1 = torch.zeros(T, H * HID), torch.zeros(H, HID, HID)
    E[:, ::HID] = x[:, None]
    W1[:, :, 0] = 1.0
    ba = torch.stack([R.grid_with(-x, HID, 8, (h + 0.37) / H) for h in range(H)])
    bb = torch.stack([R.grid_with(-x.flip(0), HID, 8, (h + 0.61) / H) for h in range(H)])
    a, b = gate_forward(dev, engine, E, W1, ba, W1, bb)
    za, zb = x.double()[:, None, None] + ba.double()[None], x.double()[:, None, None] + bb.double()[None]     # exact
    assert int((za == 0).sum()) >= T * H and int((zb == 0).sum()) >= T * H, "the exact zeros"
    check_ranges(a, b)
    ra, rb = R.tanh64(za), R.sigmoid64(zb)
    # the folded bias 2 log2e bias is rounded before the FMA and the FMA rounds once more: each half an ulp of the exponent, in z no more than
    # 2^-24 (|bias| + |z|) against a slope <= 1; doubled once for margin
    fold_a = 2.0 ** -23 * (ba.double().abs()[None] + za.abs())
    fold_b = 2.0 ** -23 * (bb.double().abs()[None] + zb.abs())
    entry = "%s_fwd[H=%d]" % (ENGINES[engine], H)
    tol_a, tol_b = 4e-7 + fold_a, 2e-7 + fold_b
    check(entry, "tanh_abs_cancelling", a, ra, tol_a + (bf16_half_ulp(ra, tol_a) if bf16 else 0.0), za)
    check(entry, "sigmoid_abs_cancelling", b, rb, tol_b + (bf16_half_ulp(rb, tol_b) if bf16 else 0.0), zb)
