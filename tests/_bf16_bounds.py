"""fp64 references and per-element error bounds of the bf16 engine (csrc/linear_bf16.hip, csrc/abmil_gate_bf16.hip,
csrc/tile_engine_bf16.hpp and the bf16 instantiations of csrc/abmil_pool.hip, csrc/preattn_act.hip), for
tests/test_bf16_elements_gpu.py (the kernels) and tests/test_bf16_bounds_cpu.py (these checkers, against a CPU emulation and seeded faults).

The contract.  Every operand of a case is bf16-representable: drawn in fp32, rounded with .to(bfloat16), and handed to both sides.  The
reference is fp64 of the documented operation, never another kernel.  Where the engine rounds (read from the sources):
  - weights are rounded to bf16 by the weight-image kernels (linb_w_cast_kernel, linb_w_transpose_kernel, gate_wk / gate_wn_bf16_kernel):
    exact here, the weights of a case being bf16-representable;
  - the gate forward rounds tanh / sigmoid to bf16 BEFORE forming the scores, (float)(bf16_t)gate_tanh_pre(...): the scores are a
    function of the stored act_a / act_b;
  - dz is a bf16 intermediate of the gate backward (gate_dz_kernel<bf16_t, bf16_t>): dE, dWa, dWb contract bf16(dz), while dba, dbb, dwc,
    dbc sum the fp32 values before that rounding;
  - Y, dX, dE and the LayerNorm y / dx are rounded once, on store;
  - every sum is fp32.
Where an entry point takes an earlier kernel's output as an argument (act_a / act_b, mean / rstd, pooled / stat_m / stat_l), the reference
of that entry point takes the values the kernel stored as exact inputs: a rounding flip upstream is not charged twice.

The bounds, per element, in fp64 beside the reference:
  - an fp32 sum of n exact products (bf16 x bf16 is exact in fp32): SUM_TOL * mag, mag the same expression on absolute values, and, as a
    second assertion, the proven gamma(n) * mag.  Terms that are themselves rounded (a product with an fp32 factor) add
    term_roundings * 2^-24 * mag to both.  A contraction over token rows that the row_scaled inputs scale by 2^[-12, 12] is held to the
    proven ceiling alone (sum_bounds: SUM_TOL is the accuracy of sums of comparable addends);
  - a bf16 output of such a sum: bf16_half_ulp(ref, slack) + slack, slack being the fp32 bound;
  - outputs through dz: the rounding of dz, bf16_half_ulp(dz) + DZ_ROUNDINGS * 2^-24 |dz|, carried through the product on absolute values;
  - softmax-bearing outputs: SOFTMAX_FACTOR times SOFTMAX_RATIO, the worst |error| / (2^-24 mag) of a plain torch fp32 CPU evaluation of
    the same formula over the tests' own inputs (measure_ratio): the exp constant is measured, not derived.
Constants: which are derived, taken from other tests or measured is said beside each."""
import math

import torch

BF = torch.bfloat16
F64 = torch.float64
U24 = 2.0 ** -24
HID = 512

# taken from tests/test_dispatch_edges_gpu.py::_chain_check: the split engine meets it at T up to 258 055, and a blocked fp32 accumulation of
# exact products has no more roundings than that engine
SUM_TOL = 4e-7
# taken from tests/test_activation_domain_gpu.py (the bounds it asserts over the whole domain)
TANH_TOL, SIGMOID_TOL = 4e-7, 2e-7
GELU_TOL_CORE, GELU_TOL_TAIL, GELU_GRAD_TOL = 8e-5, 6e-5, 4e-4        # polynomial GELU of the bf16 mode: 8e-5 on |t| <= 4, 6e-5 |t| beyond
# derived (csrc/gate_common.hpp gate_dz_t): dza = ((ds wc) (b kb) ka) (1 - a a) -- 1/(1-p) represented (2: the subtraction, the division),
# used twice, g, bd, two products, 1 - a a (exact for |a| >= 2^-5, one rounding below), the last product: 10; 12 with margin
DZ_ROUNDINGS = 12
# derived: |GELU''| <= 1.13 and |tanh'| <= 1, |sigmoid'| <= 1/4 carry an argument's error into the function value
GELU_SLOPE, GELU_GRAD_SLOPE = 1.13, 1.13
# measured: the worst |error| / (2^-24 mag) of a plain torch fp32 CPU evaluation of the same formula against fp64 (measure_ratio), over
# every case of test_pool_bags, test_pool_views and test_gate_fused_pooling_term of tests/test_bf16_elements_gpu.py, the backward ones on
# the forward results the kernels stored.  Per case the figure runs from 0.5 up to the values here (the worst case of each output is
# named); a single case's own figure is too small a sample to bound another evaluation order (a 33-token view measured 0.54 where the
# kernel, correct by reading, is at 2.3), so the bound uses the worst over the family.
SOFTMAX_RATIO = {
    "stat_l": 2.69,        # sum_t exp(s_t - m), mag = the sum itself                           (view, H = 4, cancelling)
    "pooled": 6.13,        # sum_t w_t E_t, mag = sum_t w_t |E_t|                                (view, H = 4, row_scaled)
    "w d_pooled": 3.19,    # exp(s - m) / l * d_pooled, mag = its absolute value                 (ragged bags, H = 4, uniform)
    "d_scores": 0.96,      # w (<E, dp> - <pooled, dp>), mag = w (sum |E dp| + sum |pooled dp|)  (ragged bags, H = 4, uniform)
    "pool term": 3.65,     # the same weight inside the fused gate backward                      (two ragged bags, H = 4)
}
# the margin on the measured figure: the kernel sums in another order and uses the hardware exp2; a tail or a dropped token misses by orders
# of magnitude (one of n <= 333 tokens is mag / n against an allowance of at most 4 x 6.13 x 2^-24 mag = 1.5e-6 mag)
SOFTMAX_FACTOR = 4.0


def bf16_half_ulp(ref, slack=0.0):
    """Half the bf16 spacing at |ref| + slack, the most that storing a value within `slack` of ref in bf16 adds to its error: 2^(e - 8) in
    [2^e, 2^(e+1)): between 2^-9 and 2^-8 of the value (8 significant bits)."""
    mag = (ref.double().abs() + slack).clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(mag)) - 8)


def gamma(n):
    """The ceiling of the relative error of any fp32 summation of n addends, in units of the sum of their absolute values."""
    n = max(int(n), 1)
    return n * U24 / (1.0 - n * U24)


def rb(x):
    """x rounded to bf16 (round to nearest even), as fp32."""
    return x.to(BF).float()


def truncate_bf16(x):
    """x cut to bf16 (round toward zero), as fp32: the fault a store without rounding makes."""
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


def rel_err(a, b):
    """The norm criterion the suite had: |a - b| / |b|."""
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


# --------------------------------------------------------------------------------------------------------------------------- the checkers
def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the elements (inf for a NaN or an error above a zero bound), and the flat index where."""
    err = (got.double().cpu() - ref.double().cpu()).abs().flatten()
    bound = torch.as_tensor(bound, dtype=F64).cpu().expand(ref.shape).flatten()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    ratio = torch.nan_to_num(ratio, nan=float("inf"))
    if ratio.numel() == 0:
        return 0.0, 0
    i = int(ratio.argmax())
    return float(ratio[i]), i


def check(what, got, ref, bound, second=None):
    """Asserts |got - ref| <= bound at every element (and <= second, where given); prints BF16ERR <what> <worst ratio>."""
    assert tuple(got.shape) == tuple(ref.shape), (what, tuple(got.shape), tuple(ref.shape))
    r, i = worst_ratio(got, ref, bound)
    print("BF16ERR %s worst |err| / bound = %.3f at flat index %d of %s" % (what, r, i, tuple(ref.shape)))
    assert r <= 1.0, (what, r, i)
    if second is not None:
        r2, i2 = worst_ratio(got, ref, second)
        assert r2 <= 1.0, (what + " (gamma_n ceiling)", r2, i2)
    return r


def passes(got, ref, bound, second=None):
    """check() as a predicate, for the seeded faults."""
    ok = worst_ratio(got, ref, bound)[0] <= 1.0
    return ok and (second is None or worst_ratio(got, ref, second)[0] <= 1.0)


def check_exact(what, got, ref):
    """Bit for bit: the integer cases."""
    got, ref = got.double().cpu(), ref.double().cpu()
    assert tuple(got.shape) == tuple(ref.shape), what
    bad = got != ref
    assert not bool(bad.any()), (what, int(bad.sum()), bad.nonzero()[:4].tolist())


def sum_bounds(mag, n, term_roundings=0, extra=0.0, scaled=False):
    """(working bound, proven ceiling) of an fp32 sum of n addends of total absolute value mag; extra: an error of the addends themselves.
    scaled: the addends are token rows scaled by 2^[-12, 12] (a row_scaled contraction over tokens).  The few largest addends then set mag
    and every later rounding happens at their scale: a walk of n roundings reaches several sqrt(n) 2^-24 mag (13 units at T = 300 in the
    CPU emulation, against the 6.7 of SUM_TOL), whatever the order.  SUM_TOL states the accuracy of sums of comparable addends and does
    not apply; the bound is then the proven ceiling alone."""
    mag = mag.double()
    proven = (gamma(n) + term_roundings * U24) * mag + extra
    return (proven if scaled else (SUM_TOL + term_roundings * U24) * mag + extra), proven


def stored(ref, slack):
    """The bound of a value within `slack` of ref (fp32) stored as bf16."""
    return bf16_half_ulp(ref, slack) + slack


def measure_ratio(emulated, ref, mag):
    """Worst |emulated - ref| / (2^-24 mag): the error of a plain fp32 evaluation of a softmax-bearing formula, in units of 2^-24 mag."""
    err = (emulated.double() - ref.double()).abs()
    m = mag.double() > 0
    if not bool(m.any()):
        return 0.0
    return float((err[m] / (U24 * mag.double()[m])).max())


def softmax_bound(key, mag, emulated=None, ref=None, what=""):
    """SOFTMAX_FACTOR x the measured ratio SOFTMAX_RATIO[key] x 2^-24 mag.  With a torch fp32 evaluation and the fp64 reference of the
    case, prints the case's own figure beside the constant (the measurement the constant was taken from)."""
    if emulated is not None:
        print("BF16ERR %s%s torch fp32 ratio of this case %.2f (constant %.2f, x %g allowed)"
              % (what, key, measure_ratio(emulated, ref, mag), SOFTMAX_RATIO[key], SOFTMAX_FACTOR))
    return SOFTMAX_FACTOR * SOFTMAX_RATIO[key] * U24 * mag.double()


# ------------------------------------------------------------------------------------------------------------------------------- inputs
KINDS = ("uniform", "row_scaled", "cancelling")


def uniform(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return rb((torch.rand(shape, generator=g, dtype=torch.float32) * 2 - 1) * scale)


def signs(shape, seed):
    """+-1, no zeros."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()


def small_ints(shape, seed, top=3):
    """Integers of [-top, top] without zero."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(1, top + 1, shape, generator=g).float()
    return v * signs(shape, seed + 7919)


def row_scales(rows, seed):
    """2^e per row, e an integer of [-12, 12]: an exact scaling of bf16 values."""
    g = torch.Generator().manual_seed(seed)
    return torch.exp2(torch.randint(-12, 13, (rows,), generator=g).float())[:, None]


def mirror(x, dim, sign, lo=0, hi=None):
    """The second half of x[lo:hi] along `dim` = sign * the first half (an odd length leaves its last entry alone)."""
    hi = x.shape[dim] if hi is None else hi
    h = (hi - lo) // 2
    if h:
        x.narrow(dim, lo + h, h).copy_(sign * x.narrow(dim, lo, h))
    return x


def token_operand(shape, seed, kind, scale=1.0):
    """A token-side operand (x, dY, E, d_pooled) of the given input kind; the cancelling structure is put on by the case."""
    x = uniform(shape, seed, scale)
    if kind == "row_scaled":
        x = x * row_scales(shape[0], seed + 104729)
    return x


# ------------------------------------------------------------------------------------------------------------------------------ Linear
def linear_case(T, N, K, seed, kind):
    """x [T, K], W [N, K], bias [N], dy [T, N]: `kind` in KINDS or 'exact' (+-1 operands and weights, integer bias)."""
    if kind == "exact":
        return dict(x=signs((T, K), seed), W=signs((N, K), seed + 1), b=small_ints((N,), seed + 2), dy=signs((T, N), seed + 3), kind=kind)
    x, dy = token_operand((T, K), seed, kind), token_operand((T, N), seed + 3, kind)
    W, b = uniform((N, K), seed + 1, K ** -0.5), uniform((N,), seed + 2, 0.1)
    if kind == "cancelling":
        # Y: the columns of x negate, those of W repeat; dX: the columns of dy negate, the rows of W repeat; dW, dbias: the rows of dy
        # negate, those of x repeat
        mirror(mirror(x, 1, -1), 0, +1)
        mirror(mirror(W, 1, +1), 0, +1)
        mirror(mirror(dy, 1, -1), 0, -1)
    return dict(x=x, W=W, b=b, dy=dy, kind=kind)


def linear_ref(case, device="cpu"):
    """name -> (fp64 reference, mag, number of addends) of Y, dX, dW, dbias."""
    x, W, b, dy = (case[k].to(device).double() for k in ("x", "W", "b", "dy"))
    T, K = x.shape
    N = W.shape[0]
    out = {"Y": (x @ W.t() + b, x.abs() @ W.abs().t() + b.abs(), K + 1),
           "dX": (dy @ W, dy.abs() @ W.abs(), N),
           "dW": (dy.t() @ x, dy.abs().t() @ x.abs(), T),
           "db": (dy.sum(0), dy.abs().sum(0), T)}
    return {k: (r.cpu(), m.cpu(), n) for k, (r, m, n) in out.items()}


def linear_bounds(ref, kind="uniform"):
    """name -> (bound, second assertion); dW and dbias contract over the token rows, which `kind` = 'row_scaled' scales."""
    out = {}
    for k, (r, mag, n) in ref.items():
        b1, b2 = sum_bounds(mag, n, scaled=kind == "row_scaled" and k in ("dW", "db"))
        out[k] = (stored(r, b1), stored(r, b2)) if k in ("Y", "dX") else (b1, b2)
    return out


def check_linear(got, ref, kind, what=""):
    if kind == "exact":
        assert float(ref["Y"][0].abs().max()) <= 256 and float(ref["dX"][0].abs().max()) <= 256, "the exact case leaves the integers bf16 holds"
        for k in got:
            check_exact(what + k, got[k], ref[k][0])
        return
    bounds = linear_bounds(ref, kind)
    for k in got:
        check(what + k, got[k], ref[k][0], *bounds[k])


def emulate_linear(case):
    """The contract on the CPU: fp32 products, bf16 on the store of Y and dX."""
    x, W, b, dy = case["x"], case["W"], case["b"], case["dy"]
    return {"Y": rb(x @ W.t() + b), "dX": rb(dy @ W), "dW": dy.t() @ x, "db": dy.sum(0)}


# ------------------------------------------------------------------------------------------------------------------------------ pooling
def bag_rows(lens):
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + int(n))
    return cu


def pool_case(lens, H, seed, kind, segments=None):
    """E [T, H*512], scores [T, H] (also the weights of the weighted pooling), d_pooled [segments, H*512], starting contents dE0, ds0.
    segments: a list of index tensors (rows of E) per pooled row -- whole bags by default, the views of a view call otherwise.
    'exact': +-1 E and d_pooled, small-integer weights and starting contents."""
    cu = bag_rows(lens)
    T, C = cu[-1], H * HID
    if segments is None:
        segments = [torch.arange(cu[b], cu[b + 1]) for b in range(len(lens))]
    S = len(segments)
    if kind == "exact":
        return dict(E=signs((T, C), seed), s=small_ints((T, H), seed + 1), dp=signs((S, C), seed + 2), dE0=small_ints((T, C), seed + 3),
                    ds0=small_ints((T, H), seed + 4), segments=segments, lens=list(lens), H=H, kind=kind)
    E, dp = token_operand((T, C), seed, kind), token_operand((S, C), seed + 2, kind)
    s = uniform((T, H), seed + 1, 4.0)
    if kind == "cancelling":
        mirror(dp, 1, -1)                           # d_scores: <E, d_pooled> over the channels
        for rows in segments:                       # pooled: the second half of a segment's tokens negates the first at equal scores
            h = rows.numel() // 2
            if h:
                E[rows[h:2 * h]] = -E[rows[:h]]
                s[rows[h:2 * h]] = s[rows[:h]]
        mirror(E, 1, +1)
    dE0 = token_operand((T, C), seed + 3, "uniform")
    ds0 = uniform((T, H), seed + 4)
    return dict(E=E, s=s, dp=dp, dE0=dE0, ds0=ds0, segments=segments, lens=list(lens), H=H, kind=kind)


def _softmax_parts(s, dt):
    """p = exp(s - max), its sum: the formula of the kernels (csrc/abmil_pool.hip), in dtype dt."""
    s = s.to(dt)
    m = s.max(0).values
    p = torch.exp(s - m)
    return m, p, p.sum(0)


def pool_fwd_ref(case, lin, dt=F64):
    """pooled [S, H*512], stat_m, stat_l [S, H] of the softmax pooling (lin: of the weighted pooling) in dtype dt, with mag of pooled."""
    E, s, H = case["E"].to(dt), case["s"], case["H"]
    S, C = len(case["segments"]), H * HID
    pooled, mag = torch.zeros(S, C, dtype=dt), torch.zeros(S, C, dtype=dt)
    m_, l_ = torch.zeros(S, H, dtype=dt), torch.ones(S, H, dtype=dt)
    for k, rows in enumerate(case["segments"]):
        if rows.numel() == 0:
            continue
        if lin:
            w = s[rows].to(dt)
        else:
            m_[k], p, l_[k] = _softmax_parts(s[rows], dt)
            w = p / l_[k]
        Er = E[rows].view(-1, H, HID)
        pooled[k] = (w[:, :, None] * Er).sum(0).reshape(C)
        mag[k] = (w.abs()[:, :, None] * Er.abs()).sum(0).reshape(C)
    return dict(pooled=pooled, m=m_, l=l_, mag=mag)


def pool_bwd_ref(case, lin, pooled, m, l_, acc, acc_s, dt=F64):
    """dE [T, H*512] and d_scores [T, H] in dtype dt from the STORED forward results (pooled, stat_m, stat_l: exact inputs), with the
    magnitudes: rows outside every segment keep their starting contents (acc) or are not looked at (mask)."""
    E, s, dp, H = case["E"].to(dt), case["s"].to(dt), case["dp"].to(dt), case["H"]
    T, C = E.shape
    dE = case["dE0"].to(dt).clone() if acc else torch.zeros(T, C, dtype=dt)
    ds = case["ds0"].to(dt).clone() if acc_s else torch.zeros(T, H, dtype=dt)
    wdp, ds_mag = torch.zeros(T, C, dtype=dt), torch.zeros(T, H, dtype=dt)      # the term w d_pooled alone; the magnitude of d_scores
    mask = torch.zeros(T, dtype=torch.bool)
    pooled, m, l_ = pooled.to(dt), m.to(dt), l_.to(dt)
    for k, rows in enumerate(case["segments"]):
        if rows.numel() == 0:
            continue
        mask[rows] = True
        Er, dpk = E[rows].view(-1, H, HID), dp[k].view(1, H, HID)
        dw = (Er * dpk).sum(2)
        dw_mag = (Er.abs() * dpk.abs()).sum(2)
        if lin:
            w, d_s, d_mag = s[rows], dw, dw_mag
        else:
            w = torch.exp(s[rows] - m[k]) * (1.0 / l_[k])
            D = (pooled[k].view(H, HID) * dpk[0]).sum(1)
            d_s, d_mag = w * (dw - D), w * (dw_mag + (pooled[k].view(H, HID).abs() * dpk[0].abs()).sum(1))
        term = (w[:, :, None] * dpk).reshape(-1, C)
        dE[rows] += term
        wdp[rows] = term
        ds[rows] += d_s
        ds_mag[rows] = d_mag
    return dict(dE=dE, ds=ds, wdp=wdp, ds_mag=ds_mag, mask=mask)


def check_pool_fwd(got, case, lin, what=""):
    """pooled, stat_m, stat_l of a forward against fp64; the softmax bound is measured on the case's own inputs."""
    ref = pool_fwd_ref(case, lin)
    if case["kind"] == "exact":
        assert lin
        check_exact(what + "pooled", got["pooled"], ref["pooled"])
        return
    if lin:
        n = max([r.numel() for r in case["segments"]] + [1])
        check(what + "pooled", got["pooled"], ref["pooled"], *sum_bounds(ref["mag"], n, scaled=case["kind"] == "row_scaled"))
        return
    emu = pool_fwd_ref(case, lin, torch.float32)
    check_exact(what + "stat_m", got["m"], ref["m"])
    check(what + "stat_l", got["l"], ref["l"], softmax_bound("stat_l", ref["l"], emu["l"], ref["l"], what))
    check(what + "pooled", got["pooled"], ref["pooled"], softmax_bound("pooled", ref["mag"], emu["pooled"], ref["pooled"], what))


def check_pool_bwd(got, case, lin, fwd, acc, acc_s, what=""):
    """dE (bf16) and d_scores of a backward against fp64 of the stored forward results `fwd` (pooled, m, l as the kernel wrote them)."""
    args = (case, lin, fwd["pooled"].cpu(), fwd["m"].cpu(), fwd["l"].cpu(), acc, acc_s)
    ref = pool_bwd_ref(*args)
    rows = ref["mask"] if not acc else torch.ones_like(ref["mask"])
    rows_s = ref["mask"] if not acc_s else torch.ones_like(ref["mask"])
    if case["kind"] == "exact":
        assert lin and float(ref["dE"].abs().max()) <= 256
        if got.get("dE") is not None:
            check_exact(what + "dE", got["dE"][rows], ref["dE"][rows])
        check_exact(what + "d_weights", got["ds"][rows_s], ref["ds"][rows_s])
        return
    add = U24 * ref["dE"].abs() if acc else 0.0        # adding the old contents rounds once
    if lin:
        assert not acc_s                               # (the weighted pooling always writes d_weights)
        dE_slack = add + torch.zeros_like(ref["dE"])   # w d_pooled: a product of two bf16-representable values, exact in fp32
        ds_bound = sum_bounds(ref["ds_mag"], HID)
    else:
        emu = pool_bwd_ref(*args, dt=torch.float32)
        dE_slack = softmax_bound("w d_pooled", ref["wdp"].abs(), emu["wdp"], ref["wdp"], what) + add
        ds_mag = ref["ds_mag"] + (case["ds0"].double().abs() if acc_s else 0.0)
        ds_bound = (softmax_bound("d_scores", ds_mag, emu["ds"], ref["ds"], what),)
    if got.get("dE") is not None:
        dE_bound = stored(ref["dE"], dE_slack)
        dE_bound[~ref["mask"]] = 0.0                   # a row of no bag or view keeps its contents to the bit
        check(what + "dE", got["dE"][rows], ref["dE"][rows], dE_bound[rows])
    check(what + "d_scores", got["ds"][rows_s], ref["ds"][rows_s], *[b[rows_s] for b in ds_bound])


def emulate_pool(case, lin, acc, acc_s):
    """The contract on the CPU: (forward dict, backward dict) in fp32, dE stored as bf16."""
    fwd = pool_fwd_ref(case, lin, torch.float32)
    bwd = pool_bwd_ref(case, lin, fwd["pooled"], fwd["m"], fwd["l"], acc, acc_s, torch.float32)
    return fwd, dict(dE=rb(bwd["dE"]), ds=bwd["ds"])


# --------------------------------------------------------------------------------------------------------------------------------- gate
def gate_case(T, H, seed, kind, p=0.0):
    """E [T, H*512]; Wa, Wb [H, 512, 512] bf16-representable; ba, bb, wc [H, 512], bc [H] fp32; d_scores [T, H]; starting dE0."""
    s = HID ** -0.5
    E = token_operand((T, H * HID), seed, kind)
    Wa, Wb = uniform((H, HID, HID), seed + 1, s), uniform((H, HID, HID), seed + 2, s)
    g = torch.Generator().manual_seed(seed + 3)
    ba, bb, wc = ((torch.rand((H, HID), generator=g) * 2 - 1) * s for _ in range(3))
    bc = (torch.rand((H,), generator=g) * 2 - 1) * s
    ds = token_operand((T, H), seed + 4, kind)
    if kind == "cancelling":
        for c in range(H):
            mirror(E, 1, -1, c * HID, (c + 1) * HID)
        mirror(E, 0, +1)
        mirror(Wa, 2, +1), mirror(Wb, 2, +1)
        mirror(ds, 0, -1)
    return dict(E=E, Wa=Wa, ba=ba, Wb=Wb, bb=bb, wc=wc, bc=bc, ds=ds, dE0=token_operand((T, H * HID), seed + 5, "uniform"), T=T, H=H, p=p,
                kind=kind)


def _keep(k, p, shape):
    """The dropout factor keep / (1 - p) in fp64 (all ones at p = 0)."""
    if p == 0 or k is None:
        return torch.ones(shape, dtype=F64)
    return k.double().view(shape) / (1.0 - p)


def gate_fwd_ref(case, device="cpu"):
    """fp64 tanh / sigmoid [T, H, 512] of the pre-activations with their bounds as stored bf16 values: the function's tolerance, the
    pre-activation's fp32 sum bound and the rounding of the folded bias (tests/test_activation_domain_gpu.py), through slopes <= 1, 1/4."""
    T, H = case["T"], case["H"]
    E = case["E"].to(device).double().view(T, H, HID)
    out = {}
    for name, W, b, fn, tol, slope in (("act_a", "Wa", "ba", torch.tanh, TANH_TOL, 1.0), ("act_b", "Wb", "bb", torch.sigmoid, SIGMOID_TOL, 0.25)):
        Wd, bd = case[W].to(device).double(), case[b].to(device).double()
        z = torch.einsum("tck,cjk->tcj", E, Wd) + bd
        mag = torch.einsum("tck,cjk->tcj", E.abs(), Wd.abs()) + bd.abs()
        ref = fn(z)
        arg = SUM_TOL * mag + 2.0 ** -23 * (bd.abs() + z.abs())
        slack = tol + slope * arg
        out[name] = (ref.cpu(), stored(ref, slack).cpu())
    return out


def gate_scores_ref(case, act_a, act_b, ka, kb):
    """scores [T, H] in fp64 from the STORED activations (exact inputs): bc + sum_j wc inv^2 keep a b; (ref, bound, second).  The factor
    wc inv^2 is rounded once, the products enter by FMA: one term rounding."""
    T, H, p = case["T"], case["H"], case["p"]
    shape = (T, H, HID)
    t = act_a.double().view(shape) * _keep(ka, p, shape) * act_b.double().view(shape) * _keep(kb, p, shape) * case["wc"].double()
    ref = t.sum(2) + case["bc"].double()
    mag = t.abs().sum(2) + case["bc"].double().abs()
    return (ref,) + sum_bounds(mag, HID + 1, term_roundings=2)


def gate_bwd_ref(case, act_a, act_b, ka, kb, acc, pool=None, device="cpu"):
    """The gate backward in fp64 from the STORED activations: name -> (ref, bound, second or None) for dE (bf16; with the pooling term
    w d_pooled of the fused call and / or the starting contents), dWa, dWb, dba, dbb, dwc, dbc.
    pool = (term fp64 [T, H*512], slack of the term) of gate_pool_term()."""
    T, H, p = case["T"], case["H"], case["p"]
    shape = (T, H, HID)
    dv = lambda x: x.to(device).double()       # noqa: E731
    a, b = dv(act_a).view(shape), dv(act_b).view(shape)
    fa, fb = _keep(ka, p, shape).to(device), _keep(kb, p, shape).to(device)
    ds, wc = dv(case["ds"])[:, :, None], dv(case["wc"])
    E = dv(case["E"]).view(shape)
    g = ds * wc
    dza = g * (b * fb) * fa * (1 - a * a)
    dzb = g * (a * fa) * fb * (b * (1 - b))
    pab = ds * (a * fa) * (b * fb)
    sc = case["kind"] == "row_scaled"          # every parameter gradient contracts over the token rows
    out = {"dba": (dza.sum(0),) + sum_bounds(dza.abs().sum(0), T, DZ_ROUNDINGS, scaled=sc),
           "dbb": (dzb.sum(0),) + sum_bounds(dzb.abs().sum(0), T, DZ_ROUNDINGS, scaled=sc),
           "dwc": (pab.sum(0),) + sum_bounds(pab.abs().sum(0), T, 8, scaled=sc),
           "dbc": (ds.sum(0)[:, 0],) + sum_bounds(ds.abs().sum(0)[:, 0], T, scaled=sc)}
    # the bf16 dz the contractions read: within DZ_ROUNDINGS fp32 roundings of dz, then stored
    ea = stored(dza, DZ_ROUNDINGS * U24 * dza.abs())
    eb = stored(dzb, DZ_ROUNDINGS * U24 * dzb.abs())
    Wa, Wb = dv(case["Wa"]), dv(case["Wb"])
    dE = torch.einsum("tcj,cjk->tck", dza, Wa) + torch.einsum("tcj,cjk->tck", dzb, Wb)
    dE_mag = torch.einsum("tcj,cjk->tck", dza.abs(), Wa.abs()) + torch.einsum("tcj,cjk->tck", dzb.abs(), Wb.abs())
    dE_dz = torch.einsum("tcj,cjk->tck", ea, Wa.abs()) + torch.einsum("tcj,cjk->tck", eb, Wb.abs())
    dE, dE_mag, dE_dz = (x.reshape(T, H * HID) for x in (dE, dE_mag, dE_dz))
    extra = dE_dz
    if pool is not None:
        dE = dE + pool[0].to(device)
        extra = extra + pool[1].to(device) + U24 * dE.abs()
    if acc:
        dE = dE + dv(case["dE0"])
        extra = extra + U24 * dE.abs()
    b1, b2 = sum_bounds(dE_mag, 2 * HID, extra=extra)
    out["dE"] = (dE, stored(dE, b1), stored(dE, b2))
    for name, dz, e in (("dWa", dza, ea), ("dWb", dzb, eb)):
        ref = torch.einsum("tcj,tck->cjk", dz, E)
        mag = torch.einsum("tcj,tck->cjk", dz.abs(), E.abs())
        out[name] = (ref,) + sum_bounds(mag, T, extra=torch.einsum("tcj,tck->cjk", e, E.abs()), scaled=sc)
    return {k: tuple(x.cpu() for x in v) for k, v in out.items()}


def gate_pool_term(scores, stat_m, stat_l, d_pooled, row_bag, H):
    """The pooling term of the fused backward, w[t, c] d_pooled[bag(t), c, :] with w = exp(scores - m) / l from the GIVEN scores and
    statistics, in fp64, and its slack (softmax_bound)."""
    def term(dt):
        rbag = row_bag.long()
        w = torch.exp(scores.to(dt) - stat_m.to(dt)[rbag]) * (1.0 / stat_l.to(dt)[rbag])
        return (w[:, :, None] * d_pooled.to(dt).view(-1, H, HID)[rbag]).reshape(scores.shape[0], H * HID)
    ref, emu = term(F64), term(torch.float32)
    return ref, softmax_bound("pool term", ref.abs(), emu, ref)


def emulate_gate(case, ka=None, kb=None, acc=0):
    """The contract on the CPU in fp32: stored activations (bf16), scores from them, dz rounded to bf16 before the contractions."""
    T, H, p = case["T"], case["H"], case["p"]
    shape = (T, H, HID)
    E = case["E"].view(shape)
    za = torch.einsum("tck,cjk->tcj", E, case["Wa"]) + case["ba"]
    zb = torch.einsum("tck,cjk->tcj", E, case["Wb"]) + case["bb"]
    a, b = rb(torch.tanh(za.double()).float()), rb(torch.sigmoid(zb.double()).float())
    fa, fb = _keep(ka, p, shape).float(), _keep(kb, p, shape).float()
    sc = ((a * fa) * (b * fb) * case["wc"]).sum(2) + case["bc"]
    ds = case["ds"][:, :, None]
    g = ds * case["wc"]
    dza32, dzb32 = g * (b * fb) * fa * (1 - a * a), g * (a * fa) * fb * (b * (1 - b))
    dza, dzb = rb(dza32), rb(dzb32)
    dE = (torch.einsum("tcj,cjk->tck", dza, case["Wa"]) + torch.einsum("tcj,cjk->tck", dzb, case["Wb"])).reshape(T, H * HID)
    if acc:
        dE = dE + case["dE0"]
    return dict(act_a=a, act_b=b, scores=sc, dE=rb(dE), dWa=torch.einsum("tcj,tck->cjk", dza, E), dWb=torch.einsum("tcj,tck->cjk", dzb, E),
                dba=dza32.sum(0), dbb=dzb32.sum(0), dwc=(ds * (a * fa) * (b * fb)).sum(0), dbc=case["ds"].sum(0))


# ---------------------------------------------------------------------------------------------------------------- LayerNorm-GELU-Dropout
def gelu64(t):
    return 0.5 * t * (1.0 + torch.erf(t / math.sqrt(2.0)))


def gelu_grad64(t):
    return 0.5 * (1.0 + torch.erf(t / math.sqrt(2.0))) + t * torch.exp(-0.5 * t * t) / math.sqrt(2.0 * math.pi)


def ln_case(rows, W, seed, kind, p=0.0, groups=None):
    """x, dy [rows, W] bf16-representable; gamma, beta [W]; bias [W] or, with groups = list of group lengths, [G, W]; keep uint8 or None."""
    x = token_operand((rows, W), seed, kind, 3.0) + (0.5 if kind == "uniform" else 0.0)
    x = rb(x)
    dy = token_operand((rows, W), seed + 1, kind)
    if kind == "cancelling":
        mirror(x, 0, +1)
        mirror(dy, 0, -1)
    g = torch.Generator().manual_seed(seed + 2)
    gam, beta = 1 + 0.2 * torch.randn(W, generator=g), 0.3 * torch.randn(W, generator=g)
    G = 1 if groups is None else len(groups)
    bias = 0.7 * torch.randn(G, W, generator=g)
    keep = (torch.rand(rows, W, generator=g) >= p).to(torch.uint8) if p > 0 else None
    return dict(x=x, dy=dy, gamma=gam, beta=beta, bias=bias if groups is not None else bias[0], keep=keep, p=p, groups=groups, kind=kind,
                eps=1e-5)


def _ln_bias_rows(case):
    rows = case["x"].shape[0]
    if case["groups"] is None:
        return case["bias"].double()[None].expand(rows, -1), None
    gid = torch.repeat_interleave(torch.arange(len(case["groups"])), torch.tensor(case["groups"]))
    return case["bias"].double()[gid], gid


def ln_fwd_ref(case, mean=None, rstd=None):
    """name -> (ref, bound): mean, rstd [rows] against fp64 of x + bias; y from the STORED mean / rstd when given (exact inputs)."""
    x, W = case["x"].double(), case["x"].shape[1]
    brow, _ = _ln_bias_rows(case)
    v = x + brow
    m64 = v.mean(1)
    c = v - m64[:, None]
    q = (c * c).mean(1)
    r64 = (q + case["eps"]).rsqrt()
    # v = x + bias rounds once; the sum of W values / W
    m_bound = (SUM_TOL + U24) * v.abs().mean(1)
    # c = v - mean: the roundings of v, of the mean and of the difference, 3 * 2^-24 (|v| + |mean|), into c^2 with slope 2 |c|; the sum
    dq = (2 * c.abs() * (3 * U24 * (v.abs() + m64.abs()[:, None]) + m_bound[:, None])).mean(1) + (SUM_TOL + 2 * U24) * q
    # rsqrt: slope rstd^3 / 2; the hardware rsqrt is good to 1 ulp, the result rounds, the addition of eps rounds: 4 * 2^-24 rstd
    r_bound = 0.5 * r64 ** 3 * dq + 4 * U24 * r64
    out = {"mean": (m64, m_bound), "rstd": (r64, r_bound)}
    if mean is not None:
        mean, rstd = mean.double()[:, None], rstd.double()[:, None]
        h = (v - mean) * rstd
        dh = 3 * U24 * (v.abs() + mean.abs()) * rstd
        t = h * case["gamma"].double() + case["beta"].double()
        dt = case["gamma"].double().abs() * dh + 2 * U24 * ((h * case["gamma"].double()).abs() + case["beta"].double().abs())
        kp = _keep(case["keep"], case["p"], x.shape)
        ref = gelu64(t) * kp
        tol = torch.where(t.abs() <= 4, torch.full_like(t, GELU_TOL_CORE), GELU_TOL_TAIL * t.abs())
        slack = kp * (tol + GELU_SLOPE * dt) + 2 * U24 * ref.abs()
        out["y"] = (ref, stored(ref, slack))
    return out


def ln_bwd_ref(case, mean, rstd):
    """The backward in fp64 from the STORED mean / rstd: name -> (ref, bound, second or None) for dx (bf16), dgamma, dbeta and dbias [W]
    or dgroup_bias [G, W].  GELU' carries the bf16 mode's polynomial tolerance GELU_GRAD_TOL; the rest is fp32 roundings."""
    x, dy = case["x"].double(), case["dy"].double()
    rows, W = x.shape
    gam, beta = case["gamma"].double(), case["beta"].double()
    brow, gid = _ln_bias_rows(case)
    mean, rstd = mean.double()[:, None], rstd.double()[:, None]
    v = x + brow
    h = (v - mean) * rstd
    e_h = 3 * U24 * (v.abs() + mean.abs()) * rstd
    t = h * gam + beta
    e_t = gam.abs() * e_h + 2 * U24 * ((h * gam).abs() + beta.abs())
    kp = _keep(case["keep"], case["p"], x.shape)
    dt = dy * kp * gelu_grad64(t)
    e_dt = dy.abs() * kp * (GELU_GRAD_TOL + GELU_GRAD_SLOPE * e_t) + 3 * U24 * dt.abs()
    dh = dt * gam
    e_dh = e_dt * gam.abs() + U24 * dh.abs()
    m1, m2 = dh.mean(1, keepdim=True), (dh * h).mean(1, keepdim=True)
    e_m1 = e_dh.mean(1, keepdim=True) + SUM_TOL * dh.abs().mean(1, keepdim=True)
    e_m2 = (e_dh * h.abs() + dh.abs() * e_h).mean(1, keepdim=True) + (SUM_TOL + U24) * (dh * h).abs().mean(1, keepdim=True)
    dx = rstd * (dh - m1 - h * m2)
    e_dx = rstd * (e_dh + e_m1 + h.abs() * e_m2 + e_h * m2.abs()) + 4 * U24 * rstd * (dh.abs() + m1.abs() + (h * m2).abs())
    out = {"dx": (dx, stored(dx, e_dx), None)}
    sc = case["kind"] == "row_scaled"          # the column reductions contract over the rows
    out["dgamma"] = ((dt * h).sum(0),) + sum_bounds((dt * h).abs().sum(0), rows, 1, (e_dt * h.abs() + dt.abs() * e_h).sum(0), sc)
    out["dbeta"] = (dt.sum(0),) + sum_bounds(dt.abs().sum(0), rows, 0, e_dt.sum(0), sc)
    if gid is None:
        out["dbias"] = (dx.sum(0),) + sum_bounds(dx.abs().sum(0), rows, 0, e_dx.sum(0), sc)
    else:
        G = len(case["groups"])
        sel = torch.nn.functional.one_hot(gid, G).double().t()            # [G, rows]
        out["dgroup_bias"] = (sel @ dx,) + sum_bounds(sel @ dx.abs(), max(case["groups"] + [1]), 0, sel @ e_dx, sc)
    return out


def emulate_ln(case):
    """The contract on the CPU in fp32 (erf GELU in place of the polynomial, inside its tolerance): forward and backward dicts."""
    x, dy, gam, beta = case["x"], case["dy"], case["gamma"], case["beta"]
    brow, gid = _ln_bias_rows(case)
    v = x + brow.float()
    mean = v.mean(1)
    c = v - mean[:, None]
    rstd = ((c * c).mean(1) + case["eps"]).rsqrt()
    h = c * rstd[:, None]
    t = h * gam + beta
    kp = _keep(case["keep"], case["p"], x.shape).float()
    fwd = dict(mean=mean, rstd=rstd, y=rb(gelu64(t.double()).float() * kp))
    dt = dy * kp * gelu_grad64(t.double()).float()
    dh = dt * gam
    m1, m2 = dh.mean(1, keepdim=True), (dh * h).mean(1, keepdim=True)
    dx = rstd[:, None] * (dh - m1 - h * m2)
    bwd = dict(dx=rb(dx), dgamma=(dt * h).sum(0), dbeta=dt.sum(0))
    if gid is None:
        bwd["dbias"] = dx.sum(0)
    else:
        bwd["dgroup_bias"] = torch.nn.functional.one_hot(gid, len(case["groups"])).float().t() @ dx
    return fwd, bwd
