"""fp64 references and per-element error bounds of the split-fp16 engine (csrc/split_engine.hpp, csrc/split_gemm.hip and the _img entry
points of csrc/abmil_pool.hip), for tests/test_split_elements_gpu.py (the kernels) and tests/test_split_bounds_cpu.py (these checkers,
against a CPU emulation and seeded faults).  The generic checkers are those of tests/_bf16_bounds.py, imported: worst_ratio, passes,
check_exact, gamma, sum_bounds, measure_ratio.  check() here is that file's check() with the tag SPLITERR in its printed line.

The contract, read from the sources.
  Image (split_engine.hpp sp_split8, sp_scale_for; split_gemm.hip sp_convert_kernel, sp_image_rows_kernel, sp_image_rows_reg_kernel):
    v = s x in fp32 (exact: s is a power of two), hi = RN16(v), lo = RN16(v - hi) with v - hi exact in fp32.  element = (hi + lo) / s.
    mdl_split_image: s = 2^(14 - e) for absmax = f 2^e, f in [0.5, 1) (sp_scale_for; 1 for absmax = 0), so s absmax is in [2^13, 2^14);
    scale = {s, absmax}, the absmax exact (an atomic max of bit patterns).
    mdl_split_image_rows: the same rule per row, row_inv[r] = 1 / s_r, 0 for an all-zero row (whose image is zero: s_r = 1 times 0);
    scale = {1, max |X|} where scale is given.
    Element bound (derived): |v - hi| <= 2^-11 2^E for |v| in [2^E, 2^(E+1)) and v - hi is a multiple of 2^(E-23); RN16 of it keeps 11
    bits, an error of at most 2^(E-23) <= 2^-23 |v|, or 2^-25 where lo is an fp16 subnormal (spacing 2^-24):
        |dec - x| <= max(2^-23 |x|, 2^-25 / s).
    The CPU definition (torch.half conversions) meets it with a worst ratio of exactly 1.0 (tests/test_split_bounds_cpu.py).  The planes
    are also held to the definition bit for bit: both sides round to nearest even.
  Product from the planes (sp_nt_kernel, sp_nt_tall_kernel, sp_tn_kernel): each 16-bit product is exact in fp32, every sum is fp32, 16 k
    per MFMA.  3 terms: sum_k (ah bh + ah bl + al bh); 2 terms: NT drops ah bl (B enters as its hi plane), TN drops al bh (A enters as its
    hi plane).  The reference is that expression in fp64 ON THE PLANES THE KERNEL READ, so only the accumulation is left to bound:
    sum_bounds(mag, 3 K or 2 K): the working SUM_TOL mag and the proven gamma(n) mag; a contraction over token rows that the inputs scale
    by 2^[-12, 12] is held to the proven ceiling alone (sum_bounds(scaled=True)).
  Epilogue (the emit lambdas of the three kernels): r = acc * (inv * a_row_mul[m]), inv = 1 / (s_a s_b) exact; r *= b_col_mul[n];
    r += bias[n]; r += group_bias[row_group[m]][n]; r += C (accumulate).  A factor that is a power of two (row_inv) is exact, any other
    costs one rounding; each addition costs one: term_roundings.  absmax_out is the maximum of |r| as stored, exact.
  Integer operands of [-7, 7]: lo == 0, the scale is at most 2^13, every partial sum is an integer multiple of the common factor below
    2^24 of it: the product matches fp64 bit for bit in any summation order.
  Pooling on the image (abmil_pool.hip, PoolLd of the image type): E = (hi + lo) * (1 / s) formed in fp32 -- one rounding of hi + lo
    (exact whenever lo is not far below hi's last bit) -- then the fp32 kernels' arithmetic.  The reference takes the decoded image; the
    bounds are those of the bf16 file's softmax paragraph (SOFTMAX_FACTOR x a measured ratio) with ratios measured over this file's cases.
  The gate (csrc/abmil_gate_split.hip) and the LayerNorm image kernels (csrc/preattn_act.hip): their contracts, with the images they
    build themselves from bounds, stand above their sections below.
Constants: which are derived, taken from other tests or measured is said beside each."""
import math

import torch

from tests._bf16_bounds import (F64, HID, SOFTMAX_FACTOR, SUM_TOL, U24, bag_rows, check_exact, gamma, measure_ratio, mirror,  # noqa: F401
                                passes, rel_err, row_scales, sum_bounds, worst_ratio)

F16 = torch.float16
KINDS = ("uniform", "row_scaled", "cancelling")
KINDS4 = KINDS + ("integer",)
# SUM_TOL = 4e-7: taken from tests/test_dispatch_edges_gpu.py::_chain_check (imported through tests/_bf16_bounds.py)
# derived, above: the two arms of the image element bound
IMG_REL, IMG_ABS = 2.0 ** -23, 2.0 ** -25
# the norm criterion tests/test_split_gpu.py and tests/test_grad_terms_gpu.py assert (taken from them)
OLD_NORM_TOL = 1e-6
# measured (measure_ratio; see pool_img_bounds): the worst |error| / (2^-24 mag) of a plain torch fp32 CPU evaluation of the pooling
# formulas on the decoded image against fp64, over every case of test_pool_img of tests/test_split_elements_gpu.py (bags 333, 0, 1, 63,
# 65 ragged and 65, 65, 65 dense; H in {1, 4}; the three input kinds), the score gradients on the forward results the kernel stored.
# The case that sets each figure is named.  The measurement runs on the CPU reference, never on the kernel.
SOFTMAX_RATIO = {
    "stat_l": 2.95,       # sum_t exp(s_t - m), mag = the sum                                   (dense, H = 4, cancelling: 2.945)
    "pooled": 6.86,       # sum_t w_t E_t, mag = sum_t w_t |E_t|                                (dense, H = 4, row_scaled: 6.856)
    "d_scores": 0.61,     # w (<E, dp> - <pooled, dp>), mag = w (sum |E dp| + sum |pooled dp|)  (ragged, H = 4, cancelling: 0.604)
}


def check(what, got, ref, bound, second=None):
    """Asserts |got - ref| <= bound at every element (and <= second, where given); prints SPLITERR <what> <worst ratio>."""
    assert tuple(got.shape) == tuple(ref.shape), (what, tuple(got.shape), tuple(ref.shape))
    r, i = worst_ratio(got, ref, bound)
    print("SPLITERR %s worst |err| / bound = %.3f at flat index %d of %s" % (what, r, i, tuple(ref.shape)))
    assert r <= 1.0, (what, r, i)
    if second is not None:
        r2, i2 = worst_ratio(got, ref, second)
        assert r2 <= 1.0, (what + " (gamma_n ceiling)", r2, i2)
    return r


# ------------------------------------------------------------------------------------------------------------------------------- inputs
def uniform(shape, seed, scale=1.0):
    """fp32 values of [-scale, scale] with all 24 bits in use: torch.rand alone yields multiples of 2^-24, which the two planes hold
    exactly at every magnitude -- the second factor fills the mantissa, so that the lo plane is a rounded value."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(shape, generator=g, dtype=torch.float32) * 2 - 1
    return u * (0.75 + 0.25 * torch.rand(shape, generator=g, dtype=torch.float32)) * scale


def integers(shape, seed, top=7):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-top, top + 1, shape, generator=g).float()


def operand(shape, seed, kind, scale=1.0):
    """A [rows, K] operand of the given kind (the cancelling structure is put on by the case)."""
    if kind == "integer":
        return integers(shape, seed)
    x = uniform(shape, seed, scale)
    if kind == "row_scaled":
        x = x * row_scales(shape[0], seed + 104729)
    return x


def nt_case(M, N, K, seed, kind):
    """a [M, K], b [N, K], bias [N], c0 [M, N], group bias [3, N] with row_group [M] changing inside the tiles."""
    a, b = operand((M, K), seed, kind), operand((N, K), seed + 1, kind, K ** -0.5 if kind != "integer" else 1.0)
    if kind == "cancelling":            # the columns of a negate, those of b repeat: every element of the product is 0 exactly
        mirror(a, 1, -1), mirror(b, 1, +1)
    if kind == "integer":
        bias, c0, gb = integers((N,), seed + 2), integers((M, N), seed + 3), integers((3, N), seed + 4)
    else:
        bias, c0, gb = uniform((N,), seed + 2, 0.3), uniform((M, N), seed + 3), uniform((3, N), seed + 4, 0.3)
    return dict(a=a, b=b, bias=bias, c0=c0, gb=gb, row_group=(torch.arange(M) * 7 // 5 % 3).to(torch.int32), kind=kind)


def tn_case(T, Mi, N, seed, kind):
    """x [T, Mi] (the A operand), dy [T, N] (the B operand): out [N, Mi] = dy^T x."""
    x, dy = operand((T, Mi), seed, kind), operand((T, N), seed + 1, kind)
    if kind == "cancelling":            # the token rows of x negate, those of dy repeat
        mirror(x, 0, -1), mirror(dy, 0, +1)
    return dict(x=x, dy=dy, kind=kind)


# -------------------------------------------------------------------------------------------------------------------------------- image
def scale_for(absmax):
    """sp_scale_for: 2^(14 - e) for absmax = f 2^e, f in [0.5, 1); 1 for 0."""
    absmax = float(absmax)
    if not absmax > 0 or not absmax < 3.0e38:
        return 1.0
    return 2.0 ** (14 - math.frexp(absmax)[1])


def split_planes(x, s, truncate_lo=False):
    """The definition: (hi, lo) fp16 planes of s x, s a power of two (a float, or a [rows, 1] tensor)."""
    v = x.float() * s
    hi = v.to(F16)
    r = v - hi.float()
    if truncate_lo:                   # the fault: lo cut toward zero instead of rounded
        lo = r.to(F16)
        over = lo.float().abs() > r.abs()
        bits = lo.view(torch.int16)
        lo = torch.where(over, (bits - 1).view(F16), lo)
    else:
        lo = r.to(F16)
    return hi, lo


def image(x):
    """mdl_split_image on the CPU: (hi, lo, s)."""
    s = scale_for(x.abs().max()) if x.numel() else 1.0
    return split_planes(x, s) + (s,)


def row_scale_rule(x):
    """The per-row scales of mdl_split_image_rows and its row_inv (0 for an all-zero row): ([rows] s_r, [rows] row_inv), fp32."""
    m = x.abs().amax(1) if x.shape[1] else torch.zeros(x.shape[0])
    s = torch.tensor([scale_for(v) for v in m.tolist()], dtype=torch.float32)
    return s, torch.where(m > 0, 1.0 / s, torch.zeros_like(s))


def image_rows(x):
    """mdl_split_image_rows on the CPU: (hi, lo, s_r [rows], row_inv [rows])."""
    s, inv = row_scale_rule(x)
    return split_planes(x, s[:, None]) + (s, inv)


def pack(hi, lo, rsb=None, fill=0xFF):
    """The image bytes: uint8 [rows, rsb] with, per 32-column block, the hi plane | the lo plane; bytes past 4 K hold `fill`."""
    rows, K = hi.shape
    rsb = 4 * K if rsb is None else rsb
    body = torch.stack([hi.view(rows, K // 32, 32), lo.view(rows, K // 32, 32)], 2).contiguous().view(torch.uint8).view(rows, 4 * K)
    out = torch.full((rows, rsb), fill, dtype=torch.uint8)
    out[:, :4 * K] = body
    return out


def unpack(raw, K):
    """(hi, lo) fp16 [rows, K] of image bytes uint8 [rows, rsb]."""
    rows = raw.shape[0]
    hl = raw[:, :4 * K].contiguous().view(F16).view(rows, K // 32, 2, 32)
    return hl[:, :, 0].reshape(rows, K), hl[:, :, 1].reshape(rows, K)


def decode(hi, lo, s=1.0):
    """fp64 (hi + lo) / s; s a float or a [rows] tensor."""
    s = s.double()[:, None] if torch.is_tensor(s) else float(s)
    return (hi.double() + lo.double()) / s


def image_bound(x, s):
    """max(2^-23 |x|, 2^-25 / s) per element (derived, above); s a float or a [rows] tensor."""
    s = s.double()[:, None] if torch.is_tensor(s) else float(s)
    return torch.maximum(IMG_REL * x.double().abs(), IMG_ABS / s + torch.zeros_like(x, dtype=F64))


def check_image(what, hi, lo, x, s):
    """The planes of x at scale(s) s: finite, the element bound at every element, and the definition bit for bit."""
    assert bool(torch.isfinite(hi.float()).all()) and bool(torch.isfinite(lo.float()).all()), what + ": inf / NaN in the planes"
    check(what + "element", decode(hi, lo, s), x.double(), image_bound(x, s))
    s2 = s.float()[:, None] if torch.is_tensor(s) else s
    dhi, dlo = split_planes(x, s2)
    check_exact(what + "hi plane", hi, dhi)
    check_exact(what + "lo plane", lo, dlo)


def check_scale(what, s, absmax, x):
    """scale = {s, absmax} of mdl_split_image: the absmax exact, s by sp_scale_for's rule (hence a power of two, s absmax in [2^13, 2^14))."""
    want = float(x.abs().max()) if x.numel() else 0.0
    assert float(absmax) == want, (what + "absmax", float(absmax), want)
    assert float(s) == scale_for(want), (what + "scale", float(s), scale_for(want))
    assert want == 0 or 2.0 ** 13 <= float(s) * want < 2.0 ** 14, what


def check_row_inv(what, row_inv, x):
    """row_inv of mdl_split_image_rows: 1 / s_r by the rule, 0 for an all-zero row, to the bit."""
    check_exact(what + "row_inv", row_inv, row_scale_rule(x)[1])


# ----------------------------------------------------------------------------------------------------------------------------- products
def _exact_factor(v):
    """Every entry is 0 or a power of two: multiplying by it does not round."""
    return v is None or bool((torch.frexp(v.float())[0].abs()[v != 0] == 0.5).all())


def _terms_nt(ah, al, bh, bl, terms, mm):
    out = mm(ah, bh.t()) + mm(al, bh.t())
    return out + mm(ah, bl.t()) if terms == 3 else out


def nt_ref(ah, al, bh, bl, inv, terms=3, a_row_mul=None, b_col_mul=None, bias=None, gb_rows=None, c0=None):
    """(ref, bound, proven ceiling) of C = inv a_row_mul[m] b_col_mul[n] sum_k (ah bh + al bh [+ ah bl]) + bias[n] + gb_rows[m][n] + c0
    in fp64 from the planes; inv = 1 / (s_a s_b)."""
    return nt_finish(nt_raw(ah, al, bh, bl, terms), terms * ah.shape[1], inv, a_row_mul, b_col_mul, bias, gb_rows, c0)


def nt_raw(ah, al, bh, bl, terms=3):
    """(sum of the plane products in fp64, the same on absolute values): what several epilogue variants of one image pair share."""
    p = [t.double() for t in (ah, al, bh, bl)]
    return _terms_nt(*p, terms, torch.matmul), _terms_nt(*[t.abs() for t in p], terms, torch.matmul)


def nt_finish(raw_mag, n, inv, a_row_mul=None, b_col_mul=None, bias=None, gb_rows=None, c0=None):
    """The epilogue of nt_ref on nt_raw's pair; n = terms x K addends."""
    raw, mag = raw_mag
    f = torch.full((1, 1), float(inv), dtype=F64)
    if a_row_mul is not None:
        f = f * a_row_mul.double()[:, None]
    if b_col_mul is not None:
        f = f * b_col_mul.double()[None, :]
    ref, mag = raw * f, mag * f.abs()
    roundings = (not _exact_factor(a_row_mul)) + (not _exact_factor(b_col_mul))
    for add in (bias, gb_rows, c0):
        if add is not None:
            ref, mag, roundings = ref + add.double(), mag + add.double().abs(), roundings + 1
    return (ref,) + sum_bounds(mag, n, roundings)


def tn_ref(ah, al, bh, bl, inv, terms=3, scaled=False):
    """(ref, bound, proven ceiling) of out [N, Mi] = inv sum_t (bh ah + bl ah [+ bh al]) in fp64 from the planes of A [T, Mi], B [T, N]."""
    ah, al, bh, bl = (t.double() for t in (ah, al, bh, bl))
    raw = (bh + bl).t() @ ah
    mag = (bh.abs() + bl.abs()).t() @ ah.abs()
    if terms == 3:
        raw, mag = raw + bh.t() @ al, mag + bh.abs().t() @ al.abs()
    return (raw * inv,) + sum_bounds(mag * abs(inv), terms * max(ah.shape[0], 1), scaled=scaled)


def emulate_nt(ah, al, bh, bl, inv, terms=3, a_row_mul=None, b_col_mul=None, bias=None, gb_rows=None, c0=None, skip_block=None):
    """The contract on the CPU: the plane products in fp32, 16 k per accumulate, block by block; the epilogue in the kernel's order.
    skip_block = (k block, row slice): the fault of a dropped 32-k block in those rows."""
    ah, al, bh, bl = (t.float() for t in (ah, al, bh, bl))
    M, K = ah.shape
    acc = torch.zeros(M, bh.shape[0])
    for k0 in range(0, K, 32):
        acc = _acc_in_order(acc, ah, al, bh, bl, k0, terms, skip_block)
    r = acc * (torch.tensor(float(inv)) * a_row_mul.float()[:, None] if a_row_mul is not None else torch.tensor(float(inv)))
    if b_col_mul is not None:
        r = r * b_col_mul.float()[None, :]
    for add in (bias, gb_rows, c0):
        if add is not None:
            r = r + add.float()
    return r


def _acc_in_order(acc, ah, al, bh, bl, k0, terms, skip_block):
    """acc += the 32-k block at k0, one fp32 accumulate per 16 k and term (the MFMA order), except in the rows of a skipped block."""
    new = acc
    for a, b in (((ah, bh), (ah, bl), (al, bh)) if terms == 3 else ((ah, bh), (al, bh))):
        for k in (k0, k0 + 16):
            new = new + a[:, k:k + 16] @ b[:, k:k + 16].t()
    if skip_block is not None and skip_block[0] == k0 // 32:
        new = new.clone()
        new[skip_block[1]] = acc[skip_block[1]]
    return new


def emulate_tn(ah, al, bh, bl, inv, terms=3, skip_chunk=None):
    """The TN contract on the CPU: out [N, Mi], 16 tokens per accumulate.  skip_chunk = (chunk, n slice, m slice): a dropped 32-token
    chunk in that part of the output."""
    ah, al, bh, bl = (t.float() for t in (ah, al, bh, bl))
    T = ah.shape[0]
    acc = torch.zeros(bh.shape[1], ah.shape[1])
    for t0 in range(0, T, 32):
        new = acc
        for a, b in (((ah, bh), (ah, bl), (al, bh)) if terms == 3 else ((ah, bh), (ah, bl))):
            for t in (t0, t0 + 16):
                if t < T:
                    new = new + b[t:t + 16].t() @ a[t:t + 16]
        if skip_chunk is not None and skip_chunk[0] == t0 // 32:
            new = new.clone()
            new[skip_chunk[1], skip_chunk[2]] = acc[skip_chunk[1], skip_chunk[2]]
        acc = new
    return acc * float(inv)


# ------------------------------------------------------------------------------------------------------------------ pooling on the image
POOL_BAGS = (((333, 0, 1, 63, 65), False), ((65, 65, 65), True))      # (bag lengths, dense): the cases SOFTMAX_RATIO is measured over
POOL_HEADS = (1, 4)


def pool_img_case(lens, H, kind):
    """tests/_bf16_bounds.pool_case with E given full fp32 mantissas (one factor per column, repeated in the second half of the columns:
    the cancelling structure stays).  case['E32'] is what the image is built from; case['E'] is to be set to the decoded image."""
    from tests import _bf16_bounds as B
    case = B.pool_case(lens, H, 7000 + H + sum(lens), kind)
    g = torch.Generator().manual_seed(7100 + H)
    f = 0.75 + 0.25 * torch.rand(H * HID // 2, generator=g)
    case["E32"] = case["E"] * torch.cat([f, f])
    return case


def pool_img_bounds(case, fwd=None):
    """The softmax pooling on the decoded image E (case of tests/_bf16_bounds.pool_case with E = the decoded image, fp64): references and
    bounds of pooled / stat_m / stat_l and, with the stored forward results `fwd`, of d_scores.  Each bound is SOFTMAX_FACTOR x
    SOFTMAX_RATIO x 2^-24 mag; the decode in fp32 (one rounding of hi + lo) adds 2^-24 mag.  Returns (dict name -> (ref, bound), dict of
    this case's own torch-fp32 ratios)."""
    from tests import _bf16_bounds as B
    ref, emu = B.pool_fwd_ref(case, False), B.pool_fwd_ref(case, False, torch.float32)
    out = {"stat_m": (ref["m"], None),
           "stat_l": (ref["l"], SOFTMAX_FACTOR * SOFTMAX_RATIO["stat_l"] * U24 * ref["l"]),
           "pooled": (ref["pooled"], (SOFTMAX_FACTOR * SOFTMAX_RATIO["pooled"] + 1) * U24 * ref["mag"])}
    ratios = {"stat_l": measure_ratio(emu["l"], ref["l"], ref["l"]), "pooled": measure_ratio(emu["pooled"], ref["pooled"], ref["mag"])}
    if fwd is not None:
        args = (case, False, fwd["pooled"], fwd["m"], fwd["l"], 0)
        r, e = B.pool_bwd_ref(*args, 0), B.pool_bwd_ref(*args, 0, dt=torch.float32)
        bound = (SOFTMAX_FACTOR * SOFTMAX_RATIO["d_scores"] + 1) * U24 * r["ds_mag"]
        out["d_scores"] = (r["ds"], bound, r["mask"])
        ratios["d_scores"] = measure_ratio(e["ds"], r["ds"], r["ds_mag"])
        acc = B.pool_bwd_ref(*args, 1)["ds"]                       # accumulate_scores: one more rounding, of the sum
        out["d_scores_acc"] = (acc, bound + U24 * acc.abs(), torch.ones_like(r["mask"]))
    return out, ratios


# --------------------------------------------------------------------------------------------------------------------------------- gate
# The gate on the split engine (csrc/abmil_gate_split.hip).  What the caller hands in -- the image of E, the saved activations, the
# scores and statistics of the pooling term -- is an exact input of the reference (E as its decoded planes).  The two images the gate
# builds itself are modelled by the image element bound with the scale of the documented rule:
#   weights: s_w = sp_scale_for(max(|Wa|, |Wb|)) over all heads (sp_weight_scale, then sp_gate_wk_kernel / sp_gate_wn_kernel);
#   dz:      s_dz = sp_scale_for(max|ds| max|wc| / (1-p)^2) (sp_bound_scale_kernel, a bound: no pass over dz), on top of the
#            DZ_ROUNDINGS fp32 roundings of gate_dz_t (taken from tests/_bf16_bounds.py: the same function).
# Both errors are carried through the contractions on absolute values.  A 3-term product of two images drops al bl, at most
# 2^-11 |a| 2^-11 |b| per product: DROPPED = 2^-22 of mag (derived).  With terms = 2 the operand that is not a gradient enters as its
# hi plane: the reference takes W_hi = RN16(s_w W) / s_w (by the definition) in dE and E's hi plane in dWa / dWb, and nothing is dropped.
# tanh / sigmoid tolerances: taken from tests/test_activation_domain_gpu.py through tests/_bf16_bounds.py.
DROPPED = 2.0 ** -22
# measured as SOFTMAX_RATIO above, for the weight exp(s - m) / l times d_pooled inside mdl_abmil_attnpool_bwd_split, over the cases of
# test_gate_fused_pooling_term (two ragged bags of 70 and 59 tokens, H in {1, 4}, the three kinds): worst at H = 4, row_scaled (3.540)
SOFTMAX_RATIO["pool term"] = 3.55


def gate_case(T, H, seed, kind, p=0.0):
    """tests/_bf16_bounds.gate_case with full fp32 mantissas: E32 [T, H*512] (what the image is built from), Wa, Wb [H, 512, 512], ba, bb,
    wc [H, 512], bc [H], ds [T, H], starting contents dE0."""
    s = HID ** -0.5
    E = operand((T, H * HID), seed, kind)
    Wa, Wb = uniform((H, HID, HID), seed + 1, s), uniform((H, HID, HID), seed + 2, s)
    ba, bb, wc = (uniform((H, HID), seed + 3 + i, s) for i in range(3))
    bc = uniform((H,), seed + 6, s)
    ds = operand((T, H), seed + 7, kind)
    if kind == "cancelling":
        for c in range(H):
            mirror(E, 1, -1, c * HID, (c + 1) * HID)
        mirror(E, 0, +1)
        mirror(Wa, 2, +1), mirror(Wb, 2, +1)
        mirror(ds, 0, -1)
    return dict(E32=E, Wa=Wa, ba=ba, Wb=Wb, bb=bb, wc=wc, bc=bc, ds=ds, dE0=uniform((T, H * HID), seed + 8), T=T, H=H, p=p, kind=kind)


def gate_weight_scale(case):
    return scale_for(max(float(case["Wa"].abs().max()), float(case["Wb"].abs().max())))


def gate_dz_scale(case):
    """sp_bound_scale_kernel in fp32: the scale of in[0] * in[1] * (inv * inv), inv = 1 / (1 - p) in fp32."""
    f = torch.float32
    inv = (torch.tensor(1.0, dtype=f) / (torch.tensor(1.0, dtype=f) - torch.tensor(case["p"], dtype=f))) if case["p"] > 0 else torch.tensor(1.0)
    return scale_for(float(case["ds"].abs().max() * case["wc"].abs().max() * (inv * inv)))


def gate_fwd_ref(case, E_dec, device="cpu"):
    """fp64 tanh / sigmoid [T, H, 512] of the pre-activations on the decoded image, with their bounds as fp32 values: the function's
    tolerance, and through slopes <= 1, 1/4 the pre-activation's sum bound, the weights' image error, the dropped al bl and the
    rounding of the folded bias."""
    from tests import _bf16_bounds as B
    T, H = case["T"], case["H"]
    E = E_dec.to(device).double().view(T, H, HID)
    s_w = gate_weight_scale(case)
    out = {}
    for name, W, b, fn, tol, slope in (("act_a", "Wa", "ba", torch.tanh, B.TANH_TOL, 1.0), ("act_b", "Wb", "bb", torch.sigmoid, B.SIGMOID_TOL, 0.25)):
        Wd, bd = case[W].to(device).double(), case[b].to(device).double()
        z = torch.einsum("tck,cjk->tcj", E, Wd) + bd
        mag = torch.einsum("tck,cjk->tcj", E.abs(), Wd.abs()) + bd.abs()
        e_w = torch.einsum("tck,cjk->tcj", E.abs(), image_bound(case[W], s_w).to(device))
        ref = fn(z)
        arg = (SUM_TOL + DROPPED) * mag + e_w + 2.0 ** -23 * (bd.abs() + z.abs())
        out[name] = (ref.cpu(), (tol + slope * arg + U24 * ref.abs()).cpu())
    return out


def gate_bwd_ref(case, E_dec, E_hi, act_a, act_b, ka, kb, acc, terms=3, pool=None, device="cpu"):
    """The gate backward in fp64 from the decoded image of E and the STORED activations: name -> (ref, bound, proven ceiling) for dE
    (with the pooling term of the fused call and / or the starting contents), dWa, dWb, dba, dbb, dwc, dbc.  E_hi: E's hi plane / s_e
    (terms = 2).  pool = (term fp64 [T, H*512], slack of the term)."""
    from tests import _bf16_bounds as B
    T, H, p = case["T"], case["H"], case["p"]
    shape = (T, H, HID)
    dv = lambda x: x.to(device).double()       # noqa: E731
    a, b = dv(act_a).view(shape), dv(act_b).view(shape)
    fa, fb = B._keep(ka, p, shape).to(device), B._keep(kb, p, shape).to(device)
    ds, wc = dv(case["ds"])[:, :, None], dv(case["wc"])
    g = ds * wc
    dza = g * (b * fb) * fa * (1 - a * a)
    dzb = g * (a * fa) * fb * (b * (1 - b))
    pab = ds * (a * fa) * (b * fb)
    sc = case["kind"] == "row_scaled"          # every parameter gradient contracts over the token rows
    R = B.DZ_ROUNDINGS
    # derived: a is an fp32 value here (bf16 in tests/_bf16_bounds.py, where a a is exact): a a < 1 rounds to within 2^-25, and where tanh
    # saturates 1 - a a is of that order itself -- an absolute error of 2^-25 |g b kb ka| in dza, whether or not the compiler fuses the
    # multiplication into the subtraction (both evaluations meet it; the CPU emulation is the unfused one)
    sat = 2.0 ** -25 * (g * (b * fb) * fa).abs()
    out = {"dba": (dza.sum(0),) + sum_bounds(dza.abs().sum(0), T, R, extra=sat.sum(0), scaled=sc),
           "dbb": (dzb.sum(0),) + sum_bounds(dzb.abs().sum(0), T, R, scaled=sc),
           "dwc": (pab.sum(0),) + sum_bounds(pab.abs().sum(0), T, 8, scaled=sc),
           "dbc": (ds.sum(0)[:, 0],) + sum_bounds(ds.abs().sum(0)[:, 0], T, scaled=sc)}
    s_dz, s_w = gate_dz_scale(case), gate_weight_scale(case)
    ea = R * U24 * dza.abs() + sat + torch.clamp(IMG_REL * (dza.abs() + sat), min=IMG_ABS / s_dz)     # the dz image the contractions read
    eb = R * U24 * dzb.abs() + torch.clamp(IMG_REL * dzb.abs(), min=IMG_ABS / s_dz)
    Wa, Wb = dv(case["Wa"]), dv(case["Wb"])
    if terms == 2:
        Wa, Wb = (dv(split_planes(case[k], s_w)[0]) / s_w for k in ("Wa", "Wb"))
        eWa = eWb = None
    else:
        eWa, eWb = image_bound(case["Wa"], s_w).to(device), image_bound(case["Wb"], s_w).to(device)
    mm = lambda x, w: torch.einsum("tcj,cjk->tck", x, w)       # noqa: E731
    dE, dE_mag = mm(dza, Wa) + mm(dzb, Wb), mm(dza.abs(), Wa.abs()) + mm(dzb.abs(), Wb.abs())
    extra = mm(ea, Wa.abs()) + mm(eb, Wb.abs())
    if terms == 3:
        extra = extra + mm(dza.abs(), eWa) + mm(dzb.abs(), eWb) + DROPPED * dE_mag
    dE, dE_mag, extra = (x.reshape(T, H * HID) for x in (dE, dE_mag, extra))
    if pool is not None:
        dE = dE + pool[0].to(device)
        extra = extra + pool[1].to(device) + U24 * dE.abs()
    if acc:
        dE = dE + dv(case["dE0"])
        extra = extra + U24 * dE.abs()
    out["dE"] = (dE,) + sum_bounds(dE_mag, terms * 2 * HID, extra=extra)
    E = dv(E_hi if terms == 2 else E_dec).view(shape)
    for name, dz, e in (("dWa", dza, ea), ("dWb", dzb, eb)):
        ref = torch.einsum("tcj,tck->cjk", dz, E)
        mag = torch.einsum("tcj,tck->cjk", dz.abs(), E.abs())
        extra = torch.einsum("tcj,tck->cjk", e, E.abs()) + (DROPPED * mag if terms == 3 else 0.0)
        out[name] = (ref,) + sum_bounds(mag, terms * T, extra=extra, scaled=sc)
    return {k: tuple(x.cpu() for x in v) for k, v in out.items()}


def gate_pool_term(scores, stat_m, stat_l, d_pooled, row_bag, H, what=""):
    """tests/_bf16_bounds.gate_pool_term with this file's measured ratio: (term fp64 [T, H*512], its slack); prints the case's own ratio."""
    def term(dt):
        rbag = row_bag.long()
        w = torch.exp(scores.to(dt) - stat_m.to(dt)[rbag]) * (1.0 / stat_l.to(dt)[rbag])
        return (w[:, :, None] * d_pooled.to(dt).view(-1, H, HID)[rbag]).reshape(scores.shape[0], H * HID)
    ref, emu = term(F64), term(torch.float32)
    ratio = measure_ratio(emu, ref, ref.abs())
    print("SPLITERR %spool term torch fp32 ratio of this case %.3f (constant %.2f, x %g allowed)" % (what, ratio, SOFTMAX_RATIO["pool term"],
                                                                                                  SOFTMAX_FACTOR))
    return (ref, SOFTMAX_FACTOR * SOFTMAX_RATIO["pool term"] * U24 * ref.abs()), ratio


def gate_pool_inputs(scores, lens):
    """(row_bag int32 [T], stat_m, stat_l [n_bags, H] fp32) of the given fp32 scores: the statistics the pooling forward would store."""
    row_bag = torch.repeat_interleave(torch.arange(len(lens)), torch.tensor(lens)).to(torch.int32)
    m = torch.stack([scores[row_bag == k].max(0).values for k in range(len(lens))])
    l_ = torch.stack([(scores[row_bag == k] - m[k]).double().exp().sum(0) for k in range(len(lens))]).float()
    return row_bag, m, l_


def emulate_gate_fwd(case, E_dec):
    """act_a, act_b, scores of the contract on the CPU (fp64 activations rounded to fp32, p = 0): the stand-in for the stored forward."""
    T, H = case["T"], case["H"]
    E = E_dec.double().view(T, H, HID)
    a = torch.tanh(torch.einsum("tck,cjk->tcj", E, case["Wa"].double()) + case["ba"].double()).float()
    b = torch.sigmoid(torch.einsum("tck,cjk->tcj", E, case["Wb"].double()) + case["bb"].double()).float()
    return a, b, ((a * b) * case["wc"]).sum(2) + case["bc"]


# ---------------------------------------------------------------------------------------------------------------- LayerNorm-GELU-Dropout
# The split LayerNorm entry points (csrc/preattn_act.hip) write y / row_mul dx as images whose scales come from bounds, not from a pass
# over the data (ln_bound_scale_kernel):
#   forward   bound = (max|gamma| sqrt(W - 1) + max|beta|) / (1 - p)
#   backward  bound = A 1.13 max|gamma| max|dy| / (1 - p) (2 + sqrt(W)),  A = max_r rstd[r] row_mul[r] (row_mul NULL: max rstd)
# in fp32; scale[1] holds the bound, scale[0] = sp_scale_for(scale[1]).  The bound is held to the fp64 formula within LN_BOUND_ULPS fp32
# roundings (derived: at most 6 operations, a fused multiply-add or not), the scale to the rule exactly.  The arithmetic is that of the
# fp32 kernels: the error propagation of tests/_bf16_bounds.ln_fwd_ref / ln_bwd_ref with the erfc GELU's tolerances and an fp32 store.
# taken from tests/test_activation_domain_gpu.py: the erfc GELU of fp32 storage, absolute on |t| <= 40, and GELU' through dbeta
GELU32_TOL, GELU32_GRAD_TOL = 8e-7, 5e-7
LN_BOUND_ULPS = 8


def ln_case(rows, W, seed, kind, p=0.0, group_lens=None):
    """tests/_bf16_bounds.ln_case (plain bias [W]) with full fp32 mantissas (one factor per column: the cancelling rows stay), a row_mul
    of powers of two with a zero (the row_inv of a row-scaled image with an all-zero row), and the group lengths of dgroup_bias."""
    from tests import _bf16_bounds as B
    case = B.ln_case(rows, W, seed, kind, p, None)
    g = torch.Generator().manual_seed(seed + 9)
    case["x"] = case["x"] * (0.75 + 0.25 * torch.rand(W, generator=g))
    case["dy"] = case["dy"] * (0.75 + 0.25 * torch.rand(W, generator=g))
    case["row_mul"] = torch.exp2(-torch.randint(0, 15, (rows,), generator=g).float())
    if rows >= 3:
        case["row_mul"][rows // 2] = 0.0
    case["group_lens"] = group_lens
    return case


def ln_fwd_bound(case, W):
    """The forward image bound in fp64."""
    inv = 1.0 / (1.0 - case["p"]) if case["p"] > 0 else 1.0
    return (float(case["gamma"].abs().max()) * math.sqrt(W - 1) + float(case["beta"].abs().max())) * inv


def ln_bwd_bound(case, W, rstd, row_mul):
    """The backward image bound in fp64 from the stored rstd."""
    inv = 1.0 / (1.0 - case["p"]) if case["p"] > 0 else 1.0
    a = float((rstd * row_mul).abs().max()) if row_mul is not None else float(rstd.max())
    return a * (1.13 * float(case["gamma"].abs().max()) * float(case["dy"].abs().max()) * inv) * (2.0 + math.sqrt(W))


def check_ln_scale(what, scale, want_bound, values):
    """scale = {s, bound}: the bound within LN_BOUND_ULPS roundings of the fp64 formula, s by sp_scale_for's rule from the stored bound
    (a power of two), every |value| <= bound, so that the scaled values stay below 2^15 (nothing is inf or NaN in the planes)."""
    s, bound = float(scale[0]), float(scale[1])
    assert abs(bound - want_bound) <= LN_BOUND_ULPS * U24 * want_bound, (what + "bound", bound, want_bound)
    assert s == scale_for(bound) and math.frexp(s)[0] == 0.5, (what + "scale", s, bound)
    top = float(values.abs().max()) if values.numel() else 0.0
    assert top <= bound and s * top < 2.0 ** 15, (what + "values above the bound", top, bound)


def ln_y_ref(case, mean, rstd):
    """y in fp64 from the STORED mean / rstd with the slack of the fp32 evaluation before the store: (ref, slack)."""
    from tests import _bf16_bounds as B
    x = case["x"].double()
    v = x + case["bias"].double()[None]
    mean, rstd = mean.double()[:, None], rstd.double()[:, None]
    h = (v - mean) * rstd
    dh = 3 * U24 * (v.abs() + mean.abs()) * rstd
    gam, beta = case["gamma"].double(), case["beta"].double()
    t = h * gam + beta
    dt = gam.abs() * dh + 2 * U24 * ((h * gam).abs() + beta.abs())
    kp = B._keep(case["keep"], case["p"], x.shape)
    ref = B.gelu64(t) * kp
    return ref, kp * (GELU32_TOL + B.GELU_SLOPE * dt) + 2 * U24 * ref.abs()


def ln_stats_ref(case):
    """mean, rstd against fp64 of x + bias: tests/_bf16_bounds.ln_fwd_ref's (it does not depend on the storage type)."""
    from tests import _bf16_bounds as B
    out = B.ln_fwd_ref(dict(case, groups=None))
    return out["mean"], out["rstd"]


def ln_bwd_ref(case, mean, rstd, row_mul=None):
    """The backward in fp64 from the STORED mean / rstd: name -> (ref, bound, proven ceiling or None) for dx (times row_mul where given;
    the value BEFORE the image: (ref, slack)), dgamma, dbeta, dbias and, with group_lens, dgroup_bias [G, W]."""
    from tests import _bf16_bounds as B
    x, dy = case["x"].double(), case["dy"].double()
    rows, W = x.shape
    gam, beta = case["gamma"].double(), case["beta"].double()
    mean, rstd = mean.double()[:, None], rstd.double()[:, None]
    v = x + case["bias"].double()[None]
    h = (v - mean) * rstd
    e_h = 3 * U24 * (v.abs() + mean.abs()) * rstd
    t = h * gam + beta
    e_t = gam.abs() * e_h + 2 * U24 * ((h * gam).abs() + beta.abs())
    kp = B._keep(case["keep"], case["p"], x.shape)
    dt = dy * kp * B.gelu_grad64(t)
    e_dt = dy.abs() * kp * (GELU32_GRAD_TOL + B.GELU_GRAD_SLOPE * e_t) + 3 * U24 * dt.abs()
    dh = dt * gam
    e_dh = e_dt * gam.abs() + U24 * dh.abs()
    m1, m2 = dh.mean(1, keepdim=True), (dh * h).mean(1, keepdim=True)
    e_m1 = e_dh.mean(1, keepdim=True) + SUM_TOL * dh.abs().mean(1, keepdim=True)
    e_m2 = (e_dh * h.abs() + dh.abs() * e_h).mean(1, keepdim=True) + (SUM_TOL + U24) * (dh * h).abs().mean(1, keepdim=True)
    dx = rstd * (dh - m1 - h * m2)
    e_dx = rstd * (e_dh + e_m1 + h.abs() * e_m2 + e_h * m2.abs()) + 4 * U24 * rstd * (dh.abs() + m1.abs() + (h * m2).abs())
    sc = case["kind"] == "row_scaled"
    out = {"dgamma": ((dt * h).sum(0),) + sum_bounds((dt * h).abs().sum(0), rows, 1, (e_dt * h.abs() + dt.abs() * e_h).sum(0), sc),
           "dbeta": (dt.sum(0),) + sum_bounds(dt.abs().sum(0), rows, 0, e_dt.sum(0), sc),
           "dbias": (dx.sum(0),) + sum_bounds(dx.abs().sum(0), rows, 0, e_dx.sum(0), sc)}
    if case["group_lens"] is not None:
        G = len(case["group_lens"])
        gid = torch.repeat_interleave(torch.arange(G), torch.tensor(case["group_lens"]))
        sel = torch.nn.functional.one_hot(gid, G).double().t()
        out["dgroup_bias"] = (sel @ dx,) + sum_bounds(sel @ dx.abs(), max(case["group_lens"] + [1]), 0, sel @ e_dx, sc)
    if row_mul is not None:           # the image holds row_mul[r] dx[r]: a power of two here, one rounding allowed for any other
        rm = row_mul.double()[:, None]
        dx, e_dx = dx * rm, e_dx * rm + U24 * (dx * rm).abs()
    out["dx"] = (dx, e_dx)
    return out


def check_ln_image(what, hi, lo, s, ref, slack, y32=None):
    """The decoded image against the fp64 reference: the slack of the fp32 value plus its rounding plus the image element bound of a
    value that large; and, where the fp32 value itself was stored (y32), within the element bound of it."""
    dec = decode(hi, lo, s)
    assert bool(torch.isfinite(hi.float()).all()) and bool(torch.isfinite(lo.float()).all()), what + ": inf / NaN in the planes"
    near = slack + U24 * ref.abs()
    check(what + "image", dec, ref, near + torch.clamp(IMG_REL * (ref.abs() + near), min=IMG_ABS / s))
    if y32 is not None:
        check(what + "image of the stored y", dec, y32.double(), image_bound(y32, s))
