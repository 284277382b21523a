"""The checkers of tests/_split_bounds.py, without a GPU: what tests/test_split_elements_gpu.py asserts of the split engine is asserted
here of a CPU emulation of the same contract, and of that emulation with one fault seeded.
  (a) The emulation -- torch.half planes, the three or two plane products in fp32 with 16 k per accumulate, the epilogue in the kernel's
      order -- passes every checker on the uniform, row_scaled and cancelling inputs and is bit-exact on the integer ones.  The worst
      ratios are printed (SPLITERR lines).
  (b) Ten seeded faults are each refused by a checker.  Beside each, what the criterion the suite had (rel_err < 1e-6, a Frobenius ratio
      over the whole output) says is recorded and asserted: faults 1, 2, 3, 5 and 6 pass it at these shapes.  test_fault_table prints it.
The fault operands: a [260, K] and b [260, K] with one power of two per row, the four rows of the ragged last 256-tile (256 .. 259) at
2^-10, 2^-11, 2^-12, 2^-12 of the largest rows -- the place where a norm cannot see."""
import pytest
import torch

from tests import _split_bounds as S

M, N, K = 260, 260, 128
TABLE = {}


def _images(x, rows):
    """(hi, lo, common scale, row_inv or None) of the plain or the row-scaled image of x."""
    if rows:
        hi, lo, _, inv = S.image_rows(x)
        return hi, lo, 1.0, inv
    return S.image(x) + (None,)


def _nt(case, a_rows, b_rows, terms, opts):
    """Planes and epilogue arguments of an NT case -> (kwargs for nt_ref / emulate_nt)."""
    ah, al, sa, arm = _images(case["a"], a_rows)
    bh, bl, sb, bcm = _images(case["b"], b_rows)
    kw = dict(inv=1.0 / (sa * sb), terms=terms, a_row_mul=arm, b_col_mul=bcm)
    if "bias" in opts:
        kw["bias"] = case["bias"]
    if "group" in opts:
        kw["gb_rows"] = case["gb"][case["row_group"].long()]
    if "acc" in opts:
        kw["c0"] = case["c0"]
    return (ah, al, bh, bl), kw


# ------------------------------------------------------------------------------------------------------------------ (a) the emulation passes
@pytest.mark.parametrize("rows", [0, 1], ids=["common", "rowscaled"])
@pytest.mark.parametrize("kind", S.KINDS)
def test_emulated_image_meets_the_element_bound(kind, rows):
    x = S.operand((33, 544), 5, kind)
    x[7] = 0.0
    if rows:
        hi, lo, s, inv = S.image_rows(x)
        S.check_row_inv("image_rows[%s]." % kind, inv, x)
        assert float(inv[7]) == 0.0 and float(hi[7].abs().max()) == 0.0
    else:
        hi, lo, s = S.image(x)
        S.check_scale("image[%s]." % kind, s, x.abs().max(), x)
    S.check_image("image[%s,%s]." % (kind, "rows" if rows else "common"), hi, lo, x, s)
    h2, l2 = S.unpack(S.pack(hi, lo, 4 * 544 + 16), 544)
    assert torch.equal(h2, hi) and torch.equal(l2, lo)


def test_image_bound_is_tight():
    """Rows spread over 30 binades: the worst |dec - x| / bound of the definition is exactly 1 -- the bound is met and cannot be lowered."""
    x = S.uniform((31, 4096), 9) * torch.exp2(-torch.arange(31.0))[:, None]
    hi, lo, s = S.image(x)
    r, _ = S.worst_ratio(S.decode(hi, lo, s), x.double(), S.image_bound(x, s))
    print("SPLITERR image definition over 30 binades: worst ratio %.6f" % r)
    assert r == 1.0


@pytest.mark.parametrize("terms", [3, 2])
@pytest.mark.parametrize("a_rows,b_rows,opts", [(0, 0, ()), (1, 1, ("bias", "acc")), (1, 0, ("bias", "group")), (0, 1, ("acc",))],
                         ids=["plain", "rows_bias_acc", "arows_group", "brows_acc"])
@pytest.mark.parametrize("kind", S.KINDS4)
def test_emulated_nt_passes(kind, a_rows, b_rows, opts, terms):
    case = S.nt_case(M, N, 96, 11, kind)
    planes, kw = _nt(case, a_rows, b_rows, terms, opts)
    got, (ref, b1, b2) = S.emulate_nt(*planes, **kw), S.nt_ref(*planes, **kw)
    what = "emu nt[%s,%s,terms%d]." % (kind, "+".join(opts) or "plain", terms)
    if kind == "integer":
        S.check_exact(what, got, ref)
    else:
        S.check(what, got, ref, b1, b2)


@pytest.mark.parametrize("terms", [3, 2])
@pytest.mark.parametrize("kind", S.KINDS4)
def test_emulated_tn_passes(kind, terms):
    case = S.tn_case(97, 288, 32, 21, kind)
    ah, al, sa = S.image(case["x"])
    bh, bl, sb = S.image(case["dy"])
    got = S.emulate_tn(ah, al, bh, bl, 1.0 / (sa * sb), terms)
    ref, b1, b2 = S.tn_ref(ah, al, bh, bl, 1.0 / (sa * sb), terms, scaled=kind == "row_scaled")
    if kind == "integer":
        S.check_exact("emu tn[integer,terms%d]" % terms, got, ref)
    else:
        S.check("emu tn[%s,terms%d]" % (kind, terms), got, ref, b1, b2)


def test_integer_products_are_exact_at_K_2048():
    """Operands of [-7, 7]: lo == 0, scale 2^11, every partial sum below 2^24 (49 * 2048 < 2^24): exact in any summation order."""
    case = S.nt_case(33, 36, 2048, 31, "integer")
    planes, kw = _nt(case, 0, 0, 3, ("bias", "acc"))
    assert float(planes[1].abs().max()) == 0.0 and float(planes[3].abs().max()) == 0.0
    S.check_exact("integer K=2048", S.emulate_nt(*planes, **kw), S.nt_ref(*planes, **kw)[0])
    assert torch.equal(S.nt_ref(*planes, **kw)[0], case["a"].double() @ case["b"].double().t() + case["bias"].double() + case["c0"].double())


# -------------------------------------------------------------------------------------------------------------------- (b) the seeded faults
def _tail_scaled(rows, cols, seed, scale=1.0):
    """uniform x 2^e per row: e = 12 - (r % 25) on the first 256 rows, -10, -11, -12, -12 on rows 256 .. 259."""
    assert rows == 260
    e = torch.cat([12.0 - (torch.arange(256) % 25), torch.tensor([-10.0, -11.0, -12.0, -12.0])])
    return S.uniform((rows, cols), seed, scale) * torch.exp2(e)[:, None]


def _fault_nt():
    """The row-scaled fault case on row-scaled images with bias and accumulate: (case, planes, kwargs, emulation, reference triple)."""
    case = S.nt_case(M, N, K, 41, "uniform")
    case["a"], case["b"] = _tail_scaled(M, K, 42), _tail_scaled(N, K, 43, K ** -0.5)
    case["c0"] = case["c0"] * 2.0 ** -30            # (the starting contents small everywhere: the tail tile's own values stay visible)
    case["bias"] = case["bias"] * 2.0 ** -30
    planes, kw = _nt(case, 1, 1, 3, ("bias", "acc"))
    return case, planes, kw, S.emulate_nt(*planes, **kw), S.nt_ref(*planes, **kw)


def _record(n, name, got, ref3, norm_must_pass=None):
    """One row of the fault table: the per-element checker must refuse `got`; what the norm criterion says is recorded (and asserted for
    the faults the issue names)."""
    refused = not S.passes(got, *ref3)
    norm = S.rel_err(got, ref3[0])
    TABLE[n] = "%-2s %-62s checker %s   norm %.2e -> %s" % (n, name, "refuses" if refused else "PASSES", norm,
                                                          "passes" if norm < S.OLD_NORM_TOL else "refuses")
    assert refused, TABLE[n]
    if norm_must_pass is not None:
        assert (norm < S.OLD_NORM_TOL) == norm_must_pass, TABLE[n]


def test_the_unfaulted_emulation_passes_both_criteria():
    _, _, _, emu, ref3 = _fault_nt()
    assert S.passes(emu, *ref3) and S.rel_err(emu, ref3[0]) < S.OLD_NORM_TOL
    S.check("emu nt[fault case]", emu, *ref3)


def test_fault_01_row_from_its_neighbour():
    _, _, _, emu, ref3 = _fault_nt()
    got = emu.clone()
    got[M - 1] = emu[M - 2]
    _record("1", "output row 259 taken from row 258", got, ref3, True)


def test_fault_02_k_block_dropped():
    _, planes, kw, _, ref3 = _fault_nt()
    _record("2", "32-k block 1 dropped in the ragged row tile (rows 256 ..)", S.emulate_nt(*planes, skip_block=(1, slice(256, M)), **kw), ref3,
            True)
    _record("2g", "32-k block 1 dropped in every row", S.emulate_nt(*planes, skip_block=(1, slice(0, M)), **kw), ref3, False)


def _fault_tn():
    """x [T, 288], dy [T, 288] whose token rows decay as logspace(0, -3, T); the columns past 256 of both (the ragged corner tile of the
    output) are 2^-12 of the others."""
    T = 97
    case = S.tn_case(T, 288, 288, 51, "uniform")
    decay = torch.logspace(0, -3, T)[:, None]
    col = torch.cat([torch.ones(256), torch.full((32,), 2.0 ** -12)])
    case["x"], case["dy"] = case["x"] * col, case["dy"] * decay * col
    ah, al, sa = S.image(case["x"])
    bh, bl, sb = S.image(case["dy"])
    return (ah, al, bh, bl), 1.0 / (sa * sb)


def test_fault_03_token_chunk_dropped():
    planes, inv = _fault_tn()
    ref3 = S.tn_ref(*planes, inv)
    emu = S.emulate_tn(*planes, inv)
    assert S.passes(emu, *ref3) and S.rel_err(emu, ref3[0]) < S.OLD_NORM_TOL
    S.check("emu tn[decaying rows]", emu, *ref3)
    corner = (slice(256, 288), slice(256, 288))
    _record("3", "last 32-token chunk dropped in the ragged corner tile, rows decaying", S.emulate_tn(*planes, inv, skip_chunk=(2,) + corner),
            ref3, True)
    everywhere = (slice(0, 288), slice(0, 288))
    _record("3g", "last 32-token chunk dropped in every tile, rows decaying", S.emulate_tn(*planes, inv, skip_chunk=(2,) + everywhere), ref3,
            False)


def test_fault_04_three_terms_served_by_two():
    _, planes, kw, emu, ref3 = _fault_nt()
    ah, al, bh, bl = planes
    f = kw["inv"] * kw["a_row_mul"][:, None] * kw["b_col_mul"][None, :]
    _record("4", "al bh omitted everywhere", emu - (al.float() @ bh.float().t()) * f, ref3)


def test_fault_05_b_col_mul_one_column_off():
    _, planes, kw, _, ref3 = _fault_nt()
    bcm = kw["b_col_mul"].clone()
    bcm[257:] = kw["b_col_mul"][256:-1]
    _record("5", "b_col_mul[n - 1] on the last ragged column tile", S.emulate_nt(*planes, **dict(kw, b_col_mul=bcm)), ref3, True)


def test_fault_06_a_row_mul_of_the_last_row():
    _, planes, kw, _, ref3 = _fault_nt()
    arm = kw["a_row_mul"].clone()
    arm[256:] = arm[M - 1]
    _record("6", "a_row_mul of the ragged row tile read from row M - 1", S.emulate_nt(*planes, **dict(kw, a_row_mul=arm)), ref3, True)


def test_fault_07_bias_added_twice():
    case = S.nt_case(M, N, K, 44, "uniform")
    planes, kw = _nt(case, 0, 0, 3, ("bias", "acc"))
    _record("7", "bias added twice on the accumulate path", S.emulate_nt(*planes, **kw) + case["bias"], S.nt_ref(*planes, **kw))


def _image_passes(hi, lo, x, s):
    try:
        S.check_image("", hi, lo, x, s)
    except AssertionError:
        return False
    return True


def _record_image(n, name, hi, lo, x, s, refused):
    norm = S.rel_err(S.decode(hi, lo, s), x)
    TABLE[n] = "%-2s %-62s checker %s   norm %.2e -> %s" % (n, name, "refuses" if refused else "PASSES", norm,
                                                          "passes" if norm < S.OLD_NORM_TOL else "refuses")
    assert refused, TABLE[n]


def test_fault_08_lo_plane_truncated():
    x = S.uniform((33, 512), 61)
    s = S.scale_for(x.abs().max())
    assert _image_passes(*S.split_planes(x, s), x, s)
    hi, lo = S.split_planes(x, s, truncate_lo=True)
    _record_image("8", "lo plane cut toward zero instead of rounded", hi, lo, x, s, not _image_passes(hi, lo, x, s))


def _scale_passes(s, x):
    try:
        S.check_scale("", s, x.abs().max(), x)
    except AssertionError:
        return False
    return True


def test_fault_09_scale_off_by_a_binade():
    """One binade too large leaves the scaled maximum below 2^15 -- finite in fp16 (65504), and no less accurate: only the exact scale
    rule refuses it.  Three binades too large overflow to inf, which the plane check refuses; one too small costs the small elements a
    bit and is refused by the rule and, at those elements, by the bound of the documented scale."""
    x = S.uniform((33, 512), 62) * torch.logspace(0, -6, 512)
    s = S.scale_for(x.abs().max())
    assert _scale_passes(s, x)
    for n, name, f in (("9a", "image scale one binade too large", 2.0), ("9b", "image scale three binades too large (inf)", 8.0),
                       ("9c", "image scale one binade too small", 0.5)):
        hi, lo = S.split_planes(x, s * f)
        if f == 8.0:
            assert not bool(torch.isfinite(hi.float()).all()) and not _image_passes(hi, lo, x, s * f)
        if f == 0.5:
            assert S.worst_ratio(S.decode(hi, lo, s * f), x.double(), S.image_bound(x, s))[0] > 1.0
        _record_image(n, name, hi, lo, x, s * f, not _scale_passes(s * f, x))


def test_fault_10_zero_row_with_unit_row_inv():
    """No product shows this fault (the row's image is zero); as row_mul of the paired gradient image it would let a row that
    contributes nothing set that image's scale.  The row_inv rule refuses it."""
    x = S.uniform((33, 512), 63)
    x[5] = 0.0
    hi, lo, s, inv = S.image_rows(x)
    S.check_row_inv("", inv, x)
    bad = inv.clone()
    bad[5] = 1.0
    with pytest.raises(AssertionError):
        S.check_row_inv("", bad, x)
    _record_image("10", "zero row given row_inv = 1", hi, lo, x, s, True)


def test_fault_table():
    """Prints the table the other tests of this section fill (and fills it itself when run alone)."""
    want = ["1", "2", "2g", "3", "3g", "4", "5", "6", "7", "8", "9a", "9b", "9c", "10"]
    if sorted(TABLE) != sorted(want):
        for fn in (test_fault_01_row_from_its_neighbour, test_fault_02_k_block_dropped, test_fault_03_token_chunk_dropped,
                   test_fault_04_three_terms_served_by_two, test_fault_05_b_col_mul_one_column_off, test_fault_06_a_row_mul_of_the_last_row,
                   test_fault_07_bias_added_twice, test_fault_08_lo_plane_truncated, test_fault_09_scale_off_by_a_binade,
                   test_fault_10_zero_row_with_unit_row_inv):
            fn()
    assert sorted(TABLE) == sorted(want), sorted(TABLE)
    for n in want:
        print("SPLITFAULT " + TABLE[n])
    for n in ("1", "2", "3", "5", "6"):
        assert TABLE[n].endswith("passes") and "checker refuses" in TABLE[n], TABLE[n]


# ------------------------------------------------------------------------------------------------------ (c) the measured softmax constants
def test_softmax_ratios_are_the_measured_ones():
    """SOFTMAX_RATIO of tests/_split_bounds.py is the worst torch-fp32 ratio over the GPU file's own pooling cases, measured here on the
    CPU reference (the image by the definition, which the kernels' images equal bit for bit; the stored forward = the fp32 evaluation)."""
    from tests import _bf16_bounds as B
    worst = {}
    for lens, dense in S.POOL_BAGS:
        for H in S.POOL_HEADS:
            for kind in S.KINDS:
                case = S.pool_img_case(lens, H, kind)
                hi, lo, s = S.image(case["E32"])
                case["E"] = S.decode(hi, lo, s)
                fwd = B.pool_fwd_ref(case, False, torch.float32)
                _, ratios = S.pool_img_bounds(case, dict(pooled=fwd["pooled"], m=fwd["m"], l=fwd["l"]))
                for k, v in ratios.items():
                    if v > worst.get(k, (0.0,))[0]:
                        worst[k] = (v, "%s, H = %d, %s" % ("dense" if dense else "ragged", H, kind))
    for k, (v, where) in sorted(worst.items()):
        print("SPLITERR softmax ratio %-9s measured %.3f (%s), constant %.2f" % (k, v, where, S.SOFTMAX_RATIO[k]))
    for k, (v, where) in sorted(worst.items()):
        assert v <= S.SOFTMAX_RATIO[k] <= 1.01 * v + 0.01, (k, v, where)


GATE_POOL_LENS = (70, 59)


def test_pool_term_ratio_is_the_measured_one():
    """SOFTMAX_RATIO['pool term']: the weight exp(s - m) / l times d_pooled of the fused gate backward, over the GPU file's cases (the
    scores and statistics from the CPU stand-in of the stored forward)."""
    worst = (0.0, "")
    for H in (1, 4):
        for kind in S.KINDS:
            case = S.gate_case(sum(GATE_POOL_LENS), H, 4500 + H, kind, 0.25)
            hi, lo, s = S.image(case["E32"])
            scores = S.emulate_gate_fwd(case, S.decode(hi, lo, s))[2]
            row_bag, m, l_ = S.gate_pool_inputs(scores, GATE_POOL_LENS)
            dp = S.operand((2, H * S.HID), 4600 + H, kind)
            _, ratio = S.gate_pool_term(scores, m, l_, dp, row_bag, H)
            worst = max(worst, (ratio, "H = %d, %s" % (H, kind)))
    print("SPLITERR softmax ratio pool term measured %.3f (%s), constant %.2f" % (worst + (S.SOFTMAX_RATIO["pool term"],)))
    assert worst[0] <= S.SOFTMAX_RATIO["pool term"] <= 1.01 * worst[0] + 0.01, worst


@pytest.mark.parametrize("terms", [3, 2])
@pytest.mark.parametrize("kind", S.KINDS)
def test_emulated_gate_passes(kind, terms):
    """The gate's contract on the CPU: the weights' and dz's images by the definition at the documented scales, decoded and contracted
    in fp32, against the fp64 references with the modelled image errors."""
    T, H = 45, 2
    case = S.gate_case(T, H, 71, kind)
    hi, lo, s_e = S.image(case["E32"])
    E_dec, E_hi = S.decode(hi, lo, s_e), hi.double() / s_e
    a, b, scores = S.emulate_gate_fwd(case, E_dec)
    fwd = S.gate_fwd_ref(case, E_dec)
    s_w, s_dz = S.gate_weight_scale(case), S.gate_dz_scale(case)
    img = lambda x, s: S.decode(*S.split_planes(x, s), s).float()        # noqa: E731
    hi_only = lambda x, s: (S.split_planes(x, s)[0].double() / s).float()        # noqa: E731
    Wa_i, Wb_i = ((hi_only if terms == 2 else img)(case[k], s_w) for k in ("Wa", "Wb"))
    za = torch.einsum("tck,cjk->tcj", E_dec.float().view(T, H, S.HID), img(case["Wa"], s_w)) + case["ba"]
    zb = torch.einsum("tck,cjk->tcj", E_dec.float().view(T, H, S.HID), img(case["Wb"], s_w)) + case["bb"]
    S.check("emu gate[%s].act_a" % kind, torch.tanh(za.double()).float(), *fwd["act_a"])
    S.check("emu gate[%s].act_b" % kind, torch.sigmoid(zb.double()).float(), *fwd["act_b"])
    ds = case["ds"][:, :, None]
    g = ds * case["wc"]
    dza32, dzb32 = g * b * (1 - a * a), g * a * (b * (1 - b))          # (1 - a a unfused: the evaluation with the larger error)
    dza, dzb = img(dza32, s_dz), img(dzb32, s_dz)
    Ee = (E_hi if terms == 2 else E_dec).float().view(T, H, S.HID)
    got = dict(dE=(torch.einsum("tcj,cjk->tck", dza, Wa_i) + torch.einsum("tcj,cjk->tck", dzb, Wb_i)).reshape(T, H * S.HID) + case["dE0"],
               dWa=torch.einsum("tcj,tck->cjk", dza, Ee), dWb=torch.einsum("tcj,tck->cjk", dzb, Ee), dba=dza32.sum(0), dbb=dzb32.sum(0),
               dwc=(ds * a * b).sum(0), dbc=case["ds"].sum(0))
    for k, v in S.gate_bwd_ref(case, E_dec, E_hi, a, b, None, None, 1, terms).items():
        S.check("emu gate[%s,terms%d].%s" % (kind, terms, k), got[k].reshape(v[0].shape), *v)


@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("p", [0.0, 0.25])
def test_emulated_layernorm_images_pass(kind, p):
    """The LayerNorm contract on the CPU in fp32 (erf GELU, inside the erfc form's tolerance), y and row_mul dx written as images at the
    scales of the documented bounds."""
    from tests import _bf16_bounds as B
    rows, W = 77, 256
    case = S.ln_case(rows, W, 81, kind, p, [30, 1, 46])
    x, dy, gam, beta = case["x"], case["dy"], case["gamma"], case["beta"]
    v = x + case["bias"]
    mean = v.mean(1)
    c = v - mean[:, None]
    rstd = ((c * c).mean(1) + case["eps"]).rsqrt()
    st = S.ln_stats_ref(case)
    S.check("emu ln[%s].mean" % kind, mean, *st[0])
    S.check("emu ln[%s].rstd" % kind, rstd, *st[1])
    h = c * rstd[:, None]
    t = h * gam + beta
    kp = B._keep(case["keep"], p, x.shape).float()
    y = B.gelu64(t.double()).float() * kp
    s = S.scale_for(S.ln_fwd_bound(case, W))
    S.check_ln_scale("emu ln.fwd.", (s, S.ln_fwd_bound(case, W)), S.ln_fwd_bound(case, W), y)
    S.check_ln_image("emu ln[%s,p%g].y." % (kind, p), *S.split_planes(y, s), s, *S.ln_y_ref(case, mean, rstd), y32=y)
    dt = dy * kp * B.gelu_grad64(t.double()).float()
    dh = dt * gam
    m1, m2 = dh.mean(1, keepdim=True), (dh * h).mean(1, keepdim=True)
    dx = rstd[:, None] * (dh - m1 - h * m2)
    gid = torch.repeat_interleave(torch.arange(3), torch.tensor(case["group_lens"]))
    got = dict(dgamma=(dt * h).sum(0), dbeta=dt.sum(0), dbias=dx.sum(0), dgroup_bias=torch.nn.functional.one_hot(gid, 3).float().t() @ dx)
    for rm in (None, case["row_mul"]):
        ref = S.ln_bwd_ref(case, mean, rstd, rm)
        for k in got:
            S.check("emu ln[%s,p%g].%s" % (kind, p, k), got[k], *ref[k])
        bound = S.ln_bwd_bound(case, W, rstd, rm)
        img = dx if rm is None else dx * rm[:, None]
        s = S.scale_for(bound)
        S.check_ln_scale("emu ln.bwd.", (s, bound), bound, img)
        S.check_ln_image("emu ln[%s,p%g,row_mul %s].dx." % (kind, p, rm is not None), *S.split_planes(img, s), s, *ref["dx"])
