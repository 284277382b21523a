"""fp64 references and per-element error bounds of the InfoNCE kernels (csrc/infonce.hip: the staged kernels, the opt-in fused kernels and the
explicit-negative kernels, paired and unpaired), for tests/test_nce_elements_gpu.py (the kernels) and tests/test_nce_bounds_cpu.py (these
checkers, against a CPU emulation and seeded faults).

The contract, read from csrc/infonce.hip.  Inputs are fp32 and go to both sides as they are.
  - x^ = x * (1 / max(sqrt(ss), 1e-12)), ss an fp32 fmaf chain over the row (nce_row_ss, nce_inv_norm);
  - logits z = (exact-fp32 MFMA sum of x^ y^ products) * (1 / T);
  - (m, l) = (max, log sum exp(z - m)) per row (and per column for the symmetric loss), kept apart;
  - row loss = l - (z_target - m); the loss of a problem is the mean of its rows;
  - the coefficient forms (softmax - delta) first, then scales by the loss weights, the upstream gradient and 1 / T;
  - dX^ = coefficients times normalised rows on the fp32 MFMA;
  - normalize() backward: dX = rn (dX^ - x^ <x^, dX^>), the dot dropped on a clamped row (rn >= 0.99e12);
  - explicit negatives: the same over the columns {positive} u [0, M); <N^_j, dN^_j> is taken as T sum_i C_ij Z_ij from the logits;
  - every merge (LSE chunks of 4096, dQ^ splits of 1024, paired chunks of 64) in a fixed order, no atomics.
The reference is fp64 of the documented operation on the same fp32 inputs, never another kernel and never workspace contents: only loss,
row_loss, dQ, dP and dNeg are looked at.  Gradients are written out here (the formulas torch autograd gives, which the CPU file asserts)
with one change: on the target column 1 - p is formed as the sum of the other probabilities, so that a saturated row's reference is not
itself rounding noise.

The bounds, per element, in fp64 beside the reference, u = 2^-24 (`proven` swaps SUM_TOL for gamma(D): the second assertion):
  nu      = SUM_TOL / 2 + NORM_R / 2 u: the relative error of a normalised row and of its inverse norm;
  Delta   = (1 / T) (SUM_TOL + 2 nu) sum_d |q^ p^| + SCALE_R u |z|: the slack of a logit;
  p_ij    : |error| <= s_ij = p_ij ((1 - p_ij) (exp(Delta_ij + max_k Delta_ik) - 1) + LSE_FACTOR LSE_R u (1 + |z_ij - m| + |l|)), the
            first term EXACT in the logit perturbation (derivation in DESIGN.md 4.4), the second the fp32 evaluation, measured;
  row loss: (1 - p_it) (exp(Delta_it + max_k Delta_ik) - 1) + LSE_FACTOR LSE_R u (1 + |l| + |z_it - m|); a row of ONE logit has bound 0;
  loss    : the mean of the row bounds + (gamma(k) + u) mean |row loss|;
  G_ij    : (1 / T) (w0 |g_i| s0_ij + w1 |g_j| s1_ij) + COEF_R u |terms of G_ij|;
  dX^     : sigma |Y^| + (gamma(n) + nu + u) |G| |Y^|, n the number of addends;
  dX      : rn (e + |x^| sum |x^| e) + (gamma(D) + 3 nu + 5 u) rn (|dX^| + |x^| sum |x^ dX^|); clamped: rn e + (nu + 2 u) rn |dX^|;
  dNeg    : the same with the dot's slack T sum_i (sigma_ij |z_ij| + |C_ij| Delta_ij) + (gamma(N) + 3 u) T sum_i |C_ij z_ij|.
A zero bound means exact.  Constants: which are derived, taken from other tests or measured is said beside each."""
import torch

from oracle import recipe
from tests._bf16_bounds import SUM_TOL, gamma, passes, rel_err, worst_ratio  # noqa: F401  (SUM_TOL: taken from tests/_bf16_bounds.py)

F64 = torch.float64
U = 2.0 ** -24
NAN = float("nan")
# the merge sizes of csrc/infonce.hip (the issue's statement of them; asserted against mdl_dispatch_plan in the GPU file)
NEG_LSE_CH, NEG_KCH, NEG_PCH = 4096, 1024, 64
# derived: per normalisation sqrtf (within 1 ulp = 2 u), the reciprocal (2 u; the fp32 value of 1e-12f on a clamped row is inside it) and
# the scaling x * inv (u): 5 u on x^, two rows per logit: 10; 12 with margin.  The sum of squares is charged apart (SUM_TOL / 2 per row).
NORM_R = 12
# derived: 1 / T in fp32, the product of the column scale with it (negatives: r * inv_T) and the final multiplication
SCALE_R = 3
# derived: the subtraction of delta (exact for p >= 1/2, one rounding below), the weights, g, 1 / T (itself rounded) and, in the mean
# form, d_loss / k: at most 6 roundings on either term of G
COEF_R = 6
# measured: the worst |error| / (u (1 + |l| + |z - m|)) of torch fp32 log_softmax on the CPU over the fp32-rounded reference logits,
# against fp64 of the same rounded logits, over every case of tests/test_nce_elements_gpu.py (rows, and columns where symmetric):
# tests/test_nce_bounds_cpu.py::test_lse_constant_covers_every_case measures it again.  The worst case is named there and in DESIGN.md.
LSE_R = 5.16        # measured 5.151: in-batch, Kmax = 257, D = 64, T = 0.07, degenerate, problem 0, the row direction
# the project's margin on a measured softmax figure (tests/_bf16_bounds.py SOFTMAX_FACTOR): device exp / log, another summation order
LSE_FACTOR = 4.0

FAMILIES = ("uniform", "row_scaled", "clustered", "degenerate")


def check(what, got, ref, bound, second=None):
    """Asserts |got - ref| <= bound at every element (and <= second, the gamma ceiling); prints NCEERR <what> <worst ratio>."""
    assert tuple(got.shape) == tuple(ref.shape), (what, tuple(got.shape), tuple(ref.shape))
    r, i = worst_ratio(got, ref, bound)
    print("NCEERR %s worst |err| / bound = %.3f at flat index %d of %s" % (what, r, i, tuple(ref.shape)))
    assert r <= 1.0, (what, r, i)
    if second is not None:
        r2, i2 = worst_ratio(got, ref, second)
        assert r2 <= 1.0, (what + " (gamma ceiling)", r2, i2)
    return r


# -------------------------------------------------------------------------------------------------------------------------------- inputs
def _t(shape, key, lo=-1.0, hi=1.0):
    return torch.from_numpy(recipe.uniform(shape, key, lo, hi))


def _scales(rows, key):
    """2^e per row, e an integer of [-12, 12]."""
    return torch.exp2(torch.floor(_t((rows,), key, -12.0, 13.0)).clamp(-12, 12))[:, None]


def _tiny(row):
    """The row at norm 1e-13: below the clamp of normalize()."""
    return (row.double() / row.double().norm() * 1e-13).float()


def family_rows(k, D, family, key, neg_shape=None):
    """(q [k, D], p [k, D], neg of neg_shape or None) of an input family, a pure function of the key."""
    q, p = _t((k, D), key + ":q"), _t((k, D), key + ":p")
    neg = _t(neg_shape, key + ":n") if neg_shape is not None else None
    if family == "clustered":
        c = _t((D,), key + ":c")
        q = c + 0.05 * q
        p = c + 0.05 * p + 0.5 * (q - c)
        neg = c + 0.05 * neg if neg is not None else None
        return q, p, neg
    p = p + 0.1 * q
    if family == "row_scaled":
        q, p = q * _scales(k, key + ":eq"), p * _scales(k, key + ":ep")
        if neg is not None:
            neg = (neg.reshape(-1, D) * _scales(neg.numel() // D, key + ":en")).reshape(neg_shape)
    if family == "degenerate":
        # all present together from k = 8 on; fewer rows keep those that fit
        edits = ((0, lambda: q.__setitem__(0, 0.0)),                       # an all-zero row of Q
                 (1, lambda: p.__setitem__(1, _tiny(p[1]))),               # a clamped row of P (norm 1e-13)
                 (3, lambda: q.__setitem__(3, q[2])),                      # two identical rows in Q
                 (4, lambda: p.__setitem__(4, q[4])),                      # p_i = q_i
                 (5, lambda: p.__setitem__(5, -q[5])),                     # p_j = -q_j
                 (6, lambda: p.__setitem__(6, 0.0)),                       # an all-zero row of P
                 (7, lambda: q.__setitem__(7, _tiny(q[7]))))               # a clamped row of Q
        for row, edit in edits:
            if row < k:
                edit()
        if neg is not None and neg.shape[-2] >= 4:
            neg[..., 0, :] = 0.0
            neg[..., 1, :] = (neg[..., 1, :].double() / neg[..., 1, :].double().norm(dim=-1, keepdim=True) * 1e-13).float()
            neg[..., 2, :] = q[min(2, k - 1)] if neg.dim() == 2 else q       # a negative equal to a query
    return q, p, neg


def mid_count(Kmax):
    """About Kmax / 2 and not a multiple of 32."""
    h = Kmax // 2
    return min(Kmax, h + 1 if h % 32 == 0 else h)


def inbatch_case(cnt, Kmax, D, T, sym, family, form, tag=""):
    """Q, P [S, Kmax, D] with NaN in the rows >= cnt[s]; form 'd_loss' (g [S]) or 'd_row_loss' (g [S, Kmax], NaN in the padding)."""
    S = len(cnt)
    key = "nceb:%s:%d:%d:%g:%d:%s:%s:%s" % (tag, Kmax, D, T, sym, family, form, ",".join(map(str, cnt)))
    Q, P = torch.full((S, Kmax, D), NAN), torch.full((S, Kmax, D), NAN)
    for s, k in enumerate(cnt):
        q, p, _ = family_rows(k, D, family, "%s:s%d" % (key, s))
        Q[s, :k], P[s, :k] = q, p
    if form == "d_loss":
        g = _t((S,), key + ":g", 0.5, 2.0) * torch.tensor([1.0, -1.0, 1.0] * S)[:S]
    else:
        g = torch.full((S, Kmax), NAN)
        for s, k in enumerate(cnt):
            g[s, :k] = _t((k,), "%s:g%d" % (key, s), -1.5, 1.5)
    return dict(Q=Q.float(), P=P.float(), cnt=list(cnt), Kmax=Kmax, D=D, T=T, sym=int(sym), family=family, form=form, g=g.float())


def neg_case(N, M, D, T, paired, family, form, tag=""):
    """Q, P [N, D], Neg [M, D] or [N, M, D]; form 'd_loss' (g [1]) or 'd_row_loss' (g [N])."""
    key = "ncen:%s:%d:%d:%d:%g:%d:%s:%s" % (tag, N, M, D, T, paired, family, form)
    q, p, neg = family_rows(N, D, family, key, (N, M, D) if paired else (M, D))
    g = _t((1,), key + ":g", 0.5, 2.0) * -1.0 if form == "d_loss" else _t((N,), key + ":g", -1.5, 1.5)
    return dict(Q=q.float(), P=p.float(), Neg=neg.float(), N=N, M=M, D=D, T=T, paired=int(paired), family=family, form=form, g=g.float())


def t32(T):
    """The temperature the kernels see: the C float of the Python number."""
    return float(torch.tensor(T, dtype=torch.float32))


# --------------------------------------------------------------------------------------------------------------------- shared derivations
def _nu(D, proven):
    return 0.5 * (gamma(D) if proven else SUM_TOL) + 0.5 * NORM_R * U


def _sum_tol(D, proven):
    return gamma(D) if proven else SUM_TOL


def normalize64(x):
    """x^, 1 / max(|x|, 1e-12), and which rows are clamped, in fp64 (F.normalize)."""
    x = x.double()
    n = (x * x).sum(-1).sqrt()
    rn = 1.0 / n.clamp_min(1e-12)
    return x * rn[..., None], rn, n < 1e-12


def logit_slack(z, mag, T, D, proven):
    return (1.0 / T) * (_sum_tol(D, proven) + 2 * _nu(D, proven)) * mag + SCALE_R * U * z.abs()


def direction(z, dl, tgt):
    """The softmax of every row of z [R, C] against the target column tgt [R], with the slack dl of the logits.  Returns the row losses
    and their bounds, pm = p - delta (the target column as -(sum of the others)), and s = the bound of |error of p|."""
    R, C = z.shape
    rows = torch.arange(R)
    m = z.max(1, keepdim=True).values
    l_ = torch.log(torch.exp(z - m).sum(1, keepdim=True))
    lsm = (z - m) - l_
    p = torch.exp(lsm)
    top = p.argmax(1)
    rest = p.clone()
    rest[rows, top] = 0.0
    omp = 1.0 - p
    omp[rows, top] = rest.sum(1)                       # 1 - p where p may be near 1: the sum of the others
    fp32 = LSE_FACTOR * LSE_R * U * (1.0 + (z - m).abs() + l_.abs()) if C > 1 else torch.zeros_like(z)   # one logit: l = log(exp(0)) = 0
    rel = omp * torch.expm1(dl + dl.max(1, keepdim=True).values) + fp32
    pm = p.clone()
    pm[rows, tgt] = -omp[rows, tgt]
    return dict(loss=-lsm[rows, tgt], loss_b=rel[rows, tgt], pm=pm, s=p * rel)      # the loss: the same expression at the target column


def norm_backward(xh, rn, clamped, dxh, e, D, proven):
    """dX = rn (dX^ - x^ <x^, dX^>) in fp64 (clamped rows: rn dX^) and its bound from the slack e of dX^."""
    nu = _nu(D, proven)
    dot = (xh * dxh).sum(-1, keepdim=True)
    A = (xh.abs() * dxh.abs()).sum(-1, keepdim=True)
    rn = rn[..., None]
    ref = rn * (dxh - xh * dot)
    bound = rn * (e + xh.abs() * (xh.abs() * e).sum(-1, keepdim=True)) + (gamma(D) + 3 * nu + 5 * U) * rn * (dxh.abs() + xh.abs() * A)
    c = clamped[..., None]
    ref = torch.where(c, rn * dxh, ref)
    bound = torch.where(c, rn * e + (nu + 2 * U) * rn * dxh.abs(), bound)
    return ref, bound


def lse_ratio(z):
    """The measurement behind LSE_R: torch fp32 log_softmax of the fp32-rounded logits against fp64 of the same rounded logits, in units
    of u (1 + |l| + |z - m|)."""
    if z.numel() == 0 or z.shape[1] < 2:
        return 0.0
    z32 = z.float()
    zr = z32.double()
    m = zr.max(1, keepdim=True).values
    l_ = torch.log(torch.exp(zr - m).sum(1, keepdim=True))
    err = (torch.log_softmax(z32, dim=1).double() - ((zr - m) - l_)).abs()
    return float((err / (U * (1.0 + l_.abs() + (zr - m).abs()))).max())


# ------------------------------------------------------------------------------------------------------------------------------ in-batch
def _stain_ref(q, p, T, sym, g, mean, Kp, proven):
    """One problem of k live rows: references and bounds of its loss, row losses, dQ and dP, and its logits."""
    k, D = q.shape
    qh, rq, cq = normalize64(q)
    ph, rp, cp = normalize64(p)
    z = qh @ ph.t() / T
    dl = logit_slack(z, qh.abs() @ ph.abs().t(), T, D, proven)
    idx = torch.arange(k)
    d0 = direction(z, dl, idx)
    w0, w1 = (0.5, 0.5) if sym else (1.0, 0.0)
    d1 = direction(z.t(), dl.t(), idx) if sym else dict(loss=torch.zeros(k, dtype=F64), loss_b=torch.zeros(k, dtype=F64),
                                                        pm=torch.zeros(k, k, dtype=F64), s=torch.zeros(k, k, dtype=F64))
    rows = w0 * d0["loss"] + w1 * d1["loss"]
    rows_b = w0 * d0["loss_b"] + w1 * d1["loss_b"] + (2 * U * rows.abs() if sym else 0.0)
    loss = rows.mean()
    loss_b = rows_b.mean() + (gamma(k) + U) * rows.abs().mean()
    gi = (g.double() / k).expand(k) if mean else g.double()
    t0 = (w0 / T) * gi[:, None] * d0["pm"]
    t1 = (w1 / T) * gi[None, :] * d1["pm"].t()
    G = t0 + t1
    sig = (w0 / T) * gi.abs()[:, None] * d0["s"] + (w1 / T) * gi.abs()[None, :] * d1["s"].t() + COEF_R * U * (t0.abs() + t1.abs())
    nu = _nu(D, proven)
    acc = gamma(Kp) + nu + U
    dqh, eq = G @ ph, sig @ ph.abs() + acc * (G.abs() @ ph.abs())
    dph, ep = G.t() @ qh, sig.t() @ qh.abs() + acc * (G.abs().t() @ qh.abs())
    dQ, dQ_b = norm_backward(qh, rq, cq, dqh, eq, D, proven)
    dP, dP_b = norm_backward(ph, rp, cp, dph, ep, D, proven)
    return dict(loss=(loss, loss_b), rows=(rows, rows_b), dQ=(dQ, dQ_b), dP=(dP, dP_b), z=z, clamped=(cq, cp),
                clamped_ref=(rq[:, None] * dqh, rp[:, None] * dph))


def inbatch_ref(case, proven=False):
    """name -> (reference, bound) of loss [S], row_loss [S, Kmax], dQ, dP [S, Kmax, D]: rows >= cnt[s] are 0 with bound 0 (exact)."""
    S, Kmax, D, T = len(case["cnt"]), case["Kmax"], case["D"], t32(case["T"])
    Kp = (Kmax + 31) // 32 * 32
    out = {n: (torch.zeros(sh, dtype=F64), torch.zeros(sh, dtype=F64))
           for n, sh in (("loss", (S,)), ("row_loss", (S, Kmax)), ("dQ", (S, Kmax, D)), ("dP", (S, Kmax, D)))}
    logits = []
    for s, k in enumerate(case["cnt"]):
        if k == 0:
            logits.append(torch.zeros(0, 0, dtype=F64))
            continue
        mean = case["form"] == "d_loss"
        r = _stain_ref(case["Q"][s, :k], case["P"][s, :k], T, case["sym"], case["g"][s] if mean else case["g"][s, :k], mean, Kp, proven)
        logits.append(r["z"])
        for i in (0, 1):
            out["loss"][i][s] = r["loss"][i]
            out["row_loss"][i][s, :k] = r["rows"][i]
            out["dQ"][i][s, :k] = r["dQ"][i]
            out["dP"][i][s, :k] = r["dP"][i]
    out["logits"] = logits
    return out


def check_inbatch(got, case, what=""):
    """Every element of loss, row_loss, dQ, dP against fp64, at the working bound and at the gamma ceiling.  Returns name -> worst ratio."""
    ref, top = inbatch_ref(case), inbatch_ref(case, proven=True)
    return {n: check(what + n, got[n], ref[n][0], ref[n][1], top[n][1]) for n in ("loss", "row_loss", "dQ", "dP")}


def inbatch_passes(got, case, names=("loss", "row_loss", "dQ", "dP")):
    ref, top = inbatch_ref(case), inbatch_ref(case, proven=True)
    return {n: passes(got[n], ref[n][0], ref[n][1], top[n][1]) for n in names}


def _norm32(x):
    ss = (x * x).sum(-1)
    inv = 1.0 / ss.sqrt().clamp_min(1e-12)
    return x * inv[..., None], inv


def _lse32(z, dim):
    m = z.max(dim, keepdim=True).values
    return m, torch.log(torch.exp(z - m).sum(dim, keepdim=True))


def _norm_bwd32(xh, rn, dxh, keep_dot_on_clamped=False, drop_dot_rows=()):
    dot = (xh * dxh).sum(-1, keepdim=True)
    if not keep_dot_on_clamped:
        dot = torch.where((rn >= 0.99e12)[..., None], torch.zeros_like(dot), dot)
    for r in drop_dot_rows:
        dot[r] = 0.0
    return rn[..., None] * (dxh - xh * dot)


def emulate_inbatch(case, fault=None):
    """The staged formula in torch fp32 on the CPU, on the padded [Kp, Kp] problem as the kernels lay it out.  fault: one of
    'col_lse_k_minus_1', 'col_lse_over_Kp', 'no_delta_at_32', 'g_i_for_g_j', 'no_dot_on_longest_row', 'clamped_as_unclamped',
    'mean_over_Kmax' (tests/test_nce_bounds_cpu.py)."""
    S, Kmax, D, T = len(case["cnt"]), case["Kmax"], case["D"], torch.tensor(case["T"], dtype=torch.float32)
    Kp = (Kmax + 31) // 32 * 32
    inv_T = 1.0 / T
    sym = case["sym"]
    out = dict(loss=torch.zeros(S), row_loss=torch.zeros(S, Kmax), dQ=torch.zeros(S, Kmax, D), dP=torch.zeros(S, Kmax, D))
    for s, k in enumerate(case["cnt"]):
        if k == 0:
            continue
        qh, ph = torch.zeros(Kp, D), torch.zeros(Kp, D)
        rq, rp = torch.zeros(Kp), torch.zeros(Kp)
        qh[:k], rq[:k] = _norm32(case["Q"][s, :k])
        ph[:k], rp[:k] = _norm32(case["P"][s, :k])
        Z = (qh @ ph.t()) * inv_T
        m0, l0 = _lse32(Z[:k, :k], 1)
        kc = {"col_lse_k_minus_1": max(k - 1, 1), "col_lse_over_Kp": Kp}.get(fault, k)
        m1, l1 = _lse32(Z[:kc, :k], 0)
        d = Z.diagonal()[:k]
        r0 = l0[:, 0] - (d - m0[:, 0])
        rows = 0.5 * r0 + 0.5 * (l1[0] - (d - m1[0])) if sym else r0
        out["row_loss"][s, :k] = rows
        out["loss"][s] = rows.sum() / (Kmax if fault == "mean_over_Kmax" else k)
        dlt = torch.eye(k)
        if fault == "no_delta_at_32" and k > 32:
            dlt[32, 32] = 0.0
        a = torch.exp((Z[:k, :k] - m0) - l0) - dlt
        b = torch.exp((Z[:k, :k] - m1) - l1) - dlt if sym else torch.zeros(k, k)
        w0, w1 = (0.5, 0.5) if sym else (1.0, 0.0)
        if case["form"] == "d_row_loss":
            g = case["g"][s, :k]
            gj = g[:, None] if fault == "g_i_for_g_j" else g[None, :]
            c = (w0 * g[:, None] * a + w1 * gj * b) * inv_T
        else:
            c = (w0 * a + w1 * b) * case["g"][s] * inv_T / k
        dqh, dph = c @ ph[:k], c.t() @ qh[:k]
        drop = [int(case["Q"][s, :k].norm(dim=1).argmax())] if fault == "no_dot_on_longest_row" else ()
        out["dQ"][s, :k] = _norm_bwd32(qh[:k], rq[:k], dqh, fault == "clamped_as_unclamped", drop)
        out["dP"][s, :k] = _norm_bwd32(ph[:k], rp[:k], dph, fault == "clamped_as_unclamped")
    return out


# --------------------------------------------------------------------------------------------------------------------- explicit negatives
def neg_splits(M, paired):
    ch = NEG_PCH if paired else NEG_KCH
    return (M + ch - 1) // ch if M > 0 else 1


def neg_ref(case, proven=False):
    """name -> (reference, bound) of loss [1], row_loss [N], dQ, dP [N, Dq] (Dq = D rounded up to 32; the padding columns are 0 with
    bound 0) and dNeg (the shape of Neg), and the logits [N, 1 + M]."""
    N, M, D, T, paired = case["N"], case["M"], case["D"], t32(case["T"]), case["paired"]
    Dq = (D + 31) // 32 * 32
    qh, rq, cq = normalize64(case["Q"])
    ph, rp, cp = normalize64(case["P"])
    nh, rn, cn = normalize64(case["Neg"])
    nu = _nu(Dq, proven)
    z0 = (qh * ph).sum(-1, keepdim=True) / T
    mag0 = (qh.abs() * ph.abs()).sum(-1, keepdim=True)
    if paired:
        zn, magn = torch.einsum("nd,nmd->nm", qh, nh) / T, torch.einsum("nd,nmd->nm", qh.abs(), nh.abs())
    else:
        zn, magn = qh @ nh.t() / T, qh.abs() @ nh.abs().t()
    z = torch.cat([z0, zn], 1)
    dl = logit_slack(z, torch.cat([mag0, magn], 1), T, Dq, proven)
    d = direction(z, dl, torch.zeros(N, dtype=torch.long))
    rows, rows_b = d["loss"], d["loss_b"]
    loss, loss_b = rows.mean().reshape(1), (rows_b.mean() + (gamma(N) + U) * rows.abs().mean()).reshape(1)
    g = (case["g"].double() / N).expand(N) if case["form"] == "d_loss" else case["g"].double()
    C = (g[:, None] / T) * d["pm"]
    sig = (g.abs()[:, None] / T) * d["s"] + COEF_R * U * C.abs()
    C0, s0, Cn, sn = C[:, :1], sig[:, :1], C[:, 1:], sig[:, 1:]
    acc = gamma(M + neg_splits(M, paired) + 2) + nu + 2 * U
    if paired:
        dqh = C0 * ph + torch.einsum("nm,nmd->nd", Cn, nh)
        eq = s0 * ph.abs() + torch.einsum("nm,nmd->nd", sn, nh.abs()) + acc * (C0.abs() * ph.abs() + torch.einsum("nm,nmd->nd", Cn.abs(), nh.abs()))
    else:
        dqh = C0 * ph + Cn @ nh
        eq = s0 * ph.abs() + sn @ nh.abs() + acc * (C0.abs() * ph.abs() + Cn.abs() @ nh.abs())
    dph, ep = C0 * qh, s0 * qh.abs() + (nu + 2 * U) * (C0 * qh).abs()
    pad = lambda x: torch.nn.functional.pad(x, (0, Dq - D))      # noqa: E731
    dQ, dQ_b = norm_backward(qh, rq, cq, dqh, eq, Dq, proven)
    dP, dP_b = norm_backward(ph, rp, cp, dph, ep, Dq, proven)
    # dNeg: dN^ and the dot <N^, dN^> from the definition; the kernel's dot is T sum_i C_ij Z_ij, whose slack carries T |C_ij| Delta_ij
    dln = dl[:, 1:]
    dot_e = T * (sn * zn.abs() + Cn.abs() * dln)                  # [N, M] per (i, j)
    dot_mag = T * (Cn * zn).abs()
    n_add = 1 if paired else N
    if paired:
        dnh = Cn[:, :, None] * qh[:, None, :]
        e = sn[:, :, None] * qh.abs()[:, None, :] + (nu + 2 * U) * dnh.abs()
        dot_e, dot_mag = dot_e + 3 * U * dot_mag, dot_mag
    else:
        dnh = Cn.t() @ qh
        e = sn.t() @ qh.abs() + (gamma(n_add + 1) + nu + U) * (Cn.abs().t() @ qh.abs())
        dot_mag = dot_mag.sum(0)
        dot_e = dot_e.sum(0) + (gamma(n_add + 1) + 3 * U) * dot_mag
    dot = (nh * dnh).sum(-1, keepdim=True)
    r_ = rn[..., None]
    dN = r_ * (dnh - nh * dot)
    dN_b = r_ * (e + nh.abs() * dot_e[..., None]) + (3 * nu + 6 * U) * r_ * (dnh.abs() + nh.abs() * dot_mag[..., None])
    c_ = cn[..., None]
    dN = torch.where(c_, r_ * dnh, dN)
    dN_b = torch.where(c_, r_ * e + (nu + 2 * U) * r_ * dnh.abs(), dN_b)
    return dict(loss=(loss, loss_b), row_loss=(rows, rows_b), dQ=(pad(dQ), pad(dQ_b)), dP=(pad(dP), pad(dP_b)), dNeg=(dN, dN_b), logits=z,
                clamped=(cq, cp), clamped_ref=(pad(rq[:, None] * dqh), pad(rp[:, None] * dph)))


NEG_NAMES = ("loss", "row_loss", "dQ", "dP", "dNeg")


def check_neg(got, case, what=""):
    ref, top = neg_ref(case), neg_ref(case, proven=True)
    return {n: check(what + n, got[n], ref[n][0], ref[n][1], top[n][1]) for n in NEG_NAMES if got.get(n) is not None}


def neg_passes(got, case, names=NEG_NAMES):
    ref, top = neg_ref(case), neg_ref(case, proven=True)
    return {n: passes(got[n], ref[n][0], ref[n][1], top[n][1]) for n in names}


def emulate_neg(case, fault=None):
    """The explicit-negative formula in torch fp32 on the CPU, Q and P zero-padded to Dq.  fault: one of 'lse_chunk_dropped',
    'dq_split_dropped', 'neighbours_inverse_norm', 'dot_without_T', 'tail_columns_unread' (tests/test_nce_bounds_cpu.py)."""
    N, M, D, paired = case["N"], case["M"], case["D"], case["paired"]
    Dq = (D + 31) // 32 * 32
    T = torch.tensor(case["T"], dtype=torch.float32)
    inv_T = 1.0 / T
    pad = lambda x: torch.nn.functional.pad(x, (0, Dq - D))      # noqa: E731
    qh, rq = _norm32(case["Q"])
    ph, rp = _norm32(case["P"])
    neg = case["Neg"].clone()
    if fault == "tail_columns_unread" and D % 4:
        neg[..., D - D % 4:] = 0.0
    _, rn = _norm32(neg)
    if fault == "neighbours_inverse_norm" and paired and M > NEG_PCH:
        rn[:, NEG_PCH] = rn[:, NEG_PCH - 1]
    nh = neg * rn[..., None]
    z0 = (qh * ph).sum(-1, keepdim=True) * inv_T
    zn = (torch.einsum("nd,nmd->nm", qh, neg) if paired else qh @ neg.t()) * (rn * inv_T)
    z = torch.cat([z0, zn], 1)
    zl = z
    if fault == "lse_chunk_dropped" and M > NEG_LSE_CH:
        zl = torch.cat([z[:, :1 + NEG_LSE_CH], z[:, 1 + 2 * NEG_LSE_CH:]], 1)
    m, l_ = _lse32(zl, 1)
    rows = l_[:, 0] - (z0[:, 0] - m[:, 0])
    g = (case["g"] / N).expand(N) if case["form"] == "d_loss" else case["g"]
    gi = (g * inv_T)[:, None]
    c0 = (torch.exp((z0 - m) - l_) - 1.0) * gi
    cn = torch.exp((zn - m) - l_) * gi
    cq_ = cn.clone()
    if fault == "dq_split_dropped" and not paired and M > NEG_KCH:
        cq_[:, NEG_KCH:2 * NEG_KCH] = 0.0
    dqh = c0 * ph + (torch.einsum("nm,nmd->nd", cq_, nh) if paired else cq_ @ nh)
    dph = c0 * qh
    dQ, dP = _norm_bwd32(qh, rq, dqh), _norm_bwd32(ph, rp, dph)
    scale = 1.0 if fault == "dot_without_T" else T
    if paired:
        dj = torch.where(rn >= 0.99e12, torch.zeros_like(cn), cn * (zn * scale))
        dN = (qh[:, None, :] * cn[:, :, None] - nh * dj[:, :, None]) * rn[..., None]
    else:
        dot = (cn * zn).sum(0) * scale
        dot = torch.where(rn >= 0.99e12, torch.zeros_like(dot), dot)
        dN = rn[:, None] * (cn.t() @ qh - nh * dot[:, None])
    return dict(loss=rows.mean().reshape(1), row_loss=rows, dQ=pad(dQ), dP=pad(dP), dNeg=dN)


# ---------------------------------------------------------------------------------------------------- the references the issue names, once
def oracle_inbatch(case):
    """loss, row_loss, dQ, dP from oracle.restatement.info_nce in fp64 under torch autograd: the documented operation, which the
    written-out references above are asserted against in tests/test_nce_bounds_cpu.py."""
    from oracle import restatement as R
    S, Kmax, D = len(case["cnt"]), case["Kmax"], case["D"]
    out = dict(loss=torch.zeros(S, dtype=F64), row_loss=torch.zeros(S, Kmax, dtype=F64), dQ=torch.zeros(S, Kmax, D, dtype=F64),
               dP=torch.zeros(S, Kmax, D, dtype=F64))
    for s, k in enumerate(case["cnt"]):
        if k == 0:
            continue
        q, p = case["Q"][s, :k].double().requires_grad_(), case["P"][s, :k].double().requires_grad_()
        rows = R.info_nce(q, p, t32(case["T"]), bool(case["sym"]), reduction="none")
        out["row_loss"][s, :k], out["loss"][s] = rows.detach(), rows.detach().mean()
        up = (rows.mean() * case["g"][s].double()) if case["form"] == "d_loss" else (rows * case["g"][s, :k].double()).sum()
        up.backward()
        out["dQ"][s, :k], out["dP"][s, :k] = q.grad, p.grad
    return out


def ref_loss_neg(q, p, neg, T, paired, reduction="mean"):
    """The ref_loss formula of tests/test_infonce_negatives_gpu.py (that module is GPU-marked; the formula is restated to be usable here)."""
    import torch.nn.functional as F
    qn, pn, nn_ = F.normalize(q, dim=-1), F.normalize(p, dim=-1), F.normalize(neg, dim=-1)
    pos = (qn * pn).sum(-1, keepdim=True)
    negl = (qn.unsqueeze(1) @ nn_.transpose(-2, -1)).squeeze(1) if paired else qn @ nn_.transpose(-2, -1)
    logits = torch.cat([pos, negl], dim=1)
    return F.cross_entropy(logits / T, torch.zeros(len(q), dtype=torch.long, device=q.device), reduction=reduction)


def oracle_neg(case, dtype=F64):
    q, p, n = (case[k].detach().clone().to(dtype).requires_grad_() for k in ("Q", "P", "Neg"))
    rows = ref_loss_neg(q, p, n, t32(case["T"]), bool(case["paired"]), "none")
    up = rows.mean() * case["g"][0].to(dtype) if case["form"] == "d_loss" else (rows * case["g"].to(dtype)).sum()
    up.backward()
    return dict(loss=rows.detach().mean().reshape(1), row_loss=rows.detach(), dQ=q.grad, dP=p.grad, dNeg=n.grad)
