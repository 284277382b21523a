"""The epilogues of the split engine's NT products and of the gate's dX product, one compiled body per set of optional operands
(csrc/split_engine.hpp sp_epilogue_rows_ld, sp_mode_switch): every body that the C entry points can reach, on full and partial tiles.

Each result is held to the fp64 reference on the planes the kernel read under the per-element bound of DESIGN.md 4.3, exactly as
tests/test_split_elements_gpu.py computes it (tests/_split_bounds.py: nt_raw / nt_finish, gate_bwd_ref, gate_pool_term).

mdl_split_gemm_nt and mdl_split_gemm_nt_group_bias: M of {1, 255, 256, 257, 513} x N of {4, 128, 132, 256, 260} x K of {32, 64} x ldc of
{N, N + 12}, with every PAIR of the optional operands {bias, a_row_mul, b_col_mul, accumulate, absmax_out, row_gate, group_bias} that
an entry point accepts (and each one alone).  What the entry points rule out is not a case: row_gate is only taken with accumulate and
without bias (so its pairs carry accumulate as a third operand, and (row_gate, bias) does not exist), and the group-bias entry has no
accumulate, absmax_out or row_gate.  The row gate has one all-zero 256-row tile (the first; the only one where M <= 256), the group bias
two groups that meet inside the first tile (at row 100; M = 1 has one group).  All M share one data set (the M = 513 one, cut), the
largest element of A in row 0: rows 0..255 of every M = 513 result are then compared bit for bit with the M = 256 result of the same
operands -- the 512 x 128 tile of M = 513, N <= 128 against the 256 x 256 tile included.  absmax_out is the maximum of |C| as stored,
exactly.

mdl_abmil_attnpool_bwd_split (dE): T of {255, 256, 300} x H of {1, 4}, without the pooling term and with it on dense bags of 256 tokens
(one bag per tile), dense bags of 100 tokens (three bags per tile) and ragged bags, accumulate 0 and 1."""
import itertools

import pytest
import torch

from tests import _bf16_bounds as B
from tests import _split_bounds as S
from tests.test_split_elements_gpu import Img, _call, _gap_is_nan, _gate_bwd, _gate_check_fwd, _gate_fwd, _stream, _wide

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ================================================================================================================================== NT
NT_M = (1, 255, 256, 257, 513)
NT_N = (4, 128, 132, 256, 260)
NT_K = (32, 64)
OPERANDS = ("bias", "arm", "bcol", "acc", "absmax", "gate", "group")


def _accepted(opts):
    """Whether an entry point takes this set of optional operands."""
    if "group" in opts:
        return not {"acc", "absmax", "gate"} & set(opts)
    if "gate" in opts:
        return "bias" not in opts
    return True


def nt_variants():
    """Each operand alone and every pair an entry point accepts; a row gate brings accumulate with it."""
    out = []
    for opts in [(o,) for o in OPERANDS] + list(itertools.combinations(OPERANDS, 2)):
        if _accepted(opts):
            out.append(tuple(sorted(set(opts) | ({"acc"} if "gate" in opts else set()))))
    return [()] + sorted(set(out))


def _nt_data(N, K):
    """The M = 513 data set: a [513, K] with its largest element (1.0) in row 0 and a zero row, b [N, K], bias, c0, two group rows."""
    case = S.nt_case(513, N, K, 900 + N + K, "uniform")
    case["a"][0, 0] = 1.0
    case["a"][100] = 0.0                                   # row_inv == 0 as a_row_mul
    case["gb"] = case["gb"][:2].contiguous()
    case["row_group"] = (torch.arange(513) >= 100).to(torch.int32)          # two groups meeting inside the first tile
    return case


def _nt_run(dev, A, Bm, case, M, N, K, opts, pad, gate):
    C, cbuf = _wide(dev, M, N, pad, case["c0"][:M] if "acc" in opts else None)
    bias = case["bias"].to(dev) if "bias" in opts else None
    amax = torch.zeros(1, device=dev) if "absmax" in opts else None
    arm = A.row_inv if "arm" in opts else None
    bcol = Bm.row_inv if "bcol" in opts else None
    if "group" in opts:
        _call("mdl_split_gemm_nt_group_bias", A.raw, A.rsb, A.scale, Bm.raw, Bm.rsb, Bm.scale, C, C.stride(0), M, N, K, bias, arm, bcol,
              case["gb"].to(dev), case["row_group"][:M].contiguous().to(dev), 3, _stream())
    else:
        _call("mdl_split_gemm_nt", A.raw, A.rsb, A.scale, Bm.raw, Bm.rsb, Bm.scale, C, C.stride(0), M, N, K, bias, int("acc" in opts), amax,
              gate if "gate" in opts else None, arm, bcol, 3, _stream())
    torch.cuda.synchronize()
    assert C.stride(0) == N + pad
    if pad:
        assert _gap_is_nan(cbuf, N), "the gap between the rows of C was written"
    return C.cpu(), (None if amax is None else float(amax))


@pytest.mark.parametrize("K", NT_K)
@pytest.mark.parametrize("N", NT_N)
def test_nt_epilogue_modes(dev, N, K):
    """Every accepted pair of optional operands at every M, ldc = N and N + 12: the per-element bound, absmax_out exact, a skipped tile
    untouched, and rows 0..255 of M = 513 equal to M = 256 bit for bit."""
    case = _nt_data(N, K)
    variants = nt_variants()
    imgs, raws, kept = {}, {}, {}
    for M in NT_M:
        zero_to = min(M, 256)                                                      # the gated A: its first 256-row tile all zero
        a_plain, a_gated = case["a"][:M].clone(), case["a"][:M].clone()
        a_gated[:zero_to] = 0.0
        gate = None
        for opts in variants:
            gated, a_rows, b_rows = "gate" in opts, "arm" in opts, "bcol" in opts
            if gated and gate is None:
                X, _ = _wide(dev, M, K, 4, a_gated)
                gate = torch.full(((M + 255) // 256,), float("nan"), device=dev)
                _call("mdl_split_tile_absmax", X, X.stride(0), M, K, gate, None, _stream())
                assert int((gate == 0).sum()) == 1
            if (M, gated, a_rows) not in imgs:
                imgs[M, gated, a_rows] = Img(dev, a_gated if gated else a_plain, a_rows, what="modes.a")
            if ("b", b_rows) not in imgs:
                imgs["b", b_rows] = Img(dev, case["b"], b_rows, what="modes.b")
            A, Bm = imgs[M, gated, a_rows], imgs["b", b_rows]
            rkey = (M, gated, a_rows, b_rows)
            if rkey not in raws:
                raws[rkey] = S.nt_raw(*A.planes(), *Bm.planes(), 3)
            kw = dict(inv=1.0 / (A.s * Bm.s), a_row_mul=A.inv_cpu if a_rows else None, b_col_mul=Bm.inv_cpu if b_rows else None)
            if "bias" in opts:
                kw["bias"] = case["bias"]
            if "group" in opts:
                kw["gb_rows"] = case["gb"][case["row_group"][:M].long()]
            if "acc" in opts:
                kw["c0"] = case["c0"][:M]
            ref, b1, b2 = S.nt_finish(raws[rkey], 3 * K, **kw)
            for pad in (0, 12):
                what = "modes.nt[%dx%dx%d,ldc+%d,%s]" % (M, N, K, pad, "+".join(opts) or "plain")
                got, amax = _nt_run(dev, A, Bm, case, M, N, K, opts, pad, gate)
                S.check(what, got, ref, b1, b2)
                ran = torch.ones(M, dtype=torch.bool)
                if gated:
                    ran[:zero_to] = False
                    assert torch.equal(got[~ran], case["c0"][:M][~ran]), what + ": a skipped tile changed"
                if amax is not None:
                    assert amax == (float(got[ran].abs().max()) if bool(ran.any()) else 0.0), what + ": absmax_out is not max |C| as stored"
                if M in (256, 513):
                    kept[M, opts, pad] = got[:256]
    pairs = [k for k in kept if k[0] == 513]
    assert pairs
    for _, opts, pad in pairs:
        assert torch.equal(kept[513, opts, pad], kept[256, opts, pad]), \
            "rows 0..255 of M = 513 differ from M = 256 [N %d, K %d, ldc+%d, %s]" % (N, K, pad, "+".join(opts) or "plain")


def test_nt_variants_cover_every_accepted_pair():
    """The list the test above walks: 7 single operands, the 21 pairs less (row_gate, bias) and the group-bias entry's three missing
    arguments -- 17 pairs."""
    v = nt_variants()
    pairs = [p for p in itertools.combinations(OPERANDS, 2) if _accepted(p)]
    assert len(pairs) == 17
    for p in pairs:
        want = set(p) | ({"acc"} if "gate" in p else set())
        assert any(set(o) == want for o in v), p


# ==================================================================================================== the gate's dX epilogue (pooling term)
def _bag_layouts(T):
    """(name, bag lengths, dense bag size or 0)."""
    def dense(n):
        return [n] * (T // n) + ([T % n] if T % n else [])
    return (("dense256", dense(256), 256), ("dense100", dense(100), 100), ("ragged", [70, 59, T - 129], 0))


@pytest.mark.parametrize("H", [1, 4])
@pytest.mark.parametrize("T", [255, 256, 300])
def test_gate_dx_epilogue_modes(dev, T, H):
    """dE of mdl_abmil_attnpool_bwd_split, written and accumulated: no pooling term; one bag per tile (dense bags of 256 tokens: the
    lane's d_pooled vector is loaded once); three bags in a tile (dense bags of 100 tokens: per-row vectors, loaded a group ahead of
    their use); ragged bags through row_bag.  T = 255 and 300 end in a partial tile."""
    from tests.test_bf16_elements_gpu import _gate_masks
    p, kind = 0.25, "uniform"
    case = S.gate_case(T, H, 4800 + T + H, kind, p)
    seed = 555 + T
    ka, kb = _gate_masks(dev, T, H, p, seed)
    what = "modes.gate[T%d,H%d]." % (T, H)
    Ei, ps, sc, a, b = _gate_fwd(dev, case, seed)
    E_dec, E_hi, a32, b32 = _gate_check_fwd(case, Ei, sc, a, b, ka, kb, what, dev)
    s = sc.cpu()
    layouts = [("none", None, 0)] + list(_bag_layouts(T))
    for name, lens, dense_n in layouts:
        pool, term = (), None
        if lens is not None:
            row_bag, m, l_ = S.gate_pool_inputs(s, lens)
            dp = S.operand((len(lens), H * B.HID), 4900 + H + len(lens), kind)
            term, _ = S.gate_pool_term(s, m, l_, dp, row_bag, H, what + name + ".")
            pool = [x.to(dev) for x in (s, m, l_, dp)] + ([None, dense_n] if dense_n else [row_bag.to(dev), 0])
        for acc in (0, 1):
            got = _gate_bwd(dev, case, Ei, ps, a, b, seed, acc, (3,), 3, pool)
            ref = S.gate_bwd_ref(case, E_dec, E_hi, a32, b32, ka, kb, acc, 3, term, dev)
            S.check("%s%s.acc%d.dE" % (what, name, acc), got["dE"], *ref["dE"])
