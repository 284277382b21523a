"""The cases of tests/test_stride_limits_gpu.py as plain data, and the layout they run on; importable without a GPU.

Two kinds of promises of include/madeleine_amd.h about row strides are run on a device here.
  Part A  a stride argument with a 32-bit limit `rows * stride * elem + col <= 2^31 - 1` runs AT the largest aligned stride its
          launcher accepts, on T = 2 (rows + 1) + 1 rows of the wide operand: two full tiles of the limiting expression and a ragged
          row, so that the last row of a tile sits at the 32-bit edge and the second tile starts past byte 2^32.
  Part B  a stride argument the header calls limit-free ("every offset is formed in 64 bits") runs at a stride that puts the last
          max(2, R // 8) of its R rows past element 2^31 of the operand (past byte 2^32 for a stride counted in bytes).
Rows that far apart need no large problem: the kernels do the work of a few hundred rows.  Every wide operand of a case is a column
slice of ONE device arena seen as [rows, stride]; the header allows an operand to be a column slice of a wider buffer.

Where the kernel whose expression sets a limit is only dispatched above a row count whose span would not fit the arena, the argument
is in ARGUED and has two cases instead: (i) the limit stride at T = 2 (rows + 1) + 1 on the kernel the launcher picks there (it
accepts that stride for every T), (ii) the limiting kernel at its smallest T with the largest aligned stride that fits the arena."""
import torch

LIM = 0x7FFFFFFF
ARENA_BYTES = 25 << 29                # 12.5 GiB
MIN_FREE_BYTES = 16 << 30             # the arena fixture skips below this much free device memory
LEAD = 1 << 31                        # bytes of fill in front of the first wide row: a wrapped (lower) address stays inside the arena
GAP = 64                              # bytes of fill between neighbouring slices of a row, at least
FILL = 0xFF                           # every fp32 / bf16 pattern of it is a NaN
SCAN_CHUNK = 1 << 30


def _up(n, a):
    return (n + a - 1) // a * a


# =========================================================================================================================== Part A
class A:
    """One Part A case.  family / params: which runner of tests/test_strides_gpu.py and its arguments; target: the runner's indices k
    of the operands that go wide; arg: the header's name of the stride; elem / align / rows / col: the terms of the limit as
    tests/test_strides_cpu.py carries them; T: rows of the wide operand (span_rows: rows of the tallest wide operand where zero pad
    rows follow); kind: 'limit', or 'i' / 'ii' of an ARGUED argument; covers: the (entry point, argument) pairs whose limit this is;
    plan: (product, T, a, b, expected fields) asserted before the run; capped: the operand cannot have more rows than one tile."""

    def __init__(self, id, family, params, target, arg, elem, align, rows, col, T, covers, plan, kind="limit", span_rows=None, capped=False):
        self.id, self.family, self.params, self.target, self.arg = id, family, params, frozenset(target), arg
        self.elem, self.align, self.rows, self.col, self.T, self.covers, self.plan = elem, align, rows, col, T, covers, plan
        self.kind, self.span_rows, self.capped = kind, span_rows or T, capped

    @property
    def limit_ld(self):
        """The largest aligned stride the launcher accepts: the `inside` of test_stride_refusals_before_any_launch."""
        return (LIM - self.col) // (self.rows * self.elem) // self.align * self.align

    @property
    def ld(self):
        if self.kind != "ii":
            return self.limit_ld
        return min(self.limit_ld, (ARENA_BYTES - LEAD) // (self.span_rows * self.elem) // self.align * self.align)


def _t(rows):
    return 2 * (rows + 1) + 1


GATE32_BWD = ["mdl_abmil_gate_bwd", "mdl_abmil_attnpool_bwd", "mdl_abmil_attnpool_bwd_phases"]
GATE16_BWD = [n + "_bf16" for n in GATE32_BWD]
NT = ["mdl_split_gemm_nt", "mdl_split_gemm_nt_group_bias"]


def _cov(names, arg):
    return [(n, arg) for n in names]


def _part_a():
    c = []

    def add(*a, **k):
        c.append(A(*a, **k))
    # ---- gates: E and dE share ldE (k = 0); the forward's limit is the tighter one, so the backward variants run at it too
    add("gate_fp32-fwd_limit", "gate", dict(bf16=False, H=1, forward=True), {0}, "ldE", 4, 4, 127, 48, _t(127),
        _cov(["mdl_abmil_gate_fwd"], "ldE"), [("gate_fp32_bwd", _t(127), 1, 0, dict(splits=1, chunk=16))])
    add("gate_fp32-bwd_limit", "gate", dict(bf16=False, H=1, forward=False, fwd_contig=True), {0}, "ldE", 4, 4, 15, 1020, _t(15),
        _cov(GATE32_BWD, "ldE"), [("gate_fp32_bwd", _t(15), 1, 0, dict(splits=1, chunk=16))])
    add("gate_bf16-fwd_limit-i", "gate", dict(bf16=True, H=1, forward=True), {0}, "ldE", 2, 8, 255, 112, _t(255),
        _cov(["mdl_abmil_gate_fwd_bf16"], "ldE"), [("gate_bf16_fwd", _t(255), 1, 0, dict(variant=128))], kind="i")
    add("gate_bf16-fwd_limit-ii", "gate", dict(bf16=True, H=1, forward=True), {0}, "ldE", 2, 8, 255, 112, 4097,
        _cov(["mdl_abmil_gate_fwd_bf16"], "ldE"), [("gate_bf16_fwd", 4097, 1, 0, dict(variant=256))], kind="ii")
    add("gate_bf16-bwd_limit-i", "gate", dict(bf16=True, H=1, forward=False, fwd_contig=True), {0}, "ldE", 2, 8, 63, 496, _t(63),
        _cov(GATE16_BWD, "ldE"), [("gate_bf16_bwd", _t(63), 1, 0, dict(variant=128, chunk=32))], kind="i")
    add("gate_bf16-bwd_limit-ii", "gate", dict(bf16=True, H=1, forward=False), {0}, "ldE", 2, 8, 63, 496, 16385,
        _cov(GATE16_BWD, "ldE"), [("gate_bf16_bwd", 16385, 1, 0, dict(variant=256, chunk=64))], kind="ii")
    # ---- split gate: the image of E is k = 0 (e_rsb, bytes), dE is k = 1 (ldE, floats)
    add("gate_split-e_rsb-fwd_limit", "gate_split", dict(H=1, forward=True), {0}, "e_rsb", 1, 16, 256, 0, _t(256),
        _cov(["mdl_abmil_gate_fwd_split"], "e_rsb"), [("gate_split_fwd", _t(256), 1, 0, dict(splits=1)), ("gate_split_bwd", _t(256), 1, 0, dict(splits=1))])
    add("gate_split-e_rsb-bwd_limit", "gate_split", dict(H=1, forward=False, fwd_contig=True), {0}, "e_rsb", 1, 16, 32, 0, _t(32),
        _cov(["mdl_abmil_attnpool_bwd_split"], "e_rsb"), [("gate_split_bwd", _t(32), 1, 0, dict(splits=1, chunk=32))])
    add("gate_split-ldE_of_dE", "gate_split", dict(H=1, forward=True), {1}, "ldE", 4, 4, 1, 0, _t(1),
        _cov(["mdl_abmil_attnpool_bwd_split"], "ldE"), [("gate_split_bwd", _t(1), 1, 0, dict(splits=1))])
    # ---- fp32 Linears: forward X k = 0, Y k = 1; backward X k = 0, dY k = 1, dX k = 2.  T <= 256 runs lin_small_kernel (variant 0)
    fwd, bwd = dict(forward=True, backward=False), dict(forward=False, backward=True)
    wide, tall = dict(bf16=False, N=256, K=96), dict(bf16=False, N=128, K=256)
    add("linear_fp32-fwd-ldx-wide", "linear", dict(wide, **fwd), {0}, "ldx", 4, 4, 127, 48, _t(127),
        _cov(["mdl_linear_fwd"], "ldx"), [("linear_fp32_bwd", _t(127), 256, 96, dict(variant=1))])
    add("linear_fp32-fwd-ldx-tall", "linear", dict(tall, **fwd), {0}, "ldx", 4, 4, 255, 48, _t(255),
        _cov(["mdl_linear_fwd"], "ldx"), [("linear_fp32_bwd", _t(255), 128, 256, dict(variant=2))])
    add("linear_fp32-fwd-ldy-i", "linear", dict(wide, **fwd), {1}, "ldy", 4, 4, 3, 1020, _t(3),
        _cov(["mdl_linear_fwd"], "ldy"), [("linear_fp32_bwd", _t(3), 256, 96, dict(variant=0))], kind="i")
    add("linear_fp32-fwd-ldy-ii", "linear", dict(wide, **fwd), {1}, "ldy", 4, 4, 3, 1020, 257,
        _cov(["mdl_linear_fwd"], "ldy"), [("linear_fp32_bwd", 257, 256, 96, dict(variant=1))], kind="ii")
    add("linear_fp32-bwd-ldx-i", "linear", dict(wide, **bwd), {0}, "ldx", 4, 4, 15, 4 * 96, _t(15),
        _cov(["mdl_linear_bwd"], "ldx"), [("linear_fp32_bwd", _t(15), 256, 96, dict(variant=0))], kind="i")
    add("linear_fp32-bwd-ldx-ii", "linear", dict(wide, **bwd), {0}, "ldx", 4, 4, 15, 4 * 96, 257,
        _cov(["mdl_linear_bwd"], "ldx"), [("linear_fp32_bwd", 257, 256, 96, dict(variant=1, chunk=16))], kind="ii")
    add("linear_fp32-bwd-ldy", "linear", dict(wide, **bwd), {1}, "ldy", 4, 4, 127, 48, _t(127),
        _cov(["mdl_linear_bwd"], "ldy"), [("linear_fp32_bwd", _t(127), 256, 96, dict(variant=1))])
    add("linear_fp32-bwd-lddx-i", "linear", dict(wide, **bwd), {2}, "lddx", 4, 4, 3, 1020, _t(3),
        _cov(["mdl_linear_bwd"], "lddx"), [("linear_fp32_bwd", _t(3), 256, 96, dict(variant=0))], kind="i")
    add("linear_fp32-bwd-lddx-ii", "linear", dict(wide, **bwd), {2}, "lddx", 4, 4, 3, 1020, 257,
        _cov(["mdl_linear_bwd"], "lddx"), [("linear_fp32_bwd", 257, 256, 96, dict(variant=1))], kind="ii")
    # ---- bf16 Linears: the 256-row kernels whose expressions set the limits run from T = 4097 (N = 1024) and T = 16385 on
    small, big = dict(bf16=True, N=256, K=512), dict(bf16=True, N=1024, K=512)
    add("linear_bf16-fwd-ldx-i", "linear", dict(small, **fwd), {0}, "ldx", 2, 8, 255, 112, _t(255),
        _cov(["mdl_linear_fwd_bf16"], "ldx"), [("linear_bf16_fwd", _t(255), 256, 512, dict(variant=4))], kind="i")
    add("linear_bf16-fwd-ldx-ii", "linear", dict(big, **fwd), {0}, "ldx", 2, 8, 255, 112, 4097,
        _cov(["mdl_linear_fwd_bf16"], "ldx"), [("linear_bf16_fwd", 4097, 1024, 512, dict(variant=256))], kind="ii")
    add("linear_bf16-fwd-ldy-i", "linear", dict(small, **fwd), {1}, "ldy", 2, 8, 7, 510, _t(7),
        _cov(["mdl_linear_fwd_bf16"], "ldy"), [("linear_bf16_fwd", _t(7), 256, 512, dict(variant=4))], kind="i")
    add("linear_bf16-fwd-ldy-ii", "linear", dict(big, **fwd), {1}, "ldy", 2, 8, 7, 510, 4097,
        _cov(["mdl_linear_fwd_bf16"], "ldy"), [("linear_bf16_fwd", 4097, 1024, 512, dict(variant=256))], kind="ii")
    add("linear_bf16-bwd-lddy-i", "linear", dict(small, **bwd), {1}, "lddy", 2, 8, 255, 112, _t(255),
        _cov(["mdl_linear_bwd_bf16"], "lddy"), [("linear_bf16_bwd", _t(255), 256, 512, dict(extra=4))], kind="i")
    add("linear_bf16-bwd-lddy-ii", "linear", dict(big, **bwd), {1}, "lddy", 2, 8, 255, 112, 4097,
        _cov(["mdl_linear_bwd_bf16"], "lddy"), [("linear_bf16_bwd", 4097, 1024, 512, dict(extra=256))], kind="ii")
    add("linear_bf16-bwd-ldx-i", "linear", dict(small, **bwd), {0}, "ldx", 2, 8, 63, 496, _t(63),
        _cov(["mdl_linear_bwd_bf16"], "ldx"), [("linear_bf16_bwd", _t(63), 256, 512, dict(variant=128, chunk=32))], kind="i")
    add("linear_bf16-bwd-ldx-ii", "linear", dict(small, **bwd), {0}, "ldx", 2, 8, 63, 496, 16385,
        _cov(["mdl_linear_bwd_bf16"], "ldx"), [("linear_bf16_bwd", 16385, 256, 512, dict(variant=256, chunk=64))], kind="ii")
    add("linear_bf16-bwd-lddx-i", "linear", dict(small, **bwd), {2}, "lddx", 2, 8, 7, 510, _t(7),
        _cov(["mdl_linear_bwd_bf16"], "lddx"), [("linear_bf16_bwd", _t(7), 256, 512, dict(extra=4))], kind="i")
    add("linear_bf16-bwd-lddx-ii", "linear", dict(big, **bwd), {2}, "lddx", 2, 8, 7, 510, 4097,
        _cov(["mdl_linear_bwd_bf16"], "lddx"), [("linear_bf16_bwd", 4097, 1024, 512, dict(extra=256))], kind="ii")
    # ---- split products: A k = 0, B k = 1, C k = 2.  B has N rows and N % 4 == 0: 516 stands for 2 (256 + 1) + 1 = 515
    add("split_nt-a_rsb", "split_nt", dict(M=_t(256), N=256, K=96), {0}, "a_rsb", 1, 16, 256, 0, _t(256), _cov(NT, "a_rsb"), [])
    add("split_nt-b_rsb", "split_nt", dict(M=300, N=516, K=96), {1}, "b_rsb", 1, 16, 256, 0, 516, _cov(NT, "b_rsb"), [])
    add("split_nt-ldc", "split_nt", dict(M=_t(1), N=256, K=96), {2}, "ldc", 4, 4, 1, 0, _t(1), _cov(NT, "ldc"), [])
    add("split_nt-narrow-a_rsb", "split_nt", dict(M=_t(512), N=128, K=64, only_plain=True), {0}, "a_rsb", 1, 16, 512, 0, _t(512),
        _cov(NT[:1], "a_rsb"), [])
    # the narrow-output tile exists for N <= 128 only: B cannot have a second tile, so no row of it starts past byte 2^32
    add("split_nt-narrow-b_rsb", "split_nt", dict(M=300, N=128, K=64, only_plain=True), {1}, "b_rsb", 1, 16, 128, 0, 128,
        _cov(NT[:1], "b_rsb"), [], capped=True)
    add("split_tn-a_rsb", "split_tn", dict(T=_t(32)), {0}, "a_rsb", 1, 16, 32, 0, _t(32),
        _cov(["mdl_split_gemm_tn"], "a_rsb"), [("split_tn", _t(32), 256, 128, dict(splits=1, chunk=32))])
    add("split_tn-b_rsb", "split_tn", dict(T=_t(32)), {1}, "b_rsb", 1, 16, 32, 0, _t(32),
        _cov(["mdl_split_gemm_tn"], "b_rsb"), [("split_tn", _t(32), 256, 128, dict(splits=1, chunk=32))], span_rows=_t(32) + 32)
    return c


PART_A = _part_a()

_WHY = ("the exact 32-bit edge of %s, which runs from T = %d on, is argued from its address expression and not run: %d rows at the "
        "limit stride do not fit the arena.")
ARGUED = {
    ("mdl_abmil_gate_fwd_bf16", "ldE"): _WHY % ("gate_fwd256_bf16_kernel", 4097, 4097),
    ("mdl_abmil_gate_bwd_bf16", "ldE"): _WHY % ("gate_dw256_bf16_kernel", 16385, 16385),
    ("mdl_abmil_attnpool_bwd_bf16", "ldE"): _WHY % ("gate_dw256_bf16_kernel", 16385, 16385),
    ("mdl_abmil_attnpool_bwd_phases_bf16", "ldE"): _WHY % ("gate_dw256_bf16_kernel", 16385, 16385),
    ("mdl_linear_fwd", "ldy"): _WHY % ("the tiled fp32 epilogue", 257, 257),
    ("mdl_linear_bwd", "ldx"): _WHY % ("lin_tn_kernel", 257, 257),
    ("mdl_linear_bwd", "lddx"): _WHY % ("the tiled fp32 epilogue", 257, 257),
    ("mdl_linear_fwd_bf16", "ldx"): _WHY % ("linb_nt256_kernel", 4097, 4097),
    ("mdl_linear_fwd_bf16", "ldy"): _WHY % ("the epilogue of linb_nt256_kernel", 4097, 4097),
    ("mdl_linear_bwd_bf16", "lddy"): _WHY % ("linb_nt256_kernel (the dX product)", 4097, 4097),
    ("mdl_linear_bwd_bf16", "ldx"): _WHY % ("linb_tn256_kernel", 16385, 16385),
    ("mdl_linear_bwd_bf16", "lddx"): _WHY % ("the epilogue of linb_nt256_kernel (the dX product)", 4097, 4097),
}


# =========================================================================================================================== Part B
class B:
    """One Part B case: `family` / `params` name the runner, `target` its wide operands, `R` the rows of the tallest wide operand,
    `elem` the bytes of one unit of the stride (1: a stride in bytes), `align` the stride's alignment in its unit, `covers` the
    (entry point, argument) pairs the run passes the wide stride to."""

    def __init__(self, id, family, params, target, R, elem, align, covers):
        self.id, self.family, self.params, self.target, self.R, self.elem, self.align, self.covers = id, family, params, frozenset(target), R, elem, align, covers

    @property
    def far_rows(self):
        return max(2, self.R // 8)

    @property
    def mark(self):
        """Units of the stride from the operand's base to element 2^31 (to byte 2^32 for a stride in bytes)."""
        return (1 << 32) if self.elem == 1 else (1 << 31)

    @property
    def ld(self):
        first_far = self.R - self.far_rows
        return _up(-(-self.mark // first_far), self.align)


def _pool_names(sfx):
    return ["mdl_abmil_%s%s" % (n, sfx) for n in ("pool_fwd", "pool_bwd", "wpool_fwd", "wpool_bwd")]


def _view_names(sfx):
    return ["mdl_abmil_%s%s" % (n, sfx) for n in ("pool_view_fwd", "pool_view_bwd", "pool_rview_fwd", "pool_rview_bwd")]


def _part_b():
    c = []

    def add(*a):
        c.append(B(*a))
    ragged = (300, 0, 1, 129)
    for bf16, sfx, elem in ((False, "", 4), (True, "_bf16", 2)):
        tag = "bf16" if bf16 else "fp32"
        align = 16 // elem      # (the bf16 pooling takes any multiple of 4; the slices of a row keep 16-byte alignment with 8)
        add("pool-" + tag, "pool", dict(H=1, lens=ragged, bf16=bf16), {0}, sum(ragged), elem, align, _cov(_pool_names(sfx), "ldE"))
        add("pool_views-" + tag, "pool_views", dict(H=1, bf16=bf16), {0}, 900, elem, align, _cov(_view_names(sfx), "ldE"))
    add("pool_img", "pool_img", dict(H=1, lens=ragged), {0}, sum(ragged), 1, 16,
        _cov(["mdl_abmil_pool_fwd_img", "mdl_abmil_pool_dscores_img"], "e_rsb"))
    add("split_image-ldx", "split_image", dict(K=64), {0}, 300, 4, 4,
        _cov(["mdl_split_image", "mdl_split_image_rows", "mdl_split_tile_absmax"], "ldx"))
    add("split_image-rsb", "split_image", dict(K=64), {1, 2}, 332, 1, 16, _cov(["mdl_split_image", "mdl_split_image_rows"], "rsb"))
    # ---- the newer families, on the shapes and data of their own files.  The store: 6067 rows in bags of 1 .. 4097
    store = _cov(["mdl_bag_sample", "mdl_bag_pack", "mdl_bag_mean"], "row_stride")
    add("store-fp32", "store", dict(dtype="float32"), {0}, 6067, 4, 4, store)
    add("store-bf16", "store", dict(dtype="bfloat16"), {0}, 6067, 2, 8, store)
    from madeleine_amd import _native
    keys = _native._DEFINES["MDL_ATTN_SORT_KEYS"]       # tests/test_attention_gpu.py's LENS: 970 + 6 C rows
    add("attn", "attn", dict(name="normals", H=4), {0}, 970 + 6 * keys, 4, 4, _cov(["mdl_attn_softmax", "mdl_attn_rank"], "ld"))
    add("smooth_rank", "rank", dict(n=300, d=72), {0}, 300, 4, 4, _cov(["mdl_smooth_rank", "mdl_smooth_rank_marked"], "ldE"))
    retr = dict(n=257, m=400, d=77, noise=3, k=10)
    add("retrieval-ldq", "retrieval", retr, {0}, 257, 4, 4, [("mdl_retrieval", "ldq")])
    add("retrieval-ldk", "retrieval", retr, {1}, 400, 4, 4, [("mdl_retrieval", "ldk")])
    # probes: X k = 0; the labels (time; event) of P = 10 .. 12 problems, one row each, k = 1 (k = 2)
    add("probe-ldX", "probe", dict(mod="probe", cohort="B"), {0}, 160, 4, 4, _cov(["mdl_probe_fit", "mdl_probe_scores"], "ldX"))
    add("probe-ldy", "probe", dict(mod="probe", cohort="B"), {1}, 12, 4, 4, _cov(["mdl_probe_fit", "mdl_probe_metrics"], "ldy"))
    add("logit-ldX", "probe", dict(mod="logit", cohort="FA"), {0}, 400, 4, 4, _cov(["mdl_logit_fit"], "ldX"))
    add("logit-ldy", "probe", dict(mod="logit", cohort="FA"), {1}, 10, 4, 4, _cov(["mdl_logit_fit", "mdl_logit_metrics"], "ldy"))
    add("cox-ldX", "cox", dict(cohort="A"), {0}, 330, 4, 4, _cov(["mdl_cox_fit"], "ldX"))
    add("cox-ldt", "cox", dict(cohort="A"), {1}, 10, 4, 4, _cov(["mdl_cox_fit", "mdl_surv_metrics"], "ldt"))
    add("cox-lde", "cox", dict(cohort="A"), {2}, 10, 4, 4, _cov(["mdl_cox_fit", "mdl_surv_metrics"], "lde"))
    add("heat_render", "heat", dict(C=4), {0}, 700, 4, 4, _cov(["mdl_heat_render", "mdl_heat_render_marked"], "ld"))
    return c


PART_B = _part_b()

# the tiered store reads its second tier from pinned host memory: a span of this size is not something a test should pin
TIERED_EXEMPT = {("mdl_bag_sample_tiered", "row_stride"), ("mdl_bag_pack_tiered", "row_stride"), ("mdl_bag_mean_tiered", "row_stride")}


def stride_arguments(protos):
    """{(entry point, argument)}: every int64_t row stride of a header, by the names the headers use for them."""
    import re
    pat = re.compile(r"ld[A-Za-z]*|[a-z]*_?rsb|row_stride")
    return {(name, p) for name, params in protos.items() for p, is_ptr, _ in params if not is_ptr and pat.fullmatch(p)}


# ========================================================================================================================== the layout
class WideLay:
    """A drop-in for Lay of tests/test_strides_gpu.py (inp / out / buf / track / check_padding).  An operand whose index k is in
    `target` is a column slice [rows, width] of `arena` (one uint8 tensor) seen, from byte `lead` on, as rows of ld * elem bytes: at
    the next free 16-byte-aligned column, at least GAP bytes of fill from its neighbours, all wide operands of a case side by side in
    the one span.  Every other operand goes to `small` (a Lay('pad')): exactly the targeted stride is extreme.

    The arena is filled with 0xFF (NaN as fp32 and as bf16) on construction.  check_padding(), after the caller has copied the
    outputs out: every input slice still equals its source; then every slice is overwritten with 0xFF and the WHOLE arena is compared
    with 0xFF as integers in chunks of at most 1 GiB -- no copy of the arena, nothing on the host unless a byte differs.  A wrapped
    32-bit offset can only lower an address; with `lead` >= 2^31 it then lands in fill or in another row, inside the allocation."""
    mode = "wide"

    def __init__(self, arena, target, ld, elem, small, lead=LEAD):
        assert arena.dtype == torch.uint8 and arena.dim() == 1 and arena.is_contiguous()
        assert arena.data_ptr() % 16 == 0 and lead % 16 == 0 and (ld * elem) % 16 == 0
        self.arena, self.target, self.pitch, self.lead, self.small = arena, frozenset(target), ld * elem, lead, small
        self.dev, self.col, self.slices = arena.device, GAP, []
        arena.fill_(FILL)

    # ------------------------------------------------------------------------------------------------------------------- operands
    def _slice(self, rows, width, dtype, k):
        isz = torch.empty((), dtype=dtype).element_size()
        wb, col = width * isz, _up(self.col, 16)
        assert self.pitch % isz == 0
        assert col + wb + GAP <= self.pitch, "the wide operands of this case do not fit side by side in one row"
        assert self.lead + rows * self.pitch <= self.arena.numel(), "the span does not fit the arena"
        off = self.lead + col
        raw = self.arena[off:off + (rows - 1) * self.pitch + wb]
        v = raw.view(dtype).as_strided((rows, width), (self.pitch // isz, 1))
        assert v.data_ptr() == self.arena.data_ptr() + off and v.data_ptr() % 16 == 0
        self.col = col + wb + GAP
        self.slices.append(dict(name="operand %d (k = %d, [%d, %d] %s)" % (len(self.slices), k, rows, width, str(dtype).split(".")[-1]),
                                rows=rows, col=col, wb=wb, view=v, bytes=self.arena.as_strided((rows, wb), (self.pitch, 1), off), src=None))
        return v

    def buf(self, rows, width, dtype, k):
        if k in self.target:
            return self.arena, self._slice(rows, width, dtype, k)
        return self.small.buf(rows, width, dtype, k)

    def inp(self, x, k=0, dtype=None):
        if k not in self.target:
            return self.small.inp(x, k, dtype)
        src = x.to(device=self.dev, dtype=dtype or x.dtype).contiguous()
        v = self._slice(x.shape[0], x.shape[1], src.dtype, k)
        v.copy_(src)
        self.slices[-1]["src"] = src.view(torch.uint8).view(x.shape[0], -1).clone()
        return v

    def out(self, rows, width, dtype=torch.float32, k=0, init=None):
        if k not in self.target:
            return self.small.out(rows, width, dtype, k, init)
        v = self._slice(rows, width, dtype, k)
        if init is not None:
            v.copy_(init.to(self.dev))
        return v

    def track(self, v_of_b):
        if v_of_b[0] is not self.arena:       # (a wide slice is already known)
            self.small.track(v_of_b)

    # ---------------------------------------------------------------------------------------------------------------------- checks
    def far_rows(self, mark_bytes):
        """How many rows of the tallest wide operand start at least `mark_bytes` from the operand's base."""
        rows = max(s["rows"] for s in self.slices)
        return sum(1 for i in range(rows) if i * self.pitch >= mark_bytes)

    def where(self, pos):
        """Names byte `pos` of the arena: the nearest slice, the row and the column offset relative to the slice."""
        if pos < self.lead:
            return "byte %d of the arena, in the lead, %d bytes before the first row" % (pos, self.lead - pos)
        row, colb = divmod(pos - self.lead, self.pitch)

        def dist(s):
            return 0 if s["col"] <= colb < s["col"] + s["wb"] else min(abs(colb - s["col"]), abs(colb - (s["col"] + s["wb"] - 1)))
        s = min(self.slices, key=dist) if self.slices else None
        if s is None:
            return "byte %d of the arena: row %d, column byte %d (no slice)" % (pos, row, colb)
        place = "behind the last row" if row >= s["rows"] else "in the fill beside it" if dist(s) else "inside it"
        return "byte %d of the arena: nearest %s, row %d of %d, column byte offset %d, %s" % (pos, s["name"], row, s["rows"], colb - s["col"], place)

    def scan(self):
        """Every byte of the arena is 0xFF, compared as int64 in chunks of at most SCAN_CHUNK bytes; names the first that is not."""
        n, flags, spans = self.arena.numel(), [], []
        for lo in range(0, n, SCAN_CHUNK):
            c = self.arena[lo:min(n, lo + SCAN_CHUNK)]
            m = c.numel() // 8 * 8
            f = (c[:m].view(torch.int64) != -1).any()
            if m < c.numel():
                f = f | (c[m:] != FILL).any()
            flags.append(f)
            spans.append((lo, lo + c.numel()))
        bad = torch.stack(flags).cpu()
        if not bool(bad.any()):
            return
        lo, hi = spans[int(torch.nonzero(bad)[0])]
        step = 1 << 24
        for a in range(lo, hi, step):                         # (only on failure: finds the byte)
            hit = torch.nonzero(self.arena[a:min(hi, a + step)] != FILL)
            if hit.numel():
                total = sum(int((self.arena[x:min(n, x + step)] != FILL).sum()) for x in range(0, n, step))
                raise AssertionError("a kernel wrote outside every valid slice: %s; %d bytes changed in all" % (self.where(a + int(hit[0])), total))
        raise AssertionError("the arena scan disagrees with itself")

    def check_padding(self):
        for s in self.slices:
            if s["src"] is not None:
                assert torch.equal(s["bytes"], s["src"]), "a kernel changed an input: %s" % s["name"]
        for s in self.slices:
            s["bytes"].fill_(FILL)
        self.scan()
        self.small.check_padding()
