"""torch.autograd.Function wrappers over the C ABI (include/madeleine_amd.h).

PyTorch is plumbing here: it owns device memory, the stream and the autograd graph; every numeric
step of the hot path below runs in libmadeleine_amd.so.  Tensors are contiguous, on a ROCm device, fp32 --
or, for the activation tensors of the bf16 mode (E, LayerNorm input/output), bfloat16, which selects the *_bf16 entry
points; anything else raises (there is no CPU or eager fallback).

Layouts (see include/madeleine_amd.h): token embeddings are head-major [T, H*512]; scores [T, H].
"""
import collections
import contextlib
import ctypes
import os
import threading
from typing import Optional

import torch

from . import _native

HID = 512


def _ptr(t: Optional[torch.Tensor]):
    """What _call passes for one tensor argument (for callers that bind an entry point themselves)."""
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


_ENTRY = {}   # name -> bound entry point, resolved once: a process loads one library (_native.lib() never replaces its handle)


def _entry(name):
    fn = _ENTRY[name] = getattr(_native.lib(), name)
    return fn


def _call(name, *args, unsupported=None):
    """The one way into the library: calls entry point `name` (the name actually called, _bf16 suffix included) and raises under that
    name on a non-zero return code.  A tensor argument goes in as its device address; None (a NULL pointer), numbers and host arrays
    as they are -- in one comprehension, this runs for every launch of a host-bound step.  unsupported = (text, values...): the
    NotImplementedError of a call site where MDL_E_UNSUPPORTED is the refusal of a geometry, formatted only when it is raised."""
    rc = (_ENTRY.get(name) or _entry(name))(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args])
    if rc != 0:
        if rc == _native._E_UNSUPPORTED and unsupported is not None:
            raise NotImplementedError(unsupported[0] % unsupported[1:])
        _native.check(rc, name)


ACT_DTYPES = (torch.float32, torch.bfloat16)   # storage types of the activation tensors (parity mode / bf16 mode)


def _sfx(t: torch.Tensor) -> str:
    """C-ABI entry-point suffix for the storage type of an activation tensor."""
    return "_bf16" if t.dtype == torch.bfloat16 else ""


def _require_act(t: torch.Tensor, name: str):
    if t.dtype not in ACT_DTYPES:
        raise RuntimeError("madeleine_amd: %s must be float32 or bfloat16 (got %s)" % (name, t.dtype))
    return _require(t, name, t.dtype)


def _require(t: torch.Tensor, name: str, dtype=torch.float32):
    if not t.is_cuda:
        raise RuntimeError(
            "madeleine_amd: %s must live on a ROCm device (got %s); the HIP kernels are the only backend" % (name, t.device))
    if t.dtype != dtype:
        raise RuntimeError("madeleine_amd: %s must be %s (got %s)" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise RuntimeError("madeleine_amd: %s must be contiguous" % name)
    return t


class KernelTimer:
    """Optional per-call HIP-event timing of the C-ABI launches (bench.py's roofline leg).  Events are recorded
    on the stream the kernels are launched on (torch's current stream); nothing is synchronised until report().
    A call may declare its algorithmic work -- ("flop", n) for the matrix-core contractions, ("byte", n) for the HBM-bound
    passes -- so that bench.py can print achieved TFLOP/s / GB/s per kernel family (work())."""

    def __init__(self, only=None):
        """only: names to time (None = every call).  bench.py's headline region times the A3 forward alone -- one event pair per
        step -- so that the fused backward runs as ONE call and no per-launch events sit in the measured step."""
        self.pairs = {}
        self.works = {}
        self.only = None if only is None else frozenset(only)

    def wants(self, name) -> bool:
        return self.only is None or name in self.only

    def start(self, name, work=None):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.pairs.setdefault(name, []).append((ev0, ev1))
        if work is not None:
            kind, amount = work
            w = self.works.setdefault(name, [kind, 0.0, 0])
            w[1] += float(amount)
            w[2] += 1
        ev0.record()
        return ev1

    def report(self):
        torch.cuda.synchronize()
        return {k: (sum(a.elapsed_time(b) for a, b in v) / len(v), len(v)) for k, v in self.pairs.items()}

    def work(self):
        """{name: (kind, work per call on average)} for the calls that declared it."""
        return {k: (w[0], w[1] / max(1, w[2])) for k, w in self.works.items()}


TIMER: Optional[KernelTimer] = None


class PoolDispatchTimer:
    """Execution time of the A3 forward's two kernels (pool_partial, pool_combine) from the dispatches' own begin / end events
    (mdl_pool_timer_arm / _read: hipExtLaunchKernel start / stop events on the launch stream) -- what rocprofv3 --kernel-trace
    reports for them, not the distance between two markers in a busy stream.  Every pooling forward issued while POOL_TIMER is set
    takes the next of 64 slots; nothing is synchronised until report()."""
    SLOTS = 64

    def __init__(self):
        self.n = 0

    def arm(self):
        _call("mdl_pool_timer_arm", self.n % self.SLOTS)
        self.n += 1

    def report(self):
        """[(pool_partial ms, pool_combine ms, first start -> last end ms)] of the last min(calls, 64) pooling forwards."""
        import ctypes
        out = []
        for i in range(max(0, self.n - self.SLOTS), self.n):
            ms = (ctypes.c_float * 3)()
            _call("mdl_pool_timer_read", i % self.SLOTS, ms)
            out.append((float(ms[0]), float(ms[1]), float(ms[2])))
        return out


POOL_TIMER: Optional[PoolDispatchTimer] = None


class _timed:
    def __init__(self, name, work=None):
        self.name, self.work = name, work

    def __enter__(self):
        self.ev = TIMER.start(self.name, self.work) if TIMER is not None and TIMER.wants(self.name) else None
        if POOL_TIMER is not None and self.name == "pool_fwd":
            POOL_TIMER.arm()

    def __exit__(self, *exc):
        if self.ev is not None:
            self.ev.record()
        return False


def _ws(nbytes: int, device) -> torch.Tensor:
    if nbytes < 0:
        raise RuntimeError("madeleine_amd: workspace query failed (%d)" % nbytes)
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def _ws_for(query, device, *sizes, refusal=None) -> torch.Tensor:
    """The workspace whose size the mdl_*_ws_bytes entry point `query` gives for `sizes`.  These host-only queries return a byte count,
    not a return code, which is why they do not go through _call.  refusal = (text, values...): the NotImplementedError where
    MDL_E_UNSUPPORTED from the query is the refusal of a geometry."""
    nbytes = (_ENTRY.get(query) or _entry(query))(*sizes)
    if nbytes == _native._E_UNSUPPORTED and refusal is not None:
        raise NotImplementedError(refusal[0] % refusal[1:])
    return _ws(nbytes, device)


_LN_WIDTHS = "fused LayerNorm-GELU-Dropout supports widths 256/512/1024/2048/4096 (got %d)"


def _gate_grads(Wa, Wb):
    """Uninitialised (dWa, dWb, dba, dbb, dwc, dbc) of the gate parameters Wa, Wb [H,512,512]."""
    H, dev = Wa.shape[0], Wa.device
    dWa, dWb = torch.empty_like(Wa), torch.empty_like(Wb)
    dba = torch.empty(H, HID, device=dev, dtype=torch.float32)
    dbb, dwc = torch.empty_like(dba), torch.empty_like(dba)
    dbc = torch.empty(H, device=dev, dtype=torch.float32)
    return dWa, dWb, dba, dbb, dwc, dbc


def _pool_outputs(n_out, H, device, pooled_shape=None):
    """Uninitialised (pooled [n_out, H*512] or `pooled_shape`, stat_m, stat_l [n_out, H]) of a pooling forward over n_out bags / views."""
    pooled = torch.empty(pooled_shape or (n_out, H * HID), device=device, dtype=torch.float32)
    stat_m = torch.empty(n_out, H, device=device, dtype=torch.float32)
    stat_l = torch.empty(n_out, H, device=device, dtype=torch.float32)
    return pooled, stat_m, stat_l


def h2d(t: torch.Tensor, device, dtype=None) -> torch.Tensor:
    """Host tensor -> device WITHOUT blocking the host.  A copy from pageable memory (`t.to(device, non_blocking=True)` on an
    ordinary CPU tensor) is stream-ordered AND synchronous for the caller: the host stalls until the GPU has drained everything queued
    before it -- in the pretrain step that was the whole encoder forward (8 ms at config 2, 21 ms at config 3: the host then fed
    the loss section launch by launch and the device idled between them).  Staged through a pinned buffer (PyTorch's caching host
    allocator keeps it alive until the copy has run) the copy is a queued DMA and the host stays ahead of the device."""
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    dev = torch.device(device)
    if t.device.type != "cpu" or dev.type != "cuda" or os.environ.get("MADELEINE_BLOCKING_H2D"):
        return t.to(dev)
    return t.contiguous().pin_memory().to(dev, non_blocking=True)


def new_dropout_seed() -> int:
    """Draws a 63-bit seed from torch's CPU generator (deterministic under torch.manual_seed)."""
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())


# --------------------------------------------------------------------------------------------------
# raw calls (no autograd)
# --------------------------------------------------------------------------------------------------
def _gate_src(E):
    """(entry-point suffix, leading arguments, token rows, element type of the saved activations) of a gate call on E: an fp32 / bf16
    tensor [T, ldE], or the split image of one."""
    if isinstance(E, SplitImage):
        return "_split", (E.data, E.K * 4, E.scale), E.rows, torch.float32
    return _sfx(E), (E, E.stride(0)), E.shape[0], E.dtype


def gate_fwd_raw(E, Wa, ba, Wb, bb, wc, bc, p_drop, seed, keep_a, keep_b, save_act: bool):
    """scores [T, H] (and the activations when save_act) of the gate on E: a tensor, or a SplitImage for the split engine."""
    sfx, src, T, act_dtype = _gate_src(E)
    H, dev = Wa.shape[0], Wa.device
    scores = torch.empty(T, H, device=dev, dtype=torch.float32)
    act_a = torch.empty(T, H, HID, device=dev, dtype=act_dtype) if save_act else None
    act_b = torch.empty(T, H, HID, device=dev, dtype=act_dtype) if save_act else None
    ws = _ws_for("mdl_abmil_gate_fwd%s_ws_bytes" % sfx, dev, T, H)
    with _timed("gate_fwd", ("flop", 2.0 * T * H * HID * 2 * HID)):
        _call("mdl_abmil_gate_fwd" + sfx, *src, Wa, ba, Wb, bb, wc, bc, scores, act_a, act_b, T, H, float(p_drop), int(seed), keep_a, keep_b,
              ws, _stream())
    return scores, act_a, act_b


def gate_bwd_raw(E, Wa, Wb, wc, act_a, act_b, d_scores, dE, p_drop, seed, keep_a, keep_b, pool=None, accumulate=0, dE_absmax=None,
                 phases=None):
    """Gate backward on E (a tensor, or a SplitImage for the split engine) -> (dWa, dWb, dba, dbb, dwc, dbc); dE is written, or added to
    with `accumulate` (another consumer's gradient of E already sits there).  pool = (scores, stat_m, stat_l, d_pooled, row_bag, N): the
    dX epilogue also adds the pooling term (mdl_abmil_attnpool_bwd), so dE is written once.  dE_absmax (split engine): raised to
    max |dE|.  phases: a sequence of phase masks issued one after the other on the same workspace (include/madeleine_amd.h: 1 = dz pass,
    2 = both contractions; split engine also 4 = dX alone, 8 = dW alone); None = one call.  A tensor without a pooling term goes through
    mdl_abmil_gate_bwd, which has no phases."""
    sfx, src, T, _ = _gate_src(E)
    H = Wa.shape[0]
    split = isinstance(E, SplitImage)
    if not split and (dE_absmax is not None or (pool is None and phases is not None)):
        raise ValueError("gate_bwd_raw: dE_absmax needs a SplitImage, phases a SplitImage or a pooling term")
    grads = _gate_grads(Wa, Wb)
    ws = _ws_for("mdl_abmil_gate_bwd%s_ws_bytes" % sfx, dE.device, T, H)
    args = (Wa, Wb, wc, act_a, act_b, d_scores, dE) + ((dE.stride(0),) if split else ()) + (int(accumulate), *grads, T, H, float(p_drop),
                                                                                           int(seed), keep_a, keep_b)
    if not split and pool is None:
        with _timed("gate_bwd", ("flop", 4.0 * T * H * HID * 2 * HID)):
            _call("mdl_abmil_gate_bwd" + sfx, *src, *args, ws, _stream())
        return grads
    pool = tuple(pool[:5]) + (int(pool[5]),) if pool is not None else (None,) * 5 + (0,)

    def call(ph):
        if split:
            _call("mdl_abmil_attnpool_bwd_split", *src, *args, *pool, dE_absmax, ws, _stream(), 3 if ph is None else ph, GRAD_TERMS)
        elif ph is None:
            _call("mdl_abmil_attnpool_bwd" + sfx, *src, *args, *pool, ws, _stream())
        else:
            _call("mdl_abmil_attnpool_bwd_phases" + sfx, *src, *args, *pool, ws, _stream(), ph)
    if phases is not None:
        for ph in phases:
            call(int(ph))
    elif TIMER is not None and TIMER.wants("gate_bwd_dz"):
        # profiling: the HBM-bound dz pass and the MFMA-bound contractions as two calls on the same workspace, timed separately
        # ("gate_bwd" stays their sum in KernelTimer.report)
        with _timed("gate_bwd_dz", ("byte", float(T) * H * 4 * HID * act_a.element_size())):   # reads a, b; writes dza | dzb
            call(1)
        with _timed("gate_bwd_gemm", ("flop", 4.0 * T * H * HID * 2 * HID)):
            call(2)
    else:
        call(None)
    return grads


def _pool_src(E):
    """(entry-point suffix, leading arguments) of a pooling call on E: an fp32 / bf16 tensor [T, ldE], or the split image of one."""
    if isinstance(E, SplitImage):
        return "_img", (E.data, E.K * 4, E.scale)
    return _sfx(E), (E, E.stride(0))


def _pool_fwd(stem, timed, E, scores, n_out, max_len, bags, pooled_shape=None):
    """The pooling forward mdl_abmil_<stem><suffix of E> over n_out bags or segments of at most max_len tokens -> (pooled, stat_m,
    stat_l).  bags: what the entry point takes between its outputs and H; timed: the arguments of _timed."""
    sfx, src = _pool_src(E)
    H = scores.shape[-1]
    out = _pool_outputs(n_out, H, scores.device, pooled_shape)
    ws = _ws_for("mdl_abmil_pool_ws_bytes", scores.device, n_out, max_len, H)
    with _timed(*timed):
        _call("mdl_abmil_%s%s" % (stem, sfx), *src, scores, *out, *bags, H, ws, _stream())
    return out


def _pool_bwd(stem, timed, E, scores, grads, bags):
    """The pooling backward mdl_abmil_<stem><suffix of E>.  grads: what the entry point takes between the scores and `bags`."""
    sfx, src = _pool_src(E)
    with _timed(*timed):
        _call("mdl_abmil_%s%s" % (stem, sfx), *src, scores, *grads, *bags, scores.shape[-1], _stream())


def _pool_bytes(rows, H, row_bytes, n_bags):
    """("byte", n): the HBM traffic of a whole-bag pooling pass that moves row_bytes per token and head, and one pooled row per bag."""
    return "byte", float(rows) * H * row_bytes + n_bags * H * HID * 4.0


def pool_fwd_raw(E2d, scores, n_bags, N, cu_seqlens, max_len):
    H = scores.shape[-1]
    work = _pool_bytes(E2d.shape[0], H, HID * E2d.element_size() + 4, n_bags)
    return _pool_fwd("pool_fwd", ("pool_fwd", work), E2d, scores, n_bags, max_len, (n_bags, N, cu_seqlens, max_len))


def pool_bwd_raw(E2d, scores, pooled, stat_m, stat_l, d_pooled, dE, accumulate, d_scores, accumulate_scores, n_bags, N,
                 cu_seqlens, max_len):
    H = scores.shape[-1]
    work = _pool_bytes(E2d.shape[0], H, HID * E2d.element_size() * (1 if dE is None else 2) + 8, n_bags)
    _pool_bwd("pool_bwd", ("pool_bwd", work), E2d, scores,
              (pooled, stat_m, stat_l, d_pooled, dE, int(accumulate), d_scores, int(accumulate_scores)), (n_bags, N, cu_seqlens, max_len))


def pool_fwd_img_raw(Ei, scores, n_bags, N, cu_seqlens, max_len):
    """pool_fwd_raw on the split image of E (the split GEMM mode stores E as an image only)."""
    work = _pool_bytes(Ei.rows, scores.shape[-1], HID * 4 + 4, n_bags)
    return _pool_fwd("pool_fwd", ("pool_fwd", work), Ei, scores, n_bags, max_len, (n_bags, N, cu_seqlens, max_len))


def pool_dscores_img_raw(Ei, scores, pooled, stat_m, stat_l, d_pooled, d_scores, accumulate_scores, n_bags, N, cu_seqlens, max_len):
    """The score gradients of the pooling from the split image of E (pool_bwd_raw with dE = None)."""
    work = _pool_bytes(Ei.rows, scores.shape[-1], HID * 4 + 8, n_bags)
    _pool_bwd("pool_dscores", ("pool_bwd", work), Ei, scores, (pooled, stat_m, stat_l, d_pooled, d_scores, int(accumulate_scores)),
              (n_bags, N, cu_seqlens, max_len))


def pool_view_fwd_raw(E2d, scores, n_bags, N, token_idx):
    n_idx = token_idx.numel()
    return _pool_fwd("pool_view_fwd", ("pool_view_fwd",), E2d, scores, n_bags, n_idx, (n_bags, N, token_idx, n_idx))


def pool_view_bwd_raw(E2d, scores, pooled, stat_m, stat_l, d_pooled, dE, d_scores, n_bags, N, token_idx):
    """Accumulates the view's contribution into dE and / or d_scores (either may be None)."""
    _pool_bwd("pool_view_bwd", ("pool_view_bwd",), E2d, scores, (pooled, stat_m, stat_l, d_pooled, dE, d_scores),
              (n_bags, N, token_idx, token_idx.numel()))


def pool_rview_fwd_raw(E2d, scores, n_bags, perm, vcu, max_view_len):
    """The two half-bag views of every packed bag (mdl_abmil_pool_rview_fwd): -> (pooled [n_bags, 2, H*512], stat_m, stat_l [2*n_bags, H])."""
    return _pool_fwd("pool_rview_fwd", ("pool_view_fwd",), E2d, scores, 2 * n_bags, max_view_len, (n_bags, perm, vcu, int(max_view_len)),
                     pooled_shape=(n_bags, 2, scores.shape[-1] * HID))


def pool_rview_bwd_raw(E2d, scores, pooled, stat_m, stat_l, d_pooled, dE, d_scores, n_bags, perm, vcu, max_view_len):
    """Accumulates the ragged views' contribution (d_pooled [n_bags, 2, H*512]) into dE and / or d_scores (either may be None)."""
    _pool_bwd("pool_rview_bwd", ("pool_view_bwd",), E2d, scores, (pooled, stat_m, stat_l, d_pooled, dE, d_scores),
              (n_bags, perm, vcu, int(max_view_len)))


def _check_rview(E2d, cu_seqlens, rviews):
    perm, vcu, max_view_len = rviews
    if cu_seqlens is None:
        raise ValueError("ragged views (perm, vcu) need packed bags with cu_seqlens")
    _require(perm, "view permutation", torch.int32)
    _require(vcu, "view offsets", torch.int64)
    if perm.numel() != E2d.shape[0] or vcu.numel() != 2 * (cu_seqlens.numel() - 1) + 1:
        raise ValueError("ragged views: perm must cover every packed row [T] and vcu hold 2 * n_bags + 1 offsets")
    return perm, vcu, int(max_view_len)


# --------------------------------------------------------------------------------------------------
# split-fp16 engine (include/madeleine_amd.h, csrc/split_engine.hpp): fp32-accurate contractions on v_mfma_f32_32x32x16_f16
# --------------------------------------------------------------------------------------------------
GEMM_MODE = os.environ.get("MADELEINE_GEMM", "split")   # "split": 3-term split-fp16 products; "fp32": v_mfma_f32_32x32x2_f32


def gemm_mode() -> str:
    return GEMM_MODE


# Activation recomputation for the fused A2 + A3 node (opt-in; MADELEINE_GATE_RECOMPUTE=1 or set_gate_recompute(True)): the gate forward
# then saves NO tanh / sigmoid activations (2 x 8 KiB per token at H = 4: 4.3 GB per config-2 step, 10.7 GB at config 3) and the
# backward runs the gate forward once more (same seed -> same dropout masks, same bits) to rebuild them -- memory for time
# (+1 gate forward per step).  The default keeps the activations: with 288 GB of HBM the step's 60 GiB at config 3 fit many times over.
GATE_RECOMPUTE = os.environ.get("MADELEINE_GATE_RECOMPUTE", "0") == "1"


# Matrix terms of the split engine's BACKWARD products (opt-in; MADELEINE_GRAD_TERMS=2 or set_gradient_terms(2)).  3: every product is
# ah bh + ah bl + al bh.  2: in dX = dY W the weight, and in dW = dY^T X the activations, enter rounded to their hi plane (11 bits) --
# a third fewer matrix instructions in the backward, gradients at ~2^-12 relative instead of ~2^-22; the forward (every value the
# losses and the caller see) is untouched.  Measured in DESIGN.md 3.7; never the default.
GRAD_TERMS = int(os.environ.get("MADELEINE_GRAD_TERMS", "3"))


def set_gradient_terms(terms: int):
    global GRAD_TERMS
    if terms not in (2, 3):
        raise ValueError("gradient terms: 2 or 3")
    GRAD_TERMS = int(terms)


def set_gate_recompute(on: bool):
    global GATE_RECOMPUTE
    GATE_RECOMPUTE = bool(on)


def set_gemm_mode(mode: str):
    """'split' (default): the fp32 contractions run as ah bh + ah bl + al bh on the fp16 matrix cores (fp32-level accuracy, ~2x the
    rate); 'fp32': the exact-fp32 matrix-core kernels (v_mfma_f32_32x32x2_f32)."""
    global GEMM_MODE
    if mode not in ("split", "fp32"):
        raise ValueError("gemm mode must be 'split' or 'fp32'")
    GEMM_MODE = mode


class SplitImage:
    """Split image of a [rows, K] fp32 tensor: `data` float32 [rows + pad, K] (opaque bytes: per 32-column block the fp16 hi plane
    | lo plane), `scale` float32 [2] = {scale, absmax} on the device."""
    __slots__ = ("data", "scale", "rows", "K", "row_inv")

    def __init__(self, data, scale, rows, K, row_inv=None):
        # row_inv [rows] (row-scaled images only): 1 / the power-of-two scale of every row; the common `scale` of such an image is 1
        self.data, self.scale, self.rows, self.K, self.row_inv = data, scale, rows, K, row_inv


def split_image(x2d, pad_rows=0) -> SplitImage:
    _require(x2d, "x")
    rows, K = x2d.shape
    data = torch.empty(rows + pad_rows, K, device=x2d.device, dtype=torch.float32)
    scale = torch.empty(2, device=x2d.device, dtype=torch.float32)
    with _timed("split_image", ("byte", 12.0 * rows * K)):   # absmax read + convert read + write
        _call("mdl_split_image", x2d, x2d.stride(0), rows, K, data, K * 4, pad_rows, scale, _stream())
    return SplitImage(data, scale, rows, K)


def split_image_rows(x2d, pad_rows=0):
    """Row-scaled image of x2d (mdl_split_image_rows): -> (SplitImage with common scale 1, row_inv [rows] = 1 / the row scales).  For the
    tensor whose rows the caller controls (the patch features): one outlier patch does not cost the other patches their low bits."""
    _require(x2d, "x")
    rows, K = x2d.shape
    data = torch.empty(rows + pad_rows, K, device=x2d.device, dtype=torch.float32)
    row_inv = torch.empty(rows, device=x2d.device, dtype=torch.float32)
    # scale = NULL: nothing consumes the tensor-wide maximum of a row-scaled image, and collecting it is a memset, a scale launch and one
    # atomic per wave on a single address (75 us of a 95-us launch at 30,000 rows: every wave arrives at once)
    with _timed("split_image", ("byte", 8.0 * rows * K)):   # one HBM read + write
        _call("mdl_split_image_rows", x2d, x2d.stride(0), rows, K, data, K * 4, pad_rows, row_inv, None, _stream())
    return SplitImage(data, _unit_scale(x2d.device), rows, K), row_inv


_UNIT_SCALE = {}


def _unit_scale(device):
    """The constant {1, 0} on `device`: the common scale of a row-scaled image (one tensor per device, never written)."""
    key = str(device)
    if key not in _UNIT_SCALE:
        _UNIT_SCALE[key] = torch.tensor([1.0, 0.0], device=device, dtype=torch.float32)
    return _UNIT_SCALE[key]


def weight_image(W) -> SplitImage:
    """Row-scaled image of a weight matrix W [N, K] (one power of two per output channel) in ONE launch -- instead of the memset, absmax,
    scale and convert launches of split_image, every forward and backward of every Linear.  As the B operand of split_gemm_nt its row
    factors become per-output-column factors of the product (b_col_mul)."""
    _require(W, "weight")
    rows, K = W.shape
    data = torch.empty(rows, K, device=W.device, dtype=torch.float32)
    row_inv = torch.empty(rows, device=W.device, dtype=torch.float32)
    _call("mdl_split_image_rows", W, W.stride(0), rows, K, data, K * 4, 0, row_inv, None, _stream())
    return SplitImage(data, _unit_scale(W.device), rows, K, row_inv)


def split_tile_absmax(x2d, chunks=False):
    """max |x| of every block of 256 rows (the row gate of split_gemm_nt); chunks=True: also of every 32 rows (split_gemm_tn's
    b_chunk_max) -> (gate, chunk_max)."""
    rows, K = x2d.shape
    gate = torch.empty((rows + 255) // 256, device=x2d.device, dtype=torch.float32)
    cm = torch.empty((rows + 31) // 32, device=x2d.device, dtype=torch.float32) if chunks else None
    _call("mdl_split_tile_absmax", x2d, x2d.stride(0), rows, K, gate, cm, _stream())
    return (gate, cm) if chunks else gate


def split_gemm_nt(A: SplitImage, B: SplitImage, bias=None, out=None, accumulate=False, absmax_out=None, name="split_nt", row_gate=None,
                  a_row_mul=None, terms=3):
    """C [A.rows, B.rows] (+)= A B^T (+ bias) on two images with the same K.  row_gate (accumulate mode only): per-256-row maxima of
    the tensor A is the image of; output tiles of all-zero A rows are skipped.  a_row_mul [A.rows]: per-row factor applied to the
    product (row_inv of a row-scaled A image).  terms=2: B enters with its hi plane only (GRAD_TERMS)."""
    M, N, K = A.rows, B.rows, A.K
    if B.K != K:
        raise ValueError("split_gemm_nt: contraction lengths differ")
    if a_row_mul is None:
        a_row_mul = A.row_inv
    C = out if out is not None else torch.empty(M, N, device=A.data.device, dtype=torch.float32)
    with _timed(name, ("flop", 2.0 * M * N * K)):
        _call("mdl_split_gemm_nt", A.data, K * 4, A.scale, B.data, K * 4, B.scale, C, C.stride(0), M, N, K, bias, int(accumulate),
              absmax_out, row_gate, a_row_mul, B.row_inv, int(terms), _stream())
    return C


def split_gemm_nt_group_bias(A: SplitImage, B: SplitImage, group_bias, row_group, bias=None, a_row_mul=None, name="split_nt"):
    """split_gemm_nt with a bias row per GROUP of output rows: C[m] = A[m] B^T (+ bias) + group_bias[row_group[m]] (mdl_split_gemm_nt_group_bias;
    group_bias [G, B.rows] fp32, row_group int32 [A.rows])."""
    M, N, K = A.rows, B.rows, A.K
    if B.K != K:
        raise ValueError("split_gemm_nt_group_bias: contraction lengths differ")
    _require(group_bias, "group_bias")
    _require(row_group, "row_group", torch.int32)
    if group_bias.dim() != 2 or group_bias.shape[1] != N or row_group.numel() != M:
        raise ValueError("split_gemm_nt_group_bias: group_bias must be [G, %d] and row_group [%d]" % (N, M))
    if a_row_mul is None:
        a_row_mul = A.row_inv
    C = torch.empty(M, N, device=A.data.device, dtype=torch.float32)
    with _timed(name, ("flop", 2.0 * M * N * K)):
        _call("mdl_split_gemm_nt_group_bias", A.data, K * 4, A.scale, B.data, K * 4, B.scale, C, C.stride(0), M, N, K, bias, a_row_mul,
              B.row_inv, group_bias, row_group, 3, _stream())
    return C


def split_gemm_tn(A: SplitImage, B: SplitImage, name="split_tn", b_chunk_max=None, terms=3):
    """out [B.K, A.K] = B^T A summed over the rows (tokens) of the two images; B must carry >= 32 zero pad rows.  b_chunk_max: the
    per-32-row maxima (split_tile_absmax(x, chunks=True)) of the tensor B is the image of -- its all-zero chunks are skipped."""
    T, Mi, N = A.rows, A.K, B.K
    if B.row_inv is not None:
        raise ValueError("split_gemm_tn: a row-scaled image cannot be the B operand of a contraction over its rows")
    if B.rows != T or B.data.shape[0] < T + 32:
        raise ValueError("split_gemm_tn: images need the same number of rows and B 32 zero pad rows")
    out = torch.empty(N, Mi, device=A.data.device, dtype=torch.float32)
    ws = _ws_for("mdl_split_gemm_tn_ws_bytes", A.data.device, T, Mi, N)
    with _timed(name, ("flop", 2.0 * T * Mi * N)):
        _call("mdl_split_gemm_tn", A.data, Mi * 4, A.scale, Mi, B.data, N * 4, B.scale, N, out, T, b_chunk_max, ws, int(terms), _stream())
    return out


def _split_gate(E2d) -> bool:
    """The gate (A2) contractions take the split engine for fp32 token embeddings in the 'split' GEMM mode."""
    return GEMM_MODE == "split" and E2d.dtype == torch.float32 and E2d.shape[0] > 0


def split_linear_supported(T, N, K) -> bool:
    """Geometries the split engine takes for a Linear [T,K] x [N,K]: fwd K % 32, N % 4; dX: N % 32 (contraction), K % 4; dW: both % 32."""
    return T > 256 and K % 32 == 0 and N % 32 == 0


class SplitLinearFn(torch.autograd.Function):
    """LinearFn in the split GEMM mode: Y = X W^T (+ bias) with fp32 inputs / outputs, the contraction on the split-fp16 engine.
    x may be given as a ready SplitImage (`x_img`, from a producer kernel that writes images directly); otherwise it is built here."""

    @staticmethod
    def forward(ctx, x, W, bias):
        _require(x, "x")
        _require(W, "weight")
        if bias is not None:
            _require(bias, "bias")
        xi = split_image(x)
        y = split_gemm_nt(xi, weight_image(W), bias, name="linear_fwd")
        ctx.save_for_backward(W, xi.data, xi.scale)     # (the image is an ordinary saved tensor: hooks, retain_graph, version checks)
        ctx.geom = (xi.rows, xi.K)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        W, xdata, xscale = ctx.saved_tensors
        xi = SplitImage(xdata, xscale, *ctx.geom)
        dy = dy.float().contiguous()
        dyi = split_image(dy, pad_rows=32)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = split_gemm_nt(dyi, weight_image(W.t().contiguous()), name="linear_bwd", terms=GRAD_TERMS)
        dW = split_gemm_tn(xi, dyi, name="linear_bwd", terms=GRAD_TERMS)
        db = dy.sum(0) if ctx.has_bias else None
        return dx, dW, db


# max |t| of a gradient tensor, published by the kernel that produced it (epilogue atomics) for the consumer that needs a bound on it.
# An entry binds to the CONTENTS of the buffer, not just its address: it keeps the producer's tensor alive (the address cannot be
# recycled for another tensor, and the autograd engine cannot steal the buffer to sum a second gradient into it in place -- it
# allocates the sum elsewhere, which misses here) and records the version counter the tensor had when the kernel wrote it (views share
# the counter: an in-place update by a hook or another consumer shows as a newer version).  A miss or a stale entry returns None and the
# consumer takes its own one-pass absmax (the dy_absmax = NULL path of mdl_ln_gelu_drop_bwd_split).
# The strong reference lives only as long as the backward pass that created it: the first entry of a pass queues an engine callback
# that empties the table when the outermost backward returns, so a consumer that never runs (frozen pre_attn, a hook that replaces the
# gradient, an exception) cannot pin a multi-GB gradient buffer until the next encoder forward.
_ABSMAX = {}
_ABSMAX_LOCK = threading.Lock()
_ABSMAX_CB = [False]


def _absmax_end_of_backward():
    with _ABSMAX_LOCK:
        _ABSMAX.clear()
        _ABSMAX_CB[0] = False


def _put_absmax(t, amax):
    with _ABSMAX_LOCK:
        if len(_ABSMAX) > 8:
            _ABSMAX.clear()
        _ABSMAX[(t.data_ptr(), t.numel())] = (t, t._version, amax)
        if not _ABSMAX_CB[0]:
            try:      # (only callable while the engine is running a backward -- which is where every producer lives)
                torch.autograd.Variable._execution_engine.queue_callback(_absmax_end_of_backward)
                _ABSMAX_CB[0] = True
            except RuntimeError:
                pass


def _take_absmax(t):
    with _ABSMAX_LOCK:
        e = _ABSMAX.pop((t.data_ptr(), t.numel()), None)
    if e is None:
        return None
    src, version, amax = e
    fresh = (src._version == version and t._version == version
             and src.untyped_storage().data_ptr() == t.untyped_storage().data_ptr())
    return amax if fresh else None


def _clear_absmax():
    # Start of an encoder forward.  Also re-arms the end-of-backward callback: when a backward raises, the engine skips its final
    # callbacks, so the flag set by _put_absmax would otherwise stay True for the life of the process.
    with _ABSMAX_LOCK:
        _ABSMAX.clear()
        _ABSMAX_CB[0] = False


class PreAttnBlockFn(torch.autograd.Function):
    """One block of the pre-attention MLP -- Linear -> LayerNorm -> GELU -> Dropout (Model.py:351-354, :355-358, :359-362) -- as ONE
    autograd node on the split engine.  The activations between the blocks exist as split images only (consumed by contractions):
    `x` is either the fp32 input of the first block (x_scale None) or the previous block's image (x_scale = its scale); the block
    returns (image [T,N] as an opaque float32 tensor, scale [2], fp32 output or an empty tensor).  Gradients travel as ordinary fp32
    tensors of the images' shape; in backward the LayerNorm kernel writes d(pre-LN) as an image straight away and the dX / dW
    contractions read it -- no conversion pass anywhere (scales come from rigorous bounds, include/madeleine_amd.h)."""

    @staticmethod
    def forward(ctx, x, x_scale, W, lin_bias, gamma, beta, eps, p_drop, seed, keep, want_fp32, gbias=None, row_group=None, cu_groups=None):
        # gbias [G, N] + row_group int32 [T] + cu_groups int64 [G + 1] (first block only, round 5): a bias row per GROUP of rows (= bag), rows of
        # a group contiguous -- the stain-encoding columns of MADELEINE's first Linear folded out of the contraction:
        # [x | e_g] W^T = x Wx^T + e_g We^T (Model.py:125-132, :351).  The concat [T, D + 32] never exists; the backward returns d(gbias).
        _require(x, "x")
        for t_, n_ in ((W, "weight"), (gamma, "gamma"), (beta, "beta")):
            _require(t_, n_)
        if lin_bias is not None:
            _require(lin_bias, "bias")
        T, K = x.shape
        N = W.shape[0]
        dev = x.device
        if x_scale is None:
            _clear_absmax()      # first block of an encoder forward: no published maximum outlives a step
        # first block: x = the caller's patch features -> ROW-scaled image (an outlier patch must not cost the others their low bits;
        # nn.Linear in fp32 has no coupling between rows); later blocks: the previous block's LayerNorm output, rows of one magnitude
        row_inv = None
        if x_scale is not None:
            xi = SplitImage(x, x_scale, T, K)
        else:
            xi, row_inv = split_image_rows(x)
        if gbias is not None:
            _require(cu_groups, "cu_groups", torch.int64)
            y = split_gemm_nt_group_bias(xi, weight_image(W), gbias.contiguous(), row_group, a_row_mul=row_inv, name="linear_fwd")
        else:
            y = split_gemm_nt(xi, weight_image(W), name="linear_fwd", a_row_mul=row_inv)   # pre-LN values (the Linear's bias is added by the LN kernel)
        img = torch.empty(T, N, device=dev, dtype=torch.float32)
        scale = torch.empty(2, device=dev, dtype=torch.float32)
        out = torch.empty(T, N, device=dev, dtype=torch.float32) if want_fp32 else None
        mean = torch.empty(T, device=dev, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        # max_r rstd[r] row_inv[r], a factor of the backward's image bound -- only when a backward can follow (inference: not even the
        # one atomic per workgroup)
        needs_bwd = any(ctx.needs_input_grad)
        rstd_max = torch.empty(1, device=dev, dtype=torch.float32) if needs_bwd else None
        with _timed("ln_gelu_drop_fwd", ("byte", (3.0 if want_fp32 else 2.0) * T * N * 4)):
            _call("mdl_ln_gelu_drop_fwd_split", y, lin_bias, gamma, beta, out, img, scale, mean, rstd, T, N, float(eps), float(p_drop),
                  int(seed), keep, row_inv, rstd_max, _stream(), unsupported=(_LN_WIDTHS, N))
        none = torch.empty(0)
        # (the keep mask and the group offsets are saved tensors too: an in-place change before the backward raises instead of being read)
        ctx.save_for_backward(xi.data, xi.scale, W, y, gamma, beta, mean, rstd, lin_bias if lin_bias is not None else none,
                              row_inv if row_inv is not None else none, rstd_max if rstd_max is not None else none,
                              keep if keep is not None else none, cu_groups if gbias is not None else none)
        ctx.cfg = (float(p_drop), int(seed), keep is not None, lin_bias is not None, bool(want_fp32), T, K, N, x_scale is not None)
        ctx.groups = None if gbias is None else int(gbias.shape[0])
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(scale)
        if want_fp32:
            ctx.mark_non_differentiable(img)      # the gradient arrives on the fp32 output
            return img, scale, out
        empty = x.new_empty(0)
        ctx.mark_non_differentiable(empty)
        return img, scale, empty

    @staticmethod
    def backward(ctx, d_img, _d_scale, d_out):
        xdata, xscale, W, y, gamma, beta, mean, rstd, lin_bias, row_inv, rstd_max, keep, cu_groups = ctx.saved_tensors
        p_drop, seed, has_keep, has_bias, want_fp32, T, K, N, x_is_image = ctx.cfg
        keep = keep if has_keep else None
        lin_bias = lin_bias if has_bias else None
        rstd_max = rstd_max if rstd_max.numel() else None
        # first block (row-scaled input image): the gradient image carries row_inv[r] dx[r][:], so that the row factors of the two images
        # cancel inside the dW contraction over rows
        row_inv = None if x_is_image else row_inv
        dy = d_out if want_fp32 else d_img
        if dy is None:
            dy = torch.zeros(T, N, device=y.device, dtype=torch.float32)
        dy = dy.float().contiguous().view(T, N)
        dev = y.device
        dximg = torch.empty(T + 32, N, device=dev, dtype=torch.float32)
        dxscale = torch.empty(2, device=dev, dtype=torch.float32)
        dg, db = torch.empty_like(gamma), torch.empty_like(beta)
        dbias = torch.empty_like(lin_bias) if has_bias else None
        amax = _take_absmax(dy)
        groups, d_gbias = (), None
        if ctx.groups is not None:
            G = ctx.groups
            d_gbias = torch.empty(G, N, device=dev, dtype=torch.float32)
            groups = (cu_groups, G, d_gbias)
        ws = _ws_for("mdl_ln_gelu_drop_bwd%s_ws_bytes" % ("_groups" if groups else ""), dev, T, N, *groups[1:2])

        def ln_bwd(passes, dximg, dxscale, dg, db, dbias, row_mul, rstd_max, *groups):
            # d(pre-LN) as an image under (dxscale, row_mul), and the parameter gradients
            with _timed("ln_gelu_drop_bwd", ("byte", passes * T * N * 4)):
                _call("mdl_ln_gelu_drop_bwd_split" + ("_groups" if groups else ""), y, lin_bias, gamma, beta, mean, rstd, dy, amax, dximg,
                      dxscale, dg, db, dbias, T, N, p_drop, seed, keep, row_mul, rstd_max, *groups, ws, _stream())

        ln_bwd(3.0 if amax is not None else 4.0, dximg, dxscale, dg, db, dbias, row_inv, rstd_max, *groups)   # (4: its own pass over dy for max |dy|)
        dyi = SplitImage(dximg, dxscale, T, N)
        dx = None
        if ctx.needs_input_grad[0]:
            am = torch.zeros(1, device=dev, dtype=torch.float32)
            dxi = dyi
            if row_inv is not None:
                # d(patch features) is wanted (stain-encoding tokens concatenated to the bags, Model.py:132; a caller differentiating
                # w.r.t. its features): the image above carries the dW pairing's row factors, under which a row's own gradient can sit
                # far below the image's scale.  A second pass writes d(pre-LN) under the common scale for this product alone.
                dximg2 = torch.empty(T + 32, N, device=dev, dtype=torch.float32)
                dxscale2 = torch.empty(2, device=dev, dtype=torch.float32)
                dg2, db2 = torch.empty_like(gamma), torch.empty_like(beta)
                ln_bwd(3.0, dximg2, dxscale2, dg2, db2, None, None, None)   # (no row factors: its own pass over rstd)
                dxi = SplitImage(dximg2, dxscale2, T, N)
            dx = split_gemm_nt(dxi, weight_image(W.t().contiguous()), absmax_out=am, name="linear_bwd", terms=GRAD_TERMS)
            if x_is_image:       # the consumer is the previous block's LayerNorm backward (this node's input was its image)
                _put_absmax(dx, am)
        dW = split_gemm_tn(SplitImage(xdata, xscale, T, K), dyi, name="linear_bwd", terms=GRAD_TERMS)
        return dx, None, dW, dbias, dg, db, None, None, None, None, None, d_gbias, None, None


def preattn_block(x, x_scale, W, lin_bias, gamma, beta, eps=1e-5, p_drop=0.0, seed=0, keep=None, want_fp32=False, group_bias=None,
                  row_group=None, cu_groups=None):
    return PreAttnBlockFn.apply(x, x_scale, W.contiguous(), None if lin_bias is None else lin_bias.contiguous(), gamma.contiguous(),
                                beta.contiguous(), float(eps), float(p_drop), int(seed), keep, bool(want_fp32), group_bias, row_group, cu_groups)


def preattn_split_supported(x2d, K) -> bool:
    """x2d: the [T, K] bags as the caller holds them (any floating dtype: they are widened to fp32 for the first block, no copy is made
    to answer this)."""
    return GEMM_MODE == "split" and x2d.is_cuda and x2d.is_floating_point() and x2d.shape[0] > 256 and K % 32 == 0


def linear_fwd_raw(x2d, W, bias):
    """Y = X W^T (+ bias) through mdl_linear_fwd / mdl_linear_fwd_bf16 (by the storage type of x2d)."""
    T, K = x2d.shape
    N = W.shape[0]
    sfx = _sfx(x2d)
    y = torch.empty(T, N, device=x2d.device, dtype=x2d.dtype)
    ws = _ws_for("mdl_linear_fwd%s_ws_bytes" % sfx, x2d.device, T, N, K)
    with _timed("linear_fwd", ("flop", 2.0 * T * N * K)):
        _call("mdl_linear_fwd" + sfx, x2d, x2d.stride(0), W, bias, y, N, T, N, K, ws, _stream())
    return y


def linear_bwd_raw(x2d, W, dy, dx, want_dbias):
    """(dW, dbias) of the Linear; dX is written into `dx` ([T,K], may be None)."""
    T, K = x2d.shape
    N = W.shape[0]
    sfx = _sfx(x2d)
    dW = torch.empty_like(W)
    db = torch.empty(N, device=x2d.device, dtype=torch.float32) if want_dbias else None
    ws = _ws_for("mdl_linear_bwd%s_ws_bytes" % sfx, x2d.device, T, N, K)
    with _timed("linear_bwd", ("flop", 2.0 * T * N * K * (2 if dx is not None else 1))):
        _call("mdl_linear_bwd" + sfx, x2d, x2d.stride(0), W, dy, N, dx, K, dW, db, T, N, K, ws, _stream())
    return dW, db


def _bag_geometry(E, cu_seqlens, max_len):
    """E is [n_bags,N,C] (dense) or [T,C] with cu_seqlens int64 [n_bags+1] (ragged)."""
    if cu_seqlens is None:
        if E.dim() != 3:
            raise ValueError("dense bags must be [n_bags, N, H*512]")
        n_bags, N = E.shape[0], E.shape[1]
        return n_bags, N, N, E.reshape(n_bags * N, E.shape[2])
    if E.dim() != 2:
        raise ValueError("ragged bags must be packed [T, H*512] with cu_seqlens")
    _require(cu_seqlens, "cu_seqlens", torch.int64)
    if max_len is None:
        raise ValueError("max_len is required with cu_seqlens (avoids a device sync)")
    return cu_seqlens.numel() - 1, 0, int(max_len), E


# --------------------------------------------------------------------------------------------------
# A2: gated attention scores
# --------------------------------------------------------------------------------------------------
class GateScoresFn(torch.autograd.Function):
    """scores[T,H] = gated-attention raw scores of all heads (abmil.py:41-52 per head)."""

    @staticmethod
    def forward(ctx, E2d, Wa, ba, Wb, bb, wc, bc, p_drop, seed, keep_a, keep_b):
        _require_act(E2d, "E")
        for t, n in ((Wa, "Wa"), (ba, "ba"), (Wb, "Wb"), (bb, "bb"), (wc, "wc"), (bc, "bc")):
            _require(t, n)
        need = any(ctx.needs_input_grad[:7])
        Ei = None
        if _split_gate(E2d):
            Ei = split_image(E2d)
        scores, act_a, act_b = gate_fwd_raw(Ei if Ei is not None else E2d, Wa, ba, Wb, bb, wc, bc, p_drop, seed, keep_a, keep_b, need)
        if need:
            none = torch.empty(0)
            ctx.save_for_backward(E2d, Wa, Wb, wc, act_a, act_b, Ei.data if Ei is not None else none, Ei.scale if Ei is not None else none,
                                  keep_a if keep_a is not None else none, keep_b if keep_b is not None else none)
            ctx.drop = (p_drop, seed, keep_a is not None, keep_b is not None)
            ctx.has_image = Ei is not None
        return scores

    @staticmethod
    def backward(ctx, d_scores):
        E2d, Wa, Wb, wc, act_a, act_b, Eidata, Eiscale, keep_a, keep_b = ctx.saved_tensors
        p_drop, seed, has_keep_a, has_keep_b = ctx.drop
        keep_a, keep_b = keep_a if has_keep_a else None, keep_b if has_keep_b else None
        d_scores = d_scores.float().contiguous()
        dE = torch.empty_like(E2d)
        src = SplitImage(Eidata, Eiscale, E2d.shape[0], E2d.shape[1]) if ctx.has_image else E2d
        dWa, dWb, dba, dbb, dwc, dbc = gate_bwd_raw(src, Wa, Wb, wc, act_a, act_b, d_scores, dE, p_drop, seed, keep_a, keep_b)
        return dE, dWa, dba, dWb, dbb, dwc, dbc, None, None, None, None


# --------------------------------------------------------------------------------------------------
# A3: softmax over patches + pooling
# --------------------------------------------------------------------------------------------------
class SoftmaxPoolFn(torch.autograd.Function):
    """pooled[b,c,:] = sum_t softmax_t(scores[b,:,c]) E[b,t,c,:]   (abmil.py:55 + Model.py:416-417)."""

    @staticmethod
    def forward(ctx, E, scores, cu_seqlens, max_len):
        _require_act(E, "E")
        _require(scores, "scores")
        n_bags, N, max_len, E2d = _bag_geometry(E, cu_seqlens, max_len)
        s2d = scores.reshape(E2d.shape[0], -1)
        pooled, m, l = pool_fwd_raw(E2d, s2d, n_bags, N, cu_seqlens, max_len)
        # (the inputs themselves are saved, not the 2-D views made here: a view made inside forward fails the version check of a
        # modified base with an error about no_grad views instead of "modified by an inplace operation")
        ctx.save_for_backward(E, scores, pooled, m, l, cu_seqlens if cu_seqlens is not None else torch.empty(0))
        ctx.geom = (n_bags, N, max_len, cu_seqlens is not None, E.shape, scores.shape)
        return pooled

    @staticmethod
    def backward(ctx, d_pooled):
        E, scores, pooled, m, l, cu = ctx.saved_tensors
        E2d = E.reshape(-1, E.shape[-1])
        s2d = scores.reshape(E2d.shape[0], -1)
        n_bags, N, max_len, ragged, e_shape, s_shape = ctx.geom
        cu = cu if ragged else None
        dE = torch.empty_like(E2d)
        ds = torch.empty_like(s2d)
        pool_bwd_raw(E2d, s2d, pooled, m, l, d_pooled.float().contiguous(), dE, 0, ds, 0, n_bags, N, cu, max_len)
        return dE.view(e_shape), ds.view(s_shape), None, None


class WeightedPoolFn(torch.autograd.Function):
    """pooled[b,c,:] = sum_t weights[b,t,c] E[b,t,c,:] with the weights taken as they are (no softmax): the relu / leaky_relu /
    sigmoid attention activations of abmil.py:56-61 pooled as Model.py:416-417 does."""

    @staticmethod
    def forward(ctx, E, weights, cu_seqlens, max_len):
        _require_act(E, "E")
        _require(weights, "weights")
        n_bags, N, max_len, E2d = _bag_geometry(E, cu_seqlens, max_len)
        w2d = weights.reshape(E2d.shape[0], -1)
        pooled, _, _ = _pool_fwd("wpool_fwd", ("pool_fwd",), E2d, w2d, n_bags, max_len, (n_bags, N, cu_seqlens, max_len))
        ctx.save_for_backward(E, weights, cu_seqlens if cu_seqlens is not None else torch.empty(0))     # (the inputs, as SoftmaxPoolFn)
        ctx.geom = (n_bags, N, max_len, cu_seqlens is not None, E.shape, weights.shape)
        return pooled

    @staticmethod
    def backward(ctx, d_pooled):
        E, weights, cu = ctx.saved_tensors
        E2d = E.reshape(-1, E.shape[-1])
        w2d = weights.reshape(E2d.shape[0], -1)
        n_bags, N, max_len, ragged, e_shape, w_shape = ctx.geom
        cu = cu if ragged else None
        dE = torch.empty_like(E2d)
        dw = torch.empty_like(w2d)
        _pool_bwd("wpool_bwd", ("pool_bwd",), E2d, w2d, (d_pooled.float().contiguous(), dE, 0, dw), (n_bags, N, cu, max_len))
        return dE.view(e_shape), dw.view(w_shape), None, None


def weighted_pool(E, weights, cu_seqlens=None, max_len=None):
    return WeightedPoolFn.apply(E, weights.contiguous(), cu_seqlens, max_len)


class RaggedViewPoolFn(torch.autograd.Function):
    """The two half-bag views of packed bags on their own (pooled [n_bags, 2, H*512]): the raw scores re-softmaxed over each half
    (Model.py:419-440, which uses F.softmax there whatever the attention activation) -- the views of the relu / leaky_relu / sigmoid
    activations, whose whole-bag pooling is the weighted pooling above."""

    @staticmethod
    def forward(ctx, E2d, scores, cu_seqlens, perm, vcu, max_view_len):
        _require_act(E2d, "E")
        _require(scores, "scores")
        perm, vcu, max_view_len = _check_rview(E2d, cu_seqlens, (perm, vcu, max_view_len))
        n_bags = cu_seqlens.numel() - 1
        pooled, m, l = pool_rview_fwd_raw(E2d, scores, n_bags, perm, vcu, max_view_len)
        ctx.save_for_backward(E2d, scores, pooled, m, l, perm, vcu)
        ctx.geom = (n_bags, max_view_len)
        return pooled

    @staticmethod
    def backward(ctx, d_pooled):
        E2d, scores, pooled, m, l, perm, vcu = ctx.saved_tensors
        n_bags, max_view_len = ctx.geom
        dE = torch.zeros_like(E2d)
        ds = torch.zeros_like(scores)
        pool_rview_bwd_raw(E2d, scores, pooled, m, l, d_pooled.float().contiguous(), dE, ds, n_bags, perm, vcu, max_view_len)
        return dE, ds, None, None, None, None


def ragged_view_pool(E2d, scores, cu_seqlens, perm, vcu, max_view_len):
    return RaggedViewPoolFn.apply(E2d, scores.contiguous(), cu_seqlens, perm, vcu, max_view_len)


# --------------------------------------------------------------------------------------------------
# A2 + A3 chained inside one autograd node: the pooling backward only produces d_scores, and its dE term
# w * d_pooled is added in the gate backward's dX epilogue -- dE is written exactly once.
# --------------------------------------------------------------------------------------------------
class AttnPoolFn(torch.autograd.Function):
    """(pooled [n_bags,(1+V,)H*512], raw scores [T,H], token projections [T,P]) = multi-head gated-ABMIL pooling (Model.py:406-417)
    and, with `views` = V int32 token-index lists (dense bags only), the V re-softmaxed sub-bag poolings of Model.py:419-440; on packed
    bags `rviews` = (perm, vcu, max_view_len) gives each bag its own two halves (mdl_abmil_pool_rview_*), pooled [n_bags, 3, H*512].
    With Wtok [P, H*512] (+ btok) the token_projector Linear (Model.py:140) -- the other consumer of E -- is part of the node: its dX
    is written into dE first and the gate dX epilogue accumulates onto it, so the two gradients of E are never summed by a separate
    3 x |E| elementwise pass (3.8 ms per config-3 step); without it the third output is an empty tensor."""

    @staticmethod
    def forward(ctx, E, Wa, ba, Wb, bb, wc, bc, p_drop, seed, keep_a, keep_b, cu_seqlens, max_len, Wtok, btok, Eimg, Escale, e_only_image,
                rviews, *views):
        # e_only_image: E IS the image tensor (Eimg is E, an opaque float32 [.., H*512] tensor written by the last pre_attn block's
        # LayerNorm kernel) -- no fp32 copy of E exists; the pooling kernels read the image, dE is the gradient of that tensor
        _require_act(E, "E")
        for t, n in ((Wa, "Wa"), (ba, "ba"), (Wb, "Wb"), (bb, "bb"), (wc, "wc"), (bc, "bc")):
            _require(t, n)
        n_bags, N, max_len, E2d = _bag_geometry(E, cu_seqlens, max_len)
        if views and cu_seqlens is not None:
            raise NotImplementedError("token-index views are defined on dense bags (the reference's n_views path stacks equal-N bags)")
        for v in views:
            _require(v, "view token indices", torch.int32)
        if rviews is not None:
            rviews = _check_rview(E2d, cu_seqlens, rviews)
        ctx.set_materialize_grads(False)
        need = any(ctx.needs_input_grad[:7]) or any(ctx.needs_input_grad[13:15])   # (inputs 15, 16 = the image of E: no gradient)
        Ei = None
        if e_only_image and (Eimg is None or views or rviews is not None or not _split_gate(E2d)
                             or (Wtok is not None and not split_linear_supported(E2d.shape[0], Wtok.shape[0], Wtok.shape[1]))):
            raise RuntimeError("attn_pool: an image-only E needs the split GEMM mode, no token views and a token projection the split "
                               "engine serves")
        recompute = need and GATE_RECOMPUTE
        if _split_gate(E2d):
            # the image of E: written by the producing LayerNorm kernel (Eimg / Escale), else built here (3 passes over E)
            Ei = SplitImage(Eimg, Escale, E2d.shape[0], E2d.shape[1]) if Eimg is not None else split_image(E2d)
        scores, act_a, act_b = gate_fwd_raw(Ei if Ei is not None else E2d, Wa, ba, Wb, bb, wc, bc, p_drop, seed, keep_a, keep_b,
                                            need and not recompute)
        pooled, m, l = (pool_fwd_img_raw(Ei, scores, n_bags, N, cu_seqlens, max_len) if e_only_image
                        else pool_fwd_raw(E2d, scores, n_bags, N, cu_seqlens, max_len))
        vstate = [pool_view_fwd_raw(E2d, scores, n_bags, N, v) for v in views]
        rstate = pool_rview_fwd_raw(E2d, scores, n_bags, *rviews) if rviews is not None else ()
        if Wtok is not None:
            _require(Wtok, "token_projector weight")
            if btok is not None:
                _require(btok, "token_projector bias")
            if Ei is not None and split_linear_supported(E2d.shape[0], Wtok.shape[0], Wtok.shape[1]):
                # split engine on the image of E the gate forward used (N = 128: half of the 256-wide tile idles, still faster than
                # the fp32 tall tile)
                tok = split_gemm_nt(Ei, weight_image(Wtok), btok, name="linear_fwd")
            else:
                if not linear_supported(E2d, Wtok):   # a clear message instead of a kernel return code
                    raise NotImplementedError("attn_pool: token projection %s on %s %s rows is outside the HIP Linear kernels' geometries "
                                              "(functional.linear_supported)" % (tuple(Wtok.shape), E2d.shape[0], E2d.dtype))
                tok = linear_fwd_raw(E2d, Wtok, btok)
        else:
            tok = E2d.new_empty(0)
            ctx.mark_non_differentiable(tok)
        if need:
            flat = [t for st in vstate for t in st]
            none = torch.empty(0)
            # (the image of E travels as saved tensors like everything else: saved-tensor hooks, retain_graph and version checks apply)
            # (E itself, not the 2-D view of it made here: see SoftmaxPoolFn)
            ctx.save_for_backward(E, Wa, Wb, wc, act_a if not recompute else none, act_b if not recompute else none, scores, pooled, m, l,
                                  cu_seqlens if cu_seqlens is not None else none, Wtok if Wtok is not None else none,
                                  Ei.data if Ei is not None else none, Ei.scale if Ei is not None else none,
                                  ba if recompute else none, bb if recompute else none, bc if recompute else none,
                                  keep_a if keep_a is not None else none, keep_b if keep_b is not None else none, *views, *flat,
                                  *(rviews[:2] if rviews is not None else ()), *rstate)
            ctx.rview_max = None if rviews is None else rviews[2]
            ctx.recompute = recompute
            ctx.cfg = (p_drop, seed, keep_a is not None, keep_b is not None, n_bags, N, max_len, cu_seqlens is not None, E.shape, len(views),
                       Wtok is not None, btok is not None)
            ctx.e_only_image = bool(e_only_image)
            ctx.has_image = Ei is not None
        if views:
            pooled = torch.stack([pooled] + [st[0] for st in vstate], dim=1)
        elif rviews is not None:
            pooled = torch.cat([pooled.unsqueeze(1), rstate[0]], dim=1)
        return pooled, scores, tok

    @staticmethod
    def backward(ctx, d_pooled, d_scores_in, d_tok):
        p_drop, seed, has_keep_a, has_keep_b, n_bags, N, max_len, ragged, e_shape, V, has_tok, has_btok = ctx.cfg
        saved = ctx.saved_tensors
        E, Wa, Wb, wc, act_a, act_b, scores, pooled, m, l, cu, Wtok, Eidata, Eiscale, ba, bb, bc, keep_a, keep_b = saved[:19]
        E2d = E.reshape(-1, E.shape[-1])
        keep_a, keep_b = keep_a if has_keep_a else None, keep_b if has_keep_b else None
        views, vflat = saved[19:19 + V], saved[19 + V:19 + 4 * V]
        rview = None if ctx.rview_max is None else tuple(saved[19 + 4 * V:]) + (ctx.rview_max,)   # (perm, vcu, pooled, m, l, max_view_len)
        n_out = 1 + V + (2 if rview is not None else 0)
        Ei = SplitImage(Eidata, Eiscale, E2d.shape[0], E2d.shape[1]) if ctx.has_image else None
        if ctx.recompute:   # rebuild the activations: the same kernel, seed and masks as the forward -> the same bits
            _s, act_a, act_b = gate_fwd_raw(Ei if Ei is not None else E2d, Wa, ba, Wb, bb, wc, bc, p_drop, seed, keep_a, keep_b, True)
        cu = cu if ragged else None
        dE = torch.empty_like(E2d)
        if d_scores_in is not None:
            ds = d_scores_in.float().contiguous().clone()
            acc_s = 1
        else:
            ds = torch.empty_like(scores)
            acc_s = 0
        if d_pooled is None:
            d_pooled = torch.zeros(n_bags, n_out, pooled.shape[-1], device=pooled.device) if n_out > 1 else torch.zeros_like(pooled)
        d_pooled = d_pooled.float().contiguous()
        d_main = d_pooled[:, 0].contiguous() if n_out > 1 else d_pooled
        d_rview = d_pooled[:, 1:].contiguous() if rview is not None else None
        # the other consumer of E, the token_projector: its dX is accumulated into the same dE buffer (no separate gradient tensor, no
        # add pass).  Split engine: AFTER the gate backward, and only on the 256-token tiles where d_tok is not identically zero (the
        # local loss reads the first <= 256 tokens of a bag, so d_tok is zero on ~94 % of the tiles at N = 4096); the other engines:
        # before it (the gate dX epilogue then accumulates).
        dWtok = dbtok = None
        acc_e = 0
        tok_after = has_tok and d_tok is not None and Ei is not None and split_linear_supported(E2d.shape[0], Wtok.shape[0], Wtok.shape[1])
        if has_tok and d_tok is not None and not tok_after:
            dWtok, dbtok = linear_bwd_raw(E2d, Wtok, d_tok.to(E2d.dtype).contiguous(), dE, has_btok)
            acc_e = 1
        # scores-only pooling backward (one read of E), then the gate backward whose dX epilogue adds the pooling term
        if ctx.e_only_image:
            pool_dscores_img_raw(Ei, scores, pooled, m, l, d_main, ds, acc_s, n_bags, N, cu, max_len)
        else:
            pool_bwd_raw(E2d, scores, pooled, m, l, d_main, None, 0, ds, acc_s, n_bags, N, cu, max_len)
        for i in range(V):   # the views' score gradients must be in ds before the gate backward consumes it
            vp, vm, vl = vflat[3 * i:3 * i + 3]
            pool_view_bwd_raw(E2d, scores, vp, vm, vl, d_pooled[:, 1 + i].contiguous(), None, ds, n_bags, N, views[i])
        if rview is not None:
            perm, vcu, rp, rm, rl, rmax = rview
            pool_rview_bwd_raw(E2d, scores, rp, rm, rl, d_rview, None, ds, n_bags, perm, vcu, rmax)
        row_bag = None
        if ragged:   # bag index of every packed token row, on the device (no sync)
            row_bag = torch.searchsorted(cu[1:].contiguous(), torch.arange(E2d.shape[0], device=E2d.device), right=True).to(torch.int32)
        pool = (scores, m, l, d_main, row_bag, N if not ragged else 0)
        if Ei is not None:
            am = torch.zeros(1, device=dE.device, dtype=torch.float32) if n_out == 1 else None   # (views add to dE afterwards)
            dWa, dWb, dba, dbb, dwc, dbc = gate_bwd_raw(Ei, Wa, Wb, wc, act_a, act_b, ds, dE, p_drop, seed, keep_a, keep_b, pool=pool,
                                                        accumulate=acc_e, dE_absmax=am)
            if tok_after:
                d_tok = d_tok.float().contiguous()
                dti = split_image(d_tok, pad_rows=32)
                gate, chunk_max = split_tile_absmax(d_tok, chunks=True)   # one pass: 256-row tiles (dX) and 32-row chunks (dW)
                split_gemm_nt(dti, weight_image(Wtok.t().contiguous()), out=dE, accumulate=True, absmax_out=am, name="linear_bwd",
                              row_gate=gate, terms=GRAD_TERMS)
                dWtok = split_gemm_tn(Ei, dti, name="linear_bwd", b_chunk_max=chunk_max, terms=GRAD_TERMS)
                dbtok = d_tok.sum(0) if has_btok else None
            if am is not None:
                _put_absmax(dE, am)
        else:
            dWa, dWb, dba, dbb, dwc, dbc = gate_bwd_raw(E2d, Wa, Wb, wc, act_a, act_b, ds, dE, p_drop, seed, keep_a, keep_b, pool=pool,
                                                        accumulate=acc_e)
        for i in range(V):   # ... and their dE terms are added once dE has been written (no read of E)
            vp, vm, vl = vflat[3 * i:3 * i + 3]
            pool_view_bwd_raw(E2d, scores, vp, vm, vl, d_pooled[:, 1 + i].contiguous(), dE, None, n_bags, N, views[i])
        if rview is not None:
            pool_rview_bwd_raw(E2d, scores, rp, rm, rl, d_rview, dE, None, n_bags, perm, vcu, rmax)
        return (dE.view(e_shape), dWa, dba, dWb, dbb, dwc, dbc, None, None, None, None, None, None, dWtok, dbtok, None, None, None,
                None) + (None,) * V


def attn_pool(E, Wa, ba, Wb, bb, wc, bc, p_drop=0.0, seed=0, keep_a=None, keep_b=None, cu_seqlens=None, max_len=None, views=(),
              tok_proj=None, e_img=None, e_only_image=False, rviews=None):
    """-> (pooled, raw scores), or (pooled, raw scores, token projections [T,P]) with tok_proj = (Wtok [P,H*512], btok or None).
    rviews = (perm int32 [T], vcu int64 [2*n_bags+1], max_view_len): the two half-bag views of every packed bag (pooled [n_bags,3,H*512]).
    e_img = (image data, scale) of E when the producing kernel wrote one (split GEMM mode); e_only_image: E is that image tensor itself
    (no fp32 E was written) and the node's E-gradient is the image tensor's."""
    Wtok, btok = tok_proj if tok_proj is not None else (None, None)
    Eimg, Escale = e_img if e_img is not None else (None, None)
    pooled, scores, tok = AttnPoolFn.apply(E, Wa, ba, Wb, bb, wc, bc, float(p_drop), int(seed), keep_a, keep_b, cu_seqlens, max_len,
                                           None if Wtok is None else Wtok.contiguous(), None if btok is None else btok.contiguous(),
                                           Eimg, Escale, bool(e_only_image), None if rviews is None else tuple(rviews), *views)
    return (pooled, scores) if tok_proj is None else (pooled, scores, tok)


def gate_scores(E2d, Wa, ba, Wb, bb, wc, bc, p_drop=0.0, seed=0, keep_a=None, keep_b=None):
    return GateScoresFn.apply(E2d, Wa, ba, Wb, bb, wc, bc, float(p_drop), int(seed), keep_a, keep_b)


def softmax_pool(E, scores, cu_seqlens=None, max_len=None):
    return SoftmaxPoolFn.apply(E, scores, cu_seqlens, max_len)


# --------------------------------------------------------------------------------------------------
# N1: fused LayerNorm -> GELU -> Dropout (pre-attention MLP)
# --------------------------------------------------------------------------------------------------
class LNGeluDropFn(torch.autograd.Function):
    """y = Dropout_p(GELU(LayerNorm(x + bias; gamma, beta, eps)))  over the last axis (Model.py:351-354).
    `bias` (optional) is the bias of the preceding Linear: the GEMM then runs bias-free and the bias gradient (column
    sums of dx) comes out of the same backward pass instead of a separate reduction over dx.
    With `cu_groups` (int64 [G + 1]), `bias` is [G, W], one row per GROUP of rows (rows [cu_groups[g], cu_groups[g + 1]) take bias[g]):
    the first block of the pre-attention MLP when the stain encoding is folded out of its Linear (Model.py:125-132, :351) on the bf16 /
    exact-fp32 engines -- the split engine adds the row in its GEMM epilogue instead (PreAttnBlockFn).  The bias gradient is then the
    per-group sums of dx."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, p_drop, seed, keep, bias, cu_groups):
        _require_act(x, "x")
        _require(gamma, "gamma")
        _require(beta, "beta")
        W = x.shape[-1]
        rows = x.numel() // W
        if cu_groups is None:
            if bias is not None:
                _require(bias, "bias")
            name, groups, unsupported = "mdl_ln_gelu_drop_fwd", (), (_LN_WIDTHS, W)
        else:
            _require(bias, "group_bias")
            _require(cu_groups, "cu_groups", torch.int64)
            G = bias.shape[0]
            if bias.shape != (G, W) or cu_groups.numel() != G + 1:
                raise ValueError("group_bias must be [G, W] with cu_groups [G + 1]")
            name, groups = "mdl_ln_gelu_drop_fwd_groups", (cu_groups, G)
            unsupported = ("grouped LayerNorm-GELU-Dropout supports widths 256/512/1024 (got %d)", W)
        y = torch.empty_like(x)
        mean = torch.empty(rows, device=x.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        with _timed("ln_gelu_drop_fwd", ("byte", 2.0 * x.numel() * x.element_size())):
            _call(name + _sfx(x), x, bias, gamma, beta, y, mean, rstd, rows, W, float(eps), float(p_drop), int(seed), keep, *groups, _stream(),
                  unsupported=unsupported)
        none = torch.empty(0)
        ctx.save_for_backward(x, gamma, beta, mean, rstd, bias if bias is not None else none, keep if keep is not None else none,
                              cu_groups if cu_groups is not None else none)
        ctx.cfg = (float(p_drop), int(seed), keep is not None, bias is not None, groups[1:])
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, beta, mean, rstd, bias, keep, cu_groups = ctx.saved_tensors
        p_drop, seed, has_keep, has_bias, groups = ctx.cfg
        keep = keep if has_keep else None
        groups = (cu_groups,) + groups if groups else ()
        bias = bias if has_bias else None
        W = x.shape[-1]
        rows = x.numel() // W
        dy = dy.to(x.dtype).contiguous()
        dx = torch.empty_like(x)
        dg, db = torch.empty_like(gamma), torch.empty_like(beta)
        dbias = torch.empty_like(bias) if has_bias else None
        g = "_groups" if groups else ""
        ws = _ws_for("mdl_ln_gelu_drop_bwd%s_ws_bytes" % g, x.device, rows, W, *groups[1:])
        with _timed("ln_gelu_drop_bwd", ("byte", 3.0 * x.numel() * x.element_size())):
            _call("mdl_ln_gelu_drop_bwd" + g + _sfx(x), x, bias, gamma, beta, mean, rstd, dy, dx, dg, db, dbias, rows, W, p_drop, seed, keep,
                  *groups, ws, _stream())
        return dx, dg, db, None, None, None, None, dbias, None


def ln_gelu_drop_groups(x, gamma, beta, eps, p_drop, seed, keep, group_bias, cu_groups):
    return LNGeluDropFn.apply(x.contiguous(), gamma.contiguous(), beta.contiguous(), eps, p_drop, seed, keep,
                              group_bias.float().contiguous(), cu_groups)


def ln_gelu_drop(x, gamma, beta, eps=1e-5, p_drop=0.0, seed=0, keep=None, bias=None):
    return LNGeluDropFn.apply(x.contiguous(), gamma.contiguous(), beta.contiguous(), eps, p_drop, seed, keep,
                              None if bias is None else bias.contiguous(), None)


# --------------------------------------------------------------------------------------------------
# N1: bias-free Linear of the pre-attention MLP on the fp32 matrix cores
# --------------------------------------------------------------------------------------------------
class LinearFn(torch.autograd.Function):
    """Y = X W^T (+ bias) (Model.py:351, :355, :359 without the bias, which ln_gelu_drop adds; Model.py:140 token_projector and
    Model.py:145 projector with their bias); X [T,K] fp32 or bf16 (bf16 mode: x, y and their gradients bf16; W, bias and their
    gradients fp32 -- mdl_linear_*_bf16), W [N,K]."""

    @staticmethod
    def forward(ctx, x, W, bias):
        _require_act(x, "x")
        _require(W, "weight")
        if bias is not None:
            _require(bias, "bias")
        y = linear_fwd_raw(x, W, bias)
        ctx.save_for_backward(x, W)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, W = ctx.saved_tensors
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dW, db = linear_bwd_raw(x, W, dy.to(x.dtype).contiguous(), dx, ctx.has_bias)
        return dx, dW, db


LinearBf16Fn = LinearFn   # one node for both storage types (kept for callers of the round-2 name)


def linear_supported(x, W) -> bool:
    """Geometries of mdl_linear_* (include/madeleine_amd.h).  fp32: at most 256 rows -> K % 4 == 0, N % 4 == 0; otherwise
    N % 256 == 0 with K % 32 == 0, or N % 256 == 128 with K % 256 == 0.  bf16 activations (fp32 weight): N % 128 == 0,
    K % 32 == 0 (mdl_linear_*_bf16; at most 256 rows run the fp32 small-M kernel on an fp32 copy of the rows)."""
    N, K = W.shape
    if W.dtype != torch.float32 or not x.is_cuda:
        return False
    T = x.numel() // max(1, x.shape[-1])
    if x.dtype not in ACT_DTYPES:
        return False
    if T <= 256:
        return N % 4 == 0 and K % 4 == 0
    if x.dtype == torch.bfloat16:
        return bool(_native.lib().mdl_linear_bf16_supported(N, K, 1))
    return (N % 256 == 0 and K % 32 == 0) or (N % 128 == 0 and K % 256 == 0)


def linear(x, W, bias=None):
    """Linear over the last axis through the HIP kernels (fp32, or bf16 activations with fp32 parameters).  There is no library
    fallback: a geometry outside linear_supported raises (every Linear of the encoder -- reference Model.py:140, :145, :351, :355,
    :359 with patch_embedding_dim (+ 32 stain channels) a multiple of 32 -- is inside it)."""
    if not linear_supported(x, W):
        raise NotImplementedError(
            "madeleine_amd.linear: unsupported geometry / dtype (x %s %s on %s, weight %s %s); the HIP kernels need a ROCm device, "
            "fp32 weights, fp32 / bf16 activations and in_features a multiple of 32 (4 for at most 256 rows), out_features a "
            "multiple of 256 (or of 128 with in_features a multiple of 256; of 4 for at most 256 rows)"
            % (tuple(x.shape), x.dtype, x.device, tuple(W.shape), W.dtype))
    lead = x.shape[:-1]
    x2 = x.reshape(-1, x.shape[-1]).contiguous()
    Wc, bc = W.contiguous(), None if bias is None else bias.contiguous()
    if x.dtype == torch.bfloat16 and x2.shape[0] <= 256:
        # a handful of rows (one short bag under autocast): exact fp32 FMA kernel on the widened rows, result stored as bf16
        y = LinearFn.apply(x2.float(), Wc, bc).to(torch.bfloat16)
    elif x.dtype == torch.float32 and GEMM_MODE == "split" and split_linear_supported(x2.shape[0], W.shape[0], W.shape[1]):
        y = SplitLinearFn.apply(x2, Wc, bc)
    else:
        y = (LinearBf16Fn if x.dtype == torch.bfloat16 else LinearFn).apply(x2, Wc, bc)
    return y.view(*lead, W.shape[0])


# --------------------------------------------------------------------------------------------------
# L1: InfoNCE (batched over problems)
# --------------------------------------------------------------------------------------------------
class InfoNCEFn(torch.autograd.Function):
    """(loss [S], row_loss [S,Kmax]) for S padded problems Q,P [S,Kmax,D] with cnt[S] live rows each (loss.py:111-127);
    row_loss = the per-sample losses (reduction 'none').  Use ONE of the two outputs downstream."""

    @staticmethod
    def forward(ctx, Q, P, cnt, temperature, symmetric, per_row):
        _require(Q, "query")
        _require(P, "positive_key")
        _require(cnt, "cnt", torch.int32)
        S, Kmax, D = Q.shape
        loss = torch.empty(S, device=Q.device, dtype=torch.float32)
        rows = torch.empty(S, Kmax, device=Q.device, dtype=torch.float32) if per_row else None
        ws = _ws_for("mdl_infonce_ws_bytes", Q.device, S, Kmax, D)
        with _timed("infonce_fwd"):
            _call("mdl_infonce_fwd", Q, P, cnt, loss, rows, S, Kmax, D, float(temperature), int(symmetric), ws, _stream())
        ctx.save_for_backward(cnt, ws, Q, P)
        ctx.cfg = (S, Kmax, D, float(temperature), int(symmetric), bool(per_row))
        if not per_row:
            rows = loss.new_empty(0)
            ctx.mark_non_differentiable(rows)
        return loss, rows

    @staticmethod
    def backward(ctx, d_loss, d_rows):
        cnt, ws, Q, P = ctx.saved_tensors
        S, Kmax, D, temperature, symmetric, per_row = ctx.cfg
        dev = cnt.device
        dQ = torch.empty(S, Kmax, D, device=dev, dtype=torch.float32)
        dP = torch.empty_like(dQ)
        if per_row:
            # loss [S] = mean of the rows: fold an upstream gradient on it into the per-row gradients
            g = d_rows.float().contiguous() if d_rows is not None else torch.zeros(S, Kmax, device=dev)
            if d_loss is not None:
                g = g + d_loss.float().unsqueeze(1) / cnt.clamp_min(1).unsqueeze(1).float()
            d_loss, d_rows = None, g.contiguous()
        else:
            d_loss, d_rows = d_loss.float().contiguous(), None
        with _timed("infonce_bwd"):
            _call("mdl_infonce_bwd", Q, P, d_loss, d_rows, cnt, dQ, dP, S, Kmax, D, temperature, symmetric, ws, _stream())
        return dQ, dP, None, None, None, None


def info_nce_batched(Q, P, cnt, temperature, symmetric):
    return InfoNCEFn.apply(Q, P, cnt, float(temperature), bool(symmetric), False)[0]


def info_nce_rows(Q, P, cnt, temperature, symmetric):
    """Per-sample losses [S, Kmax] (reduction 'none'); rows >= cnt[s] are zero."""
    return InfoNCEFn.apply(Q, P, cnt, float(temperature), bool(symmetric), True)[1]


class InfoNCENegFn(torch.autograd.Function):
    """(loss [], row_loss [N]) of N queries against their positives and explicit negatives (loss.py:93-110, finished with the cross
    entropy of loss.py:125).  Q,P [N,Dq] fp32 zero-padded to Dq = D rounded up to 32; Neg [M,D] (unpaired) or [N,M,D] (paired) fp32,
    contiguous, read in place.  dNeg is computed only when Neg requires grad.  Use ONE of the two outputs downstream."""

    @staticmethod
    def forward(ctx, Q, P, Neg, temperature, paired, per_row):
        _require(Q, "query")
        _require(P, "positive_key")
        _require(Neg, "negative_keys")
        N, Dq = Q.shape
        M, D = Neg.shape[-2], Neg.shape[-1]
        loss = torch.empty((), device=Q.device, dtype=torch.float32)
        rows = torch.empty(N, device=Q.device, dtype=torch.float32) if per_row else None
        ws = _ws_for("mdl_infonce_neg_ws_bytes", Q.device, N, M, D, int(paired))
        work = ("byte", 4.0 * Neg.numel()) if paired else ("flop", 2.0 * N * M * D)
        with _timed("infonce_neg_fwd", work):
            _call("mdl_infonce_neg_fwd", Q, P, Neg, loss, rows, N, M, D, int(paired), float(temperature), ws, _stream())
        ctx.save_for_backward(ws, Neg, Q, P)     # (Q, P: the backward reads what the forward left of them in ws; saved for the version check)
        ctx.cfg = (N, M, D, Dq, float(temperature), bool(paired), bool(per_row))
        if not per_row:
            rows = loss.new_empty(0)
            ctx.mark_non_differentiable(rows)
        return loss, rows

    @staticmethod
    def backward(ctx, d_loss, d_rows):
        ws, Neg, _Q, _P = ctx.saved_tensors
        N, M, D, Dq, temperature, paired, per_row = ctx.cfg
        dev = Neg.device
        dQ = torch.empty(N, Dq, device=dev, dtype=torch.float32)
        dP = torch.empty_like(dQ)
        dNeg = torch.empty_like(Neg) if ctx.needs_input_grad[2] else None
        if per_row:
            # loss = mean of the rows: fold an upstream gradient on it into the per-row gradients
            g = d_rows.float() if d_rows is not None else torch.zeros(N, device=dev)
            if d_loss is not None:
                g = g + d_loss.float() / max(N, 1)
            dl, dr = None, g.contiguous()
        else:
            dl, dr = d_loss.float().reshape(1).contiguous(), None
        passes = 2 if dNeg is not None else 1
        work = ("byte", 4.0 * Neg.numel() * (1 + passes)) if paired else ("flop", 2.0 * N * M * D * (1 + passes))
        with _timed("infonce_neg_bwd", work):
            _call("mdl_infonce_neg_bwd", Neg, dl, dr, dQ, dP, dNeg, N, M, D, int(paired), temperature, ws, _stream())
        return dQ, dP, dNeg, None, None, None


def info_nce_neg(Q, P, Neg, temperature, paired):
    """Mean loss [] of N rows against explicit negatives (InfoNCENegFn)."""
    return InfoNCENegFn.apply(Q, P, Neg, float(temperature), bool(paired), False)[0]


def info_nce_neg_rows(Q, P, Neg, temperature, paired):
    """Per-row losses [N] against explicit negatives (reduction 'none')."""
    return InfoNCENegFn.apply(Q, P, Neg, float(temperature), bool(paired), True)[1]


# --------------------------------------------------------------------------------------------------
# G0-G3: graph optimal transport
# --------------------------------------------------------------------------------------------------
class _GotFamily:
    """One GOT size class on the C ABI: the prefix of its six entry points (mdl_got / mdl_got_tiled / mdl_got_tiled_rect), the _timed
    names of its calls and the message of its refusal.  A `rect` family takes V [k, n, d] and Q [k, m, d] with n != m; its entry points
    take the sizes as (k, n, m, d)."""

    def __init__(self, prefix, timed, refusal, rect=False):
        self.prefix, self.timed, self.refusal, self.rect = prefix, timed, refusal, rect

    def sizes(self, V, Q):
        """The size arguments of this family's entry points."""
        k, n, d = V.shape
        return (k, n, Q.shape[1], d) if self.rect else (k, n, d)

    def workspace(self, V, Q):
        """The workspace of one problem, kept from the forward to the end of the backward; refuses a shape outside the class."""
        sz = self.sizes(V, Q)
        return _ws_for(self.prefix + "_ws_bytes", V.device, *sz, refusal=(self.refusal,) + sz[1:])

    def call(self, stage, sz, ws, *tensors):
        """<prefix><stage>(tensors..., sizes..., ws, stream): the argument list of every entry point of a family."""
        _call(self.prefix + stage, *tensors, *sz, ws, _stream())

    # ---- the stages of a call, once for GOTFn, got_extrema and HipGotImpl: each owns its workspace query, its _timed name and its call.
    # The state of a forward is (V, Q, ws): what the backward stages take.  timer: _timed, or _untimed for a stage that is not timed.
    def extrema(self, V, Q):
        sz = self.sizes(V, Q)
        ws = _ws_for(self.prefix + "_ws_bytes", V.device, *sz)     # (its own scratch; a shape outside the class fails as a workspace query)
        mm = torch.empty(6, device=V.device, dtype=torch.float32)
        self.call("_extrema", sz, ws, V, Q, mm)
        return mm

    def forward(self, V, Q, mm_out, minmax_in):
        ws = self.workspace(V, Q)
        out = torch.empty(2, device=V.device, dtype=torch.float32)
        with _timed(self.timed + "_fwd"):
            self.call("_fwd", self.sizes(V, Q), ws, V, Q, out, mm_out, minmax_in)
        return out, (V, Q, ws)

    def backward(self, state, d_out):
        """Both backward stages in one call: a backward that keeps its own threshold gradients."""
        V, Q, ws = state
        dV, dQ = torch.empty_like(V), torch.empty_like(Q)
        with _timed(self.timed + "_bwd"):
            self.call("_bwd", self.sizes(V, Q), ws, V, Q, d_out.contiguous(), dV, dQ)
        return dV, dQ

    def backward_begin(self, state, d_out, timer):
        V, Q, ws = state
        dmm = torch.empty(6, device=V.device, dtype=torch.float32)
        with timer(self.timed + "_bwd"):
            self.call("_bwd_begin", self.sizes(V, Q), ws, d_out.contiguous(), dmm)
        return dmm

    def backward_finish(self, state, dmm_total, timer):
        V, Q, ws = state
        dV, dQ = torch.empty_like(V), torch.empty_like(Q)
        with timer(self.timed + "_bwd_finish"):
            self.call("_bwd_finish", self.sizes(V, Q), ws, V, Q, dV, dQ, dmm_total.contiguous())
        return dV, dQ


_untimed = lambda _name: contextlib.nullcontext()      # noqa: E731  (functional.got's two-stage backward is not timed)
GOT_RESIDENT = _GotFamily("mdl_got", "got",
                          "madeleine_amd.GOT supports n <= 512 tokens per bag and d <= 128 (got n=%d, d=%d); "
                          "the reference calls it with subsample=256 (trainer.py:44)")
GOT_TILED = _GotFamily("mdl_got_tiled", "got_tiled",
                       "the tiled GOT class supports n <= 4096 tokens per bag and d <= 4096 (got n=%d, d=%d)")
GOT_TILED_RECT = _GotFamily("mdl_got_tiled_rect", "got_tiled",
                            "the tiled GOT class supports n <= 4096 and m <= 4096 tokens per bag and d <= 4096 (got n=%d, m=%d, d=%d)",
                            rect=True)


class GOTFn(torch.autograd.Function):
    """out[2] = (sum_b WD_b, sum_b GWD_b) for token sets V,Q [k,n,d] (loss.py:278-302 after the sub-sampling); Q may be [k,m,d] with
    m != n for a family that is rectangular-capable (GOT_TILED_RECT).

    minmax_in (optional float[6] device tensor) replaces the batch-local threshold extrema (data-parallel path);
    the second output is this call's own extrema [6] (non-differentiable).  `fam` selects the size class (entry-point family):
    GOT_RESIDENT (the default, functional.got), GOT_TILED or GOT_TILED_RECT (functional.got_tiled)."""

    @staticmethod
    def forward(ctx, V, Q, minmax_in, reduce_dminmax, fam=GOT_RESIDENT):
        _require(V, "v_")
        _require(Q, "q_")
        if V.dim() != 3 or Q.dim() != 3 or (V.shape[0], V.shape[2]) != (Q.shape[0], Q.shape[2]) or (
                V.shape[1] != Q.shape[1] and not fam.rect):
            raise ValueError("GOT expects two token tensors of identical shape [k, n, d]")
        mm = torch.empty(6, device=V.device, dtype=torch.float32)
        out, state = fam.forward(V, Q, mm, minmax_in)
        ctx.save_for_backward(*state)
        ctx.reduce_dminmax = reduce_dminmax
        ctx.fam = fam
        ctx.mark_non_differentiable(mm)
        return out, mm

    @staticmethod
    def backward(ctx, d_out, _d_mm):
        fam, state = ctx.fam, ctx.saved_tensors
        if ctx.reduce_dminmax is None:
            dV, dQ = fam.backward(state, d_out)
        else:
            dmm = ctx.reduce_dminmax(fam.backward_begin(state, d_out, _untimed))      # e.g. all_reduce(SUM) over ranks
            dV, dQ = fam.backward_finish(state, dmm, _untimed)
        return dV, dQ, None, None, None


def got_extrema(V, Q):
    """Extrema [6] (cross min,max | intra-V min,max | intra-Q min,max) of this batch's raw GOT cost tensors."""
    _require(V, "v_")
    _require(Q, "q_")
    return GOT_RESIDENT.extrema(V, Q)


def got_exchange_timeouts(ws) -> float:
    """Diagnostic of the split IPOT sweeps (csrc/got_resident.hip, Xch): non-zero when a workgroup gave up waiting for its partner's column
    sums in the last pass on this workspace.  That pass's numbers are void and say so themselves: the distances of a forward and the
    token gradients of a backward on a flagged workspace come back NaN (got_sum_kernel / got_cost_bwd_kernel) -- the flag is for
    diagnosis, nothing has to poll it.  The workspace's global region ends with
    {generation, time-out flag, 0, 0}; mdl_got_ws_bytes adds 64 bytes of padding behind it.  Synchronises."""
    nf = (ws.numel() * ws.element_size() - 64) // 4
    return float(ws.view(torch.uint8)[:nf * 4].view(torch.float32)[nf - 3])


def _got_set_exchange_timeout(ws, value: float = 1.0) -> None:
    """Test hook: writes the workspace's time-out flag (what a split sweep does when it gives up on its partner)."""
    nf = (ws.numel() * ws.element_size() - 64) // 4
    ws.view(torch.uint8)[:nf * 4].view(torch.float32)[nf - 3] = value


def got(V, Q, minmax_in=None, reduce_dminmax=None, return_extrema=False):
    out, mm = GOTFn.apply(V, Q, minmax_in, reduce_dminmax)
    return (out, mm) if return_extrema else out


def got_tiled(V, Q, minmax_in=None, reduce_dminmax=None, return_extrema=False):
    """functional.got on the tiled size class (1 <= n <= 4096, 1 <= d <= 4096, any k; csrc/got_tiled.hip): same contract.  Q may have
    another token count than V (V [k, n, d], Q [k, m, d], 1 <= m <= 4096): the cross cost and the plans are then n x m, and the
    data-parallel contract (global extrema in, d_minmax reduced by the caller's function) is unchanged.  GOT(V, Q) != GOT(Q, V)."""
    fam = GOT_TILED if V.dim() != 3 or Q.dim() != 3 or V.shape[1] == Q.shape[1] else GOT_TILED_RECT
    out, mm = GOTFn.apply(V, Q, minmax_in, reduce_dminmax, fam)
    return (out, mm) if return_extrema else out


def got_tiled_supported(k: int, n: int, d: int, m: int = None) -> bool:
    """True when the tiled class accepts V [k, n, d] with Q [k, m, d] (m omitted: m = n); mdl_got_tiled_rect_ws_bytes does not refuse it."""
    return _native.lib().mdl_got_tiled_rect_ws_bytes(k, n, n if m is None else m, d) >= 0


def got_resident_supported(k: int, n: int, d: int) -> bool:
    """True when the resident classes accept [k, n, d] (mdl_got_ws_bytes does not refuse it)."""
    return _native.lib().mdl_got_ws_bytes(k, n, d) >= 0


class HipGotImpl:
    """The four stages of GOT on the C ABI, as used by the multi-problem / data-parallel autograd node
    (madeleine_amd.distributed.got_multi): the calls of GOTFn, fixed to the resident size class.  A CPU implementation with the same
    interface exists only in tests/."""
    FAM = GOT_RESIDENT

    @staticmethod
    def extrema(V, Q):
        return got_extrema(V, Q)

    @staticmethod
    def forward(V, Q, minmax):
        return HipGotImpl.FAM.forward(V, Q, None, minmax.contiguous())

    @staticmethod
    def backward_begin(state, d_out):
        return HipGotImpl.FAM.backward_begin(state, d_out, _timed)

    @staticmethod
    def backward_finish(state, dmm_total):
        return HipGotImpl.FAM.backward_finish(state, dmm_total, _timed)

    # ---- several problems per launch (mdl_got_*_multi): every kernel launch covers all problems, on the caller's stream alone ----
    MAX_BATCH = _native._DEFINES["MDL_GOT_MAX_BATCH"]
    MAX_BATCH_N = 256      # tokens of a problem of a batched call (the register classes of csrc/got_resident.hip; MDL_E_UNSUPPORTED above)

    @staticmethod
    def can_batch(problems) -> bool:
        """2 .. MAX_BATCH non-empty problems on one ROCm device, every n <= MAX_BATCH_N, one d."""
        if not 2 <= len(problems) <= HipGotImpl.MAX_BATCH or os.environ.get("MADELEINE_GOT_NO_BATCH"):
            return False
        d = problems[0][0].shape[2]
        return all(V.is_cuda and V.dtype == torch.float32 and V.shape[0] >= 1 and 1 <= V.shape[1] <= HipGotImpl.MAX_BATCH_N
                   and V.shape[2] == d and V.device == problems[0][0].device for V, _ in problems)

    @staticmethod
    def _arrays(problems, wss):
        import ctypes
        np_ = len(problems)
        ptrs = lambda ts: (ctypes.c_void_p * np_)(*[t.data_ptr() for t in ts])      # noqa: E731
        ks = (ctypes.c_int * np_)(*[int(V.shape[0]) for V, _ in problems])
        ns = (ctypes.c_int * np_)(*[int(V.shape[1]) for V, _ in problems])
        return np_, ptrs([V for V, _ in problems]), ptrs([Q for _, Q in problems]), ks, ns, int(problems[0][0].shape[2]), ptrs(wss), ptrs

    @staticmethod
    def _rows(t):
        import ctypes
        return (ctypes.c_void_p * t.shape[0])(*[t.data_ptr() + i * t.stride(0) * t.element_size() for i in range(t.shape[0])])

    @staticmethod
    def extrema_multi(problems):
        dev = problems[0][0].device
        wss = [_ws_for("mdl_got_ws_bytes", dev, *V.shape) for V, _ in problems]
        np_, Vp, Qp, ks, ns, d, wsp, _ = HipGotImpl._arrays(problems, wss)
        mm = torch.empty(np_, 6, device=dev, dtype=torch.float32)
        _call("mdl_got_extrema_multi", np_, Vp, Qp, HipGotImpl._rows(mm), ks, ns, d, wsp, _stream())
        return mm

    @staticmethod
    def forward_multi(problems, minmax):
        dev = problems[0][0].device
        wss = [HipGotImpl.FAM.workspace(V, Q) for V, Q in problems]
        np_, Vp, Qp, ks, ns, d, wsp, _ = HipGotImpl._arrays(problems, wss)
        out = torch.empty(np_, 2, device=dev, dtype=torch.float32)
        mm = minmax.contiguous()
        with _timed("got_fwd"):
            _call("mdl_got_fwd_multi", np_, Vp, Qp, HipGotImpl._rows(out), HipGotImpl._rows(mm), ks, ns, d, wsp, _stream())
        return out, (list(problems), wss)

    @staticmethod
    def backward_begin_multi(state, d_outs):
        problems, wss = state
        np_, _Vp, _Qp, ks, ns, d, wsp, _ = HipGotImpl._arrays(problems, wss)
        d_outs = d_outs.contiguous()
        dmm = torch.empty(np_, 6, device=d_outs.device, dtype=torch.float32)
        with _timed("got_bwd"):
            _call("mdl_got_bwd_begin_multi", np_, HipGotImpl._rows(d_outs), HipGotImpl._rows(dmm), ks, ns, d, wsp, _stream())
        return dmm

    @staticmethod
    def backward_finish_multi(state, dmm_total):
        problems, wss = state
        np_, Vp, Qp, ks, ns, d, wsp, ptrs = HipGotImpl._arrays(problems, wss)
        dVs, dQs = [torch.empty_like(V) for V, _ in problems], [torch.empty_like(Q) for _, Q in problems]
        dmm_total = dmm_total.contiguous()
        with _timed("got_bwd_finish"):
            _call("mdl_got_bwd_finish_multi", np_, Vp, Qp, ptrs(dVs), ptrs(dQs), HipGotImpl._rows(dmm_total), ks, ns, d, wsp, _stream())
        return list(zip(dVs, dQs))


# ---- O1: multi-tensor AdamW with a device-side non-finite guard and in-stream clipping (mdl_adamw_*) ----
ADAMW_MAX_TENSORS = _native._DEFINES["MDL_ADAMW_MAX_TENSORS"]      # tensors per launch set
ADAMW_GUARD, ADAMW_CLIP, ADAMW_FINAL = (_native._DEFINES["MDL_ADAMW_" + k] for k in ("GUARD", "CLIP", "FINAL"))


def _f64_bits(x: float) -> int:
    """The bit pattern of a double: how the C ABI (which has no double) carries the hyperparameters without rounding them to fp32."""
    import struct
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def adamw_ptrs(tensors):
    """Host array of the device addresses of `tensors`, as the *_host arguments of mdl_adamw_* take them."""
    import ctypes
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def adamw_sizes(tensors):
    import ctypes
    return (ctypes.c_int64 * len(tensors))(*[t.numel() for t in tensors])


def adamw_workspace(stat_launches: int, device) -> torch.Tensor:
    """Scratch for the gradient statistics of a step with `stat_launches` statistics launches; every slot is rewritten each step."""
    return _ws_for("mdl_adamw_ws_bytes", device, int(stat_launches))


def adamw_grad_stats(nt, g_ptrs, numels, ws, slot, stat_launches):
    with _timed("adamw_stats"):
        _call("mdl_adamw_grad_stats", nt, g_ptrs, numels, ws, slot, stat_launches, _stream())


def adamw_update(nt, p_ptrs, g_ptrs, m_ptrs, v_ptrs, step_ptrs, numels, lr, beta1, beta2, eps, weight_decay, max_norm, flags, ws,
                 stat_launches):
    """p, exp_avg, exp_avg_sq of the set's tensors <- one AdamW step (nothing on a void step).  lr ... max_norm: Python floats."""
    with _timed("adamw_update"):
        _call("mdl_adamw_update", nt, p_ptrs, g_ptrs, m_ptrs, v_ptrs, step_ptrs, numels, _f64_bits(lr), _f64_bits(beta1), _f64_bits(beta2),
              _f64_bits(eps), _f64_bits(weight_decay), _f64_bits(max_norm), flags, ws, stat_launches, _stream())


def adamw_commit(nt, step_ptrs, flags, ws, stat_launches, grad_norm, skipped):
    """step += 1 for the set's tensors unless the step is void; with ADAMW_FINAL also grad_norm <- global norm, skipped += void."""
    with _timed("adamw_commit"):
        _call("mdl_adamw_commit", nt, step_ptrs, flags, ws, stat_launches, grad_norm, skipped, _stream())


# ---- S1: draw and gather a batch of bags from a device-resident feature store (mdl_bag_sample) ----
STORE_DTYPES = {torch.float32: _native._DEFINES["MDL_STORE_F32"], torch.float16: _native._DEFINES["MDL_STORE_F16"],
                torch.bfloat16: _native._DEFINES["MDL_STORE_BF16"]}
_U64 = (1 << 64) - 1


def _require_store(t, name="store_rows", on_device=True):
    """t is one tier of a store: [T, D] in one of the three store dtypes, unit column stride; on_device: and lives on a device."""
    if t.dim() != 2 or t.dtype not in STORE_DTYPES or (t.shape[1] > 1 and t.stride(1) != 1):
        raise RuntimeError("madeleine_amd: %s must be [T, D] float32 / float16 / bfloat16 with unit column stride" % name)
    if on_device and not t.is_cuda:
        raise RuntimeError("madeleine_amd: %s must live on a ROCm device (got %s); there is no CPU fallback" % (name, t.device))


def _require_draw_tables(off, bag, key_id, per):
    """The tables of the draw: off int64 [n_bags + 1], bag int32 [R], key_id None or int64 [R] (one entry per output `per`)."""
    _require(off, "off", torch.int64)
    _require(bag, "bag", torch.int32)
    if key_id is not None:
        _require(key_id, "key_id", torch.int64)
        if key_id.numel() != bag.numel():
            raise RuntimeError("madeleine_amd: key_id and bag must have one entry per output %s" % per)
    if off.dim() != 1 or off.numel() < 1:
        raise RuntimeError("madeleine_amd: off must be [n_bags + 1]")


def _require_pack_tables(cu, chunk_cu, R, n_rows, n_chunks, fn):
    """The tables of a pack: cu, chunk_cu int64 [R + 1], and their last entries n_rows, n_chunks as the caller `fn` passed them."""
    _require(cu, "cu", torch.int64)
    _require(chunk_cu, "chunk_cu", torch.int64)
    if cu.numel() != R + 1 or chunk_cu.numel() != R + 1:
        raise RuntimeError("madeleine_amd: cu and chunk_cu must be [R + 1] = [%d]" % (R + 1))
    if n_rows < 0 or n_chunks < 0:
        raise RuntimeError("madeleine_amd: %s needs n_rows >= 0 and n_chunks >= 0" % fn)


def _sample_outputs(R, N, D, device, return_indices):
    """out [R, N, D] fp32 and idx [R, N] int32 (None unless asked for)"""
    return (torch.empty(R, N, D, device=device, dtype=torch.float32),
            torch.empty(R, N, device=device, dtype=torch.int32) if return_indices else None)


def _pack_outputs(T, D, device, return_indices):
    """out [T, D] fp32, row_bag [T] int32 and idx [T] int32 (None unless asked for)"""
    return (torch.empty(T, D, device=device, dtype=torch.float32), torch.empty(T, device=device, dtype=torch.int32),
            torch.empty(T, device=device, dtype=torch.int32) if return_indices else None)


def bag_sample(store_rows, off, bag, key_id, n_tokens, seed, counter, return_indices=False):
    """out [R, n_tokens, D] fp32 <- for every output row r, n_tokens rows of stored bag bag[r] (rows off[bag[r]] .. off[bag[r] + 1] - 1
    of store_rows [T, D], fp32 / fp16 / bf16, unit column stride): without replacement in random order when the bag has at least
    n_tokens rows, with replacement when it is shorter, zeros where bag[r] == -1 (SlideDataset.sample_n + collate, in one launch on
    the current stream).  Row r's draw is a function of (seed, counter, key_id[r]) alone; key_id None: key_id[r] = bag[r].
    off int64 [n_bags + 1], bag int32 [R], key_id int64 [R], all on the device.  No autograd (features are inputs), no host read,
    no allocation beyond the outputs.  return_indices: also idx [R, n_tokens] int32, the chosen row inside the bag (-1: absent)."""
    _require_store(store_rows)
    _require_draw_tables(off, bag, key_id, "row")
    R, N, D = bag.numel(), int(n_tokens), store_rows.shape[1]
    out, idx = _sample_outputs(R, N, D, store_rows.device, return_indices)
    with _timed("bag_sample", ("byte", R * N * D * (4.0 + store_rows.element_size()))):
        _call("mdl_bag_sample", store_rows, STORE_DTYPES[store_rows.dtype], store_rows.stride(0) if store_rows.shape[0] > 1 else D,
              store_rows.shape[0], off, off.numel() - 1, bag, key_id, R, N, D, int(seed) & _U64, int(counter) & _U64, out, idx, _stream(),
              unsupported=("bag_sample: %d output rows of %d tokens exceed the int32 launch geometry", R, N))
    return (out, idx) if return_indices else out


# ---- S2: pack a batch of bags of different lengths from the store into one dense token tensor (mdl_bag_pack) ----
def bag_pack(store_rows, off, bag, key_id, cu, chunk_cu, n_rows, n_chunks, seed, counter, return_indices=False):
    """tokens [n_rows, D] fp32, row_bag [n_rows] int32 <- output bag r is rows cu[r] .. cu[r + 1] - 1: stored bag bag[r] taken whole
    and in stored order when it has at most L_r = cu[r + 1] - cu[r] rows, L_r of its rows drawn without replacement when it is longer
    (the rows bag_sample draws with n_tokens = L_r under the same seed, counter and key_id), zeros where bag[r] == -1.  row_bag is r
    on every row of bag r.  cu, chunk_cu int64 [R + 1] on the device (chunk_cu: the prefix sum of ceil(L_r / 64)); n_rows = cu[R] and
    n_chunks = chunk_cu[R] as host integers.  The other arguments, the checks and the byte accounting are bag_sample's.  No autograd,
    no host read, no allocation beyond the outputs.  return_indices: also idx [n_rows] int32 (row inside the bag, -1: zeros)."""
    _require_store(store_rows)
    _require_draw_tables(off, bag, key_id, "bag")
    R, T, D = bag.numel(), int(n_rows), store_rows.shape[1]
    _require_pack_tables(cu, chunk_cu, R, T, n_chunks, "bag_pack")
    out, row_bag, idx = _pack_outputs(T, D, store_rows.device, return_indices)
    if R == 0 or T == 0:       # nothing to pack (an empty tensor has no address to pass)
        return (out, row_bag, idx) if return_indices else (out, row_bag)
    with _timed("bag_pack", ("byte", T * D * (4.0 + store_rows.element_size()))):
        _call("mdl_bag_pack", store_rows, STORE_DTYPES[store_rows.dtype], store_rows.stride(0) if store_rows.shape[0] > 1 else D,
              store_rows.shape[0], off, off.numel() - 1, bag, key_id, cu, chunk_cu, R, int(n_chunks), T, D, int(seed) & _U64,
              int(counter) & _U64, out, row_bag, idx, _stream(),
              unsupported=("bag_pack: %d bags of %d rows in all exceed the int32 launch geometry", R, T))
    return (out, row_bag, idx) if return_indices else (out, row_bag)


# ---- S3 / S4: the same two gathers over a store in two tiers (mdl_bag_sample_tiered / mdl_bag_pack_tiered) ----
def _require_tiers(store_rows, host_rows):
    """(device, D, row stride, T_dev, T_total) of a two-tier store: store_rows [T_dev, D] on the device, host_rows [T_host, D] in PINNED
    host memory (None or no rows: no host tier), same dtype and row stride.  The pinned check is made here, before any native call: the
    kernel reads the host tier over PCIe, and a launch on pageable memory is a GPU fault, not an error code."""
    for t, name in ((store_rows, "store_rows"), (host_rows, "host_rows")):
        if t is not None:
            _require_store(t, name, on_device=False)
    if host_rows is not None and host_rows.shape[0] == 0:
        host_rows = None
    if host_rows is not None:
        if host_rows.dtype != store_rows.dtype or host_rows.shape[1] != store_rows.shape[1]:
            raise RuntimeError("madeleine_amd: the two tiers must share dtype and width (got %s x %d and %s x %d)"
                               % (store_rows.dtype, store_rows.shape[1], host_rows.dtype, host_rows.shape[1]))
        if host_rows.is_cuda or not host_rows.is_pinned():
            raise RuntimeError("madeleine_amd: host_rows must be pinned (registered) host memory (got %s, is_pinned() False): the "
                               "kernel reads it over PCIe and never touches pageable memory" % host_rows.device)
    _require_store(store_rows)      # on a device: asked after the pinned check, which holds whatever else is wrong with the call
    D = store_rows.shape[1]
    strides = {t.stride(0) for t in (store_rows, host_rows) if t is not None and t.shape[0] > 1} or {D}
    if len(strides) != 1:
        raise RuntimeError("madeleine_amd: the two tiers must share one row stride (got %s)" % sorted(strides))
    T_dev = store_rows.shape[0]
    return host_rows, D, strides.pop(), T_dev, T_dev + (0 if host_rows is None else host_rows.shape[0])


def bag_sample_tiered(store_rows, host_rows, off, bag, key_id, n_tokens, seed, counter, return_indices=False, host_wgs=0):
    """bag_sample over a store whose rows [0, T_dev) are store_rows (device) and rows [T_dev, T_total) host_rows (pinned host memory,
    read over PCIe by a grid of host_wgs persistent workgroups; 0: the library's default).  off and bag address rows of [0, T_total).
    The same draw, the same bits as bag_sample on the concatenation.  RuntimeError before any native call when host_rows is not
    pinned."""
    host_rows, D, stride, T_dev, T_total = _require_tiers(store_rows, host_rows)
    _require_draw_tables(off, bag, key_id, "row")
    R, N = bag.numel(), int(n_tokens)
    out, idx = _sample_outputs(R, N, D, store_rows.device, return_indices)
    with _timed("bag_sample", ("byte", R * N * D * (4.0 + store_rows.element_size()))):
        _call("mdl_bag_sample_tiered", store_rows if T_dev else None, host_rows, STORE_DTYPES[store_rows.dtype], stride, T_total, T_dev, off,
              off.numel() - 1, bag, key_id, R, N, D, int(seed) & _U64, int(counter) & _U64, out, idx, int(host_wgs), _stream(),
              unsupported=("bag_sample_tiered: %d output rows of %d tokens exceed the int32 launch geometry", R, N))
    return (out, idx) if return_indices else out


def bag_pack_tiered(store_rows, host_rows, off, bag, key_id, cu, chunk_cu, n_rows, n_chunks, seed, counter, return_indices=False,
                    host_wgs=0):
    """bag_pack over the two-tier store of bag_sample_tiered: the same outputs, bit for bit, as bag_pack on the concatenation."""
    host_rows, D, stride, T_dev, T_total = _require_tiers(store_rows, host_rows)
    _require_draw_tables(off, bag, key_id, "bag")
    R, T = bag.numel(), int(n_rows)
    _require_pack_tables(cu, chunk_cu, R, T, n_chunks, "bag_pack_tiered")
    out, row_bag, idx = _pack_outputs(T, D, store_rows.device, return_indices)
    if R == 0 or T == 0:       # nothing to pack (an empty tensor has no address to pass)
        return (out, row_bag, idx) if return_indices else (out, row_bag)
    with _timed("bag_pack", ("byte", T * D * (4.0 + store_rows.element_size()))):
        _call("mdl_bag_pack_tiered", store_rows if T_dev else None, host_rows, STORE_DTYPES[store_rows.dtype], stride, T_total, T_dev, off,
              off.numel() - 1, bag, key_id, cu, chunk_cu, R, int(n_chunks), T, D, int(seed) & _U64, int(counter) & _U64, out, row_bag, idx,
              int(host_wgs), _stream(),
              unsupported=("bag_pack_tiered: %d bags of %d rows in all exceed the int32 launch geometry", R, T))
    return (out, row_bag, idx) if return_indices else (out, row_bag)


# ---- S5: the column means of whole stored bags (mdl_bag_mean / mdl_bag_mean_tiered) ----
BAG_MEAN_ROWS = _native._DEFINES["MDL_BAG_MEAN_ROWS"]


def _require_mean_tables(bag, chunk_cu, n_chunks, fn):
    """The chunk table of a mean: chunk_cu int64 [R + 1] and its last entry n_chunks as the caller `fn` passed it."""
    _require(chunk_cu, "chunk_cu", torch.int64)
    if chunk_cu.numel() != bag.numel() + 1:
        raise RuntimeError("madeleine_amd: chunk_cu must be [R + 1] = [%d]" % (bag.numel() + 1))
    if n_chunks < 0:
        raise RuntimeError("madeleine_amd: %s needs n_chunks >= 0" % fn)


def _mean_outputs(R, D, n_chunks, device):
    """out [R, D] fp32 and the workspace of the partials (None when nothing is launched: out is then the zeros of absent stains)"""
    if R == 0 or n_chunks == 0:
        return torch.zeros(R, D, device=device, dtype=torch.float32), None
    ws = _ws_for("mdl_bag_mean_ws_bytes", device, int(n_chunks), D,
                 refusal=("bag_mean: %d chunks exceed the int32 launch geometry", int(n_chunks)))
    return torch.empty(R, D, device=device, dtype=torch.float32), ws


def bag_mean(store_rows, off, bag, chunk_cu, n_chunks):
    """out [R, D] fp32 <- out[r] is the mean over all rows of stored bag bag[r] (rows off[bag[r]] .. off[bag[r] + 1] - 1 of store_rows
    [T, D], fp32 / fp16 / bf16, unit column stride), zeros where bag[r] == -1.  chunk_cu int64 [R + 1] on the device: the prefix sum of
    ceil(n_r / BAG_MEAN_ROWS), n_r the rows of bag[r] (0 for -1); n_chunks = chunk_cu[R] as a host integer.  The bits of out[r] depend
    on the bag's rows alone (include/madeleine_amd.h, S5).  Two launches on the current stream, no autograd, no host read, no allocation
    beyond out and the workspace of the partials (n_chunks * D floats)."""
    _require_store(store_rows)
    _require_draw_tables(off, bag, None, "row")
    _require_mean_tables(bag, chunk_cu, n_chunks, "bag_mean")
    R, D = bag.numel(), store_rows.shape[1]
    out, ws = _mean_outputs(R, D, n_chunks, store_rows.device)
    if ws is None:
        return out
    with _timed("bag_mean"):       # (the bytes read are the listed bags' rows, which only the caller's host tables know)
        _call("mdl_bag_mean", store_rows, STORE_DTYPES[store_rows.dtype], store_rows.stride(0) if store_rows.shape[0] > 1 else D,
              store_rows.shape[0], off, off.numel() - 1, bag, chunk_cu, R, int(n_chunks), D, out, ws, _stream(),
              unsupported=("bag_mean: %d bags in %d chunks exceed the int32 launch geometry", R, int(n_chunks)))
    return out


def bag_mean_tiered(store_rows, host_rows, off, bag, chunk_cu, n_chunks, host_wgs=0):
    """bag_mean over the two-tier store of bag_sample_tiered: the same output, bit for bit, as bag_mean on the concatenation."""
    host_rows, D, stride, T_dev, T_total = _require_tiers(store_rows, host_rows)
    _require_draw_tables(off, bag, None, "row")
    _require_mean_tables(bag, chunk_cu, n_chunks, "bag_mean_tiered")
    R = bag.numel()
    out, ws = _mean_outputs(R, D, n_chunks, store_rows.device)
    if ws is None:
        return out
    with _timed("bag_mean"):
        _call("mdl_bag_mean_tiered", store_rows if T_dev else None, host_rows, STORE_DTYPES[store_rows.dtype], stride, T_total, T_dev, off,
              off.numel() - 1, bag, chunk_cu, R, int(n_chunks), D, out, ws, int(host_wgs), _stream(),
              unsupported=("bag_mean_tiered: %d bags in %d chunks exceed the int32 launch geometry", R, int(n_chunks)))
    return out


# ---- P1-P3: the few-shot linear probe (mdl_probe_fit / mdl_probe_scores / mdl_probe_metrics).  No autograd: embeddings are inputs ----
_PROBE_LIMITS = "linear probe supports at most %d training cases per problem, 2..%d classes and %d cases (got n_max %d, C %d, S %d)"


def _probe_refusal(n_max, d, C, S):      # (the signature of _logit_refusal; no limit on d)
    lim = _native._DEFINES
    return (_PROBE_LIMITS, lim["MDL_PROBE_MAX_TRAIN"], lim["MDL_PROBE_MAX_CLASSES"], lim["MDL_PROBE_MAX_CASES"], n_max, C, S)


def _probe_matrix(X):
    if X.dim() != 2 or X.dtype != torch.float32 or (X.shape[1] > 1 and X.stride(1) != 1):
        raise RuntimeError("madeleine_amd: X must be [S, d] float32 with unit column stride")
    if not X.is_cuda:
        raise RuntimeError("madeleine_amd: X must live on a ROCm device (got %s); there is no CPU fallback" % X.device)
    S, d = X.shape
    if S < 1 or d < 1:
        raise RuntimeError("madeleine_amd: X must have at least one row and one column")
    return S, d, (X.stride(0) if S > 1 else d)


def _problem_table(train_idx, n_train):
    """(P, n_max) of a problem table: train_idx [P, n_max] int32, n_train [P] int32."""
    _require(train_idx, "train_idx", torch.int32)
    _require(n_train, "n_train", torch.int32)
    if train_idx.dim() != 2 or train_idx.shape[0] < 1 or train_idx.shape[1] < 1 or n_train.shape != (train_idx.shape[0],):
        raise RuntimeError("madeleine_amd: train_idx must be [P, n_max] and n_train [P], P >= 1, n_max >= 1")
    return train_idx.shape


def _case_column(v, name, dtype, P, S):
    """Row stride of a per-case column: 0 for [S] (shared by all problems), S for [P, S]."""
    _require(v, name, dtype)
    if v.shape == (S,):
        return 0
    if v.shape == (P, S):
        return S
    raise RuntimeError("madeleine_amd: %s must be [S] or [P, S] = [%d, %d] (got %s)" % (name, P, S, tuple(v.shape)))


def _probe_problems(y, train_idx, n_train, S):
    """(P, n_max, ldy) of a problem list: y [S] (shared) or [P, S] int32, train_idx [P, n_max] int32, n_train [P] int32."""
    P, n_max = _problem_table(train_idx, n_train)
    return P, n_max, _case_column(y, "y", torch.int32, P, S)


def _class_scores(z, C):
    """(S, cols) of the decision values z [P, S, cols] of a C-class problem table."""
    _require(z, "z")
    cols = 1 if C == 2 else C
    if z.dim() != 3 or z.shape[0] < 1 or z.shape[1] < 1 or z.shape[2] != cols:
        raise RuntimeError("madeleine_amd: z must be [P, S, %d]" % cols)
    return z.shape[1], cols


def _same_problems(z, P):
    if P != z.shape[0]:
        raise RuntimeError("madeleine_amd: z holds %d problems, train_idx %d" % (z.shape[0], P))


def _logistic_fit(prefix, refusal_of, X, y, train_idx, n_train, n_classes, cost, gtol, max_iter):
    """probe_fit and logit_fit: mdl_<prefix>_fit behind its workspace query."""
    S, d, ldX = _probe_matrix(X)
    P, n_max, ldy = _probe_problems(y, train_idx, n_train, S)
    C = int(n_classes)
    refusal = refusal_of(n_max, d, C, S)
    ws = _ws_for("mdl_%s_fit_ws_bytes" % prefix, X.device, P, n_max, d, C, refusal=refusal)
    cols = 1 if C == 2 else C
    W = torch.empty(P, cols, d, device=X.device, dtype=torch.float32)
    b = torch.empty(P, cols, device=X.device, dtype=torch.float32)
    info = torch.empty(P, 4, device=X.device, dtype=torch.float32)
    with _timed(prefix + "_fit"):
        _call("mdl_%s_fit" % prefix, X, ldX, S, d, y, ldy, train_idx, n_train, P, n_max, C, float(cost), float(gtol), int(max_iter), W, b,
              info, ws, _stream(), unsupported=refusal)
    return W, b, info


def _class_metrics(prefix, refusal_of, z, y, train_idx, n_train, n_classes):
    """probe_metrics and logit_metrics: mdl_<prefix>_metrics behind its workspace query."""
    C = int(n_classes)
    S, _ = _class_scores(z, C)
    P, n_max, ldy = _probe_problems(y, train_idx, n_train, S)
    _same_problems(z, P)
    refusal = refusal_of(n_max, 1, C, S)
    ws = _ws_for("mdl_%s_metrics_ws_bytes" % prefix, z.device, P, S, C, refusal=refusal)
    confusion = torch.empty(P, C, C, device=z.device, dtype=torch.int32)
    auc = torch.empty(P, device=z.device, dtype=torch.float32)
    with _timed(prefix + "_metrics"):
        _call("mdl_%s_metrics" % prefix, z, y, ldy, train_idx, n_train, P, n_max, S, C, confusion, auc, ws, _stream(), unsupported=refusal)
    return confusion, auc


def probe_fit(X, y, train_idx, n_train, n_classes, cost=1.0, gtol=1e-4, max_iter=100):
    """(W [P, cols, d], b [P, cols], info [P, 4]) of P regularised logistic fits (P1 of the header; cols = 1 for two classes).
    info columns: Newton steps, converged, inf-norm of the gradient, CG steps.  Asynchronous, no host read."""
    return _logistic_fit("probe", _probe_refusal, X, y, train_idx, n_train, n_classes, cost, gtol, max_iter)


def probe_scores(X, W, b, n_classes):
    """z [P, S, cols] = X W_p^T + b_p: the decision values of all S cases under every fit (P2)."""
    S, d, ldX = _probe_matrix(X)
    C = int(n_classes)
    cols = 1 if C == 2 else C
    _require(W, "W")
    _require(b, "b")
    if W.dim() != 3 or W.shape[0] < 1 or W.shape[1:] != (cols, d) or b.shape != W.shape[:2]:
        raise RuntimeError("madeleine_amd: W must be [P, %d, %d] and b [P, %d]" % (cols, d, cols))
    P = W.shape[0]
    z = torch.empty(P, S, cols, device=X.device, dtype=torch.float32)
    with _timed("probe_scores", ("flop", 2.0 * P * S * cols * d)):
        _call("mdl_probe_scores", X, ldX, S, d, W, b, P, C, z, _stream(), unsupported=_probe_refusal(0, d, C, S))
    return z


def probe_metrics(z, y, train_idx, n_train, n_classes):
    """(confusion [P, C, C] int32, auc [P] fp32) over the test cases of every problem (P3): the labeled cases outside its train_idx."""
    return _class_metrics("probe", _probe_refusal, z, y, train_idx, n_train, n_classes)


# ---- L1-L2: the full-label linear probe (mdl_logit_fit / mdl_logit_metrics; the scores between them are probe_scores).  No autograd ----
_LOGIT_LIMITS = ("full-label linear probe supports at most %d training cases per problem, %d dimensions, 2..%d classes and %d cases "
                 "(got n_max %d, d %d, C %d, S %d)")


def _logit_refusal(n_max, d, C, S):
    lim = _native._DEFINES
    return (_LOGIT_LIMITS, lim["MDL_LOGIT_MAX_TRAIN"], lim["MDL_LOGIT_MAX_DIM"], lim["MDL_PROBE_MAX_CLASSES"], lim["MDL_PROBE_MAX_CASES"],
            n_max, d, C, S)


def logit_fit(X, y, train_idx, n_train, n_classes, cost=1.0, gtol=1e-4, max_iter=100):
    """(W [P, cols, d], b [P, cols], info [P, 4]) of P regularised logistic fits in the primal unknowns (L1 of the header): the objective,
    the stop rule and the info columns of probe_fit, for up to MDL_LOGIT_MAX_TRAIN training cases per problem.  Asynchronous, no host
    read."""
    return _logistic_fit("logit", _logit_refusal, X, y, train_idx, n_train, n_classes, cost, gtol, max_iter)


def logit_metrics(z, y, train_idx, n_train, n_classes):
    """probe_metrics for problem tables of up to MDL_LOGIT_MAX_TRAIN columns (L2): (confusion [P, C, C] int32, auc [P] fp32) over the
    test cases of every problem."""
    return _class_metrics("logit", _logit_refusal, z, y, train_idx, n_train, n_classes)


# ---- S1-S2: the survival probe (mdl_cox_fit / mdl_surv_metrics; the scores between them are probe_scores).  No autograd ----
_SURV_LIMITS = "survival probe supports at most %d training cases per fit and %d cases (got n_max %d, S %d)"


def _surv_refusal(n_max, S):
    d = _native._DEFINES
    return (_SURV_LIMITS, d["MDL_COX_MAX_TRAIN"], d["MDL_PROBE_MAX_CASES"], n_max, S)


def _surv_problems(time, event, train_idx, n_train, S):
    """(P, n_max, ldt, lde) of a problem list: time fp32 and event int32, each [S] (shared) or [P, S]; train_idx [P, n_max] int32,
    n_train [P] int32."""
    P, n_max = _problem_table(train_idx, n_train)
    return P, n_max, _case_column(time, "time", torch.float32, P, S), _case_column(event, "event", torch.int32, P, S)


def cox_fit(X, time, event, train_idx, n_train, cost=1.0, gtol=1e-3, max_iter=100):
    """(W [P, d], thr [P], info [P, 4]) of P ridge-penalised Cox fits (S1 of the header): thr the median of the training rows' decision
    values; info columns: Newton steps, converged, inf-norm of the gradient, CG steps.  gtol is relative to the gradient at w = 0.
    Asynchronous, no host read."""
    S, d, ldX = _probe_matrix(X)
    P, n_max, ldt, lde = _surv_problems(time, event, train_idx, n_train, S)
    refusal = _surv_refusal(n_max, S)
    ws = _ws_for("mdl_cox_order_fit_ws_bytes", X.device, P, n_max, d, refusal=refusal)
    W = torch.empty(P, d, device=X.device, dtype=torch.float32)
    thr = torch.empty(P, device=X.device, dtype=torch.float32)
    info = torch.empty(P, 4, device=X.device, dtype=torch.float32)
    with _timed("cox_fit"):
        _call("mdl_cox_fit", X, ldX, S, d, time, ldt, event, lde, train_idx, n_train, P, n_max, float(cost), float(gtol), int(max_iter), W,
              thr, info, ws, _stream(), unsupported=refusal)
    return W, thr, info


def survival_metrics(z, time, event, train_idx, n_train, thr):
    """(c_index [P] fp64, chi2 [P] fp64, counts [P, 6] int32) over the test cases of every problem (S2): the cases with follow-up outside
    its train_idx.  z [P, S]; counts columns: concordance numerator, comparable pairs, test cases, high-group size (z > thr), events in
    the low group, events in the high group."""
    _require(z, "z")
    _require(thr, "thr")
    if z.dim() != 2 or z.shape[0] < 1 or z.shape[1] < 1 or thr.shape != (z.shape[0],):
        raise RuntimeError("madeleine_amd: z must be [P, S] and thr [P]")
    S = z.shape[1]
    P, n_max, ldt, lde = _surv_problems(time, event, train_idx, n_train, S)
    _same_problems(z, P)
    refusal = _surv_refusal(n_max, S)
    ws = _ws_for("mdl_surv_metrics_ws_bytes", z.device, P, S, refusal=refusal)
    c_index = torch.empty(P, device=z.device, dtype=torch.float64)
    chi2 = torch.empty(P, device=z.device, dtype=torch.float64)
    counts = torch.empty(P, 6, device=z.device, dtype=torch.int32)
    with _timed("survival_metrics"):
        _call("mdl_surv_metrics", z, time, ldt, event, lde, train_idx, n_train, P, n_max, S, thr, c_index, chi2, counts, ws, _stream(),
              unsupported=refusal)
    return c_index, chi2, counts


# ---- R1-R3: the regression probe (mdl_ridge_fit / mdl_ridge_scores / mdl_regress_metrics, include/madeleine_amd_regress.h).  No autograd ----
_RIDGE_LIMITS = ("regression probe supports min(n_max, d) <= %d, at most %d training cases per problem, %d targets, %d penalties and "
                 "%d cases (got n_max %d, d %d, T %d, A %d, S %d)")
REG_COLUMNS = ("n_test", "pearson", "spearman", "r2", "mae", "rmse")      # the columns of regress_metrics, in the MDL_REG_* order
if [_native.REGRESS_DEFINES["MDL_REG_" + c.upper().replace("_", "")] for c in REG_COLUMNS] != list(range(6)):
    raise ImportError("madeleine_amd: REG_COLUMNS does not match the MDL_REG_* indices of %s" % _native._build.REGRESS_HEADER)


def _ridge_refusal(n_max, d, T, A, S):
    lim = _native.REGRESS_DEFINES
    return (_RIDGE_LIMITS, lim["MDL_RIDGE_MAX_SYS"], lim["MDL_RIDGE_MAX_TRAIN"], lim["MDL_RIDGE_MAX_TARGETS"], lim["MDL_RIDGE_MAX_ALPHAS"],
            _native._DEFINES["MDL_PROBE_MAX_CASES"], n_max, d, T, A, S)


def _target_matrix(Y, S):
    """(T, ldY) of the targets Y [S, T] float32 with unit column stride."""
    if Y.dim() != 2 or Y.dtype != torch.float32 or Y.shape[0] != S or Y.shape[1] < 1 or (Y.shape[1] > 1 and Y.stride(1) != 1):
        raise RuntimeError("madeleine_amd: Y must be [S, T] = [%d, T] float32 with unit column stride" % S)
    if not Y.is_cuda:
        raise RuntimeError("madeleine_amd: Y must live on a ROCm device (got %s); there is no CPU fallback" % Y.device)
    T = Y.shape[1]
    return T, (Y.stride(0) if S > 1 else T)


def _alpha_array(alphas):
    """(host float array, A) of a sequence of penalties; the library refuses the values it does not take."""
    values = [float(a) for a in alphas]
    return (ctypes.c_float * max(len(values), 1))(*values), len(values)


def ridge_fit(X, Y, train_idx, n_train, alphas):
    """(W [P, A, T, d], b [P, A, T], info [P, A, 2]) of P x A x T ridge fits with an unpenalised intercept (R1 of the regression header):
    X [S, d], Y [S, T] (NaN: no value), alphas a host sequence of A penalties > 0.  info columns: factorised (1 / 0), smallest pivot over
    largest diagonal entry.  Asynchronous, no host read."""
    S, d, ldX = _probe_matrix(X)
    T, ldY = _target_matrix(Y, S)
    P, n_max = _problem_table(train_idx, n_train)
    arr, A = _alpha_array(alphas)
    refusal = _ridge_refusal(n_max, d, T, A, S)
    ws = _ws_for("mdl_ridge_fit_ws_bytes", X.device, P, n_max, d, T, A, refusal=refusal)
    W = torch.empty(P, A, T, d, device=X.device, dtype=torch.float32)
    b = torch.empty(P, A, T, device=X.device, dtype=torch.float32)
    info = torch.empty(P, A, 2, device=X.device, dtype=torch.float32)
    with _timed("ridge_fit"):
        _call("mdl_ridge_fit", X, ldX, S, d, Y, ldY, T, train_idx, n_train, P, n_max, arr, A, W, b, info, ws, _stream(), unsupported=refusal)
    return W, b, info


def ridge_scores(X, W, b):
    """Z [..., S] = X W^T + b for W [..., d] and b [...] (R2): the decision values of all S cases under every fit, each list contiguous."""
    S, d, ldX = _probe_matrix(X)
    _require(W, "W")
    _require(b, "b")
    if W.dim() < 2 or W.shape[-1] != d or b.shape != W.shape[:-1] or b.numel() < 1:
        raise RuntimeError("madeleine_amd: W must be [..., %d] and b its leading shape" % d)
    L = b.numel()
    Z = torch.empty(*b.shape, S, device=X.device, dtype=torch.float32)
    with _timed("ridge_scores", ("flop", 2.0 * L * S * d)):
        _call("mdl_ridge_scores", X, ldX, S, d, W, b, L, Z, _stream())
    return Z


def regress_metrics(Z, Y, train_idx, n_train, return_sums=False):
    """metrics [P, A, T, 6] fp64 over the test cases of every (p, t) -- Y[i, t] finite and i outside train_idx[p] -- for every penalty
    (R3); columns REG_COLUMNS.  Z [P, A, T, S].  return_sums: also the int64 [P, A, T, 6] n, sum Rz, sum Ry, sum Rz^2, sum Ry^2, sum Rz Ry
    of the doubled average ranks Spearman's rho is formed from."""
    _require(Z, "Z")
    if Z.dim() != 4 or min(Z.shape) < 1:
        raise RuntimeError("madeleine_amd: Z must be [P, A, T, S]")
    P, A, T, S = Z.shape
    Ty, ldY = _target_matrix(Y, S)
    Pt, n_max = _problem_table(train_idx, n_train)
    _same_problems(Z, Pt)
    if Ty != T:
        raise RuntimeError("madeleine_amd: Z holds %d targets, Y %d" % (T, Ty))
    refusal = _ridge_refusal(n_max, 1, T, A, S)
    ws = _ws_for("mdl_regress_metrics_ws_bytes", Z.device, P, S, T, refusal=refusal)
    metrics = torch.empty(P, A, T, 6, device=Z.device, dtype=torch.float64)
    sums = torch.empty(P, A, T, 6, device=Z.device, dtype=torch.int64) if return_sums else None
    with _timed("regress_metrics"):
        _call("mdl_regress_metrics", Z, Y, ldY, T, train_idx, n_train, P, n_max, S, A, metrics, sums, ws, _stream(), unsupported=refusal)
    return (metrics, sums) if return_sums else metrics


# ---- A-map: the attention read-out (mdl_attn_softmax / mdl_attn_rank).  Forward only, no autograd: raw scores are inputs ----
ATTN_ROWS = _native._DEFINES["MDL_ATTN_ROWS"]
ATTN_SORT_KEYS = _native._DEFINES["MDL_ATTN_SORT_KEYS"]
_ATTN_LIMITS = "attention read-out supports 1, 2, 4 or 8 heads and T, R and its launch grids within int32 (got T %d, R %d, H %d, k %d)"


def _attn_args(scores, cu, fn):
    """(T, H, ld, R) of a read-out call: scores [T, H] fp32 on the device with unit column stride (any row stride), cu int64 [R + 1]."""
    if scores.dim() != 2 or scores.dtype != torch.float32 or (scores.shape[1] > 1 and scores.stride(1) != 1):
        raise RuntimeError("madeleine_amd: %s needs scores [T, H] float32 with unit column stride" % fn)
    if not scores.is_cuda:
        raise RuntimeError("madeleine_amd: scores must live on a ROCm device (got %s); there is no CPU fallback" % scores.device)
    _require(cu, "cu_seqlens", torch.int64)
    if cu.dim() != 1 or cu.numel() < 1:
        raise RuntimeError("madeleine_amd: cu_seqlens must be [R + 1]")
    T, H = scores.shape
    if H < 1:
        raise RuntimeError("madeleine_amd: %s needs at least one head" % fn)
    return T, H, (scores.stride(0) if T > 1 else H), cu.numel() - 1


def attn_softmax(scores, cu):
    """(attn [T, H], m [R, H], l [R, H]) of raw scores [T, H] (fp32, any row stride) over the bags of cu int64 [R + 1] on the device: per
    bag and head the maximum, l = sum expf(s - m) and attn = expf(s - m) / l.  A bag's bits depend on its own scores alone (include/
    madeleine_amd.h, A-map).  An empty bag has m = -inf, l = 0.  Six launches on the current stream, no host read."""
    T, H, ld, R = _attn_args(scores, cu, "attn_softmax")
    dev = scores.device
    refusal = (_ATTN_LIMITS, T, R, H, 0)
    attn = torch.empty(T, H, device=dev, dtype=torch.float32)
    if R == 0 or T == 0:
        return attn, torch.full((R, H), float("-inf"), device=dev), torch.zeros(R, H, device=dev)
    m = torch.empty(R, H, device=dev, dtype=torch.float32)
    l = torch.empty(R, H, device=dev, dtype=torch.float32)
    ws = _ws_for("mdl_attn_map_ws_bytes", dev, T, R, H, refusal=refusal)
    with _timed("attn_softmax", ("byte", 16.0 * T * H)):
        _call("mdl_attn_softmax", scores, ld, cu, T, R, H, attn, m, l, ws, _stream(), unsupported=refusal)
    return attn, m, l


def attn_rank(scores, cu, k=0, percentile=True):
    """(order [H, T] int32, pct [T, H] fp32 or None, topk_idx [R, H, k] int32 or None, topk_val [R, H, k] fp32 or None) of raw scores
    [T, H] over the bags of cu: order[h, cu[r] + j] is the row inside bag r of its j-th highest score in head h (ties: the lower row
    first; -0 == +0, NaNs equal and above +inf), pct the percentile rank rankdata(s, 'average') / n * 100 of every row, topk_* the
    first min(k, n) entries of order with their raw scores, padded with -1 / -inf (None for k == 0).  Exact: an LSD radix sort on HIP
    kernels, the same launches for any number of bags; no host read."""
    T, H, ld, R = _attn_args(scores, cu, "attn_rank")
    k = int(k)
    if k < 0:
        raise RuntimeError("madeleine_amd: attn_rank needs k >= 0 (got %d)" % k)
    dev = scores.device
    refusal = (_ATTN_LIMITS, T, R, H, k)
    order = torch.empty(H, T, device=dev, dtype=torch.int32)
    pct = torch.empty(T, H, device=dev, dtype=torch.float32) if percentile else None
    if R == 0 or T == 0:      # nothing is launched: the padding of empty bags is written here
        return order, pct, (torch.full((R, H, k), -1, device=dev, dtype=torch.int32) if k else None), \
            (torch.full((R, H, k), float("-inf"), device=dev, dtype=torch.float32) if k else None)
    ti = torch.empty(R, H, k, device=dev, dtype=torch.int32) if k else None
    tv = torch.empty(R, H, k, device=dev, dtype=torch.float32) if k else None
    ws = _ws_for("mdl_attn_map_ws_bytes", dev, T, R, H, refusal=refusal)
    with _timed("attn_rank", ("byte", 40.0 * T * H)):
        _call("mdl_attn_rank", scores, ld, cu, T, R, H, k, order, pct, ti, tv, ws, _stream(), unsupported=refusal)
    return order, pct, ti, tv


# ---- V1: attention heatmaps (mdl_heat_render, include/madeleine_amd_view.h).  Forward only, exact integer arithmetic ----
HEAT_REC = _native.VIEW_DEFINES["MDL_HEAT_REC"]
HEAT_MAX_R = _native.VIEW_DEFINES["MDL_HEAT_MAX_R"]
HEAT_MAX_SIDE = _native.VIEW_DEFINES["MDL_HEAT_MAX_SIDE"]
HEAT_TAP_SUM = _native.VIEW_DEFINES["MDL_HEAT_TAP_SUM"]
HEAT_WS_PER_PLANE_PIXEL = _native.VIEW_DEFINES["MDL_HEAT_WS_PER_PLANE_PIXEL"]
_HEAT_LIMITS = ("heat_render supports a blur radius <= %d, canvases <= %d a side, patch sizes <= 2^24, T < 2^24 and C * pixels within "
                "int32 (got T %d, R %d, C %d, pixels %d, r %d)")


HEAT_MARKS = _native.VIEW_DEFINES["MDL_HEAT_MARKS"]
# bytes per pixel and channel of the tile passes: the memset writes 8; hv_blur_rows reads acc (8) and writes S1, N1 (16); hv_blur_cols
# reads acc, S1, N1 (24) and writes level, covered, rgba (2 + 1 + 4).  Halo re-reads and the footprint atomics are not in it.
HEAT_PLANE_BYTES = {"clear": 8, "blur_rows": 8 + 16, "blur_cols_colour": 24 + 7}


def heat_render(xy, cu, values, records, n_pixels, ds, taps, lut, alpha=255, base=None, records_dev=None, marks=None):
    """(level uint16 [C * P], covered uint8 [C * P], rgba uint8 [C * P, 4]) of R bags x C channels: the render contract of
    include/madeleine_amd_view.h.  xy [T, 2] int32, cu [R + 1] int64, values [T, C] fp32 (unit column stride, any row stride), lut
    [256, 4] uint8 and base ([P, 3] uint8 or None) on the device; records [R, 6] int64 (ps, ox, oy, W, H, first pixel) and taps
    [2 r + 1] int32 on the HOST (they are validated there; records_dev: their device copy when the caller already has one, else one
    non-blocking upload).  P = n_pixels.  Bag b's block of every output is [C, H, W] from element C * off.  One memset and four
    launches on the current stream, no host read.  marks: a host array of HEAT_MARKS event handles for mdl_heat_render_marked
    (heat_render_stages)."""
    if xy.dim() != 2 or xy.shape[1] != 2:
        raise RuntimeError("madeleine_amd: heat_render needs xy [T, 2] int32")
    _require(xy, "xy", torch.int32)
    _require(cu, "cu_seqlens", torch.int64)
    if cu.dim() != 1 or cu.numel() < 1:
        raise RuntimeError("madeleine_amd: cu_seqlens must be [R + 1]")
    T, R = xy.shape[0], cu.numel() - 1
    if values.dim() != 2 or values.dtype != torch.float32 or not values.is_cuda or values.shape[0] != T or values.shape[1] < 1 or \
            (values.shape[1] > 1 and values.stride(1) != 1):
        raise RuntimeError("madeleine_amd: heat_render needs values [T, C] float32 on the device with unit column stride")
    C = values.shape[1]
    ld = values.stride(0) if T > 1 else C
    if records.device.type != "cpu" or records.dtype != torch.int64 or tuple(records.shape) != (R, HEAT_REC) or not records.is_contiguous():
        raise RuntimeError("madeleine_amd: heat_render needs records [R, %d] int64, contiguous, on the host" % HEAT_REC)
    if taps.device.type != "cpu" or taps.dtype != torch.int32 or taps.dim() != 1 or taps.numel() % 2 != 1 or not taps.is_contiguous():
        raise RuntimeError("madeleine_amd: heat_render needs taps [2 r + 1] int32, contiguous, on the host")
    r, P, dev = taps.numel() // 2, int(n_pixels), xy.device
    _require(lut, "lut", torch.uint8)
    if tuple(lut.shape) != (256, 4):
        raise RuntimeError("madeleine_amd: heat_render needs lut [256, 4] uint8")
    if base is not None:
        _require(base, "base", torch.uint8)
        if base.numel() != 3 * P:
            raise RuntimeError("madeleine_amd: heat_render needs base [P, 3] uint8 (P = %d, got %d bytes)" % (P, base.numel()))
    if records_dev is None:
        records_dev = h2d(records, dev)
    _require(records_dev, "records_dev", torch.int64)
    if tuple(records_dev.shape) != (R, HEAT_REC):
        raise RuntimeError("madeleine_amd: records_dev must be the [R, %d] device copy of records" % HEAT_REC)
    refusal = (_HEAT_LIMITS, HEAT_MAX_R, HEAT_MAX_SIDE, T, R, C, P, r)
    ws = _ws_for("mdl_heat_ws_bytes", dev, P, R, C, refusal=refusal)
    level = torch.empty(C * P, device=dev, dtype=torch.uint16)
    covered = torch.empty(C * P, device=dev, dtype=torch.uint8)
    rgba = torch.empty(C * P, 4, device=dev, dtype=torch.uint8)
    with _timed("heat_render", ("byte", float(C) * P * sum(HEAT_PLANE_BYTES.values()) + (8.0 + 4.0 * C) * T)):
        if marks is None:
            _call("mdl_heat_render", xy, cu, values, ld, T, R, C, records, records_dev, P, int(ds), taps, r, lut, base, int(alpha), level,
                  covered, rgba, ws, _stream(), unsupported=refusal)
        else:
            _call("mdl_heat_render_marked", xy, cu, values, ld, T, R, C, records, records_dev, P, int(ds), taps, r, lut, base, int(alpha),
                  level, covered, rgba, ws, marks, _stream(), unsupported=refusal)
    return level, covered, rgba


HEAT_STAGES = ("clear", "accumulate", "blur_rows", "blur_cols_colour")


def heat_render_stages(*args, **kwargs):
    """heat_render with its stages timed by device events: (level, covered, rgba, {"clear": the memset and the tile table,
    "accumulate", "blur_rows", "blur_cols_colour": the column pass with level and colour} in ms).  Needs R >= 1 and P >= 1.
    Synchronises the stream: for tools/exp_heatmap.py, not for a pipeline."""
    import ctypes
    events = [torch.cuda.Event(enable_timing=True) for _ in range(HEAT_MARKS)]
    for ev in events:
        ev.record()                    # an event's handle exists once it has been recorded
    marks = (ctypes.c_void_p * HEAT_MARKS)(*[ev.cuda_event for ev in events])
    out = heat_render(*args, marks=marks, **kwargs)
    events[-1].synchronize()
    ms = [events[i].elapsed_time(events[i + 1]) for i in range(HEAT_MARKS - 1)]
    return out + (dict(zip(HEAT_STAGES, ms)),)


# ---- R1: the smooth rank (mdl_smooth_rank).  fp64 Gram, tridiagonal eigenvalues, entropy.  No autograd: embeddings are inputs ----
RANK_MAX_K = _native._DEFINES["MDL_RANK_MAX_K"]
RANK_GRAM_ROWS, RANK_GRAM_MAX_CHUNKS, RANK_GRAM_TILE, RANK_TRI_ROWS = (
    _native._DEFINES["MDL_RANK_" + k] for k in ("GRAM_ROWS", "GRAM_MAX_CHUNKS", "GRAM_TILE", "TRI_ROWS"))
_RANK_LIMIT = "smooth_rank supports min(n, d) <= %d (got E [%d, %d])"


def smooth_rank_supported(E) -> bool:
    """Whether smooth_rank takes E: a non-empty 2-D fp32 tensor on a ROCm device with unit column stride, min(n, d) <= RANK_MAX_K."""
    return (torch.is_tensor(E) and E.is_cuda and E.dtype == torch.float32 and E.dim() == 2 and min(E.shape) >= 1
            and min(E.shape) <= RANK_MAX_K and (E.shape[1] == 1 or E.stride(1) == 1) and (E.shape[0] == 1 or E.stride(0) >= E.shape[1]))


def _rank_call(E, eps, marks=None):
    """(out [2] fp64: exp(H), H; sigma [k] fp64) of mdl_smooth_rank -- or, with four event handles in `marks`, of _marked."""
    if not torch.is_tensor(E) or E.dtype != torch.float32 or E.dim() != 2:
        raise ValueError("madeleine_amd: smooth_rank needs a 2-D float32 tensor (got %s)"
                         % ("%s %s" % (E.dtype, tuple(E.shape)) if torch.is_tensor(E) else type(E).__name__))
    n, d = E.shape
    if n < 1 or d < 1:
        raise ValueError("madeleine_amd: smooth_rank needs at least one row and one column (got [%d, %d])" % (n, d))
    k = min(n, d)
    if k > RANK_MAX_K:
        raise NotImplementedError("madeleine_amd: " + _RANK_LIMIT % (RANK_MAX_K, n, d))
    if not E.is_cuda:
        raise ValueError("madeleine_amd: E must live on a ROCm device (got %s); smooth_rank_measure is the host function" % E.device)
    ld = E.stride(0) if n > 1 else d
    if (d > 1 and E.stride(1) != 1) or ld < d:
        raise ValueError("madeleine_amd: smooth_rank needs unit column stride and a row stride >= d (got strides %s)" % (tuple(E.stride()),))
    dev = E.device
    refusal = (_RANK_LIMIT, RANK_MAX_K, n, d)
    ws = _ws_for("mdl_smooth_rank_ws_bytes", dev, n, d, refusal=refusal)
    sigma = torch.empty(k, device=dev, dtype=torch.float64)
    out = torch.empty(2, device=dev, dtype=torch.float64)
    with _timed("smooth_rank", ("flop", 2.0 * max(n, d) * k * k)):
        if marks is None:
            _call("mdl_smooth_rank", E, ld, n, d, _f64_bits(eps), sigma, out, ws, _stream(), unsupported=refusal)
        else:
            _call("mdl_smooth_rank_marked", E, ld, n, d, _f64_bits(eps), sigma, out, ws, marks, _stream(), unsupported=refusal)
    return out, sigma


def smooth_rank(E, eps=1e-7):
    """(rank, sigma) of E [n, d] fp32 on the device (unit column stride, any row stride >= d): rank a 0-d fp64 device tensor, the
    UNROUNDED exp(entropy of p), p = sigma / sum(sigma) + eps; sigma [min(n, d)] fp64 on the device, the singular values, descending.
    utils.smooth_rank_measure without the rounding, the copy to the host or the CPU SVD (include/madeleine_amd.h, R1): 2 min(n, d)
    launches on the current stream, no host read, no upload; the workspace comes from torch's allocator.  ValueError for a tensor that is
    not 2-D float32 on a ROCm device, NotImplementedError for min(n, d) > RANK_MAX_K."""
    out, sigma = _rank_call(E, eps)
    return out[0], sigma


def smooth_rank_stages(E, eps=1e-7):
    """smooth_rank with its three stages timed by device events: (rank, sigma, {"gram", "tridiagonal", "eigen_finish"} in ms).
    Synchronises the stream: for tools/exp_rank.py, not for a training loop."""
    import ctypes
    events = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    for ev in events:
        ev.record()                    # an event's handle exists once it has been recorded
    marks = (ctypes.c_void_p * 4)(*[ev.cuda_event for ev in events])
    out, sigma = _rank_call(E, eps, marks)
    events[3].synchronize()
    ms = [events[i].elapsed_time(events[i + 1]) for i in range(3)]
    return out[0], sigma, dict(zip(("gram", "tridiagonal", "eigen_finish"), ms))


# ---- X1: cross-stain retrieval (mdl_retrieval).  Pair ranks and top-k neighbours from streamed similarity tiles.  No autograd ----
RETR_MAX_ROWS, RETR_MAX_D, RETR_MAX_K, RETR_MAX_CHUNKS, RETR_ROW_BLOCK, RETR_COL_TILE, RETR_TARGET_WGS = (
    _native._DEFINES["MDL_RETR_" + k] for k in ("MAX_ROWS", "MAX_D", "MAX_K", "MAX_CHUNKS", "ROW_BLOCK", "COL_TILE", "TARGET_WGS"))
RETR_METRICS = {"cosine": _native._DEFINES["MDL_RETR_COSINE"], "dot": _native._DEFINES["MDL_RETR_DOT"]}
_RETR_LIMIT = ("retrieval supports n, m <= %d, d <= %d, k <= %d and col_chunks <= %d "
               "(got Q [%d, %d], K [%d, %d], k %d, col_chunks %d)")

Retrieval = collections.namedtuple("Retrieval", ("greater", "equal", "pair_sim", "topk_idx", "topk_val"))


def retrieval_chunks(n, m, col_chunks=0):
    """(chunks, tiles_per_chunk) the launcher uses for n queries and m gallery rows: col_chunks (0: its own choice) cut down to whole
    RETR_COL_TILE-row tiles.  Host arithmetic, the same as csrc/retrieval.hip's."""
    row_blocks, col_tiles = -(-n // RETR_ROW_BLOCK), -(-m // RETR_COL_TILE)
    c = col_chunks if col_chunks > 0 else -(-RETR_TARGET_WGS // row_blocks)
    c = max(1, min(c, RETR_MAX_CHUNKS, col_tiles))
    per = -(-col_tiles // c)
    return -(-col_tiles // per), per


def _retr_matrix(t, name):
    if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 2:
        raise ValueError("madeleine_amd: retrieval needs %s as a 2-D float32 tensor (got %s)"
                         % (name, "%s %s" % (t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__))
    rows, d = t.shape
    if rows < 1 or d < 1:
        raise ValueError("madeleine_amd: retrieval needs at least one row and one column in %s (got [%d, %d])" % (name, rows, d))
    ld = t.stride(0) if rows > 1 else d
    if (d > 1 and t.stride(1) != 1) or ld < d:
        raise ValueError("madeleine_amd: retrieval needs unit column stride and a row stride >= d in %s (got strides %s)"
                         % (name, tuple(t.stride())))
    return rows, d, ld


def retrieval(Q, K=None, k=0, metric='cosine', paired=True, exclude_diag=False, col_chunks=0):
    """Retrieval of the rows of K [m, d] by the rows of Q [n, d] (fp32 on the device, unit column stride, any row stride >= d; K None: Q
    itself) -> Retrieval(greater, equal, pair_sim, topk_idx, topk_val) on the device.  metric 'cosine' (rows scaled by 1 / max(|x|,
    1e-12)) or 'dot'.  paired (n <= m, the partner of query i is gallery row i): pair_sim [n] fp32 = s_ii, greater / equal [n] int32 =
    the gallery rows j != i whose similarity comes before / ties with s_ii; a NaN s_ii gives m - 1 and 0.  k >= 1: topk_idx [n, k]
    int32, topk_val [n, k] fp32, the k best gallery rows of every query (padding -1 / -inf), column i skipped for row i with
    exclude_diag (not together with paired).  Order: descending value, -0 = +0, NaNs below -inf, ties by the lower index.  Fields of a
    mode that is off are None.  Exact-fp32 MFMA similarities from streamed tiles (include/madeleine_amd.h, X1): the [n, m] matrix is
    never formed, the bits of s_ij depend on the two rows alone and no output depends on col_chunks (0: the launcher's choice).  Three
    launches on the current stream, no host read.  ValueError for dtype / device / shape / arguments, NotImplementedError past the
    limits."""
    K = Q if K is None else K
    n, d, ldq = _retr_matrix(Q, "Q")
    m, dk, ldk = _retr_matrix(K, "K")
    if dk != d:
        raise ValueError("madeleine_amd: retrieval needs Q and K of one width (got %d and %d)" % (d, dk))
    if metric not in RETR_METRICS:
        raise ValueError("madeleine_amd: retrieval metric must be 'cosine' or 'dot' (got %r)" % (metric,))
    k, col_chunks, paired, exclude_diag = int(k), int(col_chunks), bool(paired), bool(exclude_diag)
    if k < 0 or col_chunks < 0:
        raise ValueError("madeleine_amd: retrieval needs k >= 0 and col_chunks >= 0 (got %d, %d)" % (k, col_chunks))
    if paired and exclude_diag:
        raise ValueError("madeleine_amd: retrieval takes paired or exclude_diag, not both")
    if paired and n > m:
        raise ValueError("madeleine_amd: paired retrieval needs n <= m (got %d queries, %d gallery rows)" % (n, m))
    if not paired and k == 0:
        raise ValueError("madeleine_amd: retrieval needs paired=True or k >= 1")
    refusal = (_RETR_LIMIT, RETR_MAX_ROWS, RETR_MAX_D, RETR_MAX_K, RETR_MAX_CHUNKS, n, d, m, d, k, col_chunks)
    if max(n, m) > RETR_MAX_ROWS or d > RETR_MAX_D or k > RETR_MAX_K or col_chunks > RETR_MAX_CHUNKS:
        raise NotImplementedError("madeleine_amd: " + refusal[0] % refusal[1:])
    if not Q.is_cuda or K.device != Q.device:
        raise ValueError("madeleine_amd: Q and K must live on one ROCm device (got %s, %s); there is no CPU fallback" % (Q.device, K.device))
    dev = Q.device
    ws = _ws_for("mdl_retrieval_ws_bytes", dev, n, m, d, k, col_chunks, refusal=refusal)
    greater = torch.empty(n, device=dev, dtype=torch.int32) if paired else None
    equal = torch.empty(n, device=dev, dtype=torch.int32) if paired else None
    pair_sim = torch.empty(n, device=dev, dtype=torch.float32) if paired else None
    ti = torch.empty(n, k, device=dev, dtype=torch.int32) if k else None
    tv = torch.empty(n, k, device=dev, dtype=torch.float32) if k else None
    with _timed("retrieval", ("flop", 2.0 * n * m * d)):
        _call("mdl_retrieval", Q, ldq, K, ldk, n, m, d, RETR_METRICS[metric], int(paired), int(exclude_diag), k, col_chunks, greater, equal,
              pair_sim, ti, tv, ws, _stream(), unsupported=refusal)
    return Retrieval(greater, equal, pair_sim, ti, tv)


# ---- B1-B3: the test-set bootstrap of the probes' metrics (include/madeleine_amd_stats.h).  Exact integer counts, no autograd ----
BOOT_REP_BLOCK = _native.STATS_DEFINES["MDL_BOOT_REP_BLOCK"]
BOOT_SURV_MAX_TEST = _native.STATS_DEFINES["MDL_BOOT_SURV_MAX_TEST"]
BOOT_LDS_RAISE_FROM = _native.STATS_DEFINES["MDL_BOOT_LDS_RAISE_FROM"]
_BOOT_LIMITS = ("bootstrap counts support at most %d cases (survival: %d), %d training cases per problem (survival: %d), 2..%d classes "
                "and replicates within int32 (got n_max %d, C %d, S %d, R %d)")


def _boot_refusal(n_max, C, S, R):
    d = _native._DEFINES
    return (_BOOT_LIMITS, d["MDL_PROBE_MAX_CASES"], BOOT_SURV_MAX_TEST, d["MDL_LOGIT_MAX_TRAIN"], d["MDL_COX_MAX_TRAIN"],
            d["MDL_PROBE_MAX_CLASSES"], n_max, C, S, R)


def _boot_group(group, n, what):
    _require(group, "group", torch.int32)
    if group.shape != (n,):
        raise RuntimeError("madeleine_amd: group must be int32 [%d], one entry per %s (got %s)" % (n, what, tuple(group.shape)))
    return group


def _boot_replicates(replicates):
    R = int(replicates)
    if R < 0:
        raise RuntimeError("madeleine_amd: the bootstrap needs replicates >= 0 (got %d)" % R)
    return R


def boot_weights(seed, group, replicates, n_cases):
    """w [G, R + 1, S] uint16: the resampling weights of the groups group [G] (int32, on the device) -- w[g, r] is the count vector of S
    draws from [0, S), a function of (seed, group[g], r, S) alone, and w[g, 0] is all ones (B1 of include/madeleine_amd_stats.h).
    One launch on the current stream, no host read."""
    R, S = _boot_replicates(replicates), int(n_cases)
    if group.dim() != 1 or group.numel() < 1 or S < 1:
        raise RuntimeError("madeleine_amd: boot_weights needs group [G], G >= 1, and n_cases >= 1")
    G = _boot_group(group, group.numel(), "group").numel()
    w = torch.empty(G, R + 1, S, device=group.device, dtype=torch.uint16)
    with _timed("boot_weights"):
        _call("mdl_boot_weights", int(seed) & 0xFFFFFFFFFFFFFFFF, group, G, R, S, w, _stream(), unsupported=_boot_refusal(0, 2, S, R))
    return w


def boot_class_counts(z, y, train_idx, n_train, n_classes, group, seed, replicates):
    """(confusion [P, R + 1, C, C] int32, auc_num [P, R + 1, cols] int64) of every problem of probe_metrics / logit_metrics under R
    resamples of the cohort (B2): per replicate the weighted confusion matrix of the test cases and, per class column (class 1 for two
    classes), the weighted Mann-Whitney numerator sum w_i w_j (2 [s_i > s_j] + [s_i == s_j]).  Problem p uses the weights of
    (seed, group[p], r, S): problems of one group are resampled together.  Replicate 0 is the sample itself.  A problem with a NaN test
    score has auc_num -1.  Three launches on the current stream, no host read."""
    C = int(n_classes)
    S, cols = _class_scores(z, C)
    P, n_max, ldy = _probe_problems(y, train_idx, n_train, S)
    _same_problems(z, P)
    _boot_group(group, P, "problem")
    R = _boot_replicates(replicates)
    refusal = _boot_refusal(n_max, C, S, R)
    ws = _ws_for("mdl_boot_class_ws_bytes", z.device, P, S, C, refusal=refusal)
    confusion = torch.empty(P, R + 1, C, C, device=z.device, dtype=torch.int32)
    auc_num = torch.empty(P, R + 1, cols, device=z.device, dtype=torch.int64)
    with _timed("boot_class_counts"):
        _call("mdl_boot_class_counts", z, y, ldy, train_idx, n_train, P, n_max, S, C, group, int(seed) & 0xFFFFFFFFFFFFFFFF, R, confusion,
              auc_num, ws, _stream(), unsupported=refusal)
    return confusion, auc_num


def boot_surv_counts(z, time, event, train_idx, n_train, group, seed, replicates):
    """counts [P, R + 1, 2] int64 of every problem of survival_metrics under R resamples of the cohort (B3): the weighted concordance
    numerator and the weighted number of comparable pairs, so that the C-index of a replicate is counts[..., 0] / (2 counts[..., 1]).
    Replicate 0 equals the first two columns of survival_metrics' counts.  z [P, S]; S <= BOOT_SURV_MAX_TEST.  One launch on the
    current stream, no host read."""
    _require(z, "z")
    if z.dim() != 2 or z.shape[0] < 1 or z.shape[1] < 1:
        raise RuntimeError("madeleine_amd: z must be [P, S]")
    S = z.shape[1]
    P, n_max, ldt, lde = _surv_problems(time, event, train_idx, n_train, S)
    _same_problems(z, P)
    _boot_group(group, P, "problem")
    R = _boot_replicates(replicates)
    counts = torch.empty(P, R + 1, 2, device=z.device, dtype=torch.int64)
    with _timed("boot_surv_counts"):
        _call("mdl_boot_surv_counts", z, time, ldt, event, lde, train_idx, n_train, P, n_max, S, group, int(seed) & 0xFFFFFFFFFFFFFFFF, R,
              counts, _stream(), unsupported=_boot_refusal(n_max, 2, S, R))
    return counts


# ---- X1-X2: patch contributions of a linear probe's decision (include/madeleine_amd_explain.h).  Forward only, no autograd ----
CONTRIB_MAX_C = _native.EXPLAIN_DEFINES["MDL_CONTRIB_MAX_C"]
CONTRIB_ROWS = _native.EXPLAIN_DEFINES["MDL_CONTRIB_ROWS"]
CONTRIB_STATS = ("sum", "pos", "neg", "absmax")      # the second axis of contrib_stats' result
if any(_native.EXPLAIN_DEFINES["MDL_CONTRIB_" + s.upper()] != i for i, s in enumerate(CONTRIB_STATS)):
    raise ImportError("madeleine_amd: CONTRIB_STATS does not match the MDL_CONTRIB_* indices of %s" % _native._build.EXPLAIN_HEADER)
_CONTRIB_LIMITS = ("patch contributions support 1, 2, 4 or 8 heads of %d channels, 1..%d decision columns and T, R and the launch grids "
                   "within int32 (got T %d, R %d, H %d, C %d)")


def _unit_cols(t, name, fn):
    """(rows, cols, row stride) of a 2-D device tensor with unit column stride (any row stride)."""
    if t.dim() != 2 or not t.is_cuda or (t.shape[1] > 1 and t.stride(1) != 1):
        raise RuntimeError("madeleine_amd: %s needs %s [rows, cols] on a ROCm device with unit column stride" % (fn, name))
    return t.shape[0], t.shape[1], (t.stride(0) if t.shape[0] > 1 else t.shape[1])


def attn_contrib(E, attn, U, per_head=False):
    """contribution [T, C] (with per_head=True: (contribution, per_head [T, H, C])) of the head-major token embeddings E [T, H * 512]
    (fp32 or bf16, unit column stride, any row stride), the attention weights attn [T, H] fp32 (likewise) and the decision directions
    U [C, H * 512] fp32 (MADELEINE.slide_directions): per_head[t, h, c] = attn[t, h] <U[c, h], E[t, h]>, contribution = the heads added
    in ascending order (X1 of include/madeleine_amd_explain.h; row-local, fixed summation order).  One launch on the current stream, no
    host read."""
    if E.dtype not in ACT_DTYPES:
        raise RuntimeError("madeleine_amd: E must be float32 or bfloat16 (got %s)" % E.dtype)
    T, HW, ldE = _unit_cols(E, "E", "attn_contrib")
    Ta, H, ldA = _unit_cols(attn, "attn", "attn_contrib")
    _require(U, "U")
    if attn.dtype != torch.float32 or Ta != T or H < 1 or HW != H * HID or U.dim() != 2 or U.shape[0] < 1 or U.shape[1] != HW:
        raise RuntimeError("madeleine_amd: attn_contrib needs E [T, H * %d], attn [T, H] float32 and U [C, H * %d] (got %s, %s, %s)"
                           % (HID, HID, tuple(E.shape), tuple(attn.shape), tuple(U.shape)))
    C, dev = U.shape[0], E.device
    total = torch.empty(T, C, device=dev, dtype=torch.float32)
    heads = torch.empty(T, H, C, device=dev, dtype=torch.float32) if per_head else None
    with _timed("attn_contrib", ("byte", float(T) * (HW * E.element_size() + 4 * H + 4 * C * (1 + (H if per_head else 0))))):
        _call("mdl_attn_contrib", E, ldE, 1 if E.dtype == torch.bfloat16 else 0, attn, ldA, U, T, H, HID, C, heads, total, C, _stream(),
              unsupported=(_CONTRIB_LIMITS, HID, CONTRIB_MAX_C, T, 0, H, C))
    return (total, heads) if per_head else total


def contrib_stats(contrib, cu):
    """stats [R, 4, C] fp32 of contrib [T, C] (fp32, unit column stride, any row stride) over the bags of cu int64 [R + 1] on the device:
    per bag and column the sum, the sum of the positive terms, the sum of the negative terms and max |.| (CONTRIB_STATS; X2 of include/
    madeleine_amd_explain.h: chunks of CONTRIB_ROWS rows combined in ascending order, a bag's bits depend on the bag alone, an empty
    bag gives zeros).  Three launches on the current stream, no host read."""
    T, C, ld = _unit_cols(contrib, "contrib", "contrib_stats")
    if contrib.dtype != torch.float32 or C < 1:
        raise RuntimeError("madeleine_amd: contrib_stats needs contrib [T, C] float32, C >= 1")
    _require(cu, "cu_seqlens", torch.int64)
    if cu.dim() != 1 or cu.numel() < 1:
        raise RuntimeError("madeleine_amd: cu_seqlens must be [R + 1]")
    R, dev = cu.numel() - 1, contrib.device
    if R == 0 or T == 0:      # nothing is launched: the zeros of empty bags are written here
        return torch.zeros(R, 4, C, device=dev, dtype=torch.float32)
    refusal = (_CONTRIB_LIMITS, HID, CONTRIB_MAX_C, T, R, 0, C)
    stats = torch.empty(R, 4, C, device=dev, dtype=torch.float32)
    ws = _ws_for("mdl_contrib_stats_ws_bytes", dev, T, R, C, refusal=refusal)
    with _timed("contrib_stats", ("byte", 4.0 * T * C)):
        _call("mdl_contrib_stats", contrib, ld, cu, T, R, C, stats, ws, _stream(), unsupported=refusal)
    return stats


# ---- K1-K4: k-means over the rows of the slide store (include/madeleine_amd_cluster.h).  No autograd: features are inputs ----
KM_ROWS = _native.CLUSTER_DEFINES["MDL_KM_ROWS"]
KM_MAX_K = _native.CLUSTER_DEFINES["MDL_KM_MAX_K"]
_KM_LIMITS = "k-means supports 1..%d clusters and fewer than 2^31 rows per call (got k %d, T %d)"


def _km_source(store_rows, off, bag, cu, chunk_cu, fn):
    """The row source of K1-K3: store_rows [T_total, D] in a store dtype on the device, off int64 [n_bags + 1], bag int32 [R], cu and
    (unless None) chunk_cu int64 [R + 1], all on the device.  Returns the leading arguments of the entry points."""
    _require_store(store_rows)
    _require_draw_tables(off, bag, None, "bag")
    _require(cu, "cu", torch.int64)
    R = bag.numel()
    if cu.numel() != R + 1:
        raise RuntimeError("madeleine_amd: %s needs cu [R + 1] = [%d]" % (fn, R + 1))
    if chunk_cu is not None:
        _require(chunk_cu, "chunk_cu", torch.int64)
        if chunk_cu.numel() != R + 1:
            raise RuntimeError("madeleine_amd: %s needs chunk_cu [R + 1] = [%d]" % (fn, R + 1))
    D = store_rows.shape[1]
    return (store_rows, STORE_DTYPES[store_rows.dtype], store_rows.stride(0) if store_rows.shape[0] > 1 else D, store_rows.shape[0], off,
            off.numel() - 1, bag, cu)


def _km_centroids(C, D, name="centroids"):
    _require(C, name)
    if C.dim() != 2 or C.shape[1] != D or C.shape[0] < 1:
        raise RuntimeError("madeleine_amd: %s must be [k, D] = [k, %d] float32 (got %s)" % (name, D, tuple(C.shape)))
    return C.shape[0]


def _km_vector(t, name, dtype, n):
    _require(t, name, dtype)
    if t.dim() != 1 or t.numel() != n:
        raise RuntimeError("madeleine_amd: %s must be [%d] %s (got %s)" % (name, n, dtype, tuple(t.shape)))
    return t


def kmeans_assign(store_rows, off, bag, cu, chunk_cu, n_chunks, n_rows, centroids, labels=None, dist=None, stats=None, ws=None):
    """(labels [T] int32, dist [T] fp32, stats [2] int64) <- the nearest of centroids [k, D] for every row of the listed bags (K1 of
    include/madeleine_amd_cluster.h): the rows are read where they lie on the exact-fp32 MFMA, ties go to the lowest centroid, a row
    with a non-finite element gets label -1 and dist NaN.  labels is IN and OUT (None: a fresh vector of -2, so every finite row
    counts as changed); stats[0] is the number of rows whose label changed and stats[1] holds the bits of the fp64 inertia
    (stats.view(torch.float64)[1]).  n_chunks = chunk_cu[R] and n_rows = cu[R] = T as host integers; chunk_cu counts chunks of KM_ROWS
    rows.  ws: a workspace of at least mdl_kmeans_assign_ws_bytes (None: allocated here).  No host read."""
    src = _km_source(store_rows, off, bag, cu, chunk_cu, "kmeans_assign")
    T, D, dev = int(n_rows), store_rows.shape[1], store_rows.device
    k = _km_centroids(centroids, D)
    labels = torch.full((T,), -2, device=dev, dtype=torch.int32) if labels is None else _km_vector(labels, "labels", torch.int32, T)
    dist = torch.empty(T, device=dev, dtype=torch.float32) if dist is None else _km_vector(dist, "dist", torch.float32, T)
    stats = torch.empty(2, device=dev, dtype=torch.int64) if stats is None else _km_vector(stats, "stats", torch.int64, 2)
    refusal = (_KM_LIMITS, KM_MAX_K, k, T)
    if ws is None:
        ws = _ws_for("mdl_kmeans_assign_ws_bytes", dev, int(n_chunks), k, D, refusal=refusal)
    with _timed("kmeans_assign", ("flop", 2.0 * T * k * D)):
        _call("mdl_kmeans_assign", *src, chunk_cu, bag.numel(), int(n_chunks), T, D, centroids, k, labels, dist, stats, ws, _stream(),
              unsupported=refusal)
    return labels, dist, stats


def kmeans_update(store_rows, off, bag, cu, n_rows, labels, centroids, out=None, counts=None, ws=None):
    """(C_out [k, D] fp32, counts [k] int64) <- the mean of the rows of every label (K2): a stable counting sort of the call positions by
    label and S5's summation over each cluster's member list, combined in fp64.  A cluster with no member keeps its row of `centroids`.
    Five launches, no atomics on floats, no host read."""
    src = _km_source(store_rows, off, bag, cu, None, "kmeans_update")
    T, D, dev = int(n_rows), store_rows.shape[1], store_rows.device
    k = _km_centroids(centroids, D)
    _km_vector(labels, "labels", torch.int32, T)
    if out is None:
        out = torch.empty(k, D, device=dev, dtype=torch.float32)
    elif _km_centroids(out, D, "out") != k:
        raise RuntimeError("madeleine_amd: kmeans_update needs out [k, D] like centroids")
    counts = torch.empty(k, device=dev, dtype=torch.int64) if counts is None else _km_vector(counts, "counts", torch.int64, k)
    refusal = (_KM_LIMITS, KM_MAX_K, k, T)
    if ws is None:
        ws = _ws_for("mdl_kmeans_update_ws_bytes", dev, T, k, D, refusal=refusal)
    with _timed("kmeans_update", ("byte", float(T) * D * store_rows.element_size())):
        _call("mdl_kmeans_update", *src, bag.numel(), T, D, labels, centroids, k, out, counts, ws, _stream(), unsupported=refusal)
    return out, counts


def kmeans_seed(store_rows, off, bag, cu, chunk_cu, n_chunks, n_rows, u):
    """(positions [k] int64, centroids [k, D] fp32) <- k-means++ seeding from u [k] fp64 uniforms in [0, 1) on the device (K3): D^2
    sampling in-stream, two launches per centre, no host read."""
    src = _km_source(store_rows, off, bag, cu, chunk_cu, "kmeans_seed")
    T, D, dev = int(n_rows), store_rows.shape[1], store_rows.device
    _require(u, "u", torch.float64)
    if u.dim() != 1 or u.numel() < 1:
        raise RuntimeError("madeleine_amd: u must be [k] float64")
    k = u.numel()
    refusal = (_KM_LIMITS, KM_MAX_K, k, T)
    pos = torch.empty(k, device=dev, dtype=torch.int64)
    C = torch.empty(k, D, device=dev, dtype=torch.float32)
    ws = _ws_for("mdl_kmeans_seed_ws_bytes", dev, int(n_chunks), T, refusal=refusal)
    with _timed("kmeans_seed", ("byte", float(T) * D * store_rows.element_size() * k)):
        _call("mdl_kmeans_seed", *src, chunk_cu, bag.numel(), int(n_chunks), T, D, u, k, pos, C, ws, _stream(), unsupported=refusal)
    return pos, C


def kmeans_hist(labels, cu, k):
    """counts [R, k] int32 <- per bag of cu int64 [R + 1] (device), the number of its call positions with each label in [0, k); any other
    label -- the -1 of a non-finite row -- is counted nowhere (K4).  One launch, no host read."""
    _require(labels, "labels", torch.int32)
    _require(cu, "cu", torch.int64)
    if labels.dim() != 1 or labels.numel() < 1 or cu.dim() != 1 or cu.numel() < 1:
        raise RuntimeError("madeleine_amd: kmeans_hist needs labels [T], T >= 1, and cu [R + 1]")
    R, k = cu.numel() - 1, int(k)
    counts = torch.empty(R, max(k, 0), device=labels.device, dtype=torch.int32)
    with _timed("kmeans_hist", ("byte", 4.0 * labels.numel())):
        _call("mdl_kmeans_hist", labels, cu, R, labels.numel(), k, counts if counts.numel() else labels, _stream(),
              unsupported=(_KM_LIMITS, KM_MAX_K, k, labels.numel()))
    return counts
