"""The case table of tests/test_extents_gpu.py and the harness its cases run in.  Imports without a GPU: tests/test_extents_cpu.py
holds the table against the header (every export covered or exempt, every pointer parameter with a role that agrees with its const).

ROLES: entry point -> "param:role ..." for every POINTER parameter of its prototype, in prototype order.
  in     device memory the call only reads (the header says const)
  out    device memory the call writes
  inout  device memory the call reads and writes (accumulate forms, optimizer state)
  ws     the workspace, sized by the entry point's *_ws_bytes query
  host   a host address: the stream handle, *_host arrays, the arrays of per-problem device pointers of the GOT _multi forms
         (their pointees are arena buffers all the same)
A parameter that a case passes as NULL keeps the role it has when it is given."""
import re

import torch

from tests._arena import Arena, ArenaError

POINTER_ROLES = ("in", "out", "inout", "ws", "host", "null")

_GATE_FWD = "Wa:in ba:in Wb:in bb:in wc:in bc:in scores:out act_a:out act_b:out keep_a:in keep_b:in ws:ws stream:host"
_GATE_BWD = ("Wa:in Wb:in wc:in act_a:in act_b:in d_scores:in dE:inout dWa:out dWb:out dba:out dbb:out dwc:out dbc:out keep_a:in keep_b:in")
_POOL_TERM = " scores:in stat_m:in stat_l:in d_pooled:in row_bag:in"
_POOL_FWD = "scores:in pooled:out stat_m:out stat_l:out"
_POOL_BWD = "scores:in pooled:in stat_m:in stat_l:in d_pooled:in"
_LN_FWD = "gamma:in beta:in y:out mean:out rstd:out keep:in"
_LN_BWD = "gamma:in beta:in mean:in rstd:in dy:in dx:out dgamma:out dbeta:out"
_LN_BWD_SPLIT = ("x:in bias:in gamma:in beta:in mean:in rstd:in dy:in dy_absmax:in dx_img:out dx_scale:out dgamma:out dbeta:out dbias:out "
                 "keep:in row_mul:in rstd_max:in")
_GOT_FWD = "V:in Q:in out:out minmax_out:out minmax_in:in ws:ws stream:host"
_GOT_EXT = "V:in Q:in minmax_out:out ws:ws stream:host"
_GOT_BWD = "V:in Q:in d_out:in dV:out dQ:out ws:ws stream:host"
_GOT_BEGIN = "d_out:in d_minmax:out ws:ws stream:host"
_GOT_FINISH = "V:in Q:in dV:out dQ:out d_minmax_total:in ws:ws stream:host"
_FIT = "X:in y:in train_idx:in n_train:in W_out:out b_out:out info_out:out ws:ws stream:host"
_METRICS = "z:in y:in train_idx:in n_train:in confusion_out:out auc_out:out ws:ws stream:host"
_SAMPLE = "off:in bag:in key_id:in out:out idx_out:out stream:host"
_PACK = "off:in bag:in key_id:in cu:in chunk_cu:in out:out row_bag:out idx_out:out stream:host"
_MEAN = "off:in bag:in chunk_cu:in out:out ws:ws stream:host"

ROLES = {
    # gates
    "mdl_abmil_gate_fwd": "E:in " + _GATE_FWD,
    "mdl_abmil_gate_fwd_bf16": "E:in " + _GATE_FWD,
    "mdl_abmil_gate_fwd_split": "E_img:in e_scale:in " + _GATE_FWD,
    "mdl_abmil_gate_bwd": "E:in " + _GATE_BWD + " ws:ws stream:host",
    "mdl_abmil_gate_bwd_bf16": "E:in " + _GATE_BWD + " ws:ws stream:host",
    "mdl_abmil_attnpool_bwd": "E:in " + _GATE_BWD + _POOL_TERM + " ws:ws stream:host",
    "mdl_abmil_attnpool_bwd_bf16": "E:in " + _GATE_BWD + _POOL_TERM + " ws:ws stream:host",
    "mdl_abmil_attnpool_bwd_phases": "E:in " + _GATE_BWD + _POOL_TERM + " ws:ws stream:host",
    "mdl_abmil_attnpool_bwd_phases_bf16": "E:in " + _GATE_BWD + _POOL_TERM + " ws:ws stream:host",
    "mdl_abmil_attnpool_bwd_split": "E_img:in e_scale:in " + _GATE_BWD + _POOL_TERM + " dE_absmax:inout ws:ws stream:host",
    "mdl_abmil_gate_dropout_mask": "keep:out stream:host",
    # pools
    "mdl_abmil_pool_fwd": "E:in " + _POOL_FWD + " cu_seqlens:in ws:ws stream:host",
    "mdl_abmil_pool_fwd_bf16": "E:in " + _POOL_FWD + " cu_seqlens:in ws:ws stream:host",
    "mdl_abmil_pool_fwd_img": "E_img:in e_scale:in " + _POOL_FWD + " cu_seqlens:in ws:ws stream:host",
    "mdl_abmil_pool_bwd": "E:in " + _POOL_BWD + " dE:inout d_scores:inout cu_seqlens:in stream:host",
    "mdl_abmil_pool_bwd_bf16": "E:in " + _POOL_BWD + " dE:inout d_scores:inout cu_seqlens:in stream:host",
    "mdl_abmil_pool_dscores_img": "E_img:in e_scale:in " + _POOL_BWD + " d_scores:inout cu_seqlens:in stream:host",
    "mdl_abmil_wpool_fwd": "E:in weights:in pooled:out scratch_m:out scratch_l:out cu_seqlens:in ws:ws stream:host",
    "mdl_abmil_wpool_fwd_bf16": "E:in weights:in pooled:out scratch_m:out scratch_l:out cu_seqlens:in ws:ws stream:host",
    "mdl_abmil_wpool_bwd": "E:in weights:in d_pooled:in dE:inout d_weights:out cu_seqlens:in stream:host",
    "mdl_abmil_wpool_bwd_bf16": "E:in weights:in d_pooled:in dE:inout d_weights:out cu_seqlens:in stream:host",
    "mdl_abmil_pool_view_fwd": "E:in " + _POOL_FWD + " token_idx:in ws:ws stream:host",
    "mdl_abmil_pool_view_fwd_bf16": "E:in " + _POOL_FWD + " token_idx:in ws:ws stream:host",
    "mdl_abmil_pool_view_bwd": "E:in " + _POOL_BWD + " dE:inout d_scores:inout token_idx:in stream:host",
    "mdl_abmil_pool_view_bwd_bf16": "E:in " + _POOL_BWD + " dE:inout d_scores:inout token_idx:in stream:host",
    "mdl_abmil_pool_rview_fwd": "E:in " + _POOL_FWD + " perm:in vcu:in ws:ws stream:host",
    "mdl_abmil_pool_rview_fwd_bf16": "E:in " + _POOL_FWD + " perm:in vcu:in ws:ws stream:host",
    "mdl_abmil_pool_rview_bwd": "E:in " + _POOL_BWD + " dE:inout d_scores:inout perm:in vcu:in stream:host",
    "mdl_abmil_pool_rview_bwd_bf16": "E:in " + _POOL_BWD + " dE:inout d_scores:inout perm:in vcu:in stream:host",
    # LayerNorm-GELU-Dropout
    "mdl_ln_gelu_drop_fwd": "x:in bias:in " + _LN_FWD + " stream:host",
    "mdl_ln_gelu_drop_fwd_bf16": "x:in bias:in " + _LN_FWD + " stream:host",
    "mdl_ln_gelu_drop_fwd_groups": "x:in group_bias:in " + _LN_FWD + " cu_groups:in stream:host",
    "mdl_ln_gelu_drop_fwd_groups_bf16": "x:in group_bias:in " + _LN_FWD + " cu_groups:in stream:host",
    "mdl_ln_gelu_drop_fwd_split": "x:in bias:in gamma:in beta:in y:out img:out scale:out mean:out rstd:out keep:in row_mul:in rstd_max:out stream:host",
    "mdl_ln_gelu_drop_bwd": "x:in bias:in " + _LN_BWD + " dbias:out keep:in ws:ws stream:host",
    "mdl_ln_gelu_drop_bwd_bf16": "x:in bias:in " + _LN_BWD + " dbias:out keep:in ws:ws stream:host",
    "mdl_ln_gelu_drop_bwd_groups": "x:in group_bias:in " + _LN_BWD + " dgroup_bias:out keep:in cu_groups:in ws:ws stream:host",
    "mdl_ln_gelu_drop_bwd_groups_bf16": "x:in group_bias:in " + _LN_BWD + " dgroup_bias:out keep:in cu_groups:in ws:ws stream:host",
    "mdl_ln_gelu_drop_bwd_split": _LN_BWD_SPLIT + " ws:ws stream:host",
    "mdl_ln_gelu_drop_bwd_split_groups": _LN_BWD_SPLIT + " cu_groups:in dgroup_bias:out ws:ws stream:host",
    # Linears
    "mdl_linear_fwd": "X:in W:in bias:in Y:out ws:ws stream:host",
    "mdl_linear_fwd_bf16": "X:in W:in bias:in Y:out ws:ws stream:host",
    "mdl_linear_bwd": "X:in W:in dY:in dX:out dW:out dbias:out ws:ws stream:host",
    "mdl_linear_bwd_bf16": "X:in W:in dY:in dX:out dW:out dbias:out ws:ws stream:host",
    # split engine
    "mdl_split_image": "X:in img:out scale:out stream:host",
    "mdl_split_image_rows": "X:in img:out row_inv:out scale:out stream:host",
    "mdl_split_tile_absmax": "X:in gate:out chunk_max:out stream:host",
    "mdl_split_gemm_nt": "A:in a_scale:in B:in b_scale:in C:inout bias:in absmax_out:inout row_gate:in a_row_mul:in b_col_mul:in stream:host",
    "mdl_split_gemm_nt_group_bias": "A:in a_scale:in B:in b_scale:in C:out bias:in a_row_mul:in b_col_mul:in group_bias:in row_group:in stream:host",
    "mdl_split_gemm_tn": "A:in a_scale:in B:in b_scale:in out:out b_chunk_max:in ws:ws stream:host",
    # InfoNCE
    "mdl_infonce_fwd": "Q:in P:in cnt:in loss:out row_loss:out ws:ws stream:host",
    "mdl_infonce_bwd": "Q:in P:in d_loss:in d_row_loss:in cnt:in dQ:out dP:out ws:ws stream:host",
    "mdl_infonce_neg_fwd": "Q:in P:in Neg:in loss:out row_loss:out ws:ws stream:host",
    "mdl_infonce_neg_bwd": "Neg:in d_loss:in d_row_loss:in dQ:out dP:out dNeg:out ws:ws stream:host",
    # GOT
    "mdl_got_fwd": _GOT_FWD, "mdl_got_tiled_fwd": _GOT_FWD, "mdl_got_tiled_rect_fwd": _GOT_FWD,
    "mdl_got_extrema": _GOT_EXT, "mdl_got_tiled_extrema": _GOT_EXT, "mdl_got_tiled_rect_extrema": _GOT_EXT,
    "mdl_got_bwd": _GOT_BWD, "mdl_got_tiled_bwd": _GOT_BWD, "mdl_got_tiled_rect_bwd": _GOT_BWD,
    "mdl_got_bwd_begin": _GOT_BEGIN, "mdl_got_tiled_bwd_begin": _GOT_BEGIN, "mdl_got_tiled_rect_bwd_begin": _GOT_BEGIN,
    "mdl_got_bwd_finish": _GOT_FINISH, "mdl_got_tiled_bwd_finish": _GOT_FINISH, "mdl_got_tiled_rect_bwd_finish": _GOT_FINISH,
    "mdl_got_extrema_multi": "V:host Q:host minmax_out:host k:host n:host ws:host stream:host",
    "mdl_got_fwd_multi": "V:host Q:host out:host minmax_in:host k:host n:host ws:host stream:host",
    "mdl_got_bwd_begin_multi": "d_out:host d_minmax:host k:host n:host ws:host stream:host",
    "mdl_got_bwd_finish_multi": "V:host Q:host dV:host dQ:host d_minmax_total:host k:host n:host ws:host stream:host",
    # AdamW (the *_host arrays hold the device addresses; the statistics workspace is read-only in update and commit)
    "mdl_adamw_grad_stats": "g_host:host numel_host:host ws:ws stream:host",
    "mdl_adamw_update": "p_host:host g_host:host exp_avg_host:host exp_avg_sq_host:host step_host:host numel_host:host ws:in stream:host",
    "mdl_adamw_commit": "step_host:host ws:in grad_norm:out skipped:inout stream:host",
    # slide store
    "mdl_bag_sample": "store:in " + _SAMPLE,
    "mdl_bag_sample_tiered": "store:in store_host:host " + _SAMPLE,
    "mdl_bag_pack": "store:in " + _PACK,
    "mdl_bag_pack_tiered": "store:in store_host:host " + _PACK,
    "mdl_bag_mean": "store:in " + _MEAN,
    "mdl_bag_mean_tiered": "store:in store_host:host " + _MEAN,
    # evaluation
    "mdl_probe_fit": _FIT, "mdl_logit_fit": _FIT,
    "mdl_probe_scores": "X:in W:in b:in z_out:out stream:host",
    "mdl_probe_metrics": _METRICS, "mdl_logit_metrics": _METRICS,
    "mdl_cox_fit": "X:in time:in event:in train_idx:in n_train:in W_out:out thr_out:out info_out:out ws:ws stream:host",
    "mdl_surv_metrics": "z:in time:in event:in train_idx:in n_train:in thr:in c_index_out:out chi2_out:out counts_out:out ws:ws stream:host",
    "mdl_attn_softmax": "scores:in cu:in attn:out m:out l:out ws:ws stream:host",
    "mdl_attn_rank": "scores:in cu:in order:out pct:out topk_idx:out topk_val:out ws:ws stream:host",
    "mdl_smooth_rank": "E:in sigma:out out:out ws:ws stream:host",
    "mdl_smooth_rank_marked": "E:in sigma:out out:out ws:ws marks_host:host stream:host",
    "mdl_retrieval": "Q:in K:in greater:out equal:out pair_sim:out topk_idx:out topk_val:out ws:ws stream:host",
}

# Entry points that launch nothing on caller buffers: host-only queries and measurement helpers.  One sentence each.
EXEMPT = {
    "mdl_version": "Returns a static string; host only.",
    "mdl_abi_version": "Returns a constant; host only.",
    "mdl_linear_bf16_supported": "A host-only predicate on sizes.",
    "mdl_dispatch_plan": "Host only: writes a host array and launches nothing.",
    "mdl_switch_get": "Host only: writes one host integer.",
    "mdl_switch_set": "Host only: stores a process-wide value, takes no buffer.",
    "mdl_switch_set_thread": "Host only: stores the calling thread's override, takes no buffer.",
    "mdl_switch_clear_thread": "Host only: clears the calling thread's override, takes no buffer.",
    "mdl_switch_name": "Returns a static string; host only.",
    "mdl_pool_timer_arm": "Measurement only: arms a process-wide timer slot, takes no buffer.",
    "mdl_pool_timer_read": "Measurement only: blocks on events and writes three floats to a host array.",
    "mdl_stream_create_cu_mask": "Creates a stream from a host mask; no device buffer.",
    "mdl_stream_destroy": "Releases a stream; no device buffer.",
}

# Covered entry points that have no arena case in tests/test_extents_gpu.py yet: name -> what is missing.  Kept empty when the
# coverage is complete; tests/test_extents_cpu.py holds every name here to an entry of ROLES (its roles are declared already).
PENDING = {}


def is_ws_query(name):
    return name.endswith("_ws_bytes")


def exempt_reason(name):
    if is_ws_query(name):
        return "A host-only size query; its answer is what the arena cases allocate."
    return EXEMPT.get(name)


_DECL = re.compile(r"(?P<ret>[\w\s*]+?)\b(?P<name>\w+)\s*\((?P<args>[^()]*)\)")


def prototypes(header_text):
    """name -> [(parameter name, is pointer, pointee is const)] in prototype order, from the text of the C header."""
    text = re.sub(r"/\*.*?\*/", " ", header_text, flags=re.S)
    text = re.sub(r"#ifdef __cplusplus.*?#endif", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    out = {}
    for stmt in text.split(";"):
        stmt = " ".join(stmt.split())
        if not stmt:
            continue
        m = _DECL.fullmatch(stmt)
        assert m is not None, stmt[:80]
        args = m.group("args").strip()
        params = []
        for a in ([] if args == "void" else args.split(",")):
            a = a.strip()
            words = a.replace("*", " * ").split()
            params.append((words[-1], "*" in words, words[0] == "const"))
        assert m.group("name") not in out
        out[m.group("name")] = params
    return out


def roles_of(name):
    """[(parameter, role)] of a covered entry point, as the table states them."""
    return [tuple(w.split(":")) for w in ROLES[name].split()]


def header_text():
    from madeleine_amd import _build
    with open(_build.HEADER) as f:
        return f.read()


# ===================================================================================================================== the harness
F32, BF = torch.float32, torch.bfloat16


class Run:
    """One pass of a case over one arena.  A case is a function case(r) that declares its buffers with r.inp / r.out / r.inout / r.ws,
    issues its calls with r.call and returns {name: output tensor}.  It runs twice per fill: a planning pass, in which every buffer is
    a meta tensor (shapes and strides only), nothing is launched and the arena is sized; then, after one allocation, the real pass.
    r.call holds every tensor argument to the table: it must lie in the arena, and its arena role must agree with the role ROLES
    gives the parameter it is passed for."""

    def __init__(self, device, fill, protos):
        self.arena, self.device, self.protos = Arena(device, fill), device, protos
        self.planning, self.specs, self.called, self.partial, self.frozen, self.given = True, [], [], {}, set(), set()

    # ---------------------------------------------------------------------------------------------------------------- buffers
    def _buf(self, name, shape, dtype, role, init=None, pitch=None, zero_tail=0, nbytes=None, partial=None):
        shape = tuple(int(s) for s in shape)
        if self.planning:
            self.arena.reserve(name, shape, dtype, role, nbytes=nbytes, pitch=pitch, zero_tail=zero_tail)
            self.specs.append((name, shape, dtype, role, init))
            if partial:
                self.partial[name] = partial
            return torch.empty(shape, dtype=dtype, device="meta")
        b = self.arena.bufs[name]
        assert (b.shape, b.dtype, b.role) == (shape, dtype, role), "the two passes of a case disagree on %s" % name
        if name in self.given:
            raise ArenaError("arena: %s declared twice" % name)
        self.given.add(name)
        if init is not None:
            b.view.copy_(init.to(dtype).reshape(shape))
            if role == "in":
                self.arena.freeze(name)          # (the copy is stream-ordered before the snapshot's read)
        else:
            assert role in ("out", "ws"), "%s is an operand without contents" % name
        return b.view

    def data(self, make):
        """make() in the real pass, None in the planning pass: inputs and references are only built where they are used."""
        return None if self.planning else make()

    def stream(self):
        return 0 if self.planning else torch.cuda.current_stream().cuda_stream

    def inp(self, name, shape, dtype, x):
        """An operand of exactly `shape`: x (a CPU tensor; None in the planning pass) converted to dtype."""
        assert self.planning or x is not None, name
        return self._buf(name, shape, dtype, "in", init=x)

    def out(self, name, shape, dtype=F32, partial=None, zero_tail=0, pitch=None):
        """An output, holding the fill.  partial: a sentence saying which part the header leaves unwritten (compared only where
        written); None: the header says every element is written."""
        return self._buf(name, shape, dtype, "out", partial=partial, zero_tail=zero_tail, pitch=pitch)

    def inout(self, name, shape, dtype, x):
        assert self.planning or x is not None, name
        return self._buf(name, shape, dtype, "inout", init=x)

    def ws(self, name, query, *sizes, pitch=None, minimum=16):
        """A workspace of exactly the bytes its query returns (the header's minimum of 16 where the query says less)."""
        from madeleine_amd import _native
        n = int(getattr(_native.lib(), query)(*sizes))
        assert n >= 0, (query, sizes, n)
        n = max(n, minimum)
        return self._buf(name, (n,), torch.uint8, "ws", pitch=pitch, nbytes=n)

    def begin(self):
        """Between the passes: the one allocation, every buffer taken, the operands filled, the arena sealed."""
        self.arena.allocate()
        for name, shape, dtype, role, _ in self.specs:
            self.arena.take(name, shape, dtype, role)
        self.arena.seal()
        self.planning = False

    def freeze(self, *names):
        """The named outputs of the calls so far are operands from here on: later calls may only read them."""
        if self.planning:
            return
        torch.cuda.synchronize()
        for n in names:
            self.arena.freeze(n)
            self.frozen.add(n)

    # ------------------------------------------------------------------------------------------------------------------ calls
    def _owner(self, ptr):
        base = self.arena.mem.data_ptr()
        off = ptr - base
        for b in self.arena.bufs.values():
            if b.start <= off < b.start + max(b.nbytes, 1):
                return b
        return None

    def call(self, entry, *args):
        """MF._call(entry, *args) with every tensor argument checked against the table."""
        from madeleine_amd import functional as MF
        self.called.append(entry)
        proto = self.protos[entry]
        assert len(args) == len(proto), "%s takes %d arguments, %d given" % (entry, len(proto), len(args))
        if self.planning:
            return
        roles = dict(roles_of(entry))
        for (pname, is_ptr, _), a in zip(proto, args):
            if not isinstance(a, torch.Tensor):
                continue
            assert is_ptr, "%s: a tensor for the scalar %s" % (entry, pname)
            if roles[pname] == "host":
                assert not a.is_cuda and a.is_pinned(), "%s: %s is a host address" % (entry, pname)
                continue
            b = self._owner(a.data_ptr()) if a.is_cuda else None
            assert b is not None, "%s: %s is not an arena buffer" % (entry, pname)
            have = "in" if b.name in self.frozen else b.role
            want = roles[pname]
            ok = {"in": ("in", "ws"), "out": ("out", "inout"), "inout": ("inout", "out"), "ws": ("ws",)}[want]
            assert have in ok, "%s: %s is declared %s, the buffer %s is %s" % (entry, pname, want, b.name, have)
        MF._call(entry, *args)

    def ptrs(self, tensors, rows=False):
        """The host array of device addresses that a *_host / _multi parameter takes: every pointee must lie in the arena.  rows:
        one address per row of a 2-d tensor.  None in the planning pass."""
        import ctypes
        if self.planning:
            return None
        if rows:
            tensors = [tensors[i] for i in range(tensors.shape[0])]
        for t in tensors:
            assert self._owner(t.data_ptr()) is not None, "a pointee outside the arena"
        return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])

    def outputs(self):
        """{name: bytes} of every out / inout buffer."""
        return {n: self.arena.mem[b.start:b.start + b.nbytes].clone() for n, b in self.arena.bufs.items() if b.role in ("out", "inout")}


CALLED = set()      # every entry point an arena case issued in this process (tests/test_extents_gpu.py's last test reads it)


def run_case(device, case, check=None, nan_ok=(), atomics=None):
    """Runs case(r) under both fills and asserts (a) the arena's check, (b) every out / inout buffer bit-identical between the fills
    (a buffer declared partial: wherever either run wrote it) and free of NaN under 0xFF, (c) check(outputs on the CPU) for each run.
    atomics: a sentence naming the floating-point atomics that make (b) impossible for this case; both runs are then held to (c)."""
    from tests._arena import FILLS
    protos = prototypes(header_text())
    raw, got = {}, {}
    for fill in FILLS:
        r = Run(device, fill, protos)
        case(r)
        r.begin()
        res = case(r)
        torch.cuda.synchronize()
        r.arena.check()                                                                                      # (a)
        CALLED.update(r.called)
        raw[fill] = (r.outputs(), r.partial, r.arena.fill)
        got[fill] = {k: v.detach().clone().cpu() for k, v in res.items()}
        del r
    (o1, partial, f1), (o2, _, f2) = raw[FILLS[0]], raw[FILLS[1]]
    if atomics is None:
        for name in sorted(o1):                                                                              # (b)
            a, b = o1[name], o2[name]
            if name in partial:
                unwritten = (a == f1) & (b == f2)
                same = (a == b) | unwritten
            else:
                same = a == b
            if not bool(same.all()):
                first = int(torch.nonzero(~same)[0])
                raise AssertionError("%s depends on the bytes outside the stated extents: first differing byte %d, %d bytes differ "
                                     "between the fills" % (name, first, int((~same).sum())))
    for k, v in got[FILLS[0]].items():
        if v.is_floating_point() and k not in nan_ok:
            assert not bool(torch.isnan(v).any()), "%s holds NaN under the 0xFF fill" % k
    if check is not None:                                                                                    # (c)
        for fill in FILLS:
            check(got[fill])
    return got[FILLS[0]]
