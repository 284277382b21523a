"""The autograd nodes themselves -- the twelve torch.autograd.Function classes of madeleine_amd.functional, model._PermuteFn and
distributed._GOTMulti -- used the ways a training script uses them and the kernel parity tests do not: with some inputs frozen, with
some outputs unused, with a second backward over one graph, with two graphs in flight, with gradients accumulated over micro-batches,
with upstream gradients that are expanded, transposed or bf16, and with a saved tensor modified between forward and backward.

Every node configuration is one entry of NODES: the smallest graph that contains the node, at the smallest shape its engine is taken
at, and a plain fp64 CPU reference of the same operation (tests/_autograd_ref.py, oracle.restatement), whose gradients torch's own
autograd supplies for any loss and any subset of leaves.  The bound of every comparison against fp64 is the one the node's existing
all-leaves parity test asserts; the test is named beside the bound (`cite`).  Nothing here is looser than the test it cites."""
import contextlib

import numpy as np
import pytest
import torch

from tests import _autograd_ref as A
from tests._util import golden, rel_err, t
from tests.test_dispatch_edges_gpu import _gate_inputs, _linear_case, _u
from tests.test_split_gpu import _decode

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
EPS_BF16 = 2.0 ** -8
HID = 512


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------------------------ bounds
def rel(tol):
    """rel_err(got, ref) < tol."""
    return ("rel", tol)


def absmax(a, b):
    """max |got - ref| <= a * max |ref| + b."""
    return ("absmax", a, b)


def total(tol):
    """|sum got - sum ref| < tol * |sum ref| (a loss that is the sum of the node's terms)."""
    return ("total", tol)


def _holds(spec, got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    if spec[0] == "rel":
        return rel_err(got, ref) < spec[1], rel_err(got, ref)
    if spec[0] == "absmax":
        err = float((got - ref).abs().max()) if ref.numel() else 0.0
        return err <= spec[1] * float(ref.abs().max() if ref.numel() else 0.0) + spec[2], err
    err = abs(float(got.sum()) - float(ref.sum()))
    return err < spec[1] * abs(float(ref.sum())), err


# ------------------------------------------------------------------------------------------------------------------------ nodes
class Img:
    """An output that is a split image: `t` is the tensor the gradient arrives on, `value()` what it encodes."""

    def __init__(self, tensor, scale, rows, K):
        self.t, self.scale, self.rows, self.K = tensor, scale, rows, K

    def value(self):
        from madeleine_amd import functional as MF
        return _decode(MF.SplitImage(self.t.detach(), self.scale, self.rows, self.K), self.rows, self.K)


def _tensor(o):
    return o.t if isinstance(o, Img) else o


def _value(o):
    return (o.value() if isinstance(o, Img) else o.detach()).double().cpu()


class Node:
    """One configuration of one autograd node.
    fns: names of the Function classes the graph of `run` contains (the CPU test holds their union to the classes that exist).
    make(seed) -> (leaves {name: fp32 CPU tensor}, extras {name: anything that is not differentiated}).
    run(leaves on the device, extras on the device) -> tuple of outputs; ref(fp64 leaves, extras) -> the same tuple in fp64.
    fwd: one bound per output; grad: {leaf: bound} with "*" the default; cite: the existing tests the bounds are taken from.
    params: leaves shared between micro-batches; dtypes: storage type of a leaf on the device (default fp32).
    saved: leaves / extras whose in-place change before backward must raise; zero_ok: leaves whose gradient may be exactly zero in
    exact arithmetic (shift invariance), held to `1e-6 * largest gradient norm` then
    (tests/test_split_gpu.py::test_embedder_image_only_matches_fp32_tokens).
    mode: (gemm mode or None, gate recompute) set around the whole case and restored; partial: {label: (used, ...)} ways of using only
    part of the outputs (see USED); groups: leaf groups for the frozen-subset case instead of every leaf alone / all but one."""

    def __init__(self, name, fns, make, run, ref, fwd, grad, cite, params=(), dtypes=None, saved=(), zero_ok=(), mode=(None, False),
                 partial=None, groups=None, bf16_upstream=False, ref_key=None):
        self.name, self.fns, self.make, self.run, self.ref = name, fns, make, run, ref
        self.ref_key = ref_key or name      # (configurations of one operation on the same inputs share the fp64 reference)
        self.fwd, self.grad, self.cite = fwd, grad, cite
        self.params, self.dtypes, self.saved, self.zero_ok = params, dtypes or {}, saved, zero_ok
        self.mode, self.partial, self.groups, self.bf16_upstream = mode, partial or {}, groups, bf16_upstream

    def __repr__(self):
        return self.name

    @contextlib.contextmanager
    def engine(self):
        from madeleine_amd import functional as MF
        old_mode, old_rc = MF.gemm_mode(), MF.GATE_RECOMPUTE
        try:
            if self.mode[0] is not None:
                MF.set_gemm_mode(self.mode[0])
            MF.set_gate_recompute(self.mode[1])
            yield
        finally:
            MF.set_gemm_mode(old_mode)
            MF.set_gate_recompute(old_rc)

    def bound(self, leaf):
        return self.grad.get(leaf, self.grad.get("*"))

    def upstream(self, shapes, used, gseed, layout="plain"):
        """_upstream for this node.  A node with bf16 outputs takes bf16-representable gradients: the engine casts an upstream gradient
        to the output's dtype before the node sees it."""
        return _upstream(shapes, used, gseed, "bf16" if self.bf16_upstream and layout != "sum" else layout)


# ways of using an output: None = unused, "all", or a mask over its elements
USED = {
    "all": None,
    "main": lambda shp: _mask(shp, lambda m: m[:, 0].fill_(1)),       # the whole-bag row of pooled [n_bags, 1 + V, C]
    "views": lambda shp: _mask(shp, lambda m: m[:, 1:].fill_(1)),     # the view rows alone
    "e0": lambda shp: _mask(shp, lambda m: m[0].fill_(1)),            # out[0] of GOT's out [2]
    "e1": lambda shp: _mask(shp, lambda m: m[1].fill_(1)),
    "s0": lambda shp: _mask(shp, lambda m: m[0].fill_(1)),            # stain 0 of got_multi's [S, 2]
}


def _mask(shp, fill):
    m = torch.zeros(shp)
    fill(m)
    return m


def _upstream(shapes, used, gseed, layout="plain"):
    """The fp32 CPU upstream gradients of a loss sum_i (out_i * g_i).sum() over the used outputs."""
    gs = []
    for i, shp in enumerate(shapes):
        if used[i] is None:
            gs.append(None)
            continue
        g = torch.ones(shp) if layout == "sum" else _u(tuple(shp) or (1,), 7000 + 100 * gseed + i).reshape(shp)
        if USED[used[i]] is not None:
            g = g * USED[used[i]](shp)
        if layout == "bf16":
            g = g.to(BF).float()
        gs.append(g)
    return gs


def _to_dev(x, dev):
    if torch.is_tensor(x):
        return x.to(dev)
    if isinstance(x, (list, tuple)):
        return type(x)(_to_dev(v, dev) for v in x)
    return x


def _forward(node, dev, leaves, extras, req, no_grad=False):
    """-> (leaves on the device, extras on the device, outputs): `req` names the leaves that require grad."""
    dl = {}
    for n, v in leaves.items():
        d = v.clone().to(dev).to(node.dtypes.get(n, torch.float32))
        dl[n] = d.requires_grad_() if n in req else d
    de = {k: _to_dev(v, dev) for k, v in extras.items()}
    with torch.no_grad() if no_grad else contextlib.nullcontext():
        outs = node.run(dl, de)
    return dl, de, outs


def _dev_upstream(outs, gs, dev, layout="plain"):
    pairs = []
    for o, g in zip(outs, gs):
        if g is None:
            continue
        gd = g.to(dev)
        if layout == "transposed" and g.dim() >= 2:      # the same values in a non-contiguous tensor
            gd = g.transpose(-1, -2).contiguous().to(dev).transpose(-1, -2)
            assert not gd.is_contiguous() or min(g.shape[-2:]) == 1
        if layout == "bf16":
            gd = gd.to(BF)
        pairs.append((_tensor(o), gd))
    return pairs


def _backward(outs, gs, dev, layout="plain", retain=False):
    if layout == "sum":      # what a script writes: delivers a stride-0 expanded gradient
        sum(_tensor(o).sum() for o, g in zip(outs, gs) if g is not None).backward(retain_graph=retain)
        return
    pairs = _dev_upstream(outs, gs, dev, layout)
    torch.autograd.backward([p[0] for p in pairs], [p[1] for p in pairs], retain_graph=retain)


_REF = {}


def _ref_graph(node, seed, shared=None):
    """fp64 leaves and outputs of make(seed) with the graph kept, so that every loss over it costs one reverse sweep."""
    key = (node.ref_key, seed, shared is not None)      # (`shared` is always the parameter leaves of the seed-1 graph)
    if key not in _REF:
        leaves, extras = node.make(seed)
        l64 = {n: v.double().requires_grad_() for n, v in leaves.items()}
        if shared is not None:
            l64.update(shared)
        _REF[key] = (l64, node.ref(l64, extras))
    return _REF[key]


_REF_GRADS = {}


def _ref_grads(node, seed, used, gseed, layout="plain"):
    key = (node.ref_key, seed, used, gseed, "plain" if layout == "transposed" else layout, node.bf16_upstream)
    if key not in _REF_GRADS:
        l64, outs = _ref_graph(node, seed)
        gs = node.upstream([o.shape for o in outs], used, gseed, layout)
        loss = sum((o * g.double()).sum() for o, g in zip(outs, gs) if g is not None)
        grads = torch.autograd.grad(loss, list(l64.values()), retain_graph=True, allow_unused=True)
        _REF_GRADS[key] = {n: (torch.zeros_like(v) if g is None else g) for (n, v), g in zip(l64.items(), grads)}
    return _REF_GRADS[key]


def _check_forward(node, outs, seed, what=""):
    _, ref = _ref_graph(node, seed)
    for i, (o, r, spec) in enumerate(zip(outs, ref, node.fwd)):
        ok, err = _holds(spec, _value(o), r)
        print(f"{node.name} {what} output {i}: {err:.3e} {spec}")
        assert ok, (node.name, what, "output", i, err, spec, node.cite)


def _check_grads(node, got, ref, names, what=""):
    """got {leaf: tensor or None} against ref {leaf: fp64} for `names`, each within the node's bound."""
    top = max(float(r.norm()) for r in ref.values())
    for n in names:
        g, r = got[n], ref[n]
        if n in node.zero_ok and float(r.norm()) < 1e-9 * top:
            err = 0.0 if g is None else float((g.detach().double().cpu() - r).abs().max())
            print(f"{node.name} {what} d{n}: |err| {err:.3e} (zero in exact arithmetic)")
            assert err < 1e-6 * top, (node.name, what, n, err)
            continue
        if float(r.norm()) == 0.0:      # the leaf does not reach the loss: no gradient, or exact zeros
            assert g is None or float(g.abs().max()) == 0.0, (node.name, what, n, "expected no gradient")
            continue
        assert g is not None, (node.name, what, n, "a requested gradient is None")
        assert g.shape == r.shape, (node.name, what, n, g.shape, r.shape)
        ok, err = _holds(node.bound(n), g, r)
        print(f"{node.name} {what} d{n}: {err:.3e} {node.bound(n)}")
        assert ok, (node.name, what, n, err, node.bound(n), node.cite)


def _grads_of(dl):
    return {n: (None if v.grad is None else v.grad.detach().clone()) for n, v in dl.items()}


def _all_used(node, seed=1):
    _, outs = _ref_graph(node, seed)
    return ("all",) * len(outs)


# ------------------------------------------------------------------------------------------------------------------------ the table
GATE_CITE = "tests/test_hip_kernels.py::test_gate_eval, ::test_gate_dropout_explicit_masks (forward 1e-5, gradients 1e-4)"
GATE_NAMES = ("Wa", "ba", "Wb", "bb", "wc", "bc")


def _keep(shape, seed, p_keep):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) < p_keep).to(torch.uint8)


def _gate_node(T, H, mode):
    def make(seed):
        E, w, _ = _gate_inputs(T, H, 40 * seed + T, bf16=False)
        return dict(zip(("E",) + GATE_NAMES, (E,) + w)), {"ka": _keep((T, H, HID), seed, 0.75), "kb": _keep((T, H, HID), seed + 50, 0.75)}

    def run(l, e):
        from madeleine_amd import functional as MF
        return (MF.gate_scores(l["E"], *[l[n] for n in GATE_NAMES], p_drop=0.25, seed=0, keep_a=e["ka"], keep_b=e["kb"]),)

    def ref(l, e):
        return (A.gate_scores(l["E"], *[l[n] for n in GATE_NAMES], p=0.25, keep_a=e["ka"], keep_b=e["kb"]),)

    return Node(f"gate-T{T}-{mode}", ("GateScoresFn",), make, run, ref, [rel(1e-5)], {"*": rel(1e-4)}, GATE_CITE, params=GATE_NAMES,
                saved=("E", "Wa", "Wb", "wc", "ka", "kb"), mode=(mode, False))


LENS = (1, 129, 170)      # packed bags: one token, one past a 128-token tile, T = 300 in all


def _cu(lens):
    return torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64)


def _attnpool_node(name, mode, recompute, dense, tok_bias, views=False, rviews=False):
    """AttnPoolFn: gate + pooling (+ views) + token projection [128, H*512] in one node.  Bounds: the gate's (forward 1e-5, gradients
    1e-4: tests/test_hip_kernels.py::test_attn_pool_fused_with_score_grad); the token projection's output is a Linear's (1e-6:
    tests/test_hip_kernels.py::test_linear_bias_tall_and_small_paths, tests/test_split_gpu.py::test_split_linear_autograd_matches_fp32_mode)
    but its weight gradient shares dE's node, so the gradients all take the node's 1e-4."""
    H, P = 2, 128
    B, N = dense if dense else (len(LENS), 0)
    T = B * N if dense else sum(LENS)

    def make(seed):
        E, w, _ = _gate_inputs(T, H, 60 * seed + T + (7 if recompute else 0), bf16=False)
        leaves = dict(zip(("E",) + GATE_NAMES, (E.view(B, N, -1) if dense else E,) + w))
        leaves["Wtok"] = _u((P, H * HID), 61 * seed, 0.02)
        if tok_bias:
            leaves["btok"] = _u((P,), 62 * seed, 0.1)
        ex = {"ka": _keep((T, H, HID), seed + 3, 0.75), "kb": _keep((T, H, HID), seed + 53, 0.75)}
        g = torch.Generator().manual_seed(seed + 99)
        if views:      # two index lists of different lengths that share three tokens (no token twice within a list)
            order = torch.randperm(N, generator=g).to(torch.int32)
            ex["views"] = [order[:N // 2].contiguous(), order[N // 2 - 3:].contiguous()]
        if rviews:
            from madeleine_amd.model import ragged_view_plan
            np.random.seed(seed + 17)
            ex["rviews"] = ragged_view_plan(LENS)
        if not dense:
            ex["cu"] = _cu(LENS)
        return leaves, ex

    def run(l, e):
        from madeleine_amd import functional as MF
        return MF.attn_pool(l["E"], *[l[n] for n in GATE_NAMES], p_drop=0.25, seed=0, keep_a=e["ka"], keep_b=e["kb"], cu_seqlens=e.get("cu"),
                            max_len=None if dense else max(LENS), views=tuple(e.get("views", ())), tok_proj=(l["Wtok"], l.get("btok")),
                            rviews=e.get("rviews"))

    def ref(l, e):
        return A.attn_pool(l["E"], [l[n] for n in GATE_NAMES], p=0.25, keep_a=e["ka"], keep_b=e["kb"], cu=e.get("cu"),
                           tok=(l["Wtok"], l.get("btok")), views=[v.long() for v in e.get("views", ())],
                           rviews=e["rviews"][:2] if rviews else None)

    tokn = ("Wtok", "btok") if tok_bias else ("Wtok",)
    partial = {"pooled": ("all", None, None), "scores": (None, "all", None), "tok": (None, None, "all"), "pooled+scores": ("all", "all", None)}
    if views or rviews:
        partial.update({"view-rows": ("views", None, None), "main-row": ("main", None, None)})
    groups = [("E",), GATE_NAMES, tokn, ("bc",), ("E", "Wtok")]
    return Node(name, ("AttnPoolFn",), make, run, ref, [rel(1e-5), rel(1e-5), rel(1e-6)], {"*": rel(1e-4)},
                "tests/test_hip_kernels.py::test_attn_pool_fused_with_score_grad", params=GATE_NAMES + tokn,
                saved=("E", "Wa", "Wb", "wc", "Wtok", "ka", "kb") + (("cu",) if not dense else ()), zero_ok=("bc",), mode=(mode, recompute),
                partial=partial, groups=groups)


def _linear_node(name, fn, T, N, K, mode, bf16, tol):
    """tol = (y, dx, dW, db).  SplitLinearFn saves the image of x, not x: only W is under the version check there."""
    def make(seed):
        x, W, b, _ = _linear_case(T, N, K, 30 * seed + T, bf16)
        return {"x": x, "W": W, "b": b}, {}

    def run(l, e):
        from madeleine_amd import functional as MF
        return (MF.linear(l["x"], l["W"], l["b"]),)

    def ref(l, e):
        return (A.linear(l["x"], l["W"], l["b"]),)

    cite = ("tests/test_bf16_gpu.py::test_linear_bf16_vs_fp32_math (y, dx one bf16 rounding; dW, db 1e-5)" if bf16 else
            "tests/test_hip_kernels.py::test_linear_bias_tall_and_small_paths, tests/test_split_gpu.py::"
            "test_split_linear_autograd_matches_fp32_mode (1e-6 throughout)")
    return Node(name, (fn,), make, run, ref, [rel(tol[0])], {"x": rel(tol[1]), "W": rel(tol[2]), "b": rel(tol[3])}, cite, params=("W", "b"),
                dtypes={"x": BF} if bf16 else None, saved=("W",) if fn == "SplitLinearFn" else ("x", "W"), mode=(mode, False),
                bf16_upstream=bf16)


def _ln_node(name, rows, bf16, grouped):
    W = HID
    lens = (5, 1, 7)
    tol_o, tol_g = (6e-3, 1e-2) if bf16 else (1e-5, 1e-4)
    cite = ("tests/test_hip_kernels.py::test_ln_gelu_drop_groups_vs_torch (bf16: 6e-3 / 1e-2, fp32: 1e-5 / 1e-4)" if bf16 or grouped else
            "tests/test_hip_kernels.py::test_ln_gelu_drop_vs_torch (forward 1e-5, gradients 1e-4)")

    def make(seed):
        x = _u((rows, W), 20 * seed + rows, 3.0) + 0.5
        if bf16:
            x = x.to(BF).float()
        leaves = {"x": x, "gamma": 1 + 0.2 * _u((W,), seed + 1), "beta": 0.3 * _u((W,), seed + 2),
                  "bias": 0.7 * _u((len(lens), W) if grouped else (W,), seed + 3)}
        ex = {"keep": _keep((rows, W), seed + 4, 0.9)}
        if grouped:
            ex["cu"] = _cu(lens)
        return leaves, ex

    def run(l, e):
        from madeleine_amd import functional as MF
        if grouped:
            return (MF.ln_gelu_drop_groups(l["x"], l["gamma"], l["beta"], 1e-5, 0.1, 0, e["keep"], l["bias"], e["cu"]),)
        return (MF.ln_gelu_drop(l["x"], l["gamma"], l["beta"], 1e-5, 0.1, 0, e["keep"], l["bias"]),)

    def ref(l, e):
        return (A.ln_gelu_drop(l["x"], l["gamma"], l["beta"], l["bias"], 1e-5, 0.1, e["keep"], e.get("cu")),)

    return Node(name, ("LNGeluDropFn",), make, run, ref, [rel(tol_o)], {"*": rel(tol_g)}, cite, params=("gamma", "beta", "bias"),
                dtypes={"x": BF} if bf16 else None, saved=("x", "gamma", "beta", "bias", "keep") + (("cu",) if grouped else ()),
                bf16_upstream=bf16)


PRE_CITE = ("tests/test_split_gpu.py::test_preattn_block_vs_torch_fp64, ::test_preattn_blocks_chain_on_images (image and fp32 output 1e-5, "
            "gradients 2e-5)")


def _preattn_node(name, second, want_fp32, grouped=False, keep=False):
    """PreAttnBlockFn on the split engine at T = 300 (> 256), K = N = 512: the first block (x_scale None, row-scaled input image), or
    the second block behind a first one (input = the first block's image); the gradient arrives on the fp32 output (want_fp32) or on
    the image."""
    T, K, N, G = 300, 512, 512, 3
    lens = (1, 129, 170)

    def make(seed):
        leaves = {"x": _u((T, K), 10 * seed, 2.0), "W": 0.05 * _u((N, K), seed + 1), "lb": 0.3 * _u((N,), seed + 2),
                  "gamma": 1 + 0.2 * _u((N,), seed + 3), "beta": 0.3 * _u((N,), seed + 4)}
        if second:
            leaves.update({"W2": 0.05 * _u((N, N), seed + 5), "lb2": 0.3 * _u((N,), seed + 6), "gamma2": 1 + 0.1 * _u((N,), seed + 7),
                           "beta2": 0.1 * _u((N,), seed + 8)})
        ex = {}
        if grouped:
            leaves["gbias"] = 0.5 * _u((G, N), seed + 9)
            ex["cu"] = _cu(lens)
            ex["row_group"] = torch.repeat_interleave(torch.arange(G), torch.tensor(lens)).to(torch.int32)
        if keep:
            ex["keep"] = _keep((T, N), seed + 11, 0.9)
        return leaves, ex

    def run(l, e):
        from madeleine_amd import functional as MF
        p = 0.1 if keep else 0.0
        if not second:
            img, sc, out = MF.preattn_block(l["x"], None, l["W"], l["lb"], l["gamma"], l["beta"], 1e-5, p, 0, e.get("keep"), want_fp32,
                                            l.get("gbias"), e.get("row_group"), e.get("cu"))
        else:
            i1, s1, _ = MF.preattn_block(l["x"], None, l["W"], l["lb"], l["gamma"], l["beta"])
            img, sc, out = MF.preattn_block(i1, s1, l["W2"], l["lb2"], l["gamma2"], l["beta2"], 1e-5, p, 0, e.get("keep"), want_fp32)
        return (out,) if want_fp32 else (Img(img, sc, T, N),)

    def ref(l, e):
        if not second:
            return (A.preattn_block(l["x"], l["W"], l["lb"], l["gamma"], l["beta"], p=0.1, keep=e.get("keep"), gbias=l.get("gbias"),
                                    cu_groups=e.get("cu")),)
        h = A.preattn_block(l["x"], l["W"], l["lb"], l["gamma"], l["beta"])
        return (A.preattn_block(h, l["W2"], l["lb2"], l["gamma2"], l["beta2"], p=0.1, keep=e.get("keep")),)

    first = ("W", "lb", "gamma", "beta") + (("gbias",) if grouped else ())
    return Node(name, ("PreAttnBlockFn",), make, run, ref, [rel(1e-5)], {"*": rel(2e-5)}, PRE_CITE,
                params=first + (("W2", "lb2", "gamma2", "beta2") if second else ()),
                saved=("W2" if second else "W", "gamma2" if second else "gamma") + (("keep",) if keep else ()) + (("cu",) if grouped else ()),
                mode=("split", False))


POOL_CITE = ("tests/test_hip_kernels.py::test_pool_fwd_bwd_dense, ::test_pool_ragged_and_empty, ::test_weighted_pool_no_softmax (pooled "
             "and dE 1e-5; softmax d_scores max |err| <= 1e-4 max |ref| + 1e-6; weights' gradient 1e-5)")


def _pool_node(name, kind, packed):
    """SoftmaxPoolFn / WeightedPoolFn on dense bags [2, 130, H*512] (130: one past a 128-token tile) or the packed bags LENS."""
    H = 2
    B, N = (len(LENS), 0) if packed else (2, 130)
    T = sum(LENS) if packed else B * N

    def make(seed):
        E, s = _u((T, H * HID), 5 * seed + T), _u((T, H), 6 * seed + T, 4.0)
        if kind == "weighted":
            s = torch.nn.functional.leaky_relu(s / 2)
        if not packed:
            E, s = E.view(B, N, -1), s.view(B, N, H)
        return {"E": E, "s": s}, ({"cu": _cu(LENS)} if packed else {})

    def run(l, e):
        from madeleine_amd import functional as MF
        f = MF.softmax_pool if kind == "softmax" else MF.weighted_pool
        return (f(l["E"], l["s"], e.get("cu"), max(LENS) if packed else None),)

    def ref(l, e):
        return ((A.softmax_pool if kind == "softmax" else A.weighted_pool)(l["E"], l["s"], e.get("cu")),)

    return Node(name, ("SoftmaxPoolFn" if kind == "softmax" else "WeightedPoolFn",), make, run, ref, [rel(1e-5)],
                {"E": rel(1e-5), "s": absmax(1e-4, 1e-6) if kind == "softmax" else rel(1e-5)}, POOL_CITE,
                saved=("E", "s") + (("cu",) if packed else ()))


def _rview_node():
    """RaggedViewPoolFn on the packed bags LENS.  Bounds: tests/test_ragged_views_gpu.py::test_rview_pool_vs_fp64 (pooled 1e-5; dE
    elementwise within 1e-5 max |ref| + 3e-7; d_scores max |err| <= 1e-4 max |ref| + 1e-6)."""
    H = 2
    T = sum(LENS)

    def make(seed):
        from madeleine_amd.model import ragged_view_plan
        np.random.seed(seed + 23)
        perm, vcu, mx = ragged_view_plan(LENS)
        return {"E": _u((T, H * HID), 8 * seed), "s": _u((T, H), 9 * seed, 4.0)}, {"cu": _cu(LENS), "perm": perm, "vcu": vcu, "max_view": mx}

    def run(l, e):
        from madeleine_amd import functional as MF
        return (MF.ragged_view_pool(l["E"], l["s"], e["cu"], e["perm"], e["vcu"], e["max_view"]),)

    def ref(l, e):
        return (A.rview_pool(l["E"], l["s"], e["perm"], e["vcu"]),)

    return Node("rview-pool-packed", ("RaggedViewPoolFn",), make, run, ref, [rel(1e-5)], {"E": absmax(1e-5, 3e-7), "s": absmax(1e-4, 1e-6)},
                "tests/test_ragged_views_gpu.py::test_rview_pool_vs_fp64", saved=("E", "s", "perm", "vcu"))


def _infonce_node(sym, per_row):
    """InfoNCEFn: S = 2 padded problems of cnt = (7, 5) rows, D = 512.  Bounds: tests/test_hip_kernels.py::
    test_infonce_reduction_none_sum_and_odd_width (losses and rows 1e-5, gradients 1e-4; its temperature 0.07 and its positives
    p + 0.2 q)."""
    S, Kmax, D, T = 2, 7, 512, 0.07
    cnt = torch.tensor([7, 5], dtype=torch.int32)

    def make(seed):
        Q = _u((S, Kmax, D), 3 * seed)
        return {"Q": Q, "P": _u((S, Kmax, D), 3 * seed + 1) + 0.2 * Q}, {"cnt": cnt.clone()}

    def run(l, e):
        from madeleine_amd import functional as MF
        loss, rows = MF.InfoNCEFn.apply(l["Q"], l["P"], e["cnt"], T, sym, per_row)
        return (loss, rows) if per_row else (loss,)

    def ref(l, e):
        loss, rows = A.info_nce_batched(l["Q"], l["P"], e["cnt"], T, sym)
        return (loss, rows) if per_row else (loss,)

    partial = {"rows": (None, "all"), "scalar": ("all", None), "both": ("all", "all")} if per_row else {}
    return Node(f"infonce-{'sym' if sym else 'asym'}-{'rows' if per_row else 'loss'}", ("InfoNCEFn",), make, run, ref,
                [rel(1e-5)] * (2 if per_row else 1), {"*": rel(1e-4)},
                "tests/test_hip_kernels.py::test_infonce_reduction_none_sum_and_odd_width", saved=("Q", "P", "cnt"), partial=partial)


def _infonce_neg_node(paired, per_row):
    """InfoNCENegFn: N = 7 queries, M = 31 negatives, D = 128.  Bounds: tests/test_infonce_negatives_gpu.py::check_against_fp64 at
    T = 0.1 (loss 1e-3 relative; gradients within 1e-3 of the fp64 gradient's norm) with its input recipe (p + 0.5 q)."""
    N, M, D, T = 7, 31, 128, 0.1

    def make(seed):
        g = torch.Generator().manual_seed(900 + seed)
        q = torch.randn(N, D, generator=g)
        return {"Q": q, "P": torch.randn(N, D, generator=g) + 0.5 * q, "Neg": torch.randn(*((N, M, D) if paired else (M, D)), generator=g)}, {}

    def run(l, e):
        from madeleine_amd import functional as MF
        loss, rows = MF.InfoNCENegFn.apply(l["Q"], l["P"], l["Neg"], T, paired, per_row)
        return (loss, rows) if per_row else (loss,)

    def ref(l, e):
        loss, rows = A.info_nce_neg(l["Q"], l["P"], l["Neg"], T, paired)
        return (loss, rows) if per_row else (loss,)

    partial = {"rows": (None, "all"), "scalar": ("all", None), "both": ("all", "all")} if per_row else {}
    return Node(f"infonce-neg-{'paired' if paired else 'unpaired'}-{'rows' if per_row else 'loss'}", ("InfoNCENegFn",), make, run, ref,
                [rel(1e-3)] * (2 if per_row else 1), {"*": rel(1e-3)}, "tests/test_infonce_negatives_gpu.py::check_against_fp64",
                saved=("Q", "P", "Neg"), partial=partial)


def _got_inputs(k, n, m, d, seed, recipe):
    """recipe 'golden': the inputs of tests/test_hip_kernels.py::test_got_vs_golden_and_oracle (its trial of the k = 2 fixture, q + 0.7 v);
    'tiled': those of tests/test_got_tiled_gpu.py::_inputs.  seed 2 is the same instance with bags and tokens in reverse order (GOT is
    equivariant under both: the same conditioning, other data in every position)."""
    if recipe == "golden":
        trial = int(golden("got")["k2/trial"])
        v, q = t((k, max(n, m), d), f"got:v2:{trial}"), t((k, max(n, m), d), f"got:q2:{trial}")
    else:
        v, q = t((k, max(n, m), d), f"got_tiled:{k}x{n}x{d}:v"), t((k, max(n, m), d), f"got_tiled:{k}x{n}x{d}:q")
    q = q + 0.7 * v
    v, q = v[:, :n].contiguous(), q[:, :m].contiguous()
    if seed % 2 == 0:
        v, q = v.flip(0, 1).contiguous(), q.flip(0, 1).contiguous()
    return v, q


def _got_node(name, family, k, n, m, d, recipe, two_phase, fwd, grad, cite):
    def make(seed):
        v, q = _got_inputs(k, n, m, d, seed, recipe)
        return {"V": v, "Q": q}, {}

    def run(l, e):
        from madeleine_amd import functional as MF
        f = MF.got if family == "resident" else MF.got_tiled
        if family != "resident":
            assert MF.got_tiled_supported(k, n, d, m)
        return (f(l["V"], l["Q"], reduce_dminmax=(lambda dmm: dmm) if two_phase else None),)

    def ref(l, e):
        return (A.got(l["V"], l["Q"]),)

    return Node(name, ("GOTFn",), make, run, ref, [fwd], {"*": grad}, cite, saved=("V", "Q"),
                partial={"wd": ("e0",), "gwd": ("e1",), "both": ("all",)}, ref_key=f"got-{recipe}-{k}-{n}-{m}-{d}")


def _got_multi_node():
    """_GOTMulti through distributed.got_multi(local=True), one process: two stains of (2, 33, 128) and (2, 24, 128) in one node (the
    batched launches of HipGotImpl).  Bounds: the resident class's (tests/test_hip_kernels.py::test_got_large_n_vs_fp64_oracle: value
    and gradients 1e-3).  The second stain's token count is chosen by the conditioning of the instance alone: torch's own fp32
    evaluation of the oracle is within 4e-6 of its fp64 gradients at n = 24 and 33 (at n = 17 and 20 it is 1e-4 .. 3e-4 off: a cost
    close to the ReLU threshold), so the reference sits far inside the bound."""
    def make(seed):
        v0, q0 = _got_inputs(2, 33, 33, 128, seed, "golden")
        v1, q1 = _got_inputs(2, 24, 24, 128, seed + 1, "golden")
        return {"V0": v0, "Q0": q0, "V1": v1, "Q1": q1}, {}

    def run(l, e):
        from madeleine_amd import distributed as MD
        return (MD.got_multi([(l["V0"], l["Q0"]), (l["V1"], l["Q1"])], local=True),)

    def ref(l, e):
        return (torch.stack([A.got(l["V0"], l["Q0"]), A.got(l["V1"], l["Q1"])]),)

    return Node("got-multi-local", ("_GOTMulti",), make, run, ref, [rel(1e-3)], {"*": rel(1e-3)},
                "tests/test_hip_kernels.py::test_got_large_n_vs_fp64_oracle", saved=("V0", "Q1"), partial={"stain0": ("s0",), "both": ("all",)})


def _permute_node():
    """model._PermuteFn: an index_select by a bijection; copies, so every comparison is exact up to the fp32 storage of the leaf."""
    def make(seed):
        g = torch.Generator().manual_seed(seed)
        perm = torch.randperm(37, generator=g)
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(37)
        return {"w": _u((37, 5), seed)}, {"perm": perm, "inv": inv}

    def run(l, e):
        from madeleine_amd.model import _PermuteFn
        return (_PermuteFn.apply(l["w"], e["perm"], e["inv"], 0),)

    def ref(l, e):
        return (l["w"].index_select(0, e["perm"]),)

    return Node("permute", ("_PermuteFn",), make, run, ref, [rel(1e-7)], {"*": rel(1e-7)}, "exact: a gather of fp32 values", saved=("inv",))


# ---- the chain of the encoder: three pre-attention blocks -> AttnPoolFn on the image alone, split mode; the gradient bound of the
# ---- published-maximum hand-off (functional._ABSMAX) travels from AttnPoolFn to block 3, from block 3 to block 2, from 2 to 1
CHAIN_B, CHAIN_N, CHAIN_H = 2, 150, 2
CHAIN_BLOCKS = ("W1", "g1", "b1", "W2", "g2", "b2", "W3", "g3", "b3")


def _chain_make(seed):
    T = CHAIN_B * CHAIN_N
    _, w, _ = _gate_inputs(T, CHAIN_H, 70 * seed, bf16=False)
    leaves = {"x": _u((T, 512), 71 * seed), "W1": 0.05 * _u((512, 512), seed + 1), "g1": 1 + 0.1 * _u((512,), seed + 2),
              "b1": 0.1 * _u((512,), seed + 3), "W2": 0.05 * _u((512, 512), seed + 4), "g2": 1 + 0.1 * _u((512,), seed + 5),
              "b2": 0.1 * _u((512,), seed + 6), "W3": 0.05 * _u((CHAIN_H * 512, 512), seed + 7), "g3": 1 + 0.1 * _u((CHAIN_H * 512,), seed + 8),
              "b3": 0.1 * _u((CHAIN_H * 512,), seed + 9)}
    leaves.update(dict(zip(GATE_NAMES, w)))
    return leaves


def _chain_run(l, hook=None):
    from madeleine_amd import functional as MF
    i1, s1, _ = MF.preattn_block(l["x"], None, l["W1"], None, l["g1"], l["b1"])
    i2, s2, _ = MF.preattn_block(i1, s1, l["W2"], None, l["g2"], l["b2"])
    i3, s3, _ = MF.preattn_block(i2, s2, l["W3"], None, l["g3"], l["b3"])
    if hook is not None and i3.requires_grad:
        i3.register_hook(hook)
    pooled, scores = MF.attn_pool(i3.view(CHAIN_B, CHAIN_N, -1), *[l[n] for n in GATE_NAMES], e_img=(i3, s3), e_only_image=True)
    return pooled, scores


def _chain_ref(l, hook=None):
    h = A.preattn_block(l["x"], l["W1"], None, l["g1"], l["b1"])
    h = A.preattn_block(h, l["W2"], None, l["g2"], l["b2"])
    E = A.preattn_block(h, l["W3"], None, l["g3"], l["b3"])
    if hook is not None:
        E.register_hook(hook)
    pooled, scores, _ = A.attn_pool(E.view(CHAIN_B, CHAIN_N, -1), [l[n] for n in GATE_NAMES])
    return pooled, scores


def _chain_node():
    """The chain as a node of the table, so that every case runs with AttnPoolFn on the image alone (e_only_image) and with the maxima
    handed from node to node: a second backward hands them over a second time.  Bounds: the whole embedder's (tests/test_hip_kernels.py::
    test_batched_abmil_other_geometries_vs_oracle: raw scores 1e-5, the input's and every parameter's gradient 1e-4); pooled 1e-5
    (::test_attn_pool_fused_with_score_grad)."""
    return Node("chain-image-only", ("PreAttnBlockFn", "AttnPoolFn"), lambda seed: (_chain_make(seed), {}), lambda l, e: _chain_run(l),
                lambda l, e: _chain_ref(l), [rel(1e-5), rel(1e-5)], {"*": rel(1e-4)},
                "tests/test_hip_kernels.py::test_batched_abmil_other_geometries_vs_oracle", params=CHAIN_BLOCKS + GATE_NAMES,
                saved=("W1", "g2", "W3", "Wa"), zero_ok=("bc",), mode=("split", False),
                partial={"pooled": ("all", None), "scores": (None, "all")},
                groups=[("x",), CHAIN_BLOCKS, GATE_NAMES, ("W2", "g2", "b2"), ("x", "Wa")])


def _got_multi_single_node():
    """_GOTMulti with one stain: HipGotImpl.can_batch needs two problems, so this takes the per-problem calls on side streams
    (forward, backward_begin, backward_finish).  Instance and bounds of got-resident-n33."""
    def make(seed):
        v, q = _got_inputs(2, 33, 33, 128, seed, "golden")
        return {"V": v, "Q": q}, {}

    def run(l, e):
        from madeleine_amd import distributed as MD
        return (MD.got_multi([(l["V"], l["Q"])], local=True),)

    return Node("got-multi-one-stain", ("_GOTMulti",), make, run, lambda l, e: (A.got(l["V"], l["Q"]).unsqueeze(0),), [total(4e-6)],
                {"*": rel(1.3e-4)}, GOT_GOLDEN_CITE, saved=("V", "Q"))


GOT_GOLDEN_CITE = GOT_GOLDEN = "tests/test_hip_kernels.py::test_got_vs_golden_and_oracle (loss 4e-6, gradient tensors 1.3e-4)"
GOT_BIG = "tests/test_hip_kernels.py::test_got_large_n_vs_fp64_oracle (value and gradients 1e-3)"
GOT_TILED = "tests/test_got_tiled_gpu.py::test_got_tiled_vs_fp64, tests/test_got_rect_gpu.py::test_got_rect_vs_fp64 (value 2e-4, gradients 4e-5)"

NODES = [
    _gate_node(130, 2, "split"), _gate_node(300, 2, "fp32"),
    _attnpool_node("attnpool-dense-split-views", "split", False, (2, 150), tok_bias=True, views=True),
    _attnpool_node("attnpool-packed-fp32-rviews", "fp32", False, None, tok_bias=True, rviews=True),
    _attnpool_node("attnpool-T130-split-recompute", "split", True, (1, 130), tok_bias=False),
    _linear_node("split-linear-300", "SplitLinearFn", 300, 512, 512, "split", False, (1e-6,) * 4),
    _linear_node("linear-fp32-300", "LinearFn", 300, 512, 512, "fp32", False, (1e-6,) * 4),
    _linear_node("linear-fp32-40", "LinearFn", 40, 512, 512, "fp32", False, (1e-6,) * 4),
    _linear_node("linear-bf16-300", "LinearFn", 300, 512, 512, None, True, (EPS_BF16, EPS_BF16, 1e-5, 1e-5)),
    _ln_node("ln-fp32", 13, False, False), _ln_node("ln-bf16", 13, True, False), _ln_node("ln-fp32-groups", 13, False, True),
    _preattn_node("preattn-first-fp32out", False, True, keep=True), _preattn_node("preattn-first-image", False, False),
    _preattn_node("preattn-second-fp32out", True, True), _preattn_node("preattn-second-image", True, False, keep=True),
    _preattn_node("preattn-first-groups", False, True, grouped=True),
    _pool_node("softmax-pool-dense", "softmax", False), _pool_node("softmax-pool-packed", "softmax", True),
    _pool_node("weighted-pool-dense", "weighted", False), _pool_node("weighted-pool-packed", "weighted", True),
    _rview_node(),
    _infonce_node(False, False), _infonce_node(True, False), _infonce_node(False, True), _infonce_node(True, True),
    _infonce_neg_node(False, False), _infonce_neg_node(True, False), _infonce_neg_node(False, True), _infonce_neg_node(True, True),
    _got_node("got-resident-n33", "resident", 2, 33, 33, 128, "golden", False, total(4e-6), rel(1.3e-4), GOT_GOLDEN),
    _got_node("got-resident-n33-two-phase", "resident", 2, 33, 33, 128, "golden", True, total(4e-6), rel(1.3e-4), GOT_GOLDEN),
    _got_node("got-resident-n257", "resident", 2, 257, 257, 128, "golden", False, total(1e-3), rel(1e-3), GOT_BIG),
    _got_node("got-resident-n257-two-phase", "resident", 2, 257, 257, 128, "golden", True, total(1e-3), rel(1e-3), GOT_BIG),
    # the tiled classes accept every n, m >= 1 (got_tiled_supported); one token has no transport problem (all costs zero, all gradients
    # zero), so the smallest instance that can be wrong is n = 2, and n = 2 against m = 3 for the rectangular family
    _got_node("got-tiled-n2", "tiled", 2, 2, 2, 128, "tiled", False, total(2e-4), rel(4e-5), GOT_TILED),
    _got_node("got-tiled-n2-two-phase", "tiled", 2, 2, 2, 128, "tiled", True, total(2e-4), rel(4e-5), GOT_TILED),
    _got_node("got-rect-n2-m3", "rect", 2, 2, 3, 128, "tiled", False, total(2e-4), rel(4e-5), GOT_TILED),
    _got_node("got-rect-n2-m3-two-phase", "rect", 2, 2, 3, 128, "tiled", True, total(2e-4), rel(4e-5), GOT_TILED),
    _got_multi_node(), _got_multi_single_node(), _permute_node(), _chain_node(),
]
NODE_CLASSES = sorted({f for n in NODES for f in n.fns})
# autograd nodes that are deliberately not in the table, each with its reason (tests/test_autograd_contract_cpu.py accepts no others)
NOT_IN_TABLE = {
    "_AllGatherReplicatedLoss": "a collective without a kernel: it needs an initialised process group, which is process-wide state a "
                                "test of this file must not leave behind; tests/test_distributed_gpu.py drives it in worker processes",
}
node_param = pytest.mark.parametrize("node", NODES, ids=repr)


def _subsets(node):
    names = list(node.make(1)[0])
    if node.groups is not None:
        return [tuple(n for n in g if n in names) for g in node.groups]
    alone = [(n,) for n in names]
    but_one = [tuple(m for m in names if m != n) for n in names] if len(names) > 2 else []
    return alone + but_one


# ------------------------------------------------------------------------------------------------------------------------ 1 frozen subsets
@node_param
def test_frozen_subsets(dev, node):
    """Each differentiable input requiring grad alone (or the node's groups), all but one, none, and under no_grad: every requested
    gradient within the bound, no gradient on a frozen input, and forward values that do not depend on who asked."""
    leaves, extras = node.make(1)
    names, used = list(leaves), _all_used(node)
    ref = _ref_grads(node, 1, used, 1)
    with node.engine():
        dl, _, outs_all = _forward(node, dev, leaves, extras, set(names))
        _check_forward(node, outs_all, 1, "all leaves")
        gs = node.upstream([_tensor(o).shape for o in outs_all], used, 1)
        _backward(outs_all, gs, dev)
        _check_grads(node, _grads_of(dl), ref, names, "all leaves")
        for sub in _subsets(node):
            dl, _, outs = _forward(node, dev, leaves, extras, set(sub))
            for a, b in zip(outs, outs_all):
                assert torch.equal(_tensor(a), _tensor(b)), (node.name, sub, "forward differs from the all-leaves forward")
            _backward(outs, gs, dev)
            got = _grads_of(dl)
            _check_grads(node, got, ref, sub, "only " + "+".join(sub))
            for n in names:
                if n not in sub:
                    assert got[n] is None, (node.name, sub, n, "a frozen input received a gradient")
        for no_grad in (False, True):
            dl, _, outs = _forward(node, dev, leaves, extras, set(), no_grad=no_grad)
            for a, b in zip(outs, outs_all):
                assert not _tensor(a).requires_grad
                assert torch.equal(_tensor(a), _tensor(b)), (node.name, "forward without gradients differs", no_grad)


def test_preattn_first_block_input_gradient_under_an_outlier_row(dev):
    """The first block with only x requiring grad takes the second LayerNorm-backward pass (d(pre-LN) under the common scale).  One row
    of x is 1e3 times the others: a gradient left under the row-scaled image would lose that row's neighbours' low bits and miss the
    2e-5 of tests/test_split_gpu.py::test_preattn_block_vs_torch_fp64."""
    node = _preattn_node("preattn-first-outlier", False, True)
    base = node.make

    def make(seed):
        leaves, extras = base(seed)
        leaves["x"][17] *= 1e3
        return leaves, extras

    node.make = make
    leaves, extras = node.make(1)
    used = _all_used(node)
    ref = _ref_grads(node, 1, used, 1)
    with node.engine():
        dl, _, outs = _forward(node, dev, leaves, extras, {"x"})
        _check_forward(node, outs, 1, "outlier row")
        _backward(outs, node.upstream([_tensor(o).shape for o in outs], used, 1), dev)
    got = _grads_of(dl)
    _check_grads(node, got, ref, ["x"], "only x, outlier row")
    rows = [i for i in range(300) if i != 17]      # ... and row by row: the ordinary rows are not lost under the outlier
    assert rel_err(got["x"][rows], ref["x"][rows]) < 2e-5
    assert all(got[n] is None for n in leaves if n != "x")


# ------------------------------------------------------------------------------------------------------------------------ 2 unused outputs
@pytest.mark.parametrize("node", [n for n in NODES if n.partial], ids=repr)
def test_unused_outputs(dev, node):
    """A loss built from part of what the node returns: every gradient within the bound of the fp64 gradient of that loss."""
    leaves, extras = node.make(1)
    names = list(leaves)
    res = {}
    with node.engine():
        for label, used in node.partial.items():
            dl, _, outs = _forward(node, dev, leaves, extras, set(names))
            _backward(outs, node.upstream([_tensor(o).shape for o in outs], used, 1), dev)
            res[label] = _grads_of(dl)
            _check_grads(node, res[label], _ref_grads(node, 1, used, 1), names, "loss from " + label)
    if {"wd", "gwd", "both"} <= set(res):      # GOT: the two single-term gradients add up to the joint one
        ref = _ref_grads(node, 1, ("all",), 1)
        _check_grads(node, {n: res["wd"][n] + res["gwd"][n] for n in names}, ref, names, "wd + gwd")


# ------------------------------------------------------------------------------------------------------------------------ 3 second backward
@node_param
def test_second_backward_doubles_exactly(dev, node):
    """backward(retain_graph=True), then backward() on the same graph: every .grad is exactly twice the first (x + x is exact), so
    nothing a backward leaves in a saved workspace or rebuilds may differ the second time."""
    leaves, extras = node.make(1)
    names, used = list(leaves), _all_used(node)
    with node.engine():
        dl, _, outs = _forward(node, dev, leaves, extras, set(names))
        gs = node.upstream([_tensor(o).shape for o in outs], used, 1)
        _backward(outs, gs, dev, retain=True)
        g1 = _grads_of(dl)
        _backward(outs, gs, dev)
        g2 = _grads_of(dl)
    _check_grads(node, g1, _ref_grads(node, 1, used, 1), names, "first backward")
    for n in names:
        assert torch.equal(g2[n], 2 * g1[n]), (node.name, n, "second backward is not bit-identical to the first",
                                               float((g2[n].float() - 2 * g1[n].float()).abs().max()))


@node_param
def test_two_upstream_gradients_on_one_graph(dev, node):
    """torch.autograd.grad twice on one graph with two different upstream gradients: each result within the bound of its own fp64
    gradient (backward state left in a saved workspace by the first call would show in the second)."""
    leaves, extras = node.make(1)
    names, used = list(leaves), _all_used(node)
    with node.engine():
        dl, _, outs = _forward(node, dev, leaves, extras, set(names))
        for gseed in (1, 2):
            gs = node.upstream([_tensor(o).shape for o in outs], used, gseed)
            pairs = _dev_upstream(outs, gs, dev)
            got = torch.autograd.grad([p[0] for p in pairs], [dl[n] for n in names], [p[1] for p in pairs], retain_graph=gseed == 1,
                                      allow_unused=True)
            _check_grads(node, dict(zip(names, got)), _ref_grads(node, 1, used, gseed), names, f"upstream {gseed}")


# ------------------------------------------------------------------------------------------------------------------------ 4 interleaved
@node_param
def test_interleaved_graphs(dev, node):
    """forward A, forward B (other inputs, same shapes), backward B, backward A."""
    used = _all_used(node)
    with node.engine():
        runs = {}
        for seed in (1, 2):
            leaves, extras = node.make(seed)
            runs[seed] = _forward(node, dev, leaves, extras, set(leaves))
        for seed in (2, 1):
            dl, _, outs = runs[seed]
            _backward(outs, node.upstream([_tensor(o).shape for o in outs], used, seed), dev)
    for seed in (1, 2):
        dl, _, outs = runs[seed]
        _check_forward(node, outs, seed, f"graph {seed}")
        _check_grads(node, _grads_of(dl), _ref_grads(node, seed, used, seed), list(dl), f"graph {seed}")


def _chain_loss(outs, seed, device=None):
    """Both outputs under fixed weights (the scores enter, so that bc has a gradient)."""
    gs = _upstream([o.shape for o in outs], ("all", "all"), seed)
    return sum((o * (g.double() if device is None else g.to(device))).sum() for o, g in zip(outs, gs))


def _chain_check(got, ref, names, what):
    """The chain's bound: 1e-4 on the input's and every parameter's gradient, as the whole embedder (pre-attention blocks, gate,
    pooling) is held to in tests/test_hip_kernels.py::test_batched_abmil_other_geometries_vs_oracle and the fused gate + pooling node in
    ::test_attn_pool_fused_with_score_grad."""
    for n in names:
        tol = 1e-4
        err = rel_err(got[n], ref[n])
        print(f"chain {what} d{n}: {err:.3e} (< {tol})")
        assert err < tol, (what, n, err, tol)


def _chain_ref_grads(seed, hook=None):
    l64 = {n: v.double().requires_grad_() for n, v in _chain_make(seed).items()}
    _chain_loss(_chain_ref(l64, hook), seed).backward()
    return {n: v.grad for n, v in l64.items()}


@contextlib.contextmanager
def _split_mode():
    from madeleine_amd import functional as MF
    old = MF.gemm_mode()
    MF.set_gemm_mode("split")
    try:
        yield
    finally:
        MF.set_gemm_mode(old)


def test_chain_interleaved(dev):
    """Two encoder chains in flight: the second forward clears the table, the backwards run in the other order."""
    from madeleine_amd import functional as MF
    with _split_mode():
        runs = {}
        for seed in (1, 2):
            dl = {n: v.to(dev).requires_grad_() for n, v in _chain_make(seed).items()}
            runs[seed] = (dl, _chain_loss(_chain_run(dl), seed, dev))
        for seed in (2, 1):
            runs[seed][1].backward()
        assert len(MF._ABSMAX) == 0
    for seed in (1, 2):
        _chain_check(_grads_of(runs[seed][0]), _chain_ref_grads(seed), list(runs[seed][0]), f"graph {seed}")


@pytest.mark.parametrize("kind", ["new-tensor", "in-place"])
def test_chain_with_a_hook_on_the_token_gradient(dev, kind):
    """A hook doubles dE between AttnPoolFn and the last block: returning g * 2 is a table miss, g.mul_(2) leaves a stale version.  In
    both the consumer must take its own maximum: the result is the fp64 gradient under the same doubling."""
    from madeleine_amd import functional as MF
    hook = (lambda g: g * 2) if kind == "new-tensor" else (lambda g: g.mul_(2))
    with _split_mode():
        dl = {n: v.to(dev).requires_grad_() for n, v in _chain_make(3).items()}
        _chain_loss(_chain_run(dl, hook), 3, dev).backward()
        assert len(MF._ABSMAX) == 0
    _chain_check(_grads_of(dl), _chain_ref_grads(3, lambda g: g * 2), list(dl), kind)


def test_chain_with_frozen_pre_attn(dev):
    """All three blocks frozen (and x not differentiated): the gate's gradients are right, the frozen leaves have none, and nothing
    stays pinned in the table once backward has returned."""
    from madeleine_amd import functional as MF
    with _split_mode():
        dl = {n: v.to(dev) for n, v in _chain_make(4).items()}
        for n in GATE_NAMES:
            dl[n].requires_grad_()
        _chain_loss(_chain_run(dl), 4, dev).backward()
        assert len(MF._ABSMAX) == 0
    _chain_check(_grads_of(dl), _chain_ref_grads(4), GATE_NAMES, "frozen pre_attn")
    assert all(dl[n].grad is None for n in ("x",) + CHAIN_BLOCKS)


# ------------------------------------------------------------------------------------------------------------------------ 5 accumulation
@node_param
def test_accumulation_over_micro_batches(dev, node):
    """Two micro-batches backpropagated into the same parameter leaves without zeroing (a node without parameters: two losses into
    the same leaves): the fp64 gradient of the summed loss."""
    used = _all_used(node)
    la, ea = node.make(1)
    lb, eb = node.make(2)
    names = list(la)
    l64a, outs_a = _ref_graph(node, 1)
    if node.params:
        shared = {n: l64a[n] for n in node.params}
        l64b, outs_b = _ref_graph(node, 2, shared)
    else:
        l64b, outs_b = l64a, outs_a
    loss = sum((o * g.double()).sum() for o, g in zip(outs_a, node.upstream([o.shape for o in outs_a], used, 1)))
    loss = loss + sum((o * g.double()).sum() for o, g in zip(outs_b, node.upstream([o.shape for o in outs_b], used, 2)))
    ra = dict(zip(names, torch.autograd.grad(loss, [l64a[n] for n in names], retain_graph=True)))
    rb = dict(zip(names, torch.autograd.grad(loss, [l64b[n] for n in names], retain_graph=True)))
    with node.engine():
        dla, dea, outs = _forward(node, dev, la, ea, set(names))
        _backward(outs, node.upstream([_tensor(o).shape for o in outs], used, 1), dev, retain=not node.params)
        if node.params:
            dlb = {}
            for n, v in lb.items():
                dlb[n] = dla[n] if n in node.params else v.clone().to(dev).to(node.dtypes.get(n, torch.float32)).requires_grad_()
            outs = node.run(dlb, {k: _to_dev(v, dev) for k, v in eb.items()})
        else:
            dlb = dla
        _backward(outs, node.upstream([_tensor(o).shape for o in outs], used, 2), dev)
    _check_grads(node, _grads_of(dla), ra, names, "micro-batch 1 + shared")
    _check_grads(node, _grads_of(dlb), rb, names, "micro-batch 2 + shared")


# ------------------------------------------------------------------------------------------------------------------------ 6 layouts
@node_param
@pytest.mark.parametrize("layout", ["sum", "transposed", "bf16"])
def test_upstream_gradient_layouts(dev, node, layout):
    """out.sum().backward() (a stride-0 expanded gradient), a transposed non-contiguous gradient, and -- nodes with bf16 activations --
    a bf16 gradient."""
    if layout == "bf16" and not node.bf16_upstream:
        pytest.skip("the node's outputs are fp32")
    leaves, extras = node.make(1)
    names, used = list(leaves), _all_used(node)
    _, ref_outs = _ref_graph(node, 1)
    if layout == "transposed" and all(o.dim() < 2 for o in ref_outs):
        pytest.skip("no output with two axes")
    with node.engine():
        dl, _, outs = _forward(node, dev, leaves, extras, set(names))
        _backward(outs, node.upstream([_tensor(o).shape for o in outs], used, 1, layout), dev, layout)
    _check_grads(node, _grads_of(dl), _ref_grads(node, 1, used, 1, layout), names, layout)


# ------------------------------------------------------------------------------------------------------------------------ 7 saved tensors
def _saved_cases():
    return [pytest.param(n, s, id=f"{n.name}-{s}") for n in NODES for s in n.saved]


@pytest.mark.parametrize("node,victim", _saved_cases())
def test_modified_saved_tensor_raises(dev, node, victim):
    """An input (or keep mask, or group / bag offsets) modified in place between forward and backward: PyTorch's version check raises;
    no numbers come back."""
    leaves, extras = node.make(1)
    with node.engine():
        dl, de, outs = _forward(node, dev, leaves, extras, set(leaves))
        target = dl[victim] if victim in dl else de[victim]
        with torch.no_grad():
            target.add_(1 if target.is_floating_point() else 0)      # (+ 0 on a mask or an offset table: only the version counter moves)
        with pytest.raises(RuntimeError, match="modified by an inplace operation"):
            _backward(outs, node.upstream([_tensor(o).shape for o in outs], _all_used(node), 1), dev)
