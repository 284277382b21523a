"""madeleine_amd.AdamW on the GPU: parity with torch.optim.AdamW(foreach=False, fused=False) -- the optimiser the reference constructs --
at the bar of torch's own fp32 run, over tensor layouts and parameter groups; void steps (one NaN / inf anywhere changes nothing
anywhere); no host in the step; reproducible bits; NaN-filled scratch; state-dict interchange with torch; one step on the model.

All inputs come from a closed-form recipe (no model in the loop, nothing chaotic):
    parameter i:           sin(arange(n) 0.37 + i) 0.05
    its gradient, step t:  sin(arange(n) 0.11 + 1.3 i + 0.7 t) 10^((i mod 5) - 4)
generated in fp64 and cast.  Tensor 7 never gets a gradient.

The bar.  E(X) = max over the non-empty tensors of max|X - P64| / max|P64|, P64 being torch's fp64 run on the CPU; required is
E(ours) <= 2 E(P32), P32 being torch's fp32 run on the CPU, both sides computed here at run time, for the parameters and both moments.
The factor 2: a different but correctly rounded operation order (FMA contraction, one fused multiply-add for each moment) reproduces
E(P32); rounding the hyperparameters to fp32 before forming 1 - beta2 and the bias corrections gives 2.8 x and must fail.
"""
import functools
from types import SimpleNamespace

import pytest
import torch

import madeleine_amd
from madeleine_amd import functional as MF
from madeleine_amd.optim import MAX_TENSORS, AdamW

pytestmark = pytest.mark.gpu

STEPS = 6
NO_GRAD = 7
BIG = 5                     # the (1048577,) tensor
SHAPES = [(1,), (3,), (513,), (7, 129), (70001,), (1048577,), (0,)]
SHAPES = SHAPES + [(5,)] * (MAX_TENSORS + 3 - len(SHAPES))
SPLIT = 20                  # two-group runs: tensors [0, 20) and [20, ...)
GROUP_HYPER = ({"lr": 1e-3, "weight_decay": 1e-2}, {"lr": 3e-4, "weight_decay": 0.1})


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _numel(s):
    n = 1
    for d in s:
        n *= d
    return n


@functools.lru_cache(maxsize=None)
def params64():
    return tuple((torch.sin(torch.arange(_numel(s), dtype=torch.float64) * 0.37 + i) * 0.05).reshape(s) for i, s in enumerate(SHAPES))


@functools.lru_cache(maxsize=None)
def grads64(t):
    return tuple((torch.sin(torch.arange(_numel(s), dtype=torch.float64) * 0.11 + 1.3 * i + 0.7 * t) * 10.0 ** ((i % 5) - 4)).reshape(s)
                 for i, s in enumerate(SHAPES))


@functools.lru_cache(maxsize=None)
def grads32(t):
    return tuple(g.float() for g in grads64(t))


@functools.lru_cache(maxsize=None)
def lrs(base):
    """The learning rates LinearLR(start_factor=1e-5, total_iters=4) gives a group of lr `base` at steps 0 .. STEPS - 1."""
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=base)
    sched = torch.optim.lr_scheduler.LinearLR(opt, start_factor=1e-5, total_iters=4)
    out = []
    for _ in range(STEPS):
        out.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    return tuple(out)


def _groups(params, two_groups):
    if not two_groups:
        return [{"params": list(params)}]
    return [dict(params=list(params[:SPLIT]), **GROUP_HYPER[0]), dict(params=list(params[SPLIT:]), **GROUP_HYPER[1])]


def _snapshot(opt, params):
    out = {"p": [p.detach().clone() for p in params], "m": [], "v": [], "step": []}
    for p in params:
        st = opt.state.get(p, {})
        out["m"].append(st["exp_avg"].clone() if st else None)
        out["v"].append(st["exp_avg_sq"].clone() if st else None)
        out["step"].append(st["step"].clone() if st else None)
    return out


def _same_bits(a, b):
    for k in ("p", "m", "v", "step"):
        for i, (x, y) in enumerate(zip(a[k], b[k])):
            if (x is None) != (y is None) or (x is not None and not torch.equal(x, y)):
                return "%s[%d] differs" % (k, i)
    return None


@functools.lru_cache(maxsize=None)
def reference(dtype, clip, two_groups, steps=STEPS):
    """torch.optim.AdamW(foreach=False, fused=False) on the CPU (clip_grad_norm_ in front of it when `clip`), under LinearLR."""
    params = [torch.nn.Parameter(p.to(dtype).clone()) for p in params64()]
    opt = torch.optim.AdamW(_groups(params, two_groups), lr=1e-3, foreach=False, fused=False)
    sched = torch.optim.lr_scheduler.LinearLR(opt, start_factor=1e-5, total_iters=4)
    for t in range(steps):
        for i, p in enumerate(params):
            p.grad = None if i == NO_GRAD else grads64(t)[i].to(dtype).clone()
        if clip is not None:
            torch.nn.utils.clip_grad_norm_(params, clip, foreach=False)
        opt.step()
        sched.step()
    return _snapshot(opt, params)


def E(x, ref):
    """max over the non-empty tensors of max|X - P64| / max|P64|"""
    worst = 0.0
    for a, r in zip(x, ref):
        if r is None or r.numel() == 0:
            assert a is None or a.numel() == 0
            continue
        worst = max(worst, float((a.detach().double().cpu() - r).abs().max() / r.abs().max()))
    return worst


def make_params(dev, layout):
    """(parameters, set_grads(t, poison=None)).  layout "flat": parameters and gradients are views of one flat buffer each, at cumulative
    offsets from an odd start (the layout FlatGradSync hands the optimiser: 4-byte alignment is all a tensor has)."""
    p32 = [p.float() for p in params64()]
    if layout == "flat":
        total = sum(p.numel() for p in p32)
        pbuf, gbuf = torch.zeros(total + 1, device=dev), torch.zeros(total + 3, device=dev)
        params, gviews, po, go = [], [], 1, 3
        for p in p32:
            n = p.numel()
            pbuf[po:po + n].copy_(p.reshape(-1))
            params.append(torch.nn.Parameter(pbuf[po:po + n].view(p.shape)))
            gviews.append(gbuf[go:go + n].view(p.shape))
            po, go = po + n, go + n
        assert any(p.data_ptr() % 16 for p in params) and any(g.data_ptr() % 16 for g in gviews)
    else:
        params, gviews = [torch.nn.Parameter(p.to(dev)) for p in p32], None

    def set_grads(t, poison=None):
        for i, p in enumerate(params):
            if i == NO_GRAD:
                p.grad = None
                continue
            g = grads32(t)[i].to(dev)
            if gviews is not None:
                g = gviews[i].copy_(g)
            if poison is not None and poison[0] == i:
                g.view(-1)[poison[1]] = poison[2]
            p.grad = g
    return params, set_grads


def run_ours(dev, clip=None, guard=True, layout="plain", two_groups=False, steps=STEPS):
    params, set_grads = make_params(dev, layout)
    opt = AdamW(_groups(params, two_groups), lr=1e-3, max_grad_norm=clip, skip_nonfinite=guard)
    sched = torch.optim.lr_scheduler.LinearLR(opt, start_factor=1e-5, total_iters=4)
    for t in range(steps):
        set_grads(t)
        opt.step()
        sched.step()
    snap = _snapshot(opt, params)
    assert opt.skipped_steps() == 0
    return snap, opt


def check_parity(snap, clip, two_groups, what):
    p64, p32 = reference(torch.float64, clip, two_groups), reference(torch.float32, clip, two_groups)
    figures = []
    for k in ("p", "m", "v"):
        ours, torchs = E(snap[k], p64[k]), E(p32[k], p64[k])
        figures.append((k, ours, torchs))
        print("%s: E(%s) ours %.3e  torch fp32 %.3e  ratio %.2f" % (what, k, ours, torchs, ours / torchs))
    for k, ours, torchs in figures:
        assert ours <= 2.0 * torchs, (what, k, ours, torchs)
    # `step`: 6 everywhere, no state at all for the tensor that never had a gradient -- as torch shows
    for i, s in enumerate(snap["step"]):
        assert (s is None) == (p64["step"][i] is None) == (i == NO_GRAD)
        if s is not None:
            assert s.shape == () and s.dtype == torch.float32 and s.is_cuda and float(s) == float(p64["step"][i]) == STEPS
    assert torch.equal(snap["p"][NO_GRAD].cpu(), params64()[NO_GRAD].float())


# ---- 1. parity with the reference optimiser ----
@pytest.mark.parametrize("guard", [True, False])
@pytest.mark.parametrize("clip", [None, 0.5])
def test_parity_with_torch_adamw(dev, clip, guard):
    snap, opt = run_ours(dev, clip=clip, guard=guard)
    check_parity(snap, clip, False, "plain clip=%s guard=%s" % (clip, guard))
    if clip is not None or guard:
        g = [x for i, x in enumerate(grads64(STEPS - 1)) if i != NO_GRAD]
        norm = float(torch.sqrt(sum((x.float().double() ** 2).sum() for x in g)))
        assert opt.grad_norm.shape == () and opt.grad_norm.is_cuda
        assert abs(float(opt.grad_norm) - norm) <= 1e-6 * norm


# ---- 2. layouts ----
@pytest.mark.parametrize("clip", [None, 0.5])
def test_views_of_a_flat_buffer_at_odd_offsets(dev, clip):
    snap, _ = run_ours(dev, clip=clip, layout="flat")
    check_parity(snap, clip, False, "flat clip=%s" % clip)


@pytest.mark.parametrize("clip", [None, 0.5])
def test_two_parameter_groups(dev, clip):
    snap, _ = run_ours(dev, clip=clip, two_groups=True)
    check_parity(snap, clip, True, "two groups clip=%s" % clip)


def test_aligned_parameters_with_gradient_views_at_odd_offsets(dev):
    """What FlatGradSync produces: the parameters keep their own (aligned) storage, only the gradients are views at odd offsets.  The
    result is the bits of the all-aligned layout: alignment chooses the width of the loads, never the arithmetic."""
    want, _ = run_ours(dev, clip=0.5, steps=2)
    params, _ = make_params(dev, "plain")
    gbuf = torch.zeros(sum(p.numel() for p in params) + 1, device=dev)
    opt = AdamW(params, lr=1e-3, max_grad_norm=0.5)
    sched = torch.optim.lr_scheduler.LinearLR(opt, start_factor=1e-5, total_iters=4)
    for t in range(2):
        o = 1
        for i, p in enumerate(params):
            p.grad = None if i == NO_GRAD else gbuf[o:o + p.numel()].view(p.shape).copy_(grads32(t)[i])
            o += p.numel()
        opt.step()
        sched.step()
    assert _same_bits(_snapshot(opt, params), want) is None


def test_non_contiguous_gradient(dev):
    w = torch.nn.Parameter(torch.linspace(-1, 1, 35 * 130, device=dev).reshape(35, 130).contiguous())
    twin = torch.nn.Parameter(w.detach().clone())
    g = torch.cos(torch.arange(130 * 35, device=dev, dtype=torch.float32)).reshape(130, 35).t()
    assert not g.is_contiguous()
    a, b = AdamW([w], lr=1e-2), AdamW([twin], lr=1e-2)
    w.grad, twin.grad = g, g.contiguous()
    a.step()
    b.step()
    assert torch.equal(w, twin) and not torch.equal(w, torch.linspace(-1, 1, 35 * 130, device=dev).reshape(35, 130))
    assert w.grad is g                                        # the gradient itself is left as it was


# ---- 3. void step, global ----
def _two_clean_steps(dev):
    params, set_grads = make_params(dev, "plain")
    opt = AdamW(_groups(params, True), lr=1e-3, max_grad_norm=0.5)
    for t in range(2):
        set_grads(t)
        opt.step()
    return _snapshot(opt, params)


@pytest.fixture(scope="module")
def twin(dev):
    """A twin optimiser that takes the clean steps 0 and 1 and never sees a void step."""
    return _two_clean_steps(dev)


PLACES = {"last": (len(SHAPES) - 1, 4), "big": (BIG, 1048577 // 2), "group2": (SPLIT + 3, 0)}


@pytest.mark.parametrize("place", sorted(PLACES))
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
def test_one_non_finite_element_voids_the_step_everywhere(dev, twin, value, place):
    params, set_grads = make_params(dev, "plain")
    opt = AdamW(_groups(params, True), lr=1e-3, max_grad_norm=0.5)
    set_grads(0)
    opt.step()
    before, skipped = _snapshot(opt, params), opt.skipped_steps()
    set_grads(1, poison=PLACES[place] + (value,))
    opt.step()
    assert _same_bits(_snapshot(opt, params), before) is None
    assert opt.skipped_steps() == skipped + 1 == 1
    assert not torch.isfinite(opt.grad_norm)
    set_grads(1)
    opt.step()
    assert _same_bits(_snapshot(opt, params), twin) is None
    assert opt.skipped_steps() == 1 and torch.isfinite(opt.grad_norm)


def test_without_the_guard_a_nan_reaches_the_parameters(dev):
    """skip_nonfinite=False is torch's behaviour: the step is applied, and the counter stays."""
    params, set_grads = make_params(dev, "plain")
    opt = AdamW(params, lr=1e-3, skip_nonfinite=False)
    set_grads(0, poison=(2, 100, float("nan")))
    opt.step()
    assert torch.isnan(params[2].view(-1)[100]) and torch.isfinite(params[2].view(-1)[:100]).all() and torch.isfinite(params[3]).all()
    assert float(opt.state[params[2]]["step"]) == 1 and opt.skipped_steps() == 0


# ---- 4. first step void ----
def test_first_step_void(dev):
    params, set_grads = make_params(dev, "plain")
    start = [p.detach().clone() for p in params]
    opt = AdamW(params, lr=1e-3)
    set_grads(0, poison=(BIG, 17, float("nan")))
    opt.step()
    assert opt.skipped_steps() == 1
    for i, p in enumerate(params):
        assert torch.equal(p, start[i])
        st = opt.state.get(p, {})
        if i == NO_GRAD:
            assert len(st) == 0
        else:
            assert float(st["step"]) == 0 and not st["exp_avg"].any() and not st["exp_avg_sq"].any()
    set_grads(0)
    opt.step()
    fresh_params, fresh_grads = make_params(dev, "plain")
    fresh = AdamW(fresh_params, lr=1e-3)
    fresh_grads(0)
    fresh.step()
    assert _same_bits(_snapshot(opt, params), _snapshot(fresh, fresh_params)) is None
    assert all(float(opt.state[p]["step"]) == 1 for i, p in enumerate(params) if i != NO_GRAD) and opt.skipped_steps() == 1


# ---- 5. no host in the step ----
def test_step_neither_synchronises_nor_allocates(dev):
    params, set_grads = make_params(dev, "flat")
    opt = AdamW(_groups(params, True), lr=1e-3, skip_nonfinite=True, max_grad_norm=1.0)
    for t in range(2):
        set_grads(t)
        opt.step()
    set_grads(2)
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_stats()["allocation.all.allocated"]
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.step()
        norm = opt.grad_norm            # reading the tensor is no synchronisation
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == allocated
    assert float(norm) > 0 and float(opt.state[params[0]]["step"]) == 3


# ---- 6. reproducibility, 7. poisoned scratch ----
@pytest.fixture(scope="module")
def clean_run(dev):
    return run_ours(dev, clip=0.5, two_groups=True)[0]


def test_two_runs_give_the_same_bits(dev, clean_run):
    again, _ = run_ours(dev, clip=0.5, two_groups=True)
    assert _same_bits(again, clean_run) is None


def test_nan_filled_scratch_changes_nothing(dev, clean_run, monkeypatch):
    clean, served = MF._ws, []

    def poisoned(nbytes, device):
        served.append(nbytes)
        return clean(nbytes, device).fill_(0xFF)      # every float a NaN
    monkeypatch.setattr(MF, "_ws", poisoned)
    again, opt = run_ours(dev, clip=0.5, two_groups=True)
    assert served and _same_bits(again, clean_run) is None
    assert torch.isfinite(opt.grad_norm)


# ---- 8. interchange with torch.optim.AdamW ----
def _manual_steps(opt, params, set_grads, steps):
    for t in steps:
        for group, hyper in zip(opt.param_groups, GROUP_HYPER):
            group["lr"] = lrs(hyper["lr"])[t]
        set_grads(t)
        opt.step()


@pytest.mark.parametrize("direction", ["torch_to_ours", "ours_to_torch"])
def test_state_dict_interchange(dev, direction):
    """Three steps of one optimiser, its state_dict loaded into the other, three more: within the bar of test 1 of torch's six steps."""
    params, set_grads = make_params(dev, "plain")
    first_cls, second_cls = (torch.optim.AdamW, AdamW) if direction == "torch_to_ours" else (AdamW, torch.optim.AdamW)
    first = first_cls(_groups(params, True), lr=1e-3)
    _manual_steps(first, params, set_grads, range(0, 3))
    second = second_cls(_groups(params, True), lr=123.0)
    second.load_state_dict(first.state_dict())
    del first
    _manual_steps(second, params, set_grads, range(3, STEPS))
    snap = _snapshot(second, params)
    snap["step"] = [None if s is None else s.to(dev, torch.float32) for s in snap["step"]]
    check_parity(snap, None, True, direction)


# ---- 9. on the model ----
def test_on_the_model(dev):
    from madeleine_amd import InfoNCE, MADELEINE, calculate_losses
    mods = ["HE", "HER2", "ER"]
    B, N, D = 4, 64, 64
    torch.manual_seed(7)
    model = MADELEINE(SimpleNamespace(MODALITIES=mods, wsi_encoder="abmil", patch_embedding_dim=D, wsi_encoder_hidden_dim=512,
                                      activation="softmax", n_heads=4)).to(dev).eval()
    feats = torch.randn(B, len(mods), N, D, generator=torch.Generator().manual_seed(3))
    labels = torch.ones(B, len(mods))
    args = SimpleNamespace(global_loss="info-nce", symmetric_cl=True, local_loss_weight=1.0)
    opt = madeleine_amd.AdamW(model.parameters(), lr=1e-3)
    named = dict(model.named_parameters())
    start = {k: p.detach().clone() for k, p in named.items()}

    def backward(scale):
        opt.zero_grad(set_to_none=True)
        embs, toks = model({"feats": feats}, device=dev, train=True)
        loss, flag = calculate_losses(mods[1:], InfoNCE(temperature=0.001), None, None, embs, toks, labels[:, 1:], args)
        assert flag
        (loss * scale).backward()

    backward(float("nan"))
    opt.step()
    assert opt.skipped_steps() == 1
    for k, p in named.items():
        assert torch.equal(p, start[k]), k
    backward(1.0)
    opt.step()
    assert opt.skipped_steps() == 1
    trained = [k for k, p in named.items() if p.grad is not None]
    assert len(trained) >= 20
    # The token_projector takes no part in this loss.  Its bias is handed to the pooling node as it is and keeps .grad None: the optimiser
    # must leave it entirely alone.  Its weight reaches that node through the head-major column permutation, an autograd node that turns
    # the "no gradient" it is handed into an all-zero gradient: a gradient all the same, so, as in torch, weight decay alone moves it.
    no_grad = [k for k, p in named.items() if p.grad is None]
    assert no_grad and all(k.startswith("token_projector.") for k in no_grad), no_grad
    for k in no_grad:
        assert torch.equal(named[k], start[k]) and len(opt.state.get(named[k], {})) == 0, k
    for k, p in named.items():
        assert torch.isfinite(p).all(), k
        if p.grad is None:
            continue
        assert float(opt.state[p]["step"]) == 1, k
        if k.startswith("token_projector."):
            assert not p.grad.any() and not opt.state[p]["exp_avg"].any() and not opt.state[p]["exp_avg_sq"].any(), k
            assert torch.equal(p, start[k] * (1.0 - 1e-3 * 1e-2)), k
        elif bool(start[k].any()) or bool(p.grad.any()):     # a parameter moves unless both it and its gradient are exactly zero
            assert not torch.equal(p, start[k]), k
