"""madeleine_amd.AdamW without a GPU: the mdl_adamw_* entry points (declared, bound, exported, argument validation), the ABI revision,
construction / state_dict handling on CPU parameters, the argument errors and the refusal of a CPU step."""
import ctypes
import struct

import pytest
import torch

import madeleine_amd
from madeleine_amd import _build, _native
from madeleine_amd import functional as MF
from madeleine_amd.optim import MAX_TENSORS, AdamW

E_ARG, E_ALIGN, E_UNSUP = -1, -2, -3
ENTRY_POINTS = ("mdl_adamw_ws_bytes", "mdl_adamw_grad_stats", "mdl_adamw_update", "mdl_adamw_commit")


@pytest.fixture(scope="module")
def lib():
    return _native.lib()


def _params(n=3, dtype=torch.float32):
    return [torch.nn.Parameter(torch.arange(4 + i, dtype=dtype) * 0.1) for i in range(n)]


def test_entry_points_are_declared_bound_and_exported(lib):
    with open(_build.HEADER) as f:
        header = f.read()
    for name in ENTRY_POINTS:
        assert name + "(" in header
        assert name in _native.SIGNATURES
        fn = getattr(lib, name)
        res, args = _native.SIGNATURES[name]
        assert fn.restype is res and list(fn.argtypes) == list(args)
    assert _native.SIGNATURES["mdl_adamw_ws_bytes"] == (ctypes.c_int64, [ctypes.c_int64])
    # the hyperparameters travel as the bit patterns of doubles: six uint64_t, no float
    upd = _native.SIGNATURES["mdl_adamw_update"][1]
    assert upd.count(ctypes.c_uint64) == 6 and ctypes.c_float not in upd
    assert MF._f64_bits(0.999) == struct.unpack("<Q", struct.pack("<d", 0.999))[0]


def test_abi_version_is_still_26(lib):
    assert _native.ABI_VERSION == 26 and lib.mdl_abi_version() == 26


def test_constants():
    assert MAX_TENSORS == _native._DEFINES["MDL_ADAMW_MAX_TENSORS"] == MF.ADAMW_MAX_TENSORS >= 41
    assert MAX_TENSORS * 48 < 2560       # the kernel-argument table: 5 pointers and a size per tensor
    assert (MF.ADAMW_GUARD, MF.ADAMW_CLIP, MF.ADAMW_FINAL) == (1, 2, 4)
    assert madeleine_amd.AdamW is AdamW and "AdamW" in madeleine_amd.__all__


def test_workspace_query(lib):
    ws = lib.mdl_adamw_ws_bytes
    blocks = _native._DEFINES["MDL_ADAMW_STAT_BLOCKS"]
    assert ws(-1) == E_ARG and ws(-(2 ** 40)) == E_ARG
    assert ws(0) == 0 and ws(1) == 8 * blocks and ws(3) == 3 * 8 * blocks
    most = _native._DEFINES["MDL_ADAMW_MAX_STAT_LAUNCHES"]
    assert ws(most) == most * 8 * blocks and ws(most + 1) == E_UNSUP
    with pytest.raises(RuntimeError):
        MF.adamw_workspace(-1, "cpu")


def test_launchers_validate_arguments(lib):
    raw = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(raw) + 15) & ~15
    one = (ctypes.c_void_p * 1)(p)
    odd = (ctypes.c_void_p * 1)(p + 2)
    null = (ctypes.c_void_p * 1)(None)
    n1, neg = (ctypes.c_int64 * 1)(4), (ctypes.c_int64 * 1)(-1)
    bits = [MF._f64_bits(x) for x in (1e-3, 0.9, 0.999, 1e-8, 1e-2, 1.0)]
    stats, upd, commit = lib.mdl_adamw_grad_stats, lib.mdl_adamw_update, lib.mdl_adamw_commit
    # every refusal comes before any launch
    assert stats(-1, one, n1, p, 0, 1, None) == E_ARG
    assert stats(MAX_TENSORS + 1, one, n1, p, 0, 1, None) == E_UNSUP
    assert stats(1, None, n1, p, 0, 1, None) == E_ARG and stats(1, one, None, p, 0, 1, None) == E_ARG
    assert stats(1, one, n1, None, 0, 1, None) == E_ARG
    assert stats(1, one, n1, p, 1, 1, None) == E_ARG and stats(1, one, n1, p, -1, 1, None) == E_ARG and stats(1, one, n1, p, 0, 0, None) == E_ARG
    assert stats(1, one, n1, p + 4, 0, 1, None) == E_ALIGN and stats(1, odd, n1, p, 0, 1, None) == E_ALIGN
    assert stats(1, one, neg, p, 0, 1, None) == E_ARG and stats(1, null, n1, p, 0, 1, None) == E_ARG

    def update(nt=1, P=one, G=one, M=one, V=one, S=one, N=n1, flags=1, ws=p, launches=1):
        return upd(nt, P, G, M, V, S, N, *bits, flags, ws, launches, None)
    assert update(nt=-1) == E_ARG and update(nt=MAX_TENSORS + 1) == E_UNSUP
    for k in "PGMVSN":
        assert update(**{k: None}) == E_ARG
    for k in "PGMVS":
        assert update(**{k: null}) == E_ARG and update(**{k: odd}) == E_ALIGN
    assert update(N=neg) == E_ARG and update(flags=8) == E_ARG and update(flags=4) == E_ARG
    assert update(ws=None) == E_ARG and update(ws=p + 8) == E_ALIGN and update(launches=0) == E_ARG
    assert update(flags=2, ws=None) == E_ARG

    grad_norm, skipped = p, p + 8
    assert commit(-1, one, 1, p, 1, grad_norm, skipped, None) == E_ARG
    assert commit(MAX_TENSORS + 1, one, 1, p, 1, grad_norm, skipped, None) == E_UNSUP
    assert commit(1, None, 1, p, 1, grad_norm, skipped, None) == E_ARG and commit(1, null, 1, p, 1, grad_norm, skipped, None) == E_ARG
    assert commit(1, odd, 1, p, 1, grad_norm, skipped, None) == E_ALIGN
    assert commit(1, one, 8, p, 1, grad_norm, skipped, None) == E_ARG
    assert commit(1, one, 1, None, 1, grad_norm, skipped, None) == E_ARG and commit(1, one, 1 | 4, p, 1, None, skipped, None) == E_ARG
    assert commit(1, one, 1 | 4, p, 1, grad_norm, None, None) == E_ARG


def test_construction_and_state_dict_on_cpu_parameters():
    ps = _params()
    opt = AdamW(ps, lr=2e-3, weight_decay=0.1, max_grad_norm=1.0)
    assert isinstance(opt, torch.optim.Optimizer)
    g = opt.param_groups[0]
    assert g["lr"] == 2e-3 and g["betas"] == (0.9, 0.999) and g["eps"] == 1e-8 and g["weight_decay"] == 0.1
    assert opt.max_grad_norm == 1.0 and opt.skip_nonfinite is True
    assert opt.grad_norm.shape == () and opt.grad_norm.dtype == torch.float32 and opt.skipped_steps() == 0
    sd = opt.state_dict()
    assert sd["state"] == {} and len(sd["param_groups"]) == 1
    # schedulers drive it as they drive torch's
    sched = torch.optim.lr_scheduler.LinearLR(opt, start_factor=1e-5, total_iters=4)
    assert opt.param_groups[0]["lr"] == pytest.approx(2e-8)
    sched.step()
    assert isinstance(opt.param_groups[0]["lr"], float) and opt.param_groups[0]["lr"] > 2e-8
    torch.optim.lr_scheduler.CosineAnnealingLR(AdamW(_params()), T_max=3)


@pytest.mark.parametrize("kwargs", [{}, {"fused": False, "foreach": False}, {"foreach": True}])
def test_state_dicts_load_in_both_directions(kwargs):
    """torch.optim.AdamW's state (CPU `step` when it is neither fused nor capturable) becomes the fused layout here, and this class's
    state dict loads into torch.optim.AdamW, which then steps."""
    ps = _params()
    ref = torch.optim.AdamW(ps, lr=1e-3, **kwargs)
    for t in range(2):
        for i, p in enumerate(ps[:2]):      # the last parameter never gets a gradient: no state
            p.grad = torch.full_like(p, 0.1 * (i + t + 1))
        ref.step()
    ours = AdamW(ps, lr=5e-4)
    ours.load_state_dict(ref.state_dict())
    assert ours.param_groups[0]["lr"] == 1e-3
    for p in ps[:2]:
        st = ours.state[p]
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"}
        assert st["step"].shape == () and st["step"].dtype == torch.float32 and st["step"].device == p.device and float(st["step"]) == 2.0
        assert torch.equal(st["exp_avg"], ref.state[p]["exp_avg"]) and torch.equal(st["exp_avg_sq"], ref.state[p]["exp_avg_sq"])
    assert len(ours.state.get(ps[2], {})) == 0
    back = torch.optim.AdamW(ps, lr=7e-4)
    back.load_state_dict(ours.state_dict())
    before = [p.detach().clone() for p in ps]
    back.step()
    assert float(back.state[ps[0]]["step"]) == 3.0
    assert all(not torch.equal(a, p) for a, p in zip(before[:2], ps[:2])) and torch.equal(before[2], ps[2])


def test_argument_errors():
    with pytest.raises(ValueError, match="lr"):
        AdamW(_params(), lr=torch.tensor(1e-3))
    with pytest.raises(ValueError, match="betas"):
        AdamW(_params(), betas=(torch.tensor(0.9), torch.tensor(0.999)))
    for bad in ({"lr": -1.0}, {"eps": -1.0}, {"betas": (1.0, 0.999)}, {"betas": (0.9, -0.1)}, {"weight_decay": -1.0},
                {"max_grad_norm": 0.0}, {"max_grad_norm": float("inf")}, {"max_grad_norm": -2.0}):
        with pytest.raises(ValueError):
            AdamW(_params(), **bad)
    with pytest.raises(TypeError):
        AdamW(_params(), 1e-3, (0.9, 0.999), 1e-8, 1e-2, 1.0)        # max_grad_norm and skip_nonfinite are keyword-only
    # non-fp32 and non-contiguous parameters: at construction, naming the parameter
    with pytest.raises(ValueError, match="parameter 1 of group 0.*float64"):
        AdamW([_params(1)[0], torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))])
    with pytest.raises(ValueError, match="parameter 0 of group 0.*bfloat16"):
        AdamW([torch.nn.Parameter(torch.zeros(3, dtype=torch.bfloat16))])
    with pytest.raises(ValueError, match="parameter 0 of group 1.*contiguous"):
        AdamW([{"params": _params(1)}, {"params": [torch.nn.Parameter(torch.zeros(4, 6).t())]}])
    opt = AdamW(_params(2))
    with pytest.raises(ValueError, match="float16"):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(2, dtype=torch.float16))]})
    # a tensor lr that arrives later (a scheduler, a loaded group) is refused by step(), before any device work
    opt = AdamW(_params(1))
    opt.param_groups[0]["params"][0].grad = torch.zeros(4)
    opt.param_groups[0]["lr"] = torch.tensor(1e-3)
    with pytest.raises(ValueError, match="group 0"):
        opt.step()
    opt.param_groups[0]["lr"] = 1e-3
    opt.param_groups[0]["amsgrad"] = True
    with pytest.raises(ValueError, match="amsgrad"):
        opt.step()


def test_step_on_cpu_parameters_raises():
    ps = _params(2)
    opt = AdamW(ps)
    assert opt.step() is None                   # no gradient anywhere: nothing to do, nothing to refuse
    before = [p.detach().clone() for p in ps]
    ps[1].grad = torch.ones_like(ps[1])
    with pytest.raises(RuntimeError, match="parameter 1 of group 0.*cpu.*no CPU fallback"):
        opt.step()
    assert all(torch.equal(a, p) for a, p in zip(before, ps)) and len(opt.state) == 0
    named = AdamW(torch.nn.Linear(3, 2).named_parameters())
    names = named.param_groups[0].get("param_names")
    if names:                                    # torch records the names of named_parameters(): the error uses them
        p = named.param_groups[0]["params"][1]
        p.grad = torch.ones_like(p)
        with pytest.raises(RuntimeError, match="'bias'"):
            named.step()


def test_sparse_gradient_is_refused_by_name():
    emb = torch.nn.Embedding(5, 3, sparse=True)
    opt = AdamW(emb.parameters())
    emb(torch.tensor([1, 2])).sum().backward()
    assert emb.weight.grad.is_sparse
    with pytest.raises(RuntimeError, match="parameter 0 of group 0 has a sparse gradient"):
        opt.step()
