"""InfoNCE with explicit negatives (negative_keys, unpaired [M,D] and paired [N,M,D]) on the HIP kernels, against an fp64 restatement
written here: F.normalize on every row, logits [q.p | q.n^T] / T with the target in column 0, F.cross_entropy.  The reference branch
(loss.py:93-110) builds those logits and returns None, so there is no oracle value for it; the cross entropy of its in-batch branch
(loss.py:125) is the computation.  Tolerances: the loss within 1e-3 relative (+1e-5), gradients by _grad_ok (1e-3 of fp64, or twice the
fp32 torch reference's own error where T = 0.001 saturates the softmax)."""
import pytest
import torch
import torch.nn.functional as F

from tests.test_bench_path_gpu import GEMM_OPS
from tests.test_hip_kernels import _grad_ok

pytestmark = pytest.mark.gpu
TOL = 1e-3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def ref_loss(q, p, neg, T, paired, reduction="mean"):
    qn, pn, nn_ = F.normalize(q, dim=-1), F.normalize(p, dim=-1), F.normalize(neg, dim=-1)
    pos = (qn * pn).sum(-1, keepdim=True)
    negl = (qn.unsqueeze(1) @ nn_.transpose(-2, -1)).squeeze(1) if paired else qn @ nn_.transpose(-2, -1)
    logits = torch.cat([pos, negl], dim=1)
    return F.cross_entropy(logits / T, torch.zeros(len(q), dtype=torch.long, device=q.device), reduction=reduction)


def inputs(N, M, D, paired, seed, device="cpu"):
    g = torch.Generator(device=device).manual_seed(seed)
    q = torch.randn(N, D, generator=g, device=device)
    p = torch.randn(N, D, generator=g, device=device) + 0.5 * q
    neg = torch.randn(*((N, M, D) if paired else (M, D)), generator=g, device=device)
    return q, p, neg


def grads(fn, tensors):
    leaves = [x.detach().clone().requires_grad_() for x in tensors]
    out = fn(*leaves)
    out.backward()
    return out.detach(), [x.grad for x in leaves]


def check_against_fp64(dev, q, p, neg, T, paired, reduction="mean", weight=None):
    from madeleine_amd import InfoNCE
    mode = "paired" if paired else "unpaired"
    crit = InfoNCE(temperature=T, reduction=reduction, negative_mode=mode)

    def ours(a, b, c):
        out = crit(a, b, negative_keys=c)
        return (out * weight.to(dev)).sum() if weight is not None else out

    def theirs(a, b, c):
        out = ref_loss(a, b, c, T, paired, reduction)
        return (out * weight.to(a.device, a.dtype)).sum() if weight is not None else out

    hip, g_hip = grads(ours, [x.to(dev) for x in (q, p, neg)])
    r64, g64 = grads(theirs, [x.double() for x in (q, p, neg)])
    _, g32 = grads(theirs, [x.float() for x in (q, p, neg)])
    assert abs(float(hip) - float(r64)) <= TOL * abs(float(r64)) + 1e-5, (float(hip), float(r64))
    for a, b32, b64 in zip(g_hip, g32, g64):
        assert a.shape == b64.shape
        _grad_ok(a, b32.cpu(), b64.cpu())
    return hip, g_hip


@pytest.mark.parametrize("T", [0.001, 0.1])
@pytest.mark.parametrize("M", [0, 1, 31, 300, 4096])
@pytest.mark.parametrize("N", [1, 7, 33, 256])
def test_unpaired_against_fp64(dev, N, M, T):
    q, p, neg = inputs(N, M, 512, False, 1000 * N + M)
    check_against_fp64(dev, q, p, neg, T, False)


@pytest.mark.parametrize("T", [0.001, 0.1])
@pytest.mark.parametrize("D", [512, 128])
@pytest.mark.parametrize("M", [1, 15, 256])
@pytest.mark.parametrize("N", [1, 7, 64])
def test_paired_against_fp64(dev, N, M, D, T):
    q, p, neg = inputs(N, M, D, True, 7 * N + M + D)
    check_against_fp64(dev, q, p, neg, T, True)


@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("reduction", ["none", "sum"])
def test_reductions_at_an_odd_width(dev, reduction, paired):
    """D = 100 (Q, P padded to 128, the negatives read as they are), 'none' under a non-uniform upstream weight and 'sum'."""
    N, M, D = 13, 70, 100
    q, p, neg = inputs(N, M, D, paired, 5)
    w = torch.linspace(0.25, 2.0, N) if reduction == "none" else None
    check_against_fp64(dev, q, p, neg, 0.1, paired, reduction, w)


@pytest.mark.parametrize("paired", [False, True])
def test_narrow_and_misaligned_negatives(dev, paired):
    """The 4-byte load path: D = 37 (rows not 16-byte aligned), and D = 64 with the bank starting one float into its storage."""
    q, p, neg = inputs(9, 45, 37, paired, 11)
    check_against_fp64(dev, q, p, neg, 0.05, paired)
    q, p, neg = inputs(9, 45, 64, paired, 12)
    flat = torch.empty(neg.numel() + 1, device=dev)
    flat[1:] = neg.to(dev).reshape(-1)
    shifted = flat[1:].view(neg.shape)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 != 0
    from madeleine_amd import InfoNCE
    crit = InfoNCE(temperature=0.05, negative_mode="paired" if paired else "unpaired")
    a = crit(q.to(dev), p.to(dev), negative_keys=shifted)
    b = crit(q.to(dev), p.to(dev), negative_keys=neg.to(dev))
    assert abs(float(a) - float(ref_loss(q.double(), p.double(), neg.double(), 0.05, paired))) <= TOL * abs(float(b)) + 1e-5


@pytest.mark.parametrize("paired", [False, True])
def test_symmetric_is_not_read(dev, paired):
    from madeleine_amd import InfoNCE
    q, p, neg = [x.to(dev) for x in inputs(33, 300, 100, paired, 3)]
    crit = InfoNCE(temperature=0.001, negative_mode="paired" if paired else "unpaired")
    a, ga = grads(lambda x, y, z: crit(x, y, z, symmetric=False), [q, p, neg])
    b, gb = grads(lambda x, y, z: crit(x, y, z, symmetric=True), [q, p, neg])
    assert torch.equal(a, b)
    for u, v in zip(ga, gb):
        assert torch.equal(u, v)


def _kernel_names(prof):
    return [e.name for e in prof.events()]


@pytest.mark.parametrize("paired", [False, True])
def test_negatives_without_grad(dev, paired):
    """A bank that does not require grad: its grad stays None, no dNeg kernel runs, and the query / positive gradients are the bits of
    the requires_grad run."""
    from torch.profiler import ProfilerActivity, profile
    from madeleine_amd import InfoNCE
    q, p, neg = [x.to(dev) for x in inputs(40, 300, 512, paired, 4)]
    crit = InfoNCE(temperature=0.01, negative_mode="paired" if paired else "unpaired")
    _, g_all = grads(crit, [q, p, neg])
    qq, pp = q.clone().requires_grad_(), p.clone().requires_grad_()
    bank = neg.clone()
    crit(qq, pp, bank).backward()   # warm-up
    qq.grad = pp.grad = None
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        crit(qq, pp, bank).backward()
        torch.cuda.synchronize()
    names = _kernel_names(prof)
    assert bank.grad is None
    assert any("nce_neg_" in n for n in names), "the trace holds no kernel of the explicit-negative path"
    assert not any("dneg" in n for n in names), [n for n in names if "dneg" in n]
    assert torch.equal(qq.grad, g_all[0]) and torch.equal(pp.grad, g_all[1])
    bank.requires_grad_()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        crit(qq, pp, bank).backward()
        torch.cuda.synchronize()
    assert any("dneg" in n for n in _kernel_names(prof))   # the check above can see one


@pytest.mark.parametrize("paired", [False, True])
def test_bf16_under_autocast_is_the_fp32_result_of_the_rounded_values(dev, paired):
    from madeleine_amd import InfoNCE
    q, p, neg = [x.to(dev).bfloat16() for x in inputs(24, 200, 96, paired, 6)]
    crit = InfoNCE(temperature=0.001, negative_mode="paired" if paired else "unpaired")
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        a, ga = grads(crit, [q, p, neg])
    b, gb = grads(crit, [q.float(), p.float(), neg.float()])
    assert a.dtype == torch.float32 and torch.equal(a, b)
    for u, v in zip(ga, gb):
        assert u.dtype == torch.bfloat16 and torch.equal(u, v.bfloat16())


def test_bank_of_65536(dev):
    """Unpaired N = 256, M = 65,536, D = 512 (a 134 MB bank) against fp64 on the GPU."""
    q, p, neg = inputs(256, 65536, 512, False, 21, device=dev)
    check_against_fp64(dev, q, p, neg, 0.07, False)


def test_paired_past_2_to_the_31_elements(dev):
    """Paired N = 64, M = 65,600, D = 512: 2.15e9 elements (8.6 GB), so row 63's negatives straddle element 2^31.  Every row's loss
    against fp64 (row by row), and the gradients of the last row's loss alone."""
    from madeleine_amd import InfoNCE
    N, M, D, T = 64, 65600, 512, 0.05
    assert (N - 1) * M * D < 2 ** 31 < N * M * D
    q, p, neg = inputs(N, M, D, True, 31, device=dev)
    crit = InfoNCE(temperature=T, reduction="none", negative_mode="paired")
    with torch.no_grad():
        rows = crit(q, p, negative_keys=neg)
    for i in range(N):
        r = float(ref_loss(q[i:i + 1].double(), p[i:i + 1].double(), neg[i:i + 1].double(), T, True))
        assert abs(float(rows[i]) - r) <= TOL * abs(r) + 1e-5, (i, float(rows[i]), r)
    qq, pp, nn_ = q.clone().requires_grad_(), p.clone().requires_grad_(), neg.requires_grad_()
    crit(qq, pp, negative_keys=nn_)[-1].backward()
    assert not nn_.grad[0].any() and not nn_.grad[-2].any() and not qq.grad[:-1].any()
    last = [x[-1:].detach() for x in (q, p, neg)]
    _, g64 = grads(lambda a, b, c: ref_loss(a, b, c, T, True), [x.double() for x in last])
    _, g32 = grads(lambda a, b, c: ref_loss(a, b, c, T, True), [x.float() for x in last])
    for a, b32, b64 in zip((qq.grad[-1:], pp.grad[-1:], nn_.grad[-1:]), g32, g64):
        _grad_ok(a, b32.cpu(), b64.cpu())


@pytest.mark.parametrize("paired", [False, True])
def test_no_library_gemm(dev, paired):
    from torch.profiler import ProfilerActivity, profile
    from madeleine_amd import InfoNCE
    q, p, neg = [x.to(dev) for x in inputs(64, 500, 512, paired, 8)]
    crit = InfoNCE(temperature=0.001, negative_mode="paired" if paired else "unpaired")
    grads(crit, [q, p, neg])
    with profile(activities=[ProfilerActivity.CPU]) as prof:
        grads(crit, [q, p, neg])
        torch.cuda.synchronize()
    names = {e.name for e in prof.events()}
    assert not (names & set(GEMM_OPS)), sorted(names & set(GEMM_OPS))


@pytest.mark.parametrize("paired", [False, True])
def test_no_host_sync(dev, paired):
    from madeleine_amd import InfoNCE
    q, p, neg = [x.to(dev).requires_grad_() for x in inputs(32, 300, 512, paired, 9)]
    crit = InfoNCE(temperature=0.001, negative_mode="paired" if paired else "unpaired")
    crit(q, p, negative_keys=neg).backward()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = crit(q, p, negative_keys=neg)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(loss.detach()).item()


@pytest.mark.parametrize("paired", [False, True])
def test_two_runs_give_the_same_bits(dev, paired):
    from madeleine_amd import InfoNCE
    q, p, neg = [x.to(dev) for x in inputs(100, 3000, 512, paired, 10)]
    crit = InfoNCE(temperature=0.001, negative_mode="paired" if paired else "unpaired")
    a, ga = grads(crit, [q, p, neg])
    b, gb = grads(crit, [q, p, neg])
    assert torch.equal(a, b)
    for u, v in zip(ga, gb):
        assert torch.equal(u, v)


@pytest.mark.parametrize("paired", [False, True])
def test_nan_poisoned_workspace_changes_nothing(dev, paired, monkeypatch):
    from madeleine_amd import InfoNCE
    from madeleine_amd import functional as MF
    q, p, neg = [x.to(dev) for x in inputs(37, 1100, 100, paired, 13)]
    crit = InfoNCE(temperature=0.01, reduction="none", negative_mode="paired" if paired else "unpaired")
    w = torch.linspace(0.5, 1.5, 37, device=dev)
    fn = lambda a, b, c: (crit(a, b, c) * w).sum()   # noqa: E731
    a, ga = grads(fn, [q, p, neg])
    clean = MF._ws
    monkeypatch.setattr(MF, "_ws", lambda nbytes, device: clean(nbytes, device).fill_(0xFF))   # every float a NaN
    b, gb = grads(fn, [q, p, neg])
    assert torch.equal(a, b)
    for u, v in zip(ga, gb):
        assert torch.equal(u, v)
