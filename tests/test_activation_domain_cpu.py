"""The fp64 references and the argument grids of tests/_act_ref.py, which tests/test_activation_domain_gpu.py holds the kernels' fitted
activations to: the references against torch.autograd of F.gelu, tanh and sigmoid in fp64 (and the far negative GELU tail against its
asymptotic series, where 1 - Phi(|t|) would have cancelled), the grids for their size and for every special point."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import _act_ref as R


def _probe_points():
    return torch.cat([R.act_grid(2048, 40, False).double(), torch.linspace(-30, 30, 4001, dtype=torch.float64)])


def test_gelu_references_match_autograd_of_gelu():
    t = _probe_points().requires_grad_()
    y = F.gelu(t)
    (g,) = torch.autograd.grad(y.sum(), t)
    assert float((R.gelu64(t) - y.detach()).abs().max()) <= 1e-15 * 40
    assert float((R.gelu_grad64(t) - g).abs().max()) <= 1e-14


def test_gelu_reference_keeps_the_relative_accuracy_of_the_negative_tail():
    """Phi(-t) = phi(t) / t (1 - 1/t^2 + 3/t^4 - 15/t^6 + ...): the series' truncation error is below its first omitted term."""
    t = torch.linspace(10.0, 37.0, 271, dtype=torch.float64)
    phi = torch.exp(-0.5 * t * t) * R.INV_SQRT_2PI
    series = phi / t * (1 - t ** -2 + 3 * t ** -4 - 15 * t ** -6)
    got = R.gelu64(-t)
    assert bool((got < 0).all())
    assert float(((got / (-t * series)) - 1).abs().max()) <= 105 * 10.0 ** -8 + 1e-12


def test_gate_references_match_autograd_of_tanh_and_sigmoid():
    za = _probe_points().requires_grad_()
    zb = _probe_points().flip(0).clone().requires_grad_()
    wc = torch.ones_like(za).requires_grad_()
    a, b = torch.tanh(za), torch.sigmoid(zb)
    assert torch.equal(R.tanh64(za), a.detach()) and torch.equal(R.sigmoid64(zb), b.detach())
    ga, gb, gw = torch.autograd.grad((wc * a * b).sum(), (za, zb, wc))
    da, db, dw = R.gate_grads64(za, zb)
    for name, got, want in (("b (1 - a^2)", da, ga), ("a b (1 - b)", db, gb), ("a b", dw, gw)):
        assert float((got - want).abs().max()) <= 1e-15, name
    # float32 and device-less inputs come back as fp64 on the CPU
    assert R.tanh64(torch.tensor([0.5])).dtype == torch.float64 and R.gelu64(torch.tensor([0.5])).dtype == torch.float64


@pytest.mark.parametrize("n,lim,huge", [(2048, 40, True), (2048, 40, False), (4096, 100, True), (864, 8, True)])
def test_act_grid_size_and_special_points(n, lim, huge):
    g = R.act_grid(n, lim, huge)
    assert g.dtype == torch.float32 and g.shape == (n,) and bool(torch.isfinite(g).all())
    bits = set(g.view(torch.int32).tolist())
    lo4, hi4 = R._f32_neighbours(4.0)
    assert lo4 < 4.0 < hi4 and lo4 == 4.0 - 2.0 ** -22 and hi4 == 4.0 + 2.0 ** -21
    want = [0.0, -0.0, 4.0, -4.0, lo4, hi4, -lo4, -hi4, 6.0, -6.0, 12.5, -12.5, 20.0, -20.0, float(lim), -float(lim)]
    want += [s * 2.0 ** e for e in range(-100, -2) for s in (1.0, -1.0)]
    if huge:
        want += [1e4, -1e4, 1e30, -1e30]
    for v in want:
        assert torch.tensor([v], dtype=torch.float32).view(torch.int32).item() in bits, v      # by bit pattern: -0 is not +0
    assert float(g.abs().max()) == (float(torch.tensor(1e30, dtype=torch.float32)) if huge else float(lim))
    inner = g.abs() <= 4
    assert int(inner.sum()) >= n // 2 and int((g.abs() <= 13).sum()) >= n // 2 + n // 4
    assert torch.equal(g, R.act_grid(n, lim, huge)), "deterministic"


def test_act_grid_shifts_interleave_and_small_n_is_refused():
    a, b = R.act_grid(2048, 40, True, 0.0), R.act_grid(2048, 40, True, 0.5)
    assert a.shape == b.shape and int((a != b).sum()) == 2048 - 196 - 20       # all but the ladder and the special points move
    assert math.isclose(float(b[0] - a[0]), 0.5 * 8 / 1024, rel_tol=1e-5)
    with pytest.raises(ValueError):
        R.act_grid(256, 40, False)
    with pytest.raises(ValueError):
        R.act_grid(2048, 40, False, 1.0)


def test_grid_with_holds_the_given_points():
    pts = [8.0 - t / 16 for t in range(257)]
    g = R.grid_with(pts, 512, 8, 0.25)
    assert g.shape == (512,) and g[:257].tolist() == pts and float(g.abs().max()) == 8.0
    with pytest.raises(ValueError):
        R.grid_with(pts, 100, 8)
