"""fp64 references of the activations that the kernels approximate (GELU and its derivative, tanh, sigmoid, the gate's gradient terms) and
the deterministic argument grids that tests/test_activation_domain_gpu.py drives through the entry points.  Plain torch on the CPU; the
references are checked against torch.autograd in tests/test_activation_domain_cpu.py."""
import math

import torch

LADDER_EXPONENTS = range(-100, -2)          # +-2^-100 ... +-2^-3
INV_SQRT_2PI = 1.0 / math.sqrt(2.0 * math.pi)
INV_SQRT_2 = math.sqrt(0.5)


# ------------------------------------------------------------------------------------------------------------------------ references
def _f64(t):
    return torch.as_tensor(t).detach().cpu().double()


def ndtr64(t):
    """Phi(t) = erfc(-t / sqrt 2) / 2: the far negative tail keeps its relative accuracy (torch.special.ndtr forms 1 - Phi(|t|) and returns
    0 from t = -8.3 on)."""
    return 0.5 * torch.special.erfc(_f64(t) * -INV_SQRT_2)


def gelu64(t):
    t = _f64(t)
    return t * ndtr64(t)


def gelu_grad64(t):
    """d/dt [t Phi(t)] = Phi(t) + t phi(t)."""
    t = _f64(t)
    return ndtr64(t) + t * torch.exp(-0.5 * t * t) * INV_SQRT_2PI


def tanh64(z):
    return torch.tanh(_f64(z))


def sigmoid64(z):
    return torch.sigmoid(_f64(z))


def gate_grads64(za, zb):
    """The gradients of s = sum_j wc_j tanh(za_j) sigmoid(zb_j) at wc = 1, d s = 1: (d/d za, d/d zb, d/d wc) = (b (1 - a^2), a b (1 - b),
    a b).  1 - a^2 and 1 - b are formed without cancellation (sech^2, sigmoid(-z)): the saturated sides keep their relative accuracy."""
    za, zb = _f64(za), _f64(zb)
    a, b = torch.tanh(za), torch.sigmoid(zb)
    sech2 = 1.0 / torch.cosh(za.clamp(-350.0, 350.0)) ** 2
    return b * sech2, a * b * torch.sigmoid(-zb), a * b


# ----------------------------------------------------------------------------------------------------------------------------- grids
def _f32_neighbours(v):
    t = torch.tensor([v], dtype=torch.float32)
    return [float(torch.nextafter(t, torch.tensor([-math.inf]))[0]), float(torch.nextafter(t, torch.tensor([math.inf]))[0])]


def special_points(lim, huge):
    """+-0, +-4 and the fp32 neighbours of +-4 on both sides, +-6, +-12.5, +-20, +-lim; with `huge` also +-1e4 and +-1e30."""
    pts = [0.0, -0.0, 4.0, -4.0] + _f32_neighbours(4.0) + _f32_neighbours(-4.0)
    for v in (6.0, 12.5, 20.0, float(lim)) + ((1e4, 1e30) if huge else ()):
        pts += [v, -v]
    return pts


def ladder_points():
    return [s * 2.0 ** e for e in LADDER_EXPONENTS for s in (1.0, -1.0)]


def _uniform(m, lo, hi, shift):
    """m points of [lo, hi): the m cells' points at fraction `shift` of a cell, so that grids of different shifts interleave."""
    return lo + (hi - lo) * (torch.arange(m, dtype=torch.float64) + shift) / max(m, 1)


def act_grid(n, lim, huge, shift=0.0):
    """fp32 [n]: n // 2 points uniform on [-4, 4], n // 4 uniform on [-13, 13], the ladder +-2^-100 ... +-2^-3, special_points(lim, huge),
    and uniform points on [-lim, lim] for the remainder.  Deterministic; 0 <= shift < 1 moves the uniform points within their cells (the
    calls of one sweep use different shifts).  The order is fixed too: neighbouring columns see different regimes only at the seams."""
    if not 0.0 <= shift < 1.0:
        raise ValueError("act_grid: shift in [0, 1)")
    fixed = torch.tensor(ladder_points() + special_points(lim, huge), dtype=torch.float64)
    rest = n - n // 2 - n // 4 - fixed.numel()
    if rest < 0:
        raise ValueError("act_grid: n = %d cannot hold the ladder and the special points" % n)
    grid = torch.cat([_uniform(n // 2, -4.0, 4.0, shift), _uniform(n // 4, -13.0, 13.0, shift), fixed,
                      _uniform(rest, -float(lim), float(lim), shift)]).float()
    assert grid.numel() == n
    return grid


def grid_with(points, n, lim, shift=0.0):
    """fp32 [n]: the given points, then uniform points on [-lim, lim] (see act_grid) up to n."""
    points = torch.as_tensor(points, dtype=torch.float64).flatten()
    if points.numel() > n:
        raise ValueError("grid_with: more points than n")
    return torch.cat([points, _uniform(n - points.numel(), -float(lim), float(lim), shift)]).float()
