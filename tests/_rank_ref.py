"""The fp64 oracle of the smooth rank and the seeded test matrices the CPU and GPU rank tests share.  Test infrastructure."""
import functools

import numpy as np

EPS = 1e-7


def oracle(E, eps=EPS):
    """(rank, sigma): numpy's fp64 SVD of E widened to fp64, then the reference's four lines (madeleine/utils/utils.py:180-201) in
    fp64, unrounded."""
    E = np.asarray(E)
    S = np.linalg.svd(E.astype(np.float64), compute_uv=False)
    p = S / np.abs(S).sum() + eps
    p = p[:E.shape[1]]
    return float(np.exp(-np.sum(p * np.log(p)))), S


def gauss(n, d, seed):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def _low_rank(n, d, r, seed, noise=0.0):
    g = np.random.default_rng(seed)
    E = g.standard_normal((n, r)) @ g.standard_normal((r, d))
    if noise:
        E = E + noise * g.standard_normal((n, d))
    return E.astype(np.float32)


def _spectrum(n, d, lo, scale, seed):
    """U diag(s) V^T with orthonormal U, V and s geometric from 1 down to `lo`, times `scale`."""
    g = np.random.default_rng(seed)
    k = min(n, d)
    U, _ = np.linalg.qr(g.standard_normal((n, k)))
    V, _ = np.linalg.qr(g.standard_normal((d, k)))
    s = np.geomspace(1.0, lo, k) * scale
    return ((U * s) @ V.T).astype(np.float32)


def _common_row(n, d, seed):
    g = np.random.default_rng(seed)
    return (0.05 * g.standard_normal((n, d)) + g.standard_normal((1, d))).astype(np.float32)


def _repeated(rows, times, d, seed):
    return np.tile(gauss(rows, d, seed), (times, 1))


FULL, DEFICIENT = "full", "deficient"
# name -> (class, builder).  DEFICIENT: exactly rank-deficient in exact arithmetic (the true zeros come out as noise)
CASES = {
    "gauss_300x512": (FULL, lambda: gauss(300, 512, 1)),
    "gauss_512x512": (FULL, lambda: gauss(512, 512, 2)),
    "gauss_1153x512": (FULL, lambda: gauss(1153, 512, 3)),
    "gauss_37x512": (FULL, lambda: gauss(37, 512, 4)),
    "gauss_700x64": (FULL, lambda: gauss(700, 64, 5)),
    "rank1_600x512": (DEFICIENT, lambda: _low_rank(600, 512, 1, 6)),
    "rank5_600x512": (DEFICIENT, lambda: _low_rank(600, 512, 5, 7)),
    "rank5_noise_600x512": (FULL, lambda: _low_rank(600, 512, 5, 8, noise=1e-3)),
    "geometric_1e-6_800x512": (FULL, lambda: _spectrum(800, 512, 1e-6, 1.0, 9)),
    "geometric_1e-3_scaled_1e4_800x512": (FULL, lambda: _spectrum(800, 512, 1e-3, 1e4, 10)),
    "common_row_900x512": (FULL, lambda: _common_row(900, 512, 11)),
    "repeated_40x20": (DEFICIENT, lambda: _repeated(40, 20, 512, 12)),
    "one_row_1x512": (FULL, lambda: gauss(1, 512, 13)),
    "two_rows_2x512": (FULL, lambda: gauss(2, 512, 14)),
}
# |rank - oracle| <= RANK_TOL[class] * oracle.  FULL: the tridiagonalisation perturbs G by O(k 2^-52) lambda_max, every sigma moves by
# less than 1e-10 relative.  DEFICIENT: each of up to 512 true zeros comes out as at most sqrt(512 * 2^-52) = 3.4e-7 sigma_max and
# adds at most 3.4e-7 |ln 3.4e-7| to H: 2.6e-3 in all.
RANK_TOL = {FULL: 1e-6, DEFICIENT: 2.6e-3}
SIGMA_TOL = 1e-9          # |sigma_i^2 - sigma*_i^2| <= SIGMA_TOL sigma*_max^2: 15x the backward error n k 2^-53 at 1153 x 512


@functools.lru_cache(maxsize=None)
def case(name):
    """(E fp32 [n, d], oracle rank, oracle sigma [k]) of a named case: built and decomposed once per session; treat as read-only."""
    E = CASES[name][1]()
    E.setflags(write=False)
    rank, S = oracle(E)
    S.setflags(write=False)
    return E, rank, S
