#!/usr/bin/env python3
"""Writes tests/golden/got_rect.npz: the reference's own fp32 GOT(v, q) value, dV and dQ for token sets of different sizes
(v [k, n, d], q [k, m, d]).  Outputs only: the inputs come from the recipe generator (tests/test_got_rect_*.py, `inputs`).

Imports the reference the way oracle/gen_golden.py does (empty `wandb` / `h5py` modules, torch.Tensor.cuda -> identity), so it runs
only where the reference is checked out (MADELEINE_REFERENCE, default: `reference` next to this repository), on the CPU.  Usage: tools/gen_golden_got_rect.py"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("MADELEINE_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)
for _m in ("wandb", "h5py"):
    sys.modules.setdefault(_m, types.ModuleType(_m))
torch.Tensor.cuda = lambda self, *a, **k: self  # noqa: E731  (CPU only)

from madeleine.utils import loss as ref_loss  # noqa: E402  (reference)
from oracle import recipe  # noqa: E402

SHAPES = [(2, 40, 56, 128), (3, 70, 33, 128), (1, 1, 9, 32), (2, 17, 1, 64)]


def t(shape, key):
    return torch.from_numpy(recipe.uniform(shape, key, -1.0, 1.0))


def inputs(k, n, m, d):
    v = t((k, n, d), f"got_rect:{k}x{n}x{m}x{d}:v")
    q = t((k, m, d), f"got_rect:{k}x{n}x{m}x{d}:q") + 0.7 * v[:, torch.arange(m) % n]
    return v, q


def main():
    torch.set_num_threads(1)   # one summation order
    out = {}
    for k, n, m, d in SHAPES:
        v, q = inputs(k, n, m, d)
        v.requires_grad_()
        q.requires_grad_()
        loss = ref_loss.GOT(v, q, subsample=None)
        loss.backward()
        tag = f"{k}x{n}x{m}x{d}"
        out[tag + "/loss"] = np.float32(loss.item())
        out[tag + "/dv"] = v.grad.numpy().astype(np.float32)
        out[tag + "/dq"] = q.grad.numpy().astype(np.float32)
        print(tag, float(out[tag + "/loss"]))
    path = os.path.join(ROOT, "tests", "golden", "got_rect.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
