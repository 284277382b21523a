"""The host model of the dropout counter hash (tests/_drop_ref.py) on its own: it agrees with the two restatements of mix32 that tools/
keeps, it gives the thresholds the kernels' drop_threshold gives, its masks have the keep rate and the independence the dropout assumes,
and 64-bit seeds survive it.  tests/test_dropout_hash_gpu.py holds the kernels to this model bit for bit, so what is measured here is
measured of the device's masks.

Measured statistics (n = 2^22 elements each; bound: |rate - (1 - thr / 65536)| <= 5 sqrt(q (1 - q) / n), |correlation| < 5 / sqrt(n) =
2.44e-3; the pairwise figures are over n / 2 pairs and are held to the same bound):
  gate, H = 4, seed 77            rate a - q   rate b - q   corr(ka, kb)   worst of the 4-draw group   corr(seed, seed + 1) a / b
    p = 0.1   16-bit fields        +1.1e-04     -7.2e-07     +2.8e-04       --                          +2.7e-04 / -4.7e-04
    p = 0.25  16-bit (forced)      +1.5e-04     -1.1e-04     -1.3e-05       --                          +2.2e-04 / -6.3e-04
    p = 0.25  byte fields          +1.0e-04     +6.2e-05     +1.4e-04       1.7e-03                     +3.1e-05 / -9.7e-05
  LayerNorm, W = 2048, seed 77     rate - q     corr(even, odd of a pair)   corr(seed, seed + 1)
    p = 0.1                        +3.5e-05     +4.8e-04                    -1.2e-04
    p = 0.25                       -1.5e-04     +5.5e-05                    -4.7e-04
(rate bounds: 7.3e-04 at p = 0.1, 1.06e-03 at p = 0.25.)  Nothing comes near a bound but the byte-field group, whose six correlations
are over n / 2 pairs (one sigma 6.9e-04): 1.7e-03 is 2.5 sigma of the largest of six.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import _drop_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_STAT = 1 << 22
SEED = 77


def _tool(name):
    spec = importlib.util.spec_from_file_location("_tool_" + name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)          # both tools keep their work under `if __name__ == "__main__"`: importing runs nothing
    return mod


def _structured_counters():
    """2^20 counters: consecutive runs from 0, around 2^24 and up to 2^32 - 1, every single bit, the (d << 24 | d << 8) family (what
    the first fold x ^= x >> 16 cancels) alone and on top of a run."""
    run = 1 << 18
    d = np.arange(256, dtype=np.uint64)
    fam = (d << np.uint64(24)) | (d << np.uint64(8))
    parts = [np.arange(run, dtype=np.uint64),
             np.arange((1 << 24) - run // 2, (1 << 24) + run // 2, dtype=np.uint64),
             np.arange((1 << 32) - run, 1 << 32, dtype=np.uint64),
             np.uint64(1) << np.arange(32, dtype=np.uint64), fam,
             (fam[:, None] ^ np.arange(1021, dtype=np.uint64)[None, :]).reshape(-1)]
    c = np.concatenate(parts)
    c = np.concatenate([c, np.arange(0x12345678, 0x12345678 + (1 << 20) - c.size, dtype=np.uint64)])
    assert c.size == 1 << 20 and int(c.max()) == 0xFFFFFFFF
    return c


def test_mix32_agrees_with_both_restatements_in_tools():
    c = _structured_counters()
    mine = D.mix32(c)
    assert mine.dtype == np.uint64 and int(mine.max()) <= 0xFFFFFFFF
    assert np.array_equal(mine, _tool("rng_quality").mix24m(c).astype(np.uint64))
    assert np.array_equal(mine, _tool("bag_draw_restatement").mix32(c.copy()).astype(np.uint64))
    assert np.unique(mine).size == np.unique(c).size, "mix32 is injective on 32-bit counters"


def test_thresholds():
    assert D.thr(0.25) == 16384 and D.thr(0.5) == 32768                   # byte mode: multiples of 256
    assert D.thr(0.1) == 6554 and D.thr(0.3) == 19661                     # 16-bit mode
    assert D.thr(0.1) % 256 and D.thr(0.3) % 256
    assert D.thr(1e-6) == 0 and D.thr(0.99999) == 65535 and D.thr(0.0) == 0
    assert D.thr(np.float64(0.1)) == D.thr(np.float32(0.1)), "p is a C float on the way in"
    # the byte rule and the 16-bit rule keep with the same probability wherever the byte rule applies
    for t in range(256, 65536, 256):
        assert np.count_nonzero(np.arange(256) >= (t >> 8)) * 256 == np.count_nonzero(np.arange(65536) >= t)
    assert D.inv(0.25) == np.float32(4) / np.float32(3) and D.inv(0.1).dtype == np.float32


def _corr(a, b):
    a, b = a.reshape(-1).astype(np.float64), b.reshape(-1).astype(np.float64)
    return float(((a - a.mean()) * (b - b.mean())).mean() / np.sqrt(a.var() * b.var()))


def _rate_ok(mask, p):
    q = 1.0 - D.thr(p) / 65536.0
    dev = float(mask.mean()) - q
    return dev, abs(dev) <= 5.0 * np.sqrt(q * (1.0 - q) / mask.size)


@pytest.mark.parametrize("p,force16", [(0.1, False), (0.25, True), (0.25, False)], ids=["p0.1-16bit", "p0.25-16bit", "p0.25-bytes"])
def test_gate_mask_statistics(p, force16):
    """Keep rate and correlations of gate_keep at n = 2^22 (the figures are in the module docstring)."""
    H = 4
    T = N_STAT // (H * D.HID)
    ka, kb = (D.gate_keep(T, H, w, p, SEED, force16) for w in (0, 1))
    ka1, kb1 = (D.gate_keep(T, H, w, p, SEED + 1, force16) for w in (0, 1))
    assert ka.size == N_STAT
    bound = 5.0 / np.sqrt(N_STAT)
    (da, oka), (db, okb) = _rate_ok(ka, p), _rate_ok(kb, p)
    cab, csa, csb = _corr(ka, kb), _corr(ka, ka1), _corr(kb, kb1)
    line = "gate p=%g force16=%s: rate a %+.1e b %+.1e corr(ka,kb) %+.1e corr(seed,seed+1) a %+.1e b %+.1e" % (p, force16, da, db, cab, csa, csb)
    worst = 0.0
    if D.thr(p) % 256 == 0 and not force16:
        # the four draws that share one hash in byte mode: ka, kb of element 2q and of element 2q + 1
        four = [ka[..., 0::2], kb[..., 0::2], ka[..., 1::2], kb[..., 1::2]]
        worst = max(abs(_corr(four[i], four[j])) for i in range(4) for j in range(i))
        line += " worst of the 4-draw group %.1e" % worst
    print(line)
    assert oka and okb, line
    assert max(abs(cab), abs(csa), abs(csb), worst) < bound, line


@pytest.mark.parametrize("p", [0.1, 0.25])
def test_ln_mask_statistics(p):
    W = 2048
    rows = N_STAT // W
    k, k1 = D.ln_keep(rows, W, p, SEED), D.ln_keep(rows, W, p, SEED + 1)
    assert k.size == N_STAT
    dev, ok = _rate_ok(k, p)
    cpair, cseed = _corr(k[:, 0::2], k[:, 1::2]), _corr(k, k1)
    line = "ln p=%g: rate %+.1e corr(even,odd) %+.1e corr(seed,seed+1) %+.1e" % (p, dev, cpair, cseed)
    print(line)
    assert ok, line
    assert max(abs(cpair), abs(cseed)) < 5.0 / np.sqrt(N_STAT), line


def test_seeds_with_the_top_bit_and_zero():
    big = 2 ** 63 + 5
    assert int(D.key(big)) == ((((big * 0x9E3779B97F4A7C15) % 2 ** 64) >> 32) ^ (big % 2 ** 32))      # Python integers: no overflow
    assert int(D.key(0)) == 0 and int(D.key(1)) == 0x9E3779B9 ^ 1
    assert len({int(D.key(s)) for s in (0, 1, big, 5, 2 ** 62 - 1)}) == 5, "the top bit reaches the key"
    ref_g, ref_l = D.gate_keep(8, 4, 0, 0.1, 1), D.ln_keep(8, 2048, 0.1, 1)
    for s in (0, big):
        g, ln = D.gate_keep(8, 4, 0, 0.1, s), D.ln_keep(8, 2048, 0.1, s)
        assert abs(_corr(g, ref_g)) < 0.05 and abs(_corr(ln, ref_l)) < 0.05           # 16384 elements: 6 sigma of an independent pair
        assert 0.85 < g.mean() < 0.95 and 0.85 < ln.mean() < 0.95


def test_high_word_enters_the_row_key():
    """Index 2^32 + i hashes under another key than index i (drop_row_key / act_row_key), in both field widths and in the LayerNorm map."""
    lo = np.arange(4096, dtype=np.uint64)
    for p in (0.1, 0.25):
        a, b = D.gate_keep_idx(lo, p, 9)[0], D.gate_keep_idx(lo + np.uint64(1 << 32), p, 9)[0]
        assert abs(_corr(a, b)) < 0.1
    W = 4096
    a, b = D.ln_keep(1, W, 0.1, 9, row0=0), D.ln_keep(1, W, 0.1, 9, row0=(1 << 32) // W)
    assert abs(_corr(a, b)) < 0.1
    assert np.array_equal(D.gate_keep(3, 2, 1, 0.3, 4, rows=[5, 6, 7]), D.gate_keep(8, 2, 1, 0.3, 4)[5:8])
    assert np.array_equal(D.ln_keep(3, 512, 0.1, 4, row0=5), D.ln_keep(8, 512, 0.1, 4)[5:8])


def _gelu_argument(inp, x):
    x = torch.from_numpy(x).double() + torch.from_numpy(inp["bias"]).double()
    mean, var = x.mean(1, keepdim=True), x.var(1, unbiased=False, keepdim=True)
    return (x - mean) / torch.sqrt(var + D.LN_EPS) * torch.from_numpy(inp["gamma"]).double() + torch.from_numpy(inp["beta"]).double()


@pytest.mark.parametrize("W,rows", sorted(set(D.LN_SHAPES + D.LN_GROUP_SHAPES)))
def test_ln_case_inputs_tell_kept_from_dropped(W, rows):
    """The inputs of the device cases, under the fp64 LayerNorm: the GELU's argument stays within +-2.5 (above the bf16 kernels' cut at
    -4) and is never zero, so the fp64 y has no exact zero and `y != 0` recovers a hash call's mask -- as fp32 values and rounded to bf16."""
    inp = D.ln_case_inputs(W, rows)
    for x in (inp["x"], torch.from_numpy(inp["x"]).to(torch.bfloat16).float().numpy()):
        arg = _gelu_argument(inp, x)
        assert float(arg.abs().max()) <= 2.5, float(arg.abs().max())
        assert int((arg == 0).sum()) == 0
        assert int((torch.nn.functional.gelu(arg) == 0).sum()) == 0
