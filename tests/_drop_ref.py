"""Host model of the dropout counter hash (csrc/common.hpp:mix32, gate_common.hpp:make_drop / drop_keep2, preattn_act.hip:act_keep4),
written from its specification in plain numpy on uint64 with explicit masks -- it calls nothing of the library.  What the kernels must draw:

    mix32(x):   x ^= x >> 16;  x = lo24(x) * 0x58E58A + x;  x ^= x >> 13;  x = lo24(x) * 0xCA6D40 + x;  x ^= x >> 16      (mod 2^32)
    key(seed):  lo32((seed * 0x9E3779B97F4A7C15 mod 2^64) >> 32) ^ lo32(seed)
    thr(p):     min(65535, floor(double(float32(p)) * 65536 + 0.5))
    row key of an element index idx:  key ^ (hi32(idx) * 0x9E3779B9 mod 2^32)
    gate element idx = (t * H + c) * 512 + e:   16-bit fields: h = mix32(lo32(idx) ^ rowkey), ka = h[15:0] >= thr, kb = h[31:16] >= thr
        byte fields (thr > 0, thr % 256 == 0):  h = mix32((lo32(idx) >> 1) ^ rowkey), f = h >> 16 if idx odd else h,
                                                ka = f[7:0] >= thr >> 8, kb = f[15:8] >= thr >> 8
    LayerNorm element idx = r * W + c:  h = mix32(lo32(idx & ~1) ^ rowkey(r * W)), field = h >> 16 if idx odd else h[15:0], keep = field >= thr
"""
import functools

import numpy as np

_U = np.uint64
M24, M32, M64 = _U(0xFFFFFF), _U(0xFFFFFFFF), 0xFFFFFFFFFFFFFFFF
GOLDEN32, GOLDEN64 = _U(0x9E3779B9), 0x9E3779B97F4A7C15
HID = 512


def mix32(x):
    """x: array (or scalar) of counters below 2^32, any integer type -> uint64 array of 32-bit hashes."""
    x = np.asarray(x).astype(_U) & M32
    x = x ^ (x >> _U(16))
    x = ((x & M24) * _U(0x58E58A) + x) & M32
    x = x ^ (x >> _U(13))
    x = ((x & M24) * _U(0xCA6D40) + x) & M32
    return x ^ (x >> _U(16))


def key(seed):
    """seed: a Python int in [0, 2^64) (Python arithmetic: no signed overflow above 2^63)."""
    seed = int(seed) & M64
    return _U((((seed * GOLDEN64) & M64) >> 32) ^ (seed & 0xFFFFFFFF))


def thr(p):
    return int(min(65535.0, np.floor(float(np.float32(p)) * 65536.0 + 0.5)))


def inv(p):
    return np.float32(1) / (np.float32(1) - np.float32(p))


def row_key(k, idx):
    """idx: uint64 array of element indices."""
    return k ^ (((idx >> _U(32)) * GOLDEN32) & M32)


def gate_keep_idx(idx, p, seed, force16=False):
    """(ka, kb) uint8 of the gate elements `idx` (uint64 array)."""
    idx = np.asarray(idx).astype(_U)
    t, rk = thr(p), row_key(key(seed), idx)
    if t > 0 and t % 256 == 0 and not force16:
        h = mix32(((idx & M32) >> _U(1)) ^ rk)
        f = np.where((idx & _U(1)) != 0, h >> _U(16), h)
        ka, kb = (f & _U(0xFF)) >= _U(t >> 8), ((f >> _U(8)) & _U(0xFF)) >= _U(t >> 8)
    else:
        h = mix32((idx & M32) ^ rk)
        ka, kb = (h & _U(0xFFFF)) >= _U(t), (h >> _U(16)) >= _U(t)
    return ka.astype(np.uint8), kb.astype(np.uint8)


def gate_keep(T, H, which, p, seed, force16=False, rows=None):
    """uint8 [T, H, 512] (or [len(rows), H, 512] of the token rows `rows`): keep_a (which = 0) or keep_b (which = 1)."""
    t = np.arange(T, dtype=_U) if rows is None else np.asarray(rows).astype(_U)
    idx = ((t[:, None, None] * _U(H) + np.arange(H, dtype=_U)[None, :, None]) * _U(HID) + np.arange(HID, dtype=_U)[None, None, :])
    return gate_keep_idx(idx, p, seed, force16)[which]


@functools.lru_cache(maxsize=2)
def _ln_field(rows, W, seed, row0):
    """uint16 [rows, W]: the 16-bit field of every element (W is even, so the pair (idx & ~1, idx | 1) lies in one row: one hash each)."""
    r = np.arange(row0, row0 + rows, dtype=_U)[:, None]
    even = r * _U(W) + np.arange(0, W, 2, dtype=_U)[None, :]
    h = mix32((even & M32) ^ row_key(key(seed), r * _U(W)))
    field = np.empty((rows, W), dtype=np.uint16)
    field[:, 0::2] = h & _U(0xFFFF)
    field[:, 1::2] = h >> _U(16)
    return field


def ln_keep(rows, W, p, seed, row0=0):
    """uint8 [rows, W]: the keep mask of rows [row0, row0 + rows) of a LayerNorm-GELU-Dropout call of width W."""
    return (_ln_field(int(rows), int(W), int(seed), int(row0)) >= thr(p)).astype(np.uint8)


# ---- inputs of the LayerNorm cases (tests/test_dropout_hash_gpu.py (c), (d)) -------------------------------------------------------
LN_SHAPES = [(W, rows) for W in (256, 512, 1024, 2048, 4096) for rows in (1, 7)] + [(256, 8197), (2048, 8197)]
LN_GROUP_SHAPES = [(W, rows) for W in (256, 512, 1024) for rows in (1, 7, 19)] + [(256, 8197)]
LN_EPS = 1e-5


def ln_case_inputs(W, rows):
    """float32 numpy x, dy [rows, W], bias, gamma, beta [W]: every row of x is a shuffled, jittered grid over (-1, 1) -- uniform, with a
    row mean and variance that do not depend on the draw -- gamma = 1, beta = 0.5 and a small bias row, so that the argument of the GELU
    stays within +-2.5 (sqrt(3) + 0.5 plus the bias) and is never exactly zero: y != 0 then tells a kept element from a dropped one."""
    rng = np.random.default_rng(1000 * W + rows)
    grid = (np.arange(W) + 0.5) / W * 2.0 - 1.0
    x = rng.permuted(np.tile(grid, (rows, 1)), axis=1) + rng.uniform(-0.4 / W, 0.4 / W, (rows, W))
    return dict(x=np.ascontiguousarray(x, dtype=np.float32), dy=rng.standard_normal((rows, W)).astype(np.float32),
                bias=rng.uniform(-0.05, 0.05, W).astype(np.float32), gamma=np.ones(W, np.float32), beta=np.full(W, 0.5, np.float32))


def ln_case_groups(rows):
    """[0, 5, 5, 19]-style row offsets of three groups, the middle one empty."""
    return [0, max(1, (rows * 5) // 19), max(1, (rows * 5) // 19), rows]
