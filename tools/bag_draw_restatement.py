"""numpy restatement of the draw of csrc/bag_sample.hip (host only, no GPU): the same hashes, the same three paths, vectorised over
K output rows with key_id = arange(K), and the statistics of tests/test_store_gpu.py over them.  For judging a change of the round
count, the round function or the row keys before it goes near a device:

    python tools/bag_draw_restatement.py [--rounds 6] [--seed 1234] [--counter 7]

Prints every statistic with its degrees of freedom and the 1e-6 chi-square bound (Wilson-Hilferty)."""
import argparse

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
WAVE = 64


def mix32(x):
    x = x & M32
    x ^= x >> np.uint64(16)
    x = ((x & np.uint64(0xFFFFFF)) * np.uint64(0x58E58A) + x) & M32
    x ^= x >> np.uint64(13)
    x = ((x & np.uint64(0xFFFFFF)) * np.uint64(0xCA6D40) + x) & M32
    x ^= x >> np.uint64(16)
    return x


def row_key(seed, counter, key_id):
    key_id = np.asarray(key_id, dtype=np.uint64)
    words = [np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32), np.uint64(counter & 0xFFFFFFFF), np.uint64(counter >> 32),
             key_id & M32, key_id >> np.uint64(32)]
    a = np.full(key_id.shape, 0x243F6A88, dtype=np.uint64)
    b = np.full(key_id.shape, 0x85A308D3, dtype=np.uint64)
    for w in words:
        a = (mix32(a ^ w) + np.uint64(0x9E3779B9)) & M32
        b = mix32((b + w) & M32) ^ np.uint64(0x7F4A7C15)
    a = mix32(a)
    b = mix32(b ^ a)
    return a, b


def token_hash(t, a, b):
    return mix32((mix32(t ^ a) + b) & M32)


def feistel(x, half, a, b, rounds):
    mask = np.uint64((1 << half) - 1)
    L, R = x >> np.uint64(half), x & mask
    for i in range(rounds):
        rk = (a + np.uint64((i * 0x9E3779B9) & 0xFFFFFFFF)) & M32
        f = token_hash(R, rk, b) & mask
        L, R = R, L ^ f
    return (L << np.uint64(half)) | R


def draw(n, N, K, seed=1234, counter=7, rounds=6):
    """idx [K, N]: the bag rows the kernel picks for K output rows over one bag of n rows, key_id = arange(K)."""
    a, b = row_key(seed, counter, np.arange(K))
    a, b = a[:, None], b[:, None]
    if n < N:
        t = np.arange(N, dtype=np.uint64)[None, :]
        return ((token_hash(t, a, b) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)
    if n <= WAVE:
        h = token_hash(np.arange(n, dtype=np.uint64)[None, :], a, b)
        return np.argsort(h, axis=1, kind="stable")[:, :N].astype(np.int64)     # position = rank, ties by index
    bits = int(n - 1).bit_length()
    bits += bits & 1
    y = np.broadcast_to(np.arange(N, dtype=np.uint64)[None, :], (K, N)).copy()
    todo = np.ones(y.shape, dtype=bool)
    while todo.any():
        y[todo] = feistel(y[todo], bits // 2, np.broadcast_to(a, y.shape)[todo], np.broadcast_to(b, y.shape)[todo], rounds)
        todo &= y >= np.uint64(n)
    return y.astype(np.int64)


def chi2_bound(df, z=4.75):
    """Upper 1e-6 quantile of chi-square(df), Wilson-Hilferty."""
    return df * (1 - 2 / (9 * df) + z * np.sqrt(2 / (9 * df))) ** 3


def chi2_uniform(values, cells):
    c = np.bincount(values, minlength=cells).astype(np.float64)
    e = c.sum() / cells
    return float(((c - e) ** 2 / e).sum())


def stats_without_replacement(idx, n):
    K, N = idx.shape
    out = {}
    if N < n:
        q = N / n
        c = np.bincount(idx.reshape(-1), minlength=n).astype(np.float64)
        out["inclusion"] = (float(((c - K * q) ** 2).sum() / (K * q * (1 - q)) * (n - 1) / n), n - 1)
    out["position0"] = (chi2_uniform(idx[:, 0], n), n - 1)
    if N > 1:
        out["difference"] = (chi2_uniform((idx[:, 1] - idx[:, 0]) % n - 1, n - 1), n - 2)
    return out


def stats_with_replacement(idx, n):
    flat = idx.reshape(-1)
    pairs = (idx[:, 0::2] * n + idx[:, 1::2]).reshape(-1)      # disjoint pairs: independent cells, a plain chi-square
    return {"single": (chi2_uniform(flat, n), n - 1), "pairs": (chi2_uniform(pairs, n * n), n * n - 1)}


SHAPES = [(5, 3, 200000), (17, 16, 200000), (64, 33, 200000), (65, 64, 20000), (257, 256, 20000), (1000, 256, 20000),
          (1025, 64, 40000)]

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--counter", type=int, default=7)
    a = ap.parse_args()
    for n, N, K in SHAPES:
        idx = draw(n, N, K, a.seed, a.counter, a.rounds)
        assert idx.min() >= 0 and idx.max() < n and all(len(set(r)) == N for r in idx[:200])
        for name, (x, df) in stats_without_replacement(idx, n).items():
            print("n=%5d N=%4d K=%6d %-10s %9.1f  df %5d  bound %8.1f  %s" % (n, N, K, name, x, df, chi2_bound(df),
                                                                             "ok" if x <= chi2_bound(df) else "FAIL"))
    n, N, K = 3, 64, 200000
    for name, (x, df) in stats_with_replacement(draw(n, N, K, a.seed, a.counter, a.rounds), n).items():
        print("n=%5d N=%4d K=%6d %-10s %9.1f  df %5d  bound %8.1f  %s" % (n, N, K, name, x, df, chi2_bound(df),
                                                                         "ok" if x <= chi2_bound(df) else "FAIL"))
