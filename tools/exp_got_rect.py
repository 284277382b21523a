"""GOT between token sets of different sizes (functional.got_tiled with V [k, n, d], Q [k, m, d]) on the GPU, two measurements:

    python tools/exp_got_rect.py [--shapes 4x1024x512x128,1x4096x1024x128,1x512x4096x128] [--reps 20]
        forward + backward time (device events, one warm-up call, the two implementations alternating) and peak device memory of the
        HIP path and of a torch fp32 restatement of the reference algorithm (madeleine/utils/loss.py:278-302: bmm products, autograd
        through every IPOT iteration), the only alternative a user has for n != m.

    python tools/exp_got_rect.py --ab OLD.so [--square 4x1024x128,1x4096x128] [--bits 2x513x128,3x1024x128,1x4096x128] [--reps 20]
        the square shapes through the six mdl_got_tiled_* entry points of two builds of the library (OLD.so against this tree's),
        raw C ABI: bit identity of value, extrema, dV and dQ, and forward + backward times with OLD, NEW and OLD again alternating
        in one call (OLD against OLD shows the spread that NEW is read against).

Prints one JSON line per shape and implementation."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def torch_got(v, q):
    from tests.test_got_tiled_gpu import got_parts64   # the restatement is dtype-agnostic: run in fp32 here
    return got_parts64(v, q).sum()


def once(fn, v, q):
    """(forward + backward ms, peak bytes above the inputs) of one call."""
    dev = v.device
    vd, qd = v.clone().requires_grad_(), q.clone().requires_grad_()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn(vd, qd).backward()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), torch.cuda.max_memory_allocated(dev) - base


def stats(ts):
    return {"min_ms": round(min(ts), 3), "median_ms": round(statistics.median(ts), 3), "max_ms": round(max(ts), 3), "reps": len(ts)}


def rect(a):
    from madeleine_amd import functional as MF
    dev = torch.device("cuda:0")
    impls = [("hip", lambda x, y: MF.got_tiled(x, y).sum()), ("torch_fp32", torch_got)]
    for sh in a.shapes.split(","):
        k, n, m, d = (int(x) for x in sh.split("x"))
        g = torch.Generator(device=dev).manual_seed(0)
        v = torch.rand(k, n, d, device=dev, generator=g) * 2 - 1
        q = torch.rand(k, m, d, device=dev, generator=g) * 2 - 1 + 0.7 * v[:, torch.arange(m, device=dev) % n]
        times, peaks = {name: [] for name, _ in impls}, {}
        for r in range(a.reps + 1):
            for name, fn in impls:      # alternating; r == 0 warms up
                ms, peak = once(fn, v, q)
                if name == "torch_fp32":
                    torch.cuda.empty_cache()     # its autograd tape would otherwise stay cached under the other's workspace
                if r:
                    times[name].append(ms)
                peaks[name] = max(peaks.get(name, 0), peak)
        for name, _ in impls:
            print(json.dumps({"impl": name, "k": k, "n": n, "m": m, "d": d, **stats(times[name]),
                              "peak_gb": round(peaks[name] / 2 ** 30, 3)}), flush=True)
        h, t = statistics.median(times["hip"]), statistics.median(times["torch_fp32"])
        print(json.dumps({"shape": sh, "torch_over_hip": round(t / h, 3),
                          "peak_torch_over_hip": round(peaks["torch_fp32"] / peaks["hip"], 3)}), flush=True)


def load(path):
    from madeleine_amd import _native
    L = ctypes.CDLL(path)
    for name, (res, args) in _native.SIGNATURES.items():
        if name.startswith("mdl_got_tiled") and hasattr(L, name):
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
    return L


def call(L, v, q, ws, timed=True):
    k, n, d = v.shape
    dev = v.device
    out, mm = torch.empty(2, device=dev), torch.empty(6, device=dev)
    dv, dq, go = torch.empty_like(v), torch.empty_like(q), torch.ones(2, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    rc = L.mdl_got_tiled_fwd(v.data_ptr(), q.data_ptr(), out.data_ptr(), mm.data_ptr(), None, k, n, d, ws.data_ptr(), st)
    assert rc == 0, rc
    rc = L.mdl_got_tiled_bwd(v.data_ptr(), q.data_ptr(), go.data_ptr(), dv.data_ptr(), dq.data_ptr(), k, n, d, ws.data_ptr(), st)
    assert rc == 0, rc
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), (out, mm, dv, dq)


def ab(a):
    from madeleine_amd import _native
    dev = torch.device("cuda:0")
    old, new = load(a.ab), load(_native.lib_path())

    def data(sh):
        k, n, d = (int(x) for x in sh.split("x"))
        g = torch.Generator(device=dev).manual_seed(k * 10000 + n)
        v = torch.rand(k, n, d, device=dev, generator=g) * 2 - 1
        q = torch.rand(k, n, d, device=dev, generator=g) * 2 - 1 + 0.7 * v
        nb = new.mdl_got_tiled_ws_bytes(k, n, d)
        assert nb == old.mdl_got_tiled_ws_bytes(k, n, d), "workspace sizes differ"
        return v, q, torch.empty(nb, dtype=torch.uint8, device=dev)

    for sh in a.bits.split(","):
        v, q, ws = data(sh)
        _, ro = call(old, v, q, ws)
        ws.fill_(0xff)      # the second build starts from a workspace that holds none of the first one's results
        _, rn = call(new, v, q, ws)
        same = [bool(torch.equal(x, y)) for x, y in zip(ro, rn)]
        print(json.dumps({"bits": sh, "value": same[0], "extrema": same[1], "dV": same[2], "dQ": same[3],
                          "wd": float(rn[0][0]), "gwd": float(rn[0][1])}), flush=True)
        del v, q, ws
        torch.cuda.empty_cache()
    for sh in a.square.split(","):
        v, q, ws = data(sh)
        runs = [("old", old), ("new", new), ("old_again", old)]
        times = {name: [] for name, _ in runs}
        for r in range(a.reps + 1):
            for name, L in runs:
                ms, _ = call(L, v, q, ws)
                if r:
                    times[name].append(ms)
        for name, _ in runs:
            print(json.dumps({"square": sh, "lib": name, **stats(times[name])}), flush=True)
        del v, q, ws
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4x1024x512x128,1x4096x1024x128,1x512x4096x128")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ab", default=None, help="an older build of libmadeleine_amd.so to compare the square shapes against")
    ap.add_argument("--square", default="4x1024x128,1x4096x128")
    ap.add_argument("--bits", default="2x513x128,3x1024x128,1x4096x128")
    a = ap.parse_args()
    ab(a) if a.ab else rect(a)


if __name__ == "__main__":
    main()
