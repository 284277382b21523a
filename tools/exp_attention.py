"""Measures the attention read-out of the slide store on the shape of `exp_store.py --embed`: --cases H&E bags
of --rows rows x 512, fp32 store, fp32 model.  Device events after warm-up, the legs alternated inside one process.

  1. DeviceSlideStore.attention(topk=16) against DeviceSlideStore.embed over the same cohort: bags/s of both.
  2. The softmax and the rank launch sequences alone (functional.attn_softmax, functional.attn_rank with percentile ranks and top-16) on
     the raw scores of leg 1, against a torch loop on the same scores: per bag torch.softmax, per bag and head a stable descending
     argsort, ranks by scatter, top-16 by slicing.  (The loop's ranks are ordinal, not tie-averaged: it does less.)
  3. The launches per call of the two sequences.

       python tools/exp_attention.py [--cases 48] [--rows 30000] [--steps 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench as BN  # noqa: E402
from madeleine_amd import MADELEINE, DeviceSlideStore  # noqa: E402
from madeleine_amd import functional as MF  # noqa: E402


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def timed(f):
    """device milliseconds of f() between two events on the current stream"""
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    out = f()
    ev1.record()
    ev1.synchronize()
    del out
    return ev0.elapsed_time(ev1)


def torch_loop(raw, cu_host, k):
    """what a user writes today: per bag the softmax, per bag and head a stable sort, ordinal ranks by scatter, the k best"""
    T, H = raw.shape
    attn = torch.empty_like(raw)
    order = torch.empty(H, T, dtype=torch.int64, device=raw.device)
    pct = torch.empty_like(raw)
    R = len(cu_host) - 1
    top = torch.full((R, H, k), -1, dtype=torch.int64, device=raw.device)
    for r in range(R):
        a, b = cu_host[r], cu_host[r + 1]
        n = b - a
        attn[a:b] = torch.softmax(raw[a:b], 0)
        steps = torch.arange(1, n + 1, device=raw.device, dtype=torch.float32)
        for h in range(H):
            o = torch.argsort(raw[a:b, h], descending=True, stable=True)
            order[h, a:b] = o
            pct[a:b, h].scatter_(0, o, (n + 1 - steps) * (100.0 / n))
            top[r, h, :min(k, n)] = o[:k]
    return attn, order, pct, top


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=48)
    ap.add_argument("--rows", type=int, default=30000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--topk", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n, rows, D, k = a.cases, a.rows, 512, a.topk
    g = torch.Generator().manual_seed(7)
    base = torch.randn(rows + n, D, generator=g)
    bags = [[base[c:c + rows]] for c in range(n)]        # overlapping windows of one tensor: distinct bags, one host allocation
    st = DeviceSlideStore(bags, ["case%05d" % c for c in range(n)], ["HE"], dev)
    torch.manual_seed(42)
    model = MADELEINE(BN.make_cfg(2, D)).to(dev).eval()
    res = {"geometry": {"cases": n, "rows_per_bag": rows, "D": D, "topk": k}}
    lines = []

    # ---- 1. the whole read-out against the embeddings alone
    feeds = {"attention": lambda: st.attention(model, topk=k), "embed": lambda: st.embed(model)}
    for f in feeds.values():
        f()
    ms = {name: [] for name in feeds}
    for i in range(max(1, a.steps)):
        for name in (sorted(feeds) if i % 2 == 0 else sorted(feeds, reverse=True)):
            ms[name].append(timed(feeds[name]))
    res["store"] = {name: {"ms": stats(v), "bags_per_s_median": n / statistics.median(v) * 1e3} for name, v in ms.items()}
    for name, v in sorted(ms.items()):
        lines.append("store.%-10s median %.1f ms = %.1f bags/s (min %.1f max %.1f ms) over %d bags of %d rows"
                     % (name, statistics.median(v), n / statistics.median(v) * 1e3, min(v), max(v), n, rows))

    # ---- 2. the two launch sequences alone against a torch loop on the same scores
    out = st.attention(model, topk=k)
    raw, cu = out["raw"], out["cu_seqlens"]
    cu_host = cu.tolist()
    H = raw.shape[1]
    legs = {"hip_softmax": lambda: MF.attn_softmax(raw, cu), "hip_rank": lambda: MF.attn_rank(raw, cu, k=k),
            "torch_loop": lambda: torch_loop(raw, cu_host, k)}
    for f in legs.values():
        f()
    ms = {name: [] for name in legs}
    for i in range(max(1, a.steps)):
        for name in (sorted(legs) if i % 2 == 0 else sorted(legs, reverse=True)):
            ms[name].append(timed(legs[name]))
    res["readout"] = {name: {"ms": stats(v)} for name, v in ms.items()}
    hip = statistics.median(ms["hip_softmax"]) + statistics.median(ms["hip_rank"])
    res["readout"]["torch_loop_over_hip"] = statistics.median(ms["torch_loop"]) / hip
    for name, v in sorted(ms.items()):
        lines.append("%-12s median %.3f ms (min %.3f max %.3f) over %d segments of %d keys" % (name, statistics.median(v), min(v), max(v),
                                                                                             n * H, rows))
    lines.append("torch loop / (hip softmax + hip rank) = %.1f x" % res["readout"]["torch_loop_over_hip"])
    # the loop and the kernels agree where both are defined (the loop's ranks are ordinal: compare the order and the softmax)
    t_attn, t_order, _, t_top = torch_loop(raw, cu_host, k)
    res["readout"]["order_equal"] = bool(torch.equal(t_order.int(), out["order"]))
    res["readout"]["topk_equal"] = bool(torch.equal(t_top.int(), out["topk_idx"]))
    res["readout"]["softmax_max_rel_diff"] = float(((t_attn - out["attention"]).abs() / t_attn).max())
    lines.append("order equal %s, top-k equal %s, softmax max relative difference %.2e"
                 % (res["readout"]["order_equal"], res["readout"]["topk_equal"], res["readout"]["softmax_max_rel_diff"]))

    # ---- 3. launches per call (header, A-map): neither depends on R or T
    res["launches"] = {"attn_softmax": 6, "attn_rank": 2 + 12 + 1 + (1 if k else 0), "torch_loop": "R * (2 + 4 H) or more"}
    lines.append("launches per call: attn_softmax 6, attn_rank %d; the torch loop at least %d" % (res["launches"]["attn_rank"], n * (2 + 4 * H)))
    for ln in lines:
        print(ln)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
