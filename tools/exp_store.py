#!/usr/bin/env python
"""What does the device-resident slide store buy?  Two measurements on config 2's geometry (32 cases x 2 stains, bags of --rows rows
x 512 fp32, N = 4096 tokens per bag), both with device events:

  1. the gather kernel alone: median / min / max of --launches launches of DeviceSlideStore.sample over the whole cohort, as achieved
     bytes/s over the algorithmic payload (read + write of R * N * D elements: 8 B per element from an fp32 store, 6 B from a 16-bit
     one), next to a device-to-device copy of the same payload by torch (tools/micro/hbm_rate gives the box's copy ceiling);
  2. the pretrain step fed four ways, --steps timed steps each in alternating rounds of --round-steps; one phase per host-fed path
     (that path, the store and the constant batch alternate while only that path's DataLoader workers are alive; before each of its
     timed rounds the host-fed path runs workers + 6 untimed steps, which use up the batches prefetched while the other feeds ran):
       h5      DataLoader(SlideDataset(sample=N) over one h5 file per stain, collate) + DevicePrefetcher: the host-fed path as it stands
       host    the same with the bags held in host memory (no file is read, nothing is parsed: the host path at its best)
       store   DeviceSlideStore.batches
       const   one constant device-resident batch (what bench.py times)
     median / min / max per step, and the two differences the store is judged by.

--pack runs the packed ragged route instead, at one rank of config 5's shape (32 cases x 5 stains, bag lengths U{1024..16384}, D = 768,
stain-encoding tokens), with device events after warm-up:
  3. the pack kernel: DeviceSlideStore.pack of the whole cohort, every bag whole (contiguous reads) and cut to --cap rows (drawn rows),
     next to DeviceSlideStore.sample of N = 8192 tokens per bag (bags shorter than that are drawn with replacement) and of N = 1024
     (every row distinct) from the same store in the same loop, as achieved bytes/s over T * D * (4 + element size), for an fp32 and
     a bf16 store;
  4. the path pack replaces, for the same batch on the fp32 store: the torch.cat of the 160 bag views plus the host-built per-token
     bag map and its upload, against pack -- both by the host clock around a device synchronise (they differ in host work), and the
     cat alone by device events;
  5. the config-5 training step (InfoNCE + GOT, stain encoding) fed by packed_batches against the same step fed by ragged_batches on
     the fp32 store, in alternating rounds.

--tier measures the two-tier store (rows partly or wholly in pinned host memory, read over PCIe by the gather's narrow persistent grid) on
config 2's geometry, over --tier-cases cases x 2 stains of --tier-rows rows (an epoch of several batches, so that prefetch has a next
batch to fetch), with device events after warm-up, medians (min-max), the legs alternating inside one loop:
  6. the link: a pinned-to-device copy_ of one batch's payload (contiguous; the box's PCIe rate) next to the gather of a whole batch from
     an all-host fp32 store and from an all-host bf16 store, for host_wgs in {8, 16, 32, 64, 128, 256} and one workgroup per item
     (chip-wide); rate = payload read over PCIe / time.  And, by the host clock, what a tiered call costs the host per launch.
  7. the config-2 step fed by (a) the resident store, (b) the all-host fp32 store with prefetch=1, (c) the same with prefetch=0,
     (d) a store with half its bytes resident, prefetch=1 -- alternating rounds; every round is one epoch whose first step is run
     untimed (it fills the prefetch queue) -- and (e) the `host` DataLoader feed in a phase of its own, next to (a) and (b).

--embed measures the route from the store to one vector per slide, over --embed-cases H&E bags of --embed-rows rows x 512, with device
events after warm-up, medians (min-max), the legs alternating inside one loop:
  8. the mean kernel: functional.bag_mean of the whole cohort on prepared tables (its two launches, nothing else) from a resident fp32
     and a resident bf16 store, as achieved bytes/s over the rows read (T * D * element size; the partial sums and the output are
     0.1 % of that), next to DeviceSlideStore.sample of N = 4096 tokens per bag from the same store (bytes/s over its read + write
     payload, as in 1.) and to the whole DeviceSlideStore.mean_embeddings call (plan, table upload and launches: the host's share
     shows as the difference); tools/micro/hbm_rate gives the box's read ceiling for the contiguous pattern;
  9. extraction: DeviceSlideStore.embed of the cohort (fp32 store, fp32 model, its default 4 bags per launch set) against
     utils.run_inference over a DataLoader that hands over the same bags from host memory one at a time (pinned, no file is read: the
     host path at its best), both in bags/s by the host clock around a device synchronise, alternating.

Usage: python tools/exp_store.py [--rows 20000] [--launches 20] [--steps 20] [--round-steps 5] [--workers 6] [--out FILE]
       python tools/exp_store.py --pack [--launches 20] [--steps 12] [--round-steps 3] [--cap 4096] [--skip-step] [--out FILE]
       python tools/exp_store.py --tier [--tier-cases 192] [--tier-rows 4096] [--launches 10] [--steps 20] [--round-steps 5] [--out FILE]
       python tools/exp_store.py --embed [--embed-cases 48] [--embed-rows 30000] [--launches 10] [--steps 4] [--out FILE]"""
import argparse
import json
import os
import shutil
import statistics
import sys
import time
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench as BN  # noqa: E402
from madeleine_amd import MADELEINE, DeviceSlideStore, InfoNCE, calculate_losses  # noqa: E402
from madeleine_amd import functional as MF  # noqa: E402
from madeleine_amd.data import DevicePrefetcher, collate  # noqa: E402


class HostCohort(torch.utils.data.Dataset):
    """SlideDataset's item over bags held in host memory (no file is read), `repeat` epochs long so that one DataLoader pass covers
    every timed step."""

    def __init__(self, bags, n_tokens, repeat):
        self.bags, self.N, self.repeat = bags, n_tokens, repeat

    def __len__(self):
        return len(self.bags) * self.repeat

    def __getitem__(self, i):
        case = self.bags[i % len(self.bags)]
        feats = []
        for f in case:                                   # SlideDataset.sample_n
            idx = torch.randint(0, f.shape[0], (self.N,)) if f.shape[0] < self.N else torch.randperm(f.shape[0])[:self.N]
            feats.append(f[idx])
        return {'feats': feats, 'modality_labels': [1] * len(case), 'slide_id': "case%05d" % (i % len(self.bags))}


def h5_feed(bags, ids, mods, N, D, B, batches, workers, dev, h5_dir):
    """The parent's input side as it stands: the cohort as one h5 file per stain, SlideDataset(sample=N) re-reading every file for
    every item (load_features), DataLoader workers, collate, DevicePrefetcher."""
    import tempfile

    import pandas as pd
    from madeleine_amd import h5io
    from madeleine_amd.data import SlideDataset
    root = tempfile.mkdtemp(prefix="exp_store_", dir=h5_dir)
    for sid, case in zip(ids, bags):
        for m, f in zip(mods, case):
            h5io.write_datasets(os.path.join(root, "%s_%s.h5" % (sid, m)), {"features": f.numpy()})
    frame = {"slide_id": ids, "split": ["train"] * len(ids)}
    frame.update({m: [1] * len(ids) for m in mods})
    df = pd.concat([pd.DataFrame(frame)] * batches, ignore_index=True)
    ds = SlideDataset("synthetic", None, root, mods, embedding_size=D, sample=N, train=True, dataframe=df)
    loader = torch.utils.data.DataLoader(ds, batch_size=B, shuffle=False, collate_fn=collate, num_workers=workers, pin_memory=True,
                                         prefetch_factor=1 if workers else None)
    return iter(DevicePrefetcher(loader, dev, depth=2)), root


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def pack_leg(a, dev):
    """Measurements 3-5 of the module docstring.  Returns (lines, results)."""
    B, M, _N, D, _got, stain = BN.CONFIGS["c5"]
    mods = BN.MODS5[:M]
    lens = torch.randint(1024, 16385, (B, M), generator=torch.Generator().manual_seed(4321))       # bench.py's config-5 lengths
    base = torch.randn(16384, D, generator=torch.Generator().manual_seed(7))
    bags = [[base[:int(lens[b, m])] * (1.0 + 0.01 * (b * M + m)) for m in range(M)] for b in range(B)]
    ids = ["case%05d" % i for i in range(B)]
    cases, R, T = list(range(B)), B * M, int(lens.sum())
    n_dense = 8192
    lines, res = [], {"geometry": {"cases": B, "stains": M, "rows": T, "D": D, "lengths": "U{1024..16384}", "cap": a.cap,
                                   "dense_tokens": n_dense}}

    # ---- 3. the kernel
    res["kernel"] = {}
    for dtype in (torch.float32, torch.bfloat16):
        st = DeviceSlideStore(bags, ids, mods, dev, dtype=dtype)
        esz = st.rows.element_size()
        T_cap = sum(st.pack_lens(cases, a.cap))
        # sample at N = 8192 redraws rows of the bags shorter than that (with replacement: repeats are served by the caches, not by HBM);
        # sample_distinct at N = 1024, the shortest possible bag, reads every row once, as the packs do
        work = {"pack_whole": T * D * (4 + esz), "pack_capped": T_cap * D * (4 + esz), "sample": R * n_dense * D * (4 + esz),
                "sample_distinct": R * 1024 * D * (4 + esz)}
        calls = {"pack_whole": lambda i: st.pack(cases, None, counter=i), "pack_capped": lambda i: st.pack(cases, a.cap, counter=i),
                 "sample": lambda i: st.sample(cases, n_dense, counter=i), "sample_distinct": lambda i: st.sample(cases, 1024, counter=i)}
        for f in calls.values():
            for i in range(3):
                f(i)
        times = {k: [] for k in calls}
        for i in range(a.launches):
            order = sorted(calls) if i % 2 == 0 else sorted(calls, reverse=True)
            for k in ("pack_whole", "sample"):           # untimed, ~3 ms of device work: the host runs ahead of the device, so the
                del_me = calls[k](50 + i)                # first timed call of the sequence holds no launch gap either
                del del_me
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(order) + 1)]
            ev[0].record()
            for j, k in enumerate(order):
                out = calls[k](100 + i)
                ev[j + 1].record()
                del out
            ev[-1].synchronize()
            for j, k in enumerate(order):
                times[k].append(ev[j].elapsed_time(ev[j + 1]))
        res["kernel"][str(dtype)] = {k: {"ms": stats(v), "payload_bytes": work[k], "TBps_median": work[k] / statistics.median(v) * 1e-9}
                                     for k, v in times.items()}
        for k, v in sorted(times.items()):
            lines.append("%-12s %-14s median %.3f ms (min %.3f max %.3f) = %.2f TB/s over %.2f GB"
                         % (k, str(dtype), statistics.median(v), min(v), max(v), work[k] / statistics.median(v) * 1e-9, work[k] * 1e-9))
        r = res["kernel"][str(dtype)]
        r["pack_whole_over_sample"] = r["pack_whole"]["TBps_median"] / r["sample"]["TBps_median"]
        r["pack_whole_over_sample_distinct"] = r["pack_whole"]["TBps_median"] / r["sample_distinct"]["TBps_median"]
        lines.append("  pack_whole / sample = %.3f, pack_whole / sample_distinct = %.3f (bytes/s, same run)"
                     % (r["pack_whole_over_sample"], r["pack_whole_over_sample_distinct"]))
        if dtype == torch.float32:
            st32 = st
    st = st32

    # ---- 4. the path pack replaces: torch.cat of the views + the per-token bag map built on the host and uploaded
    def parent_path():
        views = [st.bag_view(c, m) for c in cases for m in range(M)]
        x = torch.cat(views, dim=0)
        n = torch.tensor([int(v.shape[0]) for v in views])
        return x, MF.h2d(torch.repeat_interleave(torch.arange(R, dtype=torch.int32), n), dev)

    def host_clock(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        del out
        return (t1 - t0) * 1e3
    for _ in range(3):
        parent_path()
        st.pack(cases)
    wall = {"cat_and_row_map": [], "pack": []}
    for i in range(a.launches):
        for k, f in (("cat_and_row_map", parent_path), ("pack", lambda: st.pack(cases, None, counter=i))):
            wall[k].append(host_clock(f))
    cat_ms = []
    views = [st.bag_view(c, m) for c in cases for m in range(M)]
    for i in range(a.launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        x = torch.cat(views, dim=0)
        e1.record()
        e1.synchronize()
        cat_ms.append(e0.elapsed_time(e1))
        del x
    res["parent_path"] = {"host_clock_ms": {k: stats(v) for k, v in wall.items()}, "cat_device_ms": stats(cat_ms),
                          "row_map_upload_bytes": 4 * T, "pack_upload_bytes": 8 * (2 * (R + 1) + (R + 1) // 2)}
    for k, v in sorted(wall.items()):
        lines.append("host clock around a synchronise, %-16s median %.3f ms (min %.3f max %.3f)" % (k, statistics.median(v), min(v), max(v)))
    lines.append("torch.cat of the %d views alone, device events: median %.3f ms (min %.3f max %.3f); uploads per step: %d B (row map) against %d B (pack)"
                 % (R, statistics.median(cat_ms), min(cat_ms), max(cat_ms), 4 * T, res["parent_path"]["pack_upload_bytes"]))

    # ---- 5. the config-5 step
    if not a.skip_step:
        from madeleine_amd import GOT
        torch.manual_seed(42)
        model = MADELEINE(BN.make_cfg(M, D), stain_encoding=stain).to(dev).train()
        opt = torch.optim.AdamW(model.parameters(), lr=1e-4, fused=True)
        crit = InfoNCE(temperature=0.001)
        largs = SimpleNamespace(global_loss="info-nce", symmetric_cl=True, local_loss_weight=1.0)

        def step(data):
            opt.zero_grad(set_to_none=True)
            embs, toks = model(data, device=dev)
            loss, _ = calculate_losses(mods[1:], crit, GOT, None, embs, toks, data["modality_labels"][:, 1:], largs)
            loss.backward()
            opt.step()
        feeds = {"ragged": st.ragged_batches(B, shuffle=True, seed=1), "packed": st.packed_batches(B, None, shuffle=True, seed=1),
                 "packed_cap": st.packed_batches(B, a.cap, shuffle=True, seed=1)}
        epoch = [0]

        def batch(k):
            feeds[k].set_epoch(epoch[0])
            epoch[0] += 1
            return next(iter(feeds[k]))
        for k in feeds:
            for _ in range(a.warmup):
                step(batch(k))
        rounds = max(1, a.steps // a.round_steps)
        times = {k: [] for k in feeds}
        for r in range(rounds):
            for k in (sorted(feeds) if r % 2 == 0 else sorted(feeds, reverse=True)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(a.round_steps):
                    step(batch(k))
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) / a.round_steps)
        res["step"] = {"rounds": rounds, "steps_per_round": a.round_steps, "step_ms": {k: stats(v) for k, v in times.items()},
                       "rounds_ms": times, "packed_minus_ragged_ms": statistics.median(times["packed"]) - statistics.median(times["ragged"])}
        for k, v in sorted(times.items()):
            lines.append("config-5 step fed by %-10s median %.3f ms  min %.3f  max %.3f   rounds: %s"
                         % (k, statistics.median(v), min(v), max(v), " ".join("%.3f" % x for x in v)))
        lines.append("  packed - ragged = %.3f ms" % res["step"]["packed_minus_ragged_ms"])
    return lines, res


def tier_leg(a, dev):
    """Measurements 6-7 of the module docstring.  Returns (lines, results)."""
    B, M, N, D, _got, stain = BN.CONFIGS["c2"]
    mods = BN.MODS5[:M]
    n_cases = a.tier_cases
    g = torch.Generator().manual_seed(7)
    bags = [[torch.randn(a.tier_rows, D, generator=g) for _ in range(M)] for _ in range(n_cases)]
    ids = ["case%05d" % i for i in range(n_cases)]
    cases = list(range(B))
    lines, res = [], {"geometry": {"cases": n_cases, "stains": M, "rows_per_bag": a.tier_rows, "D": D, "N": N, "batch": B}}
    fmt = lambda v: "%.3f ms (%.3f-%.3f)" % (statistics.median(v), min(v), max(v))      # noqa: E731

    # ---- 6. the link
    res["link"] = {}
    wgs_list = [8, 16, 32, 64, 128, 256, 1 << 30]                # the last: cut to the items, one workgroup per item (chip-wide)
    for dtype in (torch.float32, torch.bfloat16):
        st = DeviceSlideStore(bags, ids, mods, dev, dtype=dtype, resident_bytes=0)
        esz = st.rows_host.element_size()
        payload = B * M * N * D * esz                            # bytes read over PCIe per batch
        src = torch.empty(B * M * N * D, dtype=dtype).pin_memory()
        dst = torch.empty(B * M * N * D, dtype=dtype, device=dev)
        legs = {"copy": lambda i: dst.copy_(src, non_blocking=True)}
        for w in wgs_list:
            legs["wgs%d" % w if w < 1 << 30 else "chip_wide"] = lambda i, w=w: st.sample(cases, N, counter=i, host_wgs=w)
        for f in legs.values():
            for i in range(2):
                f(i)
        times = {k: [] for k in legs}
        names = list(legs)
        for i in range(a.launches):
            for k in (names if i % 2 == 0 else names[::-1]):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = legs[k](100 + i)
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1))
                del out
        r = {k: {"ms": stats(v), "GBps_median": payload / statistics.median(v) * 1e-6} for k, v in times.items()}
        grids = [k for k in names if k != "copy"]
        best = min(grids, key=lambda k: r[k]["ms"]["median"])
        default = next(k for k in grids if r[best]["ms"]["min"] <= r[k]["ms"]["median"] <= r[best]["ms"]["max"])
        r["payload_bytes"], r["best"], r["smallest_within_best_range"] = payload, best, default
        r["gather_over_copy_rate"] = r[default]["GBps_median"] / r["copy"]["GBps_median"]
        res["link"][str(dtype)] = r
        lines.append("link, %s, %.3f GB per batch over PCIe:" % (dtype, payload * 1e-9))
        for k in names:
            lines.append("  %-10s %s = %.1f GB/s" % (k, fmt(times[k]), r[k]["GBps_median"]))
        lines.append("  best grid %s; smallest grid whose median is inside the best's min-max: %s, at %.3f of the copy's rate"
                     % (best, default, r["gather_over_copy_rate"]))
        if dtype == torch.float32:
            st_host = st
        del src, dst, legs
    del st

    # what a tiered call costs the host: 300 launches of a 1-row, 1-token gather each, host clock, the device drained before and after
    st_res = DeviceSlideStore(bags, ids, mods, dev)
    one = MF.h2d(st_res.bag_table[:1, :1].reshape(-1), dev)
    calls = {"S1 (one launch)": lambda: MF.bag_sample(st_res.rows, st_res.off, one, None, 1, 0, 0),
             "S3, no host tier (one launch, no query)": lambda: MF.bag_sample_tiered(st_res.rows, None, st_res.off, one, None, 1, 0, 0),
             "S3, host tier (two launches, the queries)": lambda: MF.bag_sample_tiered(st_host.rows, st_host.rows_host, st_host.off, one, None,
                                                                                       1, 0, 0)}
    res["host_cost_us_per_call"] = {}
    for k, f in calls.items():
        per = []
        for rep in range(5):
            f()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(300):
                f()
            per.append((time.perf_counter() - t0) / 300 * 1e6)
            torch.cuda.synchronize()
        res["host_cost_us_per_call"][k] = stats(per)
        lines.append("host clock per call, %-42s median %.2f us (min %.2f max %.2f)" % (k, statistics.median(per), min(per), max(per)))

    # ---- 7. the step
    if not a.skip_step:
        torch.manual_seed(42)
        model = MADELEINE(BN.make_cfg(M, D), stain_encoding=stain).to(dev).train()
        opt = torch.optim.AdamW(model.parameters(), lr=1e-4, fused=True)
        crit = InfoNCE(temperature=0.001)
        largs = SimpleNamespace(global_loss="info-nce", symmetric_cl=True, local_loss_weight=1.0)

        def step(data):
            opt.zero_grad(set_to_none=True)
            embs, toks = model(data, device=dev)
            loss, _ = calculate_losses(mods[1:], crit, None, None, embs, toks, data["modality_labels"][:, 1:], largs)
            loss.backward()
            opt.step()
        st_half = DeviceSlideStore(bags, ids, mods, dev, resident_bytes=st_res.nbytes() // 2)
        res["stores"] = {"resident": st_res.nbytes("device"), "all_host": st_host.nbytes("host"),
                         "half": [st_half.nbytes("device"), st_half.nbytes("host")]}
        loaders = {"a_resident": st_res.batches(B, N, shuffle=True, seed=1), "b_host_prefetch1": st_host.batches(B, N, shuffle=True, seed=1, prefetch=1),
                   "c_host_prefetch0": st_host.batches(B, N, shuffle=True, seed=1, prefetch=0),
                   "d_half_prefetch1": st_half.batches(B, N, shuffle=True, seed=1, prefetch=1)}
        if len(loaders["a_resident"]) <= a.round_steps:
            raise SystemExit("--tier-cases must give more than --round-steps batches per epoch")
        epoch = [0]

        def timed_round(k):
            """One epoch of loader k: the first step untimed (it fills the prefetch queue), then round_steps timed steps."""
            loaders[k].set_epoch(epoch[0])
            epoch[0] += 1
            it = iter(loaders[k])
            step(next(it))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.round_steps):
                step(next(it))
            e1.record()
            e1.synchronize()
            it.close()
            return e0.elapsed_time(e1) / a.round_steps
        rounds = max(1, a.steps // a.round_steps)
        for k in loaders:
            timed_round(k)                                       # warm-up
        times = {k: [] for k in loaders}
        for r in range(rounds):
            for k in (sorted(loaders) if r % 2 == 0 else sorted(loaders, reverse=True)):
                times[k].append(timed_round(k))
        med = {k: statistics.median(v) for k, v in times.items()}
        res["step"] = {"rounds": rounds, "steps_per_round": a.round_steps, "rounds_ms": times, "step_ms": {k: stats(v) for k, v in times.items()},
                       "b_minus_a_ms": med["b_host_prefetch1"] - med["a_resident"],
                       "a_round_range_ms": max(times["a_resident"]) - min(times["a_resident"]),
                       "c_minus_a_ms": med["c_host_prefetch0"] - med["a_resident"], "d_minus_a_ms": med["d_half_prefetch1"] - med["a_resident"]}
        lines.append("config-2 step, %d rounds of %d timed steps per feed:" % (rounds, a.round_steps))
        for k, v in sorted(times.items()):
            lines.append("  fed by %-17s median %.3f ms  min %.3f  max %.3f   rounds: %s" % (k, med[k], min(v), max(v), " ".join("%.3f" % x for x in v)))
        lines.append("  (b) - (a) = %.3f ms, (a)'s round range %.3f ms;  (c) - (a) = %.3f ms;  (d) - (a) = %.3f ms"
                     % (res["step"]["b_minus_a_ms"], res["step"]["a_round_range_ms"], res["step"]["c_minus_a_ms"], res["step"]["d_minus_a_ms"]))

        # (e): the host DataLoader feed in a phase of its own, next to (a) and (b)
        drain = a.workers + 6
        total = a.warmup + rounds * (drain + a.round_steps) + 4
        loader = torch.utils.data.DataLoader(HostCohort(bags, N, -(-total * B // n_cases) + 1), batch_size=B, shuffle=False, collate_fn=collate,
                                             num_workers=a.workers, pin_memory=True, prefetch_factor=1 if a.workers else None)
        fed = iter(DevicePrefetcher(loader, dev, depth=2))
        for _ in range(a.warmup):
            step(next(fed))
        torch.cuda.synchronize()
        phase = {"e_host_loader": [], "a_resident": [], "b_host_prefetch1": []}
        for r in range(rounds):
            for k in (sorted(phase) if r % 2 == 0 else sorted(phase, reverse=True)):
                if k != "e_host_loader":
                    phase[k].append(timed_round(k))
                    continue
                for _ in range(drain):
                    step(next(fed))
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(a.round_steps):
                    step(next(fed))
                e1.record()
                e1.synchronize()
                phase[k].append(e0.elapsed_time(e1) / a.round_steps)
        fed.close()
        b_all = times["b_host_prefetch1"] + phase["b_host_prefetch1"]
        holds = max(b_all) < min(phase["e_host_loader"])
        res["host_phase"] = {"rounds_ms": phase, "step_ms": {k: stats(v) for k, v in phase.items()}, "workers": a.workers,
                             "slowest_b_round_ms": max(b_all), "fastest_e_round_ms": min(phase["e_host_loader"]), "required_holds": holds}
        lines.append("phase of the host DataLoader feed (%d workers), next to (a) and (b):" % a.workers)
        for k, v in sorted(phase.items()):
            lines.append("  fed by %-17s median %.3f ms  min %.3f  max %.3f   rounds: %s"
                         % (k, statistics.median(v), min(v), max(v), " ".join("%.3f" % x for x in v)))
        lines.append("  required: slowest round of (b), both phases, %.3f ms < fastest round of (e) %.3f ms: %s"
                     % (max(b_all), min(phase["e_host_loader"]), "HOLDS" if holds else "DOES NOT HOLD"))
    return lines, res


class HostBags(torch.utils.data.Dataset):
    """What a DataLoader(SimpleDataset, batch_size=1) hands run_inference -- (feats [1, N, D], [slide id]) -- over bags held in host
    memory: a view per item, nothing is read, parsed or stacked."""

    def __init__(self, bags, ids):
        self.bags, self.ids = bags, ids

    def __len__(self):
        return len(self.bags)

    def __getitem__(self, i):
        return self.bags[i][None], [self.ids[i]]


def embed_leg(a, dev):
    """Measurements 8-9 of the module docstring.  Returns (lines, results)."""
    from madeleine_amd import utils as MU
    n, rows, D, N = a.embed_cases, a.embed_rows, 512, 4096
    g = torch.Generator().manual_seed(7)
    base = torch.randn(rows + n, D, generator=g)
    bags = [[base[c:c + rows]] for c in range(n)]        # overlapping windows of one tensor: distinct bags, one host allocation
    ids = ["case%05d" % c for c in range(n)]
    cases, T = list(range(n)), n * rows
    lines, res = [], {"geometry": {"cases": n, "rows_per_bag": rows, "D": D, "sample_tokens": N}}

    # ---- 8. the mean kernel
    res["kernel"] = {}
    for dtype in (torch.float32, torch.bfloat16):
        st = DeviceSlideStore(bags, ids, ["HE"], dev, dtype=dtype)
        esz = st.rows.element_size()
        work = {"mean": T * D * esz, "mean_embeddings": T * D * esz, "sample": n * N * D * (4 + esz)}
        chunks = torch.zeros(n + 1, dtype=torch.int64)
        chunks[1:] = torch.cumsum((st.bag_lens_cpu + MF.BAG_MEAN_ROWS - 1) // MF.BAG_MEAN_ROWS, 0)
        bag_d, chunk_cu, n_chunks = torch.arange(n, dtype=torch.int32).to(dev), chunks.to(dev), int(chunks[-1])
        calls = {"mean": lambda i: MF.bag_mean(st.rows, st.off, bag_d, chunk_cu, n_chunks),
                 "mean_embeddings": lambda i: st.mean_embeddings(0)["embeds"], "sample": lambda i: st.sample(cases, N, counter=i)}
        for f in calls.values():
            for i in range(3):
                f(i)
        times = {k: [] for k in calls}
        for i in range(a.launches):
            order = sorted(calls) if i % 2 == 0 else sorted(calls, reverse=True)
            for _ in range(4):                           # untimed, ~0.6 ms of device work: the host runs ahead of the device, so the
                del_me = calls["sample"](50 + i)         # first timed call of the sequence holds no launch gap
                del del_me
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(order) + 1)]
            ev[0].record()
            for j, k in enumerate(order):
                out = calls[k](100 + i)
                ev[j + 1].record()
                del out
            ev[-1].synchronize()
            for j, k in enumerate(order):
                times[k].append(ev[j].elapsed_time(ev[j + 1]))
        res["kernel"][str(dtype)] = {k: {"ms": stats(v), "payload_bytes": work[k], "TBps_median": work[k] / statistics.median(v) * 1e-9}
                                     for k, v in times.items()}
        for k, v in sorted(times.items()):
            lines.append("%-15s %-14s median %.3f ms (min %.3f max %.3f) = %.2f TB/s over %.2f GB"
                         % (k, str(dtype), statistics.median(v), min(v), max(v), work[k] / statistics.median(v) * 1e-9, work[k] * 1e-9))
        if dtype != torch.float32:
            del st
        else:
            st32 = st
    st = st32

    # ---- 9. extraction: store.embed against run_inference over a host dataloader of the same bags
    if not a.skip_step:
        torch.manual_seed(42)
        model = MADELEINE(BN.make_cfg(2, D)).to(dev).eval()
        pinned = [case[0].contiguous().pin_memory() for case in bags]
        loader = torch.utils.data.DataLoader(HostBags(pinned, ids), batch_size=None, shuffle=False, num_workers=0)

        def host_clock(f):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = f()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            del out
            return t1 - t0
        feeds = {"store_embed": lambda: st.embed(model), "run_inference": lambda: MU.run_inference(model, loader, torch_precision=torch.float32)}
        for f in feeds.values():
            f()
        wall = {k: [] for k in feeds}
        for r in range(max(1, a.steps)):
            for k in (sorted(feeds) if r % 2 == 0 else sorted(feeds, reverse=True)):
                wall[k].append(n / host_clock(feeds[k]))
        res["extraction"] = {k: {"bags_per_s": stats(v)} for k, v in wall.items()}
        res["extraction"]["note"] = "run_inference also copies the embeddings to the host and computes their smooth rank (one SVD of [n, 512])"
        for k, v in sorted(wall.items()):
            lines.append("%-13s median %.1f bags/s (min %.1f max %.1f) over %d bags of %d rows, fp32, 4 bags per launch set"
                         % (k, statistics.median(v), min(v), max(v), n, rows))
    return lines, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--round-steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workers", type=int, default=6, help="DataLoader workers of each host-fed path")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--no-h5", action="store_true", help="leave out the feed that reads h5 files")
    ap.add_argument("--h5-dir", default=None, help="where the synthetic cohort's h5 files go (default: the system's temporary directory)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--pack", action="store_true", help="measure the packed ragged route (config 5's shape) instead")
    ap.add_argument("--cap", type=int, default=4096, help="max_tokens of the capped pack of --pack")
    ap.add_argument("--tier", action="store_true", help="measure the two-tier store (host tier read over PCIe) instead")
    ap.add_argument("--tier-cases", type=int, default=192, help="cases of the cohort of --tier: more than --round-steps batches per epoch")
    ap.add_argument("--tier-rows", type=int, default=4096, help="rows per bag of the cohort of --tier")
    ap.add_argument("--embed", action="store_true", help="measure the mean kernel and store.embed against run_inference instead")
    ap.add_argument("--embed-cases", type=int, default=48, help="H&E bags of the cohort of --embed")
    ap.add_argument("--embed-rows", type=int, default=30000, help="rows per bag of the cohort of --embed")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.pack or a.tier or a.embed:
        lines, res = (pack_leg if a.pack else tier_leg if a.tier else embed_leg)(a, dev)
        report(lines, res, a.out)
        return
    B, M, N, D, _got, stain = BN.CONFIGS["c2"]
    mods = BN.MODS5[:M]
    g = torch.Generator().manual_seed(7)
    bags = [[torch.randn(a.rows, D, generator=g) for _ in range(M)] for _ in range(B)]
    ids = ["case%05d" % i for i in range(B)]
    lines, res = [], {"geometry": {"cases": B, "stains": M, "rows_per_bag": a.rows, "D": D, "N": N}}

    # ---- 1. the kernel
    res["kernel"] = {}
    payload = B * M * N * D
    src = torch.randn(payload, device=dev)
    dst = torch.empty_like(src)
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        st = DeviceSlideStore(bags, ids, mods, dev, dtype=dtype)
        cases = list(range(B))
        for i in range(3):
            st.sample(cases, N, counter=i)
        times, copies = [], []
        for i in range(a.launches):                      # alternating: a gather, a copy of the same payload
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            dst.copy_(src)                               # untimed: the host runs ahead of the device, no launch gap is timed
            e[0].record()
            out = st.sample(cases, N, counter=100 + i)
            e[1].record()
            dst.copy_(src)
            e[2].record()
            e[2].synchronize()
            times.append(e[0].elapsed_time(e[1]))
            copies.append(e[1].elapsed_time(e[2]))
            del out
        nbytes = payload * (4 + st.rows.element_size())
        k = {"ms": stats(times), "payload_bytes": nbytes, "TBps_median": nbytes / statistics.median(times) * 1e-9,
             "torch_copy_ms": stats(copies), "torch_copy_TBps_median": payload * 8 / statistics.median(copies) * 1e-9}
        res["kernel"][str(dtype)] = k
        lines.append("gather %-14s median %.3f ms (min %.3f max %.3f) = %.2f TB/s over %.2f GB;  torch copy of 2 x %.2f GB: %.3f ms = %.2f TB/s"
                     % (str(dtype), k["ms"]["median"], k["ms"]["min"], k["ms"]["max"], k["TBps_median"], nbytes * 1e-9, payload * 4e-9,
                        k["torch_copy_ms"]["median"], k["torch_copy_TBps_median"]))
        if dtype != torch.float32:
            del st
    del src, dst
    st = DeviceSlideStore(bags, ids, mods, dev)

    # ---- 2. the step
    if not a.skip_step:
        torch.manual_seed(42)
        model = MADELEINE(BN.make_cfg(M, D), stain_encoding=stain).to(dev).train()
        opt = torch.optim.AdamW(model.parameters(), lr=1e-4, fused=True)
        crit = InfoNCE(temperature=0.001)
        largs = SimpleNamespace(global_loss="info-nce", symmetric_cl=True, local_loss_weight=1.0)

        def step(data):
            opt.zero_grad(set_to_none=True)
            embs, toks = model(data, device=dev)
            loss, _ = calculate_losses(mods[1:], crit, None, None, embs, toks, data["modality_labels"][:, 1:], largs)
            loss.backward()
            opt.step()

        drain = a.workers + 6                            # the workers' queues (prefetch_factor 1), the pinning thread, the prefetcher's ring
        rounds = max(1, a.steps // a.round_steps)
        total = a.warmup + a.steps + rounds * drain + 4
        it = st.batches(B, N, shuffle=True, seed=1)
        epoch = [0]

        def store_batch():
            it.set_epoch(epoch[0])
            epoch[0] += 1
            return next(iter(it))
        const = store_batch()

        def host_feed():
            loader = torch.utils.data.DataLoader(HostCohort(bags, N, total), batch_size=B, shuffle=False, collate_fn=collate,
                                                 num_workers=a.workers, pin_memory=True, prefetch_factor=1 if a.workers else None)
            return iter(DevicePrefetcher(loader, dev, depth=2)), None

        # one phase per host-fed path, so that only ONE set of DataLoader workers is alive while anything is timed: the path against the
        # store and the constant batch, alternating
        phases = ([] if a.no_h5 else [("h5", lambda: h5_feed(bags, ids, mods, N, D, B, total, a.workers, dev, a.h5_dir))]) + [("host", host_feed)]
        gather = res["kernel"]["torch.float32"]["ms"]["median"]
        res["step_rounds"] = {"rounds": rounds, "steps_per_round": a.round_steps, "workers": a.workers, "drained_before_a_fed_round": drain}
        res["phases"] = {}
        for name, make in phases:
            fed, scratch_dir = make()
            feeds = {name: lambda: next(fed), "store": store_batch, "const": lambda: const}
            for f in feeds.values():
                for _ in range(a.warmup):
                    step(f())
            torch.cuda.synchronize()
            times = {k: [] for k in feeds}
            for r in range(rounds):
                order = sorted(feeds) if r % 2 == 0 else sorted(feeds, reverse=True)
                for k in order:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    if k == name:                        # batches that were prefetched while the other feeds ran cost this path nothing:
                        for _ in range(drain):           # consume them untimed, so that the round times what the path can sustain
                            step(feeds[k]())
                    torch.cuda.synchronize()
                    e0.record()
                    for _ in range(a.round_steps):
                        step(feeds[k]())
                    e1.record()
                    e1.synchronize()
                    times[k].append(e0.elapsed_time(e1) / a.round_steps)
            fed.close()                                  # the prefetcher's thread and the DataLoader's workers end here
            del fed, feeds
            if scratch_dir is not None:
                shutil.rmtree(scratch_dir, ignore_errors=True)      # the synthetic cohort's h5 files (2.6 GB)
            med = {k: statistics.median(v) for k, v in times.items()}
            spread = {k: max(v) - min(v) for k, v in times.items()}
            res["phases"][name] = {"step_ms": {k: stats(v) for k, v in times.items()},
                                   "rounds_ms": times, "fed_minus_store_ms": med[name] - med["store"], "fed_spread_ms": spread[name],
                                   "store_minus_const_ms": med["store"] - med["const"], "gather_ms": gather, "const_spread_ms": spread["const"]}
            lines.append("phase %s (%d rounds of %d steps, %d workers):" % (name, rounds, a.round_steps, a.workers))
            for k, v in sorted(times.items()):
                lines.append("  step fed by %-5s median %.3f ms  min %.3f  max %.3f   rounds: %s"
                             % (k, statistics.median(v), min(v), max(v), " ".join("%.3f" % x for x in v)))
            lines.append("  %s - store = %.3f ms (spread of %s over its rounds: %.3f);  store - const = %.3f ms (gather %.3f + spread of const %.3f)"
                         % (name, med[name] - med["store"], name, spread[name], med["store"] - med["const"], gather, spread["const"]))
    report(lines, res, a.out)


def report(lines, res, out):
    text = "\n".join(lines)
    print(text)
    print(json.dumps(res))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n" + json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
