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

Usage: python tools/exp_store.py [--rows 20000] [--launches 20] [--steps 20] [--round-steps 5] [--workers 6] [--out FILE]"""
import argparse
import json
import os
import shutil
import statistics
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench as BN  # noqa: E402
from madeleine_amd import MADELEINE, DeviceSlideStore, InfoNCE, calculate_losses  # noqa: E402
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
    a = ap.parse_args()
    dev = torch.device("cuda:0")
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
    text = "\n".join(lines)
    print(text)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n" + json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
