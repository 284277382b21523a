"""Device-resident slide store: the patch features of a whole pretraining cohort loaded ONCE into one device tensor, and every step's
`[B, M, N, D]` batch drawn from it on the device by one kernel (functional.bag_sample -> mdl_bag_sample, csrc/bag_sample.hip).
Ragged batches -- every bag at its own length, optionally cut to max_tokens rows drawn without replacement -- come packed out of the
same store by one launch of its variable-length form (pack / packed_batches: functional.bag_pack -> mdl_bag_pack), from a store of
any dtype.  One vector per slide comes out of it too, for a downstream cohort: embed() runs the encoder over single-stain packs
(pack_modality -> MADELEINE.encode_packed) and mean_embeddings() reduces whole bags to their column means where they lie
(functional.bag_mean -> mdl_bag_mean); both feed probe.linear_probe without the features leaving the device.
attention() is embed() with the attention kept (MADELEINE.attend_packed): raw scores, per-bag softmax, percentile ranks, order and
top-k patches per head for the whole cohort, any stain (functional.attn_softmax / attn_rank -> mdl_attn_softmax / mdl_attn_rank,
csrc/attn_map.hip).  heatmaps() goes on from there to RGBA images: the store holds the patch coordinates of every row (set_coords) and
madeleine_amd.heatmap renders the values over them (functional.heat_render -> mdl_heat_render, csrc/heat_map.hip).

Replaces, for a cohort that fits in HBM, the reference's input side (madeleine/datasets/wsi_dataset.py): SlideDataset.__getitem__
re-reads every stain's h5 file for every item of every epoch, draws `sample` rows on the host and collate stacks them, and the stacked
batch then crosses PCIe every step.  Here the only per-step host-to-device traffic is the `[B * M]` int32 table of the batch's bags.

Layout.  `rows [T_total, D]` holds the present bags back to back, case-major then modality-major; `off [n_bags + 1]` (int64, on the
device and on the host) is the first row of every stored bag; `bag_table [cases, M]` (int32, host) maps (case, modality) to its stored
bag or -1 for an absent stain; `modality_labels [cases, M]` follow from it.  The dataset's 2-token zero bags of absent stains are not
stored: the kernel writes their zeros.

The batches iterables yield exactly what collate() / ragged_collate() yield (`feats` already on the device), so train_loop and
MADELEINE.forward take them unchanged.  There is no CPU fallback: a store may be BUILT on the CPU (packing logic, tests), sampling from
it raises.

Two tiers.  A cohort larger than HBM keeps a prefix of whole bags on the device (`rows`, at most `resident_bytes` bytes) and the rest
in pinned host memory (`rows_host`); `resident_rows` = T_dev is the split, always at a bag boundary.  The tables and the draw keys
address rows of [0, T_total) as before, the same kernels read a host-tier bag over PCIe (functional.bag_sample_tiered /
bag_pack_tiered: a narrow persistent grid), and the batches are bit-equal to those of the resident store.  batches() and
packed_batches() then gather one batch ahead of the step on a side stream (`prefetch`).
"""
import collections
import mmap
import weakref
from typing import List, NamedTuple, Optional, Tuple

import torch

from . import functional as MF

FP16_MAX = 65504.0
_MAX_BAG_ROWS = 2 ** 31 - 1
_MAX_COORD = 1 << 24       # set_coords: 0 <= value < 2^24, the integers float32 (h5io.read_dataset) holds exactly
ABSENT_BAG_ROWS = 2        # the dataset's zero bag of an absent stain (wsi_dataset.py:66)
MEAN_WS_BYTES = 64 << 20   # mean_embeddings: the partial sums of one slice of cases stay inside this


class PackedBags(NamedTuple):
    """A ragged batch in packed form (DeviceSlideStore.pack): bag r = (case, modality), case-major, is rows cu_seqlens[r] ..
    cu_seqlens[r + 1] - 1 of tokens.  MADELEINE.forward takes it under the key 'packed'."""
    tokens: torch.Tensor                 # [T, D] fp32, on the device
    cu_seqlens: torch.Tensor             # [R + 1] int64, on the device
    lens: Tuple[int, ...]                # the R bag lengths, on the host
    row_bag: torch.Tensor                # [T] int32: the bag r of every row
    idx: Optional[torch.Tensor]          # [T] int32: the row inside the stored bag, -1 where zeros were written; None unless asked for


class DeviceSlideStore:
    def __init__(self, bags, slide_ids, modalities, device, dtype=torch.float32, resident_bytes=None, coords=None, patch_size=None):
        """bags: list over cases of lists over modalities of [n, D] CPU tensors, None for an absent stain.  dtype float16 / bfloat16:
        an opt-in LOSSY store of half the size (features are rounded once, at load time; fp16 refuses a bag it cannot hold).
        coords, patch_size: the patch coordinates of every bag (set_coords, which may also be called later); without them the store
        holds none and heatmaps() refuses.

        resident_bytes None: the whole store in one device tensor.  An integer >= 0: at most that many bytes of rows go to HBM -- the
        longest prefix of whole bags (stored order) that fits -- and the other bags to the host tier; 0 puts everything on the host, a
        budget of the store's size or more leaves the host tier empty.  The host tier is ONE ordinary page-aligned host allocation of
        exactly the tier's bytes (an anonymous mapping), registered with the runtime (hipHostRegister): the pinned size is the
        tier's size rounded up to a page, not the next power of two that torch's caching host allocator would pin.
        It is never pageable to the device and never managed memory, and it is unregistered when the store is collected.  Each
        process pins its own host tier: the ranks of a node do not share one.  On a CPU `device` (build-only mode) the host tier is
        an ordinary unpinned tensor."""
        if dtype not in MF.STORE_DTYPES:
            raise ValueError("DeviceSlideStore: dtype must be float32, float16 or bfloat16 (got %s)" % dtype)
        if resident_bytes is not None and (isinstance(resident_bytes, bool) or not isinstance(resident_bytes, int) or resident_bytes < 0):
            raise ValueError("DeviceSlideStore: resident_bytes must be None or an integer >= 0 (got %r)" % (resident_bytes,))
        self.modalities = list(modalities)
        self.slide_ids = list(slide_ids)
        self.device, self.dtype = torch.device(device), dtype
        n_cases, M = len(bags), len(self.modalities)
        if len(self.slide_ids) != n_cases:
            raise ValueError("DeviceSlideStore: %d cases but %d slide ids" % (n_cases, len(self.slide_ids)))
        table = torch.full((n_cases, M), -1, dtype=torch.int32)
        lens, present, D = [], [], None
        for c, case in enumerate(bags):
            if len(case) != M:
                raise ValueError("DeviceSlideStore: case %d (%s) has %d bags for %d modalities" % (c, self.slide_ids[c], len(case), M))
            for m, bag in enumerate(case):
                if bag is None:
                    continue
                where = "bag of case %d (%s), modality %s" % (c, self.slide_ids[c], self.modalities[m])
                if not torch.is_tensor(bag) or bag.dim() != 2 or not bag.is_floating_point():
                    raise ValueError("DeviceSlideStore: the %s must be a [n, D] float tensor" % where)
                if bag.shape[0] < 1 or bag.shape[0] > _MAX_BAG_ROWS:
                    raise ValueError("DeviceSlideStore: the %s has %d rows (1 .. 2^31 - 1 are supported)" % (where, bag.shape[0]))
                if D is None:
                    D = int(bag.shape[1])
                if bag.shape[1] != D or D < 1:
                    raise ValueError("DeviceSlideStore: the %s is %d wide, earlier bags are %d wide" % (where, bag.shape[1], D))
                if dtype == torch.float16:      # the one-off host check of the lossy store: fp16 would turn such a value into inf
                    absmax = float(bag.abs().max())
                    if not absmax <= FP16_MAX:
                        raise ValueError("DeviceSlideStore: the %s has absmax %g, beyond float16's %g; use float32 or bfloat16"
                                         % (where, absmax, FP16_MAX))
                table[c, m] = len(lens)
                lens.append(int(bag.shape[0]))
                present.append(bag)
        if D is None:
            raise ValueError("DeviceSlideStore: no present bag")
        self.dim = D
        self.bag_table = table
        self.modality_labels = (table >= 0).float()
        self.off_cpu = torch.zeros(len(lens) + 1, dtype=torch.int64)
        self.bag_lens_cpu = torch.tensor(lens, dtype=torch.int64)
        self.off_cpu[1:] = torch.cumsum(self.bag_lens_cpu, 0)
        total = int(self.off_cpu[-1])
        row_bytes = D * torch.empty(0, dtype=dtype).element_size()
        n_res = len(lens)                                       # resident bags: the longest prefix of whole bags inside the budget
        if resident_bytes is not None:
            n_res = int(torch.searchsorted(self.off_cpu, resident_bytes // row_bytes, right=True)) - 1
        self.resident_rows = T_dev = int(self.off_cpu[n_res])
        nbytes = T_dev * row_bytes
        if self.device.type == "cuda":
            free, capacity = torch.cuda.mem_get_info(self.device)
            if nbytes > free:
                raise RuntimeError("DeviceSlideStore: the store needs %d bytes (%d rows x %d x %s) but %s has %d bytes free of %d"
                                   % (nbytes, T_dev, D, dtype, self.device, free, capacity))
        self.rows = torch.empty(T_dev, D, dtype=dtype, device=self.device)
        self.rows_host = self._host_tier(total - T_dev) if T_dev < total else None
        self._upload(present[:n_res])
        off = self.off_cpu.tolist()
        for g in range(n_res, len(present)):                    # cast straight into place: no second copy of the cohort
            self.rows_host[off[g] - T_dev:off[g + 1] - T_dev].copy_(present[g])
        self.off = self.off_cpu.to(self.device)
        self._zero_bag = None
        self._side = None                                       # the prefetch stream: one per store, made on first use
        self.coords = self.coord_extents = self.patch_sizes = None
        if coords is not None:
            self.set_coords(coords, patch_size)
        elif patch_size is not None:
            raise ValueError("DeviceSlideStore: patch_size without coords")

    def set_coords(self, coords, patch_size):
        """The level-0 top-left corner (x, y) of every stored row: coords is a list over cases of lists over modalities of [n, 2]
        integer arrays or tensors -- the h5 `coords` dataset beside `features` -- None where the stain is absent; row j of an array
        belongs to row j of the bag.  patch_size: the level-0 pixels of a patch side, one int for the whole store or a list over
        cases of lists over modalities (None where absent).
        Checked on the host: n equals the bag's rows, every value is integral and 0 <= value < 2^24 -- h5io.read_dataset reads through
        float32, which holds exactly the integers of that range, so a coordinate beyond it may already have been rounded.  ValueError
        names the bag.  Kept as ONE int32 [T_total, 2] device tensor in store-row order (self.coords), always resident -- in a tiered
        store too: 8 bytes a row beside at least 1 KB of features -- with the per-bag extents (self.coord_extents [n_bags, 4] int64 =
        xmin, ymin, xmax, ymax) and patch sizes (self.patch_sizes [n_bags] int64) on the host, from which heatmaps() plans its
        canvases without a device read."""
        n_cases, M = len(self), len(self.modalities)
        if len(coords) != n_cases:
            raise ValueError("DeviceSlideStore.set_coords: %d cases but %d coordinate lists" % (n_cases, len(coords)))
        per_bag = not isinstance(patch_size, int) or isinstance(patch_size, bool)
        if per_bag and (not isinstance(patch_size, (list, tuple)) or len(patch_size) != n_cases):
            raise ValueError("DeviceSlideStore.set_coords: patch_size must be one int or a list over cases of lists over modalities")
        total = int(self.off_cpu[-1])
        xy = torch.empty(total, 2, dtype=torch.int32)
        ext = torch.empty(self.n_bags, 4, dtype=torch.int64)
        sizes = torch.empty(self.n_bags, dtype=torch.int64)
        off = self.off_cpu.tolist()
        for c in range(n_cases):
            if len(coords[c]) != M or (per_bag and len(patch_size[c]) != M):
                raise ValueError("DeviceSlideStore.set_coords: case %d (%s) needs one entry per modality (%d)" % (c, self.slide_ids[c], M))
            for m in range(M):
                g = int(self.bag_table[c, m])
                where = "bag of case %d (%s), modality %s" % (c, self.slide_ids[c], self.modalities[m])
                if g < 0:
                    if coords[c][m] is not None:
                        raise ValueError("DeviceSlideStore.set_coords: coordinates for the absent %s" % where)
                    continue
                if coords[c][m] is None:
                    raise ValueError("DeviceSlideStore.set_coords: the %s is present and has no coordinates" % where)
                a = torch.as_tensor(coords[c][m])
                n = off[g + 1] - off[g]
                if a.dim() != 2 or a.shape[1] != 2 or a.shape[0] != n:
                    raise ValueError("DeviceSlideStore.set_coords: the %s has %d rows, its coordinates are %s (need [%d, 2])"
                                     % (where, n, tuple(a.shape), n))
                if a.dtype == torch.bool or a.is_complex():
                    raise ValueError("DeviceSlideStore.set_coords: the coordinates of the %s must be numbers (got %s)" % (where, a.dtype))
                if a.is_floating_point():
                    a = a.double()
                    if not bool(torch.isfinite(a).all()) or not bool((a == a.round()).all()):
                        raise ValueError("DeviceSlideStore.set_coords: the coordinates of the %s are not integral" % where)
                a = a.cpu()
                lo_xy, hi_xy = a.min(0).values.long(), a.max(0).values.long()
                lo, hi = int(lo_xy.min()), int(hi_xy.max())
                if lo < 0 or hi >= _MAX_COORD:
                    raise ValueError("DeviceSlideStore.set_coords: the coordinates of the %s span %d .. %d; 0 <= value < 2^24 is the "
                                     "range float32 reads exactly" % (where, lo, hi))
                ps = patch_size[c][m] if per_bag else patch_size
                if isinstance(ps, bool) or not isinstance(ps, int) or not 1 <= ps <= _MAX_COORD:
                    raise ValueError("DeviceSlideStore.set_coords: the patch size of the %s must be an int in [1, 2^24] (got %r)"
                                     % (where, ps))
                xy[off[g]:off[g + 1]] = a.to(torch.int32)
                ext[g] = torch.cat([lo_xy, hi_xy])
                sizes[g] = ps
        self.coords = MF.h2d(xy, self.device)
        self.coord_extents, self.patch_sizes = ext, sizes

    def coords_of(self, case_indices, modality) -> torch.Tensor:
        """xy [T, 2] int32 on the device: the coordinates of the rows of pack_modality(case_indices, modality) with whole bags, in its
        order (case_indices None: every case that has the stain).  A gather of contiguous row ranges (torch.cat of views): host work
        per bag, none per row."""
        if self.coords is None:
            raise RuntimeError("DeviceSlideStore.coords_of: the store holds no coordinates (set_coords)")
        _, bag, _ = self._modality_plan(case_indices, modality)
        off = self.off_cpu
        views = [self.coords[int(off[g]):int(off[g + 1])] for g in bag.tolist()]
        return torch.cat(views) if views else self.coords[:0]

    def _host_tier(self, n_rows):
        """[n_rows, D] of the store's dtype in host memory: registered (pinned) on a GPU device, an ordinary tensor on the CPU."""
        if self.device.type != "cuda":
            return torch.empty(n_rows, self.dim, dtype=self.dtype)
        nbytes = n_rows * self.dim * torch.empty(0, dtype=self.dtype).element_size()
        raw = mmap.mmap(-1, nbytes)                             # anonymous, page-aligned, the tier's size rounded up to a page
        tier = torch.frombuffer(raw, dtype=self.dtype).view(n_rows, self.dim)      # zero-copy: the tensor's storage IS the mapping
        with torch.cuda.device(self.device):
            rt = torch.cuda.cudart()
            err = int(rt.cudaHostRegister(tier.data_ptr(), nbytes, 0))
        if err != 0:
            raise RuntimeError("DeviceSlideStore: registering the %d-byte host tier failed (hipError_t %d)" % (nbytes, err))
        weakref.finalize(self, _unregister, rt, tier.data_ptr(), raw)      # `raw` stays alive until the registration is gone
        if not tier.is_pinned():
            raise RuntimeError("DeviceSlideStore: the registered host tier does not report is_pinned()")
        return tier

    def _upload(self, present):
        """One bag at a time through two pinned staging buffers (the cast to the store's dtype happens in the host copy): the cohort is
        never concatenated on the host."""
        off = self.off_cpu.tolist()
        if self.device.type != "cuda":
            for g, bag in enumerate(present):
                self.rows[off[g]:off[g + 1]].copy_(bag)
            return
        if not present:
            return
        longest = max(int(b.shape[0]) for b in present)
        stage = [torch.empty(longest, self.dim, dtype=self.dtype).pin_memory() for _ in range(2)]
        busy = [None, None]
        with torch.cuda.device(self.device):
            for g, bag in enumerate(present):
                s = g & 1
                if busy[s] is not None:
                    busy[s].synchronize()          # the slot's previous upload has left the staging buffer
                n = bag.shape[0]
                stage[s][:n].copy_(bag)
                self.rows[off[g]:off[g + 1]].copy_(stage[s][:n], non_blocking=True)
                busy[s] = torch.cuda.Event()
                busy[s].record()
            torch.cuda.current_stream().synchronize()

    @classmethod
    def from_dataset(cls, dataset, device, dtype=torch.float32, resident_bytes=None, coords=False, patch_size=None):
        """One pass over a SlideDataset(sample=-1, train=True): keeps feats[m] where the label is 1 and drops the 2-token zero bags.
        coords=True: also reads the `coords` dataset of every present stain from the h5 path SlideDataset builds for its features
        (h5io.read_dataset(path, "coords")) and hands them to set_coords with patch_size, which is then required."""
        if getattr(dataset, "sample", -1) != -1 or not getattr(dataset, "train", True):
            raise ValueError("DeviceSlideStore.from_dataset needs a SlideDataset(sample=-1, train=True): whole bags, every stain")
        if coords and patch_size is None:
            raise ValueError("DeviceSlideStore.from_dataset: coords=True needs patch_size (level-0 pixels of a patch side)")
        bags, ids, xy = [], [], []
        if coords:
            import os
            from . import h5io
        for i in range(len(dataset)):
            item = dataset[i]
            present = [int(lab) == 1 for lab in item['modality_labels']]
            bags.append([f if p else None for f, p in zip(item['feats'], present)])
            ids.append(item['slide_id'])
            if coords:
                split = dataset.dataframe.iloc[i]['split']
                special = "" if split == "train" else "_%s" % split
                xy.append([h5io.read_dataset(os.path.join(dataset.features_path, "%s_%s%s.h5" % (item['slide_id'], m, special)),
                                             "coords").reshape(-1, 2) if p else None for m, p in zip(dataset.modalities, present)])
        return cls(bags, ids, dataset.modalities, device, dtype=dtype, resident_bytes=resident_bytes, coords=xy if coords else None,
                   patch_size=patch_size if coords else None)

    def __len__(self):
        return len(self.slide_ids)

    @property
    def n_bags(self) -> int:
        return self.off_cpu.numel() - 1

    def nbytes(self, tier=None) -> int:
        """Bytes of stored rows: tier None both tiers, "device" the rows in HBM, "host" the rows in pinned host memory."""
        if tier not in (None, "device", "host"):
            raise ValueError("DeviceSlideStore.nbytes: tier must be None, 'device' or 'host' (got %r)" % (tier,))
        dev = self.rows.numel() * self.rows.element_size()
        host = 0 if self.rows_host is None else self.rows_host.numel() * self.rows_host.element_size()
        return dev if tier == "device" else host if tier == "host" else dev + host

    def _cases(self, case_indices) -> torch.Tensor:
        idx = torch.as_tensor(case_indices, dtype=torch.int64).reshape(-1)
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= len(self)):
            raise IndexError("DeviceSlideStore: case index outside [0, %d)" % len(self))
        return idx

    def sample(self, case_indices, n_tokens, counter, seed=None, return_indices=False, host_wgs=0):
        """feats [B, M, n_tokens, D] fp32 on the device: SlideDataset.sample_n of every bag of the cases + collate, absent stains as
        zeros.  A bag's draw is a function of (seed, counter, its stored bag id): a case draws the same rows whatever its batch mates.
        The only upload is the batch's [B * M] int32 bag table.  return_indices: also idx [B, M, n_tokens] int32 (row inside the bag,
        -1 for an absent stain).  seed None is seed 0; batches() passes its own seed.  host_wgs: the grid of the pass that reads the
        host tier (0: the library's default); without a host tier it is not used."""
        if self.device.type != "cuda":
            raise RuntimeError("DeviceSlideStore.sample: the store lives on %s; the HIP kernel is the only backend (no CPU fallback)"
                               % self.device)
        idx = self._cases(case_indices)
        B, M = idx.numel(), len(self.modalities)
        bag = MF.h2d(self.bag_table.index_select(0, idx).reshape(-1), self.device)
        if self.rows_host is None:
            res = MF.bag_sample(self.rows, self.off, bag, None, n_tokens, 0 if seed is None else seed, counter, return_indices)
        else:
            res = MF.bag_sample_tiered(self.rows, self.rows_host, self.off, bag, None, n_tokens, 0 if seed is None else seed, counter,
                                       return_indices, host_wgs=host_wgs)
        if return_indices:
            return res[0].view(B, M, n_tokens, self.dim), res[1].view(B, M, n_tokens)
        return res.view(B, M, n_tokens, self.dim)

    def bag_view(self, case: int, modality: int) -> Optional[torch.Tensor]:
        """The stored rows of one bag as a zero-copy view of the store, None for an absent stain.  ValueError for a bag in the host
        tier: the model would read such a view over PCIe on every pass."""
        g = int(self.bag_table[case, modality])
        if g >= 0 and int(self.off_cpu[g + 1]) > self.resident_rows:
            raise ValueError("DeviceSlideStore.bag_view: the bag of case %d, modality %d is in the host tier; a view of it would be read "
                             "over PCIe on every pass -- use pack() / packed_batches()" % (case, modality))
        return None if g < 0 else self.rows[int(self.off_cpu[g]):int(self.off_cpu[g + 1])]

    def batches(self, batch_size, n_tokens, shuffle=True, drop_last=False, seed=0, rank=0, world_size=1, prefetch=None):
        """Re-iterable over collate()-shaped dicts {'feats' [B, M, n_tokens, D] on the device, 'modality_labels' CPU float [B, M],
        'slide_ids'}: the drop-in for DataLoader(SlideDataset(sample=n_tokens), collate_fn=collate).  prefetch k >= 1: the gathers of
        the next k batches of the epoch run on the store's side stream while the consumer works (None: 1 with a host tier, else 0 = gather on
        the current stream when the batch is asked for).  The batches do not depend on it."""
        return StoreBatches(self, batch_size, n_tokens, shuffle, drop_last, seed, rank, world_size, ragged=False, prefetch=prefetch)

    def ragged_batches(self, batch_size, shuffle=True, drop_last=False, seed=0, rank=0, world_size=1):
        """Re-iterable over ragged_collate()-shaped dicts {'bags', 'modality_labels', 'slide_ids'}: a present stain's bag is a zero-copy
        view of the store, an absent stain's the dataset's [2, D] zero bag.  Needs an fp32 store (the model reads the views as they are)."""
        if self.dtype != torch.float32:
            raise ValueError("DeviceSlideStore.ragged_batches needs a float32 store (this one is %s): the bags are views of it" % self.dtype)
        if self.rows_host is not None:
            raise ValueError("DeviceSlideStore.ragged_batches: %d of the %d stored bags are in the host tier and the bags are zero-copy "
                             "views, which the model would read over PCIe on every pass -- use packed_batches()"
                             % (self.n_bags - int((self.off_cpu[1:] <= self.resident_rows).sum()), self.n_bags))
        return StoreBatches(self, batch_size, None, shuffle, drop_last, seed, rank, world_size, ragged=True)

    def _pack_plan(self, case_indices, max_tokens):
        """(bag [R] int32, lens [R] int64) of the packed form of the cases, on the host: case-major, then modality-major."""
        if max_tokens is not None and max_tokens < 1:
            raise ValueError("DeviceSlideStore: max_tokens must be at least 1 (got %s)" % max_tokens)
        bag = self.bag_table.index_select(0, self._cases(case_indices)).reshape(-1)
        lens = self.bag_lens_cpu.index_select(0, bag.clamp(min=0).long())
        if max_tokens is not None:
            lens = lens.clamp(max=int(max_tokens))
        return bag, torch.where(bag >= 0, lens, torch.full_like(lens, ABSENT_BAG_ROWS))

    def pack_lens(self, case_indices, max_tokens=None) -> List[int]:
        """The bag lengths of pack(case_indices, max_tokens), case-major then modality-major: a present bag's rows (at most max_tokens
        of them when a cap is given), 2 for an absent stain (the dataset's zero bag).  Host only."""
        return self._pack_plan(case_indices, max_tokens)[1].tolist()

    def pack(self, case_indices, max_tokens=None, counter=0, seed=None, return_indices=False, host_wgs=0) -> PackedBags:
        """The ragged batch of the cases, packed: every present bag whole and in stored order, or -- when it has more than max_tokens
        rows -- max_tokens of its rows drawn without replacement (the rows sample(..., max_tokens, counter, seed) draws for it); an
        absent stain as 2 rows of zeros.  One launch, from a store of any dtype; the only upload is one O(R) table (cu_seqlens, the
        chunk table of the launch and the bags); no host read and no host work per token.  host_wgs: as in sample()."""
        if self.device.type != "cuda":
            raise RuntimeError("DeviceSlideStore.pack: the store lives on %s; the HIP kernel is the only backend (no CPU fallback)"
                               % self.device)
        bag, lens = self._pack_plan(case_indices, max_tokens)
        return self._pack_bags(bag, lens, counter, seed, return_indices, host_wgs)

    def _pack_bags(self, bag, lens, counter, seed, return_indices, host_wgs) -> PackedBags:
        """The pack of stored bags `bag` [R] int32 (-1: zeros) at `lens` [R] int64 rows each, both on the host: the launch's tables, their
        one upload and the launch.  What pack() and pack_modality() share."""
        R = bag.numel()
        host = torch.zeros(2 * (R + 1) + (R + 1) // 2, dtype=torch.int64)        # cu | chunk_cu | bag (int32, two to a word)
        torch.cumsum(lens, 0, out=host[1:R + 1])
        torch.cumsum((lens + 63) // 64, 0, out=host[R + 2:2 * R + 2])
        host[2 * R + 2:].view(torch.int32)[:R] = bag
        T, n_chunks = int(host[R]), int(host[2 * R + 1])
        table = MF.h2d(host, self.device)
        cu = table[:R + 1]
        if self.rows_host is None:
            res = MF.bag_pack(self.rows, self.off, table[2 * R + 2:].view(torch.int32)[:R], None, cu, table[R + 1:2 * R + 2], T, n_chunks,
                              0 if seed is None else seed, counter, return_indices)
        else:
            res = MF.bag_pack_tiered(self.rows, self.rows_host, self.off, table[2 * R + 2:].view(torch.int32)[:R], None, cu,
                                     table[R + 1:2 * R + 2], T, n_chunks, 0 if seed is None else seed, counter, return_indices,
                                     host_wgs=host_wgs)
        return PackedBags(res[0], cu, tuple(lens.tolist()), res[1], res[2] if return_indices else None)

    def _modality_plan(self, case_indices, modality, max_tokens=None):
        """(cases [n] int64, bag [n] int32, lens [n] int64) of one stain's bags, on the host: the cases asked for in the order asked, or
        -- case_indices None -- every case that has the stain, in case order; lens are the bags' rows, at most max_tokens of them.
        IndexError for a modality outside [0, M) or a case outside the store, ValueError naming the first case asked for that lacks
        the stain."""
        M = len(self.modalities)
        if isinstance(modality, bool) or not isinstance(modality, int) or not 0 <= modality < M:
            raise IndexError("DeviceSlideStore: modality must be an integer in [0, %d) (got %r)" % (M, modality))
        if max_tokens is not None and max_tokens < 1:
            raise ValueError("DeviceSlideStore: max_tokens must be at least 1 (got %s)" % max_tokens)
        col = self.bag_table[:, modality]
        if case_indices is None:
            cases = (col >= 0).nonzero().reshape(-1)
        else:
            cases = self._cases(case_indices)
        bag = col.index_select(0, cases)
        if bool((bag < 0).any()):
            c = int(cases[int((bag < 0).nonzero()[0])])
            raise ValueError("DeviceSlideStore: case %d (%s) has no %s bag" % (c, self.slide_ids[c], self.modalities[modality]))
        lens = self.bag_lens_cpu.index_select(0, bag.long())
        if max_tokens is not None:
            lens = lens.clamp(max=int(max_tokens))
        return cases, bag, lens

    def _require_device(self, what):
        if self.device.type != "cuda":
            raise RuntimeError("DeviceSlideStore.%s: the store lives on %s; the HIP kernel is the only backend (no CPU fallback)"
                               % (what, self.device))

    def pack_modality(self, case_indices, modality, max_tokens=None, counter=0, seed=None, host_wgs=0) -> PackedBags:
        """pack() for ONE stain: bag r of the result is the `modality` bag of case case_indices[r], whole and in stored order or cut to
        max_tokens rows by pack()'s draw (a bag's draw is a function of seed, counter and its stored bag id, so these are the rows
        pack() and sample() draw for it).  ValueError naming the case when a case lacks the stain (there is no zero bag here: a slide
        that does not exist has no embedding), IndexError for a modality outside [0, M)."""
        self._require_device("pack_modality")
        _, bag, lens = self._modality_plan(case_indices, modality, max_tokens)
        return self._pack_bags(bag, lens, counter, seed, False, host_wgs)

    def _embedding_result(self, embeds, cases, rank=False):
        res = {"embeds": embeds, "cases": cases, "slide_ids": [self.slide_ids[c] for c in cases.tolist()]}
        if rank:      # the number the reference prints beside every extraction (utils.py:70), from the HIP kernels: one host read
            res["rank"] = round(MF.smooth_rank(embeds)[0].item(), 2)
        return res

    def mean_embeddings(self, modality=0, case_indices=None, host_wgs=0, rank=False) -> dict:
        """The mean patch embedding of one stain's bag of every case asked for (None: every case that has the stain): {"embeds" [n, D]
        fp32 on the device, "cases" [n] int64 on the host, "slide_ids"} -- bin/extract_mean_embs.py for a cohort in the store, the
        baseline of the linear probe.  Whole bags, read where they lie (both tiers, any store dtype) by functional.bag_mean; the bits
        of a row depend on that bag alone.  One O(n) upload per call (the bags and the chunk tables); the work goes in slices of cases
        whose partial sums stay inside MEAN_WS_BYTES (a bag whose own partials exceed it goes alone).  ValueError / IndexError as
        pack_modality; host_wgs as in sample().  rank=True adds "rank": the smooth rank of the embeddings as a Python float rounded to 2
        decimals (functional.smooth_rank on the device; NotImplementedError past min(n, D) = 1024, ValueError for no case at all)."""
        self._require_device("mean_embeddings")
        cases, bag, lens = self._modality_plan(case_indices, modality)
        n, D = bag.numel(), self.dim
        if n == 0:
            return self._embedding_result(torch.zeros(0, D, dtype=torch.float32, device=self.device), cases, rank)
        chunks = (lens + (MF.BAG_MEAN_ROWS - 1)) // MF.BAG_MEAN_ROWS
        budget = max(1, MEAN_WS_BYTES // (4 * D))                # chunks per slice
        cuts, used = [0], 0
        for i, c in enumerate(chunks.tolist()):
            if used and used + c > budget:
                cuts.append(i)
                used = 0
            used += c
        cuts.append(n)
        k = len(cuts) - 1
        host = torch.zeros(n + k + (n + 1) // 2, dtype=torch.int64)      # per slice chunk_cu [R_s + 1] | bag (int32, two to a word)
        for j in range(k):
            a, b = cuts[j], cuts[j + 1]
            torch.cumsum(chunks[a:b], 0, out=host[a + j + 1:b + j + 1])
        host[n + k:].view(torch.int32)[:n] = bag
        totals = [int(host[cuts[j + 1] + j]) for j in range(k)]
        table = MF.h2d(host, self.device)
        bag_d = table[n + k:].view(torch.int32)[:n]
        outs = []
        for j in range(k):
            a, b = cuts[j], cuts[j + 1]
            if self.rows_host is None:
                outs.append(MF.bag_mean(self.rows, self.off, bag_d[a:b], table[a + j:b + j + 1], totals[j]))
            else:
                outs.append(MF.bag_mean_tiered(self.rows, self.rows_host, self.off, bag_d[a:b], table[a + j:b + j + 1], totals[j],
                                               host_wgs=host_wgs))
        return self._embedding_result(outs[0] if k == 1 else torch.cat(outs), cases, rank)

    def _prototype_source(self, what, modality, case_indices):
        """(cases, the cluster.RowSource over one stain's bags) for the k-means read-outs: whole bags, read where they lie.  Resident
        tier only: Lloyd re-reads every row twice per iteration, and PCIe is not the place for that."""
        from . import cluster
        self._require_device(what)
        cases, bag, lens = self._modality_plan(case_indices, modality)
        ends = self.off_cpu.index_select(0, bag.long() + 1)
        if bool((ends > self.resident_rows).any()):
            c = int(cases[int((ends > self.resident_rows).nonzero()[0])])
            raise NotImplementedError("DeviceSlideStore.%s: the %s bag of case %d (%s) lies in the pinned host tier; k-means reads "
                                      "resident bags only" % (what, self.modalities[modality], c, self.slide_ids[c]))
        if bag.numel() == 0:
            raise ValueError("DeviceSlideStore.%s: no case has a %s bag" % (what, self.modalities[modality]))
        return cases, cluster.RowSource(self.rows, self.off, bag, lens, self.off_cpu.index_select(0, bag.long()))

    def prototypes(self, k, modality=0, case_indices=None, **fit) -> dict:
        """k morphological prototypes of one stain: cluster.fit_kmeans(k, **fit) over ALL rows of the bags of the cases asked for (None:
        every case that has the stain), read where they lie in any store dtype -- no packed copy.  Returns the KMeansResult's fields
        ("centroids" [k, D], "labels" [T], "dist" [T], "counts" [k], "inertia", "n_iter", "converged") plus "cu" (int64 [n + 1] on the
        device: bag r of the list is call positions cu[r] .. cu[r + 1] - 1 of labels), "cases" and "slide_ids"; bit for bit what
        fit_kmeans gives on the packed rows of the same bags.  One O(n) table upload.  NotImplementedError naming the first case whose
        bag lies in the pinned host tier; ValueError / IndexError as pack_modality."""
        from . import cluster
        cases, src = self._prototype_source("prototypes", modality, case_indices)
        res = cluster.fit_kmeans(src, k, **fit)
        out = res._asdict()
        out.update(cu=src.cu, cases=cases, slide_ids=[self.slide_ids[c] for c in cases.tolist()])
        return out

    def prototype_histograms(self, centroids, modality=0, case_indices=None, normalize=True) -> dict:
        """The bag of prototypes of every case asked for: {"embeds" [n, k] fp32 on the device, "cases", "slide_ids"}, mean_embeddings'
        shape, so it feeds linear_probe, linear_probe_cv, the *_ci functions and slide_neighbours unchanged.  embeds[r, j] is the number
        of rows of the case's bag whose nearest centroid is j (one assign pass and functional.kmeans_hist; a row with a non-finite
        element is counted nowhere), divided by the row's total when normalize (a bag of no countable row stays zeros)."""
        from . import cluster
        cases, src = self._prototype_source("prototype_histograms", modality, case_indices)
        labels, _ = cluster.assign_kmeans(src, centroids)
        hist = MF.kmeans_hist(labels, src.cu, centroids.shape[0]).to(torch.float32)
        if normalize:
            hist = hist / hist.sum(1, keepdim=True).clamp(min=1.0)
        return self._embedding_result(hist, cases)

    def embed(self, model, modality=0, case_indices=None, bags_per_launch=None, max_tokens=None, precision=None, host_wgs=0,
              rank=False) -> dict:
        """The slide embedding of one stain's bag of every case asked for (None: every case that has the stain), from `model`'s H&E
        encoder: {"embeds" [n, 512] fp32 on the device, "cases", "slide_ids"} -- utils.run_inference for a cohort in the store, without
        a dataloader, an h5 read or a host-to-device copy of features.  Eval mode under torch.no_grad() (the model's training flag is
        restored), under autocast when precision is bfloat16 / float16.  Grouping is run_inference's: up to bags_per_launch bags per
        launch set (None: 4 in fp32, 1 under autocast, for the reason its docstring gives), a bag of at most 256 rows alone; each
        group is pack_modality -> model.encode_packed, and every embedding equals model.encode_he of that bag alone bit for bit in
        fp32.  The embeddings stay on the device and the loop reads nothing back.  max_tokens, counter 0: pack_modality's cut.  A
        model with stain encoding takes modality 0 only (encode_he is the H&E path).  rank=True adds "rank" as in mean_embeddings: what
        run_inference returns beside the embeddings, without their copy to the host or the CPU SVD."""
        self._require_device("embed")
        if getattr(model, "stain_encoding", False) and modality != 0:
            raise ValueError("DeviceSlideStore.embed: a model with stain encoding embeds modality 0 only (encode_he is the H&E path; "
                             "got modality %r)" % (modality,))
        cases, _, lens = self._modality_plan(case_indices, modality, max_tokens)
        reduced = precision in (torch.bfloat16, torch.float16)
        groups = self._launch_groups(cases, lens, bags_per_launch, reduced)
        was_training = model.training
        model.eval()
        outs = []
        try:
            with torch.no_grad():
                for group in groups:
                    packed = self.pack_modality(group, modality, max_tokens, host_wgs=host_wgs)
                    with torch.autocast(device_type="cuda", dtype=precision if reduced else None, enabled=reduced):
                        outs.append(model.encode_packed(packed, self.device).float())
        finally:
            model.train(was_training)
        embeds = torch.cat(outs) if outs else torch.zeros(0, 512, dtype=torch.float32, device=self.device)
        return self._embedding_result(embeds, cases, rank)

    def embed_modality(self, model, modality, case_indices=None, bags_per_launch=None, max_tokens=None, precision=None,
                       host_wgs=0) -> dict:
        """embed() for ANY stain of any model: the same result dict, planning, grouping, eval mode under torch.no_grad() (the training
        flag is restored) and autocast rule.  A model without stain encoding goes through encode_packed, as embed() does.  A model with
        stain encoding goes through attend_packed(..., stain_idx=modality): every bag gets embedding(modality), H&E index 0 -- the
        reference's eval-branch rule (Model.py:162-203) -- which is what embed() refuses for modality != 0.  What cross-stain retrieval
        (madeleine_amd.retrieval.cross_stain_retrieval) embeds both sides with."""
        self._require_device("embed_modality")
        cases, _, lens = self._modality_plan(case_indices, modality, max_tokens)
        reduced = precision in (torch.bfloat16, torch.float16)
        groups = self._launch_groups(cases, lens, bags_per_launch, reduced)
        stained = bool(getattr(model, "stain_encoding", False))
        was_training = model.training
        model.eval()
        outs = []
        try:
            with torch.no_grad():
                for group in groups:
                    packed = self.pack_modality(group, modality, max_tokens, host_wgs=host_wgs)
                    with torch.autocast(device_type="cuda", dtype=precision if reduced else None, enabled=reduced):
                        e = model.attend_packed(packed, self.device, stain_idx=modality)[0] if stained \
                            else model.encode_packed(packed, self.device)
                    outs.append(e.float())
        finally:
            model.train(was_training)
        embeds = torch.cat(outs) if outs else torch.zeros(0, 512, dtype=torch.float32, device=self.device)
        return self._embedding_result(embeds, cases)

    @staticmethod
    def _launch_groups(cases, lens, bags_per_launch, reduced):
        """embed's grouping (run_inference's): up to bags_per_launch bags per launch set (None: 4 in fp32, 1 under autocast), a bag of at
        most 256 rows alone."""
        if bags_per_launch is None:
            bags_per_launch = 1 if reduced else 4
        groups, pending = [], []
        for c, n_rows in zip(cases.tolist(), lens.tolist()):
            if bags_per_launch <= 1 or n_rows <= 256:
                if pending:
                    groups.append(pending)
                groups.append([c])
                pending = []
                continue
            pending.append(c)
            if len(pending) >= bags_per_launch:
                groups.append(pending)
                pending = []
        if pending:
            groups.append(pending)
        return groups

    def attention(self, model, modality=0, case_indices=None, topk=0, percentile=True, bags_per_launch=None, precision=None,
                  host_wgs=0) -> dict:
        """The attention maps of one stain's bag of every case asked for (None: every case that has the stain), with the embeddings
        they belong to: embed()'s planning, grouping, eval mode under torch.no_grad() (the training flag is restored) and autocast rule,
        through model.attend_packed, whole bags only.  A model with stain encoding is given stain_idx=modality (the reference's eval
        branch), so any stain works.  Returns, on the device unless said otherwise,
          embeds [n, 512], cases (host), slide_ids      as embed()
          cu_seqlens [n + 1] int64, lens (host list)    bag i of the result is rows cu_seqlens[i] .. cu_seqlens[i + 1] - 1 below
          raw [T, H]                                    the scores before the activation; row j of a bag is row j of its stored bag
                                                        (of its h5 `features` and `coords`)
          attention [T, H]                              the softmax over the bag per head; for the relu, leaky_relu and sigmoid
                                                        activations abmil.activate applied element-wise
          percentile [T, H] or None                     rankdata(raw, 'average') / n * 100 per bag and head
          order [H, T] int32                            order[h, cu_seqlens[i] + j]: the row of bag i with its j-th highest raw score
          topk_idx, topk_val [n, H, topk] or None       the first topk of order and their raw scores, padded with -1 / -inf
        Ranks and top-k are always of the raw scores.  The softmax, the ranks and the top-k of the whole result come from one launch
        sequence each (functional.attn_softmax / attn_rank); the loop reads nothing back and the result does not depend on
        bags_per_launch."""
        from .abmil import activate
        self._require_device("attention")
        cases, _, lens = self._modality_plan(case_indices, modality)
        reduced = precision in (torch.bfloat16, torch.float16)
        groups = self._launch_groups(cases, lens, bags_per_launch, reduced)
        stain_idx = modality if getattr(model, "stain_encoding", False) else None
        was_training = model.training
        model.eval()
        embeds, raws = [], []
        try:
            with torch.no_grad():
                for group in groups:
                    packed = self.pack_modality(group, modality, host_wgs=host_wgs)
                    with torch.autocast(device_type="cuda", dtype=precision if reduced else None, enabled=reduced):
                        e, s = model.attend_packed(packed, self.device, stain_idx=stain_idx)
                    embeds.append(e.float())
                    raws.append(s.float())
        finally:
            model.train(was_training)
        H = model.wsi_embedders.n_heads
        n = cases.numel()
        cu = torch.zeros(n + 1, dtype=torch.int64)
        torch.cumsum(lens, 0, out=cu[1:])
        res = self._embedding_result(torch.cat(embeds) if embeds else torch.zeros(0, 512, dtype=torch.float32, device=self.device), cases)
        raw = torch.cat(raws).contiguous() if raws else torch.zeros(0, H, dtype=torch.float32, device=self.device)
        cu_d = MF.h2d(cu, self.device)
        act = model.wsi_embedders.attn[0].activation
        attention = MF.attn_softmax(raw, cu_d)[0] if act == 'softmax' else activate(raw, act)
        order, pct, ti, tv = MF.attn_rank(raw, cu_d, k=topk, percentile=percentile)
        res.update(cu_seqlens=cu_d, lens=lens.tolist(), raw=raw, attention=attention, percentile=pct, order=order, topk_idx=ti,
                   topk_val=tv)
        return res

    def heatmaps(self, model, modality=0, case_indices=None, source='percentile', heads='mean', downsample=None, sigma=0.0, cmap='jet',
                 alpha=255, thumbnails=None, crop=False, max_bytes=None, bags_per_launch=None, precision=None, host_wgs=0) -> dict:
        """The attention heatmaps of one stain's bag of every case asked for (None: every case that has the stain), on the device:
        attention()'s planning and read-out, then heatmap.render over the store's coordinates (set_coords).
          source 'percentile'         the value of a patch is its percentile rank / 100 (the CLAM convention)
                 'attention' | 'raw'  the softmax weights | raw scores, min-max per bag and channel on the device (a constant bag: 0.5)
          heads  'mean' | 'all' | h   one channel from the mean over the head axis (taken first, before the min-max and the quantiser),
                                      one channel per head, or head h alone
          downsample                  level-0 pixels per canvas pixel; None: the patch size (the bags asked for must then share one), so
                                      that without overlap a patch is exactly one pixel
          sigma, cmap, alpha, crop    as heatmap.render; thumbnails: per bag an [H, W, 3] uint8 image of its canvas, or None
          max_bytes                   workspace + outputs of one render group stay inside it (None: heatmap.RENDER_BYTES); the images
                                      do not depend on it
        Returns embeds, cases, slide_ids as attention() plus, per bag, rgba [C, H, W, 4] uint8, level [C, H, W] uint16, covered
        [C, H, W] uint8 (lists, on the device) and canvas (W, H, ox, oy), with the downsample used and values [T, C], cu_seqlens."""
        from . import heatmap as HM
        self._require_device("heatmaps")
        if self.coords is None:
            raise RuntimeError("DeviceSlideStore.heatmaps: the store holds no coordinates (set_coords)")
        if source not in ('percentile', 'attention', 'raw'):
            raise ValueError("DeviceSlideStore.heatmaps: source must be 'percentile', 'attention' or 'raw' (got %r)" % (source,))
        att = self.attention(model, modality, case_indices, topk=0, percentile=source == 'percentile', bags_per_launch=bags_per_launch,
                             precision=precision, host_wgs=host_wgs)
        cases, cu = att["cases"], att["cu_seqlens"]
        values = HM.heat_values(att, source, heads)
        bag = self.bag_table[:, modality].index_select(0, cases).long()
        sizes = self.patch_sizes.index_select(0, bag)
        if downsample is None:
            if sizes.numel() and int(sizes.min()) != int(sizes.max()):
                raise ValueError("DeviceSlideStore.heatmaps: downsample None means the patch size, and the bags asked for have patch "
                                 "sizes %d .. %d" % (int(sizes.min()), int(sizes.max())))
            downsample = int(sizes[0]) if sizes.numel() else 1
        out = HM.render(self.coords_of(cases, modality), cu, values, sizes, downsample, sigma, cmap, alpha, thumbnails, crop,
                        extents=self.coord_extents.index_select(0, bag), max_bytes=HM.RENDER_BYTES if max_bytes is None else max_bytes,
                        lens=att["lens"])
        res = {k: att[k] for k in ("embeds", "cases", "slide_ids", "cu_seqlens", "lens")}
        res.update(out, values=values)
        return res

    @staticmethod
    def _column_blocks(C):
        """C columns as blocks of 8, 4, 2 and 1: the widths functional.attn_rank serves, read in place through its row stride."""
        blocks, c0 = [], 0
        for w in (8, 4, 2, 1):
            while C - c0 >= w:
                blocks.append((c0, w))
                c0 += w
        return blocks

    def contributions(self, model, W, b=None, modality=0, case_indices=None, topk=0, per_head=False, bags_per_launch=None,
                      precision=None, host_wgs=0) -> dict:
        """Which patches made the linear decision z = W . embedding + b of one stain's bag of every case asked for: the exact split of z
        into one signed term per patch (include/madeleine_amd_explain.h), with attention()'s planning, grouping, eval mode under
        torch.no_grad() (the training flag is restored), autocast rule and stain rule, through model.explain_packed.  W, b: as
        MADELEINE.slide_directions ([d], [C, d], or a slice of fit_logistic's / fit_cox's weights and biases), at most
        functional.CONTRIB_MAX_C rows.  The token embeddings of one group are dropped before the next group is packed.  Returns, on the
        device unless said otherwise,
          embeds, cases, slide_ids, cu_seqlens, lens, raw, attention      as attention()
          contribution [T, C]                           the share of every patch in every decision column
          per_head [T, H, C] or None                    the same per attention head (contribution = the heads added in ascending order)
          const [C]                                     W . projector.bias + b: what no patch accounts for
          decision [n, C]                               embeds . W^T + b, so that stats[:, 0] + const = decision up to rounding
          stats [n, 4, C]                               per bag and column: sum, sum of the positive terms, sum of the negative terms,
                                                        max |.| (functional.CONTRIB_STATS)
          top_pos_idx, top_pos_val [n, C, topk]         the topk most positive patches per bag and column: the row inside the bag and
          top_neg_idx, top_neg_val [n, C, topk]         its contribution; likewise the most negative.  Ties: the lower row first; a
                                                        bag shorter than topk is padded with -1 and -inf / +inf.  None for topk == 0
        The statistics and the top-k of the whole result come from one launch sequence each (functional.contrib_stats / attn_rank);
        the loop reads nothing back and the result does not depend on bags_per_launch."""
        self._require_device("contributions")
        cases, _, lens = self._modality_plan(case_indices, modality)
        reduced = precision in (torch.bfloat16, torch.float16)
        groups = self._launch_groups(cases, lens, bags_per_launch, reduced)
        stain_idx = modality if getattr(model, "stain_encoding", False) else None
        rows, bias = model.decision_rows(W, b)
        U, const = model.slide_directions(rows, bias)
        C, H = U.shape[0], model.wsi_embedders.n_heads
        was_training = model.training
        model.eval()
        parts = [[], [], [], [], []]      # embeds, raw, attention, contribution, per_head
        try:
            with torch.no_grad():
                for group in groups:
                    packed = self.pack_modality(group, modality, host_wgs=host_wgs)
                    with torch.autocast(device_type="cuda", dtype=precision if reduced else None, enabled=reduced):
                        out = model.explain_packed(packed, self.device, U, stain_idx=stain_idx, per_head=per_head)
                    for acc, t in zip(parts, out):
                        acc.append(t.float())
        finally:
            model.train(was_training)
        n = cases.numel()
        cu = torch.zeros(n + 1, dtype=torch.int64)
        torch.cumsum(lens, 0, out=cu[1:])
        cu_d = MF.h2d(cu, self.device)

        def joined(acc, *shape):
            return torch.cat(acc).contiguous() if acc else torch.zeros(*shape, dtype=torch.float32, device=self.device)

        res = self._embedding_result(joined(parts[0], 0, 512), cases)
        contribution = joined(parts[3], 0, C)
        with torch.no_grad(), torch.autocast(device_type="cuda", enabled=False):
            rows4 = torch.cat([rows, rows.new_zeros(-C % 4, rows.shape[1])]).contiguous()      # functional.linear: row counts in fours
            decision = torch.cat([MF.linear(e, rows4)[:, :C] for e in res["embeds"].split(256)]) + bias if n else \
                torch.zeros(0, C, dtype=torch.float32, device=self.device)
        res.update(cu_seqlens=cu_d, lens=lens.tolist(), raw=joined(parts[1], 0, H), attention=joined(parts[2], 0, H),
                   contribution=contribution, per_head=joined(parts[4], 0, H, C) if per_head else None, const=const, decision=decision,
                   stats=MF.contrib_stats(contribution, cu_d), top_pos_idx=None, top_pos_val=None, top_neg_idx=None, top_neg_val=None)
        k = int(topk)
        if k > 0:
            negated = -contribution
            for name, src, sign in (("top_pos", contribution, 1.0), ("top_neg", negated, -1.0)):
                idx, val = [], []
                for c0, w in self._column_blocks(C):
                    _, _, ti, tv = MF.attn_rank(src[:, c0:c0 + w], cu_d, k=k, percentile=False)
                    idx.append(ti)
                    val.append(tv * sign)
                res[name + "_idx"], res[name + "_val"] = torch.cat(idx, 1), torch.cat(val, 1)
        return res

    def contribution_maps(self, model, W, b=None, modality=0, case_indices=None, columns=None, downsample=None, sigma=0.0,
                          cmap='coolwarm', alpha=255, thumbnails=None, crop=False, max_bytes=None, bags_per_launch=None, precision=None,
                          host_wgs=0) -> dict:
        """Signed evidence maps of the linear decision z = W . embedding + b: contributions(), then heatmap.render over the store's
        coordinates exactly as heatmaps() calls it, one channel per decision column (columns: a list of column indices, None: all).
        The value of a patch is 0.5 + 0.5 c / max_t |c| per bag and column, so that no evidence is the midpoint of a diverging
        colour map ('coolwarm': evidence against is blue, for is red), the strongest patch of the bag reaches one end, and a bag
        without any evidence is 0.5 everywhere.  A NaN contribution stays NaN (the renderer leaves such a patch out); it makes
        max |.| of its bag and column NaN too, so that whole channel of the bag is left out.  Returns contributions()'s bag-level keys
        (embeds, cases, slide_ids, cu_seqlens, lens, const, decision, stats) plus render's rgba, level, covered, canvas and
        downsample, and values [T, len(columns)]."""
        from . import heatmap as HM
        self._require_device("contribution_maps")
        if self.coords is None:
            raise RuntimeError("DeviceSlideStore.contribution_maps: the store holds no coordinates (set_coords)")
        con = self.contributions(model, W, b, modality, case_indices, bags_per_launch=bags_per_launch, precision=precision,
                                 host_wgs=host_wgs)
        cases, cu = con["cases"], con["cu_seqlens"]
        c, amax = con["contribution"], con["stats"][:, MF.CONTRIB_STATS.index("absmax")]
        if columns is not None:
            cols = [int(j) for j in columns]
            if not cols or min(cols) < 0 or max(cols) >= c.shape[1]:
                raise IndexError("DeviceSlideStore.contribution_maps: columns must name decision columns in [0, %d) (got %r)"
                                 % (c.shape[1], columns))
            sel = MF.h2d(torch.tensor(cols, dtype=torch.long), self.device)
            c, amax = c.index_select(1, sel), amax.index_select(1, sel)
        scale = torch.repeat_interleave(amax, cu[1:] - cu[:-1], dim=0, output_size=c.shape[0])
        values = torch.where(scale == 0, torch.full_like(c, 0.5), 0.5 + 0.5 * c / scale)
        bag = self.bag_table[:, modality].index_select(0, cases).long()
        sizes = self.patch_sizes.index_select(0, bag)
        if downsample is None:
            if sizes.numel() and int(sizes.min()) != int(sizes.max()):
                raise ValueError("DeviceSlideStore.contribution_maps: downsample None means the patch size, and the bags asked for have "
                                 "patch sizes %d .. %d" % (int(sizes.min()), int(sizes.max())))
            downsample = int(sizes[0]) if sizes.numel() else 1
        out = HM.render(self.coords_of(cases, modality), cu, values, sizes, downsample, sigma, cmap, alpha, thumbnails, crop,
                        extents=self.coord_extents.index_select(0, bag), max_bytes=HM.RENDER_BYTES if max_bytes is None else max_bytes,
                        lens=con["lens"])
        res = {k: con[k] for k in ("embeds", "cases", "slide_ids", "cu_seqlens", "lens", "const", "decision", "stats")}
        res.update(out, values=values)
        return res

    def packed_batches(self, batch_size, max_tokens=None, shuffle=True, drop_last=False, seed=0, rank=0, world_size=1, prefetch=None):
        """Re-iterable over {'packed': PackedBags, 'modality_labels', 'slide_ids'}: the ragged batches of ragged_batches() in packed
        form, from a store of any dtype, every bag cut to at most max_tokens rows.  Plan, sharding, set_epoch and the draw counter are
        those of batches(), and so is prefetch."""
        if max_tokens is not None and max_tokens < 1:
            raise ValueError("DeviceSlideStore: max_tokens must be at least 1 (got %s)" % max_tokens)
        return StoreBatches(self, batch_size, None, shuffle, drop_last, seed, rank, world_size, ragged=True, packed=True,
                            max_tokens=max_tokens, prefetch=prefetch)

    def _side_stream(self):
        """The store's one prefetch stream (a process has few hardware queues: it is never made per epoch or per iterator)."""
        if self._side is None:
            self._side = torch.cuda.Stream(self.device)
        return self._side

    def _absent_bag(self) -> torch.Tensor:
        if self._zero_bag is None:
            self._zero_bag = torch.zeros(2, self.dim, dtype=torch.float32, device=self.device)
        return self._zero_bag


def _unregister(rt, ptr, raw):
    rt.cudaHostUnregister(ptr)
    del raw


class StoreBatches:
    """What DeviceSlideStore.batches / ragged_batches / packed_batches return.  plan(epoch) is host-only and a function of (seed,
    epoch, rank, world_size): rank r owns the static shard r::world_size of the cases and shuffles inside it.  The draw counter of a
    batch is (epoch, batch number), so a run resumed at an epoch redraws the same batches.  set_epoch(e) before each epoch, as with
    DistributedSampler.

    prefetch = k >= 1 (dense and packed batches): when batch i is yielded the gathers of batches i + 1 .. i + k of the same epoch's plan,
    table uploads included, are already queued on the store's side stream.  At yield the current stream waits on the batch's event and
    the tensors are recorded for it, so the consumer uses them at once; the host is never synchronised.  Counters are those of
    prefetch = 0, so the batches are the same bits.  An iterator belongs to the epoch it was made in (prefetch never crosses
    set_epoch); dropping it mid-epoch leaves at most k gathers finishing into tensors nobody reads."""

    def __init__(self, store, batch_size, n_tokens, shuffle, drop_last, seed, rank, world_size, ragged, packed=False,
                 max_tokens=None, prefetch=None):
        if batch_size < 1 or world_size < 1 or not 0 <= rank < world_size:
            raise ValueError("StoreBatches: batch_size >= 1 and 0 <= rank < world_size are required")
        if not ragged and n_tokens < 1:
            raise ValueError("StoreBatches: n_tokens >= 1 is required")
        self.store, self.batch_size, self.n_tokens = store, int(batch_size), n_tokens
        self.shuffle, self.drop_last, self.seed = bool(shuffle), bool(drop_last), int(seed)
        self.rank, self.world_size, self.ragged = int(rank), int(world_size), bool(ragged)
        self.packed, self.max_tokens = bool(packed), max_tokens
        if prefetch is None:
            prefetch = 1 if store.rows_host is not None else 0
        if isinstance(prefetch, bool) or not isinstance(prefetch, int) or prefetch < 0:
            raise ValueError("StoreBatches: prefetch must be None or an integer >= 0 (got %r)" % (prefetch,))
        self.prefetch = prefetch if (self.packed or not self.ragged) else 0      # zero-copy views have nothing to fetch
        self.epoch = 0

    def set_epoch(self, epoch: int):
        self.epoch = int(epoch)

    def _shard(self) -> List[int]:
        return list(range(self.rank, len(self.store), self.world_size))

    def __len__(self):
        n = len(self._shard())
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def plan(self, epoch: Optional[int] = None) -> List[List[int]]:
        """The case indices of every batch of `epoch` (default: the current one), in order."""
        epoch = self.epoch if epoch is None else int(epoch)
        cases = self._shard()
        if self.shuffle:
            g = torch.Generator().manual_seed((self.seed * 1000003 + epoch) % (2 ** 63))
            cases = [cases[i] for i in torch.randperm(len(cases), generator=g).tolist()]
        out = [cases[i:i + self.batch_size] for i in range(0, len(cases), self.batch_size)]
        if self.drop_last and out and len(out[-1]) < self.batch_size:
            out.pop()
        return out

    def _batch(self, epoch, batch_no, cases):
        """Batch `batch_no` of `epoch`, gathered on the current stream."""
        st = self.store
        out = {"modality_labels": st.modality_labels.index_select(0, torch.tensor(cases, dtype=torch.int64)),
               "slide_ids": [st.slide_ids[c] for c in cases]}
        if self.packed:
            out["packed"] = st.pack(cases, self.max_tokens, counter=(epoch << 32) | batch_no, seed=self.seed)
        elif self.ragged:
            out["bags"] = [[st.bag_view(c, m) if int(st.bag_table[c, m]) >= 0 else st._absent_bag()
                            for m in range(len(st.modalities))] for c in cases]
        else:
            out["feats"] = st.sample(cases, self.n_tokens, counter=(epoch << 32) | batch_no, seed=self.seed)
        return out

    def __iter__(self):
        epoch, plan = self.epoch, self.plan(self.epoch)
        if self.prefetch == 0:
            for batch_no, cases in enumerate(plan):
                yield self._batch(epoch, batch_no, cases)
            return
        side, queued = self.store._side_stream(), collections.deque()
        for batch_no in range(len(plan)):
            while len(queued) <= self.prefetch and batch_no + len(queued) < len(plan):
                nxt = batch_no + len(queued)
                with torch.cuda.stream(side):
                    out = self._batch(epoch, nxt, plan[nxt])
                    done = torch.cuda.Event()
                    done.record(side)
                queued.append((out, done))
            out, done = queued.popleft()
            cur = torch.cuda.current_stream(self.store.device)
            cur.wait_event(done)
            p = out.get("packed")
            for t in (out["feats"],) if p is None else (p.tokens, p.cu_seqlens, p.row_bag):
                t.record_stream(cur)                            # allocated on the side stream, used on this one
            yield out
