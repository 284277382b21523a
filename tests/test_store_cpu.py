"""The device-resident slide store without a GPU: the mdl_bag_sample entry point (declared, bound, exported, argument refusals before
any launch), the ABI revision, the packing of a store built on the CPU, the refusal to sample there, and the host-only batch plans."""
import ctypes

import pytest
import torch

import madeleine_amd
from madeleine_amd import _build, _native
from madeleine_amd import functional as MF
from madeleine_amd.store import DeviceSlideStore, StoreBatches

E_ARG, E_ALIGN, E_UNSUP = -1, -2, -3
MODS = ["HE", "HER2", "PGR"]


@pytest.fixture(scope="module")
def lib():
    return _native.lib()


def test_entry_point_is_declared_bound_and_exported(lib):
    with open(_build.HEADER) as f:
        header = f.read()
    assert "mdl_bag_sample(" in header and "wsi_dataset.py" in header
    res, args = _native.SIGNATURES["mdl_bag_sample"]
    fn = lib.mdl_bag_sample
    assert fn.restype is res and list(fn.argtypes) == list(args)
    P, I, L, U = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64
    assert res is I and args == [P, I, L, L, P, L, P, P, L, I, I, U, U, P, P, P]
    assert [_native._DEFINES["MDL_STORE_" + k] for k in ("F32", "F16", "BF16")] == [0, 1, 2]
    assert MF.STORE_DTYPES == {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
    assert madeleine_amd.DeviceSlideStore is DeviceSlideStore and "DeviceSlideStore" in madeleine_amd.__all__


def test_abi_version_is_still_26(lib):
    assert _native.ABI_VERSION == 26 and lib.mdl_abi_version() == 26


def test_launcher_refuses_bad_arguments_before_any_launch(lib):
    raw = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(raw) + 15) & ~15          # host memory: a launch on it would fault, so every case below must refuse first
    good = dict(store=p, dtype=0, stride=8, T=4, off=p + 64, n_bags=1, bag=p + 96, key=p + 128, R=2, N=3, D=8, seed=1, ctr=2, out=p + 16,
                idx=p + 160)

    def call(**kw):
        a = dict(good, **kw)
        return lib.mdl_bag_sample(a["store"], a["dtype"], a["stride"], a["T"], a["off"], a["n_bags"], a["bag"], a["key"], a["R"], a["N"],
                                  a["D"], a["seed"], a["ctr"], a["out"], a["idx"], None)
    for name in ("store", "off", "bag", "out"):
        assert call(**{name: None}) == E_ARG, name
    assert call(R=-1) == E_ARG and call(N=0) == E_ARG and call(N=-5) == E_ARG and call(D=0) == E_ARG and call(D=-1) == E_ARG
    assert call(dtype=3) == E_ARG and call(dtype=-1) == E_ARG
    assert call(T=-1) == E_ARG and call(n_bags=-1) == E_ARG and call(stride=7) == E_ARG
    assert call(out=p + 20) == E_ALIGN and call(out=p + 8) == E_ALIGN and call(store=p + 4) == E_ALIGN
    assert call(off=p + 68) == E_ALIGN and call(bag=p + 98) == E_ALIGN
    # an optional idx_out / key_id does not soften the other checks
    assert call(idx=None, key=None, out=p + 8) == E_ALIGN and call(idx=None, key=None, N=0) == E_ARG
    assert call(R=2 ** 20, N=2 ** 11) == E_UNSUP                # R * N = 2^31
    assert call(R=2 ** 31, N=1) == E_UNSUP and call(R=2 ** 40, N=4096) == E_UNSUP
    assert call(R=0) == 0 and call(R=0, idx=None, key=None) == 0     # nothing to draw: no launch


def _bags():
    g = torch.Generator().manual_seed(0)
    r = lambda n: torch.randn(n, 6, generator=g)      # noqa: E731
    return [[r(5), None, r(3)], [r(2), r(7), None], [r(1), None, None], [r(4), r(4), r(9)]]


def test_packing_on_a_cpu_store():
    bags = _bags()
    st = DeviceSlideStore(bags, ["a", "b", "c", "d"], MODS, "cpu")
    assert len(st) == 4 and st.dim == 6 and st.n_bags == 8 and st.rows.shape == (35, 6) and st.rows.dtype == torch.float32
    assert st.off_cpu.tolist() == [0, 5, 8, 10, 17, 18, 22, 26, 35] and torch.equal(st.off, st.off_cpu) and st.off.dtype == torch.int64
    assert st.bag_table.dtype == torch.int32 and st.bag_table.tolist() == [[0, -1, 1], [2, 3, -1], [4, -1, -1], [5, 6, 7]]
    assert st.modality_labels.dtype == torch.float32
    assert st.modality_labels.tolist() == [[1, 0, 1], [1, 1, 0], [1, 0, 0], [1, 1, 1]]
    for c, case in enumerate(bags):
        for m, bag in enumerate(case):
            view = st.bag_view(c, m)
            if bag is None:
                assert view is None
            else:
                assert torch.equal(view, bag) and view.data_ptr() == st.rows[int(st.off_cpu[st.bag_table[c, m]])].data_ptr()
    assert st.nbytes() == 35 * 6 * 4
    half = DeviceSlideStore(bags, ["a", "b", "c", "d"], MODS, "cpu", dtype=torch.bfloat16)
    assert half.rows.dtype == torch.bfloat16 and half.nbytes() == 35 * 6 * 2 and torch.equal(half.bag_view(3, 2), bags[3][2].bfloat16())


def test_packing_refusals():
    bags = _bags()
    ids = ["a", "b", "c", "d"]
    wide = [list(c) for c in bags]
    wide[1][1] = torch.zeros(7, 5)
    with pytest.raises(ValueError, match=r"case 1 \(b\), modality HER2 is 5 wide.*6 wide"):
        DeviceSlideStore(wide, ids, MODS, "cpu")
    big = [list(c) for c in bags]
    big[3][2] = big[3][2].clone()
    big[3][2][4, 1] = 70000.0
    with pytest.raises(ValueError, match=r"case 3 \(d\), modality PGR has absmax 70000.*float16"):
        DeviceSlideStore(big, ids, MODS, "cpu", dtype=torch.float16)
    assert DeviceSlideStore(big, ids, MODS, "cpu", dtype=torch.bfloat16).rows.dtype == torch.bfloat16     # bf16 has fp32's range
    assert DeviceSlideStore(big, ids, MODS, "cpu").rows[26 + 4, 1] == 70000.0
    ok16 = DeviceSlideStore(bags, ids, MODS, "cpu", dtype=torch.float16)
    assert torch.equal(ok16.bag_view(0, 0), bags[0][0].half())
    empty = [list(c) for c in bags]
    empty[0][0] = torch.zeros(0, 6)
    with pytest.raises(ValueError, match="0 rows"):
        DeviceSlideStore(empty, ids, MODS, "cpu")
    with pytest.raises(ValueError, match="slide ids"):
        DeviceSlideStore(bags, ids[:3], MODS, "cpu")
    with pytest.raises(ValueError, match="2 modalities"):
        DeviceSlideStore(bags, ids, MODS[:2], "cpu")
    with pytest.raises(ValueError, match="dtype"):
        DeviceSlideStore(bags, ids, MODS, "cpu", dtype=torch.float64)
    with pytest.raises(ValueError, match="no present bag"):
        DeviceSlideStore([[None, None, None]], ["a"], MODS, "cpu")


def test_from_dataset_keeps_present_bags_and_drops_zero_bags():
    import pandas as pd
    from madeleine_amd.data import SlideDataset
    df = pd.DataFrame({"slide_id": ["a", "b"], "HE": [1, 1], "HER2": [1, 0], "PGR": [0, 1], "split": ["train"] * 2})
    feats = {"a_HE": torch.ones(5, 4), "a_HER2": torch.full((3, 4), 2.0), "b_HE": torch.full((2, 4), 3.0), "b_PGR": torch.full((6, 4), 4.0)}
    loads = []

    def loader(path):
        loads.append(path)
        return feats[path.rsplit("/", 1)[-1][:-3]]
    ds = SlideDataset("toy", None, "/feats", MODS, embedding_size=4, sample=-1, dataframe=df, feature_loader=loader)
    st = DeviceSlideStore.from_dataset(ds, "cpu")
    assert len(loads) == 4                                        # one pass: every present stain is read once
    assert st.slide_ids == ["a", "b"] and st.modalities == MODS and st.off_cpu.tolist() == [0, 5, 8, 10, 16]
    assert st.bag_table.tolist() == [[0, 1, -1], [2, -1, 3]] and torch.equal(st.rows[8:10], feats["b_HE"])
    with pytest.raises(ValueError, match="sample=-1"):
        DeviceSlideStore.from_dataset(SlideDataset("toy", None, "/feats", MODS, embedding_size=4, sample=8, dataframe=df,
                                                   feature_loader=loader), "cpu")


def test_sampling_a_cpu_store_raises():
    st = DeviceSlideStore(_bags(), ["a", "b", "c", "d"], MODS, "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        st.sample([0, 1], 4, counter=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        next(iter(st.batches(2, 4)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MF.bag_sample(st.rows, st.off, torch.zeros(1, dtype=torch.int32), None, 4, 0, 0)
    with pytest.raises(ValueError, match="float32 store"):
        DeviceSlideStore(_bags(), ["a", "b", "c", "d"], MODS, "cpu", dtype=torch.bfloat16).ragged_batches(2)
    # the ragged route needs no kernel: it runs on a CPU store, with ragged_collate's keys and the views of the store
    batch = next(iter(st.ragged_batches(2, shuffle=False)))
    assert set(batch) == {"bags", "modality_labels", "slide_ids"} and batch["slide_ids"] == ["a", "b"]
    assert batch["bags"][0][0].data_ptr() == st.rows.data_ptr() and batch["bags"][0][1].shape == (2, 6) and not batch["bags"][0][1].any()
    assert batch["modality_labels"].tolist() == [[1, 0, 1], [1, 1, 0]]


def _plan_store(n=11):
    return DeviceSlideStore([[torch.zeros(1, 2)] for _ in range(n)], ["s%d" % i for i in range(n)], ["HE"], "cpu")


def test_plan_covers_every_case_once_and_is_deterministic():
    st = _plan_store(11)
    it = st.batches(4, 8, seed=3)
    assert isinstance(it, StoreBatches) and len(it) == 3
    plan = it.plan(0)
    assert [len(b) for b in plan] == [4, 4, 3] and sorted(c for b in plan for c in b) == list(range(11))
    dropped = st.batches(4, 8, seed=3, drop_last=True)
    assert len(dropped) == 2 and dropped.plan(0) == plan[:2]
    assert it.plan(1) != plan and sorted(c for b in it.plan(1) for c in b) == list(range(11))        # epochs differ
    assert st.batches(4, 8, seed=3).plan(0) == plan and st.batches(4, 8, seed=3).plan(1) == it.plan(1)  # equal (seed, epoch): equal plan
    assert st.batches(4, 8, seed=4).plan(0) != plan
    it.set_epoch(1)
    assert it.plan() == it.plan(1)
    assert st.batches(4, 8, shuffle=False).plan(5) == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10]]
    assert len(st.batches(11, 8)) == 1 and len(st.batches(12, 8, drop_last=True)) == 0 and st.batches(12, 8, drop_last=True).plan(0) == []


@pytest.mark.parametrize("world", [2, 3])
def test_plan_shards_are_disjoint_and_cover_the_cohort(world):
    st = _plan_store(11)
    seen = []
    for rank in range(world):
        it = st.batches(2, 8, seed=1, rank=rank, world_size=world)
        for epoch in (0, 1):
            cases = [c for b in it.plan(epoch) for c in b]
            assert sorted(cases) == list(range(rank, 11, world))          # the static shard rank::world, shuffled inside
        assert len(it) == len(it.plan(0))
        seen += [c for b in it.plan(0) for c in b]
    assert sorted(seen) == list(range(11))
    with pytest.raises(ValueError):
        st.batches(2, 8, rank=world, world_size=world)
