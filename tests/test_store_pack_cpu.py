"""The packed ragged route of the slide store without a GPU: the mdl_bag_pack entry point (declared, bound, exported, argument refusals
before any launch), the ABI revision, pack_lens and the packed batch plans on a store built on the CPU, and the refusal to pack there."""
import ctypes

import pytest
import torch

import madeleine_amd
from madeleine_amd import _build, _native
from madeleine_amd import functional as MF
from madeleine_amd.store import DeviceSlideStore, PackedBags, StoreBatches

E_ARG, E_ALIGN, E_UNSUP = -1, -2, -3
MODS = ["HE", "HER2", "PGR"]


@pytest.fixture(scope="module")
def lib():
    return _native.lib()


def test_entry_point_is_declared_bound_and_exported(lib):
    with open(_build.HEADER) as f:
        header = f.read()
    assert "mdl_bag_pack(" in header and " * S2 -- " in header
    res, args = _native.SIGNATURES["mdl_bag_pack"]
    fn = lib.mdl_bag_pack
    assert fn.restype is res and list(fn.argtypes) == list(args)
    P, I, L, U = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64
    #                       store dtype stride T_total off n_bags bag key cu chunk_cu R n_chunks T_out D seed ctr out row_bag idx stream
    assert res is I and args == [P, I, L, L, P, L, P, P, P, P, L, L, L, I, U, U, P, P, P, P]
    assert hasattr(ctypes.CDLL(_native.lib_path()), "mdl_bag_pack")
    assert madeleine_amd.PackedBags is PackedBags and "PackedBags" in madeleine_amd.__all__
    assert PackedBags._fields == ("tokens", "cu_seqlens", "lens", "row_bag", "idx")
    assert callable(MF.bag_pack)


def test_abi_version_is_still_26(lib):
    assert _native.ABI_VERSION == 26 and lib.mdl_abi_version() == 26


def test_launcher_refuses_bad_arguments_before_any_launch(lib):
    raw = ctypes.create_string_buffer(512)
    p = (ctypes.addressof(raw) + 15) & ~15          # host memory: a launch on it would fault, so every case below must refuse first
    good = dict(store=p, dtype=0, stride=8, T=4, off=p + 64, n_bags=1, bag=p + 96, key=p + 128, cu=p + 192, chunk=p + 256, R=2, chunks=2,
                T_out=5, D=8, seed=1, ctr=2, out=p + 16, row_bag=p + 320, idx=p + 384)

    def call(**kw):
        a = dict(good, **kw)
        return lib.mdl_bag_pack(a["store"], a["dtype"], a["stride"], a["T"], a["off"], a["n_bags"], a["bag"], a["key"], a["cu"], a["chunk"],
                                a["R"], a["chunks"], a["T_out"], a["D"], a["seed"], a["ctr"], a["out"], a["row_bag"], a["idx"], None)
    for name in ("store", "off", "bag", "cu", "chunk", "out"):
        assert call(**{name: None}) == E_ARG, name
    assert call(R=-1) == E_ARG and call(T_out=-1) == E_ARG and call(chunks=-1) == E_ARG and call(D=0) == E_ARG and call(D=-1) == E_ARG
    assert call(dtype=3) == E_ARG and call(dtype=-1) == E_ARG
    assert call(T=-1) == E_ARG and call(n_bags=-1) == E_ARG and call(stride=7) == E_ARG
    assert call(out=p + 20) == E_ALIGN and call(out=p + 8) == E_ALIGN and call(store=p + 4) == E_ALIGN
    assert call(off=p + 68) == E_ALIGN and call(bag=p + 98) == E_ALIGN and call(key=p + 132) == E_ALIGN
    assert call(cu=p + 196) == E_ALIGN and call(chunk=p + 260) == E_ALIGN
    assert call(row_bag=p + 322) == E_ALIGN and call(idx=p + 386) == E_ALIGN
    # the optional row_bag / idx_out / key_id do not soften the other checks
    assert call(idx=None, row_bag=None, key=None, out=p + 8) == E_ALIGN and call(idx=None, row_bag=None, key=None, D=0) == E_ARG
    assert call(T_out=2 ** 31) == E_UNSUP and call(chunks=2 ** 31) == E_UNSUP and call(R=2 ** 31) == E_UNSUP
    assert call(T_out=2 ** 40, chunks=2 ** 34) == E_UNSUP
    # nothing to pack: no launch
    assert call(R=0) == 0 and call(T_out=0) == 0 and call(chunks=0) == 0 and call(R=0, idx=None, row_bag=None, key=None) == 0


def _bags():
    g = torch.Generator().manual_seed(0)
    r = lambda n: torch.randn(n, 6, generator=g)      # noqa: E731
    return [[r(5), None, r(3)], [r(2), r(7), None], [r(1), None, None], [r(4), r(4), r(9)]]


def test_pack_lens_on_a_cpu_store():
    st = DeviceSlideStore(_bags(), ["a", "b", "c", "d"], MODS, "cpu")
    assert st.pack_lens([0, 1, 2, 3]) == [5, 2, 3, 2, 7, 2, 1, 2, 2, 4, 4, 9]              # an absent stain: the 2-row zero bag
    assert st.pack_lens([0, 1, 2, 3], max_tokens=4) == [4, 2, 3, 2, 4, 2, 1, 2, 2, 4, 4, 4]   # the cap does not touch the zero bags
    assert st.pack_lens([0, 1, 2, 3], max_tokens=1) == [1, 2, 1, 1, 1, 2, 1, 2, 2, 1, 1, 1]
    assert st.pack_lens([0, 1, 2, 3], max_tokens=100) == st.pack_lens([0, 1, 2, 3])
    assert st.pack_lens([3, 0]) == [4, 4, 9, 5, 2, 3] and st.pack_lens([2, 2], 3) == [1, 2, 2, 1, 2, 2]     # case-major, in the order asked
    assert st.pack_lens([]) == [] and all(type(n) is int for n in st.pack_lens([1]))
    assert st.pack_lens(torch.tensor([1])) == [2, 7, 2]
    half = DeviceSlideStore(_bags(), ["a", "b", "c", "d"], MODS, "cpu", dtype=torch.bfloat16)
    assert half.pack_lens([3, 0], 6) == [4, 4, 6, 5, 2, 3]
    for bad in (0, -3):
        with pytest.raises(ValueError, match="max_tokens"):
            st.pack_lens([0], max_tokens=bad)
    with pytest.raises(IndexError):
        st.pack_lens([4])


def _plan_store(n=11):
    return DeviceSlideStore([[torch.zeros(1, 2)] for _ in range(n)], ["s%d" % i for i in range(n)], ["HE"], "cpu")


def test_packed_batches_share_the_dense_plan():
    st = _plan_store(11)
    for kw in (dict(seed=3), dict(seed=3, drop_last=True), dict(shuffle=False), dict(seed=1, rank=1, world_size=3),
               dict(seed=1, rank=0, world_size=2, drop_last=True)):
        dense, packed = st.batches(4, 8, **kw), st.packed_batches(4, max_tokens=8, **kw)
        assert isinstance(packed, StoreBatches) and len(packed) == len(dense)
        for epoch in (0, 1, 5):
            assert packed.plan(epoch) == dense.plan(epoch)
        packed.set_epoch(2)
        assert packed.plan() == dense.plan(2)
    assert len(st.packed_batches(4)) == 3 and st.packed_batches(4).plan(0) == st.batches(4, 1).plan(0)      # no cap: the same plan
    # a 16-bit store is welcome (ragged_batches refuses it)
    half = DeviceSlideStore(_bags(), ["a", "b", "c", "d"], MODS, "cpu", dtype=torch.bfloat16)
    assert len(half.packed_batches(3)) == 2
    with pytest.raises(ValueError, match="max_tokens"):
        st.packed_batches(4, max_tokens=0)
    with pytest.raises(ValueError):
        st.packed_batches(2, rank=2, world_size=2)


def test_packing_a_cpu_store_raises():
    st = DeviceSlideStore(_bags(), ["a", "b", "c", "d"], MODS, "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        st.pack([0, 1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        st.pack([0, 1], max_tokens=3, counter=1, seed=2, return_indices=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        next(iter(st.packed_batches(2, max_tokens=4)))
    z = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MF.bag_pack(st.rows, st.off, torch.zeros(1, dtype=torch.int32), None, z, z, 1, 1, 0, 0)
