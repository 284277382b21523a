"""The two-tier slide store without a GPU: where resident_bytes puts the split, that the tables and the plan do not depend on it and the
two tiers concatenated are the untiered rows, the zero-copy refusals, the mdl_bag_sample_tiered / mdl_bag_pack_tiered entry points
(declared, bound, exported, refusals that come before any query of the runtime) and the Python-side refusals, the unpinned host tier
among them, which must not reach the native layer.  No test hands the native layer pageable memory as a host tier."""
import ctypes

import pytest
import torch

from madeleine_amd import _build, _native
from madeleine_amd import functional as MF
from madeleine_amd.store import DeviceSlideStore

E_ARG, E_ALIGN, E_UNSUP = -1, -2, -3
MODS = ["HE", "HER2", "PGR"]
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
D = 6
LENS = [[5, None, 3], [2, 7, None], [1, None, None], [4, 4, 9], [None, 6, 8]]      # 5 cases x 3 modalities, 10 stored bags


def _bags():
    g = torch.Generator().manual_seed(0)
    return [[None if n is None else torch.randn(n, D, generator=g) for n in case] for case in LENS]


def _store(dtype=torch.float32, **kw):
    return DeviceSlideStore(_bags(), ["c%d" % i for i in range(len(LENS))], MODS, "cpu", dtype=dtype, **kw)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16", "bf16"])
def test_the_split_is_the_longest_prefix_of_whole_bags_inside_the_budget(dtype):
    ref = _store(dtype)
    off, row_bytes, n_bags = ref.off_cpu.tolist(), D * torch.empty(0, dtype=dtype).element_size(), ref.n_bags
    assert n_bags == 10 and ref.resident_rows == off[-1] and ref.rows_host is None
    assert ref.nbytes() == ref.nbytes("device") == off[-1] * row_bytes and ref.nbytes("host") == 0
    # (budget in bytes, resident bags j): 0; one byte short of the first bag; exactly k whole bags and one byte short of them; >= total
    budgets = [(0, 0), (off[1] * row_bytes - 1, 0)]
    for k in (1, 4, 9, 10):
        budgets += [(off[k] * row_bytes, k), (off[k] * row_bytes - 1, k - 1)]
    budgets += [(off[-1] * row_bytes + 1, n_bags), (1 << 50, n_bags)]
    plan = ref.batches(2, 4, shuffle=True, seed=3).plan(1)
    for budget, j in budgets:
        st = _store(dtype, resident_bytes=budget)
        assert st.resident_rows == off[j], (budget, j)
        assert st.nbytes("device") == off[j] * row_bytes <= budget and st.nbytes("host") == (off[-1] - off[j]) * row_bytes
        assert st.nbytes() == ref.nbytes() and st.rows.shape == (off[j], D) and st.rows.dtype == dtype
        assert (st.rows_host is None) == (j == n_bags)
        assert torch.equal(st.off_cpu, ref.off_cpu) and torch.equal(st.off, ref.off) and torch.equal(st.bag_table, ref.bag_table)
        assert torch.equal(st.modality_labels, ref.modality_labels) and torch.equal(st.bag_lens_cpu, ref.bag_lens_cpu)
        assert st.slide_ids == ref.slide_ids and st.batches(2, 4, shuffle=True, seed=3).plan(1) == plan
        assert st.packed_batches(2, 5, shuffle=True, seed=3).plan(1) == plan and st.pack_lens([0, 3], 5) == ref.pack_lens([0, 3], 5)
        both = st.rows if st.rows_host is None else torch.cat([st.rows, st.rows_host])
        assert both.dtype == dtype and torch.equal(both.view(torch.uint8), ref.rows.view(torch.uint8))          # bit for bit
        if st.rows_host is not None:
            assert st.rows_host.device.type == "cpu" and st.rows_host.shape == (off[-1] - off[j], D) and st.rows_host.is_contiguous()


def test_from_dataset_and_bad_budgets():
    class DS:
        sample, train, modalities = -1, True, MODS

        def __len__(self):
            return len(LENS)

        def __getitem__(self, i):
            case = _bags()[i]
            return {"feats": [torch.zeros(2, D) if b is None else b for b in case], "modality_labels": [int(b is not None) for b in case],
                    "slide_id": "c%d" % i}
    ref = _store()
    st = DeviceSlideStore.from_dataset(DS(), "cpu", resident_bytes=int(ref.off_cpu[3]) * D * 4)
    assert st.resident_rows == int(ref.off_cpu[3]) and torch.equal(torch.cat([st.rows, st.rows_host]), ref.rows)
    for bad in (-1, 1.5, "1", True):
        with pytest.raises(ValueError, match="resident_bytes"):
            _store(resident_bytes=bad)
    with pytest.raises(ValueError, match="tier"):
        ref.nbytes("hbm")


def test_zero_copy_views_of_the_host_tier_are_refused():
    ref = _store()
    off = ref.off_cpu.tolist()
    st = _store(resident_bytes=off[4] * D * 4)                   # bags 0..3 resident: cases 0 and 1
    assert st.resident_rows == off[4]
    assert torch.equal(st.bag_view(0, 0), ref.bag_view(0, 0)) and torch.equal(st.bag_view(1, 1), ref.bag_view(1, 1))
    assert st.bag_view(0, 0).data_ptr() == st.rows.data_ptr()    # still a view
    assert st.bag_view(0, 1) is None and st.bag_view(2, 1) is None          # an absent stain has no tier
    for case, m in ((2, 0), (3, 2), (4, 1)):
        with pytest.raises(ValueError, match="packed_batches"):
            st.bag_view(case, m)
    with pytest.raises(ValueError, match="packed_batches"):
        st.ragged_batches(2)
    with pytest.raises(ValueError, match="packed_batches"):
        _store(resident_bytes=0).ragged_batches(2)
    full = _store(resident_bytes=1 << 40)                        # an empty host tier: today's store
    assert len(list(full.ragged_batches(2, shuffle=False))) == 3 and torch.equal(full.bag_view(4, 2), ref.bag_view(4, 2))
    # prefetch: 1 by default with a host tier, 0 without; ragged views have nothing to fetch
    assert st.batches(2, 4).prefetch == 1 and st.packed_batches(2).prefetch == 1 and st.batches(2, 4, prefetch=0).prefetch == 0
    assert ref.batches(2, 4).prefetch == 0 and ref.packed_batches(2, prefetch=3).prefetch == 3 and full.ragged_batches(2).prefetch == 0
    with pytest.raises(ValueError, match="prefetch"):
        st.batches(2, 4, prefetch=-1)
    for f in (lambda: st.sample([0], 4, 0), lambda: st.pack([0])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f()


def test_entry_points_are_declared_bound_and_exported():
    lib = _native.lib()
    with open(_build.HEADER) as f:
        header = f.read()
    assert "mdl_bag_sample_tiered(" in header and "mdl_bag_pack_tiered(" in header and " * S3, S4 -- " in header
    P, I, L, U = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64
    want = {  # store host dtype stride T_total T_dev off n_bags bag key | R N D | seed ctr out idx host_wgs stream
        "mdl_bag_sample_tiered": [P, P, I, L, L, L, P, L, P, P, L, I, I, U, U, P, P, I, P],
        # ... | cu chunk_cu R n_chunks T_out D | seed ctr out row_bag idx host_wgs stream
        "mdl_bag_pack_tiered": [P, P, I, L, L, L, P, L, P, P, P, P, L, L, L, I, U, U, P, P, P, I, P]}
    handle = ctypes.CDLL(_native.lib_path())
    for name, args in want.items():
        res, got = _native.SIGNATURES[name]
        fn = getattr(lib, name)
        assert res is I and got == args and fn.restype is res and list(fn.argtypes) == args and hasattr(handle, name)
    assert _native.ABI_VERSION == 26 and lib.mdl_abi_version() == 26
    assert callable(MF.bag_sample_tiered) and callable(MF.bag_pack_tiered)


def test_launchers_refuse_bad_arguments_before_any_query_or_launch():
    """Every case is refused on its arguments alone.  store_host is NULL throughout (T_dev == T_total needs none): the runtime is never
    asked about a pointer and pageable memory never stands in for a host tier."""
    lib = _native.lib()
    raw = ctypes.create_string_buffer(512)
    p = (ctypes.addressof(raw) + 15) & ~15
    good = dict(store=p, host=None, dtype=0, stride=8, T=4, T_dev=4, off=p + 64, n_bags=1, bag=p + 96, key=p + 128, cu=p + 192, chunk=p + 256,
                R=2, N=3, chunks=2, T_out=5, D=8, seed=1, ctr=2, out=p + 16, row_bag=p + 320, idx=p + 384, wgs=0)

    def sample(**kw):
        a = dict(good, **kw)
        return lib.mdl_bag_sample_tiered(a["store"], a["host"], a["dtype"], a["stride"], a["T"], a["T_dev"], a["off"], a["n_bags"], a["bag"],
                                         a["key"], a["R"], a["N"], a["D"], a["seed"], a["ctr"], a["out"], a["idx"], a["wgs"], None)

    def pack(**kw):
        a = dict(good, **kw)
        return lib.mdl_bag_pack_tiered(a["store"], a["host"], a["dtype"], a["stride"], a["T"], a["T_dev"], a["off"], a["n_bags"], a["bag"],
                                       a["key"], a["cu"], a["chunk"], a["R"], a["chunks"], a["T_out"], a["D"], a["seed"], a["ctr"], a["out"],
                                       a["row_bag"], a["idx"], a["wgs"], None)
    for call in (sample, pack):
        for name in ("store", "off", "bag", "out"):
            assert call(**{name: None}) == E_ARG, name
        assert call(T_dev=5) == E_ARG and call(T_dev=-1) == E_ARG and call(T=-1) == E_ARG and call(wgs=-1) == E_ARG
        assert call(T_dev=3) == E_ARG and call(T_dev=0) == E_ARG                 # rows in a host tier, and no host tier given
        assert call(R=-1) == E_ARG and call(D=0) == E_ARG and call(dtype=3) == E_ARG and call(n_bags=-1) == E_ARG and call(stride=7) == E_ARG
        assert call(out=p + 8) == E_ALIGN and call(store=p + 4) == E_ALIGN and call(off=p + 68) == E_ALIGN and call(bag=p + 98) == E_ALIGN
        assert call(key=p + 132) == E_ALIGN and call(idx=p + 386) == E_ALIGN
        assert call(host=p + 452) == E_ALIGN and call(dtype=-1) == E_ARG           # a misaligned store_host, even with no row in it
        assert call(R=0) == 0 and call(R=0, store=None, T=0, T_dev=0) == 0        # nothing to do: no launch; an empty store needs no tier
    assert sample(N=0) == E_ARG and sample(N=-5) == E_ARG and sample(R=2 ** 31, N=2) == E_UNSUP
    assert pack(cu=None) == E_ARG and pack(chunk=None) == E_ARG and pack(T_out=-1) == E_ARG and pack(chunks=-1) == E_ARG
    assert pack(cu=p + 196) == E_ALIGN and pack(chunk=p + 260) == E_ALIGN and pack(row_bag=p + 322) == E_ALIGN
    assert pack(T_out=2 ** 31) == E_UNSUP and pack(chunks=2 ** 31) == E_UNSUP and pack(T_out=0) == 0 and pack(chunks=0) == 0


def test_python_refusals_come_before_the_native_call(monkeypatch):
    def native(*a, **k):
        pytest.fail("the native layer was reached")
    monkeypatch.setattr(MF, "_call", native)
    i64 = torch.zeros(3, dtype=torch.int64)
    i32 = torch.zeros(2, dtype=torch.int32)
    dev_rows, host_rows = torch.zeros(4, D), torch.zeros(5, D)

    def sample(store, host):
        return MF.bag_sample_tiered(store, host, i64, i32, None, 4, 0, 0)

    def pack(store, host):
        return MF.bag_pack_tiered(store, host, i64, i32, None, i64, i64, 4, 2, 0, 0)
    for call in (sample, pack):
        # an ordinary (pageable) tensor as the host tier: refused here, whatever else is wrong with the call
        assert not host_rows.is_pinned()
        with pytest.raises(RuntimeError, match="pinned"):
            call(dev_rows, host_rows)
        with pytest.raises(RuntimeError, match="float32 / float16 / bfloat16"):
            call(dev_rows.double(), host_rows)
        with pytest.raises(RuntimeError, match="float32 / float16 / bfloat16"):
            call(dev_rows, host_rows.to(torch.int32))
        with pytest.raises(RuntimeError, match=r"\[T, D\]"):
            call(dev_rows.view(-1), host_rows)
        with pytest.raises(RuntimeError, match=r"\[T, D\]"):
            call(dev_rows, host_rows.view(1, 5, D))
        with pytest.raises(RuntimeError, match="unit column stride"):
            call(dev_rows, torch.zeros(D, 5).t())
        with pytest.raises(RuntimeError, match="share dtype and width"):
            call(dev_rows, host_rows.half())
        with pytest.raises(RuntimeError, match="share dtype and width"):
            call(dev_rows, torch.zeros(5, D + 2))
        with pytest.raises(RuntimeError, match="no CPU fallback"):          # no host tier at all: the device tier must be on a device
            call(dev_rows, None)
    # the untiered functions still refuse a store that is not on a device
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MF.bag_sample(host_rows, i64, i32, None, 4, 0, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MF.bag_pack(host_rows, i64, i32, None, i64, i64, 4, 2, 0, 0)
