"""Host side of the device smooth rank (R1): the two entry points declared, bound and exported, the workspace query, the refusals
that fire before any launch, the Python wrapper's refusals, and the fp64 oracle pinned to the reference's function.  No GPU."""
import ctypes

import pytest
import torch

from madeleine_amd import _native
from tests import _rank_ref as RR

P, I32, I64, U64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64
FAKE = 1 << 20          # a 16-byte aligned address nothing dereferences: every refusal below comes before the first launch


def test_entry_points_are_declared_bound_and_exported():
    import madeleine_amd
    from madeleine_amd import functional as MF
    assert _native.ABI_VERSION == 26 and _native.lib().mdl_abi_version() == 26
    want = {"mdl_smooth_rank_ws_bytes": (I64, [I64, I64]),
            "mdl_smooth_rank": (I32, [P, I64, I64, I64, U64, P, P, P, P])}
    for name, sig in want.items():
        assert _native.SIGNATURES[name] == sig, name
        fn = getattr(_native.lib(), name)
        assert fn.restype is sig[0] and fn.argtypes == sig[1], name
    assert callable(MF.smooth_rank) and callable(madeleine_amd.device_smooth_rank)
    assert "device_smooth_rank" in madeleine_amd.__all__
    assert MF.RANK_MAX_K == 1024


def test_workspace_query():
    ws = _native.lib().mdl_smooth_rank_ws_bytes
    for n, d in ((1153, 512), (37, 512), (1, 1)):
        k = min(n, d)
        assert ws(n, d) >= 8 * (2 * k * k + 4 * k) and ws(n, d) % 16 == 0, (n, d)      # G, one partial at least, four vectors
    assert ws(0, 512) < 0 and ws(512, 0) < 0
    assert ws(2000, 1025) == _native._DEFINES["MDL_E_UNSUPPORTED"] and ws(1024, 5000) > 0


@pytest.mark.parametrize("ld, n, d, code", [(511, 600, 512, "MDL_E_ARG"), (512, 0, 512, "MDL_E_ARG"), (512, 600, 0, "MDL_E_ARG"),
                                            (2000, 1025, 2000, "MDL_E_UNSUPPORTED"), (1025, 2000, 1025, "MDL_E_UNSUPPORTED")],
                         ids=["ldE<d", "n=0", "d=0", "k=1025 rows", "k=1025 columns"])
def test_refusals_before_any_launch(ld, n, d, code):
    rc = _native.lib().mdl_smooth_rank(FAKE, ld, n, d, 0, FAKE, FAKE, FAKE, None)
    assert rc == _native._DEFINES[code]


def test_alignment_and_null_refusals():
    call = _native.lib().mdl_smooth_rank
    assert call(None, 512, 600, 512, 0, FAKE, FAKE, FAKE, None) == _native._DEFINES["MDL_E_ARG"]
    assert call(FAKE + 2, 512, 600, 512, 0, FAKE, FAKE, FAKE, None) == _native._DEFINES["MDL_E_ALIGN"]
    assert call(FAKE, 512, 600, 512, 0, FAKE + 4, FAKE, FAKE, None) == _native._DEFINES["MDL_E_ALIGN"]
    assert call(FAKE, 512, 600, 512, 0, FAKE, FAKE + 4, FAKE, None) == _native._DEFINES["MDL_E_ALIGN"]
    assert call(FAKE, 512, 600, 512, 0, FAKE, FAKE, FAKE + 8, None) == _native._DEFINES["MDL_E_ALIGN"]
    # the order of the header: a misaligned pointer is reported before the size limit
    assert call(FAKE + 2, 2000, 1025, 2000, 0, FAKE, FAKE, FAKE, None) == _native._DEFINES["MDL_E_ALIGN"]


def test_wrapper_refusals_on_cpu_tensors():
    import madeleine_amd
    from madeleine_amd import functional as MF
    for fn in (MF.smooth_rank, madeleine_amd.device_smooth_rank):
        with pytest.raises(ValueError, match="2-D float32"):
            fn(torch.zeros(8, 4, dtype=torch.float64))
        with pytest.raises(ValueError, match="2-D float32"):
            fn(torch.zeros(8, 4, dtype=torch.bfloat16))
        with pytest.raises(ValueError, match="2-D float32"):
            fn(torch.zeros(2, 8, 4))
        with pytest.raises(ValueError, match="2-D float32"):
            fn(torch.zeros(8))
        with pytest.raises(ValueError, match="at least one row"):
            fn(torch.zeros(0, 4))
        with pytest.raises(ValueError, match="ROCm device"):
            fn(torch.zeros(8, 4))
        with pytest.raises(NotImplementedError, match="1024"):
            fn(torch.zeros(1025, 1030))
    assert not MF.smooth_rank_supported(torch.zeros(8, 4))


def test_opt_in_keywords_default_to_the_host_path():
    import inspect

    from madeleine_amd import DeviceSlideStore, run_inference
    assert inspect.signature(run_inference).parameters["device_rank"].default is False
    assert inspect.signature(DeviceSlideStore.embed).parameters["rank"].default is False
    assert inspect.signature(DeviceSlideStore.mean_embeddings).parameters["rank"].default is False


def _reference_unrounded(E, eps=1e-7):
    """smooth_rank_measure (madeleine_amd/utils.py) line by line, without its round()."""
    _, S, _ = torch.svd(E)
    p = S / torch.norm(S, p=1) + eps
    p = p[:E.shape[1]]
    return torch.exp(-torch.sum(p * torch.log(p))).item()


@pytest.mark.parametrize("name", list(RR.CASES))
def test_oracle_is_the_reference_function_in_fp64(name):
    """The fp64 oracle against the reference's fp32 torch.svd route, unrounded, within 1e-3 relative on every test matrix; and the
    restatement used here is smooth_rank_measure itself up to its rounding."""
    from madeleine_amd.utils import smooth_rank_measure
    E, rank, S = RR.case(name)
    Et = torch.from_numpy(E.copy())
    ref = _reference_unrounded(Et)
    print("%s: oracle %.6f, fp32 SVD route %.6f, rel. dev. %.2e" % (name, rank, ref, abs(ref - rank) / rank))
    assert abs(ref - rank) <= 1e-3 * rank
    assert smooth_rank_measure(Et) == round(ref, 2)
    assert S.shape == (min(E.shape),) and bool((S[:-1] >= S[1:]).all()) and bool((S >= 0).all())
