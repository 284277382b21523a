"""Host side of the retrieval kernels (X1): the entry points declared, bound and exported, the workspace query (no similarity matrix),
every refusal that fires before a launch in the header's order, the Python wrappers' refusals, retrieval_metrics on hand-made counts,
the reference's own order, and the zero-ambiguity condition the GPU tests' cosine cohorts rest on.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

from madeleine_amd import _native
from tests import _retrieval_ref as RR

P, I32, I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
FAKE = 1 << 20          # a 16-byte aligned address nothing dereferences: every refusal below comes before the first launch
D = _native._DEFINES
ARG, ALIGN, UNSUPPORTED = D["MDL_E_ARG"], D["MDL_E_ALIGN"], D["MDL_E_UNSUPPORTED"]


def test_entry_points_are_declared_bound_and_exported():
    import madeleine_amd
    from madeleine_amd import functional as MF
    assert _native.ABI_VERSION == 26 and _native.lib().mdl_abi_version() == 26
    want = {"mdl_retrieval_ws_bytes": (I64, [I64, I64, I64, I32, I32]),
            "mdl_retrieval": (I32, [P, I64, P, I64, I64, I64, I64, I32, I32, I32, I32, I32, P, P, P, P, P, P, P])}
    for name, sig in want.items():
        assert _native.SIGNATURES[name] == sig, name
        fn = getattr(_native.lib(), name)
        assert fn.restype is sig[0] and fn.argtypes == sig[1], name
    assert callable(MF.retrieval)
    for name in ("cross_stain_retrieval", "retrieval_metrics", "slide_neighbours"):
        assert callable(getattr(madeleine_amd, name)) and name in madeleine_amd.__all__, name
    assert MF.RETR_MAX_ROWS >= 65536 and MF.RETR_MAX_D >= 2048 and MF.RETR_MAX_K >= 64
    assert (MF.RETR_ROW_BLOCK, MF.RETR_COL_TILE) == (D["MDL_RETR_ROW_BLOCK"], D["MDL_RETR_COL_TILE"])
    assert MF.Retrieval._fields == ("greater", "equal", "pair_sim", "topk_idx", "topk_val")


def test_workspace_query():
    from madeleine_amd import functional as MF
    ws = _native.lib().mdl_retrieval_ws_bytes
    for n, m, d, k, c in ((1153, 1153, 512, 10, 0), (1, 1, 1, 0, 1), (33, 95, 7, 64, 7), (65536, 65536, 2048, 64, 0)):
        got = ws(n, m, d, k, c)
        assert got > 0 and got % 16 == 0, (n, m, d, k, c)
        assert got >= 4 * (n + m) * d, (n, m, d, k, c)                      # the two scaled copies at least
    # the lists grow with the chunks the launcher actually uses, not with the number asked for
    chunks, _ = MF.retrieval_chunks(300, 300, 7)
    assert chunks == 3 and ws(300, 300, 64, 8, 7) == ws(300, 300, 64, 8, 3) > ws(300, 300, 64, 8, 1)
    assert ws(0, 5, 8, 1, 0) == ARG and ws(5, 0, 8, 1, 0) == ARG and ws(5, 5, 0, 1, 0) == ARG
    assert ws(5, 5, 8, -1, 0) == ARG and ws(5, 5, 8, 1, -1) == ARG
    assert ws(D["MDL_RETR_MAX_ROWS"] + 1, D["MDL_RETR_MAX_ROWS"] + 1, 8, 1, 0) == UNSUPPORTED
    assert ws(5, 5, D["MDL_RETR_MAX_D"] + 1, 1, 0) == UNSUPPORTED
    assert ws(5, 5, 8, D["MDL_RETR_MAX_K"] + 1, 0) == UNSUPPORTED
    assert ws(5, 5, 8, 1, D["MDL_RETR_MAX_CHUNKS"] + 1) == UNSUPPORTED


def test_workspace_holds_no_similarity_matrix():
    S = 16384
    assert _native.lib().mdl_retrieval_ws_bytes(S, S, 512, 64, 0) < S * S * 4 // 4


def _call(Q=FAKE, ldq=512, K=FAKE, ldk=512, n=600, m=600, d=512, metric=0, paired=1, exclude_diag=0, k=10, col_chunks=0, greater=FAKE,
          equal=FAKE, pair_sim=FAKE, topk_idx=FAKE, topk_val=FAKE, ws=FAKE):
    return _native.lib().mdl_retrieval(Q, ldq, K, ldk, n, m, d, metric, paired, exclude_diag, k, col_chunks, greater, equal, pair_sim,
                                       topk_idx, topk_val, ws, None)


REFUSALS = [
    ("Q null", dict(Q=None), ARG), ("K null", dict(K=None), ARG), ("ws null", dict(ws=None), ARG),
    ("greater null, paired", dict(greater=None), ARG), ("equal null, paired", dict(equal=None), ARG),
    ("pair_sim null, paired", dict(pair_sim=None), ARG), ("topk_idx null, k > 0", dict(topk_idx=None), ARG),
    ("topk_val null, k > 0", dict(topk_val=None), ARG),
    ("n = 0", dict(n=0), ARG), ("m = 0", dict(m=0), ARG), ("d = 0", dict(d=0), ARG),
    ("ldq < d", dict(ldq=511), ARG), ("ldk < d", dict(ldk=511), ARG),
    ("k < 0", dict(k=-1), ARG), ("col_chunks < 0", dict(col_chunks=-1), ARG), ("metric", dict(metric=2), ARG),
    ("paired = 2", dict(paired=2), ARG), ("exclude_diag = 2", dict(paired=0, exclude_diag=2), ARG),
    ("n > m, paired", dict(n=601), ARG), ("both flags", dict(exclude_diag=1), ARG), ("nothing asked for", dict(paired=0, k=0), ARG),
    ("Q misaligned", dict(Q=FAKE + 2), ALIGN), ("K misaligned", dict(K=FAKE + 2), ALIGN), ("ws misaligned", dict(ws=FAKE + 8), ALIGN),
    ("greater misaligned", dict(greater=FAKE + 2), ALIGN), ("equal misaligned", dict(equal=FAKE + 1), ALIGN),
    ("pair_sim misaligned", dict(pair_sim=FAKE + 2), ALIGN), ("topk_idx misaligned", dict(topk_idx=FAKE + 2), ALIGN),
    ("topk_val misaligned", dict(topk_val=FAKE + 3), ALIGN),
    ("k above the limit", dict(k=D["MDL_RETR_MAX_K"] + 1), UNSUPPORTED),
    ("d above the limit", dict(d=D["MDL_RETR_MAX_D"] + 1, ldq=4096, ldk=4096), UNSUPPORTED),
    ("n above the limit", dict(n=D["MDL_RETR_MAX_ROWS"] + 1, m=D["MDL_RETR_MAX_ROWS"] + 1), UNSUPPORTED),
    ("m above the limit", dict(m=D["MDL_RETR_MAX_ROWS"] + 1), UNSUPPORTED),
    ("col_chunks above the limit", dict(col_chunks=D["MDL_RETR_MAX_CHUNKS"] + 1), UNSUPPORTED),
    ("stride beyond 2^61", dict(ldq=1 << 60), UNSUPPORTED),
    # the header's order: an argument error before a misaligned pointer, a misaligned pointer before a size limit
    ("ARG before ALIGN", dict(Q=FAKE + 2, ldq=511), ARG), ("ALIGN before UNSUPPORTED", dict(Q=FAKE + 2, k=65), ALIGN),
    ("ARG before UNSUPPORTED", dict(n=601, k=65), ARG),
]


@pytest.mark.parametrize("label, change, code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_before_any_launch(label, change, code):
    assert _call(**change) == code


def test_outputs_of_a_mode_that_is_off_may_be_null():
    """Null outputs of the mode that is off pass the argument check: the call gets as far as the size limit behind it."""
    assert _call(paired=0, greater=None, equal=None, pair_sim=None, k=65) == UNSUPPORTED
    assert _call(k=0, topk_idx=None, topk_val=None, d=4096, ldq=4096, ldk=4096) == UNSUPPORTED


def test_wrapper_refusals_on_cpu_tensors():
    import madeleine_amd
    from madeleine_amd import functional as MF
    ok = torch.zeros(8, 4)
    for bad in (torch.zeros(8, 4, dtype=torch.float64), torch.zeros(8, 4, dtype=torch.bfloat16), torch.zeros(2, 8, 4), torch.zeros(8)):
        with pytest.raises(ValueError, match="2-D float32"):
            MF.retrieval(bad)
        with pytest.raises(ValueError, match="2-D float32"):
            MF.retrieval(ok, bad)
    with pytest.raises(ValueError, match="at least one row"):
        MF.retrieval(torch.zeros(0, 4))
    with pytest.raises(ValueError, match="one width"):
        MF.retrieval(ok, torch.zeros(8, 5))
    with pytest.raises(ValueError, match="unit column stride"):
        MF.retrieval(torch.zeros(4, 8).t())
    with pytest.raises(ValueError, match="'cosine' or 'dot'"):
        MF.retrieval(ok, metric="l2")
    with pytest.raises(ValueError, match="not both"):
        MF.retrieval(ok, k=2, paired=True, exclude_diag=True)
    with pytest.raises(ValueError, match="n <= m"):
        MF.retrieval(ok, torch.zeros(7, 4))
    with pytest.raises(ValueError, match="paired=True or k >= 1"):
        MF.retrieval(ok, paired=False)
    with pytest.raises(ValueError, match="k >= 0"):
        MF.retrieval(ok, k=-1)
    with pytest.raises(NotImplementedError, match="k <= 64"):
        MF.retrieval(ok, k=65)
    with pytest.raises(NotImplementedError, match="d <= 2048"):
        MF.retrieval(torch.zeros(2, 2049))
    with pytest.raises(NotImplementedError, match="col_chunks <= 64"):
        MF.retrieval(ok, col_chunks=65)
    with pytest.raises(ValueError, match="ROCm device"):
        MF.retrieval(ok)
    with pytest.raises(ValueError, match="ROCm device"):
        madeleine_amd.slide_neighbours(ok, 3)
    with pytest.raises(ValueError, match="k >= 1"):
        madeleine_amd.slide_neighbours(ok, 0)


def test_retrieval_metrics_on_hand_made_counts():
    from madeleine_amd import retrieval_metrics
    #              rank (pessimistic): 1  2  6  11 4
    greater = torch.tensor([0, 1, 2, 10, 0], dtype=torch.int32)
    equal = torch.tensor([0, 0, 3, 0, 3], dtype=torch.int32)
    got = retrieval_metrics(greater, equal)
    assert got == RR.metrics(greater.numpy(), equal.numpy())
    assert got["n"] == 5 and all(isinstance(v, float) for k, v in got.items() if k != "n")
    assert got["recall@1"] == 0.2 and got["recall_optimistic@1"] == 0.4            # the tie of the last row counts against it
    assert got["recall@5"] == 0.6 and got["recall_optimistic@5"] == 0.8            # 2 + 3 ties: pessimistic rank 6
    assert got["recall@10"] == 0.8 and got["recall_optimistic@10"] == 0.8
    assert got["median_rank"] == 4.0
    assert got["mrr"] == pytest.approx((1 + 1 / 2 + 1 / 6 + 1 / 11 + 1 / 4) / 5, rel=1e-15)
    # a collapsed encoder: everything ties with the partner
    n = 7
    col = retrieval_metrics(torch.zeros(n, dtype=torch.int32), torch.full((n,), n - 1, dtype=torch.int32), ks=(1, 5))
    assert col["recall@1"] == 0.0 and col["recall@5"] == 0.0 and col["recall_optimistic@1"] == 1.0 and col["median_rank"] == float(n)
    one = retrieval_metrics(torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), ks=(1,))
    assert one == {"n": 1, "recall@1": 1.0, "recall_optimistic@1": 1.0, "median_rank": 1.0, "mrr": 1.0}
    with pytest.raises(ValueError):
        retrieval_metrics(torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int32))
    with pytest.raises(ValueError):
        retrieval_metrics(torch.zeros(3, dtype=torch.int32), torch.zeros(2, dtype=torch.int32))


def test_reference_order():
    """The reference's key: descending value, -0 = +0, every NaN below -inf; ties by the lower index; padding."""
    nan = np.float32("nan")
    v = np.array([[0.5, -np.inf, nan, -0.0, 0.0, np.inf, -1.0, -nan, 0.5]], dtype=np.float32)
    k = RR.keys(v)[0]
    assert k[5] > k[0] == k[8] > k[3] == k[4] > k[6] > k[1] > k[2] == k[7] == RR.NAN_KEY > RR.NO_ENTRY
    _, _, _, ti, tv = RR.exact(v, False, False, 11)
    assert ti[0].tolist() == [5, 0, 8, 3, 4, 6, 1, 2, 7, -1, -1]
    assert tv[0, :2].tolist() == [np.inf, 0.5] and np.isnan(tv[0, 7:9]).all() and (tv[0, 9:] == -np.inf).all()
    assert not np.signbit(tv[0, 3])
    g, e, p, _, _ = RR.exact(np.array([[1.0, 2.0, 1.0], [nan, nan, 0.0], [nan, 3.0, 1.0]], dtype=np.float32), True, False, 0)
    assert g.tolist() == [1, 2, 1] and e.tolist() == [1, 0, 0]      # row 1: a NaN partner is last; row 2: a NaN is never ahead of a number


@pytest.mark.parametrize("n,m,d,noise", RR.COSINE_COHORTS + [RR.LAUNCHER_COHORT], ids=lambda v: str(v))
def test_cohorts_are_unambiguous_in_fp64(n, m, d, noise):
    """No row of a cosine cohort has a gallery similarity within tol(d) of its partner's: lo == hi everywhere, so the interval the GPU
    tests allow excuses nothing.  The counts are not trivial either (printed)."""
    Q, K = RR.cohort(n, m, d, noise, RR.SEED)
    sides = [(Q, K)] + ([(K, Q)] if n == m else [])
    for A, B in sides:
        lo, hi, _ = RR.bounds(RR.cosine64(A, B), RR.tol(d))
        print("(%d, %d, %d, %s): median rank %.1f, worst %d" % (n, m, d, noise, np.median(1 + lo), 1 + lo.max()))
        assert int((lo != hi).sum()) == 0
