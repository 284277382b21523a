"""The prototype read-outs of the slide store on the GPU: store.prototypes against fit_kmeans on the packed rows of the same bags (bit
for bit, in the three store dtypes, with an absent stain in the cohort), the per-slide histograms and their sums, the refusal of a
bag in the pinned host tier, and histograms feeding the linear probe end to end."""
import pytest
import torch

from madeleine_amd import cluster
from madeleine_amd.store import DeviceSlideStore

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _cohort(D, seed):
    """9 cases x 2 stains, bag lengths on both sides of the 128-row chunk, case 4 without its second stain; rows around 3 centres"""
    g = torch.Generator().manual_seed(seed)
    centres = 5.0 * torch.randn(3, D, generator=g)
    lens = [[1 + (53 * c + 17 * m) % 300 for m in range(2)] for c in range(9)]
    lens[2][0], lens[4][1] = 128, None
    bags = [[None if n is None else centres[torch.randint(0, 3, (n,), generator=g)] + 0.5 * torch.randn(n, D, generator=g) for n in case]
            for case in lens]
    return bags, lens


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16", "bf16"])
def test_prototypes_equal_fit_kmeans_on_the_packed_rows(dev, dtype):
    D, k = 24, 3
    bags, lens = _cohort(D, 1)
    st = DeviceSlideStore(bags, ["s%d" % c for c in range(9)], ["HE", "IHC"], dev, dtype=dtype)
    for m, cases in ((1, None), (0, [7, 2, 5])):
        res = st.prototypes(k, modality=m, case_indices=cases, seed=2, max_iter=30)
        want_cases = [c for c in range(9) if lens[c][m] is not None] if cases is None else cases
        assert res["cases"].tolist() == want_cases and res["slide_ids"] == ["s%d" % c for c in want_cases]
        packed = torch.cat([st.bag_view(c, m) for c in want_cases]).contiguous()
        ref = cluster.fit_kmeans(packed, k, seed=2, max_iter=30)
        assert res["cu"].tolist() == [0] + torch.tensor([lens[c][m] for c in want_cases]).cumsum(0).tolist()
        for name in ("centroids", "labels", "counts"):
            assert torch.equal(res[name], getattr(ref, name)), (m, name)
        assert torch.equal(res["dist"].view(torch.int32), ref.dist.view(torch.int32))
        assert res["inertia"] == ref.inertia and res["n_iter"] == ref.n_iter and res["converged"] == ref.converged
        # the histograms: rows sum to the bag lengths, and to 1 when normalised
        raw = st.prototype_histograms(res["centroids"], modality=m, case_indices=cases, normalize=False)
        assert raw["embeds"].shape == (len(want_cases), k) and raw["embeds"].dtype == torch.float32 and raw["cases"].tolist() == want_cases
        assert raw["embeds"].sum(1).tolist() == [float(lens[c][m]) for c in want_cases]
        assert torch.equal(raw["embeds"].sum(0).long(), res["counts"]) or not res["converged"]
        nrm = st.prototype_histograms(res["centroids"], modality=m, case_indices=cases)
        assert torch.allclose(nrm["embeds"].sum(1), torch.ones(len(want_cases), device=dev), atol=1e-6)
        assert torch.equal(nrm["embeds"], raw["embeds"] / raw["embeds"].sum(1, keepdim=True))
    with pytest.raises(ValueError, match="case 4"):
        st.prototypes(k, modality=1, case_indices=[3, 4])


def test_a_bag_in_the_host_tier_is_refused(dev):
    D = 24
    bags, lens = _cohort(D, 2)
    ids = ["s%d" % c for c in range(9)]
    res = DeviceSlideStore(bags, ids, ["HE", "IHC"], dev)
    tiered = DeviceSlideStore(bags, ids, ["HE", "IHC"], dev, resident_bytes=(res.rows.shape[0] // 2) * D * 4)
    assert tiered.rows_host is not None and 0 < tiered.resident_rows < res.rows.shape[0]
    first = next(c for c in range(9) if int(tiered.off_cpu[int(tiered.bag_table[c, 0]) + 1]) > tiered.resident_rows)
    with pytest.raises(NotImplementedError, match=r"case %d \(s%d\)" % (first, first)):
        tiered.prototypes(3)
    with pytest.raises(NotImplementedError, match="host tier"):
        tiered.prototype_histograms(torch.zeros(3, D, device=dev))
    assert tiered.prototypes(1, case_indices=[0, 1], max_iter=2)["labels"].numel() == lens[0][0] + lens[1][0]      # resident bags are served


def test_histograms_feed_the_linear_probe(dev):
    """40 cases in two classes whose patches come from different pairs of prototypes: separable by construction, so exact scores assert
    the plumbing from the store through the histograms to the probe, not a tolerance."""
    from madeleine_amd import linear_probe
    D, g = 16, torch.Generator().manual_seed(4)
    centres = 6.0 * torch.randn(4, D, generator=g)
    labels = torch.tensor([c % 2 for c in range(40)])
    bags = [[centres[2 * int(labels[c]) + torch.randint(0, 2, (20 + (7 * c) % 23,), generator=g)]
             + 0.3 * torch.randn(20 + (7 * c) % 23, D, generator=g)] for c in range(40)]
    st = DeviceSlideStore(bags, ["p%d" % c for c in range(40)], ["HE"], dev)
    hist = st.prototype_histograms(centres.to(dev))
    assert hist["embeds"].shape == (40, 4)
    res = linear_probe(hist["embeds"], labels, ks=(1,), folds=2)[("label", 1)]
    assert res["auc"].tolist() == [1.0, 1.0] and res["bacc"].tolist() == [1.0, 1.0]
