"""CPU checks of the ragged-view / absent-bag host side: the (perm, vcu) plan of MADELEINE.forward_ragged(n_views=3) against the
reference's per-bag shuffle, the ragged_collate contract, and the ragged-view entry points of the C ABI (declared, bound, exported)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests._util import ROOT

RVIEW = ["mdl_abmil_pool_rview_fwd", "mdl_abmil_pool_rview_bwd", "mdl_abmil_pool_rview_fwd_bf16", "mdl_abmil_pool_rview_bwd_bf16"]


@pytest.mark.parametrize("lens", [[1, 2, 3, 127, 128, 129, 257, 3001], [5], [1, 1, 1], [4096, 2, 2, 300]])
def test_view_plan_is_the_reference_draw_per_bag(lens):
    """Bag after bag in packed order: idx = arange(N_b); np.random.shuffle(idx); mid = N_b // 2 (Model.py:419-440 for one bag); view 1 =
    idx[:mid], view 2 = idx[mid:], as absolute packed rows."""
    from madeleine_amd.model import ragged_view_plan
    np.random.seed(1234)
    perm, vcu, max_view = ragged_view_plan(lens)
    after = np.random.random()
    assert perm.dtype == torch.int32 and vcu.dtype == torch.int64
    assert perm.numel() == sum(lens) and vcu.numel() == 2 * len(lens) + 1
    np.random.seed(1234)
    start = 0
    for b, n in enumerate(lens):
        idx = np.arange(n)
        np.random.shuffle(idx)
        mid = n // 2
        assert int(vcu[2 * b]) == start and int(vcu[2 * b + 1]) == start + mid
        assert perm[vcu[2 * b]:vcu[2 * b + 1]].tolist() == (start + idx[:mid]).tolist()
        assert perm[vcu[2 * b + 1]:vcu[2 * b + 2]].tolist() == (start + idx[mid:]).tolist()
        start += n
    assert int(vcu[-1]) == start
    assert np.random.random() == after                           # the plan consumed exactly the reference's draws
    assert sorted(perm.tolist()) == list(range(sum(lens)))       # a permutation: the two views of a bag write disjoint rows
    assert max_view == max(n - n // 2 for n in lens)
    seg = (vcu[1:] - vcu[:-1]).tolist()
    assert seg == [v for n in lens for v in (n // 2, n - n // 2)]


def test_view_plan_empty_batch():
    from madeleine_amd.model import ragged_view_plan
    perm, vcu, max_view = ragged_view_plan([])
    assert perm.numel() == 0 and vcu.tolist() == [0] and max_view == 0


def test_ragged_collate_contract():
    """SlideDataset(sample=-1) keeps every bag at its real length (an absent stain: the 2-token zero bag, wsi_dataset.py:66);
    ragged_collate batches them as lists, with the label matrix and the slide ids of collate()."""
    import pandas as pd
    from madeleine_amd.data import SlideDataset, collate, ragged_collate
    df = pd.DataFrame({"slide_id": ["a", "b", "c"], "HE": [1, 1, 1], "ER": [1, 0, 1], "split": ["train", "train", "val"]})
    sizes = {"a_HE": 7, "a_ER": 300, "b_HE": 5, "c_HE_val": 1, "c_ER_val": 3}

    def loader(path):
        key = os.path.basename(path)[:-3]
        return torch.full((sizes[key], 4), float(len(key)))

    ds = SlideDataset("x", None, "/feats", ["HE", "ER"], embedding_size=4, sample=-1, feature_loader=loader, dataframe=df)
    items = [ds[i] for i in range(3)]
    batch = ragged_collate(items)
    assert set(batch) == {"bags", "modality_labels", "slide_ids"}
    assert [[tuple(x.shape) for x in case] for case in batch["bags"]] == [[(7, 4), (300, 4)], [(5, 4), (2, 4)], [(1, 4), (3, 4)]]
    assert float(batch["bags"][1][1].abs().sum()) == 0.0
    for case, item in zip(batch["bags"], items):
        assert all(x is y for x, y in zip(case, item["feats"]))       # the items' own tensors, no copies
    assert batch["modality_labels"].dtype == torch.float32 and batch["modality_labels"].tolist() == [[1, 1], [1, 0], [1, 1]]
    assert batch["slide_ids"] == ["a", "b", "c"]
    with pytest.raises(RuntimeError):
        collate(items)                                               # what the reference's collate does with unequal bags


def test_ragged_view_entry_points_declared_bound_exported():
    from madeleine_amd import _native
    src = open(os.path.join(ROOT, "include", "madeleine_amd.h")).read()
    assert int(re.search(r"#define MDL_ABI_VERSION (\d+)", src).group(1)) == _native.ABI_VERSION == 26
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for n in RVIEW:
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert n in _native.SIGNATURES, n
    lib = _native.lib()
    raw = ctypes.CDLL(_native.lib_path())
    for n in RVIEW:
        assert hasattr(raw, n), n
    assert lib.mdl_abi_version() == 26
    # host-side argument checks (no device work): NULL perm / vcu and negative sizes are rejected before any launch
    p = ctypes.c_void_p(16)
    assert lib.mdl_abmil_pool_rview_fwd(p, 2048, p, p, p, p, 3, None, p, 8, 4, p, None) == -1
    assert lib.mdl_abmil_pool_rview_bwd(p, 2048, p, p, p, p, p, p, p, -1, p, p, 8, 4, None) == -1
    assert lib.mdl_abmil_pool_rview_bwd_bf16(p, 2048, p, p, p, p, p, None, None, 3, p, p, 8, 4, None) == -1
