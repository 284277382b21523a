"""CPU checks of InfoNCE with explicit negatives (negative_keys): the C ABI entry points (declared, bound, exported, ABI revision
unchanged), their argument validation before any launch, the dispatch-plan answers on both sides of each threshold, and the host-side
errors of InfoNCE(...)(query, positive_key, negative_keys) on CPU tensors."""
import ctypes
import re

import pytest
import torch

from tests._util import ROOT

NEG = ["mdl_infonce_neg_ws_bytes", "mdl_infonce_neg_fwd", "mdl_infonce_neg_bwd"]
E_ARG = -1


def _lib():
    from madeleine_amd import _native
    return _native.lib()


def test_header_binding_and_library_carry_the_negative_entry_points():
    from madeleine_amd import _native
    hdr = open(f"{ROOT}/include/madeleine_amd.h").read()
    for name in NEG:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in _native.SIGNATURES, name
        assert hasattr(ctypes.CDLL(_native.lib_path()), name), name
    assert "loss.py:93-110" in hdr and "F.cross_entropy(logits / temperature, labels, reduction)" in hdr


def test_abi_revision_is_still_26():
    from madeleine_amd import _native
    hdr = open(f"{ROOT}/include/madeleine_amd.h").read()
    assert re.search(r"#define MDL_ABI_VERSION 26\b", hdr)
    assert _native.ABI_VERSION == 26 and _lib().mdl_abi_version() == 26


@pytest.mark.parametrize("paired", [0, 1])
def test_workspace_query(paired):
    lib = _lib()
    assert lib.mdl_infonce_neg_ws_bytes(7, 300, 100, paired) > 0
    assert lib.mdl_infonce_neg_ws_bytes(1, 0, 512, paired) > 0
    assert lib.mdl_infonce_neg_ws_bytes(-1, 4, 512, paired) == E_ARG
    assert lib.mdl_infonce_neg_ws_bytes(4, -1, 512, paired) == E_ARG
    assert lib.mdl_infonce_neg_ws_bytes(4, 4, 0, paired) == E_ARG


@pytest.mark.parametrize("paired", [0, 1])
def test_null_pointers_and_bad_sizes_are_refused_before_any_launch(paired):
    """Every pointer below is a bogus (but 16-byte aligned, non-null) address: a launch would fault, so MDL_E_ARG proves the check
    runs first.  The stream is null; nothing reaches a device."""
    lib = _lib()
    x = 1 << 20
    fwd = lambda Q=x, P=x, Neg=x, loss=x, rows=x, N=4, M=8, D=64, T=0.1, ws=x: lib.mdl_infonce_neg_fwd(  # noqa: E731
        Q, P, Neg, loss, rows, N, M, D, paired, T, ws, None)
    bwd = lambda Neg=x, dl=x, dr=x, dQ=x, dP=x, dN=x, N=4, M=8, D=64, T=0.1, ws=x: lib.mdl_infonce_neg_bwd(  # noqa: E731
        Neg, dl, dr, dQ, dP, dN, N, M, D, paired, T, ws, None)
    for kw in ({"Q": None}, {"P": None}, {"Neg": None}, {"loss": None, "rows": None}, {"ws": None}, {"N": -1}, {"M": -1}, {"D": 0},
               {"D": -3}, {"T": 0.0}, {"T": -1.0}):
        assert fwd(**kw) == E_ARG, kw
    for kw in ({"Neg": None}, {"dl": None, "dr": None}, {"dQ": None}, {"dP": None}, {"ws": None}, {"N": -1}, {"M": -1}, {"D": 0},
               {"T": 0.0}):
        assert bwd(**kw) == E_ARG, kw


def _plan(N, M, D):
    from madeleine_amd import _native
    return _native.dispatch_plan("infonce_neg", N, M, D)


def test_dispatch_plan_on_both_sides_of_each_threshold():
    """Load width: 16-byte loads exactly when D % 4 == 0.  Splits of the unpaired dQ contraction: 1024 negatives each.  Paired
    chunks: 64 negatives per wave.  LSE partials: 4096 logits each.  M = 0 still runs one (empty) split of each."""
    assert _plan(8, 100, 100)["variant"] == 1 and _plan(8, 100, 102)["variant"] == 0 and _plan(8, 100, 7)["variant"] == 0
    assert _plan(8, 100, 512)["variant"] == 1
    assert _plan(8, 1024, 512)["splits"] == 1 and _plan(8, 1025, 512)["splits"] == 2 and _plan(8, 65536, 512)["splits"] == 64
    assert _plan(8, 64, 512)["chunk"] == 1 and _plan(8, 65, 512)["chunk"] == 2 and _plan(8, 65600, 512)["chunk"] == 1025
    assert _plan(8, 4096, 512)["extra"] == 1 and _plan(8, 4097, 512)["extra"] == 2
    p0 = _plan(8, 0, 512)
    assert (p0["splits"], p0["chunk"], p0["extra"]) == (1, 1, 1)


def test_dispatch_plan_leaves_products_1_to_10_alone():
    from madeleine_amd import _native
    assert [_native.PLAN_PRODUCTS[k] for k in ("gate_fp32_bwd", "got")] == [1, 10] and _native.PLAN_PRODUCTS["infonce_neg"] == 11
    hdr = open(f"{ROOT}/include/madeleine_amd.h").read()
    assert re.search(r"#define MDL_PLAN_INFONCE_NEG 11\b", hdr) and re.search(r"#define MDL_PLAN_GOT 10\b", hdr)


def test_unknown_negative_mode_raises_value_error():
    from madeleine_amd import InfoNCE
    crit = InfoNCE(negative_mode="both")
    with pytest.raises(ValueError, match="negative_mode must be 'paired' or 'unpaired'"):
        crit(torch.zeros(2, 4), torch.zeros(2, 4), negative_keys=torch.zeros(3, 4))


@pytest.mark.parametrize("mode,shape", [("unpaired", (5, 4)), ("paired", (2, 5, 4))])
def test_cpu_tensors_raise_the_in_batch_runtime_error(mode, shape):
    from madeleine_amd import InfoNCE
    with pytest.raises(RuntimeError, match="ROCm device"):
        InfoNCE(negative_mode=mode)(torch.zeros(2, 4), torch.zeros(2, 4), negative_keys=torch.zeros(*shape))


def test_existing_checks_still_come_first():
    """The reference's argument checks keep their order and messages ahead of the new ones (a 3-D unpaired bank, a paired bank of
    the wrong length, a width mismatch -- all ValueError on CPU tensors, before the device check)."""
    from madeleine_amd import InfoNCE
    with pytest.raises(ValueError, match="must have 2 dimensions if <negative_mode> == 'unpaired'"):
        InfoNCE()(torch.zeros(2, 4), torch.zeros(2, 4), negative_keys=torch.zeros(2, 3, 4))
    with pytest.raises(ValueError, match="must have 3 dimensions if <negative_mode> == 'paired'"):
        InfoNCE(negative_mode="paired")(torch.zeros(2, 4), torch.zeros(2, 4), negative_keys=torch.zeros(3, 4))
    with pytest.raises(ValueError, match="same number of samples as <query>"):
        InfoNCE(negative_mode="paired")(torch.zeros(2, 4), torch.zeros(2, 4), negative_keys=torch.zeros(3, 5, 4))
    with pytest.raises(ValueError, match="<query> and <negative_keys> should have the same number of components"):
        InfoNCE()(torch.zeros(2, 4), torch.zeros(2, 4), negative_keys=torch.zeros(3, 8))
