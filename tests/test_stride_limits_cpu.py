"""The footing of tests/test_stride_limits_gpu.py, without a GPU: (1) every stride argument of the two headers is run at its limit
(Part A), run far past element 2^31 (Part B) or on the tiered-store exemption, and an argument whose limiting kernel cannot be run at
its edge has its two cases and its sentence in ARGUED; (2) the inequalities every case relies on hold, from the table alone; (3) the
layout (WideLay) places its slices as it says and its scan names a stray byte wherever it is planted."""
import collections

import pytest
import torch

from tests import _extent_cases as C
from tests import _wide_cases as W
from tests.test_strides_cpu import _entries
from tests.test_strides_gpu import Lay


# ========================================================================================================================= coverage
def _limits():
    """{(entry point, argument): {(rows, elem, align): {col, ...}}} of the refusal table, and the arguments it carries without a limit."""
    lim, free = collections.defaultdict(lambda: collections.defaultdict(set)), set()
    for prm in _entries():
        name, _, strides, _ = prm.values
        for st in strides:
            if st.rows is None:
                free.add((name, st.name))
            else:
                lim[(name, st.name)][(st.rows, st.elem, st.align)].add(st.col)
    return lim, free


def _header_strides():
    from madeleine_amd import _build
    out = set()
    for path in (_build.HEADER, _build.VIEW_HEADER):
        with open(path) as f:
            out |= W.stride_arguments(C.prototypes(f.read()))
    return out


def test_every_limit_of_the_refusal_table_is_run():
    lim, _ = _limits()
    assert lim
    for key, terms in lim.items():
        cases = [c for c in W.PART_A if key in c.covers]
        for (rows, elem, align), cols in terms.items():
            hit = [c for c in cases if (c.rows, c.elem, c.align) == (rows, elem, align) and c.col in cols]
            kinds = sorted(c.kind for c in hit)
            if key in W.ARGUED:
                assert kinds == ["i", "ii"], (key, rows, kinds)
            else:
                assert kinds == ["limit"], (key, rows, kinds)
    for c in W.PART_A:
        for key in c.covers:
            assert (c.rows, c.elem, c.align) in lim[key] and c.col in lim[key][(c.rows, c.elem, c.align)], (c.id, key, "not a limit of the refusal table")


def test_the_narrow_output_tile_is_in_both_tables():
    lim, _ = _limits()
    assert (512, 1, 16) in lim[("mdl_split_gemm_nt", "a_rsb")] and (128, 1, 16) in lim[("mdl_split_gemm_nt", "b_rsb")]


def test_argued_arguments_have_two_cases_and_one_sentence():
    for key, why in W.ARGUED.items():
        kinds = sorted(c.kind for c in W.PART_A if key in c.covers)
        assert kinds == ["i", "ii"], (key, kinds)
        assert why.strip().endswith(".") and "argued" in why and "not run" in why, key
    for c in W.PART_A:
        if c.kind != "limit":
            assert all(key in W.ARGUED for key in c.covers), c.id


def test_every_stride_argument_of_the_headers_is_placed():
    lim, free = _limits()
    every = _header_strides()
    a = {k for c in W.PART_A for k in c.covers}
    b = {k for c in W.PART_B for k in c.covers}
    assert len(every) > 60 and ("mdl_heat_render", "ld") in every and ("mdl_cox_fit", "lde") in every
    assert a == set(lim), "Part A and the arguments with a limit differ: %s" % sorted(a ^ set(lim))
    assert not a & b and not (a | b) & W.TIERED_EXEMPT
    missing = every - a - b - W.TIERED_EXEMPT
    assert not missing, "run neither at a limit nor far, and not exempt: %s" % sorted(missing)
    assert not (a | b | W.TIERED_EXEMPT) - every, "not a stride argument of a header: %s" % sorted((a | b | W.TIERED_EXEMPT) - every)
    assert free <= b, "without a limit in the refusal table and not in Part B: %s" % sorted(free - b)
    assert all(name.endswith("_tiered") for name, _ in W.TIERED_EXEMPT)


def test_case_ids_are_unique():
    ids = [c.id for c in W.PART_A + W.PART_B]
    assert len(ids) == len(set(ids))


# ======================================================================================================================= arithmetic
@pytest.mark.parametrize("c", W.PART_A, ids=lambda c: c.id)
def test_part_a_arithmetic(c):
    ld = c.ld
    assert ld % c.align == 0 and (ld * c.elem) % 16 == 0
    assert c.span_rows * ld * c.elem + W.LEAD <= W.ARENA_BYTES, "span and lead do not fit the arena"
    assert W.LEAD >= 1 << 31
    far = sum(1 for i in range(c.T) if i * ld * c.elem >= 1 << 32)
    if c.kind == "ii":
        assert ld <= c.limit_ld and (c.span_rows * (ld + c.align) * c.elem + W.LEAD > W.ARENA_BYTES or ld == c.limit_ld)
        assert far >= 1
        return
    assert c.rows * ld * c.elem + c.col <= W.LIM < c.rows * (ld + c.align) * c.elem + c.col
    if c.capped:
        assert c.T <= c.rows and far == 0       # one tile at most: the operand cannot be taller
        return
    assert 0 <= c.T - (2 * (c.rows + 1) + 1) < 4, "two full tiles of the limiting expression and a ragged row"
    assert far >= 1 and (c.rows + 1) * ld * c.elem < (1 << 32) <= (c.T - 1) * ld * c.elem


@pytest.mark.parametrize("c", W.PART_B, ids=lambda c: c.id)
def test_part_b_arithmetic(c):
    ld = c.ld
    assert ld % c.align == 0 and (ld * c.elem) % 16 == 0
    assert c.R * ld * c.elem + W.LEAD <= W.ARENA_BYTES, "span and lead do not fit the arena"
    far = [i for i in range(c.R) if i * ld >= c.mark]
    assert len(far) >= 2 and far[0] == c.R - max(2, c.R // 8), "the rows from R - max(2, R // 8) on start past the mark"
    assert (far[0] - 1) * ld < c.mark


# ======================================================================================================================== the checker
LEAD, ARENA = 4096, 1 << 16


def _lay(target=(0, 1), ld=1000, elem=4):
    arena = torch.empty(ARENA, dtype=torch.uint8)
    lay = W.WideLay(arena, set(target), ld, elem, Lay("pad", torch.device("cpu")), lead=LEAD)
    g = torch.Generator().manual_seed(5)
    x = torch.rand((12, 40), generator=g)
    a = lay.inp(x, 0)
    b = lay.out(12, 24, torch.float32, 1)
    c = lay.out(10, 16, torch.bfloat16, 1, init=torch.ones(10, 16))
    d = lay.inp(x[:, :8], 2)                      # not targeted: a small padded buffer of its own
    e = lay.out(12, 8, torch.float32, 2)
    return lay, arena, x, (a, b, c, d, e)


def test_slices_are_disjoint_aligned_and_behind_the_lead():
    lay, arena, x, (a, b, c, d, e) = _lay()
    assert len(lay.slices) == 3
    base = arena.data_ptr()
    spans = []
    for s in lay.slices:
        v = s["view"]
        assert v.data_ptr() % 16 == 0 and v.data_ptr() - base >= LEAD + W.GAP
        assert v.stride(0) * v.element_size() == 4000 and v.stride(1) == 1
        assert s["col"] % 16 == 0 and s["col"] + s["wb"] + W.GAP <= 4000
        spans.append((s["col"], s["col"] + s["wb"]))
    spans.sort()
    for (_, hi), (lo, _) in zip(spans, spans[1:]):
        assert lo - hi >= W.GAP, "neighbouring slices closer than the gap"
    assert torch.equal(a, x) and a.untyped_storage().data_ptr() == arena.untyped_storage().data_ptr()
    for t in (d, e):                              # the others are as Lay('pad') has them
        assert t.untyped_storage().data_ptr() != arena.untyped_storage().data_ptr() and t.stride(0) == 8 + 3 * 4
    assert torch.equal(d, x[:, :8]) and bool(torch.isnan(e).all()) and bool(torch.isnan(b).all())


def test_an_untouched_run_passes():
    lay, arena, _, (a, b, c, d, e) = _lay()
    b.copy_(torch.zeros(12, 24))                  # a kernel writes its outputs, and nothing else
    e.copy_(torch.zeros(12, 8))
    lay.check_padding()
    assert bool((arena == W.FILL).all())


def test_a_span_that_does_not_fit_is_refused():
    lay, _, _, _ = _lay()
    with pytest.raises(AssertionError, match="does not fit the arena"):
        lay.out(16, 8, torch.float32, 0)          # lead + 16 rows of 4000 bytes > the arena
    with pytest.raises(AssertionError, match="side by side"):
        lay.out(4, 900, torch.float32, 0)


@pytest.mark.parametrize("where,pos,text", [
    ("gap between two slices", LEAD + 3 * 4000 + 270, "nearest operand 1 (k = 1, [12, 24] float32), row 3 of 12, column byte offset -18, in the fill beside it"),
    ("lead", 100, "in the lead, 3996 bytes before the first row"),
    ("behind the last row", LEAD + 13 * 4000 + W.GAP + 8, "row 13 of 12, column byte offset 8, behind the last row"),
    ("last byte of the arena", ARENA - 1, "behind the last row"),
])
def test_a_planted_byte_is_named(where, pos, text):
    lay, arena, _, _ = _lay()
    arena[pos] = 0
    with pytest.raises(AssertionError, match="outside every valid slice") as e:
        lay.check_padding()
    assert text in str(e.value) and "byte %d of the arena" % pos in str(e.value) and "1 bytes changed" in str(e.value), str(e.value)


def test_a_modified_input_fails():
    lay, _, _, (a, b, c, d, e) = _lay()
    a[7, 3] = 2.0
    with pytest.raises(AssertionError, match="changed an input: operand 0"):
        lay.check_padding()


def test_a_stray_write_into_a_small_padded_buffer_still_fails():
    lay, _, _, (a, b, c, d, e) = _lay()
    torch.as_strided(e, (12, 20), (20, 1))[2, 9] = 1.0      # a padding column of the untargeted output
    with pytest.raises(AssertionError, match="outside the valid columns"):
        lay.check_padding()


def test_far_rows_counts_from_the_operand_base():
    lay, _, _, _ = _lay()
    assert lay.far_rows(0) == 12 and lay.far_rows(4000) == 11 and lay.far_rows(44000) == 1 and lay.far_rows(44001) == 0
