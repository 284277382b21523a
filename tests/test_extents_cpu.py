"""The extent tests' own footing, without a GPU: (1) every export of include/madeleine_amd.h is either in the case table of
tests/_extent_cases.py or exempt as host-only / measurement-only, every pointer parameter of a covered export has a role, and the roles
agree with the header's const; (2) the guarded arena of tests/_arena.py catches each kind of stray write and names it."""
import pytest
import torch

from tests import _arena
from tests import _extent_cases as C
from tests._arena import Arena, ArenaError


# ================================================================================================================== completeness
@pytest.fixture(scope="module")
def protos():
    return C.prototypes(C.header_text())


def test_the_header_prototypes_are_the_export_list(protos):
    from madeleine_amd import _native
    assert set(protos) == set(_native.SIGNATURES)
    for name, params in protos.items():
        assert len(params) == len(_native.SIGNATURES[name][1]), name


def test_every_export_is_covered_or_exempt_and_never_both(protos):
    from madeleine_amd import _native
    exports = set(_native.SIGNATURES)
    exempt = {n for n in exports if C.exempt_reason(n)}
    covered = set(C.ROLES)
    assert not covered & exempt, sorted(covered & exempt)
    assert not exports - covered - exempt, "neither covered nor exempt: %s" % sorted(exports - covered - exempt)
    assert not covered - exports, "in the table and absent from the header: %s" % sorted(covered - exports)
    assert not set(C.EXEMPT) - exports, "exempt and absent from the header: %s" % sorted(set(C.EXEMPT) - exports)
    assert set(C.PENDING) <= covered


def test_exempt_holds_only_host_and_measurement_entry_points():
    allowed = {"mdl_version", "mdl_abi_version", "mdl_linear_bf16_supported", "mdl_dispatch_plan", "mdl_abmil_gate_dropout_mask",
               "mdl_pool_timer_arm", "mdl_pool_timer_read", "mdl_stream_create_cu_mask", "mdl_stream_destroy",
               "mdl_switch_get", "mdl_switch_set", "mdl_switch_set_thread", "mdl_switch_clear_thread", "mdl_switch_name"}
    assert set(C.EXEMPT) <= allowed, sorted(set(C.EXEMPT) - allowed)
    for name, reason in C.EXEMPT.items():
        assert reason.strip().endswith(".") and reason.count(".") == 1, "one sentence: %s" % name


def test_every_pointer_parameter_has_a_role_that_agrees_with_its_const(protos):
    for name in C.ROLES:
        roles = C.roles_of(name)
        pointers = [(p, const) for p, is_ptr, const in protos[name] if is_ptr]
        assert [p for p, _ in roles] == [p for p, _ in pointers], "%s: roles %s, pointer parameters %s" % (name, roles, pointers)
        for (p, role), (_, const) in zip(roles, pointers):
            assert role in C.POINTER_ROLES, (name, p, role)
            if const:
                assert role not in ("out", "inout", "ws"), "%s: const %s declared %s" % (name, p, role)
            elif role not in ("host", "null"):
                assert role != "in", "%s: %s is not const in the header and declared in" % (name, p)
            if p.endswith("_host") or p in ("stream", "stream_out"):
                assert role == "host", (name, p, role)


def test_a_new_pointer_argument_cannot_go_unnoticed(protos):
    """The check above fails for a prototype that gains a pointer the table does not name."""
    grown = dict(protos)
    grown["mdl_linear_fwd"] = protos["mdl_linear_fwd"][:4] + [("extra", True, False)] + protos["mdl_linear_fwd"][4:]
    roles = [p for p, _ in C.roles_of("mdl_linear_fwd")]
    assert roles != [p for p, is_ptr, _ in grown["mdl_linear_fwd"] if is_ptr]


def _planned():
    """{case: entry points its planning pass issues}: every case of tests/test_extents_gpu.py run without a device -- buffers are meta
    tensors, nothing is launched, and r.call still holds the argument count to the prototype."""
    import tests.test_extents_gpu as G
    protos = C.prototypes(C.header_text())
    out = {}
    for family, cases in G.FAMILIES.items():
        for cid, factory in cases.items():
            r = C.Run("cpu", 0xFF, protos)
            factory()[0](r)
            assert r.arena.bufs, (family, cid)
            out[family + ":" + cid] = set(r.called)
    return out


def test_every_covered_entry_point_is_issued_by_a_case():
    planned = _planned()
    issued = set().union(*planned.values())
    assert not issued - set(C.ROLES), sorted(issued - set(C.ROLES))
    missing = set(C.ROLES) - issued
    assert missing == set(C.PENDING), "covered in the table, issued by no case and not pending: %s; pending and issued: %s" % (
        sorted(missing - set(C.PENDING)), sorted(set(C.PENDING) - missing))


# ==================================================================================================================== the arena
def _make(fill=0xFF):
    a = Arena("cpu", fill)
    a.reserve("x", (5, 3), torch.float32, "in")
    a.reserve("y", (7, 6), torch.bfloat16, "out")
    a.reserve("w", (100,), torch.uint8, "ws", nbytes=100)
    a.reserve("img", (4 + 32, 32), torch.float32, "out", zero_tail=32 * 32 * 4)
    a.allocate()
    x = a.take("x", (5, 3), torch.float32, "in")
    x.copy_(torch.arange(15.0).view(5, 3))
    a.take("y", (7, 6), torch.bfloat16, "out")
    a.take("w", (100,), torch.uint8, "ws", nbytes=100)
    a.take("img", (36, 32), torch.float32, "out")
    a.seal()
    return a


@pytest.mark.parametrize("fill", _arena.FILLS)
def test_an_untouched_arena_passes_and_its_layout_meets_the_conditions(fill):
    a = _make(fill)
    a.check()
    order = sorted(a.bufs.values(), key=lambda b: b.start)
    assert order[0].start >= _arena.EDGE + order[0].guard and a.total - (order[-1].start + order[-1].nbytes) >= _arena.EDGE + order[-1].guard
    for prev, b in zip(order, order[1:]):
        assert b.start - (prev.start + prev.nbytes) >= prev.guard + b.guard
    for b in order:
        assert b.start % 16 == 0 and b.view.data_ptr() % 16 == 0 and b.view.numel() * b.view.element_size() == b.nbytes
        assert b.guard >= min(max(512 * b.pitch, 4096), 8 << 20)
    assert a.bufs["x"].pitch == 12 and a.bufs["y"].pitch == 12 and a.bufs["x"].guard == 512 * 12 and a.bufs["w"].guard == 8 << 20
    assert Arena.guard_bytes(4) == 4096 and Arena.guard_bytes(1 << 20) == 8 << 20
    assert bool((a["y"].view(torch.uint8) == fill).all()) and not a["img"][4:].any()
    if fill == 0xFF:
        assert bool(torch.isnan(a["y"].float()).all()) and bool(torch.isnan(a["img"][:4]).all())
        assert bool((a["y"].view(torch.int16) == -1).all())
    else:
        y = a["y"].float()
        assert bool(torch.isfinite(y).all()) and bool((y != 0).all())


@pytest.mark.parametrize("where,name,side,offset", [
    ("just_past", "y", "after", 84), ("just_before", "y", "before", -1), ("far_end_of_guard_after", "x", "after", 60 + 512 * 12 - 1),
    ("far_end_of_guard_before", "y", "before", -512 * 12), ("arena_first_byte", "x", "before", None), ("arena_last_byte", "img", "after", None)])
def test_one_stray_byte_in_a_guard_is_named(where, name, side, offset):
    a = _make()
    b = a.bufs[name]
    if where == "arena_first_byte":
        pos, offset = 0, -b.start
    elif where == "arena_last_byte":
        pos, offset = a.total - 1, a.total - 1 - b.start
    else:
        pos = b.start + offset              # offsets are relative to the buffer's first byte: y is 84 bytes, x 60
    a.mem[pos] = 0x01
    with pytest.raises(ArenaError) as e:
        a.check()
    assert "%s: guard %s the buffer changed: first at byte offset %d, 1 bytes" % (name, side, offset) in str(e.value), str(e.value)


def test_a_write_into_an_input_and_into_zero_padding_is_named():
    a = _make()
    a.mem[a.bufs["x"].start + 17] ^= 0x40
    with pytest.raises(ArenaError, match=r"x: input changed: first at byte offset 17, 1 bytes"):
        a.check()
    a = _make()
    a.mem[a.bufs["img"].start + 4 * 128 + 5] = 0x3C
    a.mem[a.bufs["img"].start + 4 * 128 + 9] = 0x3C
    with pytest.raises(ArenaError, match=r"img: zero padding changed: first at byte offset 517, 2 bytes"):
        a.check()
    a = _make()
    a["y"].fill_(1.0)                    # writing the outputs and the workspace themselves is what they are for
    a["w"].fill_(0)
    a["img"][:4] = 2.0
    a.check()
    a.freeze("y")                        # ... until an output becomes an operand
    a["y"][0, 0] = 2.0
    with pytest.raises(ArenaError, match=r"y: input changed: first at byte offset 0, "):
        a.check()


def test_sizes_and_alignment_are_refused():
    a = Arena("cpu", 0xFF)
    with pytest.raises(ArenaError, match="bytes stated"):
        a.reserve("w", (100,), torch.uint8, "ws", nbytes=112)
    with pytest.raises(ArenaError, match="uint8"):
        a.reserve("w", (25,), torch.float32, "ws")
    with pytest.raises(ArenaError, match="unknown role"):
        a.reserve("w", (25,), torch.float32, "scratch")
    a.reserve("x", (5, 3), torch.float32, "in")
    a.allocate()
    with pytest.raises(ArenaError, match="disagrees with its reservation"):
        a.take("x", (5, 4), torch.float32, "in")
    with pytest.raises(ArenaError, match="bytes stated"):
        a.take("x", (5, 3), torch.float32, "in", nbytes=64)
    with pytest.raises(ArenaError, match="not on a 16-byte boundary"):
        a.take("x", (5, 3), torch.float32, "in", start=a.bufs["x"].start + 4)
    with pytest.raises(ArenaError, match="never taken"):
        a.seal()
    with pytest.raises(ArenaError, match="before seal"):
        a.check()
