"""A guarded arena: every buffer of a call sequence carved, at exactly the byte extent the C header states, out of ONE uint8 tensor
filled with a known byte, with a guard band of that byte on both sides.  A kernel that writes past a ragged last row, or a workspace
query one slab short, gives correct values in the buffer a test looks at; here the damage lands in a guard and check() names it.

Layout conditions (conditions, not measurements):
  - a buffer starts on a 16-byte boundary and is exactly prod(shape) * itemsize bytes;
  - each guard is at least GUARD_ROWS rows of the buffer's own row pitch (512 = the tallest row tile in the tree, the narrow-output
    tile of mdl_split_gemm_nt), not below GUARD_MIN bytes, and may be capped at GUARD_CAP;
  - the arena begins and ends with EDGE bytes of fill that belong to no buffer, so that an over-read lands in mapped, recognisable
    memory instead of faulting.
Plain torch, device-agnostic: the self-test runs it on CPU tensors.

Use: reserve() every buffer (first pass: sizes only), allocate() once, take() each buffer with the same arguments, fill the inputs,
seal(), run the kernels, synchronize, check()."""
import math

import torch

GUARD_ROWS = 512
GUARD_MIN = 4096
GUARD_CAP = 8 << 20
EDGE = 4 << 20
ALIGN = 16
ROLES = ("in", "out", "inout", "ws")
FILLS = (0xFF, 0x3F)      # every fp32 / fp16 / bf16 pattern a NaN and every integer -1 | finite, non-zero floats


def _up(n, a):
    return (n + a - 1) // a * a


def _itemsize(dtype):
    return torch.empty((), dtype=dtype).element_size()


class ArenaError(AssertionError):
    pass


class _Buf:
    __slots__ = ("name", "shape", "dtype", "role", "nbytes", "pitch", "guard", "start", "view", "snapshot", "zero_tail", "taken")

    def __init__(self, name, shape, dtype, role, nbytes, pitch, guard, zero_tail):
        self.name, self.shape, self.dtype, self.role, self.nbytes, self.pitch, self.guard = name, shape, dtype, role, nbytes, pitch, guard
        self.zero_tail, self.start, self.view, self.snapshot, self.taken = zero_tail, None, None, None, False


class Arena:
    def __init__(self, device, fill):
        assert 0 <= int(fill) <= 255
        self.device, self.fill = torch.device(device), int(fill)
        self.bufs, self.mem, self.sealed = {}, None, False

    # ------------------------------------------------------------------------------------------------------------------ first pass
    @staticmethod
    def guard_bytes(pitch):
        """Bytes of one guard for a buffer whose rows are `pitch` bytes apart."""
        return _up(min(max(GUARD_ROWS * int(pitch), GUARD_MIN), GUARD_CAP), ALIGN)

    def reserve(self, name, shape, dtype, role, nbytes=None, pitch=None, zero_tail=0):
        """Declares a buffer.  shape: its exact shape; nbytes (optional) must equal prod(shape) * itemsize -- a caller that has the
        header's byte count passes it so that a disagreement is refused; pitch: bytes of one row where that is not the product of
        the trailing dimensions (a workspace: the pitch of the widest row it holds; default for 'ws': the guard cap); zero_tail:
        the last `zero_tail` bytes are padding the header requires to be zero, provided and zeroed by the test."""
        if self.mem is not None:
            raise ArenaError("arena: reserve(%s) after allocate()" % name)
        if role not in ROLES:
            raise ArenaError("arena: %s has unknown role %r" % (name, role))
        if name in self.bufs:
            raise ArenaError("arena: %s reserved twice" % name)
        shape = tuple(int(s) for s in shape)
        size = math.prod(shape) * _itemsize(dtype)
        if nbytes is not None and int(nbytes) != size:
            raise ArenaError("arena: %s: %d bytes stated, shape %s of %s is %d" % (name, nbytes, shape, dtype, size))
        if role == "ws" and dtype != torch.uint8:
            raise ArenaError("arena: workspace %s must be taken as uint8 at the byte count of its query" % name)
        if not 0 <= zero_tail <= size:
            raise ArenaError("arena: %s: zero_tail %d outside the buffer" % (name, zero_tail))
        if pitch is None:
            pitch = GUARD_CAP if role == "ws" else (math.prod(shape[1:]) if len(shape) > 1 else 1) * _itemsize(dtype)
        self.bufs[name] = _Buf(name, shape, dtype, role, size, int(pitch), self.guard_bytes(pitch), int(zero_tail))

    def allocate(self):
        if self.mem is not None:
            raise ArenaError("arena: allocated twice")
        pos = EDGE
        for b in self.bufs.values():
            pos = _up(pos + b.guard, ALIGN)
            b.start = pos
            pos = _up(pos + b.nbytes, ALIGN) + b.guard
        self.total = _up(pos, ALIGN) + EDGE
        self.mem = torch.full((self.total,), self.fill, dtype=torch.uint8, device=self.device)
        base = self.mem.data_ptr()
        if base % ALIGN:      # (torch allocations are at least 64-byte aligned; kept as a refusal, not an assumption)
            raise ArenaError("arena: base address %#x is not %d-byte aligned" % (base, ALIGN))

    # ----------------------------------------------------------------------------------------------------------------- second pass
    def take(self, name, shape, dtype, role, nbytes=None, start=None):
        """The view of a reserved buffer: exactly prod(shape) * itemsize bytes, 16-byte aligned, holding the fill."""
        b = self.bufs.get(name)
        if self.mem is None or b is None:
            raise ArenaError("arena: take(%s) without reserve() + allocate()" % name)
        shape = tuple(int(s) for s in shape)
        size = math.prod(shape) * _itemsize(dtype)
        if nbytes is not None and int(nbytes) != size:
            raise ArenaError("arena: %s: %d bytes stated, shape %s of %s is %d" % (name, nbytes, shape, dtype, size))
        if (shape, dtype, role, size) != (b.shape, b.dtype, b.role, b.nbytes):
            raise ArenaError("arena: take(%s) disagrees with its reservation" % name)
        if b.taken:
            raise ArenaError("arena: %s taken twice" % name)
        at = b.start if start is None else int(start)
        if at % ALIGN or (self.mem.data_ptr() + at) % ALIGN:
            raise ArenaError("arena: %s would start at byte %d, not on a %d-byte boundary" % (name, at, ALIGN))
        b.start = at
        b.view = self.mem[b.start:b.start + b.nbytes].view(dtype).view(shape) if size else self.mem[b.start:b.start].view(dtype).view(shape)
        b.taken = True
        if b.zero_tail:
            self.mem[b.start + b.nbytes - b.zero_tail:b.start + b.nbytes] = 0
        return b.view

    def __getitem__(self, name):
        return self.bufs[name].view

    def seal(self):
        """Call once the inputs hold what the test puts in: snapshots every 'in' buffer."""
        for b in self.bufs.values():
            if not b.taken:
                raise ArenaError("arena: %s reserved and never taken" % b.name)
            if b.role == "in":
                b.snapshot = self._bytes(b).clone()
        self.sealed = True

    def freeze(self, name):
        """From here on `name` is an operand: a buffer one call of the sequence wrote (an image built in place) and later calls only
        read.  check() then holds it to its contents of this moment.  The caller synchronizes first."""
        b = self.bufs[name]
        b.snapshot = self._bytes(b).clone()

    def _bytes(self, b):
        return self.mem[b.start:b.start + b.nbytes]

    # ----------------------------------------------------------------------------------------------------------------------- check
    def _regions(self):
        """(name, side, lo, hi, origin): every guard region; the offsets check() reports are byte - origin, relative to the buffer's
        first byte: negative before it, from the buffer's size upwards after it."""
        order = sorted(self.bufs.values(), key=lambda b: b.start)
        out, prev_end, prev = [], 0, None
        for b in order:
            if prev is None:                                   # the first buffer also owns the leading edge
                out.append((b.name, "before", 0, b.start, b.start))
            else:                                              # [prev's guard | alignment | b's guard]: split behind prev's guard
                mid = min(prev_end + prev.guard, b.start)
                out.append((prev.name, "after", prev_end, mid, prev.start))
                out.append((b.name, "before", mid, b.start, b.start))
            prev, prev_end = b, b.start + b.nbytes
        if prev is not None:
            out.append((prev.name, "after", prev_end, self.total, prev.start))
        return out

    def _diff(self, lo, hi, expected):
        """(first changed offset from lo, changed count) of mem[lo:hi] against a byte or a tensor; None when equal."""
        cur = self.mem[lo:hi]
        bad = cur != expected
        n = int(bad.sum())
        if n == 0:
            return None
        return int(torch.nonzero(bad)[0]), n

    def check(self):
        """After torch.cuda.synchronize(): every guard byte still equals the fill, every 'in' buffer (and every frozen one) is bit
        for bit what the test put in, every documented zero padding is still zero.  Names the buffer, the side, the first changed
        byte offset relative to the buffer and the number of changed bytes."""
        if not self.sealed:
            raise ArenaError("arena: check() before seal()")
        errors = []
        if self.mem is None or not self.bufs:
            return
        # one reduction for the common case: everything intact
        regions = self._regions()
        flags = [(self.mem[lo:hi] != self.fill).any() for _, _, lo, hi, _ in regions]
        snaps = [b for b in self.bufs.values() if b.snapshot is not None]
        flags += [(self._bytes(b) != b.snapshot).any() for b in snaps]
        zeros = [b for b in self.bufs.values() if b.zero_tail]
        flags += [(self.mem[b.start + b.nbytes - b.zero_tail:b.start + b.nbytes] != 0).any() for b in zeros]
        if not bool(torch.stack(flags).any()):
            return
        for name, side, lo, hi, origin in regions:
            d = self._diff(lo, hi, self.fill)
            if d is not None:
                errors.append("%s: guard %s the buffer changed: first at byte offset %d, %d bytes" % (name, side, lo + d[0] - origin, d[1]))
        for b in snaps:
            d = self._diff(b.start, b.start + b.nbytes, b.snapshot)
            if d is not None:
                errors.append("%s: input changed: first at byte offset %d, %d bytes" % (b.name, d[0], d[1]))
        for b in zeros:
            lo = b.start + b.nbytes - b.zero_tail
            d = self._diff(lo, b.start + b.nbytes, 0)
            if d is not None:
                errors.append("%s: zero padding changed: first at byte offset %d, %d bytes" % (b.name, lo + d[0] - b.start, d[1]))
        raise ArenaError("arena (fill %#04x): " % self.fill + "; ".join(errors))
