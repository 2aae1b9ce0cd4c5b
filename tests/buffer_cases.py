"""Shared by the buffer-contract tests (test_buffer_cases.py, test_buffer_contract_gpu.py): a poisoned arena out of which a test carves
every buffer it hands to the library -- at a chosen address skew, with untouched guard bytes on both sides -- and the check that nothing
but the carved outputs changed.  Works on CPU tensors as well (the helper's own tests need no GPU).

Nothing here dereferences memory the test does not own: a skewed or short buffer lies inside the arena with GUARD bytes to spare on
either side, so an overrun of less than that lands in the arena and fails assert_guards instead of touching foreign memory."""
import numpy as np

POISON = 0xA5                      # int32 / int64: a large negative number, int8: -91 -- no H, P, result field or op byte is ever that
GUARD = 256 << 10                  # more than a row of the widest case at 8 bytes per element, far more than 64 lanes x 16 bytes
POISON32 = int(np.frombuffer(bytes([POISON] * 4), np.int32)[0])
POISON64 = int(np.frombuffer(bytes([POISON] * 8), np.int64)[0])
POISON8 = int(np.frombuffer(bytes([POISON]), np.int8)[0])


def poison_of(dtype):
    """The value a poisoned element of a numpy dtype reads as."""
    return np.frombuffer(bytes([POISON] * np.dtype(dtype).itemsize), dtype)[0]


class Carve:
    """A byte range [off, off + nbytes) of an arena.  expect: None -- the library may write it (an output); otherwise the bytes it must
    still hold after the call (poison for a must-stay-untouched range, the letters for an input)."""

    def __init__(self, name, off, nbytes, addr):
        self.name, self.off, self.nbytes, self.addr = name, off, nbytes, addr
        self.expect = None

    @property
    def end(self):
        return self.off + self.nbytes


def arena_bytes(*sizes, guard=GUARD):
    """Bytes an arena needs for carves of these sizes (each with its guards and the worst case of its alignment, up to 4096)."""
    return sum(int(s) + guard + 4096 for s in sizes) + guard


class Arena:
    """One uint8 tensor full of POISON."""

    def __init__(self, torch, device, nbytes):
        self.torch = torch
        self.buf = torch.full((int(nbytes),), POISON, dtype=torch.uint8, device=device)
        self.base = self.buf.data_ptr()
        self.carves = []
        self._cursor, self._last_guard = 0, 0

    def reset(self):
        """Fresh poison everywhere, no carves."""
        self.buf.fill_(POISON)
        self.carves = []
        self._cursor, self._last_guard = 0, 0

    def carve(self, nbytes, align=1, skew=0, guard=GUARD, name=None):
        """A range of nbytes whose device address satisfies addr % align == skew, with at least `guard` untouched bytes on both sides."""
        nbytes, align, skew = int(nbytes), int(align), int(skew)
        assert nbytes >= 0 and align >= 1 and 0 <= skew < align and guard >= 0
        off = self._cursor + max(guard, self._last_guard)
        off += (skew - (self.base + off)) % align
        if off + nbytes + guard > self.buf.numel():
            raise ValueError(f"arena of {self.buf.numel()} bytes is too small for carve {name!r} ({nbytes} bytes at {off}, guard {guard})")
        c = Carve(name if name is not None else f"carve{len(self.carves)}", off, nbytes, self.base + off)
        assert c.addr % align == skew
        self.carves.append(c)
        self._cursor, self._last_guard = c.end, guard
        return c

    def bytes_of(self, c):
        return self.buf[c.off:c.end]

    def view(self, c, dtype, shape):
        """The typed view of a carve.  Skews are multiples of the element size, so the pointer is legal C."""
        t = self.bytes_of(c)
        size = t.new_empty(0, dtype=dtype).element_size()
        assert c.addr % size == 0 and c.nbytes % size == 0, f"{c.name}: address {c.addr:#x} / {c.nbytes} bytes do not suit {dtype}"
        return t.view(dtype).view(shape)

    def must_stay(self, c, expect=None):
        """The library must not change this carve: it keeps the given bytes (default: its poison)."""
        c.expect = np.full(c.nbytes, POISON, np.uint8) if expect is None else np.ascontiguousarray(expect, np.uint8).reshape(-1).copy()
        assert len(c.expect) == c.nbytes
        return c

    def place(self, data, align=1, skew=0, front=None, back=None, guard=GUARD, name=None):
        """An INPUT: `data` (uint8) at an address with addr % align == skew, `front` bytes directly before it and `back` bytes directly
        behind it (live-letter padding), all of it must-stay.  Returns (uint8 view of the data alone, carve)."""
        data = np.ascontiguousarray(data, np.uint8).reshape(-1)
        front = np.zeros(0, np.uint8) if front is None else np.ascontiguousarray(front, np.uint8).reshape(-1)
        back = np.zeros(0, np.uint8) if back is None else np.ascontiguousarray(back, np.uint8).reshape(-1)
        c = self.carve(len(front) + len(data) + len(back), align, (skew - len(front)) % align, guard, name)
        allb = np.concatenate([front, data, back])
        if len(allb):
            self.bytes_of(c).copy_(self.torch.from_numpy(allb.copy()))
        self.must_stay(c, allb)
        t = self.buf[c.off + len(front):c.off + len(front) + len(data)]
        assert len(data) == 0 or t.data_ptr() % align == skew
        return t, c


def _describe(arena, off):
    """Which carve a byte offset lies in or next to."""
    best = None
    for c in arena.carves:
        if c.off <= off < c.end:
            return f"byte {off - c.off} inside must-stay range '{c.name}'"
        d = c.off - off if off < c.off else off - c.end + 1
        if best is None or d < best[0]:
            best = (d, c, "before" if off < c.off else "behind")
    if best is None:
        return "no carve in this arena"
    return f"{best[0]} byte(s) {best[2]} carve '{best[1].name}' [{best[1].off}, {best[1].end})"


def assert_guards(arena):
    """Every byte outside the carved ranges is still POISON and every must-stay range still holds what it held.  Reports the first
    offending offset and the carve it lies in or next to."""
    torch = arena.torch
    want = torch.full_like(arena.buf, POISON)
    check = torch.ones(arena.buf.numel(), dtype=torch.bool, device=arena.buf.device)
    for c in arena.carves:
        if c.expect is None:
            check[c.off:c.end] = False
        elif c.nbytes:
            want[c.off:c.end] = torch.from_numpy(c.expect).to(arena.buf.device)
    bad = (arena.buf != want) & check
    if bool(bad.any()):
        off = int(torch.nonzero(bad)[0, 0])
        raise AssertionError(f"arena byte {off} changed: {int(arena.buf[off]):#04x}, expected {int(want[off]):#04x}; {int(bad.sum())} bytes in all; "
                             f"the first is {_describe(arena, off)}")


def live_tail(seq, n, fallback=b"A"):
    """n bytes of live-letter padding to put BEHIND seq: the sequence's own tail, repeated -- letters of its own alphabet (the kernel the
    planner picks does not change), and read as sequence data they would extend a repeat and raise the score."""
    seq = np.ascontiguousarray(seq, np.uint8).reshape(-1)
    src = seq[-16:] if len(seq) else np.frombuffer(fallback, np.uint8)
    return np.resize(src, n).astype(np.uint8)


def live_head(seq, n, fallback=b"A"):
    """n bytes of live-letter padding to put IN FRONT of seq: its own tail again, so that the bytes before seq[0] continue into it."""
    return live_tail(seq, n, fallback)
