"""The arena helper of the buffer-contract tests (tests/buffer_cases.py) on CPU tensors: carved addresses, guards, and that a planted
byte is found and attributed to the right neighbour."""
import numpy as np
import pytest
import torch

from buffer_cases import GUARD, POISON, POISON8, POISON32, POISON64, Arena, arena_bytes, assert_guards, live_tail, poison_of

SMALL = 512           # guard of the self-tests: the logic does not depend on its size


def _arena(n=1 << 16):
    return Arena(torch, "cpu", n)


def test_poison_values():
    assert (POISON8, POISON32, POISON64) == (-91, -1515870811, -6510615555426900571)
    assert poison_of(np.int32) == POISON32 and poison_of(np.int8) == POISON8 and poison_of(np.int64) == POISON64
    assert GUARD == 256 * 1024 and GUARD > 21422 * 8 and GUARD > 64 * 16


@pytest.mark.parametrize("align,skew", [(1, 0), (8, 4), (16, 8), (64, 1), (64, 3), (64, 7), (256, 4), (512, 0), (4096, 12)])
def test_carved_addresses_honour_align_and_skew(align, skew):
    ar = _arena()
    cs = [ar.carve(n, align, skew, guard=SMALL, name=f"c{n}") for n in (0, 1, 7, 64, 1000)]
    for c in cs:
        assert c.addr % align == skew and c.addr == ar.base + c.off
        assert ar.bytes_of(c).data_ptr() == c.addr if c.nbytes else True
    assert_guards(ar)


def test_carves_never_overlap_and_keep_their_guards():
    ar = _arena(1 << 18)
    rng = np.random.default_rng(1)
    spans = []
    for k in range(40):
        g = int(rng.choice([0, 16, SMALL, 2000]))
        c = ar.carve(int(rng.integers(0, 700)), int(rng.choice([1, 4, 16, 64, 256])), 0, guard=g, name=f"c{k}")
        spans.append((c.off, c.end, g))
    assert spans[0][0] >= spans[0][2]
    for (o0, e0, g0), (o1, e1, g1) in zip(spans, spans[1:]):
        assert o1 - e0 >= max(g0, g1)
    assert ar.buf.numel() - spans[-1][1] >= spans[-1][2]
    with pytest.raises(ValueError, match="too small"):
        ar.carve(1 << 18, guard=SMALL)
    assert arena_bytes(100, 200, guard=SMALL) >= 300 + 3 * SMALL


def test_typed_views_alias_the_carve():
    ar = _arena()
    c = ar.carve(6 * 4, 16, 4, guard=SMALL, name="m")
    v = ar.view(c, torch.int32, (2, 3))
    assert v.data_ptr() == c.addr and v.data_ptr() % 16 == 4
    assert bool((v == POISON32).all())
    v[1, 2] = 7
    assert ar.buf[c.off + 20:c.off + 24].tolist() == [7, 0, 0, 0]
    assert_guards(ar)                           # an output carve may change
    c8 = ar.carve(5, 8, 3, guard=SMALL)
    assert bool((ar.view(c8, torch.int8, (5,)) == POISON8).all())
    c64 = ar.carve(16, 16, 8, guard=SMALL)
    assert bool((ar.view(c64, torch.int64, (2,)) == POISON64).all())
    with pytest.raises(AssertionError):
        ar.view(ar.carve(8, 8, 2, guard=SMALL), torch.int32, (2,))


def test_untouched_arena_passes():
    ar = _arena()
    assert_guards(ar)
    a, b = ar.carve(100, guard=SMALL, name="a"), ar.carve(50, 64, 9, guard=SMALL, name="b")
    ar.must_stay(b)
    assert_guards(ar)
    ar.bytes_of(a).fill_(0)                     # the whole of an output carve, first and last byte included
    assert_guards(ar)


def test_planted_bytes_are_found_and_attributed():
    ar = _arena()
    a = ar.carve(100, guard=SMALL, name="first")
    b = ar.carve(64, 64, 4, guard=SMALL, name="second")
    keep = ar.must_stay(ar.carve(32, guard=SMALL, name="kept"))

    def planted(off, value=0):
        old = int(ar.buf[off])
        ar.buf[off] = value
        with pytest.raises(AssertionError) as e:
            assert_guards(ar)
        ar.buf[off] = old
        assert_guards(ar)
        return str(e.value)

    assert "1 byte(s) before carve 'first'" in planted(a.off - 1)
    assert "1 byte(s) behind carve 'first'" in planted(a.end)
    assert "1 byte(s) before carve 'second'" in planted(b.off - 1)
    assert "3 byte(s) behind carve 'second'" in planted(b.end + 2)
    msg = planted(keep.off + 5, 1)
    assert "byte 5 inside must-stay range 'kept'" in msg and "0x01" in msg and f"{POISON:#04x}" in msg
    assert "behind carve 'kept'" in planted(ar.buf.numel() - 1)        # the arena's last byte
    assert "before carve 'first'" in planted(0)
    # two bytes: the first is reported, both are counted
    ar.buf[b.end + 7] = 0
    ar.buf[a.off - 3] = 0
    with pytest.raises(AssertionError, match=r"arena byte %d changed.*2 bytes in all.*3 byte\(s\) before carve 'first'" % (a.off - 3)):
        assert_guards(ar)


def test_placed_inputs_carry_live_padding_and_must_stay():
    ar = _arena()
    seq = np.frombuffer(b"ACGTTGCAAC", np.uint8)
    t, c = ar.place(seq, 16, 3, front=live_tail(seq, 64), back=live_tail(seq, 64), guard=SMALL, name="query")
    assert t.data_ptr() % 16 == 3 and bytes(t.numpy()) == b"ACGTTGCAAC"
    around = ar.buf[c.off:c.end].numpy()
    assert len(around) == 138 and set(around.tolist()) <= set(seq.tolist())      # the alphabet did not grow
    assert bytes(around[64 + 10:64 + 20]) == b"ACGTTGCAAC"                         # the tail again, directly behind
    assert_guards(ar)
    t[2] = ord("A")
    with pytest.raises(AssertionError, match="byte 66 inside must-stay range 'query'"):
        assert_guards(ar)
    assert bytes(live_tail(np.zeros(0, np.uint8), 3, b"C")) == b"CCC"


def test_reset_poisons_again():
    ar = _arena()
    c = ar.carve(10, guard=SMALL)
    ar.bytes_of(c).fill_(1)
    ar.reset()
    assert ar.carves == [] and bool((ar.buf == POISON).all())
    assert ar.carve(10, guard=SMALL).off == c.off
