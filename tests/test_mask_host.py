"""CPU: the host leg of the low-complexity mask (sw_mask_low_complexity_host) against the numpy restatement of tests/mask_cases.py, byte
for byte and count for count: the exact entropy boundaries of hand-built windows, target lengths around the window, adjacent and empty
targets, runs triggered at their first start, at their last and not at all, overlapping dilations, no-letters, bytes >= 128, a mask
byte that is a letter, windows 2 and 64, an odd offsets[0] with poisoned bytes around the range, every refusal, and 400 random
targets of each of two compositions.  The restatement recomputes G from its formula, so the literals of csrc/sw_mask_table.h are
pinned too."""
import ctypes
import os
import re

import numpy as np
import pytest

import mask_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def both(swamd, targets, first=0, **p):
    """Host leg and restatement on the same bytes; returns (out, nmasked, offs) after comparing them."""
    packed, offs = mc.pack(targets, first=first, tail=mc.GUARD if first else 0)
    p = mc.params(**p)
    out, n = swamd.mask_low_complexity_host((packed, offs), **p)
    ref, nref = mc.reference(packed, offs, **p)
    assert np.array_equal(out, ref) and np.array_equal(n, nref)
    return out, n, offs


def test_table_literals_are_the_formula():
    text = open(os.path.join(ROOT, "smith-waterman_amd", "csrc", "sw_mask_table.h")).read()
    body = text[text.index("#define SW_MASK_G_LITERALS"):]
    lits = [int(x) for x in re.findall(r"\b\d+\b", body.replace("\\", " "))]
    assert lits == mc.G and len(lits) == 65
    assert (mc.G[2], mc.G[3], mc.G[12], mc.G[64]) == (131072, 311616, 2819329, 25165824)


@pytest.mark.parametrize("counts,k_low,thousand_d", [([6, 6], 1000, 786_431_000), ([4, 3, 2, 2, 1], 2189, 1_721_281_000), ([12], 0, 0)])
def test_exact_boundaries(swamd, counts, k_low, thousand_d):
    w = mc.composed(counts)
    _, _, D = mc.lows(w)
    assert len(w) == 12 and 1000 * int(D[0]) == thousand_d
    assert 1000 * int(D[0]) <= k_low * 12 * 65536 and (k_low == 0 or 1000 * int(D[0]) > (k_low - 1) * 12 * 65536)
    # one window, both bounds together: masked whole at k_low, untouched one below
    _, n, _ = both(swamd, [w], trigger_mbits=k_low, extend_mbits=k_low)
    assert n[0] == 12
    if k_low:
        _, n, _ = both(swamd, [w], trigger_mbits=k_low - 1, extend_mbits=k_low - 1)
        assert n[0] == 0
        # the trigger bound alone: the window stays low2, and is masked only where it is low1
        _, n, _ = both(swamd, [w], trigger_mbits=k_low, extend_mbits=5000)
        assert n[0] == 12
        _, n, _ = both(swamd, [w], trigger_mbits=k_low - 1, extend_mbits=5000)
        assert n[0] == 0


def test_extend_bound_alone(swamd):
    # 13 letters: window 0 has the counts {5, 3, 2, 2}, window 1 {4, 3, 2, 2, 1}; the trigger bound admits window 0 only, the extend
    # bound decides whether window 1 joins its run, that is whether the thirteenth letter is masked
    t = b"A" + b"AAAACCCDDEE" + b"F"
    _, _, D = mc.lows(t)
    assert sorted(np.bincount(np.frombuffer(t[1:], np.uint8))[65:].tolist(), reverse=True)[:5] == [4, 3, 2, 2, 1]
    k1 = -(-1000 * int(D[0]) // (12 * 65536))
    assert 1000 * int(D[1]) == 1_721_281_000 and k1 < 2188
    out, n, _ = both(swamd, [t], trigger_mbits=k1, extend_mbits=2189)
    assert n[0] == 13
    out, n, _ = both(swamd, [t], trigger_mbits=k1, extend_mbits=2188)
    assert n[0] == 12 and out[12] == ord("F")


def test_target_lengths(swamd):
    W = 12
    h = mc.hand_targets(W)
    for name, want in (("len 0", [0]), ("len 1", [0]), ("len W-1", [0]), ("len W", [W]), ("len W+1", [W + 1]), ("two of W-1", [0, 0])):
        out, n, offs = both(swamd, h[name])
        assert n.tolist() == want


def test_adjacent_targets_are_masked_and_counted_apart(swamd):
    out, n, offs = both(swamd, mc.hand_targets()["adjacent"])
    # the window of 12 A with up to 6 other letters beside it stays low: some flank is masked on the far side, none across the border
    assert n[0] >= 12 and n[1] >= 12 and (out[int(offs[1]) - 12:int(offs[1]) + 12] == ord("X")).all()
    out, n, _ = both(swamd, mc.hand_targets()["empty between"])
    assert n.tolist() == [12, 0, 0, 12, 0]


def test_runs_and_triggers(swamd):
    l1, l2, _ = mc.lows(mc.RUN_TRIGGER_FIRST)
    assert mc.runs(l2) == [(0, 16)] and np.nonzero(l1)[0].tolist() == [0]
    l1, l2, _ = mc.lows(mc.RUN_TRIGGER_LAST)
    assert mc.runs(l2) == [(0, 16)] and np.nonzero(l1)[0].tolist() == [16]
    l1, l2, _ = mc.lows(mc.RUN_NO_TRIGGER)
    assert mc.runs(l2) == [(0, 18)] and not l1.any()
    l1, l2, _ = mc.lows(mc.TWO_RUNS)
    assert mc.runs(l2) == [(0, 10), (18, 26)] and l1[0] and l1[26]       # masked [0, 22) and [18, 38): they overlap
    h = mc.hand_targets()
    assert both(swamd, h["trigger first"])[1][0] == len(mc.RUN_TRIGGER_FIRST)
    assert both(swamd, h["trigger last"])[1][0] == len(mc.RUN_TRIGGER_LAST)
    assert both(swamd, h["no trigger"])[1][0] == 0
    assert both(swamd, h["two runs"])[1][0] == 38


def test_bytes(swamd):
    h = mc.hand_targets()
    out, n, offs = both(swamd, h["no-letter splits"])
    assert n.tolist() == [0, 24] and out[int(offs[1]) + 12] == ord("*")
    out, n, _ = both(swamd, h["bytes >= 128"])
    assert n[0] == 12 and (out[:20] == 200).all()
    # bytes >= 128 as letters, and a mask byte that is itself a letter
    t = [bytes([200]) * 12 + bytes([201, 202, 203, 204, 205, 206, 207, 208, 209, 210, 211, 212])]
    out, n, _ = both(swamd, t, letters=bytes(range(200, 220)), mask_byte=201)
    assert n[0] >= 12 and (out[:12] == 201).all()
    out, n, _ = both(swamd, [b"A" * 30 + b"CDEFGHIKLMNPQRSTVWY"], mask_byte=ord("A"))
    assert n[0] >= 30


@pytest.mark.parametrize("W", [2, 64])
def test_window_sizes(swamd, W):
    for ts in mc.hand_targets(W).values():
        both(swamd, ts, window=W)
    both(swamd, mc.random_targets(40, 0, 300, seed=W, skewed=True), window=W)
    k1, k2 = {2: (0, 0), 64: (1300, 1500)}[W]          # over three letters, bounds under which some letters are masked and some are not
    _, n, offs = both(swamd, mc.random_targets(40, 0, 300, seed=W + 1, skewed=True, alphabet=b"ACD"), window=W, trigger_mbits=k1, extend_mbits=k2)
    assert 0 < n.sum() < int(offs[-1])
    # a window of one letter is low at 0 millibits whatever W
    _, n, _ = both(swamd, [b"C" * W, b"C" * (W - 1)], window=W, trigger_mbits=0, extend_mbits=0)
    assert n.tolist() == [W, 0]


def test_odd_first_offset_and_untouched_bytes(swamd):
    packed, offs = mc.hand_database(first=77)
    out = np.full(len(packed), 0x5A, np.uint8)
    res, n = swamd.mask_low_complexity_host((packed, offs), out=out)
    assert res is out and (out[:77] == 0x5A).all() and (out[int(offs[-1]):] == 0x5A).all() and len(out) - int(offs[-1]) == mc.GUARD
    ref, nref = mc.reference(packed, offs)
    assert np.array_equal(out[77:int(offs[-1])], ref[77:int(offs[-1])]) and np.array_equal(n, nref) and n.sum() > 0


def test_refusals(swamd):
    t = [b"A" * 20]
    bad = [dict(window=1), dict(window=65), dict(trigger_mbits=-1), dict(trigger_mbits=2600), dict(extend_mbits=1 << 62),
           dict(window=64, extend_mbits=(1 << 63) // (64 * 65536) + 1), dict(letters=b""), dict(letters=b"ACDA"), dict(letters=b"A" * 2 + b"C")]
    for kw in bad:
        with pytest.raises(Exception, match="sw_mask_low_complexity_host"):
            swamd.mask_low_complexity_host(t, **mc.params(**kw))
    with pytest.raises(ValueError):
        swamd.mask_low_complexity_host(t, letters=bytes(range(33)))
    # the largest bound that stays inside 64 bits is taken
    out, n = swamd.mask_low_complexity_host(t, window=64, extend_mbits=(1 << 63) // (64 * 65536) - 1)
    assert n[0] == 0
    # the C call itself: NULL pointers, in place, decreasing offsets
    lib = swamd.lib()
    mp = swamd._mask_params()
    seq = np.frombuffer(b"A" * 20, np.uint8).copy()
    out = np.zeros(20, np.uint8)
    offs = np.array([0, 20], np.int64)
    call = lambda s, o, n, p, d: lib.sw_mask_low_complexity_host(s, o, n, p, d, None)
    assert call(seq.ctypes.data, offs.ctypes.data, 1, ctypes.byref(mp), out.ctypes.data) == 0 and (out == ord("X")).all()
    assert call(None, offs.ctypes.data, 1, ctypes.byref(mp), out.ctypes.data) == -22
    assert call(seq.ctypes.data, None, 1, ctypes.byref(mp), out.ctypes.data) == -22
    assert call(seq.ctypes.data, offs.ctypes.data, 1, None, out.ctypes.data) == -22
    assert call(seq.ctypes.data, offs.ctypes.data, 1, ctypes.byref(mp), None) == -22
    assert call(seq.ctypes.data, offs.ctypes.data, -1, ctypes.byref(mp), out.ctypes.data) == -22
    assert call(seq.ctypes.data, offs.ctypes.data, 1, ctypes.byref(mp), seq.ctypes.data) == -22           # in place
    down = np.array([0, 20, 10], np.int64)
    assert call(seq.ctypes.data, down.ctypes.data, 2, ctypes.byref(mp), out.ctypes.data) == -22


@pytest.mark.parametrize("skewed", [False, True])
def test_random_targets(swamd, skewed):
    targets = mc.random_targets(400, 0, 400, seed=11 + skewed, skewed=skewed)
    out, n, offs = both(swamd, targets)
    frac = n.sum() / max(1, int(offs[-1]))
    assert (frac > 0.05) if skewed else (0 < frac < 0.03)
