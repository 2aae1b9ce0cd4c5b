"""Targets for the tests of the low-complexity mask (sw_db_mask_low_complexity / sw_mask_low_complexity_host): an INDEPENDENT restatement
of the rule of include/swhip.h in numpy -- window by window, np.bincount, the table G recomputed from its formula, so it also pins the
literals of csrc/sw_mask_table.h --, hand-made targets for every clause of the rule, random targets of two compositions, and a
database laid out against the tile borders of the device call.  No GPU, no library call."""
import math

import numpy as np

AA = b"ACDEFGHIKLMNPQRSTVWY"
DEFAULT = dict(window=12, trigger_mbits=2200, extend_mbits=2500, letters=AA, mask_byte=ord("X"))
GUARD, POISON = 64, 0xA5
G = [0, 0] + [int(math.floor(c * math.log2(c) * 65536 + 0.5)) for c in range(2, 65)]


def params(**kw):
    p = dict(DEFAULT)
    p.update(kw)
    return p


def pack(targets, first=0, tail=0, fill=POISON):
    """(packed uint8 with `first` bytes in front and `tail` behind, int64 offsets starting at `first`)."""
    offs = np.zeros(len(targets) + 1, np.int64)
    offs[0] = first
    if targets:
        offs[1:] = first + np.cumsum([len(t) for t in targets])
    packed = np.full(int(offs[-1]) + tail, fill, np.uint8)
    if targets and offs[-1] > first:
        packed[first:int(offs[-1])] = np.frombuffer(b"".join(bytes(t) for t in targets), np.uint8)
    return packed, offs


def lows(target, window=12, trigger_mbits=2200, extend_mbits=2500, letters=AA, **_):
    """(low1, low2) of every start 0 .. len - W of one target (empty arrays for a target shorter than W), and D per start (-1: not valid)."""
    t = np.frombuffer(bytes(target), np.uint8)
    W = int(window)
    cls = np.full(256, -1, np.int64)
    for k, b in enumerate(bytes(letters)):
        cls[b] = k
    c = cls[t]
    n = max(0, len(t) - W + 1)
    low1, low2, D = np.zeros(n, bool), np.zeros(n, bool), np.full(n, -1, np.int64)
    for i in range(n):
        w = c[i:i + W]
        if (w < 0).any():
            continue
        D[i] = G[W] - sum(G[int(x)] for x in np.bincount(w, minlength=32))
        low1[i] = 1000 * int(D[i]) <= int(trigger_mbits) * W * 65536
        low2[i] = 1000 * int(D[i]) <= int(extend_mbits) * W * 65536
    return low1, low2, D


def runs(low2):
    """The maximal runs (s, e) of consecutive starts with low2."""
    out, i, n = [], 0, len(low2)
    while i < n:
        if not low2[i]:
            i += 1
            continue
        e = i
        while e + 1 < n and low2[e + 1]:
            e += 1
        out.append((i, e))
        i = e + 1
    return out


def reference(packed, offs, **p):
    """The rule, restated: (out, nmasked); `out` is a copy of `packed` outside [offs[0], offs[-1])."""
    p = params(**p)
    W = int(p["window"])
    out = np.array(packed, np.uint8, copy=True)
    nmasked = np.zeros(len(offs) - 1, np.int64)
    for k in range(len(offs) - 1):
        b, e = int(offs[k]), int(offs[k + 1])
        low1, low2, _ = lows(packed[b:e].tobytes(), **p)
        masked = np.zeros(e - b, bool)
        for s, last in runs(low2):
            if low1[s:last + 1].any():
                masked[s:last + W] = True
        out[b:e][masked] = p["mask_byte"]
        nmasked[k] = int(masked.sum())
    return out, nmasked


def composed(counts, letters=AA):
    """A window of the given composition: counts[k] times letters[k], sorted."""
    return b"".join(bytes([letters[k]]) * n for k, n in enumerate(counts))


# ---- hand-made targets under the default rule (W 12, 2200 / 2500); tests/test_mask_host.py asserts the property each one is named for
# from lows() and runs().  A window of the period-five pattern has the counts {3, 3, 2, 2, 2}: 2.29 bits, low2 and never low1; with
# three more A in front the first window has {5, 2, 2, 2, 1}: 2.12 bits, low1, and the next two {4, 2, 2, 2, 2}: 2.25 bits.
RUN_NO_TRIGGER = b"ACDEF" * 6
RUN_TRIGGER_FIRST = b"AAA" + b"ACDEF" * 5              # one run, low1 at its first start only
RUN_TRIGGER_LAST = RUN_TRIGGER_FIRST[::-1]             # ... at its last start only
TWO_RUNS = b"A" * 16 + b"CDEFGHIK" + b"Q" * 14         # the runs 0..10 and 18..26: masked [0, 22) and [18, 38)


def hand_targets(W=12):
    """name -> list of targets, all under the default rule with window W (the named properties hold for W = 12)."""
    a = b"A" * W
    return {
        "len 0": [b""],
        "len 1": [b"A"],
        "len W-1": [b"A" * (W - 1)],
        "len W": [a],
        "len W+1": [b"A" * (W + 1)],
        "two of W-1": [b"A" * (W - 1), b"A" * (W - 1)],
        "adjacent": [b"CDEFGHIKLMNPQRSTVWY" + a, a + b"CDEFGHIKLMNPQRSTVWY"],
        "empty between": [a, b"", b"", a, b""],
        "trigger first": [RUN_TRIGGER_FIRST],
        "trigger last": [RUN_TRIGGER_LAST],
        "no trigger": [RUN_NO_TRIGGER],
        "two runs": [TWO_RUNS],
        "no-letter splits": [b"A" * (W - 1) + b"*" + b"A" * (W - 1), b"A" * W + b"*" + b"A" * W],
        "bytes >= 128": [bytes([200]) * 20 + a + bytes([255, 128, 0]) + a[:W - 1] + bytes([130])],
    }


def hand_database(W=12, first=0):
    """Every hand-made target in one database: (packed, offs)."""
    targets = [t for ts in hand_targets(W).values() for t in ts]
    return pack(targets, first=first, tail=GUARD if first else 0)


def random_targets(n, lo, hi, seed, skewed=False, alphabet=AA):
    """n seeded random targets with lengths lo .. hi: uniform letters, or a skewed composition (a geometric fall-off over a shuffled
    alphabet, redrawn per target, so that some targets are nearly one letter)."""
    r = np.random.default_rng(seed)
    letters = np.frombuffer(bytes(alphabet), np.uint8)
    out = []
    for _ in range(n):
        ln = int(r.integers(lo, hi + 1))
        if skewed:
            w = float(r.choice([0.5, 0.7, 0.85])) ** np.arange(len(letters))
            w = r.permutation(w / w.sum())
            out.append(letters[r.choice(len(letters), size=ln, p=w)].tobytes())
        else:
            out.append(letters[r.integers(0, len(letters), size=ln)].tobytes())
    return out


# ---- a database laid out against the tile borders of the device call.  A stretch between two no-letters '*' gives a run whose starts
# are known exactly: a stretch of L letters at position s whose windows are all low2 is the run s .. s + L - W.
P5 = b"ACDEF"          # period 5: low2, never low1 (RUN_NO_TRIGGER)


def _stretch(kind, L, W=12):
    """L letters: 'a' poly-A (low1 throughout); '5' period five (low2 only); '<' / '>' period five with W letters A at its left / right end."""
    body = (P5 * (L // 5 + 1))[:L]
    if kind == "a":
        return b"A" * L
    if kind == "5":
        return body
    if kind == "<":
        return b"A" * W + body[W:]
    return body[:L - W] + b"A" * W


def tile_database(T, W=12):
    """(targets, notes): targets whose concatenation from position 0 places, with T the tile size:
      a run across one border (poly-A, T - 20 .. T + 30);
      a run that ends with its last start on the last position of a tile, and the next run starting on the first position of the next;
      a masked stretch that ends exactly on a border; a target that ends exactly on a border;
      a run across three borders with its only trigger at its left end, then one with its only trigger at its right end, each holding
      whole tiles; an untriggered run across two borders.
    notes: name -> (first position, length) of the stretch."""
    flat = bytearray()
    cuts = []           # target ends
    notes = {}
    r = np.random.default_rng(99)
    letters = np.frombuffer(AA, np.uint8)

    def filler_to(pos):
        n = pos - len(flat)
        assert n >= 0, (pos, len(flat))
        flat.extend(letters[r.integers(0, 20, size=n)].tobytes())

    def put(name, pos, kind, L):
        filler_to(pos - 1)
        flat.extend(b"*")
        notes[name] = (pos, L)
        flat.extend(_stretch(kind, L, W))
        flat.extend(b"*")

    put("across one", T - 20, "a", 50)
    cuts.append(T + 200)
    put("ends on border", 2 * T - 1 - 40, "a", 40 + W)             # starts .. 2T - 1: the last start is the tile's last position
    filler_to(2 * T - 1 + W + 1)
    cuts.append(len(flat))
    put("masked to border", 3 * T - 30, "a", 30)                   # masked [3T - 30, 3T)
    put("starts on border", 4 * T, "a", 20)
    filler_to(5 * T)
    cuts.append(5 * T)                                             # a target that ends exactly on a border
    put("trigger left", 5 * T + 100, "<", 3 * T + 200)             # across 6T, 7T, 8T; tiles 6 and 7 whole
    put("trigger right", 9 * T - 50, ">", 3 * T + 100)             # across 9T, 10T, 11T; tiles 9 and 10 whole
    put("no trigger", 12 * T + 500, "5", 2 * T)                    # across 13T, 14T
    filler_to(14 * T + 700)
    cuts.append(len(flat))
    targets, b = [], 0
    for c in cuts:
        targets.append(bytes(flat[b:c]))
        b = c
    return targets, notes
