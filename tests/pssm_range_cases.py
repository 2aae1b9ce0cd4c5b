"""Shared by test_pssm_range_host.py and test_pssm_range_gpu.py: the case table that places the position-specific calls
(sw_db_search_pssm, sw_db_search_pssm_top, sw_db_align_pssm_hits and their host legs) at the edges of their value range and of their
alphabet.  Plain data, no GPU: four kinds of matrix whose entries reach -128 and 127, five (other, smax) pairs, alphabets of 1 .. 256
letters that begin with the bytes 0x00, 0x7F, 0x80 and 0xFF, targets drawn from all 256 byte values, the seven gap pairs of
tests/affine_range_cases.py, and the expectations of the independent checker (tests/affine_oracle.cpp; walk() of tests/align_cases.py),
each computed once per process, shared by the tests and read-only.

A matrix goes to the checker the way tests/pssm_cases.py puts it: at most 256 column TYPES, the "query" whose byte j names the type of
column j, and the (256, 256) table sub[type][x] built here in numpy from the rule of include/swhip.h -- min(entry, smax) for a listed
byte, `other` for every other byte.  Nothing here shares code with the library.

Not the full cross product: every alphabet runs under `full8` with (-128, 127) and with one clamping pair, and every matrix runs
under every pair at 4, 253 and 256 letters (CASES)."""
import functools

import numpy as np

import affine_range_cases as arc

QLENS = [1, 63, 256, 257, 513, 1025]              # 4, 8 and 16 columns per lane; one and two strips at 16
TLENS = arc.TLENS
QFRONT, FRONT = 3, 3                              # qoffsets[0], offsets[0]
MATRICES = ["full8", "floor", "ceiling", "corners"]
SCORINGS = [(-128, 127), (-128, 0), (0, 0), (127, 127), (-1, 1)]      # (other, smax)
NLETTERS = [1, 2, 3, 4, 5, 252, 253, 254, 255, 256]                   # 252 | 253: the odd-stride LDS layout | the swizzled one
MAIN_NLETTERS = [4, 253, 256]
CLAMPING = (-1, 1)
GAPS = arc.GAPS

CASES = [("full8", sc, n) for n in NLETTERS for sc in ((-128, 127), CLAMPING)]
CASES += [(m, sc, n) for m in MATRICES for sc in SCORINGS for n in MAIN_NLETTERS if (m, sc, n) not in CASES]
assert len(CASES) == 20 + 60 - 6 and len(set(CASES)) == len(CASES)

ALIGN_QUERIES = [1, 3, 4, 5]                      # the queries of 63, 257, 513 and 1025 columns
ALIGN_TARGETS = arc.ALIGN_TARGETS                 # the targets of 65, 300, 1100 and 127 letters
ALIGN_GAPS = arc.ALIGN_GAPS
ALIGN_CASES = [("full8", (-128, 127), 253), ("corners", (-128, 127), 253), ("ceiling", (-128, 127), 253), ("full8", CLAMPING, 4)]
assert [QLENS[q] for q in ALIGN_QUERIES] == [63, 257, 513, 1025] and all(c in CASES for c in ALIGN_CASES)

TOP_CASES = [(m, (-128, 127), n) for m in ("full8", "corners", "ceiling") for n in MAIN_NLETTERS]
TOP_GAPS = [(-11, -1), (0, 0)]

# where each planted homologue comes from: target -> (query, first column, columns).  The 257-column query fills a 300-letter target
# (a query of at most 258 columns that scores above 1000), the 1025-column one a 1100-letter target (a score above 32767).
PLANTS = {4: (1, 0, 63), 5: (3, 0, 257), 6: (5, 40, 960), 9: (4, 100, 120)}


def case_id(c):
    return f"{c[0]}_o{c[1][0]}_s{c[1][1]}_n{c[2]}"


@functools.lru_cache(maxsize=None)
def alphabet():
    """All 256 byte values: 0x00, 0x7F, 0x80, 0xFF first, the rest shuffled.  An alphabet of n letters is its first n bytes, so the
    252 letters are the first 252 of the 253."""
    first = np.array([0x00, 0x7F, 0x80, 0xFF], np.uint8)
    rest = np.random.default_rng(256).permutation(np.setdiff1d(np.arange(256, dtype=np.uint8), first))
    a = np.concatenate([first, rest]).astype(np.uint8)
    assert len(set(a.tolist())) == 256
    a.setflags(write=False)
    return a


def letters_of(n):
    return alphabet()[:n]


class World:
    """One matrix kind at one alphabet: 256 column types over the letters, the queries that name types, the targets, and both views --
    the column-major matrix the library takes and the (type string, table) pair the checker takes."""

    def __init__(self, kind, n):
        rng = np.random.default_rng(1000 * MATRICES.index(kind) + n)
        self.kind, self.n, self.letters = kind, n, letters_of(n)
        if kind == "full8":                                    # uniform over -128 .. 127, every type holds both ends where two letters fit
            types = rng.integers(-128, 128, (256, n)).astype(np.int8)
            if n >= 2:
                for t in range(256):
                    a, b = rng.choice(n, 2, replace=False)
                    if t % 8 == 0 and a != n - 1:              # every eighth type has its 127 at the LAST letter, so that letter decides
                        b = n - 1
                    types[t, a], types[t, b] = -128, 127
            else:
                types[:2, 0] = (127, -128)
        elif kind == "floor":
            types = np.full((256, n), -128, np.int8)
        elif kind == "ceiling":
            types = np.full((256, n), 127, np.int8)
        else:
            assert kind == "corners"
            types = np.full((256, n), -128, np.int8)
            at = rng.integers(0, n, 256)
            at[::8] = n - 1                                    # every eighth type at the LAST letter, so that letter decides
            types[np.arange(256), at] = 127
        self.types = types
        self.qoffs = np.concatenate([[QFRONT], QFRONT + np.cumsum(QLENS)]).astype(np.int64)
        self.names = rng.integers(0, 256, int(self.qoffs[-1])).astype(np.uint8)
        self.targets = [rng.integers(0, 256, t).astype(np.uint8) for t in TLENS]
        if kind != "floor":                                    # (ceiling: any listed letters -- random bytes seldom list two in a row)
            for t, (q, first, cols) in PLANTS.items():
                self.targets[t] = self._homologue(rng, q, first, cols, TLENS[t])
        edge = np.concatenate([alphabet()[:4], alphabet()[n:][-8:]])      # the four edge bytes and the last unlisted ones in a random target
        self.targets[10][20:20 + len(edge)] = edge
        self.packed, self.offs = arc.packed_of(self.targets, FRONT, rng.integers(0, 256, FRONT))
        for a in [self.types, self.qoffs, self.names, self.packed, self.offs] + self.targets:
            a.setflags(write=False)

    def _homologue(self, rng, q, first, cols, tlen):
        """The letter with the largest entry of columns [first, first + cols) of query q, with a substitution about every 40 letters
        (by an unlisted byte where there is one), three insertions and three deletions; cut or filled with random bytes to tlen."""
        names = self.query(q)[first:first + cols]
        best = self.n - 1 - np.argmax(self.types[names][:, ::-1], axis=1)       # the last of equal largest entries
        seq = (rng.choice(self.letters, len(names)) if self.kind == "ceiling" else self.letters[best]).tolist()
        unlisted = alphabet()[self.n:]
        for p in range(7, len(seq), 40):
            seq[p] = int(rng.choice(unlisted)) if len(unlisted) else int(rng.integers(0, 256))
        if cols >= 60:
            for p in sorted((cols // 8, cols // 4, 3 * cols // 8), reverse=True):   # in the first half: the second holds no gap
                del seq[p + 3]                                   # a query column without a target letter
                seq[p - 5:p - 5] = rng.integers(0, 256, 2).tolist()   # two target letters without a query column
        seq = np.array(seq, np.uint8)[:tlen]
        return np.concatenate([seq, rng.integers(0, 256, tlen - len(seq)).astype(np.uint8)])

    @property
    def matrix(self):
        """(qoffsets[nqueries], nletters) int8: row g is column g, the QFRONT unused columns included."""
        return self.types[self.names]

    def query(self, q):
        """The checker's "query" of query q: one type byte per column."""
        return self.names[self.qoffs[q]:self.qoffs[q + 1]]

    def table(self, other, smax, nletters=None):
        """The checker's (256, 256) table under (other, smax), over the first `nletters` letters (default: all of them)."""
        n = self.n if nletters is None else nletters
        tab = np.full((256, 256), other, np.int8)
        tab[:, self.letters[:n]] = np.minimum(self.types[:, :n], smax)
        return tab

    def scoring(self, sc, gaps):
        return (self.letters, sc[0], sc[1], gaps[0], gaps[1])


@functools.lru_cache(maxsize=None)
def world(kind, n):
    return World(kind, n)


_CHECKED, _ALIGNED = {}, {}


def checked(checker, case, gaps, other=None, smax=None, nletters=None):
    """The checker's (6, 11, 3) int64 table of (max_pos, max_score, 0) of one case x gaps; other / smax / nletters replace the case's
    own for the conditions that ask what a changed rule would give."""
    kind, (o, s), n = case
    key = (kind, n, o if other is None else other, s if smax is None else smax, n if nletters is None else nletters, gaps)
    if key not in _CHECKED:
        w = world(kind, n)
        tab = w.table(key[2], key[3], key[4])
        res = np.stack([checker.search(w.query(q), w.packed, w.offs, tab, *gaps) for q in range(len(QLENS))])
        res.setflags(write=False)
        _CHECKED[key] = res
    return _CHECKED[key]


def aligned(checker, case, gaps):
    """{(query, target): (sw_alignment row, ops)} over ALIGN_QUERIES x ALIGN_TARGETS: the rule's alignment over the checker's matrices."""
    if (case, gaps) not in _ALIGNED:
        from align_cases import expected
        kind, (o, s), n = case
        w = world(kind, n)
        tab = w.table(o, s)
        _ALIGNED[(case, gaps)] = {(q, t): expected(checker, w.query(q), w.targets[t], tab, *gaps)[:2] for q in ALIGN_QUERIES for t in ALIGN_TARGETS}
    return _ALIGNED[(case, gaps)]


def hit_table():
    """The (4, 4) table of target indices over ALIGN_QUERIES, every row another rotation of ALIGN_TARGETS, one entry -1."""
    return arc.hit_table()


def align_matrix(w):
    """The columns of ALIGN_QUERIES alone, back to back behind one unused column: (matrix (1 + columns, n) int8, qoffsets)."""
    rows = [w.matrix[w.qoffs[q]:w.qoffs[q + 1]] for q in ALIGN_QUERIES]
    qoffs = np.concatenate([[1], 1 + np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return np.concatenate([w.matrix[:1]] + rows), qoffs


# ---- the lane routes ("search_lanes" = 16), by the rule of include/swhip.h ----

def columns_per_lane(qlen):
    return 4 if qlen <= 256 else 8 if qlen <= 512 else 16


def packed_query(qlen, smax, longest):
    return max(smax, 0) * min(qlen, longest) <= 32767


def lane_sides(qlens, smax, gaps, longest=max(TLENS)):
    """(launches, packed launches) of one group under search_lanes = 16: a launch per class of columns per lane and kind of lanes."""
    call_ok = gaps[0] + 2 * gaps[1] >= -32768
    sides = {(columns_per_lane(n), call_ok and packed_query(n, smax, longest)) for n in qlens}
    return len(sides), sum(1 for _, p in sides if p)


CUT_QLENS = arc.CUT_QLENS                          # [300, 257, 512, 258]: one class; under smax = 127 two of them fit 16 bits


@functools.lru_cache(maxsize=None)
def cut_case(kind, n):
    """A class cut into a packed and a 32-bit side: four queries of the 8-column class over the types and targets of world(kind, n).
    (names, qoffsets with qoffsets[0] = 1)."""
    rng = np.random.default_rng(5000 + 1000 * MATRICES.index(kind) + n)
    qoffs = np.concatenate([[1], 1 + np.cumsum(CUT_QLENS)]).astype(np.int64)
    names = rng.integers(0, 256, int(qoffs[-1])).astype(np.uint8)
    w = world(kind, n)
    names[1 + 20:1 + 280] = w.query(5)[300:560]                # a slice that was planted into the 1100-letter target
    names[qoffs[3]:qoffs[4]] = np.resize(w.query(3), 258)     # the query that was planted into the 300-letter target
    names.setflags(write=False)
    qoffs.setflags(write=False)
    return names, qoffs


def cut_checked(checker, kind, n, sc, gaps):
    key = ("cut", kind, n, sc, gaps)
    if key not in _CHECKED:
        w = world(kind, n)
        names, qoffs = cut_case(kind, n)
        tab = w.table(*sc)
        _CHECKED[key] = np.stack([checker.search(names[qoffs[q]:qoffs[q + 1]], w.packed, w.offs, tab, *gaps) for q in range(len(CUT_QLENS))])
    return _CHECKED[key]
