"""Shared by test_affine_range_host.py and test_affine_range_gpu.py: the case table that places the many-query affine family -- the
many-query search, the pair-list search, the ungapped pre-filter with its packed 16-bit kernel, the per-query selection and the
alignments of a hit table, whole and checkpointed -- at the edges of its score range and its alphabet.  Plain data, no GPU: four
(256, 256) int8 tables built in numpy so that no builder clamps them, seven pairs of gap costs, one set of queries and one database
per table, and the expectations of the independent checkers (tests/affine_oracle.cpp, the numpy Kadane of tests/ungapped_cases.py,
walk() of tests/align_cases.py), each computed once per process, shared by the tests and read-only.

The near-limit alignment is out of scope here: the whole direction matrix of the (L + 1) x L pair exceeds kAlignSlotLimit, and a
checkpointed re-fill would multiply the run time of a sweep of 1.7e10 cells."""
import functools

import numpy as np

from align_cases import expected
from ungapped_cases import ungapped_table

LIMIT = 1 << 24                                   # the first score the arg-max key cannot hold; -LIMIT the last gap_open + gap_extend accepted
QLENS = [1, 63, 256, 257, 513, 1025, 2049]        # 4, 8 and 16 columns per lane, with one, two and three strips
TLENS = [0, 1, 63, 64, 65, 300, 1100, 64, 0, 127, 300]   # nine non-empty targets: the packed kernel's last rank is odd
QFRONT, FRONT = 4, 3                              # qoffsets[0], offsets[0]
TABLES = ["full8", "corners", "floor", "ceiling"]
GAPS = [(-11, -1), (0, 0), (-4, 0), (0, -3), (-LIMIT + 1, -1), (0, -LIMIT), (-LIMIT, 0)]
NO_GAP_PAYS = GAPS[4:]                            # gap_open + gap_extend = -2^24 exactly: the affine score is the ungapped score
BOTH_GAP_OPS = GAPS[:3]                           # the gap costs under which the rule's alignments carry D and I

ALIGN_QUERIES = [1, 3, 5, 6]                      # the queries of 63, 257, 1025 and 2049 letters
ALIGN_TARGETS = [4, 5, 6, 9]                      # the targets of 65, 300, 1100 and 127 letters
ALIGN_TABLES = ["full8", "corners", "ceiling"]
ALIGN_GAPS = [(-11, -1), (0, 0), (-4, 0), (-LIMIT, 0)]
assert [QLENS[q] for q in ALIGN_QUERIES] == [63, 257, 1025, 2049] and [TLENS[t] for t in ALIGN_TARGETS] == [65, 300, 1100, 127]

PACKED_QUERIES = [0, 1, 2, 3]                     # 127 x min(qlen, 1100) <= 32767: the queries of 1, 63, 256 and 257 letters
SEQ_SEED = {"full8": 101, "corners": 102, "floor": 103, "ceiling": 104}
LETTERS = {"full8": np.arange(256, dtype=np.uint8), "corners": np.array([0x00, 0xFF], np.uint8), "floor": np.arange(256, dtype=np.uint8),
           "ceiling": np.array([0x00, 0x7F, 0x80, 0xFF], np.uint8)}


@functools.lru_cache(maxsize=None)
def table(name):
    """The (256, 256) int8 table sub[query letter][target letter]."""
    if name == "full8":
        s = np.random.default_rng(1).integers(-128, 128, (256, 256)).astype(np.int8)
        assert not np.array_equal(s, s.T) and s.min() == -128 and s.max() == 127
    elif name == "corners":
        s = np.full((256, 256), -128, np.int8)
        s[0, 0] = s[255, 255] = 127
        s[255, 0] = -127
    elif name == "floor":
        s = np.full((256, 256), -128, np.int8)
    else:
        assert name == "ceiling"
        s = np.full((256, 256), 127, np.int8)
    s.setflags(write=False)
    return s


def packed_of(seqs, front, filler):
    """The sequences back to back behind `front` bytes of filler: (packed uint8, int64 offsets with offsets[0] = front)."""
    offs = np.zeros(len(seqs) + 1, np.int64)
    offs[0] = front
    offs[1:] = front + np.cumsum([len(s) for s in seqs])
    return np.concatenate([np.asarray(filler, np.uint8)[:front]] + [np.asarray(s, np.uint8) for s in seqs]).astype(np.uint8), offs


@functools.lru_cache(maxsize=None)
def sequences(name):
    """{"queries", "targets" (lists of uint8 arrays), "qpacked", "qoffs", "packed", "offs"} of one table: letters drawn from LETTERS[name]."""
    rng = np.random.default_rng(SEQ_SEED[name])
    alpha = LETTERS[name]
    queries = [rng.choice(alpha, n).astype(np.uint8) for n in QLENS]
    targets = [rng.choice(alpha, n).astype(np.uint8) for n in TLENS]
    if name == "corners":                          # slices of queries copied into targets, so that long runs exist
        targets[6][100:900] = queries[6][1000:1800]
        targets[5][10:290] = queries[4][200:480]
        targets[9][:] = queries[3][100:227]
    if name == "full8":
        for seqs in (queries, targets):
            assert {0x00, 0x7F, 0x80, 0xFF} <= set(np.concatenate(seqs).tolist())
    qpacked, qoffs = packed_of(queries, QFRONT, rng.choice(alpha, QFRONT))
    packed, offs = packed_of(targets, FRONT, rng.choice(alpha, FRONT))
    for a in queries + targets + [qpacked, qoffs, packed, offs]:
        a.setflags(write=False)
    return {"queries": queries, "targets": targets, "qpacked": qpacked, "qoffs": qoffs, "packed": packed, "offs": offs}


_CHECKED, _ALIGNED = {}, {}


def checked(checker, name, gaps):
    """The checker's (7, 11, 3) int64 table of (max_pos, max_score, 0) of one table x gaps."""
    if (name, gaps) not in _CHECKED:
        s = sequences(name)
        tab = np.stack([checker.search(q, s["packed"], s["offs"], table(name), *gaps) for q in s["queries"]])
        tab.setflags(write=False)
        _CHECKED[(name, gaps)] = tab
    return _CHECKED[(name, gaps)]


@functools.lru_cache(maxsize=None)
def ungapped(name):
    """The numpy checker's (7, 11) int64 table of the ungapped score U."""
    s = sequences(name)
    tab = ungapped_table(s["qpacked"], s["qoffs"], s["packed"], s["offs"], table(name))
    tab.setflags(write=False)
    return tab


def aligned(checker, name, gaps):
    """{(query, target): (sw_alignment row, ops)} over ALIGN_QUERIES x ALIGN_TARGETS: the rule's alignment over the checker's matrices."""
    if (name, gaps) not in _ALIGNED:
        s = sequences(name)
        _ALIGNED[(name, gaps)] = {(q, t): expected(checker, s["queries"][q], s["targets"][t], table(name), *gaps)[:2] for q in ALIGN_QUERIES for t in ALIGN_TARGETS}
    return _ALIGNED[(name, gaps)]


def hit_table():
    """The (4, 4) table of target indices over ALIGN_QUERIES, every row another rotation of ALIGN_TARGETS, one entry -1."""
    hits = np.array([np.roll(ALIGN_TARGETS, r) for r in range(4)], np.int64)
    hits[2, 1] = -1
    return hits


def pair_list():
    """The 77 pairs shuffled, ten of them a second time, and a tail of five {-1, -1}: (92, 2) int64."""
    rng = np.random.default_rng(77)
    cross = np.array([(q, t) for q in range(len(QLENS)) for t in range(len(TLENS))], np.int64)
    cross = cross[rng.permutation(len(cross))]
    return np.concatenate([cross, cross[rng.choice(len(cross), 10, replace=False)], np.full((5, 2), -1, np.int64)])


def halves_case(qlen):
    """The pre-filter's halves case under `corners`: a query of qlen x 0x00 against [0xFF x 301, 0x00 x 300, 0x00 x 299, 0xFF x 298].  The
    length-sorted schedule pairs (301, 300) and (299, 298): in the first wave the low half takes -128 at every cell while the high
    half climbs to 127 x qlen, in the second the roles are swapped.  (qpacked, qoffs, packed, offs, U (1, 4))."""
    tlens, letters = [301, 300, 299, 298], [0xFF, 0x00, 0x00, 0xFF]
    qpacked, qoffs = packed_of([np.zeros(qlen, np.uint8)], 1, [0xFF])
    packed, offs = packed_of([np.full(n, x, np.uint8) for n, x in zip(tlens, letters)], FRONT, [0x00] * FRONT)
    want = np.array([[0 if x else 127 * min(qlen, n) for n, x in zip(tlens, letters)]], np.int64)
    return qpacked, qoffs, packed, offs, want


CUT_QLENS = [300, 257, 512, 258]                  # one class (8 columns per lane: 257 .. 512 letters); 127 x qlen <= 32767 up to 258


@functools.lru_cache(maxsize=None)
def cut_case(name):
    """A class cut into a packed and a 32-bit side.  Of QLENS, 513 has 16 columns per lane (one strip of 1024), so no class there holds
    both kinds; these four queries share the 8-column class, and against the targets of sequences(name) under a largest entry of 127
    the planner's stable partition puts 257 and 258 on the packed side and 300 and 512 on 32-bit lanes.  (qpacked, qoffs, U (4, 11))."""
    rng = np.random.default_rng(SEQ_SEED[name] + 1000)
    s = sequences(name)
    queries = [rng.choice(LETTERS[name], n).astype(np.uint8) for n in CUT_QLENS]
    if name == "corners":
        queries[0][20:280] = s["targets"][6][300:560]
        queries[3][:] = s["targets"][5][20:278]
    qpacked, qoffs = packed_of(queries, 1, rng.choice(LETTERS[name], 1))
    want = ungapped_table(qpacked, qoffs, s["packed"], s["offs"], table(name))
    for a in (qpacked, qoffs, want):
        a.setflags(write=False)
    return qpacked, qoffs, want


NEAR_L = 132104                                 # 127 L < 2^24 <= 127 (L + 1)
NEAR_GAPS = (-20, -3)
assert 127 * NEAR_L < LIMIT <= 127 * (NEAR_L + 1)


def near_table():
    """submat_match(127, -128), built here."""
    s = np.full((256, 256), -128, np.int8)
    s[np.arange(256), np.arange(256)] = 127
    return s


def near_limit_case(longest=NEAR_L):
    """Queries [A x (L + 1), A x 7] against [A x longest, A x 100, C x 50]; with all letters equal H[i][j] = 127 min(i, j), whose maximum
    lies first (lowest index) at (m, m), m = min(qlen, len): (qpacked, qoffs, packed, offs, expected (2, 3, 3), U (2, 3)).  No checker
    runs the 1.7e10-cell pair; the expectation is closed-form."""
    a, c = ord("A"), ord("C")
    qlens, tlens = [NEAR_L + 1, 7], [longest, 100, 50]
    qpacked, qoffs = packed_of([np.full(n, a, np.uint8) for n in qlens], QFRONT, [c] * QFRONT)
    packed, offs = packed_of([np.full(longest, a, np.uint8), np.full(100, a, np.uint8), np.full(50, c, np.uint8)], FRONT, [c] * FRONT)
    want = np.zeros((2, 3, 3), np.int64)
    for q, qlen in enumerate(qlens):
        for t in (0, 1):
            m = min(qlen, tlens[t])
            want[q, t] = (m * (qlen + 1) + m, 127 * m, 0)
    return qpacked, qoffs, packed, offs, want, want[:, :, 1].copy()


NEAR_SMALL_PAIRS = [(1, 0), (1, 1), (1, 2), (0, 1), (0, 2)]      # every near-limit pair but the (L + 1) x L one
