"""Shared by test_search_multi_lanes_gpu.py and test_search_multi_lanes_cli_gpu.py: the cases that put the many-query search on packed
16-bit lanes ("search_lanes" = 16) beside its 32-bit form.  Plain data, no GPU, computed once per process and read-only.

The tables of tests/affine_range_cases.py hold 127, under which only one-strip queries fit 16 bits (127 x qlen <= 32767 up to 258).
TABLE24 is there for the strips: a 24-letter table with entries in -8 .. 11, asymmetric, so that every length of QLENS is eligible
against targets of up to 1100 letters (11 x 1100 = 12100) and the packed boundary column between strips is crossed at 16 columns
per lane."""
import functools

import numpy as np

import affine_range_cases as arc
from affine_cases import PROTEIN
from ungapped_cases import ungapped_table

QLENS = [1, 63, 256, 257, 513, 1025, 2049]        # 4, 8 and 16 columns per lane, with one, two and three strips
TLENS = arc.TLENS                                 # nine non-empty targets (an odd last rank), empties in between
QFRONT, FRONT = 4, 3                              # qoffsets[0], offsets[0]
GAPS = [(-11, -1), (0, 0), (-4, 0), (0, -3)]
OTHER = -8                                        # every pair with a byte outside the 24 letters
assert QLENS == arc.QLENS and (QFRONT, FRONT) == (arc.QFRONT, arc.FRONT) and len(PROTEIN) == 24

# the lower edge of the rule gap_open + 2 gap_extend >= -32768, from both sides; no alignment under TABLE24 can pay any of these gaps
# (12100 < 16384), so the affine score is the ungapped score
PACKED_GAPS = [(-32766, -1), (0, -16384)]
FALLBACK_GAPS = [(-32767, -1)] + list(arc.NO_GAP_PAYS)


@functools.lru_cache(maxsize=None)
def table24():
    """The (256, 256) int8 table: random entries in -8 .. 11 over the 24 letters, OTHER elsewhere."""
    rng = np.random.default_rng(24)
    s = np.full((256, 256), OTHER, np.int8)
    s[np.ix_(PROTEIN, PROTEIN)] = rng.integers(-8, 12, (24, 24)).astype(np.int8)
    assert s.max() == 11 and s.min() == -8 and not np.array_equal(s, s.T)
    assert all(11 * min(q, max(TLENS)) <= 32767 for q in QLENS)
    s.setflags(write=False)
    return s


def case_of(queries, targets, qfront=QFRONT, front=FRONT, filler=PROTEIN):
    """{"queries", "targets", "qpacked", "qoffs", "packed", "offs"}: the sequences back to back behind qfront / front bytes of filler."""
    queries, targets = [np.asarray(q, np.uint8) for q in queries], [np.asarray(t, np.uint8) for t in targets]
    qpacked, qoffs = arc.packed_of(queries, qfront, np.resize(filler, qfront))
    packed, offs = arc.packed_of(targets, front, np.resize(filler, front))
    for a in queries + targets + [qpacked, qoffs, packed, offs]:
        a.setflags(write=False)
    return {"queries": queries, "targets": targets, "qpacked": qpacked, "qoffs": qoffs, "packed": packed, "offs": offs}


@functools.lru_cache(maxsize=None)
def strips_case():
    """QLENS against TLENS in the 24 letters."""
    rng = np.random.default_rng(2401)
    return case_of([rng.choice(PROTEIN, n) for n in QLENS], [rng.choice(PROTEIN, n) for n in TLENS])


@functools.lru_cache(maxsize=None)
def strips_ungapped():
    """The numpy checker's (7, 11) table of the ungapped score U of strips_case() under TABLE24."""
    c = strips_case()
    u = ungapped_table(c["qpacked"], c["qoffs"], c["packed"], c["offs"], table24())
    u.setflags(write=False)
    return u


def partner_cases():
    """[(name, case)] under TABLE24, queries of 63, 300 and 1025 letters: databases in which a target's partner is missing, tiny, one
    letter shorter or longer, or itself."""
    rng = np.random.default_rng(2402)
    queries = [rng.choice(PROTEIN, n) for n in (63, 300, 1025)]
    x, y = rng.choice(PROTEIN, 301), rng.choice(PROTEIN, 301)
    long = rng.choice(PROTEIN, 1100)
    twin = rng.choice(PROTEIN, 200)
    none = np.zeros(0, np.uint8)
    return [("one_target", case_of(queries, [none, x[:300], none])),
            ("one_target_alone", case_of(queries, [long])),
            ("lengths_1_and_1100", case_of(queries, [x[:1], long])),
            ("lengths_1100_and_1", case_of(queries, [long, x[:1]])),
            ("x300_y301", case_of(queries, [x[:300], y])),          # y in the low halves, x's prefix in the high halves
            ("x301_y300", case_of(queries, [x, y[:300]])),          # and the other way round
            ("twins", case_of(queries, [twin, twin.copy()]))]


def corners_cases():
    """[(name, case)] under arc.table("corners") (0x00 / 0xFF score 127 with themselves, everything else -128 or -127): a query of 258
    letters, one target that mismatches everywhere beside one that holds a copied slice of the query -- one half sits at goe and at
    negative sums while the other climbs to 127 x 200 -- with the climbing target once as the shorter and once as the longer one."""
    rng = np.random.default_rng(2403)
    q = rng.choice(np.array([0x00, 0xFF], np.uint8), 258)
    climb = q[20:220].copy()
    return [("mismatch_low_climb_high", case_of([q], [np.full(201, 0x01, np.uint8), climb], filler=[0x01])),
            ("climb_low_mismatch_high", case_of([q], [climb, np.full(199, 0x01, np.uint8)], filler=[0x01]))]


@functools.lru_cache(maxsize=None)
def ties_case():
    """Two letters, queries of 257 and 1025, targets of 64, 65, 127 and 300: under match / mismatch 1 / -1 equal maxima occur across
    lanes and across strips, in either half."""
    rng = np.random.default_rng(2404)
    ab = np.frombuffer(b"AB", np.uint8)
    return case_of([rng.choice(ab, n) for n in (257, 1025)], [rng.choice(ab, n) for n in (64, 65, 127, 300)], filler=ab)


@functools.lru_cache(maxsize=None)
def upper_edge_case():
    """Under a table of 31 everywhere: queries of 1057 and 1058 letters against targets of 1100 and 1057.  31 x 1057 = 32767: the first
    query is eligible and reaches the last score a half can hold; 31 x 1058 is one step over."""
    rng = np.random.default_rng(2405)
    assert 31 * 1057 == 32767
    return case_of([rng.choice(PROTEIN, n) for n in (1057, 1058)], [rng.choice(PROTEIN, n) for n in (1100, 1057)])


@functools.lru_cache(maxsize=None)
def ceiling_edge_case():
    """Under arc.table("ceiling") (127 everywhere): queries of 258 and 259 letters, one class; 127 x 258 = 32766 fits, 127 x 259 does not."""
    rng = np.random.default_rng(2406)
    return case_of([rng.choice(arc.LETTERS["ceiling"], n) for n in (258, 259)], [rng.choice(arc.LETTERS["ceiling"], n) for n in (300, 258, 64)])


@functools.lru_cache(maxsize=None)
def many_targets_case():
    """QLENS against 9000 targets of 0 .. 15 letters: a result row of 9000 x 24 bytes, so that a budget of 1 MiB ("search_results_mib")
    cuts the seven queries into chunks."""
    rng = np.random.default_rng(2407)
    return case_of([rng.choice(PROTEIN, n) for n in QLENS], [rng.choice(PROTEIN, int(n)) for n in rng.integers(0, 16, 9000)])
