"""CPU: the case table of tests/pssm_range_cases.py.  First the conditions the table is built for, asserted on the independent
checker's output alone (tests/affine_oracle.cpp, walk() and replay() of tests/align_cases.py); then the host legs of the PSSM calls
(sw_search_pssm_multi_host, sw_align_pssm_hits_host) against the checker on every case x gaps, exactly.

The conditions, by number:
  1  under every smax < 127 the table changes when smax is taken as 127, and some entry read by a rule alignment exceeds smax;
  2  below 256 letters the table changes when `other` is raised by 1 (lowered by 1 at other = 127, the last value a table holds).
     Where no cell can score above 0 -- smax = 0 with other < 0, and `floor` with other <= 0 -- no rule could change a table that
     condition 4 shows to be zero; those cases are named and left to condition 4;
  3  under full8 and corners with (-128, 127) some score exceeds 32767 (from two letters on: one letter holds no planted signal), some
     query of at most 258 columns scores above 1000, some rule alignment carries both I and D under arc.BOTH_GAP_OPS;
  4  under smax = 0 (other <= 0) and under `floor` (other <= 0) every score and every max_pos is 0;
  5  at 253 letters the table differs from the one of the first 252 letters alone;
  6  (both lane routes occur: asserted in tests/test_pssm_range_gpu.py from the options; the rule itself is stated here)."""
import numpy as np
import pytest

import affine_range_cases as arc
import pssm_range_cases as prc
from affine_cases import checker  # noqa: F401
from align_cases import replay

LOW = prc.GAPS[0]                                  # (-11, -1)
NO_GAP = arc.NO_GAP_PAYS[0]                        # a substituted letter cannot be gapped around


def all_zero_by_rule(case):
    kind, (other, smax), n = case
    return other <= 0 and (smax == 0 or kind == "floor") or (kind == "floor" and n == 256)


# ---- the conditions of the table, on the checker's output ----

def test_the_table_holds_what_it_says():
    assert len(prc.alphabet()) == 256 and prc.alphabet()[:4].tolist() == [0x00, 0x7F, 0x80, 0xFF]
    assert np.array_equal(prc.letters_of(253)[:252], prc.letters_of(252))
    for n in prc.NLETTERS:
        w = prc.world("full8", n)
        assert w.matrix.shape == (prc.QFRONT + sum(prc.QLENS), n) and w.qoffs[0] == prc.QFRONT and w.offs[0] == prc.FRONT
        assert list(np.diff(w.qoffs)) == prc.QLENS and list(np.diff(w.offs)) == prc.TLENS
        assert w.types.min() == -128 and w.types.max() == 127
        if n >= 2:
            assert ((w.types == -128).any(axis=1) & (w.types == 127).any(axis=1)).all()
        seen = set(w.packed[prc.FRONT:].tolist())
        assert {0x00, 0x7F, 0x80, 0xFF} <= seen
        assert (set(prc.alphabet()[n:].tolist()) <= seen) if n >= 252 else len(seen - set(w.letters.tolist())) > 100
    assert int(prc.alphabet()[255]) in set(prc.world("full8", 255).packed.tolist())          # at 255 letters the one missing byte occurs
    for n in prc.MAIN_NLETTERS:
        assert (prc.world("floor", n).types == -128).all() and (prc.world("ceiling", n).types == 127).all()
        c = prc.world("corners", n).types
        assert ((c == 127).sum(axis=1) == 1).all() and ((c == -128).sum(axis=1) == n - 1).all()


@pytest.mark.parametrize("case", [c for c in prc.CASES if c[1][1] < 127 and c[0] != "floor"], ids=prc.case_id)
def test_1_the_clamp_decides(checker, case):  # noqa: F811
    assert any(not np.array_equal(prc.checked(checker, case, g), prc.checked(checker, case, g, smax=127)) for g in (LOW, NO_GAP))


def test_1_a_rule_alignment_reads_an_entry_above_smax(checker):  # noqa: F811
    case = ("full8", prc.CLAMPING, 4)
    w = prc.world("full8", 4)
    place = {int(x): k for k, x in enumerate(w.letters)}
    above = 0
    for (q, t), (row, ops) in prc.aligned(checker, case, LOW).items():
        i, j = row[3], row[2]
        for op in ops:
            if op == ord("M"):
                x = int(w.targets[t][i])
                above += x in place and int(w.types[w.query(q)[j], place[x]]) > case[1][1]
            i, j = i + (op != ord("I")), j + (op != ord("D"))
    assert above > 100, above


@pytest.mark.parametrize("case", [c for c in prc.CASES if c[2] < 256], ids=prc.case_id)
def test_2_other_decides(checker, case):  # noqa: F811
    other = case[1][0]
    moved = other + 1 if other < 127 else other - 1
    changed = any(not np.array_equal(prc.checked(checker, case, g), prc.checked(checker, case, g, other=moved)) for g in (NO_GAP, LOW))
    if all_zero_by_rule(case) and moved <= 0:
        assert not changed and not prc.checked(checker, case, NO_GAP).any()               # nothing scores: condition 4 covers these
    else:
        assert changed


@pytest.mark.parametrize("case", [c for c in prc.CASES if c[0] in ("full8", "corners") and c[1] == (-128, 127) and c[2] >= 2], ids=prc.case_id)
def test_3_scores_leave_16_bits(checker, case):  # noqa: F811
    for gaps in prc.GAPS:
        score = prc.checked(checker, case, gaps)[:, :, 1]
        assert score.max() > 32767, (gaps, int(score.max()))
        assert score[:4].max() > 1000 and max(prc.QLENS[:4]) <= 258, (gaps, int(score[:4].max()))


@pytest.mark.parametrize("gaps", arc.BOTH_GAP_OPS)
@pytest.mark.parametrize("case", [c for c in prc.ALIGN_CASES if c[0] != "ceiling" and c[1] == (-128, 127)], ids=prc.case_id)
def test_3_the_alignments_carry_both_gap_operations(checker, case, gaps):  # noqa: F811
    ops = b"".join(o for _, o in prc.aligned(checker, case, gaps).values())
    assert ops.count(b"D") > 10 and ops.count(b"I") > 10, (ops.count(b"D"), ops.count(b"I"))


@pytest.mark.parametrize("case", [c for c in prc.CASES if all_zero_by_rule(c)], ids=prc.case_id)
def test_4_nothing_scores(checker, case):  # noqa: F811
    assert case[1][1] == 0 or case[0] == "floor"
    for gaps in prc.GAPS:
        assert not prc.checked(checker, case, gaps).any(), gaps


def test_4_names_every_case_it_should():
    zero = [c for c in prc.CASES if all_zero_by_rule(c)]
    assert {c for c in prc.CASES if c[1][1] == 0 and c[1][0] <= 0} <= set(zero)
    assert {c for c in prc.CASES if c[0] == "floor" and c[1][0] <= 0} <= set(zero)
    assert all(c[0] == "floor" and c[2] == 256 for c in zero if c[1][0] > 0)               # 256 letters: no byte scores `other`


@pytest.mark.parametrize("case", [c for c in prc.CASES if c[2] == 253 and not all_zero_by_rule(c)], ids=prc.case_id)
def test_5_the_253rd_letter_decides(checker, case):  # noqa: F811
    if case[0] == "ceiling" and case[1] == (127, 127):                                     # every byte scores 127, listed or not
        assert np.array_equal(prc.world("ceiling", 253).table(127, 127), prc.world("ceiling", 253).table(127, 127, 252))
        return
    assert any(not np.array_equal(prc.checked(checker, case, g), prc.checked(checker, case, g, nletters=252)) for g in (NO_GAP, LOW))


def test_6_the_rule_puts_queries_on_both_kinds_of_lanes():
    assert [prc.packed_query(n, 127, 1100) for n in prc.QLENS] == [True, True, True, True, False, False]
    assert prc.lane_sides(prc.QLENS, 127, LOW) == (3, 2) and prc.lane_sides(prc.QLENS, 1, LOW) == (3, 3) == prc.lane_sides(prc.QLENS, 0, LOW)
    assert prc.lane_sides(prc.CUT_QLENS, 127, LOW) == (2, 1)
    assert [prc.lane_sides(prc.QLENS, 1, g)[1] for g in prc.GAPS] == [3, 3, 3, 3, 0, 0, 0]


@pytest.mark.parametrize("gaps", prc.ALIGN_GAPS)
@pytest.mark.parametrize("case", prc.ALIGN_CASES, ids=prc.case_id)
def test_the_expected_alignments_replay_to_their_scores(checker, case, gaps):  # noqa: F811
    w, tab = prc.world(case[0], case[2]), prc.checked(checker, case, gaps)
    table = w.table(*case[1])
    for (q, t), (row, ops) in prc.aligned(checker, case, gaps).items():
        assert row[:2] == tuple(tab[q, t, :2]) and row[1] > 0
        replay(w.query(q), w.targets[t], table, *gaps, row, ops)
        if gaps == (-arc.LIMIT, 0):
            assert set(ops) == {ord("M")}


# ---- the host legs against the checker ----

@pytest.mark.parametrize("case", prc.CASES, ids=prc.case_id)
def test_search_leg_equals_the_checker(swamd, checker, case):  # noqa: F811
    w = prc.world(case[0], case[2])
    for gaps in prc.GAPS:
        want = prc.checked(checker, case, gaps)
        got = swamd.search_pssm_multi_host((w.matrix, w.qoffs), (w.packed, w.offs), w.scoring(case[1], gaps))
        assert got.shape == (6, 11, 3) and np.array_equal(got, want), (gaps, np.argwhere((got != want).any(axis=2))[:5].tolist())


@pytest.mark.parametrize("case", [(k, sc, n) for k, sc, n in prc.CASES if k == "full8" and sc == (-128, 127)], ids=prc.case_id)
def test_search_leg_on_the_cut_class(swamd, checker, case):  # noqa: F811
    kind, sc, n = case
    w = prc.world(kind, n)
    names, qoffs = prc.cut_case(kind, n)
    got = swamd.search_pssm_multi_host((w.types[names], qoffs), (w.packed, w.offs), w.scoring(sc, LOW))
    assert np.array_equal(got, prc.cut_checked(checker, kind, n, sc, LOW))


@pytest.mark.parametrize("gaps", prc.ALIGN_GAPS)
@pytest.mark.parametrize("case", prc.ALIGN_CASES, ids=prc.case_id)
def test_hit_table_leg_equals_the_rule_over_the_checkers_matrices(swamd, checker, case, gaps):  # noqa: F811
    w, want = prc.world(case[0], case[2]), prc.aligned(checker, case, gaps)
    hits = prc.hit_table()
    m, qoffs = prc.align_matrix(w)
    aln, ops = swamd.align_pssm_hits_host((m, qoffs), (w.packed, w.offs), w.scoring(case[1], gaps), hits)
    for a, q in enumerate(prc.ALIGN_QUERIES):
        for r in range(4):
            if hits[a, r] < 0:
                assert not aln[a, r].any() and ops[a][r] == b""
            else:
                row, eops = want[(q, int(hits[a, r]))]
                assert tuple(int(x) for x in aln[a, r]) == row and ops[a][r] == eops, (q, r)
