"""CPU: the case table of tests/affine_range_cases.py.  First the conditions the table is built for, asserted on the independent
checkers' output alone (tests/affine_oracle.cpp, the numpy Kadane of tests/ungapped_cases.py, walk() and replay() of
tests/align_cases.py, swp::plan_prefilter through tests/prefilter_plan_driver.cpp); then every host leg of the many-query affine
family against those checkers on every table x gaps, exactly; then one step over every limit, refused without a write."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import affine_range_cases as arc
from affine_cases import ROOT, checker  # noqa: F401
from align_cases import replay
from top_cases import numpy_top
from ungapped_cases import passing, ungapped_table

EINVAL = -22
POISON64 = -0x5A5A5A5A5A5A5A5B
POISON32 = -0x5A5A5A5B
NONEMPTY = np.array(arc.TLENS) > 0
CASES = [(name, gaps) for name in arc.TABLES for gaps in arc.GAPS]


def case_id(c):
    return f"{c[0]}{c[1][0]}_{c[1][1]}"


# ---- the conditions of the table, on the checkers' output ----

@pytest.mark.parametrize("name", ["full8", "corners"])
def test_gaps_change_the_score_of_most_pairs(checker, name):  # noqa: F811
    differ = (arc.checked(checker, name, (-11, -1))[:, :, 1] != arc.ungapped(name))[:, NONEMPTY]
    assert differ.size == 63 and differ.sum() > 63 // 2, int(differ.sum())


@pytest.mark.parametrize("gaps", arc.NO_GAP_PAYS)
@pytest.mark.parametrize("name", ["full8", "corners"])
def test_no_gap_pays_at_minus_two_to_the_24(checker, name, gaps):  # noqa: F811
    assert gaps[0] + gaps[1] == -arc.LIMIT
    score = arc.checked(checker, name, gaps)[:, :, 1]
    assert score.shape == (7, 11) and np.array_equal(score, arc.ungapped(name)) and score.max() > 0


@pytest.mark.parametrize("gaps", arc.BOTH_GAP_OPS)
@pytest.mark.parametrize("name", ["full8", "corners"])
def test_the_alignments_carry_both_gap_operations(checker, name, gaps):  # noqa: F811
    ops = b"".join(o for _, o in arc.aligned(checker, name, gaps).values())
    assert ops.count(b"D") > 100 and ops.count(b"I") > 100, (ops.count(b"D"), ops.count(b"I"))      # hundreds of each over the 16 hits


@pytest.mark.parametrize("gaps", arc.ALIGN_GAPS)
@pytest.mark.parametrize("name", arc.ALIGN_TABLES)
def test_the_expected_alignments_replay_to_their_scores(checker, name, gaps):  # noqa: F811
    s, tab = arc.sequences(name), arc.checked(checker, name, gaps)
    for (q, t), (row, ops) in arc.aligned(checker, name, gaps).items():
        assert row[:2] == tuple(tab[q, t, :2]) and row[1] > 0
        replay(s["queries"][q], s["targets"][t], arc.table(name), *gaps, row, ops)
        if gaps == (-arc.LIMIT, 0):
            assert set(ops) == {ord("M")}


@pytest.mark.parametrize("gaps", arc.GAPS)
def test_floor_is_all_zero_and_ceiling_is_closed_form(checker, gaps):  # noqa: F811
    assert not arc.checked(checker, "floor", gaps).any() and not arc.ungapped("floor").any()
    tab = arc.checked(checker, "ceiling", gaps)
    for q, qlen in enumerate(arc.QLENS):
        for t, n in enumerate(arc.TLENS):
            m = min(qlen, n)
            assert tuple(tab[q, t]) == (m * (qlen + 1) + m, 127 * m, 0), (q, t)
    assert np.array_equal(arc.ungapped("ceiling"), tab[:, :, 1])


def test_sequences_reach_the_ends_of_the_alphabet():
    assert not np.array_equal(arc.table("full8"), arc.table("full8").T)
    s = arc.sequences("full8")
    for seqs in (s["queries"], s["targets"]):
        assert {0x00, 0x7F, 0x80, 0xFF} <= set(np.concatenate(seqs).tolist())
    assert set(arc.sequences("corners")["qpacked"].tolist()) == {0x00, 0xFF}
    assert set(arc.sequences("ceiling")["packed"].tolist()) == {0x00, 0x7F, 0x80, 0xFF}
    for name in arc.TABLES:
        s = arc.sequences(name)
        assert s["qoffs"][0] == arc.QFRONT and s["offs"][0] == arc.FRONT and list(np.diff(s["qoffs"])) == arc.QLENS and list(np.diff(s["offs"])) == arc.TLENS


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the planner")
    exe = str(tmp_path_factory.mktemp("plan") / "prefilter_plan")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "prefilter_plan_driver.cpp"),
                    os.path.join(ROOT, "smith-waterman_amd", "csrc", "sw_plan.cpp")], check=True)

    def run(qlens, **kw):
        line = "qlens=" + ",".join(str(q) for q in qlens) + " " + " ".join(f"{k}={v}" for k, v in kw.items())
        return json.loads(subprocess.run([exe], input=line + "\n", capture_output=True, text=True, check=True).stdout)
    return run


def test_the_planner_packs_what_fits_16_bits_and_cuts_a_class_that_holds_both_kinds(plan):
    assert [q for q, n in enumerate(arc.QLENS) if 127 * min(n, 1100) <= 32767] == arc.PACKED_QUERIES
    p = plan(arc.QLENS, longest=1100, nonempty=9, max_entry=127)
    kind = {}
    for l in p["launches"]:
        for e in range(l["q0"], l["q0"] + l["nq"]):
            assert kind.setdefault(p["table"][e][2], l["packed"]) == l["packed"]
    assert kind == {q: int(q in arc.PACKED_QUERIES) for q in range(7)}
    assert 0 < p["packed_launches"] < len(p["launches"])
    sides = lambda p, C: sorted((l["packed"], sorted(p["table"][e][3] for e in range(l["q0"], l["q0"] + l["nq"]))) for l in p["launches"] if l["C"] == C)  # noqa: E731
    # 513 letters take 16 columns per lane (one strip of 1024): of QLENS the 8-column class holds 257 alone, and no class has both kinds
    assert sides(p, 8) == [(1, [257])] and sides(p, 16) == [(0, [513, 1025, 2049])] and sides(p, 4) == [(1, [1, 63, 256])]
    # ... so the cut inside one class is CUT_QLENS': one class, both kinds, a launch side each
    p = plan(arc.CUT_QLENS, longest=1100, nonempty=9, max_entry=127)
    assert sides(p, 8) == [(0, [300, 512]), (1, [257, 258])] and len(p["launches"]) == 2 and p["packed_launches"] == 1
    # a table with no positive entry: max(largest, 0) = 0, every query is packed
    p = plan(arc.QLENS, longest=1100, nonempty=9, max_entry=-128)
    assert p["packed_launches"] == len(p["launches"]) > 0
    # the halves case: 127 x 258 = 32766 packed, 127 x 259 = 32893 not
    assert plan([258], longest=301, nonempty=4, max_entry=127)["packed_launches"] == 1
    assert plan([259], longest=301, nonempty=4, max_entry=127)["packed_launches"] == 0


# ---- the host legs against the checkers ----

@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_search_legs_equal_the_checker(swamd, checker, case):  # noqa: F811
    name, gaps = case
    s, want = arc.sequences(name), arc.checked(checker, name, gaps)
    scoring = (arc.table(name), *gaps)
    got = swamd.search_affine_multi_host((s["qpacked"], s["qoffs"]), (s["packed"], s["offs"]), scoring)
    assert got.shape == (7, 11, 3) and np.array_equal(got, want), np.argwhere((got != want).any(axis=2))[:5]
    pairs = arc.pair_list()
    inside = pairs[:, 0] >= 0
    got = swamd.search_affine_pairs_host((s["qpacked"], s["qoffs"]), (s["packed"], s["offs"]), scoring, pairs)
    assert inside.sum() == 87 and np.array_equal(got[inside], want[pairs[inside, 0], pairs[inside, 1]]) and not got[~inside].any()
    for top in (1, 4, 12):
        hits, nhits = swamd.search_affine_multi_top_host((s["qpacked"], s["qoffs"]), (s["packed"], s["offs"]), scoring, top, 1)
        want_hits, want_nhits = numpy_top(want, top, 1)
        assert np.array_equal(hits, want_hits) and np.array_equal(nhits, want_nhits), top


@pytest.mark.parametrize("name", arc.TABLES)
def test_prefilter_leg_equals_the_numpy_checker(swamd, name):
    s, want = arc.sequences(name), arc.ungapped(name)
    pos = np.sort(want[want > 0])
    m = int(pos[len(pos) // 2]) if len(pos) else 1
    pairs, n, scores = swamd.prefilter_ungapped_host((s["qpacked"], s["qoffs"]), (s["packed"], s["offs"]), arc.table(name), m)
    exp = passing(want, s["offs"], m)
    assert np.array_equal(scores, want) and n == len(exp) and np.array_equal(pairs[:n], exp) and (pairs[n:] == -1).all()
    assert (name == "floor") == (n == 0)


@pytest.mark.parametrize("name", ["full8", "corners", "ceiling"])
def test_prefilter_leg_on_the_cut_class(swamd, name):
    qpacked, qoffs, want = arc.cut_case(name)
    s = arc.sequences(name)
    _, n, scores = swamd.prefilter_ungapped_host((qpacked, qoffs), (s["packed"], s["offs"]), arc.table(name), 1)
    assert np.array_equal(scores, want) and n == (want > 0).sum() > 0
    if name == "ceiling":                                                               # the scores themselves lie on both sides of 16 bits
        assert want[[1, 3]].max() == 127 * 258 == 32766 and want[[0, 2]].max() == 127 * 512


@pytest.mark.parametrize("qlen", [258, 259])
def test_prefilter_leg_on_the_halves_case(swamd, qlen):
    qpacked, qoffs, packed, offs, want = arc.halves_case(qlen)
    sub = arc.table("corners")
    assert np.array_equal(ungapped_table(qpacked, qoffs, packed, offs, sub), want)
    assert want.tolist() == [[0, 127 * qlen, 127 * qlen, 0]] and (want.max() <= 32767) == (qlen == 258)
    _, n, scores = swamd.prefilter_ungapped_host((qpacked, qoffs), (packed, offs), sub, 1)
    assert np.array_equal(scores, want) and n == 2


@pytest.mark.parametrize("gaps", arc.ALIGN_GAPS)
@pytest.mark.parametrize("name", arc.ALIGN_TABLES)
def test_hit_table_leg_equals_the_rule_over_the_checkers_matrices(swamd, checker, name, gaps):  # noqa: F811
    s, want = arc.sequences(name), arc.aligned(checker, name, gaps)
    hits = arc.hit_table()
    queries = [s["queries"][q] for q in arc.ALIGN_QUERIES]
    aln, ops = swamd.align_affine_hits_host(queries, (s["packed"], s["offs"]), (arc.table(name), *gaps), hits)
    for a, q in enumerate(arc.ALIGN_QUERIES):
        for r in range(4):
            if hits[a, r] < 0:
                assert not aln[a, r].any() and ops[a][r] == b""
            else:
                row, eops = want[(q, int(hits[a, r]))]
                assert tuple(int(x) for x in aln[a, r]) == row and ops[a][r] == eops, (q, r)


def test_near_limit_small_pairs(swamd):
    qpacked, qoffs, packed, offs, want, _ = arc.near_limit_case()
    assert want[0, 0, 0] > 1 << 32 and want[0, 0, 1] == 127 * arc.NEAR_L == arc.LIMIT - 8
    assert np.array_equal(arc.near_table(), swamd.submat_match(127, -128))
    scoring = (arc.near_table(), *arc.NEAR_GAPS)
    small = np.array(arc.NEAR_SMALL_PAIRS, np.int64)
    got = swamd.search_affine_pairs_host((qpacked, qoffs), (packed, offs), scoring, small)
    assert np.array_equal(got, want[small[:, 0], small[:, 1]])
    short = (qpacked[qoffs[1]:qoffs[2]], np.array([0, 7], np.int64))
    assert np.array_equal(swamd.search_affine_multi_host(short, (packed, offs), scoring), want[1:])
    _, n, scores = swamd.prefilter_ungapped_host(short, (packed, offs), scoring[0], 1)
    assert n == 2 and scores.tolist() == [[889, 889, 0]]


# ---- one step over every limit ----

def host_calls(swamd, qpacked, qoffs, packed, offs, sub, go, ge):
    """Every host entry point of the family on poisoned outputs: [(name, return code, outputs untouched)]."""
    L = swamd.lib()
    nq, nt, top = len(qoffs) - 1, len(offs) - 1, 2
    sub = np.ascontiguousarray(sub, np.int8)
    sc = swamd._Affine(sub.ctypes.data, go, ge)
    qo, o = np.ascontiguousarray(qoffs, np.int64), np.ascontiguousarray(offs, np.int64)
    pairs = np.array([(0, 1), (nq - 1, 0)], np.int64)
    hits = np.zeros((nq, top, 3), np.int64)
    args = (qpacked.ctypes.data, qo.ctypes.data, nq, packed.ctypes.data, o.ctypes.data, nt)
    out = []

    def outputs(*shapes):
        return [np.full(shape, POISON64 if dt == np.int64 else POISON32 if dt == np.int32 else 0x5A, dt) for shape, dt in shapes]

    def done(name, rc, bufs):
        out.append((name, rc, all((b == (POISON64 if b.dtype == np.int64 else POISON32 if b.dtype == np.int32 else 0x5A)).all() for b in bufs)))

    res, = bufs = outputs(((nq * nt, 3), np.int64))
    done("multi", L.sw_search_affine_multi_host(*args, ctypes.byref(sc), res.ctypes.data), bufs)
    res, = bufs = outputs(((len(pairs), 3), np.int64))
    done("pairs", L.sw_search_affine_pairs_host(*args, ctypes.byref(sc), pairs.ctypes.data, len(pairs), res.ctypes.data), bufs)
    h, n = bufs = outputs(((nq * top, 3), np.int64), ((nq,), np.int64))
    done("top", L.sw_search_affine_multi_top_host(*args, ctypes.byref(sc), top, 1, h.ctypes.data, n.ctypes.data), bufs)
    aln, ops = bufs = outputs(((nq * top, 7), np.int64), ((nq * top, 16), np.uint8))
    done("hits", L.sw_align_affine_hits_host(*args, ctypes.byref(sc), hits.ctypes.data, None, top, aln.ctypes.data, ops.ctypes.data, 16), bufs)
    pr, cnt, scores = bufs = outputs(((4, 2), np.int64), ((1,), np.int64), ((nq, nt), np.int32))
    done("prefilter", L.sw_prefilter_ungapped_host(*args, sub.ctypes.data, 1, pr.ctypes.data, 4, cnt.ctypes.data, scores.ctypes.data), bufs)
    return out


def test_one_step_over_every_limit_is_refused_without_a_write(swamd):
    s = arc.sequences("full8")
    small = (s["qpacked"], np.array([arc.QFRONT, arc.QFRONT + 1, arc.QFRONT + 64], np.int64), s["packed"], s["offs"][:5], arc.table("full8"))
    for go, ge in arc.NO_GAP_PAYS:                                                      # the last accepted value: every call runs
        assert [(n, rc) for n, rc, _ in host_calls(swamd, *small, go, ge)] == [(n, 0) for n in ("multi", "pairs", "top", "hits", "prefilter")]
    for go, ge in [(-arc.LIMIT, -1), (-1, -arc.LIMIT), (-arc.LIMIT - 1, 0), (0, -arc.LIMIT - 1)]:
        for n, rc, untouched in host_calls(swamd, *small, go, ge):
            if n != "prefilter":                                                        # (the pre-filter has no gap costs)
                assert rc == EINVAL and untouched, (n, go, ge)
    qpacked, qoffs, packed, offs, _, _ = arc.near_limit_case(arc.NEAR_L + 1)             # a target of L + 1 letters: 127 (L + 1) reaches 2^24
    for n, rc, untouched in host_calls(swamd, qpacked, qoffs, packed, offs, arc.near_table(), *arc.NEAR_GAPS):
        assert rc == EINVAL and untouched, n
    assert b"reaches 2^24" in swamd.lib().sw_last_error()
