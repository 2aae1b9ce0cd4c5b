"""CPU: the host leg of the ungapped pre-filter (sw_prefilter_ungapped_host) against the independent checker of tests/ungapped_cases.py
-- the scores, the sorted list, a list too small for the count, the {-1, -1} tail, empty targets, offsets[0] > 0, every argument error --
and against the existing affine host leg: U <= max_score for any gap costs, U == max_score where a gap can never pay."""
import ctypes

import numpy as np
import pytest

from affine_cases import PROTEIN
from ungapped_cases import FRONT, QLENS, TLENS, mixed_case, mixed_checked, pack, passing, tables, ungapped_table

EINVAL = -22
POISON = -0x5A5A5A5A5A5A5A5B


@pytest.fixture(scope="module")
def subs(swamd):
    return tables(swamd)


@pytest.fixture(scope="module")
def case():
    qlens, qpacked, qoffs, packed, offs = mixed_case()
    return {"qlens": qlens, "q": (qpacked, qoffs), "t": (packed, offs)}


@pytest.mark.parametrize("which", ["random", "match"])
def test_scores_and_sorted_list_equal_the_checker(swamd, case, subs, which):
    want = mixed_checked(which, subs[which])
    offs = case["t"][1]
    assert offs[0] == FRONT > 0 and (np.diff(offs) == 0).sum() == 2
    nz = np.sort(want[want > 0])
    min_score = int(nz[len(nz) // 2])                                     # a score the case attains: both sides of >= are populated
    pairs, n, scores = swamd.prefilter_ungapped_host(case["q"], case["t"], subs[which], min_score)
    assert scores.dtype == np.int32 and scores.shape == (len(QLENS), len(TLENS)) and np.array_equal(scores, want)
    assert (scores[:, np.diff(offs) == 0] == 0).all() and (scores > 0).sum() > 100
    exp = passing(want, offs, min_score)
    assert 0 < len(exp) < 130 and (want[exp[:, 0], exp[:, 1]] == min_score).any() and n == len(exp)
    assert pairs.shape == (150, 2) and np.array_equal(pairs[:n], exp) and (pairs[n:] == -1).all()
    # a list too small: the true count, the first `cap` pairs of the order, nothing else; cap 0 and no list at all
    for cap in (len(exp) - 1, 1, 0):
        p2, n2, s2 = swamd.prefilter_ungapped_host(case["q"], case["t"], subs[which], min_score, cap=cap, want_scores=False)
        assert n2 == len(exp) and s2 is None and np.array_equal(p2, exp[:cap])
    # min_score above every score: no pair, the whole list is the tail
    p3, n3, _ = swamd.prefilter_ungapped_host(case["q"], case["t"], subs[which], int(want.max()) + 1, cap=7)
    assert n3 == 0 and (p3 == -1).all()
    p4, n4, _ = swamd.prefilter_ungapped_host(case["q"], case["t"], subs[which], 1)
    assert n4 == int((want[:, np.diff(offs) > 0] >= 1).sum()) and np.array_equal(p4[:n4], passing(want, offs, 1))


@pytest.mark.parametrize("which", ["random", "match"])
def test_lower_bound_of_the_affine_score_and_equal_to_it_where_no_gap_pays(swamd, case, subs, which):
    _, _, u = swamd.prefilter_ungapped_host(case["q"], case["t"], subs[which], 1)
    for go, ge in ((-11, -1), (0, -2)):
        h = swamd.search_affine_multi_host(case["q"], case["t"], (subs[which], go, ge))[:, :, 1]
        assert (u <= h).all(), (go, ge)
    assert u.max() < 30000                                                # condition of the next line: E and F stay negative everywhere
    h = swamd.search_affine_multi_host(case["q"], case["t"], (subs[which], -30000, -1))[:, :, 1]
    assert np.array_equal(u, h)


def test_small_shapes_and_edges(swamd, subs):
    rng = np.random.default_rng(9)
    for qlens, tlens, front in [([1], [1], 0), ([3, 1, 7], [0, 0], 2), ([5], [], 0), ([2, 9, 30], [4, 0, 17, 1, 33], 5)]:
        qpacked, qoffs = pack(qlens, 1, rng, PROTEIN[:20])
        packed, offs = pack(tlens, front, rng, PROTEIN[:20])
        want = ungapped_table(qpacked, qoffs, packed, offs, subs["random"])
        pairs, n, scores = swamd.prefilter_ungapped_host((qpacked, qoffs), (packed, offs), subs["random"], 3)
        exp = passing(want, offs, 3)
        assert np.array_equal(scores, want) and n == len(exp) and np.array_equal(pairs[:n], exp) and (pairs[n:] == -1).all()
    # no query
    pairs, n, scores = swamd.prefilter_ungapped_host((np.zeros(1, np.uint8), np.array([0], np.int64)), [b"ACD"], subs["random"], 1, cap=3)
    assert n == 0 and (pairs == -1).all() and scores.shape == (0, 1)
    # a planted copy scores at least its self-scores, on the diagonal
    q = rng.choice(PROTEIN[:20], 60).astype(np.uint8)
    t = rng.choice(PROTEIN[:20], 90).astype(np.uint8)
    t[31:71] = q[10:50]
    self_score = int(subs["random"][q[10:50], q[10:50]].astype(np.int64).sum())
    _, _, scores = swamd.prefilter_ungapped_host([q], [t], subs["random"], 1)
    assert scores[0, 0] >= self_score > 0 and scores[0, 0] == ungapped_table(q, [0, 60], t, [0, 90], subs["random"])[0, 0]


def test_argument_errors_leave_the_outputs_untouched(swamd, case, subs):
    L = swamd.lib()
    (qpacked, qoffs), (packed, offs) = case["q"], case["t"]
    sub = np.ascontiguousarray(subs["random"], np.int8)
    pairs = np.full((150, 2), POISON, np.int64)
    scores = np.full(150, -0x5A5A5A5B, np.int32)
    n = ctypes.c_int64(POISON)

    def call(**kw):
        a = {"q": qpacked.ctypes.data, "qoffs": qoffs, "nq": len(QLENS), "db": packed.ctypes.data, "offs": offs, "nt": len(TLENS), "sub": sub.ctypes.data,
             "min": 5, "pairs": pairs.ctypes.data, "cap": 150, "n": ctypes.addressof(n), "scores": scores.ctypes.data, **kw}
        qo = None if a["qoffs"] is None else np.ascontiguousarray(a["qoffs"], np.int64)
        to = None if a["offs"] is None else np.ascontiguousarray(a["offs"], np.int64)
        return L.sw_prefilter_ungapped_host(a["q"], None if qo is None else qo.ctypes.data, a["nq"], a["db"], None if to is None else to.ctypes.data, a["nt"],
                                            a["sub"], a["min"], a["pairs"], a["cap"], a["n"], a["scores"])

    big = np.zeros((256, 256), np.int8)
    big[65, 65] = 127
    bad = [{"q": None}, {"qoffs": None}, {"db": None}, {"offs": None}, {"sub": None}, {"nq": -1}, {"nt": -1},
           {"qoffs": [4, 4], "nq": 1}, {"qoffs": [4, 2], "nq": 1}, {"qoffs": [-1, 3], "nq": 1}, {"qoffs": [0, 1 << 20], "nq": 1},   # the query lengths
           {"offs": [3, 2], "nt": 1}, {"offs": [-1, 2], "nt": 1}, {"offs": [0, 1 << 20], "nt": 1},                                # the offsets
           {"sub": big.ctypes.data, "qoffs": [0, 1 << 18], "nq": 1, "offs": [0, 1 << 18], "nt": 1},                              # 127 x 2^18 reaches 2^24
           {"min": 0}, {"min": -3}, {"cap": -1}, {"pairs": None}, {"n": None}, {"n": None, "scores": None},
           {"n": None, "pairs": None, "cap": 0, "scores": None}]                                                                  # everything NULL
    for kw in bad:
        assert call(**kw) == EINVAL, kw
        assert (pairs == POISON).all() and (scores == -0x5A5A5A5B).all() and n.value == POISON, kw
    assert call(n=None, pairs=None, cap=0) == 0 and n.value == POISON                    # the scores alone need no count
    assert np.array_equal(scores.reshape(10, 15), mixed_checked("random", subs["random"]))
    assert call(pairs=None, cap=0, scores=None) == 0 and n.value == len(passing(mixed_checked("random", subs["random"]), offs, 5))   # the count alone
    assert call() == 0 and (pairs[n.value:] == -1).all() and (pairs[:n.value] >= 0).all()
