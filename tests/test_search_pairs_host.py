"""CPU: the host leg of the pair-list search (sw_search_affine_pairs_host) against the gathered entries of the many-query host leg
(sw_search_affine_multi_host) and against the independent checker (tests/affine_oracle.cpp); entries that name no query or no target,
duplicates, an empty list, and the argument errors sw_db_search_affine_pairs shares with it -- checked before any result is written."""
import ctypes

import numpy as np
import pytest

from affine_cases import PROTEIN, checker  # noqa: F401

EINVAL = -22
QLENS = [1, 4, 255, 256, 257, 512, 513, 1024, 1025, 2049]        # those of tests/test_search_multi_gpu.py
TLENS = [0, 1, 63, 64, 65, 127, 300, 1100, 64, 0, 1, 300, 65, 127, 63]
QFRONT, FRONT = 4, 3
INT64_MIN = -(1 << 63)


def pack(lens, front, rng, alpha):
    offs = np.zeros(len(lens) + 1, np.int64)
    offs[0] = front
    offs[1:] = front + np.cumsum(lens)
    return rng.choice(alpha, max(1, int(offs[-1]))).astype(np.uint8), offs


@pytest.fixture(scope="module")
def scorings(swamd):
    """The two scorings of tests/test_search_multi_gpu.py."""
    rng = np.random.default_rng(5)
    n = len(PROTEIN)
    sc = rng.integers(-8, 13, (n, n)).astype(np.int8)
    sc[np.arange(n), np.arange(n)] = rng.integers(4, 13, n).astype(np.int8)
    return {"affine": (swamd.submat_from_letters(PROTEIN, sc, -8), -11, -1), "linear": (swamd.submat_match(3, -3), 0, -2)}


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(2024)
    qlens = list(QLENS)
    rng.shuffle(qlens)
    qpacked, qoffs = pack(qlens, QFRONT, rng, PROTEIN[:20])
    packed, offs = pack(TLENS, FRONT, rng, PROTEIN[:20])
    pairs = np.array([(q, k) for q in range(len(QLENS)) for k in range(len(TLENS))], np.int64)
    pairs = pairs[np.random.default_rng(7).permutation(len(pairs))]
    return {"qpacked": qpacked, "qoffs": qoffs, "packed": packed, "offs": offs, "pairs": pairs}


@pytest.mark.parametrize("which", ["affine", "linear"])
def test_shuffled_cross_product_equals_the_gathered_table_and_the_checker(swamd, checker, case, scorings, which):  # noqa: F811
    q, t, pairs = (case["qpacked"], case["qoffs"]), (case["packed"], case["offs"]), case["pairs"]
    assert not np.array_equal(pairs, pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))])      # condition of this test: really shuffled
    table = swamd.search_affine_multi_host(q, t, scorings[which])
    got = swamd.search_affine_pairs_host(q, t, scorings[which], pairs)
    assert got.shape == (150, 3) and got.dtype == np.int64
    assert np.array_equal(got, table[pairs[:, 0], pairs[:, 1]])
    assert (got[np.diff(case["offs"])[pairs[:, 1]] == 0] == 0).all() and (got[:, 1] > 0).sum() > 80
    # a sample of the pairs against the independent checker: every query once, with every target
    sub, go, ge = scorings[which]
    for qi in range(len(QLENS)):
        want = checker.search(case["qpacked"][case["qoffs"][qi]:case["qoffs"][qi + 1]], case["packed"], case["offs"], sub, go, ge)
        mine = pairs[:, 0] == qi
        assert np.array_equal(got[mine], want[pairs[mine, 1]]), f"query {qi}"


def test_entries_outside_the_queries_or_the_targets_are_zero(swamd, case, scorings):
    q, t = (case["qpacked"], case["qoffs"]), (case["packed"], case["offs"])
    nq, nt = len(QLENS), len(TLENS)
    good = swamd.search_affine_pairs_host(q, t, scorings["affine"], [(3, 7)])[0]
    assert good[1] > 0
    pairs = [(3, 7)]
    for bad_q in (-1, nq, 1 << 40, INT64_MIN):
        pairs += [(bad_q, 7), (bad_q, -1), (bad_q, 0)]
    for bad_t in (-1, nt, 1 << 40, INT64_MIN):
        pairs += [(3, bad_t), (0, bad_t)]
    pairs += [(3, 7), (nq - 1, nt - 1), (3, 0), (3, 9)]                                  # good entries between and behind them; two empty targets
    got = swamd.search_affine_pairs_host(q, t, scorings["affine"], pairs)
    assert np.array_equal(got[0], good) and np.array_equal(got[21], good)
    assert (got[1:21] == 0).all() and (got[23:] == 0).all() and got[22, 1] > 0


def test_duplicates_give_equal_entries(swamd, case, scorings):
    q, t = (case["qpacked"], case["qoffs"]), (case["packed"], case["offs"])
    pairs = [(2, 7), (5, 6), (2, 7), (2, 7), (5, 6), (0, 1)]
    got = swamd.search_affine_pairs_host(q, t, scorings["affine"], pairs)
    assert np.array_equal(got[0], got[2]) and np.array_equal(got[0], got[3]) and np.array_equal(got[1], got[4])
    assert got[0, 1] > 0 and got[1, 1] > 0 and not np.array_equal(got[0], got[1])


def _call(swamd, pairs, npairs=None, qoffs=(0, 4, 10), nq=2, go=-2, ge=-1, offs=(0, 4), null=None, sub=None):
    """sw_search_affine_pairs_host on 64 letters of queries and a 4-letter database into poisoned results; `null` names an argument passed as NULL."""
    L = swamd.lib()
    queries, db = np.full(64, 65, np.uint8), np.full(8, 65, np.uint8)
    qoffs, offs = np.asarray(qoffs, np.int64), np.asarray(offs, np.int64)
    pr = np.ascontiguousarray(np.asarray(pairs, np.int64).reshape(-1, 2))
    res = np.full((max(1, len(pr)), 3), -7, np.int64)
    table, sc = swamd._affine(swamd.submat_match(3, -3) if sub is None else sub, go, ge)
    a = {"queries": queries.ctypes.data, "qoffsets": qoffs.ctypes.data, "db": db.ctypes.data, "offsets": offs.ctypes.data, "scoring": ctypes.byref(sc),
         "pairs": pr.ctypes.data, "results": res.ctypes.data}
    if null:
        a[null] = None
    rc = L.sw_search_affine_pairs_host(a["queries"], a["qoffsets"], nq, a["db"], a["offsets"], len(offs) - 1, a["scoring"], a["pairs"],
                                       len(pr) if npairs is None else npairs, a["results"])
    return rc, res, L.sw_last_error().decode()


def test_an_empty_list_writes_nothing(swamd):
    rc, res, _ = _call(swamd, [(0, 0)], npairs=0)
    assert rc == 0 and (res == -7).all()
    for null in ("pairs", "results"):                                                   # neither is looked at without a pair
        rc, res, _ = _call(swamd, [(0, 0)], npairs=0, null=null)
        assert rc == 0 and (res == -7).all()
    assert swamd.search_affine_pairs_host([b"ACGT"], [b"ACGT"], (swamd.submat_match(3, -3), -2, -1), []).shape == (0, 3)
    rc, res, _ = _call(swamd, [(0, 0), (1, 0)], qoffs=(0,), nq=0)                        # no query: every entry names none
    assert rc == 0 and (res == 0).all()


def test_every_einval_comes_before_the_first_result(swamd):
    pairs = [(0, 0), (1, 0), (0, 0)]
    rc, res, _ = _call(swamd, pairs)
    assert rc == 0 and res[:, 1].tolist() == [12, 12, 12] and (res[:, 2] == 0).all()
    for null in ("queries", "qoffsets", "db", "offsets", "scoring", "pairs", "results"):
        rc, res, _ = _call(swamd, pairs, null=null)
        assert rc == EINVAL and (res == -7).all(), null
    bad = [
        ({"npairs": -1}, "negative pair count"),
        ({"nq": -1}, "negative query count"),
        ({"qoffs": (0, 10, 4)}, "decrease"),
        ({"qoffs": (-1, 4, 10)}, "negative"),
        ({"qoffs": (0, 4, 4)}, "length 0"),
        ({"qoffs": (0, 4, 4 + (1 << 20))}, "length 1048576"),
        ({"go": 1}, "gap_open"),
        ({"ge": 1}, "gap_extend"),
        ({"go": -(1 << 24)}, "2^24"),
        ({"offs": (0, 4, 2)}, "decrease"),                                              # the offsets errors of sw_search_device
        ({"offs": (-1, 4)}, "negative"),
    ]
    for kw, word in bad:
        rc, res, msg = _call(swamd, pairs, **kw)
        assert rc == EINVAL and word in msg and "sw_search_affine_pairs_host" in msg, (kw, msg)
        assert (res == -7).all(), kw                                                    # an error leaves the results untouched


def test_device_entry_point_refuses_null_without_a_device(swamd):
    assert swamd.lib().sw_db_search_affine_pairs(None, None, None, None, 0, None, None, 0, None, None) == EINVAL
