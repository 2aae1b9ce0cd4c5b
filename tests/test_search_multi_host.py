"""CPU: the host leg of the many-query search (sw_search_affine_multi_host) against sw_search_affine_host query by query and against
the independent checker (tests/affine_oracle.cpp), and the argument errors sw_db_search_affine shares with it -- the two entry points
check their queries and scoring through one function, so what can be checked without a device is checked here."""
import ctypes

import numpy as np
import pytest

from affine_cases import PROTEIN, assert_same, checker, random_submat  # noqa: F401

EINVAL = -22


def _case(rng, qlens, tlens, qfront=5, front=3):
    qoffs = np.zeros(len(qlens) + 1, np.int64)
    qoffs[0] = qfront
    qoffs[1:] = qfront + np.cumsum(qlens)
    offs = np.zeros(len(tlens) + 1, np.int64)
    offs[0] = front
    offs[1:] = front + np.cumsum(tlens)
    return rng.choice(PROTEIN, int(qoffs[-1])).astype(np.uint8), qoffs, rng.choice(PROTEIN, max(1, int(offs[-1]))).astype(np.uint8), offs


@pytest.mark.parametrize("go,ge", [(-11, -1), (0, -2)])
def test_multi_host_equals_the_single_query_host_leg(swamd, checker, go, ge):  # noqa: F811
    rng = np.random.default_rng(11)
    qpacked, qoffs, packed, offs = _case(rng, [1, 40, 7, 130, 64], [0, 1, 63, 64, 65, 0, 127, 300, 1, 90])
    sub = random_submat(rng)
    res = swamd.search_affine_multi_host((qpacked, qoffs), (packed, offs), (sub, go, ge))
    assert res.shape == (5, 10, 3)
    for q in range(5):
        query = qpacked[qoffs[q]:qoffs[q + 1]]
        assert_same(res[q], swamd.search_affine_host(query, (packed, offs), sub, go, ge), f"query {q}")
        assert_same(res[q], checker.search(query, packed, offs, sub, go, ge), f"query {q} against the checker")
    assert (res[:, [0, 5], :] == 0).all()                     # empty targets: {0, 0, 0}


def test_multi_host_lists_and_degenerate_counts(swamd):
    sub = swamd.submat_match(3, -3)
    res = swamd.search_affine_multi_host([b"ACGT", b"GG"], [b"ACGT", b"", b"TTGG"], (sub, -2, -1))
    assert res[:, :, 1].tolist() == [[12, 0, 3], [3, 0, 6]]
    assert swamd.search_affine_multi_host([], [b"ACGT"], (sub, -2, -1)).shape == (0, 1, 3)       # no query: SW_OK, nothing written
    assert swamd.search_affine_multi_host([b"ACGT"], [], (sub, -2, -1)).shape == (1, 0, 3)       # no target


def _call(swamd, qoffs, nq, sub, go, ge, offs=(0, 4), null=None):
    """sw_search_affine_multi_host on 64 letters of queries and a 4-letter database; `null` names an argument passed as NULL."""
    L = swamd.lib()
    queries, db = np.full(64, 65, np.uint8), np.full(8, 65, np.uint8)
    qoffs, offs = np.asarray(qoffs, np.int64), np.asarray(offs, np.int64)
    res = np.full((max(1, nq) * (len(offs) - 1), 3), -7, np.int64)
    sub, sc = swamd._affine(sub, go, ge)
    a = {"queries": queries.ctypes.data, "qoffsets": qoffs.ctypes.data, "db": db.ctypes.data, "offsets": offs.ctypes.data, "scoring": ctypes.byref(sc),
         "results": res.ctypes.data}
    if null:
        a[null] = None
    rc = L.sw_search_affine_multi_host(a["queries"], a["qoffsets"], nq, a["db"], a["offsets"], len(offs) - 1, a["scoring"], a["results"])
    return rc, res, L.sw_last_error().decode()


def test_einval_list(swamd):
    sub = swamd.submat_match(3, -3)
    rc, res, _ = _call(swamd, [0, 4, 10], 2, sub, -2, -1)
    assert rc == 0 and (res[:, 2] == 0).all() and (res[:, 1] > 0).all()
    for null in ("queries", "qoffsets", "db", "offsets", "scoring", "results"):
        assert _call(swamd, [0, 4, 10], 2, sub, -2, -1, null=null)[0] == EINVAL, null
    bad = [
        ([0, 4, 10], -1, sub, -2, -1, "negative query count"),
        ([0, 10, 4], 2, sub, -2, -1, "decrease"),
        ([-1, 4, 10], 2, sub, -2, -1, "negative"),
        ([0, 4, 4], 2, sub, -2, -1, "length 0"),                               # an empty query
        ([0, 4, 4 + (1 << 20)], 2, sub, -2, -1, "length 1048576"),             # above 2^20 - 1 (checked before any byte is read)
        ([0, 4, 10], 2, sub, 1, -1, "gap_open"),
        ([0, 4, 10], 2, sub, -2, 1, "gap_extend"),
        ([0, 4, 10], 2, sub, -(1 << 24), -1, "2^24"),
    ]
    for qoffs, nq, s, go, ge, word in bad:
        rc, res, msg = _call(swamd, qoffs, nq, s, go, ge)
        assert rc == EINVAL and word in msg and "sw_search_affine_multi_host" in msg, (qoffs, nq, go, ge, msg)
        assert (res == -7).all()                                               # an error leaves the results untouched
    assert _call(swamd, [0, 4, 10], 2, sub, -2, -1, offs=(0, 4, 2))[0] == EINVAL   # the offsets errors of sw_search_device
    assert _call(swamd, [0, 4, 10], 2, sub, -2, -1, offs=(-1, 4))[0] == EINVAL


def test_score_bound_is_taken_over_the_longest_query(swamd):
    """127 x min(longest query, longest target) must stay below 2^24: a long query among short ones decides, whatever its position."""
    L = swamd.lib()
    n = (1 << 24) // 127 + 1                                   # 132 105 letters: 127 n >= 2^24
    sub, sc = swamd._affine(swamd.submat_match(127, -3), -2, -1)
    queries, db = np.full(n + 16, 65, np.uint8), np.full(n, 67, np.uint8)
    offs = np.array([0, n], np.int64)
    res = np.zeros((3, 3), np.int64)
    call = lambda qoffs: L.sw_search_affine_multi_host(queries.ctypes.data, np.asarray(qoffs, np.int64).ctypes.data, 3, db.ctypes.data,  # noqa: E731
                                                       offs.ctypes.data, 1, ctypes.byref(sc), res.ctypes.data)
    assert call([0, 4, 4 + n, 8 + n]) == EINVAL and "2^24" in L.sw_last_error().decode()
    offs[1] = 100                                              # a short longest target: min(...) is small again
    assert call([0, 4, 8, 12]) == 0


def test_device_entry_points_refuse_null_without_a_device(swamd):
    L = swamd.lib()
    h = ctypes.c_void_p()
    offs = np.array([0, 4], np.int64)
    assert L.sw_db_create(None, None, offs.ctypes.data, 1, ctypes.byref(h)) == EINVAL and h.value is None
    assert L.sw_db_info(None, None, None, None, None) == EINVAL
    assert L.sw_db_search_affine(None, None, None, None, 0, None, None, None) == EINVAL
    L.sw_db_free(None)                                         # a no-op
