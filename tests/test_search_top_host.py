"""CPU: the host leg of the per-query selection (sw_search_affine_multi_top_host) against numpy's lexsort over the full table of
sw_search_affine_multi_host, and the argument errors the device call shares with it."""
import ctypes

import numpy as np
import pytest

from affine_cases import random_submat
from top_cases import MIXED_QLENS, MIXED_TLENS, mixed_case, numpy_top

EINVAL = -22


@pytest.fixture(scope="module")
def mixed(swamd):
    """The mixed database, both scorings, and the full tables the answers are taken from (computed once, never changed)."""
    rng = np.random.default_rng(23)
    qpacked, qoffs, packed, offs = mixed_case(rng, MIXED_QLENS, MIXED_TLENS)
    sub = random_submat(rng)
    full = {(go, ge): swamd.search_affine_multi_host((qpacked, qoffs), (packed, offs), (sub, go, ge)) for go, ge in [(-11, -1), (0, -2)]}
    for f in full.values():
        f.setflags(write=False)
    return (qpacked, qoffs), (packed, offs), sub, full


@pytest.mark.parametrize("go,ge", [(-11, -1), (0, -2)])
@pytest.mark.parametrize("top", [1, 3, len(MIXED_TLENS), len(MIXED_TLENS) + 5])
def test_top_host_equals_numpy_over_the_full_table(swamd, mixed, go, ge, top):
    queries, targets, sub, full = mixed
    table = full[(go, ge)]
    occurs = int(np.sort(table[:, :, 1].reshape(-1))[table[:, :, 1].size // 2])         # a score that occurs: the median
    for min_score in (0, occurs, int(table[:, :, 1].max()) + 1):
        hits, nhits = swamd.search_affine_multi_top_host(queries, targets, (sub, go, ge), top, min_score)
        want_hits, want_nhits = numpy_top(table, top, min_score)
        assert hits.shape == (len(MIXED_QLENS), top, 3)
        assert np.array_equal(nhits, want_nhits), (top, min_score)
        assert np.array_equal(hits, want_hits), (top, min_score)
    assert (numpy_top(table, top, int(table[:, :, 1].max()) + 1)[1] == 0).all()          # above the maximum: no hit at all
    assert occurs > 0 and (numpy_top(table, len(MIXED_TLENS), occurs)[1] < len(MIXED_TLENS)).any()   # the filter does cut


def test_top_host_ties_go_to_the_lower_target(swamd):
    sub = swamd.submat_match(3, -3)
    targets = [b"ACGT", b"", b"TTGG", b"ACGT", b"GG", b"ACGT"]
    hits, nhits = swamd.search_affine_multi_top_host([b"ACGT", b"GG"], targets, (sub, -2, -1), 4)
    assert hits[0, :, 0].tolist() == [0, 3, 5, 2] and hits[0, :, 2].tolist() == [12, 12, 12, 3]
    assert hits[1, :, 0].tolist() == [2, 4, 0, 3] and nhits.tolist() == [4, 4]
    hits, nhits = swamd.search_affine_multi_top_host([b"ACGT"], targets, (sub, -2, -1), 8, min_score=1)
    assert nhits.tolist() == [5] and hits[0, :, 0].tolist() == [0, 3, 5, 2, 4, -1, -1, -1] and (hits[0, 5:, 1:] == 0).all()
    hits, nhits = swamd.search_affine_multi_top_host([b"ACGT"], targets, (sub, -2, -1), 8)           # min_score 0: empty targets qualify
    assert nhits.tolist() == [6] and hits[0, 5].tolist() == [1, 0, 0]
    assert swamd.search_affine_multi_top_host([], targets, (sub, -2, -1), 3)[0].shape == (0, 3, 3)
    hits, nhits = swamd.search_affine_multi_top_host([b"ACGT"], [], (sub, -2, -1), 3)                # no target: the fill pattern
    assert nhits.tolist() == [0] and hits.tolist() == [[[-1, 0, 0]] * 3]


def _call(swamd, qoffs, nq, sub, go, ge, top=2, offs=(0, 4), null=None):
    L = swamd.lib()
    queries, db = np.full(64, 65, np.uint8), np.full(8, 65, np.uint8)
    qoffs, offs = np.asarray(qoffs, np.int64), np.asarray(offs, np.int64)
    hits = np.full((max(1, nq) * max(1, min(top, 8)), 3), -7, np.int64)
    nhits = np.full(max(1, nq), -7, np.int64)
    sub, sc = swamd._affine(sub, go, ge)
    a = {"queries": queries.ctypes.data, "qoffsets": qoffs.ctypes.data, "db": db.ctypes.data, "offsets": offs.ctypes.data, "scoring": ctypes.byref(sc),
         "hits": hits.ctypes.data, "nhits": nhits.ctypes.data}
    if null:
        a[null] = None
    rc = L.sw_search_affine_multi_top_host(a["queries"], a["qoffsets"], nq, a["db"], a["offsets"], len(offs) - 1, a["scoring"], top, 0, a["hits"], a["nhits"])
    return rc, hits, nhits, L.sw_last_error().decode()


def test_einval_list(swamd):
    sub = swamd.submat_match(3, -3)
    rc, hits, nhits, _ = _call(swamd, [0, 4, 10], 2, sub, -2, -1, top=1)
    assert rc == 0 and nhits.tolist() == [1, 1] and hits[:, 0].tolist() == [0, 0]
    for null in ("queries", "qoffsets", "db", "offsets", "scoring", "hits", "nhits"):
        assert _call(swamd, [0, 4, 10], 2, sub, -2, -1, null=null)[0] == EINVAL, null
    bad = [
        ([0, 4, 10], -1, sub, -2, -1, 2, "negative query count"),
        ([0, 10, 4], 2, sub, -2, -1, 2, "decrease"),
        ([-1, 4, 10], 2, sub, -2, -1, 2, "negative"),
        ([0, 4, 4], 2, sub, -2, -1, 2, "length 0"),
        ([0, 4, 4 + (1 << 20)], 2, sub, -2, -1, 2, "length 1048576"),
        ([0, 4, 10], 2, sub, 1, -1, 2, "gap_open"),
        ([0, 4, 10], 2, sub, -2, 1, 2, "gap_extend"),
        ([0, 4, 10], 2, sub, -(1 << 24), -1, 2, "2^24"),
        ([0, 4, 10], 2, sub, -2, -1, 0, "top = 0"),
        ([0, 4, 10], 2, sub, -2, -1, -3, "top = -3"),
        ([0, 4, 10], 2, sub, -2, -1, swamd.SW_TOP_MAX + 1, "top = 4097"),
    ]
    for qoffs, nq, s, go, ge, top, word in bad:
        rc, hits, nhits, msg = _call(swamd, qoffs, nq, s, go, ge, top=top)
        assert rc == EINVAL and word in msg and "sw_search_affine_multi_top_host" in msg, (qoffs, nq, go, ge, top, msg)
        assert (hits == -7).all() and (nhits == -7).all()                      # an error leaves the outputs untouched
    assert _call(swamd, [0, 4, 10], 2, sub, -2, -1, offs=(0, 4, 2))[0] == EINVAL   # the offsets errors of sw_search_device
    assert _call(swamd, [0, 4, 10], 2, sub, -2, -1, offs=(-1, 4))[0] == EINVAL
    assert swamd.SW_TOP_MAX >= 4096


def test_device_entry_points_refuse_null_without_a_device(swamd):
    L = swamd.lib()
    assert L.sw_top_hits_device(None, None, 1, 1, 1, 0, None, None, None) == EINVAL
    assert L.sw_db_search_affine_top(None, None, None, None, 0, None, 1, 0, None, None, None) == EINVAL
