"""CPU: the host leg of the selection from a scored pair list (sw_top_hits_pairs_host) against numpy on synthetic lists, its argument
errors, and the chain of host legs prefilter_ungapped_host -> search_affine_pairs_host -> top_hits_pairs_host against the full table."""
import numpy as np
import pytest

from affine_cases import random_submat
from pairs_top_cases import PATTERNS, SCORE_MAX, junk_entries, numpy_top_pairs, synthetic_list, with_junk
from top_cases import MIXED_QLENS, MIXED_TLENS, mixed_case, numpy_top

EINVAL = -22
# the lengths at which the device kernels change their path (tests/test_top_pairs_gpu.py), in two lists of five queries
SEGLENS_A = [0, 1, 63, 4095, 2 * 4096 + 1]
SEGLENS_B = [2, 64, 65, 4096, 4097]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("top", [1, 2, 3, 64, 65, 4096])
@pytest.mark.parametrize("SEGLENS", [SEGLENS_A, SEGLENS_B], ids=["a", "b"])
def test_host_equals_numpy_on_synthetic_lists(swamd, pattern, top, SEGLENS):
    rng = np.random.default_rng(5)
    nq, nt = len(SEGLENS), 1 << 14
    pairs, results = synthetic_list(rng, SEGLENS, nt, pattern, last_target=True)
    pairs, results = with_junk(rng, pairs, results, nq, nt)
    smax = int(results[:len(results), 1][(pairs[:, 0] >= 0) & (pairs[:, 0] < nq) & (pairs[:, 1] >= 0) & (pairs[:, 1] < nt)].max())
    for min_score in (-3, 0, 1, 6, 77, 78, smax, smax + 1):
        hits, nhits = swamd.top_hits_pairs_host(pairs, results, nq, nt, top, min_score)
        want_hits, want_nhits = numpy_top_pairs(pairs, results, nq, nt, top, min_score)
        assert np.array_equal(nhits, want_nhits), (pattern, top, min_score)
        assert np.array_equal(hits, want_hits), (pattern, top, min_score)
    assert (swamd.top_hits_pairs_host(pairs, results, nq, nt, top, smax + 1)[1] == 0).all()       # above the maximum: no hit at all


def test_junk_alone_gives_empty_rows(swamd):
    jp, jr = junk_entries(3, 10)
    hits, nhits = swamd.top_hits_pairs_host(jp, jr, 3, 10, 4)
    assert nhits.tolist() == [0, 0, 0] and (hits[:, :, 0] == -1).all() and (hits[:, :, 1:] == 0).all()


def test_the_key_of_zero_is_a_hit(swamd):
    # score 0 at the last target of a power-of-two database: the key is 0, and with min_score <= 0 it is a hit like any other
    pairs = np.array([[0, 7], [0, 3], [1, 7]], np.int64)
    results = np.array([[11, 0, 0], [12, 0, 0], [13, 0, 0]], np.int64)
    hits, nhits = swamd.top_hits_pairs_host(pairs, results, 2, 8, 3, 0)
    assert nhits.tolist() == [2, 1] and hits[0].tolist() == [[3, 12, 0], [7, 11, 0], [-1, 0, 0]] and hits[1, 0].tolist() == [7, 13, 0]
    assert swamd.top_hits_pairs_host(pairs, results, 2, 8, 3, 1)[1].tolist() == [0, 0]


def test_duplicates_come_out_by_list_position(swamd):
    pairs = np.array([[0, 5], [0, 2], [0, 5], [0, 5], [0, 2]], np.int64)
    results = np.array([[40, 9, 0], [41, 9, 0], [42, 9, 0], [43, 10, 0], [44, 9, 0]], np.int64)
    hits, nhits = swamd.top_hits_pairs_host(pairs, results, 1, 6, 8)
    assert nhits.tolist() == [5]
    assert hits[0, :5].tolist() == [[5, 43, 10], [2, 41, 9], [2, 44, 9], [5, 40, 9], [5, 42, 9]]
    assert np.array_equal(hits, numpy_top_pairs(pairs, results, 1, 6, 8)[0])


def test_empty_calls(swamd):
    none = np.zeros((0, 2), np.int64), np.zeros((0, 3), np.int64)
    hits, nhits = swamd.top_hits_pairs_host(*none, 3, 5, 2)
    assert nhits.tolist() == [0, 0, 0] and hits.tolist() == [[[-1, 0, 0]] * 2] * 3
    assert swamd.top_hits_pairs_host(*none, 0, 5, 2)[0].shape == (0, 2, 3)
    pairs, results = synthetic_list(np.random.default_rng(1), [3], 1 << 20, "random")
    hits, nhits = swamd.top_hits_pairs_host(pairs, results, 1, 1, 2)        # one target: only target 0 is inside
    assert nhits[0] == int((pairs[:, 1] == 0).sum())
    hits, nhits = swamd.top_hits_pairs_host(np.array([[0, 0], [0, 0]], np.int64), np.array([[1, 4, 0], [2, 5, 0]], np.int64), 1, 1, 2)
    assert hits[0].tolist() == [[0, 2, 5], [0, 1, 4]]
    assert swamd.top_hits_pairs_host(pairs, results, 1, 0, 2)[1].tolist() == [0]


def _call(swamd, npairs=2, nq=2, nt=4, top=2, null=None):
    L = swamd.lib()
    pairs, results = np.zeros((4, 2), np.int64), np.zeros((4, 3), np.int64)
    hits, nhits = np.full((16, 3), -7, np.int64), np.full(4, -7, np.int64)
    a = {"pairs": pairs.ctypes.data, "results": results.ctypes.data, "hits": hits.ctypes.data, "nhits": nhits.ctypes.data}
    if null:
        a[null] = None
    rc = L.sw_top_hits_pairs_host(a["pairs"], a["results"], npairs, nq, nt, top, 0, a["hits"], a["nhits"])
    return rc, hits, nhits, L.sw_last_error().decode()


def test_einval_list(swamd):
    rc, hits, nhits, _ = _call(swamd)
    assert rc == 0 and nhits[:2].tolist() == [2, 0] and (hits[4:] == -7).all()
    for null in ("pairs", "results", "hits", "nhits"):
        assert _call(swamd, null=null)[0] == EINVAL, null
    assert _call(swamd, npairs=0, null="pairs")[0] == 0 and _call(swamd, npairs=0, null="results")[0] == 0   # no entry, nothing to read
    bad = [({"npairs": -1}, "npairs"), ({"npairs": 1 << 31}, "npairs"), ({"nq": -1}, "negative query count"), ({"nt": -1}, "ntargets"),
           ({"nt": 1 << 31}, "ntargets"), ({"top": 0}, "top = 0"), ({"top": -3}, "top = -3"), ({"top": swamd.SW_TOP_MAX + 1}, "top = 4097")]
    for kw, word in bad:
        rc, hits, nhits, msg = _call(swamd, **kw)
        assert rc == EINVAL and word in msg and "sw_top_hits_pairs_host" in msg, (kw, msg)
        assert (hits == -7).all() and (nhits == -7).all()                      # an error leaves the outputs untouched


def test_device_entry_points_refuse_null_without_a_device(swamd):
    L = swamd.lib()
    assert L.sw_top_hits_pairs_device(None, None, None, 0, 1, 1, 1, 0, None, None, None) == EINVAL
    assert L.sw_db_search_affine_top_prefiltered(None, None, None, None, 0, None, 1, 0, 1, 0, None, None, None, None) == EINVAL


@pytest.fixture(scope="module")
def mixed(swamd):
    """The mixed protein case, its full table and its ungapped scores (computed once, never changed)."""
    rng = np.random.default_rng(23)
    qpacked, qoffs, packed, offs = mixed_case(rng, MIXED_QLENS, MIXED_TLENS)
    sub = random_submat(rng)
    queries, targets = (qpacked, qoffs), (packed, offs)
    full = swamd.search_affine_multi_host(queries, targets, (sub, -11, -1))
    full.setflags(write=False)
    return queries, targets, sub, full


@pytest.mark.parametrize("top", [1, 3, len(MIXED_TLENS) + 5])
def test_chain_of_host_legs_equals_the_masked_full_table(swamd, mixed, top):
    queries, targets, sub, full = mixed
    nq, nt = len(MIXED_QLENS), len(MIXED_TLENS)
    _, _, u = swamd.prefilter_ungapped_host(queries, targets, sub, 1)
    S = int(np.sort(u[u > 0])[(u > 0).sum() // 2])                              # a threshold the case attains: both sides are populated
    pairs, n, _ = swamd.prefilter_ungapped_host(queries, targets, sub, S)
    assert 0 < n < nq * nt and pairs.shape == (nq * nt, 2) and (pairs[n:] == -1).all()
    results = swamd.search_affine_pairs_host(queries, targets, (sub, -11, -1), pairs)      # all cap entries: the tail gives zeros
    occurs = int(np.sort(full[:, :, 1].reshape(-1))[full[:, :, 1].size // 2])
    for min_score in (0, 1, occurs, int(full[:, :, 1].max()) + 1):
        hits, nhits = swamd.top_hits_pairs_host(pairs, results, nq, nt, top, min_score)
        masked = full.copy()
        masked[u < S] = (0, -1, 0)                                              # a pair the filter removed qualifies under no min_score >= 0 ...
        want_hits, want_nhits = numpy_top(masked, top, max(min_score, 0))
        empty = np.diff(targets[1]) == 0                                        # (... an empty target never passes: U = 0 < S)
        assert (u[:, empty] == 0).all() and S >= 1
        assert np.array_equal(nhits, want_nhits) and np.array_equal(hits, want_hits), (top, min_score)


@pytest.mark.parametrize("top", [1, 4, len(MIXED_TLENS)])
def test_chain_with_threshold_one_equals_the_top_host_leg(swamd, mixed, top):
    queries, targets, sub, full = mixed
    nq, nt = len(MIXED_QLENS), len(MIXED_TLENS)
    pairs, n, _ = swamd.prefilter_ungapped_host(queries, targets, sub, 1)
    results = swamd.search_affine_pairs_host(queries, targets, (sub, -11, -1), pairs)
    hits, nhits = swamd.top_hits_pairs_host(pairs, results, nq, nt, top, 1)
    want_hits, want_nhits = swamd.search_affine_multi_top_host(queries, targets, (sub, -11, -1), top, 1)
    assert hits.tobytes() == want_hits.tobytes() and nhits.tobytes() == want_nhits.tobytes()
    assert want_nhits.max() > 0 and SCORE_MAX > int(full[:, :, 1].max())
