"""GPU: the best entries per query selected on the device from a scored pair list (sw_top_hits_pairs_device,
sw_db_search_affine_top_prefiltered; csrc/sw_top_pairs.hip).  The selection alone runs on synthetic lists uploaded from numpy -- no
search at all -- and is compared exactly with numpy's lexsort (tests/pairs_top_cases.py); the chain filter -> rescoring -> selection
-> alignment is compared with numpy over the full table of Database.search_affine_device masked by the filter's own scores.  Inputs and
outputs lie in poisoned arenas between guards at odd bases: every output entry must be written, nothing else may change."""
import ctypes

import numpy as np
import pytest

from affine_cases import PROTEIN
from buffer_cases import POISON64, Arena, arena_bytes, assert_guards
from pairs_top_cases import PATTERNS, SCORE_MAX, junk_entries, max_pos_of, numpy_top_pairs, synthetic_list, with_junk
from top_cases import numpy_top

pytestmark = pytest.mark.gpu
EINVAL = -22
TOP_MAX = 4096
NT = 1 << 14                        # a power of two: target NT - 1 with score 0 has the key 0
# the whole-sort boundary (4096), the first streamed block (4097), a second merge (2 * 4096 + 1), and the small ones
SEGLENS_A = [0, 1, 63, 4095, 2 * 4096 + 1]
SEGLENS_B = [2, 64, 65, 4096, 4097]
TOPS = [1, 2, 3, 64, 65, TOP_MAX]


class Bench:
    """The list and its results in one arena (inputs: they must stay as they are), the outputs in another that is poisoned anew for
    every call."""

    def __init__(self, engine, pairs, results, nq, nt, max_top=TOP_MAX):
        t = engine.torch
        self.engine, self.pairs, self.results, self.nq, self.nt = engine, pairs, results, nq, nt
        self.n = len(pairs)
        self.ain = Arena(t, f"cuda:{engine.device}", arena_bytes(self.n * 16, self.n * 24))
        self.d_pairs, _ = self.ain.place(pairs.reshape(-1).view(np.uint8), align=16, skew=8, name="pairs")     # 8 bytes of alignment, no more
        self.d_results, _ = self.ain.place(results.reshape(-1).view(np.uint8), align=16, skew=8, name="results")
        self.aout = Arena(t, f"cuda:{engine.device}", 2 * arena_bytes(max(1, nq) * max_top * 24, max(1, nq) * 8))

    def outputs(self, top):
        t = self.engine.torch
        ch = self.aout.carve(self.nq * top * 24, 16, 8, name=f"hits{len(self.aout.carves)}")
        cn = self.aout.carve(self.nq * 8, 16, 8, name=f"nhits{len(self.aout.carves)}")
        return self.aout.view(ch, t.int64, (self.nq * top * 3,)), self.aout.view(cn, t.int64, (self.nq,))

    def select(self, top, min_score, twice=False):
        self.aout.reset()
        outs = [self.outputs(top) for _ in range(2 if twice else 1)]
        got = [self.engine.top_hits_pairs_device(self.d_pairs, self.d_results, self.n, self.nq, self.nt, top, min_score, out=o) for o in outs]
        self.engine.synchronize()
        assert_guards(self.aout)
        assert_guards(self.ain)
        return [(h.cpu().numpy(), n.cpu().numpy()) for h, n in got]

    def check(self, top, min_score, what):
        (hits, nhits), = self.select(top, min_score)
        want_hits, want_nhits = numpy_top_pairs(self.pairs, self.results, self.nq, self.nt, top, min_score)
        assert np.array_equal(nhits, want_nhits), f"{what} top {top} min_score {min_score}: nhits {nhits.tolist()[:8]} vs {want_nhits.tolist()[:8]}"
        bad = np.argwhere((hits != want_hits).any(axis=2))
        assert len(bad) == 0, (f"{what} top {top} min_score {min_score}: {len(bad)} hits differ, first (query, rank) {tuple(bad[0])}: "
                               f"{hits[tuple(bad[0])]} vs {want_hits[tuple(bad[0])]}")
        return nhits


def thresholds(pairs, results, nq, nt):
    """<= 0 twice, at the lowest score, inside a tie run (the median), just above it, above the maximum."""
    ok = (pairs[:, 0] >= 0) & (pairs[:, 0] < nq) & (pairs[:, 1] >= 0) & (pairs[:, 1] < nt)
    s = np.sort(results[ok, 1])
    lo, mid, hi = int(s[0]), int(s[len(s) // 2]), int(s[-1])
    return [-7, 0, lo, mid, mid + 1, hi + 1], hi


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("seglens", [SEGLENS_A, SEGLENS_B], ids=["a", "b"])
def test_selection_alone_five_queries(engine, pattern, seglens):
    """Five queries of mixed lengths in one shuffled list with the entries that must drop out mixed in."""
    rng = np.random.default_rng(len(pattern) + seglens[0])
    pairs, results = synthetic_list(rng, seglens, NT, pattern, last_target=True)
    pairs, results = with_junk(rng, pairs, results, len(seglens), NT)
    b = Bench(engine, pairs, results, len(seglens), NT)
    mins, hi = thresholds(pairs, results, b.nq, NT)
    for top in TOPS:
        for min_score in mins:
            nhits = b.check(top, min_score, f"{pattern} {seglens}")
            if min_score == hi + 1:
                assert (nhits == 0).all()
            if min_score <= 0:
                assert nhits.tolist() == [min(top, n) for n in seglens]           # every in-range entry qualifies, the key-0 item included
    assert engine.get_option("last_top_pairs_kernel") == 1 and engine.get_option("last_top_pairs_launches") == 4


@pytest.mark.parametrize("pattern", PATTERNS)
def test_selection_alone_one_query(engine, pattern):
    """One query, every segment length in a list of its own."""
    rng = np.random.default_rng(len(pattern))
    for n in sorted(SEGLENS_A + SEGLENS_B):
        pairs, results = synthetic_list(rng, [n], NT, pattern, last_target=True)
        pairs, results = with_junk(rng, pairs, results, 1, NT)
        b = Bench(engine, pairs, results, 1, NT)
        mins, hi = thresholds(pairs, results, 1, NT) if n else ([0], 0)
        mid = mins[len(mins) // 2]
        for top, min_score in [(1, 0), (3, mid), (65, mid + 1), (TOP_MAX, -1), (TOP_MAX, mid), (2, hi + 1)]:
            b.check(top, min_score, f"{pattern} one query of {n}")
        assert engine.get_option("last_top_pairs_kernel") == (1 if len(pairs) > TOP_MAX else 0)


def test_more_queries_than_the_lds_form_takes(engine):
    """8197 queries, most of them empty: count and scatter take one atomic per entry, the scan runs over three tiles."""
    rng = np.random.default_rng(8197)
    nq = 8192 + 5
    seglens = {0: 3, 1: 65, 4000: 4097, 4095: 7, 4096: 9, 8191: 1, 8192: 1, nq - 1: 2}
    pairs, results = synthetic_list(rng, seglens, NT, "four", last_target=True)
    pairs, results = with_junk(rng, pairs, results, nq, NT)
    b = Bench(engine, pairs, results, nq, NT, max_top=65)
    for top, min_score in [(1, 0), (3, 5), (65, 6), (65, -1), (2, 901)]:
        nhits = b.check(top, min_score, "8197 queries")
        if min_score <= 0:
            assert int(nhits.sum()) == sum(min(top, n) for n in seglens.values())


def test_the_key_of_zero_lies_before_the_padding(engine):
    """Three entries are sorted as four items: the padding must sort behind the real item whose key is 0 (score 0, target 2^tbits - 1)."""
    for nt in (8, NT):
        pairs = np.array([[0, nt - 1], [0, 3], [1, nt - 1], [0, 5]], np.int64)
        results = np.array([[11, 0, 0], [12, 0, 0], [13, 0, 0], [14, 0, 0]], np.int64)
        b = Bench(engine, pairs, results, 2, nt, max_top=8)
        for top in (1, 3, 4, 8):
            nhits = b.check(top, 0, "key 0")
            assert nhits.tolist() == [min(top, 3), 1]
        (hits, _), = b.select(4, -3)
        assert hits[0].tolist() == [[3, 12, 0], [5, 14, 0], [nt - 1, 11, 0], [-1, 0, 0]] and hits[1, 0].tolist() == [nt - 1, 13, 0]
        assert b.check(4, 1, "key 0").tolist() == [0, 0]


def test_duplicates_come_out_by_list_position(engine):
    """Duplicates of one pair whose results a caller made differ (max_pos): each takes a rank, in list order -- in a sort of a few
    items and across the blocks of a streamed segment of 9000 equal keys."""
    pairs = np.array([[0, 5], [0, 2], [0, 5], [0, 5], [0, 2]], np.int64)
    results = np.array([[40, 9, 0], [41, 9, 0], [42, 9, 0], [43, 10, 0], [44, 9, 0]], np.int64)
    b = Bench(engine, pairs, results, 1, 6, max_top=8)
    (hits, nhits), = b.select(8, 0)
    assert nhits.tolist() == [5] and hits[0, :5].tolist() == [[5, 43, 10], [2, 41, 9], [2, 44, 9], [5, 40, 9], [5, 42, 9]]
    rng = np.random.default_rng(3)
    n = 9000
    pairs = np.stack([np.zeros(n, np.int64), np.where(rng.random(n) < 0.5, 17, 4).astype(np.int64)], axis=1)
    results = np.stack([max_pos_of(0, pairs[:, 1], NT, extra=5 * np.arange(n)), np.full(n, 123, np.int64), np.zeros(n, np.int64)], axis=1)
    b = Bench(engine, pairs, results, 1, NT)
    for top in (1, 65, TOP_MAX):
        b.check(top, 100, "9000 duplicates")
    (hits, _), = b.select(TOP_MAX, 0)
    fours = np.nonzero(pairs[:, 1] == 4)[0]
    assert np.array_equal(hits[0, :min(TOP_MAX, len(fours)), 1], results[fours[:TOP_MAX], 0])       # target 4 first, in list order


@pytest.mark.parametrize("pattern", ["four", "random", "equal"])
def test_a_permuted_list_gives_the_same_bytes(engine, pattern):
    rng = np.random.default_rng(41)
    seglens = [65, 4097, 0, 2 * 4096 + 1, 300]
    pairs, results = synthetic_list(rng, seglens, NT, pattern)
    got = []
    for _ in range(3):
        perm = rng.permutation(len(pairs))
        b = Bench(engine, np.ascontiguousarray(pairs[perm]), np.ascontiguousarray(results[perm]), len(seglens), NT)
        got.append(b.select(TOP_MAX, 5)[0])
    assert all(h.tobytes() == got[0][0].tobytes() and n.tobytes() == got[0][1].tobytes() for h, n in got[1:])
    want_hits, want_nhits = numpy_top_pairs(pairs, results, len(seglens), NT, TOP_MAX, 5)
    assert np.array_equal(got[0][0], want_hits) and np.array_equal(got[0][1], want_nhits)


def test_two_runs_into_different_buffers_are_byte_equal(engine):
    rng = np.random.default_rng(9)
    pairs, results = synthetic_list(rng, [4097, 2 * 4096 + 1, 64], NT, "four")
    b = Bench(engine, pairs, results, 3, NT)
    (h0, n0), (h1, n1) = b.select(TOP_MAX, 5, twice=True)
    assert h0.tobytes() == h1.tobytes() and n0.tobytes() == n1.tobytes()
    want_hits, want_nhits = numpy_top_pairs(pairs, results, 3, NT, TOP_MAX, 5)
    assert np.array_equal(h0, want_hits) and np.array_equal(n0, want_nhits)


def test_degenerate_calls(engine):
    t = engine.torch
    none = np.zeros((0, 2), np.int64), np.zeros((0, 3), np.int64)
    b = Bench(engine, *none, 3, 5, max_top=4)                             # an empty list: nhits 0 and the fill pattern
    (hits, nhits), = b.select(4, 0)
    assert nhits.tolist() == [0, 0, 0] and (hits[:, :, 0] == -1).all() and (hits[:, :, 1:] == 0).all()
    assert engine.get_option("last_top_pairs_launches") == 1 and engine.get_option("last_top_pairs_kernel") == 0
    pairs, results = synthetic_list(np.random.default_rng(1), [5, 70], 300, "random")
    b = Bench(engine, pairs, results, 2, 1, max_top=4)                    # one target: only the entries that name target 0 are inside
    b.check(4, 0, "one target")
    dup = np.array([[0, 0], [0, 0], [0, 0]], np.int64), np.array([[1, 4, 0], [2, 5, 0], [3, 4, 0]], np.int64)
    assert Bench(engine, *dup, 1, 1, max_top=4).select(4, 0)[0][0][0].tolist() == [[0, 2, 5], [0, 1, 4], [0, 3, 4], [-1, 0, 0]]
    b = Bench(engine, pairs, results, 2, 0, max_top=4)                    # no target: nothing is inside
    assert b.check(4, 0, "no target").tolist() == [0, 0]
    jp, jr = junk_entries(2, 300)                                         # nothing but entries that drop out
    assert Bench(engine, jp, jr, 2, 300, max_top=4).check(4, 0, "junk").tolist() == [0, 0]
    b = Bench(engine, pairs, results, 2, 300, max_top=4)                  # no query: nothing is launched, nothing is written
    out = (t.full((6,), POISON64, dtype=t.int64, device=b.d_pairs.device), t.full((2,), POISON64, dtype=t.int64, device=b.d_pairs.device))
    hits, nhits = engine.top_hits_pairs_device(b.d_pairs, b.d_results, b.n, 0, 300, 2, out=out)
    engine.synchronize()
    assert hits.shape == (0, 2, 3) and (out[0] == POISON64).all() and (out[1] == POISON64).all()
    assert engine.get_option("last_top_pairs_launches") == 0


def test_errors(engine, swamd):
    L = swamd.lib()
    t = engine.torch
    dev = f"cuda:{engine.device}"
    hits = t.full((2 * 8 * 3,), POISON64, dtype=t.int64, device=dev)
    nhits = t.full((2,), POISON64, dtype=t.int64, device=dev)
    pairs, results = t.zeros(8, dtype=t.int64, device=dev), t.zeros(12, dtype=t.int64, device=dev)

    def select(npairs=4, nq=2, nt=5, top=2, pp=pairs.data_ptr(), rp=results.data_ptr(), hp=hits.data_ptr(), np_=nhits.data_ptr()):
        return L.sw_top_hits_pairs_device(engine._h, pp, rp, npairs, nq, nt, top, 0, hp, np_, None)

    for kw, word in [({"top": 0}, "top"), ({"top": -1}, "top"), ({"top": TOP_MAX + 1}, "top"), ({"npairs": -1}, "npairs"), ({"npairs": 1 << 31}, "npairs"),
                     ({"nq": -1}, "nqueries"), ({"nt": -1}, "ntargets"), ({"nt": 1 << 31}, "ntargets"), ({"hp": None}, "d_hits"), ({"np_": None}, "d_nhits"),
                     ({"pp": None}, "d_pairs"), ({"rp": None}, "d_results")]:
        assert select(**kw) == EINVAL, kw
        msg = L.sw_last_error().decode()
        assert word in msg and "sw_top_hits_pairs_device" in msg, (kw, msg)
    engine.synchronize()
    assert (hits == POISON64).all() and (nhits == POISON64).all()         # an error writes nothing
    with pytest.raises(ValueError):
        engine.top_hits_pairs_device(pairs.view(4, 2), results.view(4, 3), 4, 2, 5, 2, out=(hits[:5], nhits))
    assert select(npairs=0, pp=None, rp=None) == 0                        # no entry: nothing to read
    assert select() == 0                                                  # and the same arguments are fine
    engine.synchronize()
    assert nhits.tolist() == [2, 0]                                       # four entries {0, 0} with score 0


# ---- the chain on the device: filter -> rescoring -> selection -> alignment

QLENS = [257, 1, 513, 4, 255, 256]
TLENS = [0, 1, 63, 64, 65, 127, 300, 700, 64, 0, 1, 300, 65, 127, 63, 90, 17]
QFRONT, FRONT = 4, 3
GO, GE = -11, -1


def pack(lens, front, rng, alpha):
    offs = np.zeros(len(lens) + 1, np.int64)
    offs[0] = front
    offs[1:] = front + np.cumsum(lens)
    return rng.choice(alpha, max(1, int(offs[-1]))).astype(np.uint8), offs


def to_dev(engine, packed, skew):
    t = engine.torch
    buf = t.zeros(len(packed) + skew + 16, dtype=t.uint8, device=f"cuda:{engine.device}")
    buf[skew:skew + len(packed)] = t.from_numpy(packed.copy())
    return buf[skew:skew + len(packed)]


@pytest.fixture(scope="module")
def mixed(engine, swamd):
    """Mixed protein queries (odd base) and targets (offsets[0] > 0) on the device, the handle, the full table of
    Database.search_affine_device and the filter's own scores on the same buffers -- computed once, never changed."""
    rng = np.random.default_rng(2026)
    n = len(PROTEIN)
    sc = rng.integers(-8, 13, (n, n)).astype(np.int8)
    sc[np.arange(n), np.arange(n)] = rng.integers(4, 13, n).astype(np.int8)
    sub = swamd.submat_from_letters(PROTEIN, sc, -8)
    qpacked, qoffs = pack(QLENS, QFRONT, rng, PROTEIN[:20])
    packed, offs = pack(TLENS, FRONT, rng, PROTEIN[:20])
    d_q, d_db = to_dev(engine, qpacked, 1), to_dev(engine, packed, 0)
    db = engine.prepare_db(d_db, offs)
    full = db.search_affine_device(d_q, qoffs, (sub, GO, GE)).cpu().numpy()
    _, _, u = db.prefilter_ungapped_device(d_q, qoffs, sub, 1, 0, want_scores=True)
    u = u.cpu().numpy()
    full.setflags(write=False)
    u.setflags(write=False)
    nz = np.sort(u[u > 0])
    yield {"qpacked": qpacked, "qoffs": qoffs, "packed": packed, "offs": offs, "d_q": d_q, "d_db": d_db, "db": db, "full": full, "u": u,
           "scoring": (sub, GO, GE), "S": int(nz[len(nz) // 2]), "nq": len(QLENS), "nt": len(TLENS)}
    db.close()


def masked_top(m, S, top, min_score):
    """numpy over the full table with the pairs the filter removes taken out (a score no min_score >= 0 lets through)."""
    table = m["full"].copy()
    table[m["u"] < S] = (0, -1, 0)
    return numpy_top(table, top, max(0, min_score))


def guarded_out(engine, nq, top):
    t = engine.torch
    arena = Arena(t, f"cuda:{engine.device}", arena_bytes(max(1, nq) * top * 24, max(1, nq) * 8))
    ch, cn = arena.carve(nq * top * 24, 16, 8, name="hits"), arena.carve(nq * 8, 16, 8, name="nhits")
    return arena, (arena.view(ch, t.int64, (nq * top * 3,)), arena.view(cn, t.int64, (nq,)))


def hand_chain(engine, m, S, cap, top, min_score):
    """The three calls enqueued back to back, nothing read in between: torch (hits, nhits, npairs, arena)."""
    db, d_q, qoffs = m["db"], m["d_q"], m["qoffs"]
    pairs, npairs, _ = db.prefilter_ungapped_device(d_q, qoffs, m["scoring"][0], S, cap)
    res = db.search_affine_pairs_device(d_q, qoffs, m["scoring"], pairs)                      # all cap entries
    arena, out = guarded_out(engine, m["nq"], top)
    hits, nhits = engine.top_hits_pairs_device(pairs, res, cap, m["nq"], m["nt"], top, min_score, out=out)
    return hits, nhits, npairs, arena


@pytest.mark.parametrize("top", [1, 3, 10, len(TLENS) + 5])
def test_chain_on_the_device_equals_numpy_over_the_masked_table(engine, mixed, top):
    m = mixed
    S, cap = m["S"], m["nq"] * m["nt"]
    count = int((m["u"] >= S).sum())
    assert 0 < count < (m["u"] > 0).sum()
    occurs = int(np.sort(m["full"][:, :, 1].reshape(-1))[m["full"][:, :, 1].size // 2])
    for min_score in (0, occurs, int(m["full"][:, :, 1].max()) + 1):
        hits, nhits, npairs, arena = hand_chain(engine, m, S, cap, top, min_score)
        engine.synchronize()
        assert_guards(arena)
        want_hits, want_nhits = masked_top(m, S, top, min_score)
        assert int(npairs.item()) == count
        assert np.array_equal(nhits.cpu().numpy(), want_nhits) and np.array_equal(hits.cpu().numpy(), want_hits), (top, min_score)


def test_alignment_of_the_chains_table_agrees_with_the_host_leg(engine, swamd, mixed):
    m = mixed
    top, cap = 4, m["nq"] * m["nt"]
    hits, nhits, _, _ = hand_chain(engine, m, m["S"], cap, top, 1)
    ops_cap = max(QLENS) + max(TLENS)
    aln, ops = m["db"].align_affine_hits_device(m["d_q"], m["qoffs"], m["scoring"], hits, nhits, ops_cap=ops_cap)
    engine.synchronize()
    aln, ops, h, n = aln.cpu().numpy(), ops.cpu().numpy(), hits.cpu().numpy(), nhits.cpu().numpy()
    want_aln, want_ops = swamd.align_affine_hits_host((m["qpacked"], m["qoffs"]), (m["packed"], m["offs"]), m["scoring"], h, n)
    assert np.array_equal(aln, want_aln) and n.sum() > m["nq"]
    for q in range(m["nq"]):
        for r in range(top):
            assert ops[q, r, :aln[q, r, 6]].tobytes() == want_ops[q][r], (q, r)
            if r < n[q]:
                assert aln[q, r, 0] == h[q, r, 1] and aln[q, r, 1] == h[q, r, 2]                # the alignment ends where the search said


@pytest.mark.parametrize("top,min_score", [(1, 0), (5, 1), (len(TLENS) + 5, 0)])
def test_one_call_equals_the_hand_chain(engine, mixed, top, min_score):
    m = mixed
    S, cap = m["S"], m["nq"] * m["nt"]
    h0, n0, c0, _ = hand_chain(engine, m, S, cap, top, min_score)
    arena, out = guarded_out(engine, m["nq"], top)
    h1, n1, c1 = m["db"].search_affine_top_prefiltered_device(m["d_q"], m["qoffs"], m["scoring"], S, cap, top, min_score, out=out)
    engine.synchronize()
    assert_guards(arena)
    assert h0.cpu().numpy().tobytes() == h1.cpu().numpy().tobytes() and n0.cpu().numpy().tobytes() == n1.cpu().numpy().tobytes()
    assert int(c0.item()) == int(c1.item()) == int((m["u"] >= S).sum())
    want_hits, want_nhits = masked_top(m, S, top, min_score)
    assert np.array_equal(h1.cpu().numpy(), want_hits) and np.array_equal(n1.cpu().numpy(), want_nhits)
    hn, nn, cn = m["db"].search_affine_top_prefiltered((m["qpacked"], m["qoffs"]), m["scoring"], S, top, min_score)     # the numpy wrapper
    assert isinstance(hn, np.ndarray) and np.array_equal(hn, want_hits) and np.array_equal(nn, want_nhits) and cn == int(c1.item())


@pytest.mark.parametrize("top", [1, 4, len(TLENS)])
def test_threshold_one_equals_the_unfiltered_search_byte_for_byte(engine, mixed, top):
    m = mixed
    hits, nhits, _ = m["db"].search_affine_top_prefiltered_device(m["d_q"], m["qoffs"], m["scoring"], 1, m["nq"] * m["nt"], top, 1)
    want_hits, want_nhits = m["db"].search_affine_top_device(m["d_q"], m["qoffs"], m["scoring"], top, 1)
    engine.synchronize()
    assert hits.cpu().numpy().tobytes() == want_hits.cpu().numpy().tobytes() and nhits.cpu().numpy().tobytes() == want_nhits.cpu().numpy().tobytes()
    assert int(want_nhits.min()) == min(top, int((m["full"][:, :, 1] >= 1).sum(axis=1).min())) > 0     # every query has such hits


def test_a_cap_below_the_count(engine, swamd, mixed):
    """The count is the true one; the table is built from the pairs the list kept: each hit a passing pair with the full table's
    result, every row in rank order."""
    m = mixed
    S, top = m["S"], 6
    count = int((m["u"] >= S).sum())
    cap = count // 2
    arena, out = guarded_out(engine, m["nq"], top)
    hits, nhits, npairs = m["db"].search_affine_top_prefiltered_device(m["d_q"], m["qoffs"], m["scoring"], S, cap, top, 0, out=out)
    engine.synchronize()
    assert_guards(arena)
    hits, nhits = hits.cpu().numpy(), nhits.cpu().numpy()
    assert int(npairs.item()) == count > cap and 0 < int(nhits.sum()) <= cap
    for q in range(m["nq"]):
        row = hits[q, :nhits[q]]
        for target, pos, score in row:
            assert m["u"][q, target] >= S and (m["full"][q, target, 0], m["full"][q, target, 1]) == (pos, score)
        keys = [(-int(s), int(k)) for k, _, s in row]
        assert keys == sorted(keys) and len(set(keys)) == len(keys)
        assert (hits[q, nhits[q]:, 0] == -1).all() and (hits[q, nhits[q]:, 1:] == 0).all()
    with pytest.raises(swamd.SwError):
        m["db"].search_affine_top_prefiltered((m["qpacked"], m["qoffs"]), m["scoring"], S, top, 0, cap=cap)


def test_a_cap_beyond_search_results_mib_is_refused_before_anything_is_launched(engine, swamd, mixed):
    m = mixed
    L = swamd.lib()
    t = engine.torch
    sub, sc = swamd._affine(*m["scoring"])
    hits = t.full((m["nq"] * 2 * 3,), POISON64, dtype=t.int64, device=m["d_q"].device)
    nhits = t.full((m["nq"],), POISON64, dtype=t.int64, device=m["d_q"].device)
    npairs = t.full((1,), POISON64, dtype=t.int64, device=m["d_q"].device)

    def call(cap=10, S=1, top=2, hp=hits.data_ptr(), np_=nhits.data_ptr(), cp=npairs.data_ptr(), scoring=sc):
        return L.sw_db_search_affine_top_prefiltered(engine._h, m["db"]._h, m["d_q"].data_ptr(), m["qoffs"].ctypes.data, m["nq"], ctypes.byref(scoring), S, cap,
                                                     top, 0, hp, np_, cp, None)

    assert engine.get_option("search_results_mib") == 1024
    engine.set_option("search_results_mib", 1)
    try:
        fits = (1 << 20) // 56
        assert call(cap=fits + 1) == EINVAL
        msg = L.sw_last_error().decode()
        assert "search_results_mib" in msg and "sw_db_search_affine_top_prefiltered" in msg
        engine.synchronize()
        assert (hits == POISON64).all() and (nhits == POISON64).all() and (npairs == POISON64).all()
        assert call(cap=fits) == 0
        engine.synchronize()
        assert int(npairs.item()) == int((m["u"] >= 1).sum()) and (nhits != POISON64).all()
    finally:
        engine.set_option("search_results_mib", 1024)
    hits.fill_(POISON64), nhits.fill_(POISON64), npairs.fill_(POISON64)
    bad = swamd._affine(m["scoring"][0], 1, -1)[1]
    for kw in ({"S": 0}, {"cap": -1}, {"cap": 1 << 31}, {"top": 0}, {"top": TOP_MAX + 1}, {"hp": None}, {"np_": None}, {"cp": None}, {"scoring": bad}):
        assert call(**kw) == EINVAL, kw
    engine.synchronize()
    assert (hits == POISON64).all() and (nhits == POISON64).all() and (npairs == POISON64).all()       # an error writes nothing
