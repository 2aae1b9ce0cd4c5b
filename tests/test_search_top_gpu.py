"""GPU: the best targets per query selected on the device (sw_top_hits_device, sw_db_search_affine_top; csrc/sw_search_top.hip).
The selection alone runs on synthetic tables uploaded from numpy -- no search at all -- and is compared exactly with numpy's lexsort
(tests/top_cases.py); search + selection is compared with numpy over the full table of Database.search_affine_device on the same
buffers, and with the host leg.  Outputs lie in a poisoned arena between guards: every entry must be written, nothing else."""
import ctypes

import numpy as np
import pytest

from affine_cases import PROTEIN
from buffer_cases import POISON64, Arena, arena_bytes, assert_guards
from top_cases import SCORE_MAX, numpy_top, table_of

pytestmark = pytest.mark.gpu
EINVAL = -22
TOP_MAX = 4096
PATTERNS = ["equal", "zero", "ascending", "descending", "four", "edges", "random"]


def scores_of(pattern, nq, nt, rng):
    k = np.arange(nt, dtype=np.int64)
    if pattern == "equal":
        return np.full((nq, nt), 37, np.int64)                       # the hits are the lowest indices
    if pattern == "zero":
        return np.zeros((nq, nt), np.int64)
    if pattern == "ascending":
        return np.stack([k + q for q in range(nq)])                  # strictly: the hits are the LAST targets
    if pattern == "descending":
        return np.stack([nt - k + q for q in range(nq)])
    if pattern == "four":
        return rng.choice(np.array([0, 7, 8, 100], np.int64), (nq, nt))   # long tie runs across every slice boundary
    if pattern == "edges":
        return rng.choice(np.array([0, SCORE_MAX], np.int64), (nq, nt))   # the ends of the key's score field
    return rng.integers(0, 200, (nq, nt)).astype(np.int64)


class Bench:
    """The table in one arena (an input: it must stay as it is), the outputs in another that is poisoned anew for every call."""

    def __init__(self, engine, table):
        t = engine.torch
        self.engine, self.table = engine, table
        self.nq, self.nt = table.shape[:2]
        raw = table.reshape(-1).view(np.uint8)
        self.ain = Arena(t, f"cuda:{engine.device}", arena_bytes(len(raw)))
        self.d_table, _ = self.ain.place(raw, align=16, skew=8, name="table")    # an sw_result needs 8 bytes of alignment, no more
        self.aout = Arena(t, f"cuda:{engine.device}", 2 * arena_bytes(self.nq * TOP_MAX * 24, self.nq * 8))

    def outputs(self, top):
        t = self.engine.torch
        ch = self.aout.carve(self.nq * top * 24, 16, 8, name=f"hits{len(self.aout.carves)}")
        cn = self.aout.carve(self.nq * 8, 16, 8, name=f"nhits{len(self.aout.carves)}")
        return self.aout.view(ch, t.int64, (self.nq * top * 3,)), self.aout.view(cn, t.int64, (self.nq,))

    def select(self, top, min_score, twice=False):
        self.aout.reset()
        outs = [self.outputs(top) for _ in range(2 if twice else 1)]
        got = [self.engine.top_hits_device(self.d_table, self.nq, self.nt, top, min_score, out=o) for o in outs]
        self.engine.synchronize()
        assert_guards(self.aout)
        assert_guards(self.ain)
        return [(h.cpu().numpy(), n.cpu().numpy()) for h, n in got]

    def check(self, top, min_score, what):
        (hits, nhits), = self.select(top, min_score)
        want_hits, want_nhits = numpy_top(self.table, top, min_score)
        assert np.array_equal(nhits, want_nhits), f"{what} top {top} min_score {min_score}: nhits {nhits.tolist()} vs {want_nhits.tolist()}"
        bad = np.argwhere((hits != want_hits).any(axis=2))
        assert len(bad) == 0, (f"{what} top {top} min_score {min_score}: {len(bad)} hits differ, first (query, rank) {tuple(bad[0])}: "
                               f"{hits[tuple(bad[0])]} vs {want_hits[tuple(bad[0])]}")
        return nhits


def occurring(table):
    """A score in the middle of the table's distribution and the largest one."""
    s = np.sort(table[:, :, 1].reshape(-1))
    return int(s[len(s) // 2]), int(s[-1])


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("nt", [1, 2, 63, 64, 65, 257, 4097])
def test_selection_alone_small_rows(engine, nt, pattern):
    """Up to 4096 targets one workgroup sorts the row whole; 4097 is the first length that goes through the radix select."""
    rng = np.random.default_rng(nt)
    for nq in (1, 5):
        b = Bench(engine, table_of(scores_of(pattern, nq, nt, rng)))
        mid, hi = occurring(b.table)
        tops = sorted({1, 2, 64, 65, TOP_MAX, min(TOP_MAX, nt + 3)})
        for top in tops:
            for min_score in (0, mid, mid + 1, hi + 1):                 # exactly at a tie run, just above it, above the maximum
                nhits = b.check(top, min_score, f"{pattern} {nq} x {nt}")
                if min_score == hi + 1:
                    assert (nhits == 0).all()
        assert engine.get_option("last_search_top_kernel") == (1 if nt > TOP_MAX else 0)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_selection_alone_several_workgroups_per_row(engine, pattern):
    """300 000 targets: 74 workgroups per row with one row, 5 rows at once; the cut falls inside tie runs that span the slices."""
    rng = np.random.default_rng(len(pattern))
    nt = 300000
    for nq in ((1, 5) if pattern == "four" else (5,)):
        b = Bench(engine, table_of(scores_of(pattern, nq, nt, rng)))
        mid, hi = occurring(b.table)
        for top, min_score in [(1, 0), (65, 0), (TOP_MAX, 0), (TOP_MAX, mid), (64, mid + 1), (2, hi), (TOP_MAX, hi + 1)]:
            b.check(top, min_score, f"{pattern} {nq} x {nt}")
        assert engine.get_option("last_search_top_kernel") == 1 and engine.get_option("last_search_top_chunks") == 1


def test_few_qualify_in_a_long_row(engine):
    """Fewer targets qualify than `top`, scattered over the slices of a long row: every one is a hit, the tail is the fill pattern."""
    rng = np.random.default_rng(77)
    scores = rng.integers(0, 50, (3, 100000)).astype(np.int64)
    scores[0, rng.choice(100000, 37, replace=False)] = 900
    scores[2, [0, 4095, 4096, 99999]] = 901
    b = Bench(engine, table_of(scores))
    assert b.check(100, 900, "scattered").tolist() == [37, 0, 4]
    assert b.check(3, 900, "scattered").tolist() == [3, 0, 3]
    assert b.check(TOP_MAX, 45, "scattered").tolist() == [TOP_MAX, TOP_MAX, TOP_MAX]      # about 10 000 of a row qualify


def test_two_runs_into_different_buffers_are_byte_equal(engine):
    rng = np.random.default_rng(9)
    b = Bench(engine, table_of(scores_of("four", 5, 300000, rng)))
    (h0, n0), (h1, n1) = b.select(TOP_MAX, 7, twice=True)
    assert h0.tobytes() == h1.tobytes() and n0.tobytes() == n1.tobytes()
    want_hits, want_nhits = numpy_top(b.table, TOP_MAX, 7)
    assert np.array_equal(h0, want_hits) and np.array_equal(n0, want_nhits)


# ---- search + selection through a prepared handle

QLENS = [257, 1, 513, 4, 1025, 255, 256]
TLENS = [0, 1, 63, 64, 65, 127, 300, 1100, 64, 0, 1, 300, 65, 127, 63]
QFRONT, FRONT = 4, 3


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


def search_top(engine, db, d_q, qoffs, scoring, top, min_score=0):
    """Database.search_affine_top_device into poisoned, guarded outputs: numpy (hits, nhits)."""
    t = engine.torch
    nq = len(qoffs) - 1
    arena = Arena(t, f"cuda:{engine.device}", arena_bytes(max(1, nq) * top * 24, max(1, nq) * 8))
    ch, cn = arena.carve(nq * top * 24, 16, 8, name="hits"), arena.carve(nq * 8, 16, 8, name="nhits")
    out = (arena.view(ch, t.int64, (nq * top * 3,)), arena.view(cn, t.int64, (nq,)))
    hits, nhits = db.search_affine_top_device(d_q, qoffs, scoring, top, min_score, out=out)
    engine.synchronize()
    assert_guards(arena)
    return hits.cpu().numpy(), nhits.cpu().numpy()


@pytest.fixture(scope="module")
def scorings(swamd):
    rng = np.random.default_rng(5)
    n = len(PROTEIN)
    sc = rng.integers(-8, 13, (n, n)).astype(np.int8)
    sc[np.arange(n), np.arange(n)] = rng.integers(4, 13, n).astype(np.int8)
    return {"affine": (swamd.submat_from_letters(PROTEIN, sc, -8), -11, -1), "linear": (swamd.submat_match(3, -3), 0, -2)}


@pytest.fixture(scope="module")
def mixed(engine, scorings):
    """Mixed queries (odd base) and targets (offsets[0] > 0) on the device, the handle, and per scoring the full table of
    Database.search_affine_device on the same buffers -- computed once, never changed."""
    rng = np.random.default_rng(2025)
    qpacked, qoffs = pack(QLENS, QFRONT, rng, PROTEIN[:20])
    packed, offs = pack(TLENS, FRONT, rng, PROTEIN[:20])
    d_q, d_db = to_dev(engine, qpacked, 1), to_dev(engine, packed, 0)
    assert (d_q.data_ptr() + QFRONT) % 2 == 1
    db = engine.prepare_db(d_db, offs)
    full = {}
    for k, s in scorings.items():
        full[k] = db.search_affine_device(d_q, qoffs, s).cpu().numpy()
        full[k].setflags(write=False)
    yield {"qpacked": qpacked, "qoffs": qoffs, "packed": packed, "offs": offs, "d_q": d_q, "d_db": d_db, "db": db, "full": full}
    db.close()


@pytest.mark.parametrize("which", ["affine", "linear"])
def test_mixed_queries_equal_numpy_over_the_full_table_and_the_host_leg(engine, swamd, mixed, scorings, which):
    table = mixed["full"][which]
    mid, hi = occurring(table)
    assert (table[:, :, 1] > 0).sum() > len(QLENS) * 8
    for top in (1, 3, 10, len(TLENS), len(TLENS) + 5):
        for min_score in (0, mid, hi + 1):
            hits, nhits = search_top(engine, mixed["db"], mixed["d_q"], mixed["qoffs"], scorings[which], top, min_score)
            want_hits, want_nhits = numpy_top(table, top, min_score)
            assert np.array_equal(nhits, want_nhits) and np.array_equal(hits, want_hits), (top, min_score)
            host_hits, host_nhits = swamd.search_affine_multi_top_host((mixed["qpacked"], mixed["qoffs"]), (mixed["packed"], mixed["offs"]), scorings[which],
                                                                       top, min_score)
            assert np.array_equal(nhits, host_nhits) and np.array_equal(hits, host_hits), (top, min_score, "host leg")
    assert engine.get_option("last_search_top_chunks") == 1 and engine.get_option("last_search_top_kernel") == 0


def test_numpy_wrapper_and_one_query(engine, mixed, scorings):
    queries = (mixed["qpacked"], mixed["qoffs"])
    hits, nhits = mixed["db"].search_affine_top(queries, scorings["affine"], 10)
    want_hits, want_nhits = numpy_top(mixed["full"]["affine"], 10)
    assert isinstance(hits, np.ndarray) and hits.shape == (len(QLENS), 10, 3) and np.array_equal(hits, want_hits) and np.array_equal(nhits, want_nhits)
    hits, nhits = search_top(engine, mixed["db"], mixed["d_q"], mixed["qoffs"][2:4], scorings["affine"], 10)
    assert np.array_equal(hits, want_hits[2:3]) and nhits.tolist() == [10]


@pytest.mark.parametrize("copies", [400, 1000])
def test_duplicate_targets_tie_across_the_cut(engine, scorings, copies):
    """Copies of 5 distinct short targets: real searches whose scores tie `copies` times; the cut of top = 10 lies inside a tie run.
    400 copies are sorted whole (2000 targets), 1000 go through the radix select."""
    rng = np.random.default_rng(copies)
    five = [rng.choice(PROTEIN[:20], n).astype(np.uint8) for n in (12, 30, 21, 30, 9)]
    order = rng.permutation(np.repeat(np.arange(5), copies))
    packed = np.concatenate([five[k] for k in order])
    offs = np.concatenate([[0], np.cumsum([len(five[k]) for k in order])]).astype(np.int64)
    queries = [five[1][3:25], five[3][:20], rng.choice(PROTEIN[:20], 16).astype(np.uint8)]
    qpacked, qoffs = np.concatenate(queries), np.concatenate([[0], np.cumsum([len(q) for q in queries])]).astype(np.int64)
    d_q, d_db = to_dev(engine, qpacked, 1), to_dev(engine, packed, 0)
    with engine.prepare_db(d_db, offs) as db:
        table = db.search_affine_device(d_q, qoffs, scorings["affine"]).cpu().numpy()
        assert len(np.unique(table[0, :, 1])) <= 5
        for top, min_score in [(10, 0), (10, int(table[0, :, 1].max())), (copies + 7, 0), (TOP_MAX, int(np.median(table[1, :, 1])))]:
            hits, nhits = search_top(engine, db, d_q, qoffs, scorings["affine"], top, min_score)
            want_hits, want_nhits = numpy_top(table, top, min_score)
            assert np.array_equal(nhits, want_nhits) and np.array_equal(hits, want_hits), (top, min_score)
        assert engine.get_option("last_search_top_kernel") == (1 if 5 * copies > TOP_MAX else 0)
    top10 = numpy_top(table, 10)[0]
    assert (top10[0, :, 2] == top10[0, 0, 2]).all() and (np.diff(top10[0, :, 0]) > 0).all()   # ten equal scores: the lowest ten of the copies


@pytest.mark.parametrize("ntargets,nq,chunks", [(20000, 10, 5), (50000, 3, 3)])
def test_chunks_under_a_budget_of_one_mib(engine, scorings, ntargets, nq, chunks):
    """1 MiB holds 43 690 results: two rows of 20 000, not one of 50 000 -- which is then a chunk of its own."""
    rng = np.random.default_rng(ntargets)
    packed, offs = pack(list(rng.integers(8, 25, ntargets)), FRONT, rng, PROTEIN[:20])
    qpacked, qoffs = pack([16] * nq, QFRONT, rng, PROTEIN[:20])
    d_q, d_db = to_dev(engine, qpacked, 1), to_dev(engine, packed, 0)
    with engine.prepare_db(d_db, offs) as db:
        table = db.search_affine_device(d_q, qoffs, scorings["affine"]).cpu().numpy()
        want_hits, want_nhits = numpy_top(table, 100, 3)
        whole_hits, whole_nhits = search_top(engine, db, d_q, qoffs, scorings["affine"], 100, 3)
        assert engine.get_option("last_search_top_chunks") == 1 and engine.get_option("search_results_mib") == 1024
        engine.set_option("search_results_mib", 1)
        try:
            hits, nhits = search_top(engine, db, d_q, qoffs, scorings["affine"], 100, 3)
            assert engine.get_option("last_search_top_chunks") == chunks and engine.get_option("last_search_top_kernel") == 1
        finally:
            engine.set_option("search_results_mib", 1024)
    assert np.array_equal(hits, whole_hits) and np.array_equal(nhits, whole_nhits)
    assert np.array_equal(hits, want_hits) and np.array_equal(nhits, want_nhits)


def test_degenerate_handles(engine, scorings):
    rng = np.random.default_rng(1)
    qpacked, qoffs = pack([5, 40], 0, rng, PROTEIN[:20])
    d_q = to_dev(engine, qpacked, 1)
    d_db = to_dev(engine, np.full(16, 65, np.uint8), 0)
    with engine.prepare_db(d_db, np.zeros(1, np.int64)) as db:            # no target: nhits 0 and the fill pattern
        hits, nhits = search_top(engine, db, d_q, qoffs, scorings["affine"], 4)
        assert nhits.tolist() == [0, 0] and (hits[:, :, 0] == -1).all() and (hits[:, :, 1:] == 0).all()
    with engine.prepare_db(d_db, np.full(6, 2, np.int64)) as db:         # five empty targets: they qualify at min_score <= 0 only
        hits, nhits = search_top(engine, db, d_q, qoffs, scorings["affine"], 7)
        assert nhits.tolist() == [5, 5] and hits[0, :, 0].tolist() == [0, 1, 2, 3, 4, -1, -1] and (hits[:, :, 1:] == 0).all()
        hits, nhits = search_top(engine, db, d_q, qoffs, scorings["affine"], 7, min_score=1)
        assert nhits.tolist() == [0, 0] and (hits[:, :, 0] == -1).all()
        t = engine.torch                                                  # no query: nothing is launched, nothing is written
        out = (t.full((6,), POISON64, dtype=t.int64, device=d_q.device), t.full((2,), POISON64, dtype=t.int64, device=d_q.device))
        hits, nhits = db.search_affine_top_device(d_q, np.zeros(1, np.int64), scorings["affine"], 2, out=out)
        engine.synchronize()
        assert hits.shape == (0, 2, 3) and (out[0] == POISON64).all() and (out[1] == POISON64).all()


def test_errors(engine, swamd, mixed, scorings):
    L = swamd.lib()
    t = engine.torch
    db, d_q, qoffs = mixed["db"], mixed["d_q"], mixed["qoffs"]
    sub, sc = swamd._affine(*scorings["affine"])
    hits = t.full((len(QLENS) * 8 * 3,), POISON64, dtype=t.int64, device=d_q.device)
    nhits = t.full((len(QLENS),), POISON64, dtype=t.int64, device=d_q.device)
    table = t.zeros(30, dtype=t.int64, device=d_q.device)

    def search(top=2, hp=hits.data_ptr(), np_=nhits.data_ptr(), nq=len(QLENS)):
        return L.sw_db_search_affine_top(engine._h, db._h, d_q.data_ptr(), qoffs.ctypes.data, nq, ctypes.byref(sc), top, 0, hp, np_, None)

    def select(top=2, hp=hits.data_ptr(), np_=nhits.data_ptr(), nq=2, nt=5, tp=table.data_ptr()):
        return L.sw_top_hits_device(engine._h, tp, nq, nt, top, 0, hp, np_, None)

    for call in (search, select):
        for top in (0, -1, TOP_MAX + 1):
            assert call(top=top) == EINVAL and "top" in L.sw_last_error().decode(), (call.__name__, top)
        assert call(hp=None) == EINVAL and call(np_=None) == EINVAL
        assert call(nq=-1) == EINVAL
    assert select(nt=-1) == EINVAL and select(nt=1 << 31) == EINVAL and select(tp=None) == EINVAL
    assert L.sw_db_search_affine_top(engine._h, None, d_q.data_ptr(), qoffs.ctypes.data, 1, ctypes.byref(sc), 2, 0, hits.data_ptr(), nhits.data_ptr(), None) == EINVAL
    bad = swamd._affine(scorings["affine"][0], 1, -1)[1]                   # the scoring errors of sw_db_search_affine
    assert L.sw_db_search_affine_top(engine._h, db._h, d_q.data_ptr(), qoffs.ctypes.data, 1, ctypes.byref(bad), 2, 0, hits.data_ptr(), nhits.data_ptr(), None) == EINVAL
    engine.synchronize()
    assert (hits == POISON64).all() and (nhits == POISON64).all()         # an error writes nothing
    with pytest.raises(ValueError):
        engine.top_hits_device(table, 2, 5, 2, out=(hits[:5], nhits))
    assert swamd.SW_TOP_MAX == TOP_MAX
    assert search(top=2) == 0 and select(top=2) == 0                      # and the same arguments are fine once `top` is
    engine.synchronize()
