"""GPU: queries that are position-specific scoring matrices (sw_db_search_pssm, sw_db_search_pssm_top, sw_db_align_pssm_hits) against
the independent checker (tests/pssm_cases.py says how it expresses a PSSM), against the sequence calls on derived matrices, and at the
edges of the contract: every class of query length in one call, qoffsets[0] > 0, a matrix at an odd address between 127s, 1..256 letters,
several groups, several chunks, checkpointed alignments, the 24-bit bound from both sides.  Equality is exact everywhere; every output
is carved out of a poisoned arena (tests/buffer_cases.py) and the guards are checked."""
import numpy as np
import pytest

import align_cases
import pssm_cases
from affine_cases import GAPS, PROTEIN, assert_same, checker, random_submat  # noqa: F401
from buffer_cases import POISON, POISON64, Arena, arena_bytes, assert_guards

pytestmark = pytest.mark.gpu

OTHER, SMAX = -3, 9                # entries are drawn from -8..12: the clamp is at work in every case
PAD = 4096                         # bytes of 127 in front of and behind the matrix


def _dev(engine):
    return f"cuda:{engine.device}"


@pytest.fixture(scope="module")
def dbase(engine):
    """The database of the affine tests and its handle, shared by every case."""
    rng = np.random.default_rng(77)
    packed, offs = pssm_cases.small_database(rng, PROTEIN)
    with engine.prepare_db((packed, offs)) as db:
        yield packed, offs, db


_worlds = {}


def world(checker, dbase, nletters):  # noqa: F811
    """One matrix per number of letters, its gap pair and the checker's table for it: computed once, shared, never changed."""
    if nletters not in _worlds:
        packed, offs, _ = dbase
        rng = np.random.default_rng(1000 + nletters)
        ty = pssm_cases.Typed(rng, pssm_cases.letters_of(rng, nletters), OTHER, SMAX, pssm_cases.QLENS)
        go, ge = GAPS[pssm_cases.NLETTERS.index(nletters) % len(GAPS)]
        _worlds[nletters] = (ty, go, ge, ty.expected(checker, packed, offs, go, ge))
    return _worlds[nletters]


def place_matrix(engine, ty):
    """The matrix in an arena of its own at an ODD address, 127s in front of it, behind it and in the unused columns before
    qoffsets[0]; all of it must stay as it is.  Returns (arena, int8 tensor that starts at column 0)."""
    t = engine.torch
    m = ty.matrix.copy()
    m[:ty.qoffs[0]] = 127
    inp = Arena(t, _dev(engine), arena_bytes(m.size + 2 * PAD))
    d, _ = inp.place(m.view(np.uint8).reshape(-1), align=64, skew=1, front=np.full(PAD, 127, np.uint8), back=np.full(PAD, 127, np.uint8), name="pssm")
    assert d.data_ptr() % 2 == 1
    return inp, d.view(t.int8)


def carve_i64(arena, n, name):
    c = arena.carve(n * 8, align=8, name=name)
    return arena.view(c, arena.torch.int64, (n,))


@pytest.mark.parametrize("nletters", pssm_cases.NLETTERS)
def test_search_equals_the_checker(engine, checker, dbase, nletters):  # noqa: F811
    packed, offs, db = dbase
    ty, go, ge, exp = world(checker, dbase, nletters)
    nq, nt = exp.shape[:2]
    inp, d_pssm = place_matrix(engine, ty)
    out = Arena(engine.torch, _dev(engine), arena_bytes(nq * nt * 24))
    res = db.search_pssm_device(d_pssm, ty.qoffs, ty.scoring(go, ge), out=carve_i64(out, nq * nt * 3, "results"))
    engine.synchronize()
    got = res.cpu().numpy()
    for q in range(nq):
        assert_same(got[q], exp[q], f"nletters {nletters}, query {q} of {pssm_cases.QLENS[q]} columns")
    assert engine.get_option("last_search_multi_groups") == 1 and engine.get_option("last_search_multi_launches") >= 3   # every class has queries
    assert_guards(out)
    assert_guards(inp)
    # several groups: the same bytes
    try:
        engine.set_option("search_profile_mib", 1)
        out.reset()
        res = db.search_pssm_device(d_pssm, ty.qoffs, ty.scoring(go, ge), out=carve_i64(out, nq * nt * 3, "results"))
        engine.synchronize()
        assert np.array_equal(res.cpu().numpy(), got)
        assert engine.get_option("last_search_multi_groups") > 1
        assert_guards(out)
        assert_guards(inp)
    finally:
        engine.set_option("search_profile_mib", 256)


@pytest.mark.parametrize("nletters", pssm_cases.NLETTERS)
def test_derived_matrices_equal_the_sequence_search_byte_for_byte(engine, swamd, nletters):
    """sw_pssm_from_queries, then sw_db_search_pssm: the bytes of sw_db_search_affine.  The targets are drawn from the letters, so no
    byte is `other`; smax = 127 clamps nothing."""
    t = engine.torch
    rng = np.random.default_rng(2000 + nletters)
    letters = pssm_cases.letters_of(rng, nletters)
    packed, offs = pssm_cases.small_database(rng, letters, budget=1e6)
    qoffs = np.concatenate([[pssm_cases.QFRONT], pssm_cases.QFRONT + np.cumsum(pssm_cases.QLENS)]).astype(np.int64)
    qpacked = rng.choice(letters, int(qoffs[-1])).astype(np.uint8)
    sub = random_submat(rng)
    go, ge = GAPS[(pssm_cases.NLETTERS.index(nletters) + 1) % len(GAPS)]
    m, moffs = swamd.pssm_from_queries((qpacked, qoffs), sub, letters)
    assert moffs[0] == 0 and m.shape == (sum(pssm_cases.QLENS), nletters)
    with engine.prepare_db((packed, offs)) as db:
        a = db.search_affine_device(t.from_numpy(qpacked.copy()).to(_dev(engine)), qoffs, (sub, go, ge))
        b = db.search_pssm_device(t.from_numpy(m.reshape(-1).copy()).to(_dev(engine)), moffs, (letters, -128, 127, go, ge))
        engine.synchronize()
        assert t.equal(a, b) and int(a[:, :, 1].max()) > 0


def test_top_equals_the_rank_order_of_the_full_table(engine, checker):  # noqa: F811
    """4000 short targets: 12 rows of 96 000 bytes exceed search_results_mib = 1, so the call runs in chunks."""
    t = engine.torch
    rng = np.random.default_rng(31)
    lens = rng.integers(0, 41, 4000)
    offs = np.concatenate([[5], 5 + np.cumsum(lens)]).astype(np.int64)
    packed = rng.choice(PROTEIN, int(offs[-1])).astype(np.uint8)
    ty = pssm_cases.Typed(rng, PROTEIN, OTHER, SMAX, pssm_cases.QLENS)
    go, ge = GAPS[0]
    nq, nt, top = len(pssm_cases.QLENS), 4000, 7
    inp, d_pssm = place_matrix(engine, ty)
    with engine.prepare_db((packed, offs)) as db:
        full = db.search_pssm_device(d_pssm, ty.qoffs, ty.scoring(go, ge)).cpu().numpy()
        for q in (0, 1, 2):                                        # the full table is the checker's (the short queries: cheap)
            assert_same(full[q], checker.search(ty.query(q), packed, offs, ty.table, go, ge), f"query {q}")
        for min_score, mib in ((0, 1), (25, 1), (25, 1024)):
            want_hits, want_n = pssm_cases.rank_order(full, top, min_score)
            out = Arena(t, _dev(engine), arena_bytes(nq * top * 24, nq * 8))
            o = (carve_i64(out, nq * top * 3, "hits"), carve_i64(out, nq, "nhits"))
            try:
                engine.set_option("search_results_mib", mib)
                hits, nhits = db.search_pssm_top_device(d_pssm, ty.qoffs, ty.scoring(go, ge), top, min_score, out=o)
                engine.synchronize()
                assert (engine.get_option("last_search_top_chunks") > 1) == (mib == 1)
            finally:
                engine.set_option("search_results_mib", 1024)
            assert np.array_equal(hits.cpu().numpy(), want_hits) and np.array_equal(nhits.cpu().numpy(), want_n), (min_score, mib)
            assert_guards(out)
        assert_guards(inp)
        assert pssm_cases.rank_order(full, top, 25)[1].tolist() == [0] + [top] * (nq - 1)      # one column scores 9 at the most


TOP = 2
_aligned = {}


def expected_alignments(checker, dbase):  # noqa: F811
    """The two best targets of every query of the 24-letter matrix, by the checker's scores, and their canonical alignments."""
    if not _aligned:
        packed, offs, _ = dbase
        ty, go, ge, exp = world(checker, dbase, 24)
        table, _ = pssm_cases.rank_order(exp, TOP, 0)
        table[5, 1, 0] = len(offs) - 1 + 3                         # an entry outside the database
        ref = {}
        for q in range(len(exp)):
            for r in range(TOP):
                k = int(table[q, r, 0])
                if 0 <= k < len(offs) - 1:
                    target = packed[offs[k]:offs[k + 1]]
                    row, ops, _ = align_cases.expected(checker, ty.query(q), target, ty.table, go, ge)
                    align_cases.replay(ty.query(q), target, ty.table, go, ge, row, ops)
                    ref[(q, r)] = (row, ops)
        _aligned.update(table=table, ref=ref)
    return _aligned["table"], _aligned["ref"]


@pytest.mark.parametrize("checkpoint", [0, 1])
def test_align_hits_equal_the_walk_of_the_checker(engine, swamd, checker, dbase, checkpoint):  # noqa: F811
    packed, offs, db = dbase
    ty, go, ge, exp = world(checker, dbase, 24)
    table, ref = expected_alignments(checker, dbase)
    t = engine.torch
    nq, n = len(exp), len(exp) * TOP
    cap = max(pssm_cases.QLENS) + int(np.diff(offs).max())
    inp, d_pssm = place_matrix(engine, ty)
    out = Arena(t, _dev(engine), arena_bytes(n * 56, n * cap))
    d_aln = carve_i64(out, n * 7, "aln")
    c = out.carve(n * cap, name="ops")
    d_hits = t.from_numpy(table.copy()).to(_dev(engine))
    aln, ops = db.align_pssm_hits_device(d_pssm, ty.qoffs, ty.scoring(go, ge), d_hits, None, ops_cap=cap, out=(d_aln, out.view(c, t.uint8, (n * cap,))),
                                         checkpoint=checkpoint)
    engine.synchronize()
    assert engine.get_option("last_align_hits_checkpointed") == checkpoint and engine.get_option("last_align_hits_launches") > 3
    aln, ops = aln.cpu().numpy(), ops.cpu().numpy()
    assert len(ref) == n - 1 and max(row[6] for row, _ in ref.values()) > 100
    for q in range(nq):
        for r in range(TOP):
            if (q, r) in ref:
                row, eo = ref[(q, r)]
                assert tuple(aln[q, r]) == row, (q, r)
                assert ops[q, r, :row[6]].tobytes() == eo and (ops[q, r, row[6]:] == POISON).all(), (q, r)
            else:
                assert not aln[q, r].any() and (ops[q, r] == POISON).all(), (q, r)
    assert_guards(out)
    assert_guards(inp)
    # the host leg gives the same table
    haln, hops = swamd.align_pssm_hits_host((ty.matrix, ty.qoffs), (packed, offs), ty.scoring(go, ge), table)
    assert np.array_equal(aln, haln) and all(ops[q, r, :aln[q, r, 6]].tobytes() == hops[q][r] for q in range(nq) for r in range(TOP))


def test_the_24_bit_bound_from_both_sides(engine):
    """One target of 132 200 letters, one matrix of 132 200 columns over one letter: smax x 132 200 reaches 2^24 at 127 and not at
    126.  The refused call launches nothing and leaves the outputs poisoned; the accepted one scores the whole diagonal, 126 a cell."""
    t = engine.torch
    n = 132200
    assert 126 * n < (1 << 24) <= 127 * n
    d_pssm = t.full((n,), 127, dtype=t.int8, device=_dev(engine))
    qoffs = np.array([0, n], np.int64)
    out = Arena(t, _dev(engine), arena_bytes(24, 24, 8, 56))
    res, hits, nhits, aln = carve_i64(out, 3, "results"), carve_i64(out, 3, "hits"), carve_i64(out, 1, "nhits"), carve_i64(out, 7, "aln")
    for c in out.carves:
        out.must_stay(c)
    with engine.prepare_db([np.full(n, 65, np.uint8)]) as db:
        refused = (b"A", -1, 127, -2, -1)
        for call in (lambda: db.search_pssm_device(d_pssm, qoffs, refused, out=res),
                     lambda: db.search_pssm_top_device(d_pssm, qoffs, refused, 1, 0, out=(hits, nhits)),
                     lambda: db.align_pssm_hits_device(d_pssm, qoffs, refused, t.zeros((1, 1, 3), dtype=t.int64, device=_dev(engine)), None, out=(aln, None))):
            with pytest.raises(Exception) as e:
                call()
            assert "2^24" in str(e.value) and "smax = 127" in str(e.value)
        engine.synchronize()
        assert_guards(out)                                         # every output is still poison
        assert int(res[0]) == POISON64
        out.carves[0].expect = None                                # the accepted call writes the results
        got = db.search_pssm_device(d_pssm, qoffs, (b"A", -1, 126, -2, -1), out=res)
        engine.synchronize()
        assert got.cpu().numpy().tolist() == [[[n * (n + 1) + n, 126 * n, 0]]]
        assert_guards(out)
