"""GPU: the hit weights written on the device (sw_db_pssm_hit_weights) against their host leg, byte for byte, on the cases of
tests/test_pssm_weights_host.py: the synthetic, garbage and real tables of tests/pssm_hits_cases.py, the closed forms, a 513-column query
cut into several tiles (the cross-tile sum), top = 4096 over a handful of duplicate targets, 256 letters, d_nhits == NULL, an output
pre-filled with poison inside guard words, the same bytes on two runs -- and the weighted loop search -> align -> weights -> update ->
search on one stream with no synchronisation in between against the host legs chained, and two calls of different shapes back to back
on two streams."""
import ctypes

import numpy as np
import pytest

import pssm_hits_cases as hc
import pssm_weights_cases as cases
from pssm_cases import rank_order

pytestmark = pytest.mark.gpu

GUARD, POISON32 = 1024, 0x55555555
A, C, G, T_ = (ord(x) for x in "ACGT")


def _dev(engine):
    return f"cuda:{engine.device}"


def device_weights(engine, db, c, per_hit, inc, tables=None):
    """One call into an output pre-filled with poison between guard words.  Returns the (nq, top) weights after checking that the guards
    are whole, that every entry was written and that the call made two launches."""
    t = engine.torch
    nq, top = len(c.qoffs) - 1, c.hits.shape[1]
    hits, nhits, aln, ops = tables or cases.device_tables(engine, c)
    whole = t.full((GUARD + nq * top + GUARD,), POISON32, dtype=t.int32, device=_dev(engine))
    out = db.pssm_hit_weights_device(c.qoffs, hc.scoring(c), (per_hit, inc), hits, nhits, aln, ops, c.cap, out=whole[GUARD:], top=top)
    assert out.data_ptr() == whole[GUARD:].data_ptr()
    assert engine.get_option("last_pssm_weights_launches") == 2
    engine.synchronize()
    w = whole.cpu().numpy()
    assert (w[:GUARD] == POISON32).all() and (w[GUARD + nq * top:] == POISON32).all(), "the weights were written outside their buffer"
    w = w[GUARD:GUARD + nq * top].reshape(nq, top)
    assert (w != POISON32).all(), "an entry was not written"
    return w


def equal_to_host(swamd, engine, c, per_hit, inc):
    exp = cases.host_leg(swamd, c, per_hit, inc)
    with engine.prepare_db((c.packed, c.offs)) as db:
        tables = cases.device_tables(engine, c)
        w = device_weights(engine, db, c, per_hit, inc, tables)
        assert (w == exp).all(), f"{(w != exp).sum()} weights differ, first at {np.argwhere(w != exp)[:1].tolist()}"
        assert (device_weights(engine, db, c, per_hit, inc, tables) == w).all()          # once more: the same bytes
    return w


@pytest.mark.parametrize("nletters,top", [(1, 1), (3, 3), (24, 64), (255, 9), (256, 3), (256, 64)])
def test_synthetic_tables_equal_the_host_leg(swamd, engine, nletters, top):
    rng = np.random.default_rng(100 * nletters + top)
    c = hc.synthetic(rng, nletters, top)
    for per_hit, inc in [(1, 0), (16, 0), (65535, 0), (100, 50)]:
        assert equal_to_host(swamd, engine, c, per_hit, inc).any()


def test_a_513_column_query_over_several_tiles(swamd, engine):
    """256 letters cut tiles of 63 columns: the hits of the 513-column query that start at column 0 and run through 300 ops have their
    pairs in five tiles, and every (entry, tile) adds its share to the entry's accumulator."""
    rng = np.random.default_rng(513)
    c = hc.synthetic(rng, 256, 64, qlens=[513, 64])
    assert ((c.aln[0, :, 2] == 0) & (c.aln[0, :, 6] > 2 * 63)).any()
    w = equal_to_host(swamd, engine, c, 16, 0)
    assert engine.get_option("last_pssm_weights_tiles") == 9 > 1
    assert (w == cases.reference(c, 16, 0)[0]).all()


def test_top_4096_over_five_targets(swamd, engine):
    """Every entry names one of five targets, most of them the same columns: n[j][k] in the thousands, LDS adds piled onto few addresses."""
    rng = np.random.default_rng(4096)
    c = hc.synthetic(rng, 24, 4096, qlens=[300, 65], dup_targets=[300, 64, 65, 300, 1])
    c.aln[:, ::2, 2] = 0
    c.aln[:, ::2, 3] = 0
    w = equal_to_host(swamd, engine, c, 16, 0)
    assert (w > 0).sum() > 4096 and len(set(w[0].tolist())) > 2


def test_closed_forms(swamd, engine):
    for per_hit, U in [(1, 1), (16, 7), (65535, 64)]:
        c = cases.sequences_case([[A, C, G, T_, A, A][:5 + U % 2]] * U)
        assert (equal_to_host(swamd, engine, c, per_hit, 0) == per_hit).all()
    c = cases.sequences_case([[A, C, G, T_, A], [A, C, G, T_, A], [C, G, T_, A, C]])
    assert equal_to_host(swamd, engine, c, 16, 0).tolist() == [[12, 12, 24]]
    c = cases.sequences_case([[C, G, T_]] + [[A, C, G]] * 4095)                          # the clamp at 65535 reached
    w = equal_to_host(swamd, engine, c, 65535, 0)
    assert w[0, 0] == 65535 and 0 < w[0, 1] < 65535
    c = cases.sequences_case([[A, C, G]] * 3, other_queries=[(4, [[A, C, G, T_]] * 2)])   # a query without a used entry
    c.aln[1, :, 1] = 10
    w = equal_to_host(swamd, engine, c, 16, 20)
    assert (w[0] == 16).all() and not w[1].any()


@pytest.mark.parametrize("nletters,top", [(24, 64), (256, 9)])
def test_garbage_tables_equal_the_host_leg_inside_the_buffers(swamd, engine, nletters, top):
    rng = np.random.default_rng(3 * nletters + top)
    c = hc.garbage(rng, hc.synthetic(rng, nletters, top))
    w = equal_to_host(swamd, engine, c, 7, 0)
    nh = np.clip(c.nhits, 0, top)
    assert w.any() and all(not w[q, nh[q]:].any() for q in range(len(nh)))
    c.nhits = None                                                                       # d_nhits == NULL: whole rows
    equal_to_host(swamd, engine, c, 7, 0)


def test_real_tables_and_the_numpy_mirror(swamd, engine):
    rng = np.random.default_rng(11)
    c = hc.real(swamd, rng, top=8)
    w = equal_to_host(swamd, engine, c, 16, 1)
    with engine.prepare_db((c.packed, c.offs)) as db:
        aln, ops = db.align_pssm_hits((c.prior, c.qoffs), hc.scoring(c), c.hits, c.nhits)
        assert (db.pssm_hit_weights(hc.scoring(c), (16, 1), (c.prior, c.qoffs), c.hits, c.nhits, aln, ops) == w).all()
        assert (db.pssm_hit_weights(hc.scoring(c), (16, 1), c.qoffs, c.hits, c.nhits, aln, ops) == w).all()


def test_refusals_and_empty_calls(swamd, engine):
    rng = np.random.default_rng(5)
    c = hc.synthetic(rng, 4, 3)
    t, dev = engine.torch, _dev(engine)
    nq = len(c.qoffs) - 1
    hits, _, aln, ops = cases.device_tables(engine, c)
    out = t.full((nq * 3,), POISON32, dtype=t.int32, device=dev)
    with engine.prepare_db((c.packed, c.offs)) as db:
        def call(weighting=(16, 0), cap=c.cap, top=3, sc=hc.scoring(c)):
            return db.pssm_hit_weights_device(c.qoffs, sc, weighting, hits, None, aln, ops, cap, out=out, top=top)

        for kw in (dict(cap=0), dict(cap=-1), dict(weighting=(0, 0)), dict(weighting=(-1, 0)), dict(weighting=(65536, 0)), dict(top=0),
                   dict(sc=(np.frombuffer(b"ACCA", np.uint8), -4, 11, -10, -1)), dict(sc=(c.letters, -4, 128, -10, -1)), dict(sc=(c.letters, -4, 11, 1, -1))):
            with pytest.raises(swamd.SwError):
                call(**kw)
            engine.synchronize()
            assert (out.cpu().numpy() == POISON32).all(), kw                              # refused before the first launch
        L = swamd.lib()
        lt, sc = swamd._pssm_scoring(hc.scoring(c))
        wt = swamd._pssm_weighting((16, 0))
        args = [engine._h, db._h, c.qoffs.ctypes.data, nq, ctypes.byref(sc), ctypes.byref(wt), hits.data_ptr(), None, 3, aln.data_ptr(), ops.data_ptr(), c.cap,
                out.data_ptr(), None]
        for null in (0, 1, 2, 4, 5, 6, 9, 10, 12):                                        # ctx, db, qoffsets, scoring, weighting, d_hits, d_aln, d_ops, d_weights
            a = list(args)
            a[null] = None
            assert L.sw_db_pssm_hit_weights(*a) == -22, null
        for top in (0, 4097, -1):
            a = list(args)
            a[8] = top
            assert L.sw_db_pssm_hit_weights(*a) == -22, top
        a = list(args)                                                                    # no query: nothing is launched, nothing written
        a[3] = 0
        assert L.sw_db_pssm_hit_weights(*a) == 0 and engine.get_option("last_pssm_weights_launches") == 0
        engine.synchronize()
        assert (out.cpu().numpy() == POISON32).all()
    with engine.prepare_db([]) as empty:                                                  # a handle without targets: every weight is 0
        empty.pssm_hit_weights_device(c.qoffs, hc.scoring(c), (16, 0), hits, None, aln, ops, c.cap, out=out, top=3)
        engine.synchronize()
        assert not out.cpu().numpy().any()


def _weighted_case(swamd, rng, top):
    """homologue_database with 8 copies of one homologue and 1 distinct one per query: the eight outvote the one 8 to 1 unless weighted."""
    letters = hc.letters_of(rng, 24)
    alpha = hc.PROTEIN[:20]
    qlens = [65, 129, 257]
    queries = [rng.choice(alpha, n).astype(np.uint8) for n in qlens]
    packed, offs = hc.homologue_database(rng, queries, 40, copies=1, alpha=alpha)
    extra = []
    for qs in queries:
        h = hc.mutate(rng, hc.mutate(rng, qs, alpha), alpha)
        extra += [h] * 8
    offs = np.concatenate([offs, offs[-1] + np.cumsum([len(x) for x in extra])]).astype(np.int64)
    packed = np.concatenate([packed] + extra)
    sub = hc.random_submat(rng, lo=-6, hi=8)
    sub = np.minimum(sub, sub.T)
    for x in alpha:
        sub[x, x] = 9                                                                     # homologues score well above chance
    c = hc._case(rng, letters, 127, qlens, packed, offs, top, sub=sub)
    m, _ = swamd.pssm_from_queries(queries, sub, letters)
    c.prior[hc.QFRONT:] = m
    c.cap = max(qlens) + int(np.diff(offs).max())
    return c


def test_weighted_loop_on_one_stream_equals_the_host_legs_chained(swamd, engine):
    """search_pssm_top -> align_pssm_hits -> pssm_hit_weights -> pssm_from_hits -> search_pssm_top, enqueued back to back: the device
    tables go from call to call and nothing is synchronised or read in between."""
    rng = np.random.default_rng(2026)
    top, per_hit, pw, inc = 12, 16, 32, 40
    c = _weighted_case(swamd, rng, top)
    sc, tg, nq = hc.scoring(c), (c.packed, c.offs), len(c.qoffs) - 1
    # the host legs chained
    hits0, nhits0 = rank_order(swamd.search_pssm_multi_host((c.prior, c.qoffs), tg, sc), top, inc)
    aln0, ops0 = swamd.align_pssm_hits_host((c.prior, c.qoffs), tg, sc, hits0, nhits0)
    w0 = swamd.pssm_hit_weights_host(c.qoffs, tg, sc, (per_hit, inc), hits0, nhits0, aln0, ops0)
    m1 = swamd.pssm_from_hits_host((c.prior, c.qoffs), tg, sc, (c.sub, pw, inc), hits0, nhits0, aln0, ops0, weights=w0)
    m1_unweighted = swamd.pssm_from_hits_host((c.prior, c.qoffs), tg, sc, (c.sub, pw // per_hit, inc), hits0, nhits0, aln0, ops0)
    hits1, nhits1 = rank_order(swamd.search_pssm_multi_host((m1, c.qoffs), tg, sc), top, inc)
    assert (nhits0 >= 9).all(), "the copies and the distinct homologue are not all among the hits"
    assert all(len(set(w0[q, :nhits0[q]].tolist())) > 1 for q in range(nq)), "every hit weighs the same"
    assert (m1 != m1_unweighted).any(), "the weighted matrix equals the unweighted one: the test shows nothing"
    t, dev = engine.torch, _dev(engine)
    with engine.prepare_db(tg) as db:
        d_m = t.from_numpy(c.prior.reshape(-1).copy()).to(dev)
        engine.synchronize()
        h0, n0 = db.search_pssm_top_device(d_m, c.qoffs, sc, top, inc)
        aln, ops = db.align_pssm_hits_device(d_m, c.qoffs, sc, h0, n0, ops_cap=c.cap)
        w = db.pssm_hit_weights_device(c.qoffs, sc, (per_hit, inc), h0, n0, aln, ops, c.cap)
        d_m1 = db.pssm_from_hits_device(d_m, c.qoffs, sc, (c.sub, pw, inc), h0, n0, aln, ops, c.cap, weights=w)
        h1, n1 = db.search_pssm_top_device(d_m1, c.qoffs, sc, top, inc)
        engine.synchronize()
    assert (h0.cpu().numpy() == hits0).all() and (n0.cpu().numpy() == nhits0).all()
    assert (w.cpu().numpy() == w0).all()
    assert (d_m1.cpu().numpy().reshape(m1.shape) == m1).all()
    assert (h1.cpu().numpy() == hits1).all() and (n1.cpu().numpy() == nhits1).all()


def test_two_calls_of_different_shapes_back_to_back_on_two_streams(swamd, engine):
    """Nothing is synchronised between the calls: the second call's table, accumulators and launches must not disturb the first's."""
    rng = np.random.default_rng(31)
    t = engine.torch
    c1 = hc.synthetic(rng, 256, 9)
    c2 = hc.synthetic(rng, 24, 64, qlens=[65, 300])
    c2.packed, c2.offs = c1.packed, c1.offs                                               # one database: c2's entries name targets 0..7 as c1's do
    exp1, exp2 = cases.host_leg(swamd, c1, 16, 0), cases.host_leg(swamd, c2, 3, 20)
    with engine.prepare_db((c1.packed, c1.offs)) as db:
        t1, t2 = cases.device_tables(engine, c1), cases.device_tables(engine, c2)
        s1, s2 = t.cuda.Stream(device=_dev(engine)), t.cuda.Stream(device=_dev(engine))
        engine.synchronize()
        with t.cuda.stream(s1):
            w1 = db.pssm_hit_weights_device(c1.qoffs, hc.scoring(c1), (16, 0), *t1, c1.cap, top=9)
        with t.cuda.stream(s2):
            w2 = db.pssm_hit_weights_device(c2.qoffs, hc.scoring(c2), (3, 20), *t2, c2.cap, top=64)
        with t.cuda.stream(s1):
            w1b = db.pssm_hit_weights_device(c1.qoffs, hc.scoring(c1), (16, 0), *t1, c1.cap, top=9)
        s1.synchronize()
        s2.synchronize()
    assert (w1.cpu().numpy() == exp1).all() and (w2.cpu().numpy() == exp2).all() and (w1b.cpu().numpy() == exp1).all()
