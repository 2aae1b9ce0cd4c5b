"""GPU: the score histogram inside the bounded-memory searches (sw_db_search_affine_top_stats, sw_db_search_pssm_top_stats): 5 queries
of 1, 17, 64, 300 and 513 letters against 25 000 targets of 0..40 letters with "search_results_mib" = 1, so that every query is a chunk
of its own and the full table never exists.  The histogram equals score_hist_host of the full host table; the hits and counts equal
those of the plain top call byte for byte; under "search_lanes" 32 and 16, and for the PSSM twin on the matrices of
pssm_from_queries.  The refusals the stats calls add."""
import ctypes

import numpy as np
import pytest

import pssm_hits_cases as hc
import score_stats_cases as sc

pytestmark = pytest.mark.gpu

TOP, MIN_SCORE, QLENS = 10, 1, (1, 17, 64, 300, 513)


@pytest.fixture(scope="module")
def case(swamd):
    rng = np.random.default_rng(513)
    alpha = hc.PROTEIN[:20]
    c = type("Case", (), {})()
    c.alpha = alpha
    c.queries = [rng.choice(alpha, n).astype(np.uint8) for n in QLENS]
    c.tg = swamd._pack_targets([rng.choice(alpha, int(n)).astype(np.uint8) for n in rng.integers(0, 41, 25000)])
    c.qpacked, c.qoffs = swamd._pack_targets(c.queries)
    sub = hc.random_submat(rng, lo=-6, hi=8)
    sub = np.minimum(sub, sub.T)
    for x in alpha:
        sub[x, x] = 9
    c.scoring, c.psc = (sub, -10, -1), (alpha, -4, 127, -10, -1)
    c.pssm, _ = swamd.pssm_from_queries(c.queries, sub, alpha)
    c.table = swamd.search_affine_multi_host(c.queries, c.tg, c.scoring)
    c.ptable = swamd.search_pssm_multi_host((c.pssm, c.qoffs), c.tg, c.psc)
    c.hist = {s: swamd.score_hist_host(c.table, c.tg[1], s) for s in (0, 2)}
    c.phist = swamd.score_hist_host(c.ptable, c.tg[1], 0)
    return c


def test_the_case_shows_something(case):
    c = case
    assert (c.hist[0].sum(axis=(1, 2)) == (np.diff(c.tg[1]) > 0).sum()).all() and (np.diff(c.tg[1]) == 0).any()
    assert ((c.hist[0] > 0).sum(axis=(1, 2)) >= 12).all()                     # several classes and bins per query
    assert (c.hist[0][0] != c.hist[0][4]).any() and (c.hist[0] != c.hist[2]).any()


@pytest.mark.parametrize("lanes", [32, 16])
def test_affine_top_stats(swamd, engine, case, lanes):
    c = case
    t, dev = engine.torch, f"cuda:{engine.device}"
    engine.set_option("search_results_mib", 1)
    engine.set_option("search_lanes", lanes)
    try:
        with engine.prepare_db(c.tg) as db:
            d_q = t.from_numpy(c.qpacked.copy()).to(dev)
            h0, n0 = db.search_affine_top_device(d_q, c.qoffs, c.scoring, TOP, MIN_SCORE)
            engine.synchronize()
            assert engine.get_option("last_search_top_chunks") == 5
            for shift in (0, 2):
                hist = t.full((sc.GUARD + 5 * sc.CELLS + sc.GUARD,), sc.P32, dtype=t.int32, device=dev)
                h1, n1, hs = db.search_affine_top_stats_device(d_q, c.qoffs, c.scoring, TOP, MIN_SCORE, shift, hist=hist[sc.GUARD:sc.GUARD + 5 * sc.CELLS])
                engine.synchronize()
                assert engine.get_option("last_search_top_chunks") == 5 and engine.get_option("last_score_hist_launches") == 5
                assert (hs.cpu().numpy().view(np.uint32) == c.hist[shift]).all()
                g = hist.cpu().numpy()
                assert (g[:sc.GUARD] == sc.P32).all() and (g[-sc.GUARD:] == sc.P32).all()
                assert t.equal(h1, h0) and t.equal(n1, n0)                    # the hits of the plain call, byte for byte
            hh, nn, hist = db.search_affine_top_stats(c.queries, c.scoring, TOP, MIN_SCORE)
            assert (hist == c.hist[0]).all() and (hh == h0.cpu().numpy()).all() and (nn == n0.cpu().numpy()).all()
    finally:
        engine.set_option("search_results_mib", 1024)
        engine.set_option("search_lanes", 32)
    # ... and the hits are the host table's best
    eh, en = swamd.search_affine_multi_top_host(c.queries, c.tg, c.scoring, TOP, MIN_SCORE)
    assert (hh == eh).all() and (nn == en).all()


@pytest.mark.parametrize("lanes", [32, 16])
def test_pssm_top_stats(swamd, engine, case, lanes):
    c = case
    t, dev = engine.torch, f"cuda:{engine.device}"
    engine.set_option("search_results_mib", 1)
    engine.set_option("search_lanes", lanes)
    try:
        with engine.prepare_db(c.tg) as db:
            d_m = t.from_numpy(c.pssm.reshape(-1).copy()).to(dev)
            h0, n0 = db.search_pssm_top_device(d_m, c.qoffs, c.psc, TOP, MIN_SCORE)
            h1, n1, hs = db.search_pssm_top_stats_device(d_m, c.qoffs, c.psc, TOP, MIN_SCORE, 0)
            engine.synchronize()
            assert engine.get_option("last_search_top_chunks") == 5
            assert (hs.cpu().numpy().view(np.uint32) == c.phist).all() and t.equal(h1, h0) and t.equal(n1, n0)
            hh, nn, hist = db.search_pssm_top_stats((c.pssm, c.qoffs), c.psc, TOP, MIN_SCORE)
            assert (hist == c.phist).all() and (hh == h0.cpu().numpy()).all()
    finally:
        engine.set_option("search_results_mib", 1024)
        engine.set_option("search_lanes", 32)


def test_refusals_of_the_stats_calls(swamd, engine, case):
    c = case
    t, dev = engine.torch, f"cuda:{engine.device}"
    L = swamd.lib()
    with engine.prepare_db(c.tg) as db:
        d_q = t.from_numpy(c.qpacked.copy()).to(dev)
        hits = t.full((5 * TOP * 3,), sc.P64, dtype=t.int64, device=dev)
        nhits = t.full((5,), sc.P64, dtype=t.int64, device=dev)
        hist = t.full((5 * sc.CELLS,), sc.P32, dtype=t.int32, device=dev)
        sub, a = swamd._affine(*c.scoring)
        for shift, hp in ((0, None), (-1, hist.data_ptr()), (17, hist.data_ptr())):
            assert L.sw_db_search_affine_top_stats(engine._h, db._h, d_q.data_ptr(), c.qoffs.ctypes.data, 5, ctypes.byref(a), TOP, MIN_SCORE, hits.data_ptr(),
                                                   nhits.data_ptr(), shift, hp, None) == -22
            assert b"sw_db_search_affine_top_stats" in L.sw_last_error()
            engine.synchronize()
            assert (hits == sc.P64).all().item() and (nhits == sc.P64).all().item() and (hist == sc.P32).all().item()
        assert L.sw_db_search_affine_top_stats(engine._h, db._h, d_q.data_ptr(), c.qoffs.ctypes.data, 0, ctypes.byref(a), TOP, MIN_SCORE, hits.data_ptr(),
                                               nhits.data_ptr(), 0, hist.data_ptr(), None) == 0
        engine.synchronize()
        assert (hist == sc.P32).all().item()                                  # no query: nothing is launched
