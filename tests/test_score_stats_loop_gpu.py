"""GPU: the E-value inclusion in its place in the loop -- search_affine_top_stats -> the histograms to the host, score_fit,
score_thresholds, the thresholds back -> hits_threshold (a COPY of the hit table) -> align_affine_hits (the untouched table) ->
msa_from_hits (column rows), pssm_hit_weights and pssm_from_hits on the copy with include_min_score at its minimum -- over a small
database with planted homologues, twice: the matrix, the weights, the column rows and the thresholded table equal the host legs
chained, byte for byte.  With evalue = 1e-3 the host legs alone keep every planted copy and no random target (asserted on the case)."""
import numpy as np
import pytest

import pssm_hits_cases as hc

pytestmark = pytest.mark.gpu

TOP, EVALUE, PER_HIT, PRIOR_WEIGHT, COPIES, NRANDOM = 24, 1e-3, 16, 160, 4, 400
INCLUDE_MIN = -(1 << 63)                                                     # the inclusion is the thresholded table's alone


def build_case(swamd):
    """Three queries; per query COPIES mutated copies inside flanks among NRANDOM random targets (and three empty ones).  The host legs
    chained; shared, the tests leave it unchanged."""
    rng = np.random.default_rng(2028)
    alpha = hc.PROTEIN[:20]
    queries = [rng.choice(alpha, n).astype(np.uint8) for n in (65, 129, 257)]
    targets = [rng.choice(alpha, int(n)).astype(np.uint8) for n in [0, 0, 0] + rng.integers(20, 400, NRANDOM).tolist()]
    planted = []
    for qs in queries:
        flank = lambda: rng.choice(alpha, int(rng.integers(0, 30))).astype(np.uint8)
        planted.append(list(range(len(targets), len(targets) + COPIES)))
        targets += [np.concatenate([flank(), hc.mutate(rng, qs, alpha), flank()]) for _ in range(COPIES)]
    order = rng.permutation(len(targets))
    place = np.argsort(order)
    targets = [targets[k] for k in order]
    sub = hc.random_submat(rng, lo=-8, hi=4)
    sub = np.minimum(sub, sub.T)
    for x in alpha:
        sub[x, x] = 7
    c = type("Case", (), {})()
    c.planted = [sorted(int(place[k]) for k in ks) for ks in planted]
    c.queries, c.tg, c.sub = queries, swamd._pack_targets(targets), sub
    c.qpacked, c.qoffs = swamd._pack_targets(queries)
    c.scoring, c.psc = (sub, -10, -1), (alpha, -8, 127, -10, -1)
    c.prior, _ = swamd.pssm_from_queries(queries, sub, alpha)
    c.cap = 257 + int(np.diff(c.tg[1]).max())
    q, pq = (c.qpacked, c.qoffs), (c.prior, c.qoffs)
    c.table = swamd.search_affine_multi_host(queries, c.tg, c.scoring)
    c.hits, c.nhits = swamd.search_affine_multi_top_host(queries, c.tg, c.scoring, TOP, 1)
    c.hist = swamd.score_hist_host(c.table, c.tg[1], 0)
    c.fit = swamd.score_fit(c.hist, 0)
    c.thr = swamd.score_thresholds(c.fit, EVALUE)
    c.keep, c.nkept, c.included = swamd.hits_threshold_host(c.tg[1], c.thr, c.hits, c.nhits)
    c.aln, c.ops = swamd.align_affine_hits_host(queries, c.tg, c.scoring, c.hits, c.nhits)
    c.cols = swamd.msa_from_hits_host(q, c.tg, INCLUDE_MIN, c.included, c.nhits, c.aln, c.ops)[0]
    c.w = swamd.pssm_hit_weights_host(c.qoffs, c.tg, c.psc, (PER_HIT, INCLUDE_MIN), c.included, c.nhits, c.aln, c.ops)
    c.m1 = swamd.pssm_from_hits_host(pq, c.tg, c.psc, (sub, PRIOR_WEIGHT, INCLUDE_MIN), c.included, c.nhits, c.aln, c.ops, weights=c.w)
    c.w_all = swamd.pssm_hit_weights_host(c.qoffs, c.tg, c.psc, (PER_HIT, INCLUDE_MIN), c.hits, c.nhits, c.aln, c.ops)
    c.m1_all = swamd.pssm_from_hits_host(pq, c.tg, c.psc, (sub, PRIOR_WEIGHT, INCLUDE_MIN), c.hits, c.nhits, c.aln, c.ops, weights=c.w_all)
    return c


@pytest.fixture(scope="module")
def case(swamd):
    return build_case(swamd)


def test_the_planted_copies_are_kept_and_no_random_target_is(case):
    c = case
    assert (c.fit["valid"] == 1).all() and (c.nhits == TOP).all()
    for q in range(3):
        kept = sorted(int(t) for t in c.included[q, :, 0] if t >= 0)
        assert kept == c.planted[q], (q, kept, c.planted[q])
    assert (c.nkept == COPIES).all() and (c.w != c.w_all).any() and (c.m1 != c.m1_all).any() and (c.m1 != c.prior).any()


def test_loop_equals_the_host_legs_chained_twice(swamd, engine, case):
    c = case
    t, dev = engine.torch, f"cuda:{engine.device}"
    nq = 3
    runs = []
    with engine.prepare_db(c.tg) as db:
        d_q = t.from_numpy(c.qpacked.copy()).to(dev)
        d_prior = t.from_numpy(c.prior.reshape(-1).copy()).to(dev)
        engine.synchronize()
        for _ in range(2):
            h, n, hist = db.search_affine_top_stats_device(d_q, c.qoffs, c.scoring, TOP, 1, 0)
            engine.synchronize()                                              # the one round trip: 40 KiB per query
            hist_h = hist.cpu().numpy().view(np.uint32)
            thr = swamd.score_thresholds(swamd.score_fit(hist_h, 0), EVALUE)
            d_thr = t.from_numpy(thr.reshape(-1).copy()).to(dev)
            inc = t.empty_like(h.view(-1))
            keep, nkept, _ = db.hits_threshold_device(d_thr, nq, TOP, h.view(-1), n, hits_out=inc)
            aln, ops = db.align_affine_hits_device(d_q, c.qoffs, c.scoring, h, n, ops_cap=c.cap)
            inc3 = inc.view(nq, TOP, 3)
            cols = db.msa_from_hits_device(d_q, c.qoffs, INCLUDE_MIN, inc3, n, aln, ops, c.cap, rows=False)[0]
            w = db.pssm_hit_weights_device(c.qoffs, c.psc, (PER_HIT, INCLUDE_MIN), inc3, n, aln, ops, c.cap)
            m1 = db.pssm_from_hits_device(d_prior, c.qoffs, c.psc, (c.sub, PRIOR_WEIGHT, INCLUDE_MIN), inc3, n, aln, ops, c.cap, weights=w)
            runs.append((hist_h, thr, h, n, inc, keep, nkept, aln, cols, w, m1))
        engine.synchronize()
    for hist_h, thr, h, n, inc, keep, nkept, aln, cols, w, m1 in runs:
        h, n, inc, keep, nkept, aln, cols, w, m1 = (x.cpu().numpy() for x in (h, n, inc, keep, nkept, aln, cols, w, m1))
        assert (hist_h == c.hist).all() and (thr == c.thr).all()
        assert (h.reshape(c.hits.shape) == c.hits).all() and (n == c.nhits).all()                 # the table of the printer is untouched
        assert (inc.reshape(c.hits.shape) == c.included).all()
        assert (keep[:nq * TOP].reshape(nq, TOP) == c.keep).all() and (nkept[:nq] == c.nkept).all()
        assert (aln.reshape(c.aln.shape) == c.aln).all() and (cols[:len(c.cols)] == c.cols).all()
        assert (w.reshape(-1)[:nq * TOP].reshape(nq, TOP) == c.w).all()
        assert (m1.reshape(c.m1.shape) == c.m1).all()
