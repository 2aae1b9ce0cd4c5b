"""GPU: the filter in its place in the loop -- search_affine_top -> align_affine_hits -> msa_from_hits (column rows) -> msa_filter (in
place on the hit table) -> pssm_hit_weights -> pssm_from_hits -> msa_from_hits (A3M) -- enqueued back to back on one stream over a small
database with planted families, nothing synchronised or read in between, twice: the matrix, the weights and the A3M bytes equal the host
legs chained, and write_a3m on the second alignment holds exactly the kept entries."""
import numpy as np
import pytest

import pssm_hits_cases as hc

pytestmark = pytest.mark.gpu

TOP, IDENT, COVER, PER_HIT, PRIOR_WEIGHT, INCLUDE = 24, 90, 30, 16, 160, 30


def build_case(swamd):
    """Three queries; per query the query itself (a self-hit), a family of one homologue with seven near copies, two distant homologues
    and two fragments, among 150 random targets.  The host legs chained; shared, the tests leave it unchanged."""
    rng = np.random.default_rng(2027)
    alpha = hc.PROTEIN[:20]
    queries = [rng.choice(alpha, n).astype(np.uint8) for n in (65, 129, 257)]
    targets = [rng.choice(alpha, int(n)).astype(np.uint8) for n in [0, 1, 64] + rng.integers(2, 400, 150).tolist()]
    for qs in queries:
        member = hc.mutate(rng, qs, alpha)
        family = [member]
        for _ in range(7):
            near = member.copy()
            near[rng.integers(0, len(near), 2)] = rng.choice(alpha, 2)
            family.append(near)
        distant = [hc.mutate(rng, hc.mutate(rng, qs, alpha), alpha) for _ in range(2)]
        fragments = [qs[:len(qs) // 5].copy(), hc.mutate(rng, qs, alpha)[len(qs) // 2:len(qs) // 2 + len(qs) // 4]]
        flank = lambda: rng.choice(alpha, int(rng.integers(0, 30))).astype(np.uint8)
        targets += [qs.copy()] + [np.concatenate([flank(), x, flank()]) for x in family + distant + fragments]
    targets = [targets[k] for k in rng.permutation(len(targets))]
    sub = hc.random_submat(rng, lo=-6, hi=8)
    sub = np.minimum(sub, sub.T)
    for x in alpha:
        sub[x, x] = 9
    c = type("Case", (), {})()
    c.queries, c.tg, c.sub = queries, swamd._pack_targets(targets), sub
    c.qpacked, c.qoffs = swamd._pack_targets(queries)
    c.scoring, c.psc = (sub, -10, -1), (alpha, -4, 127, -10, -1)
    c.prior, _ = swamd.pssm_from_queries(queries, sub, alpha)
    c.cap = 257 + int(np.diff(c.tg[1]).max())
    q, pq = (c.qpacked, c.qoffs), (c.prior, c.qoffs)
    c.hits, c.nhits = swamd.search_affine_multi_top_host(queries, c.tg, c.scoring, TOP, 1)
    c.aln, c.ops = swamd.align_affine_hits_host(queries, c.tg, c.scoring, c.hits, c.nhits)
    c.cols = swamd.msa_from_hits_host(q, c.tg, INCLUDE, c.hits, c.nhits, c.aln, c.ops)[0]
    c.keep, c.nkept, c.kept_hits = swamd.msa_filter_host(c.cols, q, TOP, IDENT, COVER, hits=c.hits)
    c.w = swamd.pssm_hit_weights_host(c.qoffs, c.tg, c.psc, (PER_HIT, INCLUDE), c.kept_hits, c.nhits, c.aln, c.ops)
    c.m1 = swamd.pssm_from_hits_host(pq, c.tg, c.psc, (sub, PRIOR_WEIGHT, INCLUDE), c.kept_hits, c.nhits, c.aln, c.ops, weights=c.w)
    c.cols1, c.rows1, c.a3m1 = swamd.msa_from_hits_host(q, c.tg, INCLUDE, c.kept_hits, c.nhits, c.aln, c.ops)
    c.w_all = swamd.pssm_hit_weights_host(c.qoffs, c.tg, c.psc, (PER_HIT, INCLUDE), c.hits, c.nhits, c.aln, c.ops)
    c.m1_all = swamd.pssm_from_hits_host(pq, c.tg, c.psc, (sub, PRIOR_WEIGHT, INCLUDE), c.hits, c.nhits, c.aln, c.ops, weights=c.w_all)
    return c


@pytest.fixture(scope="module")
def case(swamd):
    return build_case(swamd)


def test_the_case_shows_something(case):
    c = case
    used = np.array([(c.cols[int(c.qoffs[q]) * TOP:int(c.qoffs[q + 1]) * TOP].reshape(TOP, -1) != ord("-")).any(axis=1) for q in range(3)])
    assert (used.sum(axis=1) >= 10).all(), "the planted targets are not among the aligned hits"
    assert ((c.nkept >= 2) & (c.nkept <= used.sum(axis=1) - 6)).all(), c.nkept           # the self-hit and most of the family fall
    assert (c.keep[:, 0] == 0).all()                                                      # rank 0 is the query itself
    assert (c.w != c.w_all).any() and (c.m1 != c.m1_all).any()                            # the filter changes the weights and the matrix
    assert (c.rows1["len"] > 0).sum() == c.nkept.sum()


def test_loop_on_one_stream_equals_the_host_legs_chained_twice(swamd, engine, case, tmp_path):
    c = case
    t, dev = engine.torch, f"cuda:{engine.device}"
    runs = []
    with engine.prepare_db(c.tg) as db:
        d_q = t.from_numpy(c.qpacked.copy()).to(dev)
        d_prior = t.from_numpy(c.prior.reshape(-1).copy()).to(dev)
        engine.synchronize()
        for _ in range(2):
            h, n = db.search_affine_top_device(d_q, c.qoffs, c.scoring, TOP, 1)
            aln, ops = db.align_affine_hits_device(d_q, c.qoffs, c.scoring, h, n, ops_cap=c.cap)
            cols = db.msa_from_hits_device(d_q, c.qoffs, INCLUDE, h, n, aln, ops, c.cap, rows=False)[0]
            keep, nkept, _ = engine.msa_filter_device(cols, d_q, c.qoffs, TOP, (IDENT, COVER), hits=h.view(-1), hits_out=h.view(-1))
            w = db.pssm_hit_weights_device(c.qoffs, c.psc, (PER_HIT, INCLUDE), h, n, aln, ops, c.cap)
            m1 = db.pssm_from_hits_device(d_prior, c.qoffs, c.psc, (c.sub, PRIOR_WEIGHT, INCLUDE), h, n, aln, ops, c.cap, weights=w)
            a3m = t.full((len(c.a3m1) + 64,), 0xA5, dtype=t.uint8, device=dev)
            cols1, rows1, a3m, total = db.msa_from_hits_device(d_q, c.qoffs, INCLUDE, h, n, aln, ops, c.cap, a3m=a3m)
            runs.append((h, n, aln, cols, keep, nkept, w, m1, cols1, rows1, a3m, total))
        engine.synchronize()
    nq = len(c.qoffs) - 1
    for h, n, aln, cols, keep, nkept, w, m1, cols1, rows1, a3m, total in runs:
        h, n, aln, cols, keep, nkept, w, m1, cols1, a3m = (x.cpu().numpy() for x in (h, n, aln, cols, keep, nkept, w, m1, cols1, a3m))
        assert (h.reshape(c.hits.shape) == c.kept_hits).all() and (n == c.nhits).all() and (aln.reshape(c.aln.shape) == c.aln).all()
        assert (cols[:len(c.cols)] == c.cols).all()
        assert (keep[:nq * TOP].reshape(nq, TOP) == c.keep).all() and (nkept[:nq] == c.nkept).all()
        assert (w.reshape(-1)[:nq * TOP].reshape(nq, TOP) == c.w).all()
        assert (m1.reshape(c.m1.shape) == c.m1).all()
        rows1 = rows1.cpu().numpy().view(swamd.MSA_ROW).reshape(-1)[:nq * TOP].reshape(nq, TOP)
        assert (cols1[:len(c.cols1)] == c.cols1).all() and (rows1 == c.rows1).all() and int(total.item()) == len(c.a3m1)
        assert (a3m[:len(c.a3m1)] == c.a3m1).all() and (a3m[len(c.a3m1):] == 0xA5).all()
        for q in range(nq):                                                               # the file: the query and exactly the kept entries
            path = str(tmp_path / f"q{q}.a3m")
            swamd.write_a3m(path, f"query{q}", c.queries[q], None, h.reshape(c.hits.shape)[q], c.aln[q], rows1[q], a3m)
            names = [line[1:].split()[0] for line in open(path).read().splitlines() if line.startswith(">")]
            assert names == [f"query{q}"] + [str(int(x)) for x in c.hits[q, :, 0][c.keep[q] == 1]]
