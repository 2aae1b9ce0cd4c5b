"""GPU: the mask in front of the loop.  8 queries and 2000 targets with planted Q-rich stretches and planted homologues whose alignments
cross such a stretch: mask on the device (sw_db_mask_low_complexity), a second handle on the result, search_affine_top_stats and
align_affine_hits on the MASKED handle, msa_from_hits through the UNMASKED one -- enqueued back to back on one stream, nothing read in
between.  Hits, histograms, alignments and A3M bytes equal the host legs chained; the A3M rows hold original letters at positions
whose search saw the mask byte."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LETTERS = np.frombuffer(b"ACDEFGHIKLMNPRSTVWY", np.uint8)          # (no Q: every Q below is planted)
TOP, INCLUDE, GO, GE = 8, 30, -8, -1


def build_case(swamd):
    rng = np.random.default_rng(2031)
    rnd = lambda n: LETTERS[rng.integers(0, len(LETTERS), int(n))]
    qrich = lambda n: np.where(rng.random(n) < 0.75, np.uint8(ord("Q")), rnd(n)).astype(np.uint8)
    queries = [np.concatenate([rnd(50), qrich(16), rnd(50)]) for _ in range(4)] + [rnd(n) for n in (40, 90, 130)] + [np.concatenate([qrich(30), rnd(30)])]
    targets = [rnd(n) for n in rng.integers(0, 350, 1900)]
    targets += [np.concatenate([rnd(rng.integers(0, 60)), qrich(30), rnd(rng.integers(0, 60))]) for _ in range(60)]
    for q in queries[:6]:                                            # homologues: copies with a few letters changed, in random flanks
        for _ in range(6):
            h = q.copy()
            at = rng.integers(0, len(h), 4)
            h[at] = np.where(h[at] == ord("Q"), h[at], rnd(4))
            targets.append(np.concatenate([rnd(rng.integers(0, 40)), h, rnd(rng.integers(0, 40))]))
    targets += [rnd(n) for n in rng.integers(0, 350, 2000 - len(targets))]
    targets = [targets[k] for k in rng.permutation(len(targets))]
    assert len(queries) == 8 and len(targets) == 2000
    c = type("Case", (), {})()
    c.queries, c.tg = queries, swamd._pack_targets(targets)
    c.qpacked, c.qoffs = swamd._pack_targets(queries)
    sub = swamd.submat_match(5, -4)
    c.scoring = (sub, GO, GE)
    c.cap = int(np.diff(c.qoffs).max() + np.diff(c.tg[1]).max())
    # the host legs chained
    c.masked, c.nmasked = swamd.mask_low_complexity_host(c.tg)
    mtg = (c.masked, c.tg[1])
    c.hits, c.nhits = swamd.search_affine_multi_top_host(queries, mtg, c.scoring, TOP, 1)
    c.hist = swamd.score_hist_host(swamd.search_affine_multi_host(queries, mtg, c.scoring), c.tg[1], 0)
    c.aln, c.ops = swamd.align_affine_hits_host(queries, mtg, c.scoring, c.hits, c.nhits)
    q = (c.qpacked, c.qoffs)
    c.cols, c.rows, c.a3m = swamd.msa_from_hits_host(q, c.tg, INCLUDE, c.hits, c.nhits, c.aln, c.ops)               # the ORIGINAL letters
    c.cols_m, c.rows_m, c.a3m_m = swamd.msa_from_hits_host(q, mtg, INCLUDE, c.hits, c.nhits, c.aln, c.ops)         # what the search saw
    return c


@pytest.fixture(scope="module")
def case(swamd):
    return build_case(swamd)


def test_the_case_shows_something(swamd, case):
    c = case
    assert (c.nmasked > 0).sum() >= 80 and c.nmasked.sum() < 0.1 * len(c.masked)
    plain_hits, _ = swamd.search_affine_multi_top_host(c.queries, c.tg, c.scoring, TOP, 1)
    assert (plain_hits != c.hits).any()                                                   # the mask changes who is found
    # the two alignments differ exactly where the search saw the mask byte: there the one through the unmasked handle holds a letter
    assert len(c.cols) == len(c.cols_m) and len(c.a3m) == len(c.a3m_m) and (c.rows["len"] == c.rows_m["len"]).all()
    differ = c.a3m != c.a3m_m
    assert differ.sum() >= 50 and np.isin(c.a3m_m[differ], [ord("X"), ord("x")]).all() and not np.isin(c.a3m, [ord("X"), ord("x")]).any()


def test_device_chain_equals_the_host_legs_chained(swamd, engine, case):
    c = case
    t, dev = engine.torch, f"cuda:{engine.device}"
    d_db = t.from_numpy(c.tg[0].copy()).to(dev)
    d_q = t.from_numpy(c.qpacked.copy()).to(dev)
    nq = len(c.qoffs) - 1
    with engine.prepare_db(d_db, c.tg[1]) as plain:
        engine.synchronize()
        d_masked, d_n = plain.mask_low_complexity()
        with engine.prepare_db(d_masked, c.tg[1]) as masked:       # (sw_db_create reads the host offsets only)
            h, n, hist = masked.search_affine_top_stats_device(d_q, c.qoffs, c.scoring, TOP, 1)
            aln, ops = masked.align_affine_hits_device(d_q, c.qoffs, c.scoring, h, n, ops_cap=c.cap)
            a3m = t.full((len(c.a3m) + 64,), 0xA5, dtype=t.uint8, device=dev)
            cols, rows, a3m, total = plain.msa_from_hits_device(d_q, c.qoffs, INCLUDE, h, n, aln, ops, c.cap, a3m=a3m)
            engine.synchronize()
    assert np.array_equal(d_masked.cpu().numpy(), c.masked) and np.array_equal(d_n.cpu().numpy(), c.nmasked)
    assert np.array_equal(h.cpu().numpy().reshape(c.hits.shape), c.hits) and np.array_equal(n.cpu().numpy(), c.nhits)
    assert np.array_equal(hist.cpu().numpy().view(np.uint32).reshape(c.hist.shape), c.hist)
    assert np.array_equal(aln.cpu().numpy().reshape(c.aln.shape), c.aln)
    rows = rows.cpu().numpy().view(swamd.MSA_ROW).reshape(-1)[:nq * TOP].reshape(nq, TOP)
    a3m = a3m.cpu().numpy()
    assert (cols.cpu().numpy()[:len(c.cols)] == c.cols).all() and (rows == c.rows).all() and int(total.item()) == len(c.a3m)
    assert (a3m[:len(c.a3m)] == c.a3m).all() and (a3m[len(c.a3m):] == 0xA5).all()
