"""GPU: the next iteration's PSSM built on the device (sw_db_pssm_from_hits) against its host leg, byte for byte on counts and matrix:
the synthetic, garbage and real tables of tests/pssm_hits_cases.py, top = 4096 over a five-target database, a query longer than one
tile, in place, counts only, matrix only, the same bytes on two runs, guard bytes and poisoned unused columns around every output --
and the closed loop search -> align -> update -> search on one stream with no synchronisation in between against the host legs chained.
The arithmetic edges (equal_to_reference: the device against the numpy rule directly, then against the host leg): products C x S of
1.7e10 and sums beyond 2^32 at N[j] = 4096 x 65535, the rounding table at that magnitude, both clamps, unobserved columns, alphabets
of 3, 5, 255 and 256 letters, S and prior over all of -128 .. 127 under smax 0, 1 and 127."""
import numpy as np
import pytest

import pssm_hits_cases as cases
from pssm_cases import rank_order

pytestmark = pytest.mark.gpu

GUARD, POISON, POISON32 = 4096, 0x55, 0x55555555


def _dev(engine):
    return f"cuda:{engine.device}"


class Device:
    """A case on the device: the tables as the search and alignment calls leave them, the prior with poisoned unused columns, and
    outputs inside guard bytes."""

    def __init__(self, engine, c, weights=None):
        t, dev = engine.torch, _dev(engine)
        self.engine, self.c, self.t = engine, c, t
        self.nl = len(c.letters)
        self.front, self.total = int(c.qoffs[0]) * self.nl, int(c.qoffs[-1]) * self.nl
        prior = np.full(GUARD + self.total + GUARD, POISON, np.int8)
        prior[GUARD + self.front:GUARD + self.total] = c.prior.reshape(-1)[self.front:]
        self.prior_h = prior
        self.hits = t.from_numpy(np.ascontiguousarray(c.hits)).to(dev)
        self.nhits = t.from_numpy(c.nhits.copy()).to(dev) if c.nhits is not None else None
        self.aln = t.from_numpy(np.ascontiguousarray(c.aln)).to(dev)
        self.ops = t.from_numpy(np.ascontiguousarray(c.ops)).to(dev)
        self.w = t.from_numpy(np.ascontiguousarray(weights, np.int32)).to(dev) if weights is not None else None

    def run(self, db, pw, inc, want_out=True, want_counts=True, in_place=False):
        """One call.  Returns (matrix of the queries' columns or None, counts or None) after checking every byte around them."""
        t, dev, c = self.t, _dev(self.engine), self.c
        whole = t.from_numpy(self.prior_h.copy()).to(dev)
        prior = whole[GUARD:]
        out_whole = whole if in_place else t.full((GUARD + self.total + GUARD,), POISON, dtype=t.int8, device=dev)
        ncnt = self.total - self.front
        cnt_whole = t.full((GUARD + ncnt + GUARD,), POISON32, dtype=t.int32, device=dev)
        top = c.hits.shape[1]
        db.pssm_from_hits_device(prior, c.qoffs, cases.scoring(c), (c.sub, pw, inc), self.hits, self.nhits, self.aln, self.ops, c.cap, weights=self.w,
                                 out=out_whole[GUARD:] if want_out else False, top=top, counts=cnt_whole[GUARD:] if want_counts else None)
        assert self.engine.get_option("last_pssm_hits_launches") == 1
        self.engine.synchronize()
        out, cnt, pri = out_whole.cpu().numpy(), cnt_whole.cpu().numpy(), whole.cpu().numpy()
        assert (out[:GUARD + self.front] == POISON).all() and (out[GUARD + self.total:] == POISON).all(), "the matrix was written outside the queries' columns"
        assert (cnt[:GUARD] == POISON32).all() and (cnt[GUARD + ncnt:] == POISON32).all(), "the counts were written outside their buffer"
        if not in_place:
            assert (pri == self.prior_h).all(), "the prior changed"
            if not want_out:
                assert (out == POISON).all()
        if not want_counts:
            assert (cnt == POISON32).all()
        return (out[GUARD + self.front:GUARD + self.total].reshape(-1, self.nl) if want_out else None,
                cnt[GUARD:GUARD + ncnt].reshape(-1, self.nl) if want_counts else None)


def equal_to_host(swamd, engine, c, pw, inc, weights=None):
    exp_out, exp_cnt = cases.host_leg(swamd, c, pw, inc, weights)
    with engine.prepare_db((c.packed, c.offs)) as db:
        d = Device(engine, c, weights)
        out, cnt = d.run(db, pw, inc)
        assert (cnt == exp_cnt).all(), f"{(cnt != exp_cnt).sum()} counts differ"
        assert (out == exp_out).all(), f"{(out != exp_out).sum()} entries differ"
        # in place, counts only, matrix only, and once more: the same bytes
        assert (d.run(db, pw, inc, want_counts=False, in_place=True)[0] == exp_out).all()
        assert (d.run(db, pw, inc, want_out=False)[1] == exp_cnt).all()
        out2, cnt2 = d.run(db, pw, inc)
        assert (out2 == out).all() and (cnt2 == cnt).all()
    return exp_out, exp_cnt


def weights_of(rng, nq, top):
    w = rng.integers(-3, 9, (nq, top)).astype(np.int32)
    w.reshape(-1)[::5] = 70000
    w.reshape(-1)[1::7] = -2**31
    return w


@pytest.mark.parametrize("nletters,top", [(1, 1), (4, 3), (24, 64), (256, 3), (256, 64)])
def test_synthetic_tables_equal_the_host_leg(swamd, engine, nletters, top):
    """(256 letters: tiles of 63 columns, so the 257- and 513-column queries take several tiles and a tile's edges fall INSIDE a 64-op chunk;
    with top = 64 every (nops, pattern) pair of the builder crosses such an edge)"""
    rng = np.random.default_rng(100 * nletters + top)
    c = cases.synthetic(rng, nletters, top)
    nq = len(cases.QLENS)
    equal_to_host(swamd, engine, c, 0, 0)
    equal_to_host(swamd, engine, c, 3, 20, weights_of(rng, nq, top))
    out, cnt = equal_to_host(swamd, engine, c, 65535, int(c.aln[:, :, 1].max()) + 1)      # nothing included: the clamped prior
    assert (cnt == 0).all() and (out == np.minimum(c.prior[int(c.qoffs[0]):], c.smax)).all()


@pytest.mark.parametrize("nletters,top", [(24, 64), (256, 9)])
def test_garbage_tables_equal_the_host_leg_inside_the_buffers(swamd, engine, nletters, top):
    rng = np.random.default_rng(3 * nletters + top)
    c = cases.garbage(rng, cases.synthetic(rng, nletters, top))
    equal_to_host(swamd, engine, c, 1, 0)
    equal_to_host(swamd, engine, c, 0, 0, weights_of(rng, len(cases.QLENS), top))


def test_real_tables_equal_the_host_leg(swamd, engine):
    rng = np.random.default_rng(11)
    c = cases.real(swamd, rng, top=8)
    out, cnt = equal_to_host(swamd, engine, c, 10, 1)
    assert (out != np.minimum(c.prior[int(c.qoffs[0]):], c.smax)).any()
    equal_to_host(swamd, engine, c, 0, 30)
    # the numpy mirror: the outputs of align_pssm_hits go straight in
    with engine.prepare_db((c.packed, c.offs)) as db:
        aln, ops = db.align_pssm_hits((c.prior, c.qoffs), cases.scoring(c), c.hits, c.nhits)
        m, counts = db.pssm_from_hits((c.prior, c.qoffs), cases.scoring(c), (c.sub, 10, 1), c.hits, c.nhits, aln, ops, want_counts=True)
    front = int(c.qoffs[0])
    assert (m[front:] == out).all() and (counts == cnt).all() and (m[:front] == c.prior[:front]).all()


def test_top_4096_over_five_targets(swamd, engine):
    """Every entry names one of five targets, most of them the same columns: the LDS adds pile onto few addresses."""
    rng = np.random.default_rng(4096)
    c = cases.synthetic(rng, 24, 4096, qlens=[300, 65], dup_targets=[300, 64, 65, 300, 1])
    c.aln[:, ::2, 2] = 0                                 # half of the entries start at column 0, target byte 0, all-M or nearly
    c.aln[:, ::2, 3] = 0
    _, cnt = equal_to_host(swamd, engine, c, 1, 0, weights_of(rng, 2, 4096))
    assert cnt.sum(axis=1).max() > 1000 * 65535 // 100   # a column that thousands of entries, many at weight 65535, added to
    assert cnt.sum(axis=1).max() < 2**28


def equal_to_reference(swamd, engine, c, pw, inc, weights=None):
    """The device against the numpy rule of tests/pssm_hits_cases.py directly, then equal_to_host (the host leg, in place, counts only,
    matrix only, twice the same)."""
    exp_out, exp_cnt, _ = cases.reference(c, pw, inc, weights)
    exp_out = exp_out[int(c.qoffs[0]):]
    with engine.prepare_db((c.packed, c.offs)) as db:
        out, cnt = Device(engine, c, weights).run(db, pw, inc)
    assert (cnt == exp_cnt).all(), f"{(cnt != exp_cnt).sum()} counts differ from the rule"
    assert (out == exp_out).all(), f"{(out != exp_out).sum()} entries differ from the rule, first {np.argwhere(out != exp_out)[0].tolist()}: " \
                                   f"{out[out != exp_out][0]} vs {exp_out[out != exp_out][0]}"
    host_out, host_cnt = equal_to_host(swamd, engine, c, pw, inc, weights)
    assert (host_out == exp_out).all() and (host_cnt == exp_cnt).all()
    return exp_out, exp_cnt


@pytest.mark.parametrize("first", [2048, 3072])
def test_products_beyond_32_bits(swamd, engine, first):
    """N[j] = 4096 x 65535 and C x S = 1.7e10 (the builder asserts both): equal halves give the exact half -1/2, the twin of 3072 and
    1024 a sum beyond 2^32 whose low 32 bits have the other sign."""
    c, w = cases.overflow_case(first)
    for pw in (0, 1, 65535):
        out, cnt = equal_to_reference(swamd, engine, c, pw, 0, w)
        want = [63, 63, 63] if first == 3072 else [0, 0, 0] if pw == 0 else [-1, 0, -1]
        assert (out == want).all() and (cnt.sum(axis=1) == 4096 * 65535).all(), (pw, out[0])


@pytest.mark.parametrize("row", cases.ROUNDING, ids=lambda r: f"pw{r[0]}_p{r[1]}_s{r[2][0]}_{r[2][1]}_n{r[3][0]}")
def test_rounding_at_numerators_of_1e10(swamd, engine, row):
    c, w = cases.rounding_case(*row)
    out, _ = equal_to_reference(swamd, engine, c, row[0], 0, w)
    assert (out == row[5]).all()


@pytest.mark.parametrize("pw,prior,s,w,exp", [(1, -3, 0, 1, -1), (1, -5, 0, 1, -2), (1, -5, 0, 2, -2), (2, -1, 0, 1, -1), (1, 5, 0, 1, 3), (1, 4, -7, 2, -3),
                                              (0, 9, -128, 1, -128), (1, 100, 127, 65535, 127)])
def test_round_half_up_with_floor_division(swamd, engine, pw, prior, s, w, exp):
    """The table of tests/test_pssm_hits_host.py on the device: one column, one letter, one 'M'."""
    c = cases.all_m_case([s], [1], prior=prior, ncols=1)
    out, cnt = equal_to_reference(swamd, engine, c, pw, 0, np.array([[w]], np.int32))
    assert cnt[0, 0] == w and out[0, 0] == exp


@pytest.mark.parametrize("smax", [0, 127])
@pytest.mark.parametrize("s", [127, -128])
def test_both_clamps(swamd, engine, s, smax):
    c = cases.clamp_case(s, smax)
    for pw in (0, 1, 65535):
        out, cnt = equal_to_reference(swamd, engine, c, pw, 0)
        assert (out[cnt.sum(axis=1) == 0] == -128).all()
    out, cnt = equal_to_reference(swamd, engine, c, 0, 0)
    assert (out[cnt.sum(axis=1) > 0] == s).all()


@pytest.mark.parametrize("smax", [0, 1, 127])
def test_an_unobserved_column_keeps_its_clamped_prior_exactly(swamd, engine, smax):
    """den == 0 (prior_weight 0) and the shortcut at N[j] == 0: P itself, negative and odd P among them."""
    rng = np.random.default_rng(40 + smax)
    c = cases.full_range_case(rng, 5, 3, smax)
    want = np.minimum(c.prior[int(c.qoffs[0]):], smax)
    for pw in (0, 1, 2, 65535):
        out, cnt = equal_to_reference(swamd, engine, c, pw, int(c.aln[:, :, 1].max()) + 1)
        assert not cnt.any() and (out == want).all()


@pytest.mark.parametrize("nletters", [3, 5, 255, 256])
def test_alphabets_of_3_5_255_and_256_letters(swamd, engine, nletters):
    """(the write loop steps k by 256 % nletters with a carry; code 255 is "none" at 255 letters and a letter at 256)"""
    rng = np.random.default_rng(7000 + nletters)
    c, at = cases.alphabet_case(rng, nletters, 9)
    for pw, kind in [(0, None), (2, "wild")]:
        _, cnt = equal_to_reference(swamd, engine, c, pw, 0, weights_of(rng, len(cases.QLENS), 9) if kind else None)
    if nletters == 256:
        assert cnt[:, 255].sum() > 0


@pytest.mark.parametrize("smax", [0, 1, 127])
@pytest.mark.parametrize("nletters", [5, 256])
def test_full_range_inputs(swamd, engine, nletters, smax):
    rng = np.random.default_rng(8000 + nletters + smax)
    c = cases.full_range_case(rng, nletters, 9, smax)
    for pw, w in [(0, None), (1, None), (3, weights_of(rng, len(cases.QLENS), 9)), (65535, weights_of(rng, len(cases.QLENS), 9))]:
        equal_to_reference(swamd, engine, c, pw, 0, w)


def test_refusals_and_empty_calls(swamd, engine):
    rng = np.random.default_rng(5)
    c = cases.synthetic(rng, 4, 3)
    t, dev = engine.torch, _dev(engine)
    with engine.prepare_db((c.packed, c.offs)) as db:
        d = Device(engine, c)
        prior = t.from_numpy(d.prior_h[GUARD:GUARD + d.total].copy()).to(dev)
        out = t.full((d.total,), POISON, dtype=t.int8, device=dev)

        def call(update=(c.sub, 1, 0), cap=c.cap, top=3, o=out, counts=None, sc=cases.scoring(c)):
            return db.pssm_from_hits_device(prior, c.qoffs, sc, update, d.hits, None, d.aln, d.ops, cap, out=o, top=top, counts=counts)

        for kw in (dict(cap=0), dict(cap=-1), dict(update=(c.sub, -1, 0)), dict(update=(c.sub, 65536, 0)), dict(o=False), dict(top=0),
                   dict(sc=(np.frombuffer(b"ACCA", np.uint8), -4, 11, -10, -1)), dict(sc=(c.letters, -4, 128, -10, -1)), dict(sc=(c.letters, -4, 11, 1, -1))):
            with pytest.raises(swamd.SwError):
                call(**kw)
            engine.synchronize()
            assert (out.cpu().numpy() == POISON).all(), kw                            # refused before the first launch
        L = swamd.lib()
        lt, sc = swamd._pssm_scoring(cases.scoring(c))
        sub, up = swamd._pssm_update((c.sub, 1, 0))
        import ctypes
        args = [engine._h, db._h, prior.data_ptr(), c.qoffs.ctypes.data, len(c.qoffs) - 1, ctypes.byref(sc), ctypes.byref(up), d.hits.data_ptr(), None, 3,
                d.aln.data_ptr(), d.ops.data_ptr(), c.cap, None, out.data_ptr(), None, None]
        for null in (2, 5, 6, 7, 10, 11):                                               # d_prior, scoring, upd, d_hits, d_aln, d_ops
            a = list(args)
            a[null] = None
            assert L.sw_db_pssm_from_hits(*a) == -22, null
        for top in (0, 4097, -1):
            a = list(args)
            a[9] = top
            assert L.sw_db_pssm_from_hits(*a) == -22, top
        up.sub = None
        assert L.sw_db_pssm_from_hits(*args) == -22
        # no query: nothing is launched, nothing written
        a = list(args)
        a[4] = 0
        up.sub = sub.ctypes.data
        assert L.sw_db_pssm_from_hits(*a) == 0 and engine.get_option("last_pssm_hits_launches") == 0
        engine.synchronize()
        assert (out.cpu().numpy() == POISON).all()
    # a handle without targets: no entry is used, the clamped prior comes out and the counts are zero
    with engine.prepare_db([]) as empty:
        cnt = t.full((d.total - d.front,), POISON32, dtype=t.int32, device=dev)
        empty.pssm_from_hits_device(prior, c.qoffs, cases.scoring(c), (c.sub, 1, 0), d.hits, None, d.aln, d.ops, c.cap, out=out, top=3, counts=cnt)
        engine.synchronize()
        assert (cnt.cpu().numpy() == 0).all()
        assert (out.cpu().numpy()[d.front:].reshape(-1, 4) == np.minimum(c.prior[int(c.qoffs[0]):], c.smax)).all()


def test_closed_loop_on_one_stream_equals_the_host_legs_chained(swamd, engine):
    """search_pssm_top -> align_pssm_hits -> pssm_from_hits -> search_pssm_top, enqueued back to back: the device tables go from call to
    call and nothing is synchronised or read in between."""
    rng = np.random.default_rng(2025)
    qlens = cases.QLENS * 2
    top, pw, inc = 5, 2, 1
    c = cases.real(swamd, rng, top=top, qlens=qlens, nrandom=170)
    assert len(c.offs) - 1 >= 200
    sc, tg = cases.scoring(c), (c.packed, c.offs)
    # the host legs chained (cases.real has done the first search and the alignment)
    m1 = swamd.pssm_from_hits_host((c.prior, c.qoffs), tg, sc, (c.sub, pw, inc), c.hits, c.nhits, c.aln, c.ops.reshape(len(qlens), top, -1))
    hits1, nhits1 = rank_order(swamd.search_pssm_multi_host((m1, c.qoffs), tg, sc), top, 1)
    changed = [(hits1[q, :nhits1[q], 0].tolist(), hits1[q, :nhits1[q], 2].tolist()) != (c.hits[q, :c.nhits[q], 0].tolist(), c.hits[q, :c.nhits[q], 2].tolist())
               for q in range(len(qlens))]
    assert any(changed), "the second table equals the first: the loop shows nothing"
    t, dev = engine.torch, _dev(engine)
    with engine.prepare_db(tg) as db:
        d_m = t.from_numpy(c.prior.reshape(-1).copy()).to(dev)
        engine.synchronize()
        h0, n0 = db.search_pssm_top_device(d_m, c.qoffs, sc, top, 1)
        aln, ops = db.align_pssm_hits_device(d_m, c.qoffs, sc, h0, n0, ops_cap=c.cap)
        d_m1 = db.pssm_from_hits_device(d_m, c.qoffs, sc, (c.sub, pw, inc), h0, n0, aln, ops, c.cap)
        h1, n1 = db.search_pssm_top_device(d_m1, c.qoffs, sc, top, 1)
        engine.synchronize()
    assert (h0.cpu().numpy() == c.hits).all() and (n0.cpu().numpy() == c.nhits).all()
    assert (d_m1.cpu().numpy().reshape(m1.shape) == m1).all()
    assert (h1.cpu().numpy() == hits1).all() and (n1.cpu().numpy() == nhits1).all()
