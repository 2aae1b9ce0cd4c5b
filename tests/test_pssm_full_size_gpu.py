"""GPU: the hit weights (sw_db_pssm_hit_weights) and the PSSM update (sw_db_pssm_from_hits) at their full size, byte for byte against
what tests/test_pssm_full_size_host.py has held to the numpy rules and the closed forms:
  * the 40-bit field: a query of 2^20 - 1 columns in several hundred tiles whose T_0 sets the top bits of the accumulator's low field
    (2^40 - 2^20 with one entry), then the update on the same tables, weighted by the device's own output, with counts, out of place
    and in place;
  * SUM = 2^32 in the finish kernel: 4096 entries of A_r = 2^20 at per_hit 1, 16, 65535, and the sibling at 2^32 - 2^20;
  * the second turn of every grid-stride loop: 2^20 + 3 queries of 9 tiles over 2^20 workgroups, where a tile with counts is followed in
    its workgroup by another query's tile without and the reverse (asserted by the case builder), and the finish kernel's workgroups
    0 .. 2 take a second query.
Every output is pre-filled with poison between guard words, every call runs twice, and the launches and tiles the library reports are
asserted.  The large results are compared on the device."""
import numpy as np
import pytest

import pssm_hits_cases as hc
import pssm_weights_cases as wc

pytestmark = pytest.mark.gpu

GUARD, POISON, POISON32 = 4096, 0x55, 0x55555555


def _dev(engine):
    return f"cuda:{engine.device}"


def weights_twice(engine, db, c, per_hit, inc, tables, tiles):
    """Two calls into poisoned outputs between guard words: asserts the launches reported and tiles(the tiles per query reported),
    whole guards, every entry written and the same bytes both times.  Returns the (nq, top) weights as a device tensor."""
    t = engine.torch
    nq, top = len(c.qoffs) - 1, c.hits.shape[1]
    got = []
    for _ in range(2):
        whole = t.full((GUARD + nq * top + GUARD,), POISON32, dtype=t.int32, device=_dev(engine))
        out = db.pssm_hit_weights_device(c.qoffs, hc.scoring(c), (per_hit, inc), *tables, c.cap, out=whole[GUARD:], top=top)
        assert out.data_ptr() == whole[GUARD:].data_ptr()
        assert engine.get_option("last_pssm_weights_launches") == 2 and tiles(engine.get_option("last_pssm_weights_tiles"))
        engine.synchronize()
        assert bool((whole[:GUARD] == POISON32).all()) and bool((whole[GUARD + nq * top:] == POISON32).all()), "the weights were written outside their buffer"
        w = whole[GUARD:GUARD + nq * top]
        assert not bool((w == POISON32).any()), "an entry was not written"
        got.append(w.reshape(nq, top))
    assert t.equal(got[0], got[1]), "two runs gave other bytes"
    return got[0]


class Update:
    """The update of a case on the device: the prior with poisoned unused columns between guard bytes, outputs likewise; the results
    are compared on the device with the expected matrix (the queries' columns) and the expected counts, given as (rows, their counts) --
    every other row of the counts must be zero."""

    def __init__(self, engine, c, tables, d_w, exp_out, rows, exp_cnt):
        t, dev = engine.torch, _dev(engine)
        self.engine, self.c, self.t, self.tables, self.d_w = engine, c, t, tables, d_w
        self.nl = len(c.letters)
        self.front, self.total = int(c.qoffs[0]) * self.nl, int(c.qoffs[-1]) * self.nl
        self.prior = t.full((GUARD + self.total + GUARD,), POISON, dtype=t.int8, device=dev)
        self.prior[GUARD + self.front:GUARD + self.total] = t.from_numpy(np.ascontiguousarray(c.prior).reshape(-1)[self.front:]).to(dev)
        self.exp_out = t.from_numpy(np.ascontiguousarray(exp_out).reshape(-1)).to(dev)
        self.rows = t.from_numpy(np.ascontiguousarray(rows, np.int64)).to(dev)
        self.exp_cnt = t.from_numpy(np.ascontiguousarray(exp_cnt, np.int32)).to(dev)
        self.nonzero = int(np.count_nonzero(exp_cnt))

    def run(self, db, pw, inc, in_place):
        t, dev, c = self.t, _dev(self.engine), self.c
        whole = self.prior.clone()
        out_whole = whole if in_place else t.full((GUARD + self.total + GUARD,), POISON, dtype=t.int8, device=dev)
        ncnt = self.total - self.front
        cnt_whole = t.full((GUARD + ncnt + GUARD,), POISON32, dtype=t.int32, device=dev)
        hits, nhits, aln, ops = self.tables
        db.pssm_from_hits_device(whole[GUARD:], c.qoffs, hc.scoring(c), (c.sub, pw, inc), hits, nhits, aln, ops, c.cap, weights=self.d_w,
                                 out=out_whole[GUARD:], top=c.hits.shape[1], counts=cnt_whole[GUARD:])
        assert self.engine.get_option("last_pssm_hits_launches") == 1
        self.engine.synchronize()
        assert bool((out_whole[:GUARD + self.front] == POISON).all()) and bool((out_whole[GUARD + self.total:] == POISON).all()), \
            "the matrix was written outside the queries' columns"
        assert bool((cnt_whole[:GUARD] == POISON32).all()) and bool((cnt_whole[GUARD + ncnt:] == POISON32).all()), "the counts were written outside their buffer"
        if not in_place:
            assert t.equal(whole, self.prior), "the prior changed"
        out = out_whole[GUARD + self.front:GUARD + self.total]
        assert t.equal(out, self.exp_out), f"{int((out != self.exp_out).sum())} entries differ"
        cnt = cnt_whole[GUARD:GUARD + ncnt].reshape(-1, self.nl)
        assert t.equal(cnt[self.rows], self.exp_cnt), "the counts of the observed columns differ"
        assert int(t.count_nonzero(cnt)) == self.nonzero, "a count that should be zero is not"


@pytest.mark.parametrize("second", [True, False])
def test_the_40_bit_field(swamd, engine, second):
    """T_0 = (L - 3) 2^20 + 3 x 2^19, and with one entry L x 2^20 = 2^40 - 2^20: the sums of several hundred tiles added into bits 30 .. 39
    of the accumulator, directly below the pair count.  Expected: the closed forms and the host legs."""
    c, T, A = wc.field_case(second)
    exp16 = [21, 11] if second else [16, 0]
    assert wc.shares(A, 16) == exp16
    with engine.prepare_db((c.packed, c.offs)) as db:
        tables = wc.device_tables(engine, c)
        for per_hit in (65535, 16):
            d_w = weights_twice(engine, db, c, per_hit, 0, tables, tiles=lambda n: n > 200)       # (512 on 256 compute units)
            w = d_w.cpu().numpy()
            assert w[0].tolist() == wc.shares(A, per_hit) and (w == wc.host_leg(swamd, c, per_hit, 0)).all()
        assert w[0].tolist() == exp16
        exp_out, exp_cnt = hc.host_leg(swamd, c, 32, 0, w)
        u = Update(engine, c, tables, d_w.reshape(-1), exp_out, np.arange(len(exp_cnt)), exp_cnt)
        u.run(db, 32, 0, in_place=False)
        u.run(db, 32, 0, in_place=False)
        u.run(db, 32, 0, in_place=True)


@pytest.mark.parametrize("sibling", [False, True])
def test_sum_2_to_the_32(swamd, engine, sibling):
    """4096 entries of A_r = 2^20: the finish kernel's SUM is 2^32 exactly and the numerator 2^49 at per_hit 65535.  Expected: the
    closed form -- every weight per_hit --, and for the sibling (two entries on one column: SUM = 2^32 - 2^20) the header's last line
    in Python integers; the host leg beside both."""
    c, A = wc.sum_case(sibling)
    with engine.prepare_db((c.packed, c.offs)) as db:
        tables = wc.device_tables(engine, c)
        for per_hit in (1, 16, 65535):
            w = weights_twice(engine, db, c, per_hit, 0, tables, tiles=lambda n: n >= 1).cpu().numpy()
            assert w[0].tolist() == wc.shares(A, per_hit)
            if not sibling:
                assert (w == per_hit).all()
            assert (w == wc.host_leg(swamd, c, per_hit, 0)).all()


def test_the_second_turn_of_the_grid_stride_loops(swamd, engine):
    """2^20 + 3 queries x 9 tiles over 2^20 workgroups: every workgroup of the tile kernels takes nine jobs (ten the first 27), the finish
    kernel's workgroups 0 .. 2 two queries.  Expected: the host legs on the queries with a used entry, and the closed form for every
    other query -- weight 0, counts 0, min(prior, smax) --; tests/test_pssm_full_size_host.py holds the host legs over the whole call
    to exactly that."""
    c, used_q, s = hc.second_turn_case()
    inc, t = hc.TURN_INCLUDE_MIN, engine.torch
    nq = len(c.qoffs) - 1
    ws = wc.host_leg(swamd, s, 16, inc)
    exp_w = np.zeros((nq, 1), np.int32)
    exp_w[used_q] = ws
    assert (wc.host_leg(swamd, c, 16, inc) == exp_w).all()
    sub_out, sub_cnt = hc.host_leg(swamd, s, 32, inc, ws)
    exp_out, rows, exp_cnt = hc.second_turn_expected(c, used_q, sub_out, sub_cnt)
    with engine.prepare_db((c.packed, c.offs)) as db:
        tables = wc.device_tables(engine, c)
        d_w = weights_twice(engine, db, c, 16, inc, tables, tiles=lambda n: n == 9)
        assert t.equal(d_w, t.from_numpy(exp_w).to(_dev(engine))), f"{int((d_w.cpu() != t.from_numpy(exp_w)).sum())} weights differ"
        u = Update(engine, c, tables, d_w.reshape(-1), exp_out, rows, exp_cnt)
        u.run(db, 32, inc, in_place=False)
        u.run(db, 32, inc, in_place=False)
        u.run(db, 32, inc, in_place=True)
