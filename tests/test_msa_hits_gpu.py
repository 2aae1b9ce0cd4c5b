"""GPU: the query-anchored alignment written on the device (sw_db_msa_from_hits) against its host leg, byte for byte -- the column
rows, every sw_msa_row, the A3M rows up to the cap and the true total -- on the case tables of tests/msa_cases.py: outputs pre-filled
with poison between guard bytes, at odd byte bases, the column rows alone and the A3M alone, every cap, garbage tables, 300 queries x
top 64 (the scan crosses workgroups), one query of 1500 columns with top 4096, op rows of 3000 ops, and the loop search -> align -> msa
on one stream without synchronisation against the host legs chained, twice, byte-identical."""
import numpy as np
import pytest

import msa_cases as mc

pytestmark = pytest.mark.gpu

G, POISON = mc.GUARD, mc.POISON


def _dev(engine):
    return f"cuda:{engine.device}"


def device_tables(engine, c):
    t, dev = engine.torch, _dev(engine)
    up = lambda a: t.from_numpy(np.ascontiguousarray(a).reshape(-1).copy()).to(dev)
    return (up(c.qpacked) if c.qpacked is not None else None, up(c.hits), up(c.nhits) if c.nhits is not None else None, up(c.aln), up(c.ops))


def device_leg(swamd, engine, db, c, tables, want_cols=True, want_rows=True, want_a3m=True, a3m_cap=None, null_queries=False, odd=0):
    """One call into outputs pre-filled with poison between guard bytes, the byte buffers `odd` bytes off their aligned base.  Returns
    what mc.host_leg returns, after the same checks of the guards."""
    t, dev = engine.torch, _dev(engine)
    nq, top = c.hits.shape[:2]
    n, ncols = nq * top, int(c.qoffs[-1] - c.qoffs[0]) * top
    if a3m_cap is None:
        a3m_cap = _total(swamd, c)
    cols = t.full((G + odd + ncols + G,), POISON, dtype=t.uint8, device=dev)
    rows = t.full((G + 24 * n + G,), POISON, dtype=t.uint8, device=dev)
    a3m = t.full((G + odd + a3m_cap + G,), POISON, dtype=t.uint8, device=dev)
    total = t.full((3,), 0x5555555555555555, dtype=t.int64, device=dev)
    d_q, hits, nhits, aln, ops = tables
    db.msa_from_hits_device(None if null_queries else d_q, c.qoffs, c.include_min, hits, nhits, aln, ops, c.cap, top=top,
                            cols=cols[G + odd:G + odd + ncols] if want_cols else False, rows=rows[G:G + 24 * n].view(t.int64) if want_rows else False,
                            a3m=a3m[G + odd:G + odd + a3m_cap] if want_a3m else None, a3m_cap=a3m_cap, a3m_bytes=total[1:2] if want_rows else None)
    assert engine.get_option("last_msa_hits_launches") == (4 if want_rows else 1)
    engine.synchronize()
    cols, rows, a3m, total = (x.cpu().numpy() for x in (cols, rows, a3m, total))
    assert (cols[G:G + odd] == POISON).all() and (a3m[G:G + odd] == POISON).all()
    strip = lambda w: np.concatenate([w[:G], w[G + odd:]])
    return mc.check_guards(swamd, strip(cols), rows, strip(a3m), total, ncols, n, a3m_cap, want_cols, want_rows, want_a3m)


def _total(swamd, c):
    nq, top = c.hits.shape[:2]
    rows = swamd.msa_from_hits_host(c.qoffs if c.qpacked is None else (c.qpacked, c.qoffs), (c.packed, c.offs), c.include_min, c.hits, c.nhits, c.aln,
                                    c.ops.reshape(nq, top, -1))[1].reshape(-1)
    return int(rows["off"][-1] + rows["len"][-1])


def equal_to_host(swamd, engine, c, **kw):
    host = {k: v for k, v in kw.items() if k != "odd"}
    if "a3m_cap" not in host:
        host["a3m_cap"] = kw["a3m_cap"] = _total(swamd, c)
    exp = mc.host_leg(swamd, c, **host)
    with engine.prepare_db((c.packed, c.offs)) as db:
        tables = device_tables(engine, c)
        got = device_leg(swamd, engine, db, c, tables, **kw)
        assert mc.same(got, exp), _first_difference(got, exp)
        assert mc.same(device_leg(swamd, engine, db, c, tables, **kw), got)               # once more: the same bytes
    return got


def _first_difference(got, exp):
    if got[0] != exp[0]:
        d = next(k for k in range(len(exp[0])) if got[0][k] != exp[0][k])
        return f"cols differ first at byte {d}: {got[0][d:d + 20]} != {exp[0][d:d + 20]}"
    if got[1] != exp[1]:
        d = next(k for k in range(len(exp[1])) if got[1][k] != exp[1][k])
        return f"rows differ first at entry {d}: {got[1][d]} != {exp[1][d]}"
    if got[3] != exp[3]:
        return f"totals differ: {got[3]} != {exp[3]}"
    d = np.flatnonzero(got[2] != exp[2])[:1]
    return f"A3M bytes differ first at {d.tolist()}"


@pytest.mark.parametrize("nalpha,nhits,odd", [(4, False, 0), (20, True, 1), (20, False, 3), (4, True, 2)])
def test_hand_written_tables_equal_the_host_leg(swamd, engine, nalpha, nhits, odd):
    c = mc.synthetic(nalpha, 12, nhits=nhits)
    got = equal_to_host(swamd, engine, c, odd=odd)
    mc.assert_matches_reference(c, got)


def test_one_column_top_one_and_no_letters(swamd, engine):
    equal_to_host(swamd, engine, mc.synthetic(20, 30, qlens=(1,)))
    equal_to_host(swamd, engine, mc.synthetic(4, 1, qlens=(1, 5, 64, 70, 130) * 6), odd=1)
    got = equal_to_host(swamd, engine, mc.synthetic(20, 12, with_letters=False))
    assert all(w[3] == 0 for w in got[1])
    got = equal_to_host(swamd, engine, mc.synthetic(20, 12), null_queries=True)
    assert all(w[3] == 0 for w in got[1]) and any(w[2] > 0 for w in got[1])


def test_the_cap_of_the_a3m_buffer(swamd, engine):
    c = mc.synthetic(20, 12)
    _, rows, _, total, _ = mc.reference(c)
    boundary = [o for o, n, *_ in rows if n > 0 and 0 < o < total]
    for cap in (total, total - 1, 0, boundary[len(boundary) // 2], total + 5):
        got = equal_to_host(swamd, engine, c, a3m_cap=cap, odd=cap % 4)
        assert got[3] == total                                                            # the TRUE total, also beyond the cap


def test_outputs_alone(swamd, engine):
    c = mc.synthetic(20, 12, nhits=True)
    equal_to_host(swamd, engine, c, want_rows=False, want_a3m=False, odd=1)               # the column rows alone
    equal_to_host(swamd, engine, c, want_cols=False, odd=3)                               # the A3M alone
    equal_to_host(swamd, engine, c, want_cols=False, want_a3m=False)                      # a sizing call


@pytest.mark.parametrize("seed", [11, 12])
def test_garbage_tables_equal_the_host_leg_inside_the_buffers(swamd, engine, seed):
    equal_to_host(swamd, engine, mc.garbage(seed, nalpha=(4, 20)[seed % 2]), odd=1)


def test_300_queries_top_64(swamd, engine):
    """19 200 entries: 75 scan chunks, so the second level adds real offsets; query lengths 1..700."""
    rng = np.random.default_rng(300)
    qlens = [1, 700, 256, 257, 512, 513] + rng.integers(1, 701, 294).tolist()
    c = mc.synthetic(20, 64, qlens=tuple(qlens), nhits=True)
    got = equal_to_host(swamd, engine, c, odd=1)
    assert got[3] > (1 << 20) and sum(w[1] > 0 for w in got[1]) > 5000


def test_1500_columns_top_4096(swamd, engine):
    c = mc.synthetic(20, 4096, qlens=(1500,))
    got = equal_to_host(swamd, engine, c)
    assert sum(w[1] > 0 for w in got[1]) > 2000


def test_long_op_rows(swamd, engine):
    c = mc.long_ops_case()
    got = equal_to_host(swamd, engine, c, odd=3)
    mc.assert_matches_reference(c, got)
    assert max(w[4] for w in got[1]) > 1000


def test_loop_on_one_stream_equals_the_host_legs_chained_twice(swamd, engine):
    """search_affine_top -> align_affine_hits -> msa_from_hits, enqueued back to back on real device tables: nothing is synchronised or
    read in between.  The whole loop twice: the same bytes."""
    c = mc.real(swamd, 20)
    nq, top = c.hits.shape[:2]
    exp = mc.host_leg(swamd, c, a3m_cap=nq * top * c.cap)
    t, dev = engine.torch, _dev(engine)
    runs = []
    with engine.prepare_db((c.packed, c.offs)) as db:
        d_q = t.from_numpy(c.qpacked.copy()).to(dev)
        engine.synchronize()
        for _ in range(2):
            h, n = db.search_affine_top_device(d_q, c.qoffs, c.scoring, top, 1)
            aln, ops = db.align_affine_hits_device(d_q, c.qoffs, c.scoring, h, n, ops_cap=c.cap)
            a3m = t.full((nq * top * c.cap,), POISON, dtype=t.uint8, device=dev)
            runs.append(db.msa_from_hits_device(d_q, c.qoffs, c.include_min, h, n, aln, ops, c.cap, a3m=a3m) + (h, n, aln))
        engine.synchronize()
    for cols, rows, a3m, total, h, n, aln in runs:
        assert (h.cpu().numpy() == c.hits).all() and (n.cpu().numpy() == c.nhits).all() and (aln.cpu().numpy() == c.aln).all()
        rows = [tuple(int(x) for x in w) for w in rows.cpu().numpy().view(swamd.MSA_ROW)[:nq * top]]
        assert bytes(cols.cpu().numpy()) == exp[0] and rows == exp[1] and int(total.item()) == exp[3]
        got = a3m.cpu().numpy()
        assert (got[exp[2] >= 0] == exp[2][exp[2] >= 0]).all() and (got[exp[2] < 0] == POISON).all()
    assert exp[3] > 0 and all((x.cpu().numpy() == y.cpu().numpy()).all() for x, y in zip(runs[0][:4], runs[1][:4]))


def test_refusals_and_empty_calls(swamd, engine):
    c = mc.synthetic(20, 3)
    t, dev = engine.torch, _dev(engine)
    nq, top = c.hits.shape[:2]
    d_q, hits, _, aln, ops = device_tables(engine, c)
    ncols = int(c.qoffs[-1] - c.qoffs[0]) * top
    cols = t.full((ncols,), POISON, dtype=t.uint8, device=dev)
    rows = t.full((nq * top * 3,), 0x5555555555555555, dtype=t.int64, device=dev)
    a3m = t.full((4096,), POISON, dtype=t.uint8, device=dev)
    total = t.full((1,), 0x5555555555555555, dtype=t.int64, device=dev)
    L = swamd.lib()

    def untouched():
        engine.synchronize()
        return all((x.cpu().numpy() == (POISON if x.dtype == t.uint8 else 0x5555555555555555)).all() for x in (cols, rows, a3m, total))
    with engine.prepare_db((c.packed, c.offs)) as db:
        args = [engine._h, db._h, d_q.data_ptr(), c.qoffs.ctypes.data, nq, 0, hits.data_ptr(), None, top, aln.data_ptr(), ops.data_ptr(), c.cap,
                cols.data_ptr(), rows.data_ptr(), a3m.data_ptr(), 4096, total.data_ptr(), None]
        bad_q = c.qoffs.copy(); bad_q[2] = bad_q[1]
        for over in ({0: None}, {1: None}, {3: None}, {4: -1}, {3: bad_q.ctypes.data}, {8: 0}, {8: 4097}, {6: None}, {9: None}, {10: None}, {11: 0},
                     {12: None, 13: None, 14: None, 16: None}, {12: None, 13: None, 14: None}, {13: None}, {13: None, 14: None}, {16: None}, {15: -1}):
            a = list(args)
            for k, v in over.items():
                a[k] = v
            assert L.sw_db_msa_from_hits(*a) == -22, over
            assert untouched(), over                                                      # refused before the first launch
        a = list(args)                                                                    # no query: nothing is launched, nothing written
        a[4] = 0
        assert L.sw_db_msa_from_hits(*a) == 0 and engine.get_option("last_msa_hits_launches") == 0 and untouched()
    with engine.prepare_db([]) as empty:                                                  # a handle without targets: '-' and zero rows
        empty.msa_from_hits_device(d_q, c.qoffs, 0, hits, None, aln, ops, c.cap, top=top, cols=cols, rows=rows, a3m=a3m, a3m_bytes=total)
        engine.synchronize()
        assert (cols.cpu().numpy() == ord("-")).all() and not rows.cpu().numpy().any() and total.item() == 0 and (a3m.cpu().numpy() == POISON).all()
