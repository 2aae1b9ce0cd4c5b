"""GPU: the alignment filter on the device (sw_msa_filter_device) against its host leg, byte for byte, and twice in a row the same
bytes -- on the seeded families of tests/msa_filter_cases.py (bytes from all 256 values; between a tenth and nine tenths of the entries
kept, asserted): every output pre-filled with poison between guard words, the column rows and the query letters 1 and 3 bytes off
alignment, qoffsets[0] != 0, query lengths and tops around the tile and the staged chunk, one query of top 4096, 300 queries x top 64,
the workspace at its minimum (several chunks), the greedy chain across a row block and across two tiles, each output alone and all
together in place, the refusals and the empty call."""
import ctypes

import numpy as np
import pytest

import msa_filter_cases as fc

pytestmark = pytest.mark.gpu

G = fc.GUARD
P32, P64 = 0x55555555, 0x5555555555555555
QLENS = (1, 3, 4, 5, 63, 64, 65, 255, 257, 1500)


def _dev(engine):
    return f"cuda:{engine.device}"


def device_leg(engine, c, ident, cover, with_query=True, want_keep=True, want_nkept=True, want_hits="in place", odd_cols=1, odd_q=3):
    """One call: the column rows and the letters at odd byte bases, every output pre-filled with poison between guard words.
    Returns (keep, nkept, hits) as numpy, None where not asked for, after checking the guards and, out of place, the input table."""
    t, dev = engine.torch, _dev(engine)
    n = c.nq * c.top
    colbuf = t.full((G + odd_cols + len(c.cols),), fc.POISON, dtype=t.uint8, device=dev)
    colbuf[G + odd_cols:] = t.from_numpy(c.cols.copy()).to(dev)
    qbuf = t.full((G + odd_q + len(c.qpacked),), fc.POISON, dtype=t.uint8, device=dev)
    qbuf[G + odd_q:] = t.from_numpy(c.qpacked.copy()).to(dev)
    d_cols, d_q = colbuf[G + odd_cols:], qbuf[G + odd_q:]
    assert d_cols.data_ptr() % 4 == odd_cols % 4 and d_q.data_ptr() % 4 == odd_q % 4
    keep = t.full((G + n + G,), P32, dtype=t.int32, device=dev)
    nkept = t.full((G + c.nq + G,), P64, dtype=t.int64, device=dev)
    hits = t.full((G + 3 * n + G,), P64, dtype=t.int64, device=dev)
    hits[G:G + 3 * n] = t.from_numpy(c.hits.reshape(-1).copy()).to(dev)
    out = t.full((G + 3 * n + G,), P64, dtype=t.int64, device=dev)
    h_in = hits[G:G + 3 * n]
    h_out = {"in place": h_in, "apart": out[G:G + 3 * n], None: None}[want_hits]
    engine.msa_filter_device(d_cols, d_q if with_query else None, c.qoffs, c.top, (ident, cover), hits=h_in if want_hits else None, hits_out=h_out,
                             keep=keep[G:G + n] if want_keep else False, nkept=nkept[G:G + c.nq] if want_nkept else False)
    assert engine.get_option("last_msa_filter_launches") == 2 * engine.get_option("last_msa_filter_chunks") >= 2
    engine.synchronize()
    keep, nkept, hits, out = (x.cpu().numpy() for x in (keep, nkept, hits, out))
    for buf, body, poison, used in ((keep, n, P32, want_keep), (nkept, c.nq, P64, want_nkept), (hits, 3 * n, P64, True),
                                    (out, 3 * n, P64, want_hits == "apart")):
        assert (buf[:G] == poison).all() and (buf[G + body:] == poison).all()
        assert used or (buf[G:G + body] == poison).all()
    if want_hits != "in place":
        assert (hits[G:G + 3 * n] == c.hits.reshape(-1)).all()                # the input table is only read
    res = {"in place": hits, "apart": out, None: None}[want_hits]
    return (keep[G:G + n].reshape(c.nq, c.top) if want_keep else None, nkept[G:G + c.nq] if want_nkept else None,
            res[G:G + 3 * n].reshape(c.nq, c.top, 3) if res is not None else None)


def host_leg(swamd, c, ident, cover, with_query=True):
    return swamd.msa_filter_host(c.cols, (c.qpacked, c.qoffs) if with_query else c.qoffs, c.top, ident, cover, hits=c.hits)


def same(got, exp):
    return all(g is None or (g == e).all() for g, e in zip(got, exp))


def equal_to_host(swamd, engine, c, ident=90, cover=50, thinned=True, **kw):
    exp = host_leg(swamd, c, ident, cover, kw.get("with_query", True))
    if thinned:                                                               # neither all 0 nor all 1 would pass
        assert 0.1 <= exp[0].mean() <= 0.9, exp[0].mean()
    got = device_leg(engine, c, ident, cover, **kw)
    assert same(got, exp), [int((g != e).sum()) for g, e in zip(got, exp) if g is not None]
    assert same(device_leg(engine, c, ident, cover, **kw), got)               # once more: the same bytes
    return got


@pytest.mark.parametrize("top", [1, 2, 63, 64, 65, 100])
def test_families_equal_the_host_leg(swamd, engine, top):
    c = fc.families(100 + top, top, QLENS, q0=5)
    equal_to_host(swamd, engine, c, odd_cols=1, odd_q=3)
    equal_to_host(swamd, engine, c, with_query=False, odd_cols=3, odd_q=1)
    equal_to_host(swamd, engine, c, ident=40, cover=10, thinned=False, odd_cols=2, odd_q=0)
    keep = equal_to_host(swamd, engine, c, ident=101, cover=0, thinned=False)[0]
    assert (keep == (np.array([(c.rows(q) != fc.DASH).any(axis=1) for q in range(c.nq)]))).all()   # every row with a letter


def test_each_output_alone_and_all_together(swamd, engine):
    c = fc.families(9, 65, (40, 5, 129), q0=1)
    equal_to_host(swamd, engine, c)                                                                # all, the hit table in place
    equal_to_host(swamd, engine, c, want_nkept=False, want_hits=None)                              # keep alone
    equal_to_host(swamd, engine, c, want_keep=False, want_nkept=False)                             # the hit table alone, in place
    equal_to_host(swamd, engine, c, want_keep=False, want_nkept=False, want_hits="apart")
    equal_to_host(swamd, engine, c, want_keep=False, want_hits="apart")                            # ... with the counts


def test_one_query_top_4096(swamd, engine):
    equal_to_host(swamd, engine, fc.families(7, 4096, (37,), q0=2))


def test_300_queries_top_64(swamd, engine):
    qlens = [1, 200, 64, 65] + np.random.default_rng(300).integers(1, 201, 296).tolist()
    equal_to_host(swamd, engine, fc.families(8, 64, tuple(qlens)))


def test_several_chunks_at_the_least_workspace(swamd, engine):
    """40 queries of top 1000 take 136 KiB of bit planes each: 3 MiB hold 22 of them."""
    c = fc.families(9, 1000, (9,) * 40)
    assert engine.get_option("msa_filter_workspace_mib") == 256
    with pytest.raises(swamd.SwError):
        engine.set_option("msa_filter_workspace_mib", 2)
    engine.set_option("msa_filter_workspace_mib", 3)
    try:
        equal_to_host(swamd, engine, c)
        assert engine.get_option("last_msa_filter_chunks") == 2 and engine.get_option("last_msa_filter_launches") == 4
        equal_to_host(swamd, engine, fc.families(7, 4096, (5, 4)), thinned=False)                                 # one query of top 4096 per chunk
        assert engine.get_option("last_msa_filter_chunks") == 2
    finally:
        engine.set_option("msa_filter_workspace_mib", 256)
    equal_to_host(swamd, engine, c)
    assert engine.get_option("last_msa_filter_chunks") == 1


@pytest.mark.parametrize("places", [(63, 64, 65), (10, 70, 129), (0, 127, 128), (62, 63, 129)])
def test_greedy_chain_across_row_blocks_and_tiles(swamd, engine, places):
    """A kept; B falls to A -- from the next row block (another tile), from the end of A's own --; C, redundant to B only, in B's block
    or a later one, stays."""
    c = fc.chain_case(places, 130)
    keep = equal_to_host(swamd, engine, c, ident=90, cover=0, thinned=False)[0]
    assert np.flatnonzero(keep[0]).tolist() == [places[0], places[2]]
    without_a = fc.chain_case(places, 130)
    without_a.rows(0)[places[0]] = fc.DASH
    keep = equal_to_host(swamd, engine, without_a, ident=90, cover=0, thinned=False)[0]
    assert np.flatnonzero(keep[0]).tolist() == [places[1]]                                         # ... and falls where B is kept


def test_refusals_and_the_empty_call(swamd, engine):
    c = fc.families(2, 4, (6, 9))
    t, dev = engine.torch, _dev(engine)
    n = c.nq * c.top
    d_cols = t.from_numpy(c.cols.copy()).to(dev)
    d_q = t.from_numpy(c.qpacked.copy()).to(dev)
    hits = t.from_numpy(c.hits.reshape(-1).copy()).to(dev)
    out = t.full((3 * n,), P64, dtype=t.int64, device=dev)
    keep = t.full((n,), P32, dtype=t.int32, device=dev)
    nkept = t.full((c.nq,), P64, dtype=t.int64, device=dev)
    L = swamd.lib()

    def untouched():
        engine.synchronize()
        return (keep.cpu().numpy() == P32).all() and (nkept.cpu().numpy() == P64).all() and (out.cpu().numpy() == P64).all()

    def call(filt=(90, 50), **over):
        f = swamd._MsaFilter(*filt)
        a = dict(ctx=engine._h, cols=d_cols.data_ptr(), queries=d_q.data_ptr(), qoffs=c.qoffs.ctypes.data, nq=c.nq, top=c.top, filter=ctypes.pointer(f),
                 hits=hits.data_ptr(), hits_out=out.data_ptr(), keep=keep.data_ptr(), nkept=nkept.data_ptr())
        a.update(over)
        return L.sw_msa_filter_device(*a.values(), None)
    neg = c.qoffs.copy(); neg[0] = -1
    empty = c.qoffs.copy(); empty[1] = empty[0]
    back = c.qoffs.copy(); back[1] = back[2] + 1
    long = np.array([0, 1 << 20], np.int64)
    for over in (dict(ctx=None), dict(qoffs=None), dict(nq=-1), dict(qoffs=neg.ctypes.data), dict(qoffs=empty.ctypes.data), dict(qoffs=back.ctypes.data),
                 dict(qoffs=long.ctypes.data, nq=1), dict(top=0), dict(top=4097), dict(cols=None), dict(filter=None), dict(keep=None, hits_out=None),
                 dict(hits=None), dict(hits=None, keep=None)):
        assert call(**over) == -22, over
        assert untouched(), over                                                                   # refused before the first launch
    for filt in ((0, 50), (102, 50), (90, -1), (90, 101)):
        assert call(filt=filt) == -22 and untouched(), filt
    assert call(nq=0) == 0 and engine.get_option("last_msa_filter_launches") == 0 and engine.get_option("last_msa_filter_chunks") == 0 and untouched()
    assert call() == 0 and not untouched() and engine.get_option("last_msa_filter_launches") == 2
