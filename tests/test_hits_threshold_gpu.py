"""GPU: the thresholds on a hit table on the device (sw_hits_threshold_device) against the host leg, byte for byte, on the tables of
the host test (tests/score_stats_cases.py: scores around their thresholds, targets of every kind, counts of every kind): top 1, 63, 64,
65 and 4096, 1 and 70 queries, with and without the counts, every output pre-filled with poison between guards, each output alone and
all together, in place and apart, twice the same bytes; the refusals and the empty call."""
import numpy as np
import pytest

import score_stats_cases as sc

pytestmark = pytest.mark.gpu

G = sc.GUARD


def handle(engine, offs):
    t = engine.torch
    return engine.prepare_db(t.zeros(1, dtype=t.uint8, device=f"cuda:{engine.device}"), offs)   # (only the offsets are read)


def device_leg(engine, db, thr, hits, nhits, want_keep=True, want_nkept=True, want_hits="in place"):
    t, dev = engine.torch, f"cuda:{engine.device}"
    nq, top = hits.shape[:2]
    n = nq * top
    d_thr = t.from_numpy(thr.reshape(-1).copy()).to(dev)
    d_n = t.from_numpy(nhits.copy()).to(dev) if nhits is not None else None
    keep = t.full((G + n + G,), sc.P32, dtype=t.int32, device=dev)
    nkept = t.full((G + nq + G,), sc.P64, dtype=t.int64, device=dev)
    tab = t.full((G + 3 * n + G,), sc.P64, dtype=t.int64, device=dev)
    tab[G:G + 3 * n] = t.from_numpy(hits.reshape(-1).copy()).to(dev)
    out = t.full((G + 3 * n + G,), sc.P64, dtype=t.int64, device=dev)
    h_in = tab[G:G + 3 * n]
    h_out = {"in place": h_in, "apart": out[G:G + 3 * n], None: None}[want_hits]
    db.hits_threshold_device(d_thr, nq, top, h_in, d_n, hits_out=h_out, keep=keep[G:G + n] if want_keep else False,
                             nkept=nkept[G:G + nq] if want_nkept else False)
    engine.synchronize()
    keep, nkept, tab, out = (x.cpu().numpy() for x in (keep, nkept, tab, out))
    for buf, body, poison, used in ((keep, n, sc.P32, want_keep), (nkept, nq, sc.P64, want_nkept), (tab, 3 * n, sc.P64, True),
                                    (out, 3 * n, sc.P64, want_hits == "apart")):
        assert (buf[:G] == poison).all() and (buf[G + body:] == poison).all()
        assert used or (buf[G:G + body] == poison).all()
    if want_hits != "in place":
        assert (tab[G:G + 3 * n] == hits.reshape(-1)).all()                   # the input table is only read
    res = {"in place": tab, "apart": out, None: None}[want_hits]
    return (keep[G:G + n].reshape(nq, top) if want_keep else None, nkept[G:G + nq] if want_nkept else None,
            res[G:G + 3 * n].reshape(nq, top, 3) if res is not None else None)


def same(got, exp):
    return all(g is None or (g == e).all() for g, e in zip(got, exp))


def equal_to_host(swamd, engine, case, with_counts=True, **kw):
    offs, thr, hits, nhits = case
    n = nhits if with_counts else None
    exp = swamd.hits_threshold_host(offs, thr, hits, n)
    with handle(engine, offs) as db:
        got = device_leg(engine, db, thr, hits, n, **kw)
        assert same(got, exp), [int((g != e).sum()) for g, e in zip(got, exp) if g is not None]
        assert same(device_leg(engine, db, thr, hits, n, **kw), got)          # once more: the same bytes
    return exp


@pytest.mark.parametrize("top", [1, 63, 64, 65, 4096])
@pytest.mark.parametrize("nq", [1, 70])
def test_equals_the_host_leg(swamd, engine, nq, top):
    case = sc.hits_case(nq * 10000 + top, nq, top) if top < 4096 else hits_case_4096(nq)
    exp = equal_to_host(swamd, engine, case)
    equal_to_host(swamd, engine, case, with_counts=False, want_hits="apart")
    if nq * top > 1:
        assert 0 < exp[0].mean() < 1


def hits_case_4096(nq):
    """The table of top 4096: one query's rows drawn once, rotated per query (the restated case builder walks every entry in Python)."""
    offs, thr, hits, nhits = sc.hits_case(4096, 1, 4096)
    hits = np.stack([np.roll(hits[0], q, axis=0) for q in range(nq)])
    return offs, np.repeat(thr, nq, axis=0), hits, np.array([4096 - 7 * q for q in range(nq)], np.int64)


def test_each_output_alone_and_all_together(swamd, engine):
    case = sc.hits_case(77, 9, 300)
    equal_to_host(swamd, engine, case, want_nkept=False, want_hits=None)      # keep alone
    equal_to_host(swamd, engine, case, want_keep=False, want_nkept=False)     # the hit table alone, in place
    equal_to_host(swamd, engine, case, want_keep=False, want_nkept=False, want_hits="apart")
    equal_to_host(swamd, engine, case, want_keep=False, want_hits="apart")
    equal_to_host(swamd, engine, case, want_hits="apart")


def test_host_wrapper_round_trip(swamd, engine):
    offs, thr, hits, nhits = sc.hits_case(3, 5, 20)
    with handle(engine, offs) as db:
        got = db.hits_threshold(thr, hits, nhits)
    assert same(got, swamd.hits_threshold_host(offs, thr, hits, nhits))


def test_refusals_and_the_empty_call(swamd, engine):
    t, dev = engine.torch, f"cuda:{engine.device}"
    L = swamd.lib()
    offs, thr, hits, nhits = sc.hits_case(6, 2, 4)
    d_thr = t.from_numpy(thr.reshape(-1).copy()).to(dev)
    d_hits = t.from_numpy(hits.reshape(-1).copy()).to(dev)
    d_n = t.from_numpy(nhits.copy()).to(dev)
    out = t.full((24,), sc.P64, dtype=t.int64, device=dev)
    keep = t.full((8,), sc.P32, dtype=t.int32, device=dev)
    nkept = t.full((2,), sc.P64, dtype=t.int64, device=dev)

    def untouched():
        engine.synchronize()
        return (keep == sc.P32).all().item() and (nkept == sc.P64).all().item() and (out == sc.P64).all().item()
    with handle(engine, offs) as db:
        a = dict(ctx=engine._h, db=db._h, thr=d_thr.data_ptr(), nq=2, top=4, hits=d_hits.data_ptr(), nhits=d_n.data_ptr(), out=out.data_ptr(),
                 keep=keep.data_ptr(), nkept=nkept.data_ptr())
        for over in (dict(ctx=None), dict(db=None), dict(thr=None), dict(hits=None), dict(nq=-1), dict(top=0), dict(top=4097), dict(out=None, keep=None)):
            assert L.sw_hits_threshold_device(*{**a, **over}.values(), None) == -22 and untouched(), over
            assert b"sw_hits_threshold_device" in L.sw_last_error()
        assert L.sw_hits_threshold_device(*{**a, "nq": 0}.values(), None) == 0 and untouched()
        assert L.sw_hits_threshold_device(*a.values(), None) == 0 and not untouched()
