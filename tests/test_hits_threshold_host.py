"""CPU: the thresholds on a hit table, host leg (sw_hits_threshold_host), against the numpy restatement (tests/score_stats_cases.py):
scores one below, at and one above their threshold; every used-entry guard -- the count clamped to 0..top (negative, above top, NULL),
target -1, negative, >= ntargets and far beyond, an empty target --; in place; d_keep only and d_hits_out only; every refusal."""
import numpy as np
import pytest

import score_stats_cases as sc


@pytest.mark.parametrize("nq, top", [(1, 1), (5, 7), (9, 64), (3, 300)])
def test_equals_the_restatement(swamd, nq, top):
    offs, thr, hits, nhits = sc.hits_case(nq * 1000 + top, nq, top)
    for n in (nhits, None):
        exp = sc.threshold_ref(offs, thr, hits, n)
        got = swamd.hits_threshold_host(offs, thr, hits, n)
        assert all((g == e).all() for g, e in zip(got, exp))
        if top > 1 and n is None:
            assert 0 < exp[0].mean() < 1                                      # neither all kept nor all dropped would pass
        assert (got[2][..., 1:] == hits[..., 1:]).all()                       # max_pos and max_score stay


def test_equality_from_both_sides_and_the_guards(swamd):
    offs = sc.offsets_of([0, 1, 37, 150, 0, 800], first=9)
    thr = np.zeros((1, sc.CLASSES), np.int64)
    thr[0, sc.length_class(37)], thr[0, sc.length_class(150)], thr[0, sc.length_class(800)], thr[0, 0] = 40, 50, 60, 7
    rows = [(2, 39, 0), (2, 40, 1), (2, 41, 1), (3, 49, 0), (3, 50, 1), (5, 59, 0), (5, 60, 1), (1, 6, 0), (1, 7, 1),
            (0, 1000, 0), (4, 1000, 0), (-1, 1000, 0), (6, 1000, 0), (1 << 32, 1000, 0), (-(1 << 32) + 2, 1000, 0), (2, 1000, 1), (2, 1000, 0)]
    hits = np.array([[(t, 77, s) for t, s, _ in rows]], np.int64)
    want = np.array([[k for _, _, k in rows]], np.int32)
    nhits = np.array([len(rows) - 1], np.int64)                               # the last entry lies beyond the count
    keep, nkept, out = swamd.hits_threshold_host(offs, thr, hits, nhits)
    assert (keep == want).all() and nkept[0] == want.sum()
    assert (out[0, :, 0] == np.where(want[0] == 1, hits[0, :, 0], -1)).all() and (out[..., 1:] == hits[..., 1:]).all()
    for n, kept_last in ((len(rows), 1), (len(rows) + 9, 1), (None, 1), (-1, None), (0, None)):
        k = swamd.hits_threshold_host(offs, thr, hits, None if n is None else np.array([n], np.int64))[0]
        assert (k[0, -1] == kept_last) if kept_last is not None else (k == 0).all(), n


def test_outputs_alone_and_in_place(swamd):
    L = swamd.lib()
    offs, thr, hits, nhits = sc.hits_case(5, 4, 65)
    exp = sc.threshold_ref(offs, thr, hits, nhits)
    nt, n = len(offs) - 1, 4 * 65
    G = sc.GUARD

    def run(want_keep, want_out, want_nkept, in_place):
        keep = np.full(G + n + G, sc.P32, np.int32)
        nkept = np.full(G + 4 + G, sc.P64, np.int64)
        h = np.full(G + 3 * n + G, sc.P64, np.int64); h[G:G + 3 * n] = hits.reshape(-1)
        out = np.full(G + 3 * n + G, sc.P64, np.int64)
        dst = h if in_place else out
        assert L.sw_hits_threshold_host(offs.ctypes.data, nt, thr.ctypes.data, 4, 65, h[G:].ctypes.data, nhits.ctypes.data,
                                        dst[G:].ctypes.data if want_out else None, keep[G:].ctypes.data if want_keep else None,
                                        nkept[G:].ctypes.data if want_nkept else None) == 0
        for buf, body, poison in ((keep, n, sc.P32), (nkept, 4, sc.P64), (h, 3 * n, sc.P64), (out, 3 * n, sc.P64)):
            assert (buf[:G] == poison).all() and (buf[G + body:] == poison).all()
        assert (keep[G:G + n].reshape(4, 65) == exp[0]).all() if want_keep else (keep == sc.P32).all()
        assert (nkept[G:G + 4] == exp[1]).all() if want_nkept else (nkept == sc.P64).all()
        if want_out:
            assert (dst[G:G + 3 * n].reshape(4, 65, 3) == exp[2]).all()
        if not (want_out and in_place):
            assert (h[G:G + 3 * n] == hits.reshape(-1)).all()                 # the input table is only read
        if not want_out or in_place:
            assert (out == sc.P64).all()
    run(True, True, True, True)
    run(True, True, True, False)
    run(True, False, False, False)                                            # d_keep only
    run(False, True, False, False)                                            # d_hits_out only
    run(False, True, True, True)


def test_refusals(swamd):
    L = swamd.lib()
    offs, thr, hits, nhits = sc.hits_case(6, 2, 4)
    nt = len(offs) - 1
    keep = np.full(8, sc.P32, np.int32)
    out = np.full(24, sc.P64, np.int64)
    back = offs.copy(); back[5] = back[4] - 1
    long = np.array([0, 1 << 20], np.int64)
    a = dict(offs=offs.ctypes.data, nt=nt, thr=thr.ctypes.data, nq=2, top=4, hits=hits.ctypes.data, nhits=nhits.ctypes.data, out=out.ctypes.data,
             keep=keep.ctypes.data, nkept=None)
    for over in (dict(offs=None), dict(thr=None), dict(hits=None), dict(nq=-1), dict(nt=-1), dict(nt=1 << 31), dict(top=0), dict(top=4097),
                 dict(out=None, keep=None), dict(offs=back.ctypes.data), dict(offs=long.ctypes.data, nt=1)):
        assert L.sw_hits_threshold_host(*{**a, **over}.values()) == -22, over
        assert b"sw_hits_threshold_host" in L.sw_last_error() and (keep == sc.P32).all() and (out == sc.P64).all(), over
    assert L.sw_hits_threshold_host(*{**a, "nq": 0}.values()) == 0 and (keep == sc.P32).all()
    assert L.sw_hits_threshold_host(*a.values()) == 0 and not (keep == sc.P32).any()
    with pytest.raises(ValueError):
        swamd.hits_threshold_host(offs, thr[:, :39], hits, nhits)
