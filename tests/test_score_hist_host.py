"""CPU: the score histogram's host leg (sw_score_hist_host) against the numpy restatement of the rule (tests/score_stats_cases.py) on
hand-made tables: lengths on both sides of every half-octave edge up to 2^20 - 1 (only the offsets exist), scores 0, 1, 254, 255, 256,
2^24 - 1 and negative ones, shifts 0, 3 and 16, empty targets, an offset base that is not 0; every counter is written; every refusal."""
import numpy as np
import pytest

import score_stats_cases as sc


def test_length_classes_are_half_octaves(swamd):
    assert [sc.length_class(L) for L in (1, 2, 3, 4, 5, 6, 7, 8, 11, 12, 15, 16)] == [0, 2, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8]
    assert sc.length_class((1 << 20) - 1) == 39 and sc.length_class(3 << 18) == 39 and sc.length_class((3 << 18) - 1) == 38
    assert all(swamd.length_class(L) == sc.length_class(L) for L in sc.edge_lengths())
    seen = {sc.length_class(L) for L in sc.edge_lengths()}
    assert seen == set(range(40)) - {1}                                       # no length has class 1


@pytest.mark.parametrize("shift", sc.SHIFTS)
def test_edges_equal_the_restatement(swamd, shift):
    res, offs = sc.edge_case(shift)
    exp = sc.hist_ref(res, offs, shift)
    got = swamd.score_hist_host(res, offs, shift)
    assert got.dtype == np.uint32 and got.shape == exp.shape and (got == exp).all()
    nonempty = int((np.diff(offs) > 0).sum())
    assert (got.sum(axis=(1, 2)) == nonempty).all() and nonempty < len(offs) - 1   # empty targets are counted nowhere
    if shift == 0:
        assert got[:, :, 255].sum() > 0 and got[:, :, 254].sum() > 0 and got[:, :, 0].sum() > 0 and got[:, :, 1].sum() > 0


def test_bins_of_the_edge_scores(swamd):
    offs = sc.offsets_of([150] * len(sc.SCORES))
    res = sc.table([list(sc.SCORES)])
    for shift, bins in ((0, [0, 1, 254, 255, 255, 255, 0, 0]), (3, [0, 0, 31, 31, 32, 255, 0, 0]), (16, [0, 0, 0, 0, 0, 255, 0, 0])):
        h = swamd.score_hist_host(res, offs, shift)[0]
        exp = np.zeros((sc.CLASSES, sc.BINS), np.uint32)
        np.add.at(exp, (np.full(len(bins), sc.length_class(150)), np.array(bins)), 1)
        assert (h == exp).all(), shift


def test_every_counter_is_written_and_nothing_else(swamd):
    L = swamd.lib()
    res, offs = sc.edge_case(0, nq=2)
    nt = len(offs) - 1
    buf = np.full(sc.GUARD + 2 * sc.CELLS + sc.GUARD, sc.P32, np.uint32)
    assert L.sw_score_hist_host(res.ctypes.data, 2, offs.ctypes.data, nt, 0, buf[sc.GUARD:].ctypes.data) == 0
    assert (buf[:sc.GUARD] == sc.P32).all() and (buf[-sc.GUARD:] == sc.P32).all()
    assert (buf[sc.GUARD:-sc.GUARD].reshape(2, sc.CLASSES, sc.BINS) == sc.hist_ref(res, offs, 0)).all()
    # no target: zeros; no query: nothing
    buf[:] = sc.P32
    assert L.sw_score_hist_host(res.ctypes.data, 2, offs.ctypes.data, 0, 0, buf[sc.GUARD:].ctypes.data) == 0
    assert (buf[sc.GUARD:-sc.GUARD] == 0).all() and (buf[:sc.GUARD] == sc.P32).all() and (buf[-sc.GUARD:] == sc.P32).all()
    buf[:] = sc.P32
    assert L.sw_score_hist_host(res.ctypes.data, 0, offs.ctypes.data, nt, 0, buf[sc.GUARD:].ctypes.data) == 0 and (buf == sc.P32).all()


def test_refusals(swamd):
    L = swamd.lib()
    res, offs = sc.edge_case(0, nq=1)
    nt = len(offs) - 1
    hist = np.full(sc.CELLS, sc.P32, np.uint32)
    back = offs.copy(); back[3] = back[2] - 1
    long = np.array([0, 1 << 20], np.int64)
    a = dict(res=res.ctypes.data, nq=1, offs=offs.ctypes.data, nt=nt, shift=0, hist=hist.ctypes.data)
    for over in (dict(res=None), dict(offs=None), dict(hist=None), dict(nq=-1), dict(nt=-1), dict(nt=1 << 31), dict(shift=-1), dict(shift=17),
                 dict(offs=back.ctypes.data), dict(offs=long.ctypes.data, nt=1)):
        assert L.sw_score_hist_host(*{**a, **over}.values()) == -22, over
        assert b"sw_score_hist_host" in L.sw_last_error() and (hist == sc.P32).all(), over
    with pytest.raises(ValueError):
        swamd.score_hist_host(res[:, :-1], offs, 0)
    with pytest.raises(swamd.SwError):
        swamd.score_hist_host(res, offs, 17)
