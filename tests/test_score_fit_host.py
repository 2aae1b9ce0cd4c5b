"""CPU: the fit, the E-value and the thresholds (sw_score_fit_hist, sw_score_evalue, sw_score_thresholds) against the numpy restatement
of the header's formulas (tests/score_stats_cases.py): a, b, sigma to 1e-9 relative -- double rounding over 10^4 terms with a wide
margin --, thresholds within +-1; the degenerate histograms; monotonic thresholds; E(T) <= evalue < E(T - 1); planted outliers move the
fit by less than the planted-free fit's own rounds differ; the refusals."""
import math

import numpy as np
import pytest

import score_stats_cases as sc

REL = 1e-9
EVALUES = (1e-10, 1e-3, 0.5, 1.0, 10.0, 100.0, 3999.0)


def close(got, exp):
    return abs(got - exp) <= REL * max(abs(exp), 1e-300)


@pytest.mark.parametrize("shift", sc.SHIFTS)
def test_fit_equals_the_restatement(swamd, shift):
    hists = np.stack([sc.null_hist(s) for s in (1, 7, 11)] + [sc.null_hist(3, planted=50), sc.null_hist(5, n=400)])
    hists[2, :, 255] += 9                                                     # censored scores never enter the fit
    fit = swamd.score_fit(hists, shift)
    for q in range(len(hists)):
        exp, _ = sc.fit_ref(hists[q], shift)
        for f in ("a", "b", "sigma"):
            assert close(float(fit[q][f]), exp[f]), (q, f, float(fit[q][f]), exp[f])
        for f in ("n_db", "n_fit", "n_censored", "valid"):
            assert int(fit[q][f]) == exp[f], (q, f)
        assert int(fit[q]["shift"]) == shift and exp["valid"] == 1
        for ev in EVALUES:
            got, ref = swamd.score_thresholds(fit[q:q + 1], ev)[0], sc.thresholds_ref(exp, ev)
            assert np.abs(got - ref).max() <= 1, (q, ev)
        for L, s in ((1, 0), (20, 30), (150, 45), (800, 60), ((1 << 20) - 1, 200)):
            e, r = swamd.score_evalue(fit[q], L, s << shift), sc.evalue_ref(exp, L, s << shift)
            assert abs(e - r) <= 1e-7 * r, (q, L, s, e, r)                    # (exp of exp: the relative error of z times |dE / E dz| <= 1.3 |z|)
    assert int(fit[2]["n_censored"]) == 9 * sc.CLASSES and int(fit[2]["n_db"]) == 4000 + 9 * sc.CLASSES


def test_degenerate_histograms(swamd):
    one_class = np.zeros((sc.CLASSES, sc.BINS), np.uint32)
    one_class[14] = sc.null_hist(1).sum(axis=0)                               # every target in one class: no slope
    all_equal = np.zeros_like(one_class); all_equal[10:20, 33] = 50           # every score equal: no spread
    few = np.zeros_like(one_class); few[12, 20:49] = 1                        # 29 targets
    thirty = few.copy(); thirty[13, 30] = 1
    empty = np.zeros_like(one_class)
    censored = np.zeros_like(one_class); censored[:, 255] = 100               # nothing below bin 255
    fit = swamd.score_fit(np.stack([one_class, all_equal, few, thirty, empty, censored]), 0)
    assert fit[0]["valid"] == 1 and fit[0]["b"] == 0.0 and fit[0]["sigma"] > 0
    assert fit[1]["valid"] == 0 and fit[1]["sigma"] == 0.0 and fit[1]["a"] == 33.0 and fit[1]["n_fit"] == 500
    assert fit[2]["valid"] == 0 and fit[2]["n_fit"] == 29 and fit[2]["sigma"] > 0
    assert fit[3]["valid"] == 1 and fit[3]["n_fit"] == 30
    assert fit[4]["valid"] == 0 and fit[4]["n_db"] == 0
    assert fit[5]["valid"] == 0 and fit[5]["n_fit"] == 0 and fit[5]["n_censored"] == fit[5]["n_db"] == 4000
    thr = swamd.score_thresholds(fit, 1e-3)
    for q in (1, 2, 4, 5):                                                    # an invalid fit drops nothing and has no E-value
        assert (thr[q] == 0).all() and math.isnan(swamd.score_evalue(fit[q], 150, 40))
    assert (thr[0] > 0).all() and (thr[0] == thr[0][0]).all()                 # b = 0: one threshold for every class
    assert (swamd.score_thresholds(fit, 1e9) == 0).all()                      # evalue >= n_db
    assert math.isnan(swamd.score_evalue(fit[0], 0, 40))


def test_thresholds_are_monotonic_and_tight(swamd):
    fit = swamd.score_fit(np.stack([sc.null_hist(1), sc.null_hist(7)]), 0)
    prev = None
    for ev in sorted(EVALUES, reverse=True):
        thr = swamd.score_thresholds(fit, ev)
        if prev is not None:
            assert (thr >= prev).all(), ev                                    # a smaller evalue never lowers a threshold
        prev = thr
        for q in range(2):
            for c in range(sc.CLASSES):
                if c == 1:
                    continue
                L = 1 if c == 0 else (2 + (c & 1)) << (c // 2 - 1)
                assert sc.length_class(L) == c
                T = int(thr[q, c])
                assert swamd.score_evalue(fit[q], L, T) <= ev < swamd.score_evalue(fit[q], L, T - 1), (ev, q, c, T)
    assert (np.diff(prev[:, 2:], axis=1) >= 0).all()                          # b > 0: longer targets need more


def test_planted_outliers_do_not_move_the_fit(swamd):
    """50 scores of 200 among 4000 null scores.  The bound comes from the planted-free histogram alone: per parameter the spread of its
    own four rounds (restated in numpy).  Seed 3 gives 0.0999 for a, 0.0059 for b and 0.0758 for sigma; the planted scores inflate the
    first round's sigma to about 19, still lie beyond z = 5 and are gone from the second round on, so the planted fit is the
    planted-free fit one round behind: measured, it moves a, b and sigma by 0.0 (the trimming has converged by then)."""
    free, planted = sc.null_hist(3), sc.null_hist(3, planted=50)
    assert int(planted.sum()) == 4050 and (planted - free)[:, 200].sum() == 50
    _, rounds = sc.fit_ref(free, 0)
    bound = [max(r[i] for r in rounds) - min(r[i] for r in rounds) for i in range(3)]
    print("bound a, b, sigma:", bound)
    assert all(b > 0 for b in bound)
    fit = swamd.score_fit(np.stack([free, planted]), 0)
    for i, f in enumerate(("a", "b", "sigma")):
        moved = abs(float(fit[1][f]) - float(fit[0][f]))
        print(f, float(fit[0][f]), float(fit[1][f]), moved)
        assert moved < bound[i], (f, moved, bound[i])
    assert fit[1]["n_db"] == 4050 and fit[1]["n_fit"] <= 4000                 # the planted scores are left out, not censored
    # ... and one untrimmed least-squares round would have been moved far beyond the bound
    w = planted[:, :255].astype(np.float64)
    assert abs((w * np.arange(255)).sum() / w.sum() - (free[:, :255] * np.arange(255.0)).sum() / free[:, :255].sum()) > 1.0


def test_refusals(swamd):
    L = swamd.lib()
    h = sc.null_hist(1)
    fit = np.zeros(1, swamd.SCORE_FIT)
    thr = np.full(sc.CLASSES, sc.P64, np.int64)
    for args in ((None, 1, 0, fit.ctypes.data), (h.ctypes.data, 1, 0, None), (h.ctypes.data, -1, 0, fit.ctypes.data), (h.ctypes.data, 1, -1, fit.ctypes.data),
                 (h.ctypes.data, 1, 17, fit.ctypes.data)):
        assert L.sw_score_fit_hist(*args) == -22 and b"sw_score_fit_hist" in L.sw_last_error(), args
    assert L.sw_score_fit_hist(h.ctypes.data, 1, 0, fit.ctypes.data) == 0 and fit[0]["valid"] == 1
    for args in ((None, 1, 1.0, thr.ctypes.data), (fit.ctypes.data, 1, 1.0, None), (fit.ctypes.data, -1, 1.0, thr.ctypes.data),
                 (fit.ctypes.data, 1, 0.0, thr.ctypes.data), (fit.ctypes.data, 1, -1.0, thr.ctypes.data), (fit.ctypes.data, 1, math.nan, thr.ctypes.data)):
        assert L.sw_score_thresholds(*args) == -22 and (thr == sc.P64).all(), args
    assert math.isnan(L.sw_score_evalue(None, 10, 10))
    assert L.sw_score_fit_hist(h.ctypes.data, 0, 0, fit.ctypes.data) == 0 and L.sw_score_thresholds(fit.ctypes.data, 0, 1.0, thr.ctypes.data) == 0
    assert (thr == sc.P64).all()
