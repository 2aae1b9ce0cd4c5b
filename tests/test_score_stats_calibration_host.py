"""CPU: the statistical claim.  A null database -- 4000 targets of i.i.d. letters from a 20-letter background, lengths log-normal (median
150, sigma 0.6, clipped to 20..800) -- is searched with two queries of 120 and two of 300 letters from the same background under a
log-odds table in half-bits with a negative expected score and gaps -11 / -1 (search_affine_multi_host).  The scores go through
score_hist_host, score_fit and score_thresholds; for evalue = 100 the number of targets at or above their class threshold must lie in
[50, 200] for every query: the E-value is right to a factor of 2, held against the search's own scores.

Measured with this file's seeds (1 and 7), the four queries each: evalue 100 -> 93..119 targets, 10 -> 9..12, 1 -> 0..2;
b = 1.05..1.19 per half octave, sigma = 3.55..3.79."""
import math

import numpy as np
import pytest

import score_stats_cases as sc

LETTERS = b"ACDEFGHIKLMNPQRSTVWY"


def null_search(swamd, seed):
    rng = np.random.default_rng(seed)
    p = rng.dirichlet(np.full(20, 30.0))                                      # a background near uniform, no letter rarer than ~2 %
    m = 0.3                                                                    # q_ij = m p_i [i == j] + (1 - m) p_i p_j: symmetric, sums to 1
    odds = (1 - m) + m * np.eye(20) / p[:, None]
    S = np.rint(2 * np.log2(odds)).astype(np.int64)                           # half-bits
    assert (p[:, None] * p[None, :] * S).sum() < 0 and S.max() > 0
    lens = np.clip(np.exp(rng.normal(math.log(150), 0.6, 4000)).astype(np.int64), 20, 800)
    alphabet = np.frombuffer(LETTERS, np.uint8)
    targets = [alphabet[rng.choice(20, int(L), p=p)] for L in lens]
    queries = [alphabet[rng.choice(20, L, p=p)] for L in (120, 120, 300, 300)]
    sub = swamd.submat_from_letters(LETTERS, S, int(S.min()))
    res = swamd.search_affine_multi_host(queries, targets, (sub, -11, -1))
    return res, sc.offsets_of(lens), lens


@pytest.mark.parametrize("seed", [1, 7])
def test_evalue_100_keeps_50_to_200_of_4000_null_targets(swamd, seed):
    res, offs, lens = null_search(swamd, seed)
    hist = swamd.score_hist_host(res, offs, 0)
    fit = swamd.score_fit(hist, 0)
    cls = np.array([sc.length_class(int(L)) for L in lens])
    counts = {}
    for ev in (100.0, 10.0, 1.0):
        thr = swamd.score_thresholds(fit, ev)
        counts[ev] = [int((res[q, :, 1] >= thr[q, cls]).sum()) for q in range(4)]
    print("seed", seed, "counts", counts, "b", fit["b"].round(3).tolist(), "sigma", fit["sigma"].round(3).tolist())
    assert (fit["valid"] == 1).all() and (fit["n_db"] == 4000).all() and (fit["n_censored"] == 0).all()
    assert all(50 <= n <= 200 for n in counts[100.0]), counts
