"""CPU: what the mask is for, on host legs only.  The null database of tests/test_score_stats_calibration_host.py -- 4000 targets of
i.i.d. letters, lengths log-normal -- with a Q-rich stretch (40 letters, 70 % Q) planted in 40 of them, and one query of 150 letters
with such a stretch of its own; nothing else relates them.  Searched plain (search_affine_multi_host for the table of the histogram,
search_affine_multi_top_host for the hits, score_hist_host, score_fit, score_evalue), the biased targets are the outliers the trimmed
fit leaves out of the null line, and they get tiny E-values; searched after mask_low_complexity_host on the database AND the query,
none of them does, while fewer than 3 % of the letters of the null targets are masked.

Measured with this file's seed (1): plain, 40 of the 40 planted targets have E <= 1e-3 and no null target has; masked, 0 of 40 and
no null target; 4975 of the 702 894 letters of the null targets are masked (0.71 %), 54 of the query's 150, and every planted target
has masked letters.  Seeds 2 and 3: 39 of 40 plain, 0 masked, 0.65 % and 0.80 %."""
import math

import numpy as np

import score_stats_cases as sc

LETTERS = b"ACDEFGHIKLMNPQRSTVWY"
SEED, PLANTED, STRETCH, TOP = 1, 40, 40, 64


def test_masking_takes_the_biased_targets_out_of_the_significant_hits(swamd):
    rng = np.random.default_rng(SEED)
    p = rng.dirichlet(np.full(20, 30.0))
    m = 0.3
    odds = (1 - m) + m * np.eye(20) / p[:, None]
    S = np.rint(2 * np.log2(odds)).astype(np.int64)                           # half-bits, as in the calibration of the E-values
    lens = np.clip(np.exp(rng.normal(math.log(150), 0.6, 4000)).astype(np.int64), 20, 800)
    alphabet = np.frombuffer(LETTERS, np.uint8)
    targets = [alphabet[rng.choice(20, int(n), p=p)].copy() for n in lens]

    def stretch():
        s = alphabet[rng.choice(20, STRETCH, p=p)].copy()
        s[rng.random(STRETCH) < 0.7] = ord("Q")
        return s

    planted = rng.choice(np.nonzero(lens >= 2 * STRETCH)[0], PLANTED, replace=False)
    for k in planted:
        at = int(rng.integers(0, lens[k] - STRETCH + 1))
        targets[k][at:at + STRETCH] = stretch()
    query = alphabet[rng.choice(20, 150, p=p)].copy()
    query[55:55 + STRETCH] = stretch()
    sub = swamd.submat_from_letters(LETTERS, S, int(S.min()))                 # a masked letter scores the table's smallest entry
    offs = sc.offsets_of(lens)
    scoring = (sub, -11, -1)
    is_planted = np.zeros(4000, bool)
    is_planted[planted] = True

    masked_db, nmasked = swamd.mask_low_complexity_host((np.concatenate(targets), offs))
    masked_q, qmasked = swamd.mask_low_complexity_host([query.tobytes()])
    null_fraction = nmasked[~is_planted].sum() / lens[~is_planted].sum()

    significant = {}
    for name, q, db in (("plain", query, np.concatenate(targets)), ("masked", masked_q, masked_db)):
        res = swamd.search_affine_multi_host([q], (db, offs), scoring)
        fit = swamd.score_fit(swamd.score_hist_host(res, offs, 0), 0)
        assert fit["valid"][0] == 1 and fit["n_db"][0] == 4000
        hits, nhits = swamd.search_affine_multi_top_host([q], (db, offs), scoring, TOP, 1)
        sig = [int(t) for t, _, score in hits[0, :int(nhits[0])] if swamd.score_evalue(fit[0:1], int(lens[t]), int(score)) <= 1e-3]
        # the hit list is long enough to hold every significant target: the last hit is not significant
        t, _, score = hits[0, int(nhits[0]) - 1]
        assert swamd.score_evalue(fit[0:1], int(lens[t]), int(score)) > 1e-3
        significant[name] = (int(is_planted[sig].sum()), int((~is_planted[sig]).sum()))
    print("planted / null targets with E <= 1e-3:", significant, "null letters masked:", int(nmasked[~is_planted].sum()), "of", int(lens[~is_planted].sum()),
          "query letters masked:", int(qmasked[0]), "planted targets with masked letters:", int((nmasked[planted] > 0).sum()))
    assert significant["plain"][0] >= PLANTED // 2
    assert significant["masked"][0] == 0
    assert null_fraction < 0.03
