"""Shared by the tests of the per-query selection (test_search_top_host.py, test_search_top_gpu.py, test_search_top_cli_gpu.py): the
independent answer in numpy and the builders of the mixed cases.  The rule restated: of the targets with max_score >= min_score, the first
`top` by max_score descending, then target ascending; unused entries are (-1, 0, 0)."""
import numpy as np

from affine_cases import PROTEIN

SCORE_MAX = (1 << 24) - 1           # the largest score a search call can report: the edge of the key's score field


def numpy_top(results, top, min_score=0):
    """results: (nq, nt, 3) int64 of (max_pos, max_score, path_len) -> (hits (nq, top, 3) of (target, max_pos, max_score), nhits (nq,)).
    np.lexsort per row with the min_score filter; nothing of the library is used."""
    results = np.asarray(results, np.int64)
    nq, nt = results.shape[0], results.shape[1]
    hits = np.zeros((nq, top, 3), np.int64)
    hits[:, :, 0] = -1
    nhits = np.zeros(nq, np.int64)
    for q in range(nq):
        score = results[q, :, 1]
        index = np.arange(nt)
        order = np.lexsort((index, -score))
        order = order[score[order] >= min_score][:top]
        n = len(order)
        hits[q, :n, 0] = order
        hits[q, :n, 1] = results[q, order, 0]
        hits[q, :n, 2] = results[q, order, 1]
        nhits[q] = n
    return hits, nhits


def table_of(scores):
    """A synthetic result table from (nq, nt) scores: max_pos is a function of the position that no two entries share, path_len 0."""
    scores = np.asarray(scores, np.int64)
    nq, nt = scores.shape
    res = np.zeros((nq, nt, 3), np.int64)
    res[:, :, 1] = scores
    res[:, :, 0] = 7 + 3 * np.arange(nq * nt, dtype=np.int64).reshape(nq, nt)
    return res


def mixed_case(rng, qlens, tlens, qfront=5, front=3):
    """(qpacked, qoffs, packed, offs) of random protein letters, both offset arrays starting above 0."""
    qoffs = np.zeros(len(qlens) + 1, np.int64)
    qoffs[0] = qfront
    qoffs[1:] = qfront + np.cumsum(qlens)
    offs = np.zeros(len(tlens) + 1, np.int64)
    offs[0] = front
    offs[1:] = front + np.cumsum(tlens)
    return rng.choice(PROTEIN, int(qoffs[-1])).astype(np.uint8), qoffs, rng.choice(PROTEIN, max(1, int(offs[-1]))).astype(np.uint8), offs


MIXED_QLENS = [1, 4, 255, 256, 257, 513]
MIXED_TLENS = [0, 1, 63, 64, 65, 0, 127, 300, 1, 90, 64, 300, 17]
