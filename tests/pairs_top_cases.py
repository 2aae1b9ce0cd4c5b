"""Shared by the tests of the selection from a scored pair list (test_top_pairs_host.py, test_top_pairs_gpu.py, test_top_pairs_cli_gpu.py):
the independent answer in numpy and the builders of synthetic lists.  The rule restated: an entry qualifies when 0 <= query < nq,
0 <= target < nt and max_score >= min_score; row q holds the first `top` qualifying entries of query q by max_score descending, then
target ascending, then list position ascending, as (target, max_pos, max_score); unused entries are (-1, 0, 0)."""
import numpy as np

SCORE_MAX = (1 << 24) - 1           # the largest score a search call can report: the edge of the key's score field
PATTERNS = ("equal", "zero", "ascending", "descending", "four", "edges", "random")


def numpy_top_pairs(pairs, results, nq, nt, top, min_score=0):
    """pairs (n, 2) int64 of (query, target), results (n, 3) int64 of (max_pos, max_score, path_len) -> (hits (nq, top, 3), nhits (nq,)).
    np.lexsort over (position, target, -score) inside every query; nothing of the library is used."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    results = np.asarray(results, np.int64).reshape(-1, 3)
    hits = np.zeros((nq, top, 3), np.int64)
    hits[:, :, 0] = -1
    nhits = np.zeros(nq, np.int64)
    q, t, score = pairs[:, 0], pairs[:, 1], results[:, 1]
    idx = np.nonzero((q >= 0) & (q < nq) & (t >= 0) & (t < nt) & (score >= min_score))[0]
    idx = idx[np.lexsort((idx, t[idx], -score[idx], q[idx]))]             # last key first: query, then the rank order inside it
    lo = np.searchsorted(q[idx], np.arange(nq), "left")
    hi = np.searchsorted(q[idx], np.arange(nq), "right")
    for k in np.nonzero(hi > lo)[0]:
        order = idx[lo[k]:hi[k]][:top]
        n = len(order)
        hits[k, :n, 0] = t[order]
        hits[k, :n, 1] = results[order, 0]
        hits[k, :n, 2] = results[order, 1]
        nhits[k] = n
    return hits, nhits


def pattern_scores(rng, pattern, n):
    """n scores of one of PATTERNS, all inside 0 .. SCORE_MAX."""
    if pattern == "equal":
        return np.full(n, 77, np.int64)
    if pattern == "zero":
        return np.zeros(n, np.int64)
    if pattern == "ascending":
        return np.arange(n, dtype=np.int64)
    if pattern == "descending":
        return np.arange(n, dtype=np.int64)[::-1].copy()
    if pattern == "four":
        return rng.choice(np.array([0, 5, 6, 900], np.int64), n)
    if pattern == "edges":
        return rng.choice(np.array([0, SCORE_MAX], np.int64), n)
    if pattern == "random":
        return rng.integers(0, 5000, n).astype(np.int64)
    raise ValueError(pattern)


def max_pos_of(query, target, nt, extra=0):
    """A max_pos that depends on the PAIR, not on where it lies in the list (a permuted list keeps it), and that no two pairs share;
    `extra` tells duplicates of one pair apart."""
    return 7 + 3 * (np.asarray(query, np.int64) * nt + np.asarray(target, np.int64)) + extra


def synthetic_list(rng, seglens, nt, pattern="random", shuffle=True, last_target=False):
    """A list with seglens[q] entries of query q (len(seglens) queries, or a {query: length} dict), distinct targets inside a query
    (needs nt >= max(seglens)), scores of `pattern` per query, shuffled so that every query's entries are scattered through the list.
    last_target: every non-empty query names target nt - 1 -- with a power of two for nt and a score of 0 that is the item whose key
    is 0.  Returns (pairs (n, 2), results (n, 3))."""
    qs, ts, ss = [], [], []
    for q, n in (seglens.items() if isinstance(seglens, dict) else enumerate(seglens)):
        t = rng.choice(nt, n, replace=False).astype(np.int64)
        if last_target and n and nt - 1 not in t:
            t[rng.integers(n)] = nt - 1
        qs.append(np.full(n, q, np.int64))
        ts.append(t)
        ss.append(pattern_scores(rng, pattern, n))
    q, t, s = (np.concatenate(x) if x else np.zeros(0, np.int64) for x in (qs, ts, ss))
    pairs = np.stack([q, t], axis=1)
    results = np.stack([max_pos_of(q, t, nt), s, np.zeros(len(q), np.int64)], axis=1)
    if shuffle:
        perm = rng.permutation(len(q))
        pairs, results = pairs[perm], results[perm]
    return np.ascontiguousarray(pairs), np.ascontiguousarray(results)


def junk_entries(nq, nt):
    """Entries that must drop out, each with a large score so that a miss shows: the pre-filter's {-1, -1}, an index at its bound, a
    negative index, and 2^32 + a valid index (which a 32-bit compare would let through).  Returns (pairs, results)."""
    big = 1 << 32
    pr = np.array([[-1, -1], [nq, 0], [0, nt], [nq, nt], [-1, 0], [0, -1], [-5, nt - 1], [big + 0, 0], [0, big + 0], [big + nq - 1, nt - 1],
                   [nq - 1, big + nt - 1], [-big, 0], [0, -big]], np.int64)
    res = np.stack([1000 + np.arange(len(pr), dtype=np.int64), np.full(len(pr), SCORE_MAX, np.int64), np.zeros(len(pr), np.int64)], axis=1)
    return pr, res


def with_junk(rng, pairs, results, nq, nt):
    """The list with junk_entries mixed in at random places."""
    jp, jr = junk_entries(nq, nt)
    p, r = np.concatenate([pairs, jp]), np.concatenate([results, jr])
    perm = rng.permutation(len(p))
    return np.ascontiguousarray(p[perm]), np.ascontiguousarray(r[perm])
