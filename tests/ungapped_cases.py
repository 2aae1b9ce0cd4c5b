"""Shared by the pre-filter tests: the independent checker of the ungapped score U (include/swhip.h), a few lines of numpy that share no
code with the library, and the mixed case the host and the GPU tests run.  For a pair the checker forms the score matrix
s[q[:, None], t[None, :]] and, on every diagonal, the running max(0, x + s) (Kadane); U is the highest value any diagonal reaches."""
import functools

import numpy as np

from affine_cases import PROTEIN

QLENS = [1, 4, 255, 256, 257, 512, 513, 1024, 1025, 2049]        # every class (4 / 8 / 16 columns per lane), one strip and several
TLENS = [0, 1, 63, 64, 65, 127, 300, 1100, 64, 0, 1, 300, 65, 127, 63]   # unequal neighbours in the length-sorted schedule
QFRONT, FRONT = 4, 3                                             # qoffsets[0], offsets[0]


def ungapped_score(q, t, sub):
    """U(q, t) under the (256, 256) table sub[query letter][target letter].  Kadane on a diagonal x in closed form: with the prefix sums
    P (P[0] = 0) the running max(0, run + x) at step i is P[i] - min(P[0..i])."""
    q, t = np.asarray(q, np.uint8), np.asarray(t, np.uint8)
    if len(q) == 0 or len(t) == 0:
        return 0
    s = np.asarray(sub, np.int64)[q[:, None], t[None, :]]       # s[j, i]: query letter j against target letter i
    best = 0
    for off in range(-(len(q) - 1), len(t)):
        p = np.concatenate([[0], np.cumsum(np.diagonal(s, off))])
        best = max(best, int((p - np.minimum.accumulate(p)).max()))
    return best


def ungapped_table(qpacked, qoffs, packed, offs, sub):
    """The (nqueries, ntargets) int64 table of U."""
    nq, nt = len(qoffs) - 1, len(offs) - 1
    out = np.zeros((nq, nt), np.int64)
    for a in range(nq):
        for b in range(nt):
            out[a, b] = ungapped_score(qpacked[qoffs[a]:qoffs[a + 1]], packed[offs[b]:offs[b + 1]], sub)
    return out


def passing(table, offs, min_score):
    """The sorted (query, target) pairs with a non-empty target and U >= min_score, as an (n, 2) int64 array."""
    nonempty = np.diff(offs) > 0
    qs, ks = np.nonzero((np.asarray(table) >= min_score) & nonempty[None, :])
    return np.stack([qs, ks], axis=1).astype(np.int64).reshape(-1, 2)


def pack(lens, front, rng, alpha):
    offs = np.zeros(len(lens) + 1, np.int64)
    offs[0] = front
    offs[1:] = front + np.cumsum(lens)
    return rng.choice(alpha, max(1, int(offs[-1]))).astype(np.uint8), offs


def tables(swamd):
    """An asymmetric random table over the protein letters and a match table."""
    rng = np.random.default_rng(5)
    n = len(PROTEIN)
    sc = rng.integers(-8, 13, (n, n)).astype(np.int8)
    sc[np.arange(n), np.arange(n)] = rng.integers(4, 13, n).astype(np.int8)
    assert not np.array_equal(sc, sc.T)
    return {"random": swamd.submat_from_letters(PROTEIN, sc, -8), "match": swamd.submat_match(3, -3)}


@functools.lru_cache(maxsize=None)
def mixed_case():
    """The ten query lengths shuffled against the fifteen targets: (qlens, qpacked, qoffs, packed, offs).  Computed once, never changed."""
    rng = np.random.default_rng(2024)
    qlens = list(QLENS)
    rng.shuffle(qlens)
    qpacked, qoffs = pack(qlens, QFRONT, rng, PROTEIN[:20])
    packed, offs = pack(TLENS, FRONT, rng, PROTEIN[:20])
    return qlens, qpacked, qoffs, packed, offs


_CHECKED = {}


def mixed_checked(which, sub):
    """The checker's table of the mixed case under table `which` of tables(): computed once per process, shared by the tests, read-only."""
    if which not in _CHECKED:
        _, qpacked, qoffs, packed, offs = mixed_case()
        tab = ungapped_table(qpacked, qoffs, packed, offs, sub)
        tab.setflags(write=False)
        _CHECKED[which] = tab
    return _CHECKED[which]
