"""Shared by the tests of the hit weights (test_pssm_weights_host.py, test_pssm_weights_gpu.py, test_pssm_weights_cli_gpu.py): a
restatement of the rule in include/swhip.h (sw_db_pssm_hit_weights) in numpy and Python integers that shares no code with the library,
the host leg through ctypes inside guard words, and the builders of the small cases whose weights are known in closed form.  The
tables themselves -- synthetic, garbage, real -- are those of tests/pssm_hits_cases.py."""
import functools

import numpy as np

import pssm_hits_cases as hc
from pssm_hits_cases import D, I, M, QFRONT   # noqa: F401  (re-exported for the tests)

F = 1 << 20
GUARD, POISON32 = 64, 0x55555555


def accumulators(c, include_min, code=None):
    """(T_r, m_r, used), each (nq, top): the sum of an entry's terms and the number of its counted pairs, as Python integers.  code: 256
    places to take in the place of the letters' own (as in pssm_hits_cases.reference): what a call would sum had it read another call's
    code table."""
    nl, nq, top = len(c.letters), len(c.qoffs) - 1, c.hits.shape[1]
    ntargets = len(c.offs) - 1
    if code is None:
        code = np.full(256, -1, np.int64)
        code[c.letters] = np.arange(nl)
    else:
        code = np.where((np.asarray(code, np.int64) >= 0) & (np.asarray(code, np.int64) < nl), np.asarray(code, np.int64), -1)
    T_all, m_all = np.zeros((nq, top), object), np.zeros((nq, top), object)
    used = np.zeros((nq, top), bool)
    for q in range(nq):
        qlen = int(c.qoffs[q + 1] - c.qoffs[q])
        nh = top if c.nhits is None else int(np.clip(c.nhits[q], 0, top))
        n = np.zeros((qlen, nl), np.int64)
        pairs = {}
        for r in range(nh):
            t = int(c.hits[q, r, 0])
            if not 0 <= t < ntargets:
                continue
            ms, qb, tb, nops = (int(c.aln[q, r, f]) for f in (1, 2, 3, 6))
            if ms < include_min or not 0 < nops <= c.cap:
                continue
            ln = int(c.offs[t + 1] - c.offs[t])
            if not (0 <= qb <= qlen and 0 <= tb <= ln):
                continue
            used[q, r] = True
            o = c.ops[q * top + r, :nops]
            is_m = o == M
            cq, ct = is_m | (o == I), is_m | (o == D)
            j, i = qb + np.cumsum(cq) - cq, tb + np.cumsum(ct) - ct        # where every op stands before it consumes anything
            pair = is_m & (j < qlen) & (i < ln)
            k = code[c.packed[c.offs[t] + i[pair]]]
            jj, kk = j[pair][k >= 0], k[k >= 0]
            assert len(np.unique(jj)) == len(jj)                           # a walk visits a column at most once
            n[jj, kk] += 1
            pairs[r] = (jj, kk)
        kj = (n > 0).sum(axis=1)
        for r, (jj, kk) in pairs.items():
            T = int((F // (kj[jj] * n[jj, kk])).sum())                     # (int64: every term <= 2^20, at most 2^20 of them)
            assert T < 2**40
            T_all[q, r], m_all[q, r] = T, len(jj)
    return T_all, m_all, used


def weights_of(T_all, m_all, per_hit):
    """((nq, top) int32 weights, (nq, top) A_r) from the entries' T_r and m_r by the last lines of the rule."""
    nq, top = T_all.shape
    w = np.zeros((nq, top), np.int32)
    A_all = np.zeros((nq, top), object)
    for q in range(nq):
        A = [int(T) // int(m) if m else 0 for T, m in zip(T_all[q], m_all[q])]
        assert all(m == 0 or 1 <= a <= F for a, m in zip(A, m_all[q]))
        U, S = sum(a > 0 for a in A), sum(A)
        assert S <= 2**32 and 2 * per_hit * U * max(A) + S < 2**51
        for r in range(top):
            w[q, r] = min(65535, (2 * per_hit * U * A[r] + S) // (2 * S)) if S > 0 else 0
            A_all[q, r] = A[r]
    return w, A_all


def reference(c, per_hit, include_min, code=None):
    """((nq, top) int32 weights, (nq, top) A_r as Python ints, used (nq, top) bool) by the rule of the header."""
    T_all, m_all, used = accumulators(c, include_min, code)
    w, A_all = weights_of(T_all, m_all, per_hit)
    return w, A_all, used


def host_leg(swamd, c, per_hit, include_min):
    """sw_pssm_hit_weights_host through ctypes on an output inside guard words and pre-filled with poison: asserts SW_OK, that the guards
    are whole and that every entry was written.  Returns the (nq, top) int32 weights."""
    import ctypes
    L = swamd.lib()
    lt, sc = swamd._pssm_scoring(hc.scoring(c))
    wt = swamd._pssm_weighting((per_hit, include_min))
    nq, top = len(c.qoffs) - 1, c.hits.shape[1]
    out = np.full(GUARD + nq * top + GUARD, POISON32, np.int32)
    hits, aln, ops = np.ascontiguousarray(c.hits), np.ascontiguousarray(c.aln), np.ascontiguousarray(c.ops)
    rc = L.sw_pssm_hit_weights_host(c.qoffs.ctypes.data, nq, c.packed.ctypes.data, c.offs.ctypes.data, len(c.offs) - 1, ctypes.byref(sc), ctypes.byref(wt),
                                    hits.ctypes.data, c.nhits.ctypes.data if c.nhits is not None else None, top, aln.ctypes.data, ops.ctypes.data, c.cap,
                                    out[GUARD:].ctypes.data)
    assert rc == 0, L.sw_last_error().decode()
    assert (out[:GUARD] == POISON32).all() and (out[GUARD + nq * top:] == POISON32).all(), "the weights were written outside their buffer"
    w = out[GUARD:GUARD + nq * top].reshape(nq, top).copy()
    assert (w != POISON32).all(), "an entry was not written"
    return w


def sequences_case(seqs, letters=hc.PROTEIN[:20], ncols=None, other_queries=()):
    """One query (the first; other_queries: further (ncols, seqs) queries behind it) whose entry r is sequence seqs[r] paired with the
    columns 0 .. len - 1 through len 'M': a gapless multiple alignment, written as a hit table over a database of those sequences.
    All queries share one `top`: the longest list; the entries behind a shorter list are past its nhits."""
    rng = np.random.default_rng(len(seqs))
    queries = [(ncols or max(len(s) for s in seqs), seqs)] + list(other_queries)
    top = max(len(s) for _, s in queries)
    targets = [np.asarray(s, np.uint8) for _, ss in queries for s in ss]
    offs = np.concatenate([[7], 7 + np.cumsum([len(t) for t in targets])]).astype(np.int64)
    packed = np.concatenate([rng.integers(0, 256, 7).astype(np.uint8)] + targets)
    c = hc._case(rng, letters, 11, [n for n, _ in queries], packed, offs, top)
    c.cap = max(len(t) for t in targets)
    c.ops = np.full((len(queries) * top, c.cap), 0x5A, np.uint8)
    c.nhits = np.array([len(ss) for _, ss in queries], np.int64)
    t = 0
    for q, (_, ss) in enumerate(queries):
        for r, s in enumerate(ss):
            c.hits[q, r] = (t, 0, 0)
            c.aln[q, r] = (0, 50, 0, 0, 0, 0, len(s))
            c.ops[q * top + r, :len(s)] = M
            t += 1
    return c


def device_tables(engine, c):
    """(hits, nhits or None, aln, ops) of a case as torch tensors on the engine's device."""
    t, dev = engine.torch, f"cuda:{engine.device}"
    return (t.from_numpy(np.ascontiguousarray(c.hits)).to(dev), t.from_numpy(c.nhits.copy()).to(dev) if c.nhits is not None else None,
            t.from_numpy(np.ascontiguousarray(c.aln)).to(dev), t.from_numpy(np.ascontiguousarray(c.ops)).to(dev))


# ---- the call at its full size (test_pssm_full_size_host.py, test_pssm_full_size_gpu.py) ----

LMAX = (1 << 20) - 1                       # SW_MAX_DIM: the longest query


@functools.lru_cache(maxsize=None)
def field_case(second=True):
    """One query of LMAX columns over 4 letters, smax 15 (15 x LMAX < 2^24), top = 2.  Entry 0: a target of LMAX letters paired with every
    column through LMAX 'M' from (0, 0).  Entry 1 (second): a 3-letter target, 'MMM' from column 5, whose letters differ from entry 0's
    at the columns 5, 6, 7 -- those three columns hold two letters once each (k_j = 2, terms 2^19), every other one letter once (2^20):
        T_0 = (LMAX - 3) 2^20 + 3 x 2^19,  A_0 = floor(T_0 / LMAX) = 2^20 - 2,  T_1 = 3 x 2^19,  A_1 = 2^19.
    Without the second entry (nhits = 1) T_0 = LMAX x 2^20 = 2^40 - 2^20: every bit of the accumulator's 40-bit field that can be set.
    (case, T, A) with T and A by these closed forms, for the tests to hold the numpy rule to; built once, and left unchanged."""
    rng = np.random.default_rng(40 + second)
    letters = np.frombuffer(b"ACGT", np.uint8)
    long_t = rng.choice(letters, LMAX).astype(np.uint8)
    short_t = np.array([letters[(list(letters).index(x) + 1 + n) % 4] for n, x in enumerate(long_t[5:8])], np.uint8)
    assert (short_t != long_t[5:8]).all()
    offs = np.array([7, 7 + LMAX, 7 + LMAX + 3], np.int64)
    packed = np.concatenate([rng.integers(0, 256, 7).astype(np.uint8), long_t, short_t])
    c = hc._case(rng, letters, 15, [LMAX], packed, offs, 2)
    assert c.smax * min(LMAX, int(np.diff(offs).max())) < 2**24
    c.cap = LMAX
    c.ops = np.full((2, LMAX), 0x5A, np.uint8)
    c.ops[0, :] = M
    c.ops[1, :3] = M
    c.hits[0, :, 0] = (0, 1)
    c.aln[0, 0] = (0, 50, 0, 0, 0, 0, LMAX)
    c.aln[0, 1] = (0, 50, 5, 0, 0, 0, 3)
    c.nhits = np.array([2 if second else 1], np.int64)
    if second:
        T = [(LMAX - 3) * F + 3 * (F // 2), 3 * (F // 2)]
        A = [F - 2, F // 2]
        assert [T[0] // LMAX, T[1] // 3] == A and T[0] >> 30 and T[0] < 2**40
    else:
        T, A = [LMAX * F, 0], [F, 0]
        assert T[0] == 2**40 - 2**20                       # the largest value the field can hold: its top twenty bits are all set
    return c, T, A


def shares(A, per_hit):
    """The weights of one query from its A_r by the header's last line, in Python integers."""
    U, S = sum(a > 0 for a in A), sum(A)
    return [min(65535, (2 * per_hit * U * a + S) // (2 * S)) if S else 0 for a in A]


def sum_case(sibling=False):
    """top = 4096 over a query of 4096 columns and 4 letters: entry r is one 'M' alone on column r (target r % 4, one letter), so every
    column holds one letter once, every A_r = 2^20, U = 4096 and SUM = 2^32 exactly: every weight is per_hit.  sibling: entry 1 moves
    onto column 0 beside entry 0, with another letter: A_0 = A_1 = 2^19, SUM = 2^32 - 2^20.  (case, A)"""
    rng = np.random.default_rng(4096 + sibling)
    letters = np.frombuffer(b"ACGT", np.uint8)
    top = 4096
    offs = np.arange(7, 12, dtype=np.int64)
    packed = np.concatenate([rng.integers(0, 256, 7).astype(np.uint8), letters])
    c = hc._case(rng, letters, 11, [top], packed, offs, top)
    c.cap = 3
    c.ops = np.full((top, 3), 0x5A, np.uint8)
    c.ops[:, 0] = M
    c.hits[0, :, 0] = np.arange(top) % 4
    c.aln[0, :] = (0, 50, 0, 0, 0, 0, 1)
    c.aln[0, :, 2] = np.arange(top)
    A = [F] * top
    if sibling:
        c.aln[0, 1, 2] = 0
        A[0] = A[1] = F // 2
    assert sum(A) == (2**32 - 2**20 if sibling else 2**32)
    return c, A
