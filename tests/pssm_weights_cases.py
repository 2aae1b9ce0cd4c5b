"""Shared by the tests of the hit weights (test_pssm_weights_host.py, test_pssm_weights_gpu.py, test_pssm_weights_cli_gpu.py): a
restatement of the rule in include/swhip.h (sw_db_pssm_hit_weights) in numpy and Python integers that shares no code with the library,
the host leg through ctypes inside guard words, and the builders of the small cases whose weights are known in closed form.  The
tables themselves -- synthetic, garbage, real -- are those of tests/pssm_hits_cases.py."""
import numpy as np

import pssm_hits_cases as hc
from pssm_hits_cases import D, I, M, QFRONT   # noqa: F401  (re-exported for the tests)

F = 1 << 20
GUARD, POISON32 = 64, 0x55555555


def reference(c, per_hit, include_min):
    """((nq, top) int32 weights, (nq, top) A_r as Python ints, used (nq, top) bool) by the rule of the header."""
    nl, nq, top = len(c.letters), len(c.qoffs) - 1, c.hits.shape[1]
    ntargets = len(c.offs) - 1
    code = np.full(256, -1, np.int64)
    code[c.letters] = np.arange(nl)
    w = np.zeros((nq, top), np.int32)
    A_all = np.zeros((nq, top), object)
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
            assert len(set(jj.tolist())) == len(jj)                        # a walk visits a column at most once
            n[jj, kk] += 1
            pairs[r] = (jj, kk)
        kj = (n > 0).sum(axis=1)
        A = [0] * top
        for r, (jj, kk) in pairs.items():
            m = len(jj)
            T = sum(F // (int(kj[a]) * int(n[a, b])) for a, b in zip(jj.tolist(), kk.tolist()))
            assert T < 2**40
            A[r] = T // m if m else 0
            assert m == 0 or 1 <= A[r] <= F
        U, S = sum(a > 0 for a in A), sum(A)
        assert S <= 2**32 and 2 * per_hit * U * max(A) + S < 2**51
        for r in range(top):
            w[q, r] = min(65535, (2 * per_hit * U * A[r] + S) // (2 * S)) if S > 0 else 0
            A_all[q, r] = A[r]
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
