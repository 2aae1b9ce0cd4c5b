"""Shared by the tests of the query-anchored alignment (test_msa_hits_host.py, test_msa_hits_gpu.py, test_msa_hits_cli_gpu.py): a
pure-Python replay of the rule in include/swhip.h (sw_db_msa_from_hits) -- used entries, the walk, valid inserts, the two layouts --
that shares no code with the library, the builders of the case tables, and the host leg through ctypes on guarded buffers.  The
builders assert that what they build is not vacuous."""
import functools
import types

import numpy as np

from affine_cases import PROTEIN, random_submat
from pssm_hits_cases import homologue_database

DNA = np.frombuffer(b"ACGT", np.uint8)
ALPHABETS = {4: DNA, 20: PROTEIN[:20]}
NOPS = [1, 63, 64, 65, 128, 129, 200]
OPS_CAP = 200
INCLUDE_MIN = 20
GUARD, POISON = 64, 0x55


def replay(qs, qlen, t, qb, tb, ops):
    """One used entry by the rule, op by op -> (column row, A3M row, nmatch, nident, ninsert).  qs: the query's letters or None."""
    col, row, j, i, nm, ni, nins = [ord("-")] * qlen, [ord("-")] * qb, qb, tb, 0, 0, 0
    for op in bytes(ops):
        if op == ord("M") or op == ord("I"):
            pair = op == ord("M") and j < qlen and i < len(t)
            if pair:
                col[j], nm, ni = t[i], nm + 1, ni + (qs is not None and qs[j] == t[i])
            if j < qlen:
                row.append(t[i] if pair else ord("-"))
            j, i = j + 1, i + (op == ord("M"))
        elif op == ord("D"):
            if i < len(t) and j <= qlen:
                row.append(t[i] + 32 if ord("A") <= t[i] <= ord("Z") else t[i])
                nins += 1
            i += 1
    return bytes(col), bytes(row + [ord("-")] * (qlen + nins - len(row))), nm, ni, nins


def reference(c, a3m_cap=None):
    """(cols bytes, rows as a list of (off, len, nmatch, nident, ninsert), a3m bytes of the true total -- or, with a3m_cap, of a3m_cap
    bytes with None where the call leaves the buffer as it was --, total, used (nq, top) bool) by the rule of the header."""
    nq, top = c.hits.shape[:2]
    ntargets = len(c.offs) - 1
    cols, rows, a3m, used = [], [], [], np.zeros((nq, top), bool)
    off = 0
    for q in range(nq):
        g0, qlen = int(c.qoffs[q]), int(c.qoffs[q + 1] - c.qoffs[q])
        qs = None if c.qpacked is None else bytes(c.qpacked[g0:g0 + qlen])
        nh = top if c.nhits is None else min(max(int(c.nhits[q]), 0), top)
        for r in range(top):
            t = int(c.hits[q, r, 0])
            ms, qb, tb, nops = (int(c.aln[q, r, f]) for f in (1, 2, 3, 6))
            ok = r < nh and 0 <= t < ntargets and ms >= c.include_min and 0 < nops <= c.cap
            tg = bytes(c.packed[c.offs[t]:c.offs[t + 1]]) if ok else b""
            ok = ok and 0 <= qb <= qlen and 0 <= tb <= len(tg)
            used[q, r] = ok
            if ok:
                col, row, nm, ni, nins = replay(qs, qlen, tg, qb, tb, c.ops[q * top + r, :nops])
            else:
                col, row, nm, ni, nins = b"-" * qlen, b"", 0, 0, 0
            cols.append(col)
            rows.append((off, len(row), nm, ni, nins))
            a3m.append(row)
            off += len(row)
    if a3m_cap is None:
        return b"".join(cols), rows, b"".join(a3m), off, used
    buf = [None] * a3m_cap
    for (o, n, *_), row in zip(rows, a3m):
        if o + n <= a3m_cap:
            buf[o:o + n] = row
    return b"".join(cols), rows, buf, off, used


def _case(alpha, qlens, targets, top, with_letters=True, front=3, seed=0):
    rng = np.random.default_rng(seed)
    c = types.SimpleNamespace()
    c.qoffs = np.concatenate([[front], front + np.cumsum(qlens)]).astype(np.int64)
    c.qpacked = rng.choice(alpha, int(c.qoffs[-1])).astype(np.uint8) if with_letters else None
    c.offs = np.concatenate([[7], 7 + np.cumsum([len(t) for t in targets])]).astype(np.int64)
    c.packed = np.concatenate([rng.choice(alpha, 7).astype(np.uint8)] + [np.asarray(t, np.uint8) for t in targets])
    nq = len(qlens)
    c.hits = np.zeros((nq, top, 3), np.int64)
    c.nhits = None
    c.aln = np.zeros((nq, top, 7), np.int64)
    c.cap = OPS_CAP
    c.ops = np.full((nq * top, OPS_CAP), 0x5A, np.uint8)
    c.include_min = INCLUDE_MIN
    return c


def _mix(rng, n):
    return rng.choice(np.frombuffer(b"MMMMID", np.uint8), n)


KINDS = len(NOPS) + 15


def synthetic(nalpha, top, qlens=(1, 5, 64, 70, 130), with_letters=True, nhits=False, seed=1):
    """Tables written by hand, kind after kind in turn over the entries: every nops of NOPS; only 'D', only 'I', inserts in front of
    column 0 and behind the last column; q_begin == qlen, t_begin == len; targets -1 and ntargets; max_score one below and at
    include_min_score; nops 0 and ops_cap + 1; a target of lower-case and non-letter bytes; random op bytes.  The query letters are
    drawn so that some pairs are identities.  nhits: counts of 0, negative, above top and inside, in turn over the queries."""
    rng = np.random.default_rng(seed)
    alpha = ALPHABETS[nalpha]
    tlens = [0, 1, 5, 64, 65, 130, 300]
    targets = [rng.choice(alpha, n).astype(np.uint8) for n in tlens]
    odd = np.frombuffer(b"acgt*-.\x00\xff\x7fxyz[@`{AZ", np.uint8)
    targets.append(rng.choice(odd, 90).astype(np.uint8))          # lower-case and non-letter target bytes
    ODD = len(targets) - 1
    c = _case(alpha, list(qlens), targets, top, with_letters, seed=seed)
    nq, seen = len(qlens), set()
    for n, (q, r) in enumerate((q, r) for q in range(nq) for r in range(top)):
        kind = (n + q) % KINDS                                    # (+ q: a query's entries do not start at the same kind)
        qlen = int(qlens[q])
        t = int(rng.integers(3, len(tlens)))
        score, qb, tb = INCLUDE_MIN + int(rng.integers(0, 50)), 0, 0
        if kind < len(NOPS):
            o = _mix(rng, NOPS[kind])
            qb, tb = int(rng.integers(0, qlen)), int(rng.integers(0, 20))
        elif kind == len(NOPS):
            o = np.full(10, ord("D"), np.uint8)
        elif kind == len(NOPS) + 1:
            o = np.full(10, ord("I"), np.uint8)
        elif kind == len(NOPS) + 2:                               # inserts in front of column 0
            o = np.frombuffer(b"DDD" + b"M" * min(qlen, 40), np.uint8)
        elif kind == len(NOPS) + 3:                               # ... and behind the last column: the 'M's end exactly at qlen
            qb = max(0, qlen - 30)
            o = np.frombuffer(b"M" * (qlen - qb) + b"DDDD", np.uint8)
        elif kind == len(NOPS) + 4:
            qb, o = qlen, np.frombuffer(b"DDMID", np.uint8)       # q_begin == qlen: inserts behind the last column only
        elif kind == len(NOPS) + 5:
            tb, o = len(targets[t]), _mix(rng, 30)                # t_begin == len: nothing pairs, nothing is inserted
        elif kind == len(NOPS) + 6:
            t, o = -1, _mix(rng, 30)
        elif kind == len(NOPS) + 7:
            t, o = len(targets), _mix(rng, 30)
        elif kind == len(NOPS) + 8:
            score, o = INCLUDE_MIN - 1, _mix(rng, 30)
        elif kind == len(NOPS) + 9:
            score, o = INCLUDE_MIN, _mix(rng, 30)
        elif kind == len(NOPS) + 10:
            o = np.zeros(0, np.uint8)                             # nops 0
        elif kind == len(NOPS) + 11:
            o = _mix(rng, OPS_CAP)                                # nops = ops_cap + 1 (set below)
        elif kind == len(NOPS) + 12:
            t, o = ODD, _mix(rng, 80)
        elif kind == len(NOPS) + 13:
            o = rng.integers(0, 256, 150).astype(np.uint8)        # op rows of random bytes
        else:                                                     # a walk that runs past qlen and past len
            t, o = 2, np.full(OPS_CAP, ord("M"), np.uint8)
        c.hits[q, r] = (t, 0, score)
        c.aln[q, r] = (0, score, qb, tb, 0, 0, len(o) + (kind == len(NOPS) + 11))
        c.ops[q * top + r, :len(o)] = o
        seen.add(kind)
        # identities: the query repeats what the first ops pair it with
        if c.qpacked is not None and 0 <= t < len(targets) and kind < len(NOPS) and r % 2 == 0:
            k = min(qlen - qb, len(targets[t]) - tb, 8)
            if k > 0:
                c.qpacked[c.qoffs[q] + qb:c.qoffs[q] + qb + k] = targets[t][tb:tb + k]
    if nhits:
        c.nhits = np.array([(0, -5, top + 7, max(1, top - 1), top)[q % 5] for q in range(nq)], np.int64)
    if nq * top >= KINDS + nq:
        assert len(seen) == KINDS
        _, rows, _, _, used = reference(c)
        assert used.any() and not used.all()
        if nhits is False:
            assert any(w[4] > 0 for w in rows) and any(w[2] > 0 for w in rows)
            assert c.qpacked is None or any(0 < w[3] for w in rows)
    return c


def garbage(seed, nalpha=20, top=40):
    """Op rows of random bytes and alignment entries of random int64 (a part of them with small fields, so that some pass the guards)."""
    rng = np.random.default_rng(seed)
    c = synthetic(nalpha, top, seed=seed)
    nq = c.hits.shape[0]
    c.ops = rng.integers(0, 256, c.ops.shape).astype(np.uint8)
    c.ops[::2] = rng.choice(np.frombuffer(b"MID\x00Z", np.uint8), c.ops[::2].shape)
    c.aln = rng.integers(-2**63, 2**63 - 1, c.aln.shape, dtype=np.int64)
    small = rng.random((nq, top)) < 0.6
    k = int(small.sum())                                          # (max_pos, max_score, q_begin, t_begin, q_end, t_end, nops) around the guards
    c.aln[small] = np.stack([rng.integers(lo, hi, k) for lo, hi in ((-3, 9), (0, 80), (-1, 72), (-1, 72), (-3, 9), (-3, 9), (-1, OPS_CAP + 3))], axis=-1)
    c.hits = rng.integers(-2**63, 2**63 - 1, c.hits.shape, dtype=np.int64)
    c.hits[:, :, 0] = np.where(rng.random((nq, top)) < 0.7, rng.integers(-1, len(c.offs), (nq, top)), c.hits[:, :, 0])
    c.nhits = rng.integers(-3, top + 3, nq).astype(np.int64)
    used = reference(c)[4]
    assert used.any() and not used.all()
    return c


def long_ops_case(seed=5, nops=3000):
    """One query of 700 columns against targets of 2500 letters, alignments of up to `nops` ops in which runs of 'D' push a row's
    inserts across many 64-op rounds."""
    rng = np.random.default_rng(seed)
    alpha = ALPHABETS[20]
    targets = [rng.choice(alpha, 2500).astype(np.uint8) for _ in range(3)]
    c = _case(alpha, [700], targets, 6, seed=seed)
    c.cap = nops
    c.ops = np.full((6, nops), 0x5A, np.uint8)
    for r in range(6):
        n = (nops, nops - 1, 2049, 1000, nops, 130)[r]
        o = rng.choice(np.frombuffer(b"MMMDDDDI", np.uint8), n) if r != 4 else np.tile(np.frombuffer(b"M" + b"D" * 70, np.uint8), n // 71 + 1)[:n]
        c.hits[0, r] = (r % 3, 0, 99)
        c.aln[0, r] = (0, 99, r, 3 * r, 0, 0, n)
        c.ops[r, :n] = o
    rows = reference(c)[1]
    assert max(w[4] for w in rows) > 1000
    return c


@functools.lru_cache(maxsize=None)
def real(swamd, nalpha=20, top=8, seed=3, qlens=(33, 64, 150)):
    """Real tables on the host: sequence queries through sw_search_affine_multi_top_host and sw_align_affine_hits_host over a database
    with planted homologues.  Shared: the tests leave it unchanged."""
    rng = np.random.default_rng(seed)
    alpha = ALPHABETS[nalpha]
    queries = [rng.choice(alpha, n).astype(np.uint8) for n in qlens]
    packed, offs = homologue_database(rng, queries, 30, alpha=alpha)
    sub = swamd.submat_match(5, -4) if nalpha == 4 else np.minimum(random_submat(rng, lo=-6, hi=8), random_submat(rng, lo=-6, hi=8).T)
    if nalpha != 4:
        sub[np.arange(256), np.arange(256)] = 9
    scoring = (sub, -8, -1)
    c = types.SimpleNamespace()
    c.sub, c.scoring, c.queries = sub, scoring, queries
    c.qoffs = np.concatenate([[0], np.cumsum(qlens)]).astype(np.int64)
    c.qpacked = np.concatenate(queries)
    c.packed, c.offs = packed, offs
    c.hits, c.nhits = swamd.search_affine_multi_top_host(queries, (packed, offs), scoring, top, 1)
    c.aln, ops = swamd.align_affine_hits_host(queries, (packed, offs), scoring, c.hits, c.nhits)
    c.cap = max(1, max(qlens) + int(np.diff(offs).max()))
    c.ops = np.full((len(qlens) * top, c.cap), 0x5A, np.uint8)
    for q, row in enumerate(ops):
        for r, b in enumerate(row):
            c.ops[q * top + r, :len(b)] = np.frombuffer(b, np.uint8)
    c.include_min = int(np.percentile(c.aln[:, :, 1], 30))
    _, rows, _, _, used = reference(c)
    assert used.any() and not used.all() and any(w[4] > 0 for w in rows) and any(w[3] > 0 for w in rows)
    return c


def host_leg(swamd, c, want_cols=True, want_rows=True, want_a3m=True, a3m_cap=None, null_queries=False):
    """sw_msa_from_hits_host through ctypes on buffers with guard bytes around them: asserts SW_OK and that nothing outside the outputs
    changed.  Returns (cols bytes or None, rows as a list of tuples or None, the a3m_cap bytes of the A3M buffer as int16 with -1 where the
    poison stayed -- or None --, total or None)."""
    L = swamd.lib()
    nq, top = c.hits.shape[:2]
    ncols = int(c.qoffs[-1] - c.qoffs[0]) * top
    if a3m_cap is None:
        a3m_cap = reference(c)[3]
    cols = np.full(GUARD + ncols + GUARD, POISON, np.uint8)
    rows = np.full(GUARD + nq * top * 24 + GUARD, POISON, np.uint8)
    a3m = np.full(GUARD + a3m_cap + GUARD, POISON, np.uint8)
    total = np.full(3, 0x5555555555555555, np.int64)
    hits, aln, ops = np.ascontiguousarray(c.hits), np.ascontiguousarray(c.aln), np.ascontiguousarray(c.ops)
    qp = None if (c.qpacked is None or null_queries) else np.ascontiguousarray(c.qpacked)
    rc = L.sw_msa_from_hits_host(qp.ctypes.data if qp is not None else None, c.qoffs.ctypes.data, nq, c.packed.ctypes.data, c.offs.ctypes.data,
                                 len(c.offs) - 1, c.include_min, hits.ctypes.data, c.nhits.ctypes.data if c.nhits is not None else None, top,
                                 aln.ctypes.data, ops.ctypes.data, c.cap, cols[GUARD:].ctypes.data if want_cols else None,
                                 rows[GUARD:].ctypes.data if want_rows else None, a3m[GUARD:].ctypes.data if want_a3m else None, a3m_cap,
                                 total[1:].ctypes.data if want_rows else None)
    assert rc == 0, L.sw_last_error().decode()
    return check_guards(swamd, cols, rows, a3m, total, ncols, nq * top, a3m_cap, want_cols, want_rows, want_a3m)


def check_guards(swamd, cols, rows, a3m, total, ncols, n, a3m_cap, want_cols, want_rows, want_a3m):
    """The guards of host_leg's layout (numpy arrays, from the host or the device), then the outputs as host_leg returns them."""
    assert (cols[:GUARD] == POISON).all() and (cols[GUARD + ncols:] == POISON).all(), "the column rows were written outside their buffer"
    assert (rows[:GUARD] == POISON).all() and (rows[GUARD + 24 * n:] == POISON).all(), "the row table was written outside its buffer"
    assert (a3m[:GUARD] == POISON).all() and (a3m[GUARD + a3m_cap:] == POISON).all(), "the A3M rows were written outside their buffer"
    assert total[0] == total[2] == 0x5555555555555555
    if not want_cols:
        assert (cols == POISON).all()
    if not want_rows:
        assert (rows == POISON).all() and total[1] == 0x5555555555555555
    if not want_a3m:
        assert (a3m == POISON).all()
    out_rows = [tuple(int(x) for x in w) for w in rows[GUARD:GUARD + 24 * n].copy().view(swamd.MSA_ROW)] if want_rows else None
    out_a3m = None
    if want_a3m:                               # int16: a byte of a written row, -1 where the call left the buffer alone (its poison is checked)
        body = a3m[GUARD:GUARD + a3m_cap]
        written = np.zeros(a3m_cap, bool)
        for o, ln, *_ in out_rows:
            if 0 <= o and o + ln <= a3m_cap:
                written[o:o + ln] = True
        assert (body[~written] == POISON).all(), "A3M bytes outside every written row changed"
        out_a3m = np.where(written, body.astype(np.int16), -1)
    return (bytes(cols[GUARD:GUARD + ncols]) if want_cols else None, out_rows, out_a3m, int(total[1]) if want_rows else None)


def same(got, exp):
    """Two results of host_leg's shape, byte for byte."""
    return got[0] == exp[0] and got[1] == exp[1] and got[3] == exp[3] and (got[2] is None) == (exp[2] is None) and (got[2] is None or np.array_equal(got[2], exp[2]))


def assert_matches_reference(c, got, a3m_cap=None, null_queries=False):
    """got: what host_leg / the device leg return, against reference(c) at the same cap."""
    cols, rows, a3m, total = got
    ref = c if not null_queries else types.SimpleNamespace(**{**vars(c), "qpacked": None})
    full = reference(ref)
    cap = full[3] if a3m_cap is None else a3m_cap
    rcols, rrows, ra3m, rtotal, _ = reference(ref, cap)
    if cols is not None:
        assert cols == rcols
    if rows is not None:
        assert rows == rrows and total == rtotal
    if a3m is not None:
        assert np.array_equal(a3m, np.array([-1 if x is None else x for x in ra3m], np.int16))
