"""Shared by the tests of the PSSM update (test_pssm_hits_host.py, test_pssm_hits_gpu.py, test_pssm_hits_cli_gpu.py): a numpy
restatement of the rule in include/swhip.h (sw_db_pssm_from_hits) -- used entries, the walk, weights, counts, round half up with floor
division -- that shares no code with the library, and the builders of the cases: synthetic tables that put ops on every side of a
64-op chunk, garbage tables, and real tables from the host legs of the search and the alignment over a database with planted
homologues.  The builders assert that what they build is not vacuous."""
import functools
import types

import numpy as np

from affine_cases import PROTEIN, random_submat

QLENS = [1, 63, 64, 65, 257, 513]
QFRONT = 3                                     # qoffsets[0]: unused columns in front of the first query
NOPS = [1, 63, 64, 65, 128, 129, 300]
OPS_CAP = 300
M, I, D = ord("M"), ord("I"), ord("D")


def letters_of(rng, n):
    """n distinct target bytes, the protein letters (what the databases are drawn from) first."""
    if n <= len(PROTEIN):
        return PROTEIN[:n].copy()
    rest = np.setdiff1d(np.arange(256, dtype=np.uint8), PROTEIN)
    return np.concatenate([PROTEIN, rng.permutation(rest)[:n - len(PROTEIN)]]).astype(np.uint8)


def reference(c, prior_weight, include_min, weights=None, code=None):
    """(new matrix int8 in the layout of c.prior, counts int32 rebased to the first query, used (nq, top) bool) by the rule of the header.
    code: 256 places to take in the place of the letters' own -- what a call would count had it read another call's code table (a
    place outside the letters counts nothing); the session tests ask that."""
    nl, nq, top = len(c.letters), len(c.qoffs) - 1, c.hits.shape[1]
    ntargets = len(c.offs) - 1
    if code is None:
        code = np.full(256, -1, np.int64)
        code[c.letters] = np.arange(nl)
    else:
        code = np.where((np.asarray(code, np.int64) >= 0) & (np.asarray(code, np.int64) < nl), np.asarray(code, np.int64), -1)
    S = c.sub[np.ix_(c.letters, c.letters)].astype(np.int64)             # S[b][k]: the observed residue plays the query letter
    P = np.minimum(c.prior.astype(np.int64), c.smax)
    out = c.prior.astype(np.int64).copy()
    counts = np.zeros((int(c.qoffs[-1] - c.qoffs[0]), nl), np.int64)
    used = np.zeros((nq, top), bool)
    for q in range(nq):
        g0, qlen = int(c.qoffs[q]), int(c.qoffs[q + 1] - c.qoffs[q])
        nh = top if c.nhits is None else int(np.clip(c.nhits[q], 0, top))
        C = np.zeros((qlen, nl), np.int64)
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
            w = 1 if weights is None else int(np.clip(weights[q, r], 0, 65535))
            o = c.ops[q * top + r, :nops]
            is_m = o == M
            cq, ct = is_m | (o == I), is_m | (o == D)
            j, i = qb + np.cumsum(cq) - cq, tb + np.cumsum(ct) - ct        # where every op stands before it consumes anything
            pair = is_m & (j < qlen) & (i < ln)
            k = code[c.packed[c.offs[t] + i[pair]]]
            np.add.at(C, (j[pair][k >= 0], k[k >= 0]), w)
        counts[g0 - int(c.qoffs[0]):g0 - int(c.qoffs[0]) + qlen] = C
        N = C.sum(axis=1)
        den = (prior_weight + N)[:, None]
        num = prior_weight * P[g0:g0 + qlen] + C @ S
        new = np.clip((2 * num + den) // np.maximum(2 * den, 1), -128, 127)    # numpy's // floors
        out[g0:g0 + qlen] = np.where(den == 0, P[g0:g0 + qlen], new)
    assert counts.max(initial=0) < 2**28
    return out.astype(np.int8), counts.astype(np.int32), used


def _case(rng, letters, smax, qlens, packed, offs, top, lo=-8, hi=12, sub=None):
    c = types.SimpleNamespace()
    c.letters, c.smax, c.other = np.asarray(letters, np.uint8), int(smax), -4
    c.qoffs = np.concatenate([[QFRONT], QFRONT + np.cumsum(qlens)]).astype(np.int64)
    c.prior = rng.integers(lo, hi + 1, (int(c.qoffs[-1]), len(c.letters))).astype(np.int8)   # the unused front columns too
    c.packed, c.offs = packed, offs
    c.sub = random_submat(rng) if sub is None else sub
    nq = len(qlens)
    c.hits = np.zeros((nq, top, 3), np.int64)
    c.nhits = None
    c.aln = np.zeros((nq, top, 7), np.int64)
    c.cap = OPS_CAP
    c.ops = np.full((nq * top, OPS_CAP), 0x5A, np.uint8)
    return c


def scoring(c):
    return (c.letters, c.other, c.smax, -10, -1)


def _pattern(rng, kind, nops):
    """nops op bytes of one of the shapes the chunked walk can get wrong."""
    if kind == 0:
        o = np.full(nops, M)
    elif kind == 1:                          # a run of I longer than a chunk: a whole chunk consumes the query only
        o = np.concatenate([np.full(3, M), np.full(70, I), np.full(max(0, nops - 73), M)])
    elif kind == 2:                          # ... and of D: the target only
        o = np.concatenate([np.full(3, M), np.full(70, D), np.full(max(0, nops - 73), M)])
    elif kind == 3:                          # an M directly on each side of every chunk edge, nothing else pairs
        o = np.where(np.arange(nops) % 2 == 0, I, D)
        edge = np.arange(64, nops, 64)
        o[edge] = M
        o[edge - 1] = M
    else:
        o = rng.choice([M, M, M, I, D], nops)
    return o[:nops].astype(np.uint8)


def synthetic(rng, nletters, top, qlens=QLENS, smax=11, dup_targets=None):
    """Tables written by hand over a small database: every nops of NOPS, every pattern, q_begin at 0 and at qlen - 1, alignments that end
    exactly at qlen and at len, in turn over the entries."""
    letters = letters_of(rng, nletters)
    tlens = [0, 1, 5, 64, 65, 130, 400, 700] if dup_targets is None else dup_targets
    offs = np.concatenate([[7], 7 + np.cumsum(tlens)]).astype(np.int64)
    packed = rng.choice(PROTEIN, int(offs[-1])).astype(np.uint8)
    c = _case(rng, letters, smax, qlens, packed, offs, top)
    nq, n = len(qlens), 0
    kinds = set()
    for q in range(nq):
        qlen = qlens[q]
        for r in range(top):
            nops, kind, place = NOPS[n % len(NOPS)], (n // len(NOPS)) % 5, (n // (5 * len(NOPS))) % 4
            n += 1
            t = int(rng.integers(0, len(tlens)))
            ln = tlens[t]
            o = _pattern(rng, kind, nops)
            nq_used, nt_used = int(((o == M) | (o == I)).sum()), int(((o == M) | (o == D)).sum())
            if place == 0:
                qb, tb = 0, 0
            elif place == 1:
                qb, tb = qlen - 1, int(rng.integers(0, ln + 1))
            elif place == 2:                 # ends exactly at qlen and at len where it fits (a walk past either end is defined too)
                qb, tb = max(0, qlen - nq_used), max(0, ln - nt_used)
            else:
                qb, tb = int(rng.integers(0, qlen + 1)), int(rng.integers(0, ln + 1))
            c.hits[q, r] = (t, 0, 0)
            c.aln[q, r] = (0, int(rng.integers(0, 100)), qb, tb, 0, 0, nops)
            c.ops[q * top + r, :nops] = o
            kinds.add((nops, kind, place))
    if nq * top >= 5 * len(NOPS):
        assert len({(a, b) for a, b, _ in kinds}) == 5 * len(NOPS)         # every nops with every pattern
    return c


def garbage(rng, c):
    """The same case with entries no alignment call would write: the call has to stay defined and inside its buffers."""
    nq, top, _ = c.hits.shape
    ntargets = len(c.offs) - 1
    flat = [(q, r) for q in range(nq) for r in range(top)]
    for n, (q, r) in enumerate(flat):
        what = n % 9
        if what == 0:
            c.hits[q, r, 0] = -1
        elif what == 1:
            c.hits[q, r, 0] = ntargets
        elif what == 2:
            c.aln[q, r, 6] = 0
        elif what == 3:
            c.aln[q, r, 6] = c.cap + 1
        elif what == 4:
            c.aln[q, r, 2] = int(c.qoffs[q + 1] - c.qoffs[q]) + 1
        elif what == 5:
            c.ops[q * top + r, ::3] = 0x00
            c.ops[q * top + r, 1::3] = 0xFF
        elif what == 6:                      # a walk that runs past qlen and len
            c.aln[q, r, 6] = c.cap
            c.ops[q * top + r] = M
        elif what == 7:
            c.aln[q, r, 3] = -1
        # 8: left as it is
    c.nhits = np.array([(-5, top + 7, top, max(0, top - 1))[q % 4] for q in range(nq)], np.int64)
    return c


def mutate(rng, seq, alpha):
    """A homologue: substitutions, insertions and deletions."""
    out = []
    for x in seq:
        u = rng.random()
        if u < 0.03:
            continue
        out.append(int(rng.choice(alpha)) if u < 0.15 else int(x))
        if rng.random() < 0.03:
            out.extend(int(y) for y in rng.choice(alpha, int(rng.integers(1, 4))))
    return np.array(out, np.uint8)


def homologue_database(rng, queries, nrandom, copies=3, alpha=PROTEIN[:20]):
    """Random protein targets of 0..600 letters with `copies` mutated copies of every query planted inside flanks."""
    targets = [rng.choice(alpha, int(n)).astype(np.uint8) for n in [0, 1, 63, 64, 65, 0] + list(rng.integers(2, 601, nrandom))]
    for qs in queries:
        for _ in range(copies):
            targets.append(np.concatenate([rng.choice(alpha, int(rng.integers(0, 40))).astype(np.uint8), mutate(rng, qs, alpha),
                                           rng.choice(alpha, int(rng.integers(0, 40))).astype(np.uint8)]))
    order = rng.permutation(len(targets))
    targets = [targets[k] for k in order]
    offs = np.concatenate([[7], 7 + np.cumsum([len(t) for t in targets])]).astype(np.int64)
    packed = np.concatenate([rng.integers(0, 256, 7).astype(np.uint8)] + targets)
    return packed, offs


def real(swamd, rng, top, qlens=QLENS, nrandom=40, nletters=24, alpha=PROTEIN[:20], sub=None):
    """Iteration 0 of a search on the host: sequence queries through sw_pssm_from_queries, the search, the rank order, the alignment.
    alpha: the letters the sequences are drawn from; sub: the table (default: a random symmetric one)."""
    from pssm_cases import rank_order
    letters = letters_of(rng, nletters)
    queries = [rng.choice(alpha, n).astype(np.uint8) for n in qlens]
    packed, offs = homologue_database(rng, queries, nrandom, alpha=alpha)
    if sub is None:
        sub = random_submat(rng, lo=-6, hi=8)
        sub = np.minimum(sub, sub.T)                                        # (symmetric, as real tables are; nothing depends on it)
    c = _case(rng, letters, 127, qlens, packed, offs, top, sub=sub)
    m, moffs = swamd.pssm_from_queries(queries, sub, letters)
    c.prior[QFRONT:] = m
    c.queries = queries
    sc = scoring(c)
    res = swamd.search_pssm_multi_host((c.prior, c.qoffs), (packed, offs), sc)
    c.hits, c.nhits = rank_order(res, top, 1)
    aln, ops = swamd.align_pssm_hits_host((c.prior, c.qoffs), (packed, offs), sc, c.hits, c.nhits)
    c.aln = aln
    c.cap = max(1, max(qlens) + int(np.diff(offs).max()))
    c.ops = np.full((len(qlens) * top, c.cap), 0x5A, np.uint8)
    for q, row in enumerate(ops):
        for r, b in enumerate(row):
            c.ops[q * top + r, :len(b)] = np.frombuffer(b, np.uint8)
    # not vacuous: conditions on the inputs
    _, counts, used = reference(c, 1, 1)
    live = c.ops[np.arange(c.cap)[None, :] < c.aln.reshape(-1, 7)[:, 6:7]]       # the op bytes inside every row's nops
    assert used.sum() * 2 >= used.size, "fewer than half of the entries are used"
    assert (live == I).any() and (live == D).any(), "the alignments hold no I or no D"
    assert c.aln[:, :, 6].max() > 64, "no alignment exceeds 64 ops"
    assert counts.sum(axis=1).max() >= 2, "no column was observed twice"
    return c


GUARD, POISON = 64, 0x55


def host_leg(swamd, c, prior_weight, include_min, weights=None, want_out=True, want_counts=True, in_place=False):
    """sw_pssm_from_hits_host through ctypes on buffers with guard bytes around them and poison in the unused front columns: asserts
    SW_OK and that nothing outside the queries' columns changed.  Returns (matrix of the queries' columns or None, counts or None)."""
    import ctypes
    L = swamd.lib()
    lt, sc = swamd._pssm_scoring(scoring(c))
    sub, up = swamd._pssm_update((c.sub, prior_weight, include_min))
    nl, nq, top = len(c.letters), len(c.qoffs) - 1, c.hits.shape[1]
    front, total = int(c.qoffs[0]) * nl, int(c.qoffs[-1]) * nl
    prior = np.full(GUARD + total + GUARD, POISON, np.int8)
    prior[GUARD + front:GUARD + total] = c.prior.reshape(-1)[front:]
    out = prior if in_place else np.full(GUARD + total + GUARD, POISON, np.int8)
    ncnt = total - front
    counts = np.full(GUARD + ncnt + GUARD, 0x55555555, np.int32)
    hits, aln, ops = np.ascontiguousarray(c.hits), np.ascontiguousarray(c.aln), np.ascontiguousarray(c.ops)
    w = None if weights is None else np.ascontiguousarray(weights, np.int32)
    rc = L.sw_pssm_from_hits_host(prior[GUARD:].ctypes.data, c.qoffs.ctypes.data, nq, c.packed.ctypes.data, c.offs.ctypes.data, len(c.offs) - 1,
                                  ctypes.byref(sc), ctypes.byref(up), hits.ctypes.data, c.nhits.ctypes.data if c.nhits is not None else None, top,
                                  aln.ctypes.data, ops.ctypes.data, c.cap, w.ctypes.data if w is not None else None,
                                  out[GUARD:].ctypes.data if want_out else None, counts[GUARD:].ctypes.data if want_counts else None)
    assert rc == 0, L.sw_last_error().decode()
    assert (out[:GUARD + front] == POISON).all() and (out[GUARD + total:] == POISON).all(), "the matrix was written outside the queries' columns"
    assert (counts[:GUARD] == 0x55555555).all() and (counts[GUARD + ncnt:] == 0x55555555).all(), "the counts were written outside their buffer"
    if not want_out and not in_place:
        assert (out == POISON).all()
    if not want_counts:
        assert (counts == 0x55555555).all()
    return (out[GUARD + front:GUARD + total].reshape(-1, nl).copy() if want_out else None,
            counts[GUARD:GUARD + ncnt].reshape(-1, nl).copy() if want_counts else None)


# ---- the update at its arithmetic edges ----

def all_m_case(svals, parts, prior, smax=127, ncols=65):
    """One query of ncols columns over len(svals) letters, top = sum(parts): `parts[b]` entries name target b, ncols x letter b, and pair
    every column with it from (0, 0) through ncols 'M'; row b of S is svals[b] at every k.  So every column has C[j][b] = parts[b] x w
    and the same new row, whose entries are all equal.  prior: one value for every entry."""
    rng = np.random.default_rng(len(svals) + sum(parts))
    nl, top = len(svals), int(sum(parts))
    letters = PROTEIN[:nl].copy()
    offs = np.concatenate([[7], 7 + ncols * np.arange(1, nl + 1)]).astype(np.int64)
    packed = np.concatenate([rng.choice(PROTEIN, 7).astype(np.uint8)] + [np.full(ncols, x, np.uint8) for x in letters])
    c = _case(rng, letters, smax, [ncols], packed, offs, top)
    c.prior[:] = prior
    c.sub = rng.integers(-128, 128, (256, 256)).astype(np.int8)
    for b, s in enumerate(svals):
        c.sub[letters[b], :] = s
    c.hits[0, :, 0] = np.repeat(np.arange(nl), parts)
    c.aln[0, :] = (0, 5, 0, 0, 0, 0, ncols)
    c.cap = ncols
    c.ops = np.full((top, ncols), M, np.uint8)
    return c


def overflow_case(first=2048):
    """65 columns, 3 letters, top = 4096 at weight 65535: `first` entries pair every column with the letter whose row of S is 127, the
    others with the one whose row is -128.  (case, weights).  C x S passes 2^31 and N[j] is the largest the header allows; with equal
    halves num is an exact -1/2 of den, with unequal ones num itself passes 2^32 and a sum kept in 32 bits has another sign."""
    c = all_m_case([127, -128, 5], [first, 4096 - first, 0], prior=3)
    c.prior[:, 0], c.prior[:, 2] = -3, -77                # rows [-3, 3, -77]: both signs beside the half
    w = np.full((1, 4096), 65535, np.int32)
    front = int(c.qoffs[0])
    S = c.sub[np.ix_(c.letters, c.letters)].astype(np.int64)
    for pw in (0, 1, 65535):
        out, counts, used = reference(c, pw, 0, w)
        C = counts.astype(np.int64)
        assert used.all() and (C.sum(axis=1) == 4096 * 65535).all() and 4096 * 65535 < 2**28
        assert (np.abs(C[:, :, None] * S[None, :, :]) > 2**31).any()
        assert out[front:].min() > -128 and out[front:].max() < 127                     # at no clamp
        total = (C @ S)[0, 0]
        if first == 2048:
            assert 2 * total == -4096 * 65535 and (pw > 0 or not out[front:].any())     # the exact half -1/2 rounds up to 0
        else:
            wrapped = (int(total) + 2**31) % 2**32 - 2**31
            assert abs(total) > 2**32 and (wrapped < 0) != (total < 0) and abs(int(out[front, 0])) > 30
    return c, w


def clamp_case(s, smax):
    """Five letters, S == s everywhere and a prior of -128 everywhere: an observed column gives s under prior_weight 0 (127 and -128 are
    the two clamps), an unobserved one min(-128, smax) = -128."""
    rng = np.random.default_rng(1000 + s + smax)
    c = synthetic(rng, 5, 3, smax=smax)
    c.prior[:] = -128
    c.sub = np.full((256, 256), s, np.int8)
    front = int(c.qoffs[0])
    out, counts, _ = reference(c, 0, 0)
    seen = counts.sum(axis=1) > 0
    assert seen.any() and not seen.all() and (out[front:][seen] == s).all() and (out[front:][~seen] == -128).all()
    return c


ROUNDING = [                 # (prior_weight, prior, S per letter, entries per letter, weight, expected entry)
    (0, 0, (127, 126), (2048, 2048), 65535, 127),          # 126.5: an exact half, num = 3.4e10
    (0, 0, (-127, -128), (2048, 2048), 65535, -127),       # -127.5 -> -127, num = -3.4e10
    (0, 0, (-127, -128), (1024, 3072), 65535, -128),       # -127.75 -> -128; truncating (2 num + den) / (2 den) = -127.25 would give -127
    (0, 0, (127, 126), (1024, 3072), 65535, 126),          # 126.25
    (65535, -128, (-127, -128), (2048, 2047), 65535, -127),   # -127.5 exactly, the prior's share (65535 x -128) included
    (1, 127, (100, -100), (2048, 2048), 65535, 0),         # 127 / den: just above 0
    (1, -127, (100, -100), (2048, 2048), 65535, 0),        # -127 / den: just below 0 and far above -1/2
    (1, -128, (1, -2), (2048, 2048), 65535, -1),           # (-128 - 2048 x 65535) / (1 + 4096 x 65535): a hair BELOW -1/2 -> -1
    (1, 127, (1, -2), (2048, 2048), 65535, 0),             # ... and a hair above it -> 0
    (0, 0, (1, -2), (2048, 2048), 65535, 0),               # -1/2 exactly -> 0
    (0, 0, (-1, -2), (2048, 2048), 65535, -1),             # -3/2 exactly -> -1
]


def rounding_case(pw, prior, svals, parts, weight, exp):
    """One column; (case, weights).  The expected entry is checked here against the header's formula in Python integers."""
    c = all_m_case(list(svals), list(parts), prior=prior, ncols=1)
    num = pw * prior + sum(n * weight * s for n, s in zip(parts, svals))
    den = pw + sum(parts) * weight
    assert exp == max(-128, min(127, (2 * num + den) // (2 * den))), (num, den)
    return c, np.full((1, sum(parts)), weight, np.int32)


def alphabet_case(rng, nletters, top):
    """synthetic() at another alphabet.  At 255 letters the one byte that is no letter stands at every third place of the targets (code
    255: "none"), at 256 letters the letter at place 255 does (code 255: a letter): (case, the counts of that byte's pairs)."""
    c = synthetic(rng, nletters, top)
    if nletters < 255:
        return c, None
    byte = np.setdiff1d(np.arange(256, dtype=np.uint8), c.letters)[0] if nletters == 255 else c.letters[255]
    c.packed[::3] = byte
    if nletters == 256:
        at = reference(c, 1, 0)[1][:, 255]
        assert at.sum() > 0                                    # the letter at place 255 is paired and counted
        return c, at
    wide = types.SimpleNamespace(**vars(c))
    wide.letters = np.concatenate([c.letters, [byte]]).astype(np.uint8)
    wide.prior = np.concatenate([c.prior, c.prior[:, :1]], axis=1)
    counts, wcounts = reference(c, 1, 0)[1], reference(wide, 1, 0)[1]
    assert wcounts[:, 255].sum() > 0                           # some 'M' pairs the missing byte ...
    assert (counts == wcounts[:, :255]).all()                  # ... and nothing is counted for it
    return c, wcounts[:, 255]


def full_range_case(rng, nletters, top, smax):
    """synthetic() with S from the full-range table of tests/affine_range_cases.py and a prior uniform over -128 .. 127."""
    import affine_range_cases as arc
    c = synthetic(rng, nletters, top, smax=smax)
    c.sub = arc.table("full8").copy()
    c.prior = rng.integers(-128, 128, c.prior.shape).astype(np.int8)
    assert c.prior.min() == -128 and c.prior.max() == 127
    return c


# ---- the second turn of the grid-stride loops (test_pssm_full_size_host.py, test_pssm_full_size_gpu.py) ----

GRID_MAX = 1 << 20                         # swp::kPssmHitsGridMax
TURN_INCLUDE_MIN = 20                      # include_min_score of the calls on second_turn_case()
TURN_LONG, TURN_TILE = 567, 63             # three queries of 9 tiles of 63 columns (256 letters) among one-column queries


def subcase(c, qs):
    """The queries qs of a case as a case of their own (a query depends on no other query): what the numpy rule can walk when the whole
    case has a million queries."""
    top = c.hits.shape[1]
    s = types.SimpleNamespace(**vars(c))
    qlens = [int(c.qoffs[q + 1] - c.qoffs[q]) for q in qs]
    s.qoffs = np.concatenate([[QFRONT], QFRONT + np.cumsum(qlens)]).astype(np.int64)
    rows = np.concatenate([np.arange(c.qoffs[q], c.qoffs[q + 1]) for q in qs])
    s.prior = np.concatenate([c.prior[:QFRONT], c.prior[rows]])
    s.hits, s.aln = c.hits[qs], c.aln[qs]
    s.nhits = None if c.nhits is None else c.nhits[qs]
    s.ops = c.ops.reshape(len(c.qoffs) - 1, top, -1)[qs].reshape(len(qs) * top, -1)
    return s


def live_jobs(c, tiles_per_query, tile_cols, group):
    """The jobs workgroup `group` of a grid of GRID_MAX takes in its grid-stride loop and does not skip, in order: (query, tile)."""
    nq = len(c.qoffs) - 1
    out = []
    for job in range(group, nq * tiles_per_query, GRID_MAX):
        q, tile = divmod(job, tiles_per_query)
        if tile * tile_cols < int(c.qoffs[q + 1] - c.qoffs[q]):
            out.append((q, tile))
    return out


@functools.lru_cache(maxsize=None)
def second_turn_case():
    """GRID_MAX + 3 queries over 256 letters, top = 1: one column each, except TURN_LONG columns (9 tiles) at the indices 0, 2^19 and
    last.  9 x (GRID_MAX + 3) jobs over GRID_MAX workgroups: workgroup g takes the jobs g, g + GRID_MAX, ...; those it does not skip are the
    tiles of the long queries and tile 0 of the others.  Used entries: the three long queries (each across a tile edge), some 2000 one-
    column queries drawn at random, and the one-column queries that follow or precede a long query's tile in the same workgroup, set
    so that a tile WITH counts is followed by another query's tile WITHOUT and the reverse (asserted below from job % GRID_MAX).  Entries
    that are not used are so in turn for each reason the rule names.  (case, the queries with a used entry, sorted, subcase(case,
    those queries)): built once and shared -- the tests leave it unchanged."""
    rng = np.random.default_rng(20)
    nq, nl, cap, tpq = GRID_MAX + 3, 256, 16, TURN_LONG // TURN_TILE
    assert tpq * TURN_TILE == TURN_LONG and tpq == 9
    longq = [0, GRID_MAX // 2, nq - 1]
    qlens = np.ones(nq, np.int64)
    qlens[longq] = TURN_LONG
    c = types.SimpleNamespace()
    c.letters, c.smax, c.other = letters_of(rng, nl), 11, -4
    c.qoffs = np.concatenate([[QFRONT], QFRONT + np.cumsum(qlens)]).astype(np.int64)
    c.prior = rng.integers(-128, 128, (int(c.qoffs[-1]), nl), dtype=np.int8)
    tlens = [0, 1, 5, 64, 65, 130, 400, 700]
    c.offs = np.concatenate([[7], 7 + np.cumsum(tlens)]).astype(np.int64)
    c.packed = rng.integers(0, 256, int(c.offs[-1]), dtype=np.uint8)
    c.sub = random_submat(rng)
    c.cap, c.nhits = cap, None
    c.ops = np.full((nq, cap), 0x5A, np.uint8)
    # nothing is used until it is made so below: a target out of range, a score below include_min = 20, nops 0 or beyond ops_cap, in turn
    c.hits = np.zeros((nq, 1, 3), np.int64)
    c.hits[:, 0, 0] = np.where(np.arange(nq) % 4 == 0, len(tlens), rng.integers(3, len(tlens), nq))
    c.aln = np.zeros((nq, 1, 7), np.int64)
    c.aln[:, 0, 1] = np.where(np.arange(nq) % 4 == 1, 19, 50)
    c.aln[:, 0, 6] = np.select([np.arange(nq) % 4 == 2, np.arange(nq) % 4 == 3], [0, cap + 1], 7)
    c.ops[:, :7] = M                                              # (ops that WOULD count, were the entry used)

    def use(q, qb, nops, lead_d=0):
        t = int(rng.integers(5, len(tlens)))                      # a target of 130 letters or more
        c.hits[q, 0] = (t, 0, 0)
        c.aln[q, 0] = (0, 20 + int(rng.integers(0, 50)), qb, int(rng.integers(0, 100)), 0, 0, nops)
        c.ops[q] = 0x5A
        c.ops[q, :lead_d] = D
        c.ops[q, lead_d:nops] = M

    # the long queries: 16 'M' across the edges of the tiles 0|1, 3|4 and 7|8
    for q, qb in zip(longq, (55, 4 * TURN_TILE - 8, 8 * TURN_TILE - 8)):
        use(q, qb, cap)
    counted = {(longq[0], 0), (longq[0], 1), (longq[1], 3), (longq[1], 4), (longq[2], 7), (longq[2], 8)}
    ones = np.setdiff1d(rng.choice(nq, 2000, replace=False), longq)
    # the workgroups of the long queries' tiles: which one-column query each takes, and whether it gets a used entry
    groups = sorted({(q * tpq + tile) % GRID_MAX for q in longq for tile in range(tpq)})
    forced = {}
    for g in groups:
        for q, tile in live_jobs(types.SimpleNamespace(qoffs=c.qoffs), tpq, TURN_TILE, g):
            if q not in longq:
                forced[q] = g % 2 == 1                           # with a used entry in the odd workgroups, without in the even ones
    forced[1], forced[GRID_MAX + 1] = True, False                # (the finish kernel's workgroup 1, below)
    ones = np.setdiff1d(ones, [q for q, u in forced.items() if not u])
    ones = np.union1d(ones, [q for q, u in forced.items() if u]).astype(np.int64)
    for n, q in enumerate(ones):
        use(int(q), 0, 1 + n % cap, lead_d=n % 3 if n % cap >= 3 else 0)
    used_q = np.union1d(ones, longq).astype(np.int64)
    counted |= {(int(q), 0) for q in ones}
    # the pairing, from job % GRID_MAX: in some workgroup counts -> none and in some none -> counts, between different queries
    seen = set()
    for g in groups:
        jobs = live_jobs(c, tpq, TURN_TILE, g)
        for (q0, t0), (q1, t1) in zip(jobs, jobs[1:]):
            if q0 != q1:
                seen.add(((q0, t0) in counted, (q1, t1) in counted))
    assert {(True, False), (False, True), (True, True)} <= seen, seen
    # the finish kernel's second turn: the workgroups 0, 1, 2 take the queries GRID_MAX, GRID_MAX + 1, GRID_MAX + 2 after 0, 1, 2
    first, second = np.isin([0, 1, 2], used_q), np.isin([GRID_MAX, GRID_MAX + 1, GRID_MAX + 2], used_q)
    assert first.tolist() == [True, True, False] and second.tolist() == [False, False, True]      # used -> not used twice, and the reverse
    return c, used_q, subcase(c, used_q)


def second_turn_expected(c, used_q, sub_out, sub_counts):
    """The whole call's matrix (the queries' columns) and the nonzero counts as (rows, counts of those rows), from the results of
    subcase(c, used_q): min(prior, smax) and zero counts in every query without a used entry."""
    front = int(c.qoffs[0])
    out = np.minimum(c.prior[front:], c.smax).astype(np.int8)
    rows = np.concatenate([np.arange(c.qoffs[q], c.qoffs[q + 1]) for q in used_q]) - front
    out[rows] = sub_out
    return out, rows, sub_counts
