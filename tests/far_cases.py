"""Shared by test_far_host.py and test_far_gpu.py: the database-search family with its buffers and offsets beyond 4 GiB.  Plain data and
helpers, no GPU.

Only PLACEMENT changes between the cases: the sequences are tiny and the same everywhere, so every expected value comes from the
independent checker (tests/affine_oracle.cpp) or the numpy reference of the ungapped score (tests/ungapped_cases.py) on the small
arrays, once per process, read-only.  No result depends on placement: max_pos is row * (qlen + 1) + col of the pair's own matrix.

THE FAR RANGE.  Every far offset lies in [2^32, 2^32 + 2^31).  Its low 32 bits are then a small positive number whether a wrong kernel
takes them as u32 or as int32, so a truncated address lands inside the same allocation at offset - 2^32.  There lies a DECOY: a second
world of the same lengths from another seed whose result differs from the true one for every (query, non-empty target) pair -- a
kernel (or a ctypes argtypes entry) that drops the high half shows as wrong values and never as a fault.

The PSSM update and the hit weights read the same world through the reference's hit table and the rule's alignments (hits_case); their
decoy condition (hits_decoy_failures) is part of decoy_failures(), and count_case() is the one case whose OUTPUT passes 4 GiB."""
import functools

import numpy as np

import lanes_cases as lc
from affine_cases import PROTEIN
from align_cases import expected as rule_alignment
from pssm_cases import letters_of, rank_order
from ungapped_cases import ungapped_score

WRAP = 2**32
FAR = 2**32 + 2**20                                # offsets[0], qoffsets[0] and the byte where a far PSSM of 256 letters begins
STRADDLE = 2**32 - 150                             # offsets[0] with the 300-letter target first: it spans the 2^32 byte line
PSSM_FAR = {256: 2**24 + 4096, 24: 2**32 // 24 + 4096}   # qoffsets[0] in COLUMNS: below 2^32, times nletters beyond it
BATCH_STRIDE = 2**30 + 64                          # a_stride = b_stride of the batch case: pair 4 starts at 4 x that
FAR_CONSTANTS = {"FAR": FAR, "pssm 256": PSSM_FAR[256] * 256, "pssm 24": PSSM_FAR[24] * 24, "batch pair 4": 4 * BATCH_STRIDE,
                 "straddle, second target": STRADDLE + 300}
for _name, _v in FAR_CONSTANTS.items():
    assert 2**32 <= _v < 2**32 + 2**31, _name
    assert 0 < (_v & 0xFFFFFFFF) < 2**31 and _v - WRAP == (_v & 0xFFFFFFFF), _name   # the same small number as u32 and as int32
assert PSSM_FAR[256] < 2**32 and PSSM_FAR[24] < 2**32 and STRADDLE < 2**32 < STRADDLE + 300

QLENS = [1, 63, 257, 513, 1025]                    # 4, 8 and 16 columns per lane, and two strips
TLENS = [0, 1, 5, 64, 65, 0, 127, 300, 301]        # empties in between; seven non-empty targets, so the packed schedule ends on a lone one
NQ, NT = len(QLENS), len(TLENS)
GAPS = [(-11, -1), (0, 0)]
LINEAR = (3, -3, -2)                               # sw_search_device: match, mismatch, gap
OTHER, SMAX = lc.OTHER, 11
STRADDLE_ORDER = [7, 0, 1, 2, 3, 4, 5, 6, 8]       # the 300-letter target first
NATURAL_ORDER = list(range(NT))
TAIL = 16                                          # spare bytes behind a payload
WORLD_SEED, DECOY_SEED = 3315, 4635      # searched: the decoy condition of decoy_failures() holds for this pair
TOP, MIN_SCORE, PREFILTER_MIN = 4, 1, 12           # the selecting calls of the small world
NHITS_CUT = [4, 0, 3, 4, 2]                        # the counts of the alignment calls: unused entries in the table, one empty row
# the update and the hit weights over the small world: hits_decoy_failures() is empty for these.  per_hit 16 rounds the shares of the
# three-hit query to the same weights in the world and in the decoy; a prior weight of 2 beside weights of some 256 leaves the prior no
# say (a decoy PRIOR would not show), so the weighted update takes 2 x per_hit; and two hits alone weigh the same whatever their
# residues (every term is 1/2 or 1 by the columns they share, not by the letters), so the last query gets three.
PRIOR_WEIGHT, PER_HIT, INCLUDE_MIN = 2, 256, 1
PRIOR_WEIGHT_WEIGHTED = 2 * PER_HIT
HITS_NHITS_CUT = [4, 0, 3, 4, 4]
OPS_CAP = max(QLENS) + max(TLENS)
OPS_POISON = 0xA5


def table24():
    return lc.table24()


def linear_table():
    """sw_submat_match(3, -3) in numpy."""
    s = np.full((256, 256), LINEAR[1], np.int8)
    s[np.arange(256), np.arange(256)] = LINEAR[0]
    return s


def _draw(seed, letters=PROTEIN):
    rng = np.random.default_rng(seed)
    queries = [rng.choice(letters, n).astype(np.uint8) for n in QLENS]
    targets = [rng.choice(letters, n).astype(np.uint8) for n in TLENS]
    for a in queries + targets:
        a.setflags(write=False)
    return {"queries": queries, "targets": targets}


@functools.lru_cache(maxsize=None)
def world():
    """{"queries", "targets"}: the true sequences."""
    return _draw(WORLD_SEED)


@functools.lru_cache(maxsize=None)
def decoy():
    """The same lengths from another seed: what lies 2^32 bytes below every far payload.  It holds only the second half of the
    letters: the ungapped score of a one-letter sequence is the maximum of its table row (or column) over the letters the other
    sequence holds, and against 64 random letters of the whole alphabet no seed alone would change that."""
    return _draw(DECOY_SEED, PROTEIN[12:])


def packed(seqs, at, order=None):
    """(payload bytes, int64 offsets with offsets[0] = at) of the sequences back to back, in `order`."""
    seqs = [seqs[k] for k in (order if order is not None else range(len(seqs)))]
    offs = np.zeros(len(seqs) + 1, np.int64)
    offs[0] = at
    offs[1:] = at + np.cumsum([len(s) for s in seqs])
    return (np.concatenate(seqs) if offs[-1] > at else np.zeros(0, np.uint8)).astype(np.uint8), offs


def far_buffer(payload, at, decoy_bytes=None):
    """A byte array description {"size", "pieces": [(byte, bytes)]}: `payload` at byte `at` and, where `at` is far, the decoy at
    at - 2^32 (cut at the front where that is negative: the straddle case).  Nothing else of the array is ever written; a test
    realises it on numpy.empty or torch.empty."""
    payload = np.ascontiguousarray(payload).view(np.uint8).reshape(-1)
    pieces = []
    if decoy_bytes is not None and at + len(payload) > WRAP:
        d = np.ascontiguousarray(decoy_bytes).view(np.uint8).reshape(-1)
        assert len(d) == len(payload)
        lo = at - WRAP
        cut = max(0, -lo)
        assert lo + len(d) <= at, "decoy and payload overlap"
        pieces.append((lo + cut, d[cut:]))
    pieces.append((at, payload))
    return {"size": at + len(payload) + TAIL, "pieces": pieces}


def realise_numpy(desc, dtype=np.uint8):
    """The description on numpy.empty: only the pieces' pages become resident."""
    buf = np.empty(desc["size"], np.uint8)
    for at, b in desc["pieces"]:
        buf[at:at + len(b)] = b
    return buf.view(dtype)


def layouts(seqs_true, seqs_decoy, at, order=None):
    """(description, offsets) of a packed sequence set at byte `at` with its decoy."""
    p, offs = packed(seqs_true, at, order)
    d, _ = packed(seqs_decoy, at, order)
    offs.setflags(write=False)
    return far_buffer(p, at, d), offs


# ---- PSSMs that reproduce the queries under table24 (the rule of include/swhip.h, in numpy) ----

@functools.lru_cache(maxsize=None)
def pssm_letters(nletters):
    lt = PROTEIN.copy() if nletters == 24 else letters_of(np.random.default_rng(3203), nletters)
    assert len(lt) == nletters and len(set(lt.tolist())) == nletters
    lt.setflags(write=False)
    return lt


def pssm_of(queries, nletters):
    """(total columns, nletters) int8: column j of query q is table24's row of letter q[j] over the letters."""
    m = np.concatenate([table24()[q][:, pssm_letters(nletters)] for q in queries]).astype(np.int8)
    return np.ascontiguousarray(m)


def pssm_scoring(nletters, gaps):
    return (pssm_letters(nletters), OTHER, SMAX, *gaps)


def pssm_layout(nletters, first_column):
    """(description in bytes, column offsets) of the true PSSMs at column `first_column`, the decoy's 2^32 bytes below."""
    desc = far_buffer(pssm_of(world()["queries"], nletters), first_column * nletters, pssm_of(decoy()["queries"], nletters))
    desc["size"] = -(-desc["size"] // nletters) * nletters       # whole columns: the Python layer reshapes to (-1, nletters)
    offs = np.zeros(NQ + 1, np.int64)
    offs[0] = first_column
    offs[1:] = first_column + np.cumsum(QLENS)
    offs.setflags(write=False)
    return desc, offs


# ---- expected values ----

_EXPECTED = {}


def _table(checker, queries, targets, sub, gaps):
    p, offs = packed(targets, 0)
    return np.stack([checker.search(q, p, offs, sub, *gaps) for q in queries])


def _ungapped(queries, targets, sub):
    return np.array([[ungapped_score(q, t, sub) for t in targets] for q in queries], np.int64)


def expected(checker):
    """Everything the small world gives, in the natural target order: "R" {gaps: (5, 9, 3)} from the checker, "LIN" (5, 9, 3) under
    LINEAR, "U" (5, 9) from the numpy reference, "ALN" {gaps: {(q, t): (sw_alignment row, ops)}} from the rule's walk over the
    checker's matrices.  Computed once per process, read-only."""
    if not _EXPECTED:
        w = world()
        out = {"R": {g: _table(checker, w["queries"], w["targets"], table24(), g) for g in GAPS},
               "LIN": _table(checker, w["queries"], w["targets"], linear_table(), (0, LINEAR[2])),
               "U": _ungapped(w["queries"], w["targets"], table24()),
               "ALN": {g: {(q, t): rule_alignment(checker, w["queries"][q], w["targets"][t], table24(), *g)[:2]
                           for q in range(NQ) for t in range(NT) if TLENS[t]} for g in GAPS}}
        for a in list(out["R"].values()) + [out["LIN"], out["U"]]:
            a.setflags(write=False)
        for g in GAPS:
            for (q, t), (row, _) in out["ALN"][g].items():
                assert tuple(row[:2]) == tuple(out["R"][g][q, t, :2])
        _EXPECTED.update(out)
    return _EXPECTED


def hit_table(exp, gaps, order=NATURAL_ORDER):
    """(hits (5, TOP, 3), nhits (5,)): the reference's rank order of the table in target order `order`."""
    return rank_order(exp["R"][gaps][:, order], TOP, MIN_SCORE)


def prefiltered_table(exp, gaps, order=NATURAL_ORDER):
    """The hit table restricted to the pairs whose ungapped score reaches PREFILTER_MIN."""
    r = exp["R"][gaps][:, order].copy()
    r[exp["U"][:, order] < PREFILTER_MIN, 1] = -1
    return rank_order(r, TOP, MIN_SCORE)


def alignments(exp, gaps, hits, nhits, order=NATURAL_ORDER):
    """(aln (nq, top, 7) int64, ops rows as a list per query of bytes) the rule gives for a hit table in target order `order`."""
    nq, top, _ = hits.shape
    aln, ops = np.zeros((nq, top, 7), np.int64), [[b""] * top for _ in range(nq)]
    for q in range(nq):
        for r in range(int(nhits[q])):
            k = int(hits[q, r, 0])
            if 0 <= k < len(order) and TLENS[order[k]]:
                row, o = exp["ALN"][gaps][(q, order[k])]
                aln[q, r], ops[q][r] = row, o
    return aln, ops


def pair_list():
    """Every (query, target) pair shuffled, eight of them twice, and the three invalid kinds: query -1, target = ntargets, and the
    empty targets of whatever order the database has (every target index occurs): (npairs, 2) int64."""
    rng = np.random.default_rng(3204)
    cross = np.array([(q, t) for q in range(NQ) for t in range(NT)], np.int64)
    cross = cross[rng.permutation(len(cross))]
    pr = np.concatenate([cross, cross[rng.choice(len(cross), 8, replace=False)], np.array([(-1, 3), (2, NT), (-1, -1)], np.int64)])
    assert len(pr) % 2 == 0
    return pr


def pair_results(exp, gaps, pairs, order=NATURAL_ORDER):
    r = exp["R"][gaps][:, order]
    out = np.zeros((len(pairs), 3), np.int64)
    for p, (q, t) in enumerate(pairs):
        if 0 <= q < NQ and 0 <= t < NT:
            out[p] = r[q, t]
    return out


# ---- the PSSM update and the hit weights over the small world ----

def hits_case(exp, gaps, order=NATURAL_ORDER, nletters=24, targets=None, queries=None, nhits_cut=HITS_NHITS_CUT, hits=None):
    """The small world as a case of tests/pssm_hits_cases.py, compact: the prior is the PSSM of the queries (pssm_of), the tables are
    the reference's hit table in target order `order` (or `hits` = (hits, nhits)), cut to nhits_cut, with the rule's alignments and ops
    (poison behind every row's ops), S is table24.  targets / queries: other sequences of the same lengths in the place of the world's
    -- what a call would read had it dropped the high half of an address: the tables stay those of the true world."""
    import types
    w = world()
    c = types.SimpleNamespace()
    c.letters, c.smax, c.other = pssm_letters(nletters), SMAX, OTHER
    c.qoffs = np.concatenate([[0], np.cumsum(QLENS)]).astype(np.int64)
    c.prior = pssm_of(queries if queries is not None else w["queries"], nletters)
    c.packed, c.offs = packed(targets if targets is not None else w["targets"], 0, order)
    c.sub = table24()
    h, n = hits if hits is not None else hit_table(exp, gaps, order)
    c.hits, c.nhits = np.ascontiguousarray(h), np.minimum(n, nhits_cut).astype(np.int64)
    c.aln, ops = alignments(exp, gaps, c.hits, c.nhits, order)
    c.cap = OPS_CAP
    c.ops = np.full((c.hits.shape[0] * c.hits.shape[1], OPS_CAP), OPS_POISON, np.uint8)
    for q, row in enumerate(ops):
        for r, o in enumerate(row):
            c.ops[q * c.hits.shape[1] + r, :len(o)] = np.frombuffer(o, np.uint8)
    return c


def hits_want(c, weighted):
    """(weights, new matrix, counts) of a case by the numpy rules (tests/pssm_weights_cases.py, tests/pssm_hits_cases.py): the weights
    under PER_HIT, the update under PRIOR_WEIGHT_WEIGHTED with those weights or under PRIOR_WEIGHT with none."""
    import pssm_hits_cases as hc
    import pssm_weights_cases as wc
    w = wc.reference(c, PER_HIT, INCLUDE_MIN)[0]
    out, counts, _ = hc.reference(c, PRIOR_WEIGHT_WEIGHTED if weighted else PRIOR_WEIGHT, INCLUDE_MIN, w if weighted else None)
    return w, out, counts


# ---- the decoy condition ----

def decoy_failures(checker):
    """The (kind, mixture, query, target) for which a decoy does NOT change the result: must be empty.  A far database with near queries
    gives true queries x decoy targets under truncation, far queries the other mixture, both far the third.  The linear kind
    (sw_search_device) takes one query at an address of its own: only its database can be far."""
    w, d, exp = world(), decoy(), expected(checker)
    mixes = {"decoy targets": (w["queries"], d["targets"]), "decoy queries": (d["queries"], w["targets"]),
             "both decoys": (d["queries"], d["targets"])}
    live = [t for t in range(NT) if TLENS[t]]
    bad = []
    for name, (qs, ts) in mixes.items():
        for g in GAPS:
            got = _table(checker, qs, ts, table24(), g)
            bad += [(f"affine {g}", name, q, t) for q in range(NQ) for t in live if tuple(got[q, t]) == tuple(exp["R"][g][q, t])]
        got = _ungapped(qs, ts, table24())
        bad += [("ungapped", name, q, t) for q in range(NQ) for t in live if got[q, t] == exp["U"][q, t]]
    got = _table(checker, w["queries"], d["targets"], linear_table(), (0, LINEAR[2]))
    bad += [("linear", "decoy targets", q, t) for q in range(NQ) for t in live if tuple(got[q, t]) == tuple(exp["LIN"][q, t])]
    # the straddling target: a kernel that wraps in the middle of it reads the true first 150 letters and the decoy's rest
    hybrid = np.concatenate([w["targets"][7][:WRAP - STRADDLE], d["targets"][7][WRAP - STRADDLE:]])
    for g in GAPS:                                 # (a short query's best cell can lie in the true part: one query that differs shows the wrap)
        got = _table(checker, w["queries"], [hybrid], table24(), g)
        if all(tuple(got[q, 0]) == tuple(exp["R"][g][q, 7]) for q in range(NQ)):
            bad.append((f"affine {g}", "straddle hybrid", -1, 7))
    return bad + hits_decoy_failures(checker)


HITS_EXCUSED = [("pssm_hit_weights", 0)]
# query 0 has ONE column: its four hits pair that column with one residue each, and the weights only tell which of those residues
# coincide -- four different letters in the world and in the decoy alike give four equal weights.  The update of the same query does
# change (its counts name the letters), and so does every other query of both calls.


def hits_decoy_failures(checker):
    """The (family, mixture, nletters, target order, query) for which a decoy does NOT change a byte of the result of
    sw_db_pssm_hit_weights or sw_db_pssm_from_hits (with and without weights) under either of GAPS, over the queries with a used entry
    and but for HITS_EXCUSED: must be empty.  A far database gives decoy targets under truncation (both calls, the natural and the
    straddle order), far PSSM columns a decoy prior (the update only); the tables are the true world's.  The tests run every family
    under both GAPS, so a query shows a truncation when it differs under one of them: under GAPS[0] no column of the longest query is
    paired by more than two of its hits, and then no term of the weights depends on a residue (1/2 where two hits share the column,
    whatever their letters, 1 where one stands alone); under GAPS[1] its four hits run over the whole query."""
    w, d, exp = world(), decoy(), expected(checker)
    same = {}
    for g in GAPS:
        for nl in (24, 256):
            for order in (NATURAL_ORDER, STRADDLE_ORDER):
                true = hits_case(exp, g, order, nl)
                has = [q for q in range(NQ) if true.nhits[q] > 0 and (true.aln[q, :true.nhits[q], 6] > 0).any()]
                assert len(has) == 4
                mixes = {"decoy targets": hits_case(exp, g, order, nl, targets=d["targets"])}
                if order is NATURAL_ORDER:
                    mixes["decoy prior"] = hits_case(exp, g, order, nl, queries=d["queries"])
                    mixes["both decoys"] = hits_case(exp, g, order, nl, targets=d["targets"], queries=d["queries"])
                for weighted in (True, False):
                    tw, tout, _ = hits_want(true, weighted)
                    for name, c in mixes.items():
                        gw, gout, _ = hits_want(c, weighted)
                        for q in has:
                            rows = slice(int(true.qoffs[q]), int(true.qoffs[q + 1]))
                            key = ("pssm_from_hits" + (" weighted" if weighted else ""), name, nl, tuple(order), q)
                            same[key] = same.get(key, True) and np.array_equal(gout[rows], tout[rows])
                            if weighted and name != "decoy prior" and ("pssm_hit_weights", q) not in HITS_EXCUSED:
                                key = ("pssm_hit_weights", name, nl, tuple(order), q)
                                same[key] = same.get(key, True) and np.array_equal(gw[q], tw[q])
    assert len(same) == 2 * 4 * 2 * 4 + 3 * 2 * 3          # the update: 4 mixtures x 2 alphabets x 4 queries, twice; the weights: 3 x 2 x 3
    return [k for k, v in same.items() if v]


# ---- placements ----

PLACEMENTS = {"near": (3, 4), "db_far": (FAR, 4), "db_straddle": (STRADDLE, 4), "q_far": (3, FAR), "both_far": (FAR, FAR)}   # offsets[0], qoffsets[0]


def placement(kind):
    """{"db", "q": byte array descriptions, "offs", "qoffs", "order": the target order}: the small world at one of PLACEMENTS, with
    the decoy world 2^32 bytes below whatever is far."""
    at, qat = PLACEMENTS[kind]
    order = STRADDLE_ORDER if kind == "db_straddle" else NATURAL_ORDER
    db, offs = layouts(world()["targets"], decoy()["targets"], at, order)
    q, qoffs = layouts(world()["queries"], decoy()["queries"], qat)
    assert (len(db["pieces"]) == 2) == (kind in ("db_far", "db_straddle", "both_far")) and (len(q["pieces"]) == 2) == (kind in ("q_far", "both_far"))
    return {"db": db, "offs": offs, "q": q, "qoffs": qoffs, "order": order}


# ---- far outputs: the same nine targets among 2^24 - 9 empty ones ----

BIG_NT = 2**24
BIG_LIVE = [0, 1, 2**23] + list(range(BIG_NT - 6, BIG_NT))       # where the nine targets of the world sit, in their order
BIG_NQ = 12                                                      # the five queries, repeated: 12 x 2^24 x 24 bytes = 4.5 GiB
FILTER_NQ = 72                                                   # the queries of 1 and 63 letters in turn: 72 x 2^24 x 4 bytes = 4.5 GiB
assert (BIG_NQ - 1) * BIG_NT * 24 > WRAP > (BIG_NQ - 2) * BIG_NT * 24 and (FILTER_NQ - 7) * BIG_NT * 4 > WRAP
assert len(BIG_LIVE) == NT


def big_offsets(front=3):
    """The 2^24 + 1 offsets of the big database: its bytes are those of the near placement."""
    lens = np.zeros(BIG_NT, np.int64)
    lens[BIG_LIVE] = TLENS
    offs = np.zeros(BIG_NT + 1, np.int64)
    offs[0] = front
    offs[1:] = front + np.cumsum(lens)
    return offs


def repeated_queries(which, at=4):
    """(description, offsets, the world's query index of each) of the world's queries `which`, back to back at byte `at`."""
    p, offs = packed(world()["queries"], at, which)
    return far_buffer(p, at), offs, list(which)


def rank_pairs(pairs, results, nqueries, ntargets, top, min_score):
    """The selection over a scored pair list by the rule of include/swhip.h, in numpy: an entry qualifies when its query and target are
    in range and max_score >= min_score; a row is ordered by score descending, then target, then list position; duplicates are kept.
    Returns (hits (nqueries, top, 3) of (target, max_pos, max_score), unused entries (-1, 0, 0); nhits (nqueries,))."""
    pairs, results = np.asarray(pairs, np.int64).reshape(-1, 2), np.asarray(results, np.int64).reshape(-1, 3)
    hits = np.zeros((nqueries, top, 3), np.int64)
    hits[:, :, 0] = -1
    nhits = np.zeros(nqueries, np.int64)
    ok = (pairs[:, 0] >= 0) & (pairs[:, 0] < nqueries) & (pairs[:, 1] >= 0) & (pairs[:, 1] < ntargets) & (results[:, 1] >= min_score)
    for q in range(nqueries):
        at = np.nonzero(ok & (pairs[:, 0] == q))[0]
        at = at[np.lexsort((at, pairs[at, 1], -results[at, 1]))][:top]
        nhits[q] = len(at)
        hits[q, :len(at)] = np.stack([pairs[at, 1], results[at, 0], results[at, 1]], axis=1)
    return hits, nhits


def sparse_rank(live_rows, top, min_score):
    """The reference's rank order over 2^24 targets of which only BIG_LIVE can score: live_rows (nq, 9, 3).  Targets that score 0 rank
    by ascending index, so the first top + 9 indices hold every one a row of `top` can name."""
    cand = sorted(set(BIG_LIVE) | set(range(top + NT)))
    small = np.zeros((live_rows.shape[0], len(cand), 3), np.int64)
    small[:, [cand.index(k) for k in BIG_LIVE]] = live_rows
    hits, nhits = rank_order(small, top, min_score)
    used = hits[:, :, 0] >= 0
    hits[:, :, 0][used] = np.array(cand, np.int64)[hits[:, :, 0][used]]
    return hits, nhits


# ---- a pair list of 2^28 entries: 4 GiB of pairs, 6 GiB of results ----

BIG_NPAIRS = 2**28
_C = WRAP // 24                                                  # the entry whose result crosses byte 2^32
BIG_LIVE_PAIRS = [0, 1] + list(range(_C - 6, _C + 6)) + list(range(BIG_NPAIRS - 27, BIG_NPAIRS))   # (entry 2^32 // 16 - 1 is the list's last)
assert BIG_NPAIRS * 16 == WRAP and BIG_NPAIRS * 24 > WRAP and BIG_LIVE_PAIRS[-1] == WRAP // 16 - 1 and len(BIG_LIVE_PAIRS) == 41


def big_live_pairs():
    """(41, 2) int64: the (query, non-empty target) pairs of the live entries, every combination in turn.  The last chunk holds 27 of
    them, an odd number: some query, and so some (query, bucket) cell of the packed kernel, gets an odd count there."""
    combos = [(q, t) for t in range(NT) if TLENS[t] for q in range(NQ)]
    return np.array([combos[(7 * i) % len(combos)] for i in range(len(BIG_LIVE_PAIRS))], np.int64)


# ---- batch strides ----

BATCH = {"cols": 513, "rows": 65, "npairs": 5, "stride": BATCH_STRIDE, "wrap": 4 * BATCH_STRIDE - WRAP}
assert BATCH["wrap"] == 256 and BATCH["stride"] % 16 == 0


@functools.lru_cache(maxsize=None)
def batch_case():
    """{"A" (5, 513), "B" (5, 65), "a_decoy" (513,), "b_decoy" (65,)} over ACGT.  Pair 4 starts at byte 2^32 + 256 of either buffer.  The
    wrapped address, byte 256, lies inside pair 0's a (its letters 256 .. 512, then 256 letters of a_decoy) and behind pair 0's b
    (b_decoy): "a_wrapped" is what a kernel that drops the high half would read as pair 4's a."""
    rng = np.random.default_rng(3205)
    dna = np.frombuffer(b"ACGT", np.uint8)
    c = {"A": rng.choice(dna, (5, 513)), "B": rng.choice(dna, (5, 65)), "a_decoy": rng.choice(dna, 513), "b_decoy": rng.choice(dna, 65)}
    c["a_wrapped"] = np.concatenate([c["A"][0, 256:], c["a_decoy"][:256]])
    for a in c.values():
        a.setflags(write=False)
    return c


# ---- C. far internal workspaces ----

PROFILE_NQ, PROFILE_QLEN, PROFILE_MIB = 8100, 2049, 6144
# 257 profile rows x 3072 padded columns per query: 8100 queries need 6 394 982 400 bytes, one group under 6144 MiB and beyond 2^32
# (tests/search_multi_plan_driver.cpp confirms both; 8300 queries would need 6 552 883 200 bytes and split into two groups)
assert WRAP < PROFILE_NQ * 257 * 3072 <= PROFILE_MIB * 2**20 < 8300 * 257 * 3072
PROFILE_TARGETS = [2, 3]                                         # the world's targets of 5 and 64 letters


@functools.lru_cache(maxsize=None)
def profile_case():
    """{"distinct": the five queries tiled and cut to 2049 letters, "which": the distinct query of each of the 8100, "qpacked", "qoffs",
    "packed", "offs"}."""
    w = world()
    distinct = [np.resize(q, PROFILE_QLEN).astype(np.uint8) for q in w["queries"]]
    which = np.arange(PROFILE_NQ) % NQ
    qpacked = np.concatenate([np.zeros(4, np.uint8)] + [distinct[k] for k in which])
    qoffs = 4 + PROFILE_QLEN * np.arange(PROFILE_NQ + 1, dtype=np.int64)
    p, offs = packed([w["targets"][k] for k in PROFILE_TARGETS], 3)
    out = {"distinct": distinct, "which": which, "qpacked": qpacked, "qoffs": qoffs, "packed": np.concatenate([np.zeros(3, np.uint8), p]), "offs": offs}
    for a in distinct + [which, qpacked, qoffs, out["packed"], offs]:
        a.setflags(write=False)
    return out


_PROFILE_EXPECTED = {}


def profile_expected(checker):
    """{"R": (5, 2, 3) under GAPS[0], "U": (5, 2)} of the five distinct queries."""
    if not _PROFILE_EXPECTED:
        c, ts = profile_case(), [world()["targets"][k] for k in PROFILE_TARGETS]
        _PROFILE_EXPECTED.update({"R": _table(checker, c["distinct"], ts, table24(), GAPS[0]), "U": _ungapped(c["distinct"], ts, table24())})
        for a in _PROFILE_EXPECTED.values():
            a.setflags(write=False)
    return _PROFILE_EXPECTED


SLOTS = {"qlen": 2049, "tlens": [1099, 1100, 1101], "top": 2048, "workspace_mib": 8192, "checkpoint_rows": 1024}
# tests/align_ckpt_plan_driver.cpp drives both planners.  On 256 CUs, with at least two workgroups of the 16-column kernel per CU, the 2048
# entries of the one query get 2048 slots: whole direction matrices of 1101 x 3072 = 3 382 272 bytes (6 926 893 056 in all), and under
# "align_checkpoint_rows" = 1024 slots of 3072 x (1024 + 8) = 3 170 304 bytes (6 492 782 592).  The GPU test plans with the driver itself.


@functools.lru_cache(maxsize=None)
def slots_case():
    """{"query" (2049 letters), "targets": three slices of it of about 1100 letters with every tenth letter replaced and a few letters
    dropped or doubled, so that the alignments run through most of a direction matrix}."""
    rng = np.random.default_rng(3206)
    q = rng.choice(PROTEIN, SLOTS["qlen"]).astype(np.uint8)
    targets = []
    for k, n in enumerate(SLOTS["tlens"]):
        t = q[100 + 300 * k:100 + 300 * k + n + 4].copy()
        t[::10] = rng.choice(PROTEIN, len(t[::10]))
        t = np.delete(t, [200, 201, 500, 800 + k])                # four letters missing from the target ...
        t[600:603] = t[599]                                       # ... and a repeat
        assert len(t) == n
        targets.append(t.astype(np.uint8))
    for a in [q] + targets:
        a.setflags(write=False)
    return {"query": q, "targets": targets}


_SLOTS_EXPECTED = {}


def slots_expected(checker):
    """[(sw_alignment row, ops)] of the three targets under GAPS[0]: the rule's walk over the checker's matrices."""
    if not _SLOTS_EXPECTED:
        c = slots_case()
        _SLOTS_EXPECTED["aln"] = [rule_alignment(checker, c["query"], t, table24(), *GAPS[0])[:2] for t in c["targets"]]
    return _SLOTS_EXPECTED["aln"]


# ---- a count matrix beyond 4 GiB ----

COUNT_NQ, COUNT_QLEN, COUNT_NL, COUNT_TOP = 5, 2**20 - 1, 256, 4
COUNT_PRIOR, COUNT_PW, COUNT_INC = 13, 3, 20                    # a constant prior above SMAX: an unobserved entry comes out as SMAX
assert COUNT_NQ * COUNT_QLEN > 2**22 and COUNT_NQ * COUNT_QLEN * COUNT_NL * 4 > WRAP          # the int32 counts pass 4 GiB
assert (COUNT_NQ - 1) * COUNT_QLEN * COUNT_NL * 4 == WRAP - 4096                              # the last query's counts begin 4 columns below byte 2^32
assert SMAX * min(COUNT_QLEN, max(TLENS)) < 2**24 and max(TLENS) == 301                       # what the call checks of smax and the sizes


@functools.lru_cache(maxsize=None)
def count_case():
    """Five queries of 2^20 - 1 columns over 256 letters against the small world, top = 4.  Used entries in the first and the last query
    only -- the entries of the queries 1 and 3 fail one guard of the rule each, query 2 has a count of 0 --, every one `nops` 'M' from
    (q_begin, t_begin); one runs past its target's end, the last one past the query's.  Every used entry of the last query pairs
    columns >= 4, so its counts lie wholly beyond byte 2^32, and the count 2^32 bytes below each (the first query's column j - 4, same
    letter) is an expected zero (asserted).  {"qoffs", "hits", "nhits", "aln", "ops", "cap", "weights", "windows": [(query, first
    column, columns, entry)], "compact": the windows as a case of tests/pssm_hits_cases.py -- one query per window, top 1 --, which the
    numpy rule can walk: the prior is constant and no two used entries of a query share a column}."""
    import types
    w = world()
    L, top = COUNT_QLEN, COUNT_TOP
    packed_, offs = packed(w["targets"], 0)
    targets = [7, 8, 6, 4]                                       # 300, 301, 127 and 65 letters
    begins = {0: [0, 2000, 70000, 500000], COUNT_NQ - 1: [10000, 600000, 900000, L - 62]}
    cap = max(TLENS) + 3
    hits = np.zeros((COUNT_NQ, top, 3), np.int64)
    aln = np.zeros((COUNT_NQ, top, 7), np.int64)
    ops = np.full((COUNT_NQ * top, cap), OPS_POISON, np.uint8)
    weights = np.array([[3, 1, 2, 5]] * COUNT_NQ, np.int32)
    windows = []
    for q in range(COUNT_NQ):
        for r, t in enumerate(targets):
            hits[q, r] = (t, 0, 50)
            tb = 10 if r == 1 else 0                             # entry 1 runs past its target's end
            aln[q, r] = (0, 50, begins.get(q, begins[0])[r], tb, 0, 0, TLENS[t])
            ops[q * top + r, :TLENS[t]] = ord("M")
            if q in begins:
                windows.append((q, begins[q][r], min(TLENS[t], L - begins[q][r]), r))
    hits[1, :, 0] = (-1, NT, 2**40, -2**40)                      # query 1: no target in range
    aln[3, :, 1] = COUNT_INC - 1                                 # query 3: below include_min_score
    aln[3, 2, 6], aln[3, 3, 6] = 0, cap + 1
    nhits = np.array([top, top, 0, top + 3, top], np.int64)
    assert windows[-1][2] == 62 < TLENS[4]                       # the last entry runs past the end of the last query
    cols = {q: set() for q in begins}
    for q, c0, n, _ in windows:
        assert not cols[q] & set(range(c0, c0 + n))              # no two entries of a query share a column
        cols[q] |= set(range(c0, c0 + n))
    assert min(cols[COUNT_NQ - 1]) >= 4 and not {j - 4 for j in cols[COUNT_NQ - 1]} & cols[0]
    c = types.SimpleNamespace()
    c.letters, c.smax, c.other = pssm_letters(COUNT_NL), SMAX, OTHER
    c.qoffs = np.concatenate([[0], np.cumsum([n for _, _, n, _ in windows])]).astype(np.int64)
    c.prior = np.full((int(c.qoffs[-1]), COUNT_NL), COUNT_PRIOR, np.int8)
    c.packed, c.offs, c.sub = packed_, offs, table24()
    c.hits = np.stack([hits[q, r] for q, _, _, r in windows])[:, None, :]
    c.aln = np.stack([aln[q, r] for q, _, _, r in windows])[:, None, :].copy()
    c.aln[:, 0, 2] = 0
    c.nhits, c.cap = None, cap
    c.ops = np.stack([ops[q * top + r] for q, _, _, r in windows])
    c.weights = np.array([[weights[q, r]] for q, _, _, r in windows], np.int32)
    out = {"qoffs": COUNT_QLEN * np.arange(COUNT_NQ + 1, dtype=np.int64), "hits": hits, "nhits": nhits, "aln": aln, "ops": ops, "cap": cap,
           "weights": weights, "windows": windows, "compact": c}
    for a in (out["qoffs"], hits, nhits, aln, ops, weights, c.prior, c.hits, c.aln, c.ops, c.weights):
        a.setflags(write=False)
    return out


def count_want():
    """(new matrix, counts) of count_case()["compact"] by the numpy rule, each (columns of all windows, 256)."""
    import pssm_hits_cases as hc
    c = count_case()["compact"]
    m, counts, used = hc.reference(c, COUNT_PW, COUNT_INC, c.weights)
    assert used.all() and (counts.sum(axis=1) > 0).sum() > 1000 and (m != SMAX).any()
    return m, counts
