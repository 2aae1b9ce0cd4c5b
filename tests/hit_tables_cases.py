"""Seeded hit tables for tests/test_hit_tables_agree_*.py: one set of tables (hits, nhits, aln, ops) that the PSSM update, the hit
weights and the query-anchored alignment all read, every entry either unused in one of the seven ways include/swhip.h names or used
with random begins and random op rows that are free to run past either end.  Nothing here restates the rule: the tests compare what
the three calls make of the same tables with each other."""
import types

import numpy as np

LETTERS = np.frombuffer(b"ACGT", np.uint8)
QLENS = (1, 64, 130)                    # 130 crosses the 64-column tile twice, and the walk's 64-op chunk
TLENS = (0, 1, 63, 64, 65, 200)
TOP, OPS_CAP, INCLUDE_MIN, PER_HIT = 8, 200, 20, 16
SCORING = (LETTERS, -4, 127, -8, -1)
UNUSED_KINDS = 7
SEEDS = (1, 2, 3)


def tables(seed):
    rng = np.random.default_rng(seed)
    c = types.SimpleNamespace(top=TOP, cap=OPS_CAP, include_min=INCLUDE_MIN)
    nq, nt = len(QLENS), len(TLENS)
    c.qoffs = np.concatenate([[3], 3 + np.cumsum(QLENS)]).astype(np.int64)
    c.offs = np.concatenate([[5], 5 + np.cumsum(TLENS)]).astype(np.int64)
    c.packed = rng.choice(LETTERS, int(c.offs[-1])).astype(np.uint8)          # never '-'
    c.nhits = np.array([TOP, rng.integers(0, TOP + 1), rng.integers(-1, TOP + 3)], np.int64)
    c.hits = np.zeros((nq, TOP, 3), np.int64)
    c.aln = np.zeros((nq, TOP, 7), np.int64)
    c.ops = np.zeros((nq, TOP, OPS_CAP), np.uint8)
    c.kind = np.zeros((nq, TOP), np.int64)                                    # 0: used, 1..7: the way it is unused
    for q, qlen in enumerate(QLENS):
        for r in range(TOP):
            t = int(rng.integers(0, nt))
            tlen = TLENS[t]
            score = INCLUDE_MIN + int(rng.integers(0, 50))                    # from include_min_score itself on
            nops = int(rng.choice((1, 64, 65, OPS_CAP, int(rng.integers(1, OPS_CAP + 1))), p=(0.05, 0.05, 0.05, 0.15, 0.7)))   # the edges of the guard and of the chunk
            qb, tb = int(rng.integers(0, qlen + 1)), int(rng.integers(0, tlen + 1))
            kind = int(rng.integers(1, UNUSED_KINDS + 1)) if rng.random() < 0.45 else 0
            if kind == 1:
                t = -1
            elif kind == 2:
                t = nt
            elif kind == 3:
                score = INCLUDE_MIN - 1
            elif kind == 4:
                nops = 0
            elif kind == 5:
                nops = OPS_CAP + 1
            elif kind == 6:
                qb = (-1, qlen + 1)[int(rng.integers(0, 2))]
            elif kind == 7:
                tb = (-1, tlen + 1)[int(rng.integers(0, 2))]
            if rng.random() < 0.3:
                row = np.full(OPS_CAP, ord("M"), np.uint8)
            else:                                                             # about 70 % 'M', 12 % 'I', 12 % 'D', plus 'X' and 0 bytes
                row = rng.choice(np.frombuffer(b"MID" + b"X\x00", np.uint8), OPS_CAP, p=(0.70, 0.12, 0.12, 0.03, 0.03)).astype(np.uint8)
            c.hits[q, r] = (t, 0, score)
            c.aln[q, r] = (0, score, qb, tb, 0, 0, nops)
            c.ops[q, r] = row
            c.kind[q, r] = kind
    return c


def host_legs(swamd, c):
    """(counts, weights, cols, rows) of the three host legs on the tables of c."""
    nq = len(QLENS)
    prior = (np.zeros((int(c.qoffs[-1]), len(LETTERS)), np.int8), c.qoffs)
    sub = swamd.submat_match(2, -3)
    _, counts = swamd.pssm_from_hits_host(prior, (c.packed, c.offs), SCORING, (sub, 1, c.include_min), c.hits, c.nhits, c.aln, c.ops, want_counts=True)
    weights = swamd.pssm_hit_weights_host(c.qoffs, (c.packed, c.offs), SCORING, (PER_HIT, c.include_min), c.hits, c.nhits, c.aln, c.ops)
    cols, rows, _ = swamd.msa_from_hits_host(c.qoffs, (c.packed, c.offs), c.include_min, c.hits, c.nhits, c.aln, c.ops)
    return counts, weights, cols, rows.reshape(nq, c.top)


def assert_agree(c, counts, weights, cols, rows):
    """The three calls read the tables the same way."""
    at, pairs = 0, 0
    for q, qlen in enumerate(QLENS):
        mat = np.asarray(cols, np.uint8)[at * c.top:(at + qlen) * c.top].reshape(c.top, qlen)
        letters = mat != ord("-")
        assert (counts[at:at + qlen].sum(axis=1) == letters.sum(axis=0)).all(), q
        assert (letters.sum(axis=1) == rows[q]["nmatch"]).all(), q
        assert ((rows[q]["len"] == 0) | (rows[q]["len"] == qlen + rows[q]["ninsert"])).all(), q
        assert (weights[q][rows[q]["nmatch"] == 0] == 0).all(), q
        assert (weights[q].sum() > 0) == bool((rows[q]["nmatch"] > 0).any()), q
        at += qlen
        pairs += int(letters.sum())
    return pairs
