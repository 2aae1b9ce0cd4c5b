"""CPU: the host leg of the hit-table alignment (sw_align_affine_hits_host) against sw_align_affine_host per query, entry by entry --
tables with duplicates, rows with nhits 0, below and above top, NULL nhits, targets outside the database --, the zero entries and
untouched ops rows against a poison pattern, the argument rules, and one case against the independent checker.  No GPU is needed."""
import ctypes

import numpy as np
import pytest

from affine_cases import GAPS, PROTEIN, checker, random_submat  # noqa: F401
from align_cases import expected, pack, replay

POISON = 0x5A
EINVAL = -22


def make_case(rng, nq=5, top=6):
    queries = [rng.choice(PROTEIN, int(n)).astype(np.uint8) for n in (1, 40, 130, 64, 257)[:nq]]
    targets = [rng.choice(PROTEIN, int(n)).astype(np.uint8) for n in [0, 1, 63, 64, 65] + list(rng.integers(2, 200, 7))]
    targets.append(np.concatenate([queries[2][:50], queries[2][55:]]))                 # related to a query: alignments with gaps
    targets.append(np.concatenate([queries[4][:90], rng.choice(PROTEIN, 3).astype(np.uint8), queries[4][90:]]))
    nt = len(targets)
    hits = rng.integers(0, nt, (nq, top)).astype(np.int64)
    hits[0, :3] = (3, 3, 3)                                                             # duplicates
    hits[1, 1], hits[1, 3], hits[2, 0] = -1, nt, -7                                     # outside the database, inside the used part
    hits[2, 1], hits[4, 0] = nt - 2, nt - 1
    nhits = np.array([top, 4, top + 3, 0, 2][:nq], np.int64)                            # full, below top, above top (clamped), none, two
    table = np.stack([hits, rng.integers(0, 99, hits.shape), rng.integers(0, 99, hits.shape)], axis=-1).astype(np.int64)   # only `target` is read
    return queries, targets, table, nhits


def raw_call(swamd, queries, targets, sub, go, ge, table, nhits, cap, use_ops=True):
    """The C call on poisoned outputs: (rc, aln (nq, top, 7), ops (nq, top, cap))."""
    qp, qo = pack(queries)
    tp, to = pack(targets)
    nq, top = table.shape[:2]
    aln = np.full((nq, top, 7), 0x5A5A5A5A5A5A5A5A, np.int64)
    ops = np.full((nq, top, max(1, cap)), POISON, np.uint8)
    sc = swamd._Affine(sub.ctypes.data, go, ge)
    table = np.ascontiguousarray(table)
    rc = swamd.lib().sw_align_affine_hits_host(qp.ctypes.data, qo.ctypes.data, nq, tp.ctypes.data, to.ctypes.data, len(targets), ctypes.byref(sc),
                                               table.ctypes.data, nhits.ctypes.data if nhits is not None else None, top, aln.ctypes.data,
                                               ops.ctypes.data if use_ops else None, cap if use_ops else 0)
    return rc, aln, ops


def check_against_single_query_leg(swamd, queries, targets, sub, go, ge, table, nhits, aln, ops, cap):
    nq, top = table.shape[:2]
    nt = len(targets)
    tp, to = pack(targets)
    for q in range(nq):
        used = top if nhits is None else int(np.clip(nhits[q], 0, top))
        for r in range(top):
            k = int(table[q, r, 0])
            if r < used and 0 <= k < nt:
                ea, eo = swamd.align_affine_host(queries[q], (tp, to), sub, go, ge, [k])
                assert tuple(aln[q, r]) == tuple(ea[0]), f"entry {q, r} (target {k})"
                n = int(ea[0, 6])
                if n <= cap:
                    assert ops[q, r, :n].tobytes() == eo[0]
                    assert np.all(ops[q, r, n:] == POISON)
                # (nops > ops_cap: that row's bytes are unspecified; the neighbours' rows are checked like any other)
            else:
                assert not aln[q, r].any(), f"entry {q, r} must be all zeros"
                assert np.all(ops[q, r] == POISON), f"ops row of entry {q, r} was touched"


@pytest.mark.parametrize("go,ge", GAPS[:3])
@pytest.mark.parametrize("with_counts", [True, False])
def test_equals_the_single_query_leg(swamd, go, ge, with_counts):
    rng = np.random.default_rng(100 - go)
    queries, targets, table, nhits = make_case(rng)
    sub = random_submat(rng)
    cap = 257 + 260
    counts = nhits if with_counts else None
    rc, aln, ops = raw_call(swamd, queries, targets, sub, go, ge, table, counts, cap)
    assert rc == 0, swamd.lib().sw_last_error()
    check_against_single_query_leg(swamd, queries, targets, sub, go, ge, table, counts, aln, ops, cap)
    assert aln[..., 6].max() > 100                                                     # long alignments among them
    # the Python wrapper: the same rows, ops as lists
    waln, wops = swamd.align_affine_hits_host(queries, targets, (sub, go, ge), table, counts)
    assert np.array_equal(waln, aln) and waln.shape == (len(queries), table.shape[1], 7)
    assert all(wops[q][r] == ops[q, r, :aln[q, r, 6]].tobytes() for q in range(len(queries)) for r in range(table.shape[1]))


def test_small_ops_cap_and_no_ops(swamd):
    rng = np.random.default_rng(8)
    queries, targets, table, nhits = make_case(rng)
    sub = random_submat(rng)
    _, full, _ = raw_call(swamd, queries, targets, sub, -3, -2, table, nhits, 600)
    cap = 20
    rc, aln, ops = raw_call(swamd, queries, targets, sub, -3, -2, table, nhits, cap)
    assert rc == 0 and np.array_equal(aln, full)                                        # the true nops, whatever fits
    assert (full[..., 6] > cap).any() and ((full[..., 6] > 0) & (full[..., 6] <= cap)).any()
    check_against_single_query_leg(swamd, queries, targets, sub, -3, -2, table, nhits, aln, ops, cap)
    rc, aln, ops = raw_call(swamd, queries, targets, sub, -3, -2, table, nhits, 0, use_ops=False)
    assert rc == 0 and np.array_equal(aln, full) and np.all(ops == POISON)


def test_against_the_independent_checker(swamd, checker):  # noqa: F811
    rng = np.random.default_rng(21)
    queries, targets, table, nhits = make_case(rng)
    sub = random_submat(rng)
    go, ge = -10, -1
    aln, ops = swamd.align_affine_hits_host(queries, targets, (sub, go, ge), table, nhits)
    seen = 0
    for q in range(len(queries)):
        for r in range(min(int(nhits[q]), table.shape[1])):
            k = int(table[q, r, 0])
            if not 0 <= k < len(targets):
                continue
            row, eops, _ = expected(checker, queries[q], targets[k], sub, go, ge)
            assert tuple(int(x) for x in aln[q, r]) == row and ops[q][r] == eops, f"entry {q, r} (target {k})"
            replay(queries[q], targets[k], sub, go, ge, aln[q, r], ops[q][r])
            seen += 1
    assert seen >= 10


def test_argument_rules(swamd):
    L = swamd.lib()
    rng = np.random.default_rng(2)
    queries, targets, table, nhits = make_case(rng)
    sub = random_submat(rng)
    qp, qo = pack(queries)
    tp, to = pack(targets)
    nq, top = table.shape[:2]
    aln = np.full((nq, top, 7), 0x5A5A5A5A5A5A5A5A, np.int64)
    ops = np.full((nq, top, 600), POISON, np.uint8)

    def call(qoffs=qo, offs=to, go=-3, ge=-1, top=top, hits=table.ctypes.data, alnp=aln.ctypes.data, opsp=ops.ctypes.data, cap=600, subp=sub.ctypes.data,
             nq=nq, nt=len(targets)):
        sc = swamd._Affine(subp, go, ge)
        qoffs, offs = np.ascontiguousarray(qoffs, np.int64), np.ascontiguousarray(offs, np.int64)
        return L.sw_align_affine_hits_host(qp.ctypes.data, qoffs.ctypes.data, nq, tp.ctypes.data, offs.ctypes.data, nt, ctypes.byref(sc), hits,
                                           nhits.ctypes.data, top, alnp, opsp, cap)

    bad_q, bad_t, empty_q = qo.copy(), to.copy(), qo.copy()
    bad_q[2] = bad_q[1] - 1
    bad_t[3] = bad_t[2] - 1
    empty_q[1] = empty_q[0]
    refusals = [dict(top=0), dict(top=swamd.SW_TOP_MAX + 1), dict(hits=None), dict(alnp=None), dict(cap=-1), dict(opsp=None, cap=5),
                dict(go=1), dict(ge=1), dict(go=-(1 << 24), ge=-1), dict(qoffs=bad_q), dict(qoffs=empty_q), dict(offs=bad_t), dict(nq=-1), dict(nt=-1),
                dict(subp=None)]
    for kw in refusals:
        assert call(**kw) == EINVAL, kw
        assert L.sw_last_error()
        assert np.all(aln == 0x5A5A5A5A5A5A5A5A) and np.all(ops == POISON), f"{kw}: an output was touched on refusal"
    assert b"top" in (call(top=0), L.sw_last_error())[1] and b"ops_cap" in (call(cap=-1), L.sw_last_error())[1]
    assert call(nq=0) == 0 and np.all(aln == 0x5A5A5A5A5A5A5A5A)                        # nothing to do
    assert call(opsp=None, cap=0) == 0 and np.all(ops == POISON)                        # coordinates only
    assert call() == 0 and not np.all(aln == 0x5A5A5A5A5A5A5A5A)
    # a 24-bit score bound taken over the longest query against the longest target
    big = np.full((256, 256), 127, np.int8)
    long_q = np.zeros(1 << 18, np.uint8)
    qo2, to2 = np.array([0, 1 << 18], np.int64), np.array([0, 1 << 18], np.int64)
    sc = swamd._Affine(big.ctypes.data, -1, -1)
    one = np.zeros((1, 1, 3), np.int64)
    out = np.zeros(7, np.int64)
    assert L.sw_align_affine_hits_host(long_q.ctypes.data, qo2.ctypes.data, 1, long_q.ctypes.data, to2.ctypes.data, 1, ctypes.byref(sc), one.ctypes.data,
                                       None, 1, out.ctypes.data, None, 0) == EINVAL and b"2^24" in L.sw_last_error()
