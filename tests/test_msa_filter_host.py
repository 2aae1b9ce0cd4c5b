"""CPU: sw_msa_filter_host (the host leg of sw_msa_filter_device) against the rule of include/swhip.h on hand-made column rows --
identical rows, subsets, both inequalities at exact equality from both sides, the greedy chain, max_ident_pct 101, rows without a
letter, the query with and without letters, idempotence, independence of the queries, in place, every SW_EINVAL -- and on real tables:
sameq equals nident of sw_msa_row."""
import ctypes

import numpy as np
import pytest

import msa_cases as mc
import msa_filter_cases as fc

DASH = fc.DASH


def run(swamd, rows, ident, cover, query=None):
    """One query of the given (top, qlen) rows -> keep as a list."""
    rows = np.asarray(rows, np.uint8)
    top, qlen = rows.shape
    q = [np.asarray(query, np.uint8)] if query is not None else np.array([0, qlen], np.int64)
    keep, nkept, _ = swamd.msa_filter_host(rows.reshape(-1), q, top, ident, cover)
    assert int(nkept[0]) == int(keep.sum())
    return keep[0].tolist()


def letters(n, qlen, byte=ord("A")):
    row = np.full(qlen, DASH, np.uint8)
    row[:n] = byte
    return row


def test_identical_rows_only_the_first_is_kept(swamd):
    row = np.frombuffer(b"MKV-LAAGIT", np.uint8)
    for u in (1, 2, 7, 70):
        assert run(swamd, np.tile(row, (u, 1)), 90, 0) == [1] + [0] * (u - 1)


@pytest.mark.parametrize("ident", [1, 50, 90, 100])
def test_a_subset_of_a_kept_row_is_dropped(swamd, ident):
    full = np.frombuffer(b"ACDEFGHIKLMNPQRS", np.uint8)
    part = full.copy(); part[3:9] = DASH
    assert run(swamd, [full, part], ident, 0) == [1, 0]
    assert run(swamd, [part, full], 100, 0) == [1, 1]                # the longer row shows more than the kept one: 10 of 16 letters


def test_identity_at_exact_equality_from_both_sides(swamd):
    first = letters(100, 100)                                         # 100 letters 'A'
    for same, kept in ((45, 0), (44, 1)):
        row = np.full(100, DASH, np.uint8)
        row[:same] = ord("A")
        row[same:50] = ord("C")                                       # n_r = 50
        assert run(swamd, [first, row], 90, 0) == [1, kept], same     # 100 x 45 >= 90 x 50: dropped; 100 x 44 < 90 x 50: kept


def test_cover_at_exact_equality_from_both_sides(swamd):
    # qlen 200, min_cover_pct 35: 100 x 70 == 35 x 200 is covered, 69 letters are not
    assert run(swamd, [letters(70, 200)], 90, 35) == [1]
    assert run(swamd, [letters(69, 200)], 90, 35) == [0]
    assert run(swamd, [letters(1, 200)], 90, 0) == [1] and run(swamd, [letters(0, 200)], 90, 0) == [0]
    assert run(swamd, [letters(200, 200)], 90, 100) == [1] and run(swamd, [letters(199, 200)], 90, 100) == [0]


def test_greedy_chain(swamd):
    a, b, c = fc.chain_rows()
    assert run(swamd, [a, b, c], 90, 0) == [1, 0, 1]                  # B falls to A; C, redundant to B only, stays
    assert run(swamd, [b, c], 90, 0) == [1, 0]                        # ... and falls where B is kept
    assert run(swamd, [a, c], 90, 0) == [1, 1]


def test_max_ident_101_keeps_every_covered_row(swamd):
    row = np.frombuffer(b"WWWWWWWWWW", np.uint8)
    short = letters(4, 10, ord("W"))
    assert run(swamd, [row, row, short, row], 101, 50, query=row) == [1, 1, 0, 1]


def test_a_row_without_a_letter_is_never_kept_and_suppresses_nothing(swamd):
    dashes = np.full(12, DASH, np.uint8)
    row = np.frombuffer(b"ACDEFGHIKLMN", np.uint8)
    for ident in (1, 90, 101):
        assert run(swamd, [dashes, row, dashes, row], ident, 0) == [0, 1, 0, 0 if ident <= 100 else 1]
    # a target byte 0x2D is no letter either: the row shows its eleven other bytes
    odd = row.copy(); odd[5] = DASH
    assert run(swamd, [odd], 90, 100) == [0] and run(swamd, [odd], 90, 91) == [1]


def test_self_hit_with_and_without_the_query(swamd):
    query = np.frombuffer(b"MKVLAAGITRWQ", np.uint8)
    other = np.frombuffer(b"CCCCCCCCCCCC", np.uint8)
    assert run(swamd, [query, other], 90, 0, query=query) == [0, 1]
    assert run(swamd, [query, other], 90, 0) == [1, 1]
    near = query.copy(); near[0] = ord("C")                           # 11 of 12: 91.7 percent
    assert run(swamd, [near], 92, 0, query=query) == [1] and run(swamd, [near], 91, 0, query=query) == [0]
    # dropped against the query, the self-hit suppresses nothing: `near` would have fallen to it
    assert run(swamd, [query, near], 92, 0, query=query) == [0, 1] and run(swamd, [query, near], 91, 0) == [1, 0]


@pytest.mark.parametrize("top", [1, 2, 63, 64, 65, 100])
def test_families_equal_the_rule_restated(swamd, top):
    c = fc.families(top, top, (1, 3, 4, 5, 63, 64, 65, 255, 257), q0=7)
    for with_query in (True, False):
        q = (c.qpacked, c.qoffs) if with_query else c.qoffs
        keep, nkept, hits = swamd.msa_filter_host(c.cols, q, top, 90, 50, hits=c.hits)
        ekeep, enkept, ehits = fc.reference(c, 90, 50, with_query)
        assert (keep == ekeep).all() and (nkept == enkept).all() and (hits == ehits).all()
        assert (hits[..., 1:] == c.hits[..., 1:]).all() and (hits[..., 0][keep == 1] == c.hits[..., 0][keep == 1]).all()


def test_idempotent(swamd):
    """Filtering the filtered table and its re-built column rows changes nothing: a dropped entry's row is all '-' in the rows
    sw_msa_from_hits_host builds from the filtered table."""
    c = mc.real(swamd, 20, top=8)
    q = (c.qpacked, c.qoffs)
    nq, top = c.hits.shape[:2]
    ops = c.ops.reshape(nq, top, -1)
    cols = swamd.msa_from_hits_host(q, (c.packed, c.offs), c.include_min, c.hits, c.nhits, c.aln, ops)[0]
    keep, nkept, hits = swamd.msa_filter_host(cols, q, top, 60, 20, hits=c.hits)
    assert 0 < keep.sum() < keep.size
    cols2 = swamd.msa_from_hits_host(q, (c.packed, c.offs), c.include_min, hits, c.nhits, c.aln, ops)[0]
    keep2, nkept2, hits2 = swamd.msa_filter_host(cols2, q, top, 60, 20, hits=hits)
    assert (keep2 == keep).all() and (nkept2 == nkept).all() and (hits2 == hits).all()


def test_sameq_is_nident_on_real_tables(swamd):
    c = mc.real(swamd, 20, top=8)
    q = (c.qpacked, c.qoffs)
    nq, top = c.hits.shape[:2]
    cols, rows, _ = swamd.msa_from_hits_host(q, (c.packed, c.offs), c.include_min, c.hits, c.nhits, c.aln, c.ops.reshape(nq, top, -1))
    seen = set()
    for qi in range(nq):
        qlen = int(c.qoffs[qi + 1] - c.qoffs[qi])
        base = int(c.qoffs[qi]) * top
        for r in range(top):
            w = rows[qi, r]
            if w["nmatch"] == 0:
                continue
            row = cols[base + r * qlen:base + (r + 1) * qlen]
            n = int((row != DASH).sum())
            assert n == w["nmatch"]                                   # (no target holds 0x2D)
            # the row alone: kept against the query exactly when 100 x nident < pct x n_r, at the threshold from both sides
            t = -(-100 * int(w["nident"]) // n)                       # the least pct with 100 nident <= pct n
            for pct in {max(1, min(101, t + d)) for d in (-1, 0, 1)}:
                keep, _, _ = swamd.msa_filter_host(row, [c.queries[qi]], 1, pct, 0)
                assert int(keep[0, 0]) == (100 * int(w["nident"]) < pct * n), (qi, r, pct)
                seen.add(int(keep[0, 0]))
    assert seen == {0, 1}


def test_a_query_depends_on_no_other(swamd):
    c = fc.families(5, 20, (30, 7, 64, 129), q0=3)
    keep, nkept, hits = swamd.msa_filter_host(c.cols, (c.qpacked, c.qoffs), 20, 90, 50, hits=c.hits)
    for q in range(c.nq):
        g0, g1 = int(c.qoffs[q]), int(c.qoffs[q + 1])
        k1, n1, h1 = swamd.msa_filter_host(c.rows(q).reshape(-1), [c.qpacked[g0:g1]], 20, 90, 50, hits=c.hits[q:q + 1])
        assert (k1[0] == keep[q]).all() and n1[0] == nkept[q] and (h1[0] == hits[q]).all()


def _call(swamd, c, filt=(90, 50), **over):
    """The raw call; over: cols, queries, qoffs, nq, top, filter, hits, hits_out, keep, nkept by name."""
    f = swamd._MsaFilter(*filt)
    a = dict(cols=c.cols.ctypes.data, queries=c.qpacked.ctypes.data, qoffs=c.qoffs.ctypes.data, nq=c.nq, top=c.top, filter=ctypes.addressof(f),
             hits=None, hits_out=None, keep=None, nkept=None)
    a.update(over)
    return swamd.lib().sw_msa_filter_host(a["cols"], a["queries"], a["qoffs"], a["nq"], a["top"], ctypes.cast(a["filter"], ctypes.POINTER(swamd._MsaFilter))
                                          if a["filter"] else None, a["hits"], a["hits_out"], a["keep"], a["nkept"])


def test_in_place_and_each_output_alone(swamd):
    c = fc.families(9, 65, (40, 5), q0=1)
    ekeep, enkept, ehits = fc.reference(c, 90, 50)
    G = fc.GUARD
    hits = np.full(G + c.hits.size + G, 0x55, np.int64)
    hits[G:-G] = c.hits.reshape(-1)
    assert _call(swamd, c, hits=hits[G:].ctypes.data, hits_out=hits[G:].ctypes.data) == 0           # in place, no other output
    assert (hits[G:-G].reshape(ehits.shape) == ehits).all() and (hits[:G] == 0x55).all() and (hits[-G:] == 0x55).all()
    keep = np.full(G + ekeep.size + G, 0x55555555, np.int32)
    assert _call(swamd, c, keep=keep[G:].ctypes.data) == 0                                          # keep alone
    assert (keep[G:-G].reshape(ekeep.shape) == ekeep).all() and (keep[:G] == 0x55555555).all() and (keep[-G:] == 0x55555555).all()
    nkept = np.full(G + c.nq + G, 0x55, np.int64)
    keep[:] = 0x55555555
    assert _call(swamd, c, keep=keep[G:].ctypes.data, nkept=nkept[G:].ctypes.data) == 0
    assert (nkept[G:-G] == enkept).all() and (nkept[:G] == 0x55).all() and (nkept[-G:] == 0x55).all()


def test_refusals(swamd):
    c = fc.families(2, 4, (6, 9))
    keep = np.full(c.nq * c.top, 0x55555555, np.int32)
    hits = c.hits.copy()
    ok = dict(keep=keep.ctypes.data)
    assert _call(swamd, c, **ok) == 0
    keep[:] = 0x55555555
    neg = c.qoffs.copy(); neg[0] = -1
    empty = c.qoffs.copy(); empty[1] = empty[0]
    back = c.qoffs.copy(); back[1] = back[2] + 1
    long = np.array([0, 1 << 20], np.int64)
    for over in (dict(qoffs=None), dict(nq=-1), dict(qoffs=neg.ctypes.data), dict(qoffs=empty.ctypes.data), dict(qoffs=back.ctypes.data),
                 dict(qoffs=long.ctypes.data, nq=1), dict(top=0), dict(top=4097), dict(cols=None), dict(filter=None), dict(keep=None),
                 dict(keep=None, nkept=keep.ctypes.data), dict(hits_out=hits.ctypes.data), dict(keep=None, hits_out=hits.ctypes.data)):
        assert _call(swamd, c, **{**ok, **over}) == -22, over
    for filt in ((0, 50), (102, 50), (-5, 50), (90, -1), (90, 101)):
        assert _call(swamd, c, filt=filt, **ok) == -22, filt
    for filt in ((1, 0), (101, 100)):
        assert _call(swamd, c, filt=filt, **ok) == 0
    keep[:] = 0x55555555
    assert _call(swamd, c, nq=0, **ok) == 0 and (keep == 0x55555555).all() and (hits == c.hits).all()   # no query: nothing is written
