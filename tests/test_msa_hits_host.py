"""CPU: sw_msa_from_hits_host (the host leg of sw_db_msa_from_hits) against the pure-Python replay of the rule in tests/msa_cases.py --
hand-written tables at every edge the rule names, garbage tables, real tables of the host search and alignment --, the cross-checks
against sw_pssm_from_hits_host and the targets themselves, the cap of the A3M buffer, every SW_EINVAL, and sw_write_a3m."""
import types

import numpy as np
import pytest

import msa_cases as mc


@pytest.mark.parametrize("nalpha", [4, 20])
@pytest.mark.parametrize("nhits", [False, True])
def test_hand_written_tables(swamd, nalpha, nhits):
    c = mc.synthetic(nalpha, 12, nhits=nhits)
    mc.assert_matches_reference(c, mc.host_leg(swamd, c))


@pytest.mark.parametrize("nalpha", [4, 20])
def test_one_column_and_top_one(swamd, nalpha):
    c = mc.synthetic(nalpha, 30, qlens=(1,))
    mc.assert_matches_reference(c, mc.host_leg(swamd, c))
    c = mc.synthetic(nalpha, 1, qlens=(1, 5, 64, 70, 130) * 6)
    mc.assert_matches_reference(c, mc.host_leg(swamd, c))


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_garbage_tables(swamd, seed):
    c = mc.garbage(seed, nalpha=(4, 20)[seed % 2])
    mc.assert_matches_reference(c, mc.host_leg(swamd, c))


def test_long_op_rows(swamd):
    c = mc.long_ops_case()
    mc.assert_matches_reference(c, mc.host_leg(swamd, c))


@pytest.mark.parametrize("nalpha", [4, 20])
def test_null_queries_count_no_identity(swamd, nalpha):
    c = mc.synthetic(nalpha, 12)
    got = mc.host_leg(swamd, c, null_queries=True)
    mc.assert_matches_reference(c, got, null_queries=True)
    assert all(w[3] == 0 for w in got[1]) and any(w[2] > 0 for w in got[1])
    c = mc.synthetic(nalpha, 12, with_letters=False)
    mc.assert_matches_reference(c, mc.host_leg(swamd, c))


@pytest.mark.parametrize("nalpha", [4, 20])
def test_the_cap_of_the_a3m_buffer(swamd, nalpha):
    c = mc.synthetic(nalpha, 12)
    _, rows, _, total, _ = mc.reference(c)
    boundary = [o for o, n, *_ in rows if n > 0 and 0 < o < total]
    for cap in (total, total - 1, 0, boundary[len(boundary) // 2], total + 5):
        mc.assert_matches_reference(c, mc.host_leg(swamd, c, a3m_cap=cap), a3m_cap=cap)


def test_outputs_alone(swamd):
    c = mc.synthetic(20, 12)
    mc.assert_matches_reference(c, mc.host_leg(swamd, c, want_rows=False, want_a3m=False))       # the column rows alone
    mc.assert_matches_reference(c, mc.host_leg(swamd, c, want_cols=False))                         # the A3M alone
    mc.assert_matches_reference(c, mc.host_leg(swamd, c, want_cols=False, want_a3m=False))         # a sizing call


def test_no_query_and_no_target(swamd):
    c = mc.synthetic(20, 3)
    e = types.SimpleNamespace(**vars(c))
    e.offs, e.packed = np.array([0], np.int64), np.zeros(1, np.uint8)
    cols, rows, a3m, total = mc.host_leg(swamd, e, a3m_cap=4)
    assert set(cols) == {ord("-")} and total == 0 and all(w == (0, 0, 0, 0, 0) for w in rows) and (a3m == -1).all() and len(a3m) == 4
    z = np.zeros(1, np.int64)
    assert swamd.lib().sw_msa_from_hits_host(None, z.ctypes.data, 0, c.packed.ctypes.data, c.offs.ctypes.data, len(c.offs) - 1, 0, z.ctypes.data, None, 1,
                                             z.ctypes.data, z.ctypes.data, 1, z.ctypes.data, None, None, 0, None) == 0


@pytest.mark.parametrize("nalpha", [4, 20])
def test_real_tables_against_the_update_and_the_targets(swamd, nalpha):
    c = mc.real(swamd, nalpha)
    got = mc.host_leg(swamd, c)
    mc.assert_matches_reference(c, got)
    cols, rows, a3m, total = got
    nq, top = c.hits.shape[:2]
    # the per-column letter histogram of the column rows is the count matrix of the update, unweighted, at the same include_min_score
    letters = mc.ALPHABETS[nalpha]
    m, moffs = swamd.pssm_from_queries(c.queries, c.sub, letters)
    sc = (letters, -4, 127, -8, -1)
    _, counts = swamd.pssm_from_hits_host((m, moffs), (c.packed, c.offs), sc, (c.sub, 1, c.include_min), c.hits, c.nhits, c.aln, c.ops.reshape(nq, top, -1),
                                          want_counts=True)
    at = 0
    for q in range(nq):
        qlen = int(c.qoffs[q + 1] - c.qoffs[q])
        mat = np.frombuffer(cols, np.uint8)[at * top:(at + qlen) * top].reshape(top, qlen)
        hist = np.stack([(mat == x).sum(axis=0) for x in letters], axis=1)
        assert (hist == counts[at:at + qlen]).all()
        at += qlen
    assert counts.sum() > 0
    # an A3M row without its '-' and with its lower case raised is the aligned stretch of its target
    seen = 0
    for e, (off, ln, nm, ni, nins) in enumerate(rows):
        if ln == 0:
            continue
        q, r = divmod(e, top)
        t, tb, te = int(c.hits[q, r, 0]), int(c.aln[q, r, 3]), int(c.aln[q, r, 5])
        row = bytes(a3m[off:off + ln].astype(np.uint8))
        assert row.replace(b"-", b"").upper() == bytes(c.packed[c.offs[t] + tb:c.offs[t] + te])
        assert len([x for x in row if not 97 <= x <= 122]) == int(c.qoffs[q + 1] - c.qoffs[q])
        seen += 1
    assert seen >= 3


def _call(swamd, c, **over):
    a = dict(queries=c.qpacked.ctypes.data, qoffs=c.qoffs.ctypes.data, nq=len(c.qoffs) - 1, db=c.packed.ctypes.data, offs=c.offs.ctypes.data,
             nt=len(c.offs) - 1, inc=0, hits=c.hits.ctypes.data, nhits=None, top=c.hits.shape[1], aln=c.aln.ctypes.data, ops=c.ops.ctypes.data, cap=c.cap,
             cols=c._cols.ctypes.data, rows=c._rows.ctypes.data, a3m=c._a3m.ctypes.data, a3m_cap=len(c._a3m), total=c._total.ctypes.data)
    a.update(over)
    return swamd.lib().sw_msa_from_hits_host(*a.values())


def test_einval(swamd):
    c = mc.synthetic(20, 3)
    nq, top = c.hits.shape[:2]
    c._cols = np.zeros(int(c.qoffs[-1]) * top, np.uint8)
    c._rows = np.zeros(nq * top, swamd.MSA_ROW)
    c._a3m = np.zeros(10000, np.uint8)
    c._total = np.zeros(1, np.int64)
    assert _call(swamd, c) == 0
    bad_q = c.qoffs.copy(); bad_q[2] = bad_q[1]                       # an empty query
    neg_q = c.qoffs - c.qoffs[0] - 1
    bad_t = c.offs.copy(); bad_t[2] = bad_t[1] - 1                    # offsets that decrease
    for over in (dict(qoffs=None), dict(db=None), dict(offs=None), dict(nq=-1), dict(nt=-1), dict(qoffs=bad_q.ctypes.data), dict(qoffs=neg_q.ctypes.data),
                 dict(offs=bad_t.ctypes.data), dict(top=0), dict(top=4097), dict(hits=None), dict(aln=None), dict(ops=None), dict(cap=0),
                 dict(cols=None, rows=None, a3m=None, total=None), dict(cols=None, rows=None, a3m=None), dict(rows=None), dict(rows=None, a3m=None),
                 dict(total=None), dict(a3m_cap=-1)):
        rc = _call(swamd, c, **over)
        assert rc != 0 and rc == _call(swamd, c, top=0), over
        assert swamd.lib().sw_last_error()
    assert _call(swamd, c, a3m=None, total=None) == 0                          # the rows alone
    assert _call(swamd, c, a3m=None) == 0 and _call(swamd, c, queries=None) == 0 and _call(swamd, c, a3m_cap=0) == 0


def test_write_a3m(swamd, tmp_path):
    c = mc.real(swamd, 20)
    cols, rows, a3m = swamd.msa_from_hits_host((c.qpacked, c.qoffs), (c.packed, c.offs), c.include_min, c.hits, c.nhits, c.aln, c.ops.reshape(3, 8, -1))
    ref = mc.reference(c)
    assert bytes(cols) == ref[0] and [tuple(int(x) for x in w) for w in rows.reshape(-1)] == ref[1] and bytes(a3m) == ref[2]
    names = [f"t{k}" for k in range(len(c.offs) - 1)]
    for q in range(3):
        qs = bytes(c.qpacked[c.qoffs[q]:c.qoffs[q + 1]])
        for query, tn in ((qs, names), (len(qs), None)):
            path = str(tmp_path / f"{q}.a3m")
            swamd.write_a3m(path, f"query{q}", query, tn, c.hits[q], c.aln[q], rows[q], a3m)
            lines = open(path, "rb").read().split(b"\n")
            assert lines[-1] == b""
            exp = [b">query%d" % q, qs] if tn else []
            for r in range(8):
                off, ln, nm, ni, nins = (int(x) for x in rows[q, r])
                if ln:
                    t = int(c.hits[q, r, 0])
                    al = c.aln[q, r]
                    exp.append(b">%s score=%d q=%d-%d t=%d-%d ident=%d/%d" % ((names[t] if tn else str(t)).encode(), al[1], al[2], al[4], al[3], al[5], ni, nm))
                    exp.append(bytes(a3m[off:off + ln]))
            assert lines[:-1] == exp and len(exp) >= 2
    with pytest.raises(swamd.SwError):
        swamd.write_a3m(str(tmp_path / "no" / "dir.a3m"), "q", 5, None, c.hits[0], c.aln[0], rows[0], a3m)
