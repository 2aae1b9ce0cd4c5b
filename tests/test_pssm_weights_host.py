"""CPU: the host leg of the hit weights (sw_pssm_hit_weights_host) against the restatement of its rule in Python integers
(tests/pssm_weights_cases.py), byte for byte: the synthetic tables of tests/pssm_hits_cases.py around every 64-op chunk edge, real
tables, garbage tables between guard words; the four properties the header derives from the rule, as exact equalities; per_hit 1 and
65535, the clamp at 65535 reached, a query without a used entry, bytes outside the letters, 1 to 256 letters; and every refusal."""
import ctypes

import numpy as np
import pytest

import pssm_hits_cases as hc
import pssm_weights_cases as cases

EINVAL = -22
A, C, G, T_, W, Y = (ord(x) for x in "ACGTWY")


def check(swamd, c, per_hit, inc):
    exp, A_r, used = cases.reference(c, per_hit, inc)
    w = cases.host_leg(swamd, c, per_hit, inc)
    assert (w == exp).all(), f"{(w != exp).sum()} weights differ, first at {np.argwhere(w != exp)[:1].tolist()}"
    assert not w[~used].any()
    return w, A_r, used


@pytest.mark.parametrize("top", [1, 3, 64])
@pytest.mark.parametrize("nletters", [1, 3, 24, 255, 256])
def test_synthetic_tables(swamd, nletters, top):
    rng = np.random.default_rng(100 * nletters + top)
    c = hc.synthetic(rng, nletters, top)
    assert len(hc.QLENS) == 6 and max(hc.QLENS) == 513 and max(hc.NOPS) == 300 and hc.QFRONT == 3
    for per_hit, inc in [(1, 0), (16, 0), (65535, 0), (100, 50)]:
        w, A_r, used = check(swamd, c, per_hit, inc)
        assert used.any() and w.any()
    if nletters >= 3 and top == 64:
        assert len(set(w[w > 0].tolist())) > 1                   # not every hit weighs the same: the rule is at work


def test_real_tables(swamd):
    rng = np.random.default_rng(11)
    c = hc.real(swamd, rng, top=8)
    w, A_r, used = check(swamd, c, 16, 1)
    for q in range(len(c.qoffs) - 1):
        U = int((w[q] > 0).sum())
        assert abs(int(w[q].sum()) - 16 * U) <= U                # the weights of a query sum to about per_hit x U (each is rounded once)
    # the Python wrapper: the outputs of align_pssm_hits_host go straight in
    ops = c.ops.reshape(len(c.qoffs) - 1, 8, -1)
    assert (swamd.pssm_hit_weights_host(c.qoffs, (c.packed, c.offs), hc.scoring(c), (16, 1), c.hits, c.nhits, c.aln, ops) == w).all()
    assert (swamd.pssm_hit_weights_host((c.prior, c.qoffs), (c.packed, c.offs), hc.scoring(c), (16, 1), c.hits, c.nhits, c.aln, ops) == w).all()


@pytest.mark.parametrize("nletters,top", [(24, 64), (256, 9)])
def test_garbage_tables_stay_defined_inside_the_buffers(swamd, nletters, top):
    rng = np.random.default_rng(3 * nletters + top)
    c = hc.garbage(rng, hc.synthetic(rng, nletters, top))
    w, A_r, used = check(swamd, c, 7, 0)
    assert used.any() and not used.all()
    nh = np.clip(c.nhits, 0, top)
    assert all(not w[q, nh[q]:].any() for q in range(len(nh)))   # at or beyond the clamped count: 0


@pytest.mark.parametrize("per_hit", [1, 16, 65535])
@pytest.mark.parametrize("U", [1, 2, 7, 64])
def test_identical_entries_get_exactly_per_hit(swamd, per_hit, U):
    seq = [A, C, G, T_, A, A, W][:5 + U % 3]
    c = cases.sequences_case([seq] * U)
    w = cases.host_leg(swamd, c, per_hit, 0)
    assert (w == per_hit).all()
    assert (cases.reference(c, per_hit, 0)[0] == w).all()


def test_permuting_the_entries_permutes_the_weights(swamd):
    rng = np.random.default_rng(77)
    c = hc.synthetic(rng, 24, 64)
    w = cases.host_leg(swamd, c, 16, 0)
    top = 64
    for q in range(len(c.qoffs) - 1):
        perm = rng.permutation(top)
        c.hits[q], c.aln[q] = c.hits[q, perm], c.aln[q, perm]
        c.ops[q * top:(q + 1) * top] = c.ops[q * top + perm]
        w[q] = w[q, perm]
    assert (cases.host_leg(swamd, c, 16, 0) == w).all()


@pytest.mark.parametrize("per_hit", [4, 16, 40000])
def test_two_copies_beside_one_that_differs_in_every_column(swamd, per_hit):
    c = cases.sequences_case([[A, C, G, T_, A], [A, C, G, T_, A], [C, G, T_, A, C]])
    w = cases.host_leg(swamd, c, per_hit, 0)
    assert w.tolist() == [[3 * per_hit // 4, 3 * per_hit // 4, 3 * per_hit // 2]] and 3 * per_hit % 4 == 0     # 0.75, 0.75, 1.5 x per_hit
    assert (cases.reference(c, per_hit, 0)[0] == w).all()


def test_a_query_depends_on_no_other_query(swamd):
    rng = np.random.default_rng(5)
    c = hc.synthetic(rng, 24, 64)
    w = cases.host_leg(swamd, c, 16, 0)
    top = 64
    for q in (1, 2):                                             # other tables for the queries 1 and 2: every entry one 'M' at (0, 0)
        c.aln[q, :, 2], c.aln[q, :, 3], c.aln[q, :, 6] = 0, 0, 1
        c.ops[q * top:(q + 1) * top, 0] = hc.M
    w2 = cases.host_leg(swamd, c, 16, 0)
    keep = [0, 3, 4, 5]
    assert (w2[keep] == w[keep]).all() and (w2[1] != w[1]).any() and (w2[2] != w[2]).any()


def test_the_clamp_at_65535_is_reached(swamd):
    """One distinct hit beside 4095 copies of another at per_hit 65535: the share of the distinct one is about 2^27."""
    c = cases.sequences_case([[C, G, T_]] + [[A, C, G]] * 4095)
    w, A_r, _ = check(swamd, c, 65535, 0)
    S, U = sum(A_r[0]), 4096
    assert (2 * 65535 * U * A_r[0, 0] + S) // (2 * S) > 65535 and w[0, 0] == 65535            # reached, and clamped
    assert (w[0, 1:] == w[0, 1]).all() and 0 < w[0, 1] < 65535


def test_a_query_without_a_used_entry_gets_zeros(swamd):
    """The second query's entries all lie below include_min_score; so do all entries past nhits."""
    c = cases.sequences_case([[A, C, G]] * 3, other_queries=[(4, [[A, C, G, T_]] * 2)])
    c.aln[1, :, 1] = 10                                                                       # below include_min = 20
    w, _, used = check(swamd, c, 16, 20)
    assert used[0].all() and not used[1].any() and not w[1].any() and (w[0] == 16).all()
    c.nhits[:] = 0
    assert not check(swamd, c, 16, 0)[0].any()


def test_bytes_outside_the_letters_count_nothing(swamd):
    """'W' and 'Y' are no letters here: the pairs with them are not counted, and a hit made of them alone has m_r = 0 and weight 0."""
    letters = np.array([A, C, G, T_], np.uint8)
    c = cases.sequences_case([[A, C, W, G], [A, C, Y, G], [W, Y, W, Y]], letters=letters)
    w, A_r, used = check(swamd, c, 16, 0)
    assert used.all() and A_r[0, 2] == 0 and w.tolist() == [[16, 16, 0]]
    wide = cases.sequences_case([[A, C, W, G], [A, C, Y, G], [W, Y, W, Y]], letters=np.array([A, C, G, T_, W, Y], np.uint8))
    assert (check(swamd, wide, 16, 0)[0] > 0).all()


def test_refusals(swamd):
    rng = np.random.default_rng(5)
    c = hc.synthetic(rng, 4, 3)
    L = swamd.lib()
    lt, sc = swamd._pssm_scoring(hc.scoring(c))
    wt = swamd._pssm_weighting((16, 0))
    nq, top = len(c.qoffs) - 1, 3
    out = np.full(nq * top, cases.POISON32, np.int32)
    hits, aln, ops = np.ascontiguousarray(c.hits), np.ascontiguousarray(c.aln), np.ascontiguousarray(c.ops)

    def args():
        return [c.qoffs.ctypes.data, nq, c.packed.ctypes.data, c.offs.ctypes.data, len(c.offs) - 1, ctypes.byref(sc), ctypes.byref(wt), hits.ctypes.data, None, top,
                aln.ctypes.data, ops.ctypes.data, c.cap, out.ctypes.data]

    assert L.sw_pssm_hit_weights_host(*args()) == 0 and (out != cases.POISON32).all()
    out[:] = cases.POISON32
    for null in (0, 2, 3, 5, 6, 7, 10, 11, 13):                   # qoffsets, db, offsets, scoring, weighting, hits, aln, ops, weights
        a = args()
        a[null] = None
        assert L.sw_pssm_hit_weights_host(*a) == EINVAL, null
    for at, bad in [(9, 0), (9, 4097), (9, -1), (12, 0), (12, -1), (1, -1), (4, -1)]:          # top, ops_cap, nqueries, ntargets
        a = args()
        a[at] = bad
        assert L.sw_pssm_hit_weights_host(*a) == EINVAL, (at, bad)
    for per_hit in (0, -1, 65536, 2**31 - 1):
        wt.per_hit = per_hit
        assert L.sw_pssm_hit_weights_host(*args()) == EINVAL, per_hit
        assert b"per_hit" in L.sw_last_error()
    wt.per_hit = 16
    for bad in ((np.frombuffer(b"ACCA", np.uint8), -4, 11, -10, -1), (c.letters, -4, 128, -10, -1), (c.letters, -4, 11, 1, -1), (c.letters[:0], -4, 11, -10, -1)):
        keep, sc2 = swamd._pssm_scoring(bad)
        a = args()
        a[5] = ctypes.byref(sc2)
        assert L.sw_pssm_hit_weights_host(*a) == EINVAL, bad
    qo = c.qoffs.copy()
    qo[2] = qo[1]                                                                              # an empty query
    a = args()
    a[0] = qo.ctypes.data
    assert L.sw_pssm_hit_weights_host(*a) == EINVAL
    assert (out == cases.POISON32).all()                                                       # refused before the first weight was written
    # no query: nothing is written; no target: every weight is 0
    a = args()
    a[1] = 0
    assert L.sw_pssm_hit_weights_host(*a) == 0 and (out == cases.POISON32).all()
    a = args()
    a[4] = 0
    assert L.sw_pssm_hit_weights_host(*a) == 0 and not out.any()
    with pytest.raises(swamd.SwError):
        swamd.pssm_hit_weights_host(c.qoffs, (c.packed, c.offs), hc.scoring(c), (0, 0), c.hits, None, c.aln, c.ops.reshape(nq, top, -1))
