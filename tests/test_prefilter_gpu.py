"""GPU: the ungapped pre-filter (sw_db_prefilter_ungapped, Database.prefilter_ungapped_device) against the independent checker of
tests/ungapped_cases.py, the host leg and the existing affine search with gap costs no gap can pay -- exact equality everywhere, on
32-bit lanes ("prefilter_lanes" = 32) and with the planner's choice (0: the packed kernel wherever a query's scores fit 16 bits);
"last_prefilter_packed_launches" says which ran.  The shapes and tables are those of tests/test_search_pairs_gpu.py."""
import numpy as np
import pytest

from affine_cases import PROTEIN
from buffer_cases import Arena, arena_bytes, assert_guards
from ungapped_cases import FRONT, QFRONT, mixed_case, mixed_checked, pack, passing, tables, ungapped_table

pytestmark = pytest.mark.gpu

EINVAL = -22
POISON64 = -0x5A5A5A5A5A5A5A5B
POISON32 = -0x5A5A5A5B
LANES = [0, 32]


def to_dev(engine, packed, skew):
    """The bytes on the device at an address with addr % 2 == skew % 2 (torch aligns allocations to 512 bytes)."""
    t = engine.torch
    buf = t.zeros(len(packed) + skew + 16, dtype=t.uint8, device=f"cuda:{engine.device}")
    buf[skew:skew + len(packed)] = t.from_numpy(packed.copy())
    d = buf[skew:skew + len(packed)]
    assert d.data_ptr() % 2 == skew % 2
    return d


def poisoned(engine, cap, nq, nt, want_scores=True):
    t = engine.torch
    dev = f"cuda:{engine.device}"
    return (t.full((cap, 2), POISON64, dtype=t.int64, device=dev), t.full((1,), POISON64, dtype=t.int64, device=dev),
            t.full((nq, nt), POISON32, dtype=t.int32, device=dev) if want_scores else None)


def run(engine, db, d_q, qoffs, sub, min_score, cap, lanes, want_scores=True):
    """One call into poisoned outputs under prefilter_lanes = lanes: numpy (pairs (cap, 2), npairs, scores or None) and what the options say."""
    nq = len(qoffs) - 1
    engine.set_option("prefilter_lanes", lanes)
    try:
        pairs, n, scores = db.prefilter_ungapped_device(d_q, qoffs, sub, min_score, cap, want_scores=want_scores, out=poisoned(engine, cap, nq, db.ntargets, want_scores))
        engine.synchronize()
        said = {k: engine.get_option("last_prefilter_" + k) for k in ("groups", "launches", "packed_launches")}
    finally:
        engine.set_option("prefilter_lanes", 0)
    return pairs.cpu().numpy(), int(n.item()), None if scores is None else scores.cpu().numpy(), said


def check_list(pairs, n, want_pairs, cap):
    """n is the true count; the first min(n, cap) rows are distinct passing pairs; the rest is {-1, -1}."""
    assert n == len(want_pairs)
    k = min(n, cap)
    got, want = {tuple(p) for p in pairs[:k].tolist()}, {tuple(p) for p in want_pairs.tolist()}
    assert len(got) == k and got <= want and (n > cap or got == want)
    assert (pairs[k:] == -1).all()


@pytest.fixture(scope="module")
def subs(swamd):
    return tables(swamd)


@pytest.fixture(scope="module")
def case(engine, swamd, subs):
    """The mixed case on the device (query base odd), its handle, the checker's tables (computed once per process, read-only) and the
    host leg's."""
    qlens, qpacked, qoffs, packed, offs = mixed_case()
    d_q, d_db = to_dev(engine, qpacked, 1), to_dev(engine, packed, 0)
    assert (d_q.data_ptr() + QFRONT) % 2 == 1
    db = engine.prepare_db(d_db, offs)
    want = {k: mixed_checked(k, s) for k, s in subs.items()}
    host = {k: swamd.prefilter_ungapped_host((qpacked, qoffs), (packed, offs), s, 1)[2] for k, s in subs.items()}
    db.search_affine_device(d_q, qoffs, (subs["random"], -11, -1))
    classes = engine.get_option("last_search_multi_launches")     # one launch per class of queries there: what this device's occupancy makes of QLENS
    yield {"qlens": qlens, "qpacked": qpacked, "qoffs": qoffs, "packed": packed, "offs": offs, "d_q": d_q, "d_db": d_db, "db": db, "want": want, "host": host,
           "classes": classes}
    db.close()


def median_score(want):
    nz = np.sort(want[want > 0])
    return int(nz[len(nz) // 2])


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("which", ["random", "match"])
def test_scores_equal_the_checker_the_host_leg_and_the_affine_search_without_gaps(engine, case, subs, which, lanes):
    pairs, n, scores, said = run(engine, case["db"], case["d_q"], case["qoffs"], subs[which], 1, 150, lanes)
    want = case["want"][which]
    assert scores.shape == (10, 15) and np.array_equal(scores, want), np.argwhere(scores != want)[:5]
    assert np.array_equal(scores, case["host"][which])
    assert (scores[:, np.diff(case["offs"]) == 0] == 0).all()                           # empty targets: zero over the poison
    # every query's scores fit 16 bits here (12 x 1100): the planner packs them all, "prefilter_lanes" = 32 none
    assert said["groups"] == 1 and case["classes"] <= said["launches"] <= 3
    assert said["packed_launches"] == (said["launches"] if lanes == 0 else 0)
    check_list(pairs, n, passing(want, case["offs"], 1), 150)
    # the second witness: with every score below 30000 E and F stay negative, so Gotoh's H is D
    assert want.max() < 30000
    h = case["db"].search_affine_device(case["d_q"], case["qoffs"], (subs[which], -30000, -1)).cpu().numpy()[:, :, 1]
    assert np.array_equal(scores, h)


@pytest.mark.parametrize("lanes", LANES)
def test_list_at_a_score_the_case_attains(engine, case, subs, lanes):
    want = case["want"]["random"]
    m = median_score(want)
    exp = passing(want, case["offs"], m)
    assert 0 < len(exp) < 130 and (want[exp[:, 0], exp[:, 1]] == m).any() and (want[want > 0] < m).any()
    pairs, n, scores, _ = run(engine, case["db"], case["d_q"], case["qoffs"], subs["random"], m, 150, lanes)
    check_list(pairs, n, exp, 150)
    assert {tuple(p) for p in pairs[:n].tolist()} == {tuple(p) for p in exp.tolist()} and np.array_equal(scores, want)


@pytest.mark.parametrize("lanes", LANES)
def test_list_too_small_no_list_and_scores_alone(engine, swamd, case, subs, lanes):
    """The guards around a list shorter than the count stay untouched (the list lies at an odd multiple of 8); cap 0 with and without a
    pointer; a call for the scores alone, with neither list nor count."""
    torch = engine.torch
    dev = f"cuda:{engine.device}"
    want = case["want"]["random"]
    m = median_score(want)
    exp = passing(want, case["offs"], m)
    sub = np.ascontiguousarray(subs["random"], np.int8)
    for cap in (len(exp) - 1, 5, 0):
        arena = Arena(torch, dev, arena_bytes(cap * 16, 8))
        c = arena.carve(cap * 16, 16, 8, name="pairs")
        cn = arena.carve(8, 8, 0, name="npairs")
        d_pairs, d_n = arena.view(c, torch.int64, (cap, 2)), arena.view(cn, torch.int64, (1,))
        engine.set_option("prefilter_lanes", lanes)
        try:
            case["db"].prefilter_ungapped_device(case["d_q"], case["qoffs"], subs["random"], m, cap, out=(d_pairs, d_n, None))   # cap 0: a NULL list
            engine.synchronize()
            assert int(d_n.item()) == len(exp)
            check_list(d_pairs.cpu().numpy(), int(d_n.item()), exp, cap)
            assert_guards(arena)
            if cap == 0:                                                                # cap 0 with a pointer: nothing is written through it
                d_n.fill_(POISON64)
                rc = swamd.lib().sw_db_prefilter_ungapped(engine._h, case["db"]._h, case["d_q"].data_ptr(), case["qoffs"].ctypes.data, 10, sub.ctypes.data, m,
                                                          arena.base + c.off, 0, d_n.data_ptr(), None, engine._stream())
                engine.synchronize()
                assert rc == 0 and int(d_n.item()) == len(exp)
                assert_guards(arena)
            # the scores alone: no list, no count
            arena2 = Arena(torch, dev, arena_bytes(150 * 4))
            cs = arena2.carve(150 * 4, 8, 4, name="scores")
            d_s = arena2.view(cs, torch.int32, (10, 15))
            rc = swamd.lib().sw_db_prefilter_ungapped(engine._h, case["db"]._h, case["d_q"].data_ptr(), case["qoffs"].ctypes.data, 10, sub.ctypes.data, m,
                                                      None, 0, None, d_s.data_ptr(), engine._stream())
            engine.synchronize()
            assert rc == 0 and np.array_equal(d_s.cpu().numpy(), want)
            assert_guards(arena2)
        finally:
            engine.set_option("prefilter_lanes", 0)


@pytest.fixture(scope="module")
def planted(subs):
    """Copies of query letters placed in targets so that the diagonal crosses a lane boundary, a strip boundary (columns 1023 .. 1025 of
    a 16-column query) and, for 2049, both strip boundaries: (qpacked, qoffs, packed, offs, [(query, target, columns)])."""
    rng = np.random.default_rng(40)
    qlens = [200, 400, 1100, 2049]
    qpacked, qoffs = pack(qlens, QFRONT, rng, PROTEIN[:20])
    q = [qpacked[qoffs[i]:qoffs[i + 1]] for i in range(4)]
    plan = [(0, 2, 40, 90, 17), (0, 160, 40, 41, 0), (1, 3, 40, 300, 255), (1, 250, 40, 64, 11),      # lane boundaries of 4 and 8 columns
            (2, 10, 40, 65, 20), (2, 1004, 40, 127, 63), (2, 1060, 40, 40, 0),                      # 16 columns; the strip boundary at 1024
            (3, 1004, 40, 300, 100), (3, 2020, 29, 63, 30), (3, 1000, 1049, 1100, 50)]              # 2049: one boundary, the other, both
    targets = []
    for qi, c0, n, tlen, at in plan:
        t = rng.choice(PROTEIN[:20], tlen).astype(np.uint8)
        t[at:at + n] = q[qi][c0:c0 + n]
        targets.append(t)
    offs = np.zeros(len(targets) + 1, np.int64)
    offs[0] = FRONT
    offs[1:] = FRONT + np.cumsum([len(t) for t in targets])
    packed = np.concatenate([rng.choice(PROTEIN[:20], FRONT).astype(np.uint8)] + targets)
    floor = [int(subs["random"][q[qi][c0:c0 + n], q[qi][c0:c0 + n]].astype(np.int64).sum()) for qi, c0, n, _, _ in plan]
    want = ungapped_table(qpacked, qoffs, packed, offs, subs["random"])
    return qpacked, qoffs, packed, offs, [(p[0], k, floor[k]) for k, p in enumerate(plan)], want


@pytest.mark.parametrize("lanes", LANES)
def test_planted_diagonals_across_lane_and_strip_boundaries(engine, subs, planted, lanes):
    qpacked, qoffs, packed, offs, plants, want = planted
    d_q, d_db = to_dev(engine, qpacked, 1), to_dev(engine, packed, 0)
    with engine.prepare_db(d_db, offs) as db:
        _, _, scores, said = run(engine, db, d_q, qoffs, subs["random"], 1, 0, lanes)
    assert said["packed_launches"] == (said["launches"] if lanes == 0 else 0)
    for qi, k, floor in plants:
        assert scores[qi, k] >= floor > 0 and scores[qi, k] == want[qi, k], (qi, k, scores[qi, k], want[qi, k], floor)
    assert np.array_equal(scores, want)


@pytest.mark.parametrize("qlen,longest,packed", [(258, 300, True), (259, 300, False), (400, 258, True), (400, 259, False)])
def test_packed_limit_from_both_sides(engine, qlen, longest, packed):
    """One-letter sequences under a table whose entry is 127: 127 x 258 = 32766 runs packed, 127 x 259 = 32893 on 32-bit lanes."""
    sub = np.full((256, 256), -1, np.int8)
    sub[65, 65] = 127
    tlens = [longest, 100, 1, longest - 1]
    qpacked, qoffs = np.full(qlen + 1, 65, np.uint8), np.array([1, qlen + 1], np.int64)
    offs = np.concatenate([[0], np.cumsum(tlens)]).astype(np.int64)
    packed_db = np.full(int(offs[-1]), 65, np.uint8)
    want = np.array([[127 * min(qlen, n) for n in tlens]])
    assert (want.max() <= 32767) == packed
    d_q, d_db = to_dev(engine, qpacked, 0), to_dev(engine, packed_db, 1)
    with engine.prepare_db(d_db, offs) as db:
        for lanes in LANES:
            pairs, n, scores, said = run(engine, db, d_q, qoffs, sub, int(want.max()), 4, lanes)
            assert np.array_equal(scores, want), (lanes, scores)
            assert said["launches"] == 1 and said["packed_launches"] == (1 if packed and lanes == 0 else 0)
            check_list(pairs, n, passing(want, offs, int(want.max())), 4)


@pytest.mark.parametrize("lanes", LANES)
def test_one_target_an_odd_number_and_none(engine, swamd, case, subs, lanes):
    qpacked, qoffs, packed, offs = case["qpacked"], case["qoffs"], case["packed"], case["offs"]
    assert (np.diff(offs) > 0).sum() == 13                                              # the mixed case itself: an odd last rank
    for o in ([int(offs[6]), int(offs[7])], [FRONT, FRONT + 5, FRONT + 5, FRONT + 70, FRONT + 71, FRONT + 400]):   # one target; three non-empty ones of five
        o = np.array(o, np.int64)
        want = swamd.prefilter_ungapped_host((qpacked, qoffs), (packed, o), subs["random"], 1)[2]
        with engine.prepare_db(case["d_db"], o) as db:
            pairs, n, scores, said = run(engine, db, case["d_q"], qoffs, subs["random"], 9, 20, lanes)
        assert np.array_equal(scores, want) and said["launches"] >= 2
        check_list(pairs, n, passing(want, o, 9), 20)
    for o in ([7], [5, 5, 5, 5]):                                                       # no target; only empty ones
        o = np.array(o, np.int64)
        with engine.prepare_db(case["d_db"], o) as db:
            pairs, n, scores, said = run(engine, db, case["d_q"], qoffs, subs["random"], 1, 6, lanes)
        assert n == 0 and (pairs == -1).all() and (scores == 0).all() and scores.shape == (10, len(o) - 1) and said["launches"] == 0
    pairs, n, scores, said = run(engine, case["db"], case["d_q"], np.array([4], np.int64), subs["random"], 1, 6, lanes)   # no query
    assert n == 0 and (pairs == -1).all() and said["launches"] == 0


@pytest.mark.parametrize("lanes", LANES)
def test_several_groups_give_the_same_bytes(engine, case, subs, lanes):
    """The ten profiles (2.3 MiB) under a budget of 1 MiB: the groups of sw_db_search_affine under the same budget, the scores and the
    list of the uncut call."""
    m = median_score(case["want"]["random"])
    whole = run(engine, case["db"], case["d_q"], case["qoffs"], subs["random"], m, 150, lanes)
    engine.set_option("search_profile_mib", 1)
    try:
        case["db"].search_affine_device(case["d_q"], case["qoffs"], (subs["random"], -11, -1))
        groups = engine.get_option("last_search_multi_groups")
        cut = run(engine, case["db"], case["d_q"], case["qoffs"], subs["random"], m, 150, lanes)
    finally:
        engine.set_option("search_profile_mib", 256)
    assert cut[3]["groups"] == groups >= 2 and cut[3]["launches"] >= groups > whole[3]["groups"] == 1
    assert cut[2].tobytes() == whole[2].tobytes() and cut[1] == whole[1]
    assert sorted(map(tuple, cut[0].tolist())) == sorted(map(tuple, whole[0].tolist()))


@pytest.mark.parametrize("lanes", LANES)
def test_chain_into_the_pair_list_search_without_reading_the_count(engine, case, subs, lanes):
    scoring = (subs["random"], -11, -1)
    m = median_score(case["want"]["random"])
    table = case["db"].search_affine_device(case["d_q"], case["qoffs"], scoring).cpu().numpy()
    engine.set_option("prefilter_lanes", lanes)
    try:
        d_pairs, d_n, _ = case["db"].prefilter_ungapped_device(case["d_q"], case["qoffs"], subs["random"], m, 150, out=poisoned(engine, 150, 10, 15, False))
        res = case["db"].search_affine_pairs_device(case["d_q"], case["qoffs"], scoring, d_pairs)      # all 150 entries; nothing came to the host
        engine.synchronize()
    finally:
        engine.set_option("prefilter_lanes", 0)
    pairs, n, res = d_pairs.cpu().numpy(), int(d_n.item()), res.cpu().numpy()
    check_list(pairs, n, passing(case["want"]["random"], case["offs"], m), 150)
    assert 0 < n < 150 and np.array_equal(res[:n], table[pairs[:n, 0], pairs[:n, 1]]) and (res[:n, 1] >= m).all()
    assert (res[n:] == 0).all()


def test_argument_errors_launch_nothing_and_leave_the_outputs_poisoned(engine, swamd, case, subs):
    L = swamd.lib()
    db, d_q, qoffs = case["db"], case["d_q"], case["qoffs"]
    d_pairs, d_n, d_s = poisoned(engine, 150, 10, 15)
    sub = np.ascontiguousarray(subs["random"], np.int8)
    big = np.zeros((256, 256), np.int8)
    big[65, 65] = 127

    def call(**kw):
        a = {"ctx": engine._h, "db": db._h, "queries": d_q.data_ptr(), "qoffs": qoffs, "nq": 10, "sub": sub.ctypes.data, "min": 5, "pairs": d_pairs.data_ptr(),
             "cap": 150, "n": d_n.data_ptr(), "scores": d_s.data_ptr(), **kw}
        qo = None if a["qoffs"] is None else np.ascontiguousarray(a["qoffs"], np.int64)
        rc = L.sw_db_prefilter_ungapped(a["ctx"], a["db"], a["queries"], None if qo is None else qo.ctypes.data, a["nq"], a["sub"], a["min"], a["pairs"], a["cap"],
                                        a["n"], a["scores"], engine._stream())
        engine.synchronize()
        return rc

    bad = [{"ctx": None}, {"db": None}, {"queries": None}, {"qoffs": None}, {"sub": None}, {"nq": -1},
           {"qoffs": [4, 4], "nq": 1}, {"qoffs": [4, 2], "nq": 1}, {"qoffs": [-1, 3], "nq": 1}, {"qoffs": [0, 1 << 20], "nq": 1},
           {"min": 0}, {"min": -1}, {"cap": -1}, {"pairs": None}, {"n": None}, {"n": None, "scores": None}, {"n": None, "pairs": None, "cap": 0, "scores": None}]
    assert call() == 0
    launches = engine.get_option("last_prefilter_launches")
    d_pairs.fill_(POISON64), d_n.fill_(POISON64), d_s.fill_(POISON32)
    for kw in bad:
        assert call(**kw) == EINVAL, kw
        assert bool((d_pairs == POISON64).all()) and bool((d_n == POISON64).all()) and bool((d_s == POISON32).all()), kw
    assert engine.get_option("last_prefilter_launches") == launches                     # an error leaves the report of the last good call
    for v in (1, 16, 64, -1):
        with pytest.raises(Exception):
            engine.set_option("prefilter_lanes", v)
    assert engine.get_option("prefilter_lanes") == 0
    assert call() == 0 and np.array_equal(d_s.cpu().numpy(), case["want"]["random"])     # the handle is as good as before
