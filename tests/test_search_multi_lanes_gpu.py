"""GPU: the many-query search on packed 16-bit lanes ("search_lanes" = 16; smith-waterman_amd/csrc/sw_search_multi16.hip).  Every
comparison is bitwise and three-way: search_lanes = 16 against search_lanes = 32 on the same device buffers, and against the host leg
(sw_search_affine_multi_host / sw_search_pssm_multi_host); the scoring edges go against tests/affine_oracle.cpp as well.  Every call
writes into poisoned outputs, and after each call the route is asserted from "last_search_multi_packed_launches", so that no case
passes on a path it was not meant for.  The cases are tests/lanes_cases.py's."""
import numpy as np
import pytest

import affine_range_cases as arc
import buffer_cases as bc
import lanes_cases as lc
from affine_cases import PROTEIN, checker  # noqa: F401
from pssm_cases import Typed

pytestmark = pytest.mark.gpu

EINVAL = -22
POISON64 = -0x5A5A5A5A5A5A5A5B


def to_dev(engine, packed, skew):
    """The bytes on the device at an address with addr % 2 == skew % 2 (torch aligns allocations to 512 bytes)."""
    t = engine.torch
    buf = t.zeros(len(packed) + skew + 16, dtype=t.uint8, device=f"cuda:{engine.device}")
    buf[skew:skew + len(packed)] = t.from_numpy(np.array(packed))
    return buf[skew:skew + len(packed)]


def full(engine, n, value=POISON64):
    t = engine.torch
    return t.full((n,), value, dtype=t.int64, device=f"cuda:{engine.device}")


def differ(got, want):
    got, want = np.asarray(got).reshape(-1, 3), np.asarray(want).reshape(-1, 3)
    if got.shape != want.shape:
        return f"shape {got.shape} vs {want.shape}"
    bad = np.nonzero((got != want).any(axis=1))[0]
    return f"{len(bad)} entries differ, first {bad[0]}: {tuple(got[bad[0]])} vs {tuple(want[bad[0]])}" if len(bad) else ""


def under(engine, lanes, call):
    """call() under search_lanes = lanes: (what it returned, as numpy, {"launches", "packed", "groups"}); the option is 32 again afterwards."""
    engine.set_option("search_lanes", lanes)
    try:
        assert engine.get_option("search_lanes") == lanes
        out = call()
        engine.synchronize()
        said = {"launches": engine.get_option("last_search_multi_launches"), "packed": engine.get_option("last_search_multi_packed_launches"),
                "groups": engine.get_option("last_search_multi_groups")}
    finally:
        engine.set_option("search_lanes", 32)
    out = tuple(x.cpu().numpy() for x in out) if isinstance(out, tuple) else out.cpu().numpy()
    return out, said


class OnDevice:
    """A case of tests/lanes_cases.py on the device: queries at an odd base, the database and its handle."""

    def __init__(self, engine, case):
        self.case, self.engine = case, engine
        self.d_q, self.d_db = to_dev(engine, case["qpacked"], 1), to_dev(engine, case["packed"], 0)
        self.db = engine.prepare_db(self.d_db, case["offs"])
        self.nq, self.nt = len(case["qoffs"]) - 1, len(case["offs"]) - 1

    def close(self):
        self.db.close()

    def search(self, scoring, lanes):
        return under(self.engine, lanes, lambda: self.db.search_affine_device(self.d_q, self.case["qoffs"], scoring, out=full(self.engine, self.nq * self.nt * 3)))


def three_way(engine, swamd, case, scoring, what, dev=None):
    """The call under 32, under 16 and on the host, byte for byte: (the table, what the call under 16 said)."""
    d = dev or OnDevice(engine, case)
    try:
        r32, said32 = d.search(scoring, 32)
        r16, said16 = d.search(scoring, 16)
    finally:
        if dev is None:
            d.close()
    host = swamd.search_affine_multi_host((case["qpacked"], case["qoffs"]), (case["packed"], case["offs"]), scoring)
    assert said32["packed"] == 0, what
    assert r16.tobytes() == r32.tobytes(), f"{what}: 16 vs 32: " + differ(r16, r32) + " (entry = query * ntargets + target)"
    assert r16.tobytes() == host.tobytes(), f"{what}: 16 vs host: " + differ(r16, host)
    empty = np.diff(case["offs"]) == 0
    assert not r16[:, empty].any(), what                                                # {0, 0, 0} over the poison
    return r16, said16, said32


def checked(checker, case, sub, gaps):  # noqa: F811
    return np.stack([checker.search(q, case["packed"], case["offs"], sub, *gaps) for q in case["queries"]])


@pytest.fixture(scope="module")
def strips(engine):
    d = OnDevice(engine, lc.strips_case())
    assert (d.d_q.data_ptr() + lc.QFRONT) % 2 == 1 and (d.d_db.data_ptr() + lc.FRONT) % 2 == 1
    yield d
    d.close()


# ---- classes and strips ----

@pytest.mark.parametrize("gaps", lc.GAPS, ids=lambda g: f"{g[0]}_{g[1]}")
def test_classes_and_strips(engine, swamd, checker, strips, gaps):  # noqa: F811
    got, said16, said32 = three_way(engine, swamd, strips.case, (lc.table24(), *gaps), f"table24 {gaps}", strips)
    assert got.shape == (7, 11, 3)
    assert (said16["launches"], said16["packed"], said16["groups"]) == (3, 3, 1) and said32["launches"] == 3     # one launch per class, all packed
    if gaps == lc.GAPS[0]:
        want = checked(checker, strips.case, lc.table24(), gaps)
        assert not differ(got, want), differ(got, want)


# ---- partners that must not disturb each other ----

@pytest.mark.parametrize("name,case", lc.partner_cases(), ids=[n for n, _ in lc.partner_cases()])
def test_partners(engine, swamd, name, case):
    for gaps in ((-11, -1), (0, 0)):
        got, said16, _ = three_way(engine, swamd, case, (lc.table24(), *gaps), f"{name} {gaps}")
        assert said16["packed"] == said16["launches"] == 3                              # queries of 63, 300 and 1025 letters: three classes
        if name == "twins":
            assert np.array_equal(got[:, 0], got[:, 1])


@pytest.mark.parametrize("name,case", lc.corners_cases(), ids=[n for n, _ in lc.corners_cases()])
def test_one_half_at_the_floor_while_the_other_climbs(engine, swamd, checker, name, case):  # noqa: F811
    sub = arc.table("corners")
    for gaps in ((-11, -1), (0, 0), (-4, 0)):
        got, said16, _ = three_way(engine, swamd, case, (sub, *gaps), f"{name} {gaps}")
        assert said16["packed"] == said16["launches"] == 1
        want = checked(checker, case, sub, gaps)
        assert not differ(got, want), differ(got, want)
        climb = 1 if name.startswith("mismatch") else 0
        assert got[0, climb, 1] == 127 * 200 and got[0, 1 - climb, 1] == 0, got.tolist()


# ---- ties ----

@pytest.mark.parametrize("gaps", [(0, 0), (-1, 0)], ids=lambda g: f"{g[0]}_{g[1]}")
def test_ties_take_the_lowest_index_in_either_half(engine, swamd, checker, gaps):  # noqa: F811
    case, sub = lc.ties_case(), swamd.submat_match(1, -1)
    got, said16, _ = three_way(engine, swamd, case, (sub, *gaps), f"ties {gaps}")
    assert said16["packed"] == said16["launches"] == 2                                  # 257 and 1025 letters: two classes
    want = checked(checker, case, sub, gaps)
    assert not differ(got, want), differ(got, want)


# ---- the upper edge: scores up to 32767 ----

def test_upper_edge_31(engine, swamd, checker):  # noqa: F811
    case, sub = lc.upper_edge_case(), np.full((256, 256), 31, np.int8)
    got, said16, said32 = three_way(engine, swamd, case, (sub, -11, -1), "table 31")
    assert (said16["launches"], said16["packed"]) == (2, 1) and said32["launches"] == 1    # one class: 1057 packed, 1058 on 32-bit lanes in the same call
    assert got[0, :, 1].tolist() == [32767, 32767] and got[1, :, 1].tolist() == [31 * 1058, 31 * 1057]
    want = checked(checker, case, sub, (-11, -1))
    assert not differ(got, want), differ(got, want)


def test_upper_edge_ceiling(engine, swamd, checker):  # noqa: F811
    case, sub = lc.ceiling_edge_case(), arc.table("ceiling")
    got, said16, said32 = three_way(engine, swamd, case, (sub, -11, -1), "ceiling")
    assert (said16["launches"], said16["packed"]) == (2, 1) and said32["launches"] == 1
    assert got[0, :, 1].tolist() == [127 * 258, 127 * 258, 127 * 64]
    want = checked(checker, case, sub, (-11, -1))
    assert not differ(got, want), differ(got, want)


# ---- the lower edge: gap_open + 2 gap_extend = -32768 ----

@pytest.mark.parametrize("gaps", lc.PACKED_GAPS + lc.FALLBACK_GAPS, ids=lambda g: f"{g[0]}_{g[1]}")
def test_lower_edge(engine, swamd, strips, gaps):
    got, said16, said32 = three_way(engine, swamd, strips.case, (lc.table24(), *gaps), f"table24 {gaps}", strips)
    assert np.array_equal(got[:, :, 1], lc.strips_ungapped()), f"{gaps}: first (query, target) {np.argwhere(got[:, :, 1] != lc.strips_ungapped())[:3].tolist()}"
    assert said16["launches"] == said32["launches"] == 3
    assert said16["packed"] == (3 if gaps in lc.PACKED_GAPS else 0)
    assert (gaps[0] + 2 * gaps[1] >= -32768) == (gaps in lc.PACKED_GAPS)


# ---- eligible and other queries of one class in one call ----

def test_mixed_call_under_full8(engine, swamd, checker):  # noqa: F811
    qpacked, qoffs, _ = arc.cut_case("full8")                                           # 300, 257, 512, 258 letters: one class; 257 and 258 fit 16 bits
    s = arc.sequences("full8")
    case = {"queries": [qpacked[qoffs[k]:qoffs[k + 1]] for k in range(4)], "targets": s["targets"], "qpacked": qpacked, "qoffs": qoffs, "packed": s["packed"],
            "offs": s["offs"]}
    for gaps in ((-11, -1), (0, -3)):
        got, said16, said32 = three_way(engine, swamd, case, (arc.table("full8"), *gaps), f"full8 cut {gaps}")
        assert said32["launches"] == 1 and said16["packed"] == 1 and said16["launches"] == 2 > said32["launches"]
        want = checked(checker, case, arc.table("full8"), gaps)
        assert not differ(got, want), differ(got, want)


# ---- groups and chunks ----

def test_several_groups(engine, swamd, strips):
    before = engine.get_option("search_profile_mib")
    engine.set_option("search_profile_mib", 1)
    try:
        _, said16, said32 = three_way(engine, swamd, strips.case, (lc.table24(), -11, -1), "1 MiB of profiles", strips)
    finally:
        engine.set_option("search_profile_mib", before)
    assert said16["groups"] == said32["groups"] >= 3 and said16["packed"] == said16["launches"] == said32["launches"] >= 3


@pytest.mark.parametrize("min_score", [0, 40])
@pytest.mark.parametrize("top", [1, 10])
def test_top_hits_in_chunks(engine, swamd, top, min_score):
    case, scoring = lc.many_targets_case(), (lc.table24(), -11, -1)
    d = OnDevice(engine, case)
    before = engine.get_option("search_results_mib")
    engine.set_option("search_results_mib", 1)
    try:
        def call():
            return d.db.search_affine_top_device(d.d_q, case["qoffs"], scoring, top, min_score, out=(full(engine, d.nq * top * 3), full(engine, d.nq)))
        (h32, n32), said32 = under(engine, 32, call)
        chunks = engine.get_option("last_search_top_chunks")
        (h16, n16), said16 = under(engine, 16, call)
        assert engine.get_option("last_search_top_chunks") == chunks >= 2
    finally:
        engine.set_option("search_results_mib", before)
        d.close()
    hh, hn = swamd.search_affine_multi_top_host((case["qpacked"], case["qoffs"]), (case["packed"], case["offs"]), scoring, top, min_score)
    assert said32["packed"] == 0 and said16["packed"] > 0
    assert h16.tobytes() == h32.tobytes() and n16.tobytes() == n32.tobytes()
    assert h16.tobytes() == hh.tobytes() and n16.tobytes() == hn.tobytes()
    assert 0 < n16.max() <= top                                                        # something was selected


# ---- PSSM twins ----

def pssm_on_device(engine, matrix):
    t = engine.torch
    return t.from_numpy(np.ascontiguousarray(matrix, np.int8).reshape(-1).copy()).to(f"cuda:{engine.device}")


def test_pssm_twins_of_the_table_calls(engine, swamd, strips):
    case, gaps = strips.case, (-11, -1)
    m, moffs = swamd.pssm_from_queries((case["qpacked"], case["qoffs"]), lc.table24(), PROTEIN)
    scoring = (PROTEIN, lc.OTHER, 11, *gaps)
    d_m = pssm_on_device(engine, m)
    table16, _ = strips.search((lc.table24(), *gaps), 16)
    r32, said32 = under(engine, 32, lambda: strips.db.search_pssm_device(d_m, moffs, scoring, out=full(engine, 7 * 11 * 3)))
    r16, said16 = under(engine, 16, lambda: strips.db.search_pssm_device(d_m, moffs, scoring, out=full(engine, 7 * 11 * 3)))
    host = swamd.search_pssm_multi_host((m, moffs), (case["packed"], case["offs"]), scoring)
    assert said32["packed"] == 0 and (said16["launches"], said16["packed"]) == (3, 3)
    assert r16.tobytes() == r32.tobytes() == host.tobytes() == table16.tobytes(), differ(r16, table16)
    for top, min_score in ((1, 0), (10, 40)):
        def call_pssm():
            return strips.db.search_pssm_top_device(d_m, moffs, scoring, top, min_score, out=(full(engine, 7 * top * 3), full(engine, 7)))

        def call_table():
            return strips.db.search_affine_top_device(strips.d_q, case["qoffs"], (lc.table24(), *gaps), top, min_score, out=(full(engine, 7 * top * 3), full(engine, 7)))
        (h32, n32), s32 = under(engine, 32, call_pssm)
        (h16, n16), s16 = under(engine, 16, call_pssm)
        (ht, nt), st = under(engine, 16, call_table)
        assert s32["packed"] == 0 and s16["packed"] == 3 and st["packed"] == 3
        assert h16.tobytes() == h32.tobytes() == ht.tobytes() and n16.tobytes() == n32.tobytes() == nt.tobytes()


def test_pssm_eligibility_comes_from_smax(engine, swamd, checker, strips):  # noqa: F811
    case = strips.case
    rng = np.random.default_rng(2408)
    # entries up to 40 under smax = 11: they count as 11, and 11 x min(qlen, 1100) fits 16 bits for every query
    ty = Typed(rng, PROTEIN, -8, 11, lc.QLENS, lo=-8, hi=40, front=0)
    assert ty.types.max() > 11
    d_m = pssm_on_device(engine, ty.matrix)
    for gaps in ((-11, -1), (0, 0)):
        scoring = ty.scoring(*gaps)
        r32, said32 = under(engine, 32, lambda: strips.db.search_pssm_device(d_m, ty.qoffs, scoring, out=full(engine, 7 * 11 * 3)))
        r16, said16 = under(engine, 16, lambda: strips.db.search_pssm_device(d_m, ty.qoffs, scoring, out=full(engine, 7 * 11 * 3)))
        host = swamd.search_pssm_multi_host((ty.matrix, ty.qoffs), (case["packed"], case["offs"]), scoring)
        assert said32["packed"] == 0 and (said16["launches"], said16["packed"]) == (3, 3)
        assert r16.tobytes() == r32.tobytes() == host.tobytes(), differ(r16, r32) or differ(r16, host)
    want = ty.expected(checker, case["packed"], case["offs"], 0, 0)
    assert not differ(r16, want), differ(r16, want)
    # smax = 127 and a query of 300 columns against a longest target of 1100: 127 x 300 > 32767, the call runs on 32-bit lanes
    ty = Typed(rng, PROTEIN, -8, 127, [300], lo=-8, hi=12, front=0)
    d_m = pssm_on_device(engine, ty.matrix)
    scoring = ty.scoring(-11, -1)
    r32, said32 = under(engine, 32, lambda: strips.db.search_pssm_device(d_m, ty.qoffs, scoring, out=full(engine, 11 * 3)))
    r16, said16 = under(engine, 16, lambda: strips.db.search_pssm_device(d_m, ty.qoffs, scoring, out=full(engine, 11 * 3)))
    host = swamd.search_pssm_multi_host((ty.matrix, ty.qoffs), (case["packed"], case["offs"]), scoring)
    assert (said16["launches"], said16["packed"]) == (1, 0) and said32["packed"] == 0
    assert r16.tobytes() == r32.tobytes() == host.tobytes()


# ---- the buffer contract ----

def test_nothing_is_written_outside_the_results(engine, swamd):
    case, scoring = lc.strips_case(), (lc.table24(), -11, -1)
    t = engine.torch
    nq, nt = 7, 11
    arena = bc.Arena(t, f"cuda:{engine.device}", bc.arena_bytes(len(case["qpacked"]), len(case["packed"]), nq * nt * 24))
    d_q, _ = arena.place(case["qpacked"], align=2, skew=1, name="queries")              # odd bases: the letters start at even addresses ...
    d_db, _ = arena.place(case["packed"], align=2, skew=1, name="database")             # ... (QFRONT = 4 behind an odd base) and at odd ones (FRONT = 3)
    c_res = arena.carve(nq * nt * 24, align=8, name="results")
    res = arena.view(c_res, t.int64, (nq * nt * 3,))
    assert d_q.data_ptr() % 2 == 1 and d_db.data_ptr() % 2 == 1
    with engine.prepare_db(d_db, case["offs"]) as db:
        got, said = under(engine, 16, lambda: db.search_affine_device(d_q, case["qoffs"], scoring, out=res))
    assert said["packed"] == 3
    bc.assert_guards(arena)
    host = swamd.search_affine_multi_host((case["qpacked"], case["qoffs"]), (case["packed"], case["offs"]), scoring)
    assert got.tobytes() == host.tobytes(), differ(got, host)


# ---- the option ----

def test_option_values(engine, swamd, strips):
    assert engine.get_option("search_lanes") == 32                                      # the default
    for v in (0, 8, 64):
        with pytest.raises(swamd.SwError) as e:
            engine.set_option("search_lanes", v)
        assert e.value.code == EINVAL and "search_lanes must be" in str(e.value)
        assert engine.get_option("search_lanes") == 32
    engine.set_option("search_lanes", 16)
    try:
        assert engine.get_option("search_lanes") == 16
    finally:
        engine.set_option("search_lanes", 32)
    assert engine.get_option("search_lanes") == 32
    # the counter reads 0 after a call under 32 and after a call that launched nothing
    _, said = strips.search((lc.table24(), -11, -1), 16)
    assert said["packed"] == 3
    _, said = strips.search((lc.table24(), -11, -1), 32)
    assert said["packed"] == 0
    _, said = strips.search((lc.table24(), -11, -1), 16)
    assert said["packed"] == 3
    none = lc.case_of(strips.case["queries"][:2], [np.zeros(0, np.uint8)] * 3)
    d = OnDevice(engine, none)
    try:
        got, said = d.search((lc.table24(), -11, -1), 16)
    finally:
        d.close()
    assert said["packed"] == 0 and got.shape == (2, 3, 3) and not got.any()
