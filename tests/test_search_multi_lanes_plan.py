"""CPU: the planner of the many-query search with a choice of lanes (swp::plan_search_multi_lanes, smith-waterman_amd/csrc/sw_plan.cpp),
built with g++ and driven through tests/search_multi_lanes_plan_driver.cpp: under lanes = 32 the launches of plan_search_multi field
for field; under 16 which queries run packed (both bounds from both sides), the order inside a class, the pairing of the ranks, the
cover of every (query, target rank) pair, the boundary workspace and the count of packed launches.  Occupancies are given, not
measured: 3 workgroups per CU for all six kernels unless a case says otherwise."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIB = 1 << 20
MAX_ITEMS = (1 << 31) - 1
MIXED = [1, 4, 255, 256, 257, 512, 513, 1024, 1025, 2049, 8, 8, 8, 700, 300]

# the cases of tests/test_search_multi_plan.py
MULTI_CASES = [
    ([1, 256, 257, 512, 513, 1024, 1025, 2049], {}),
    ([2049, 4, 300, 1, 600, 256, 512], {}),
    ([512, 513, 2049], {"per_cu": "5,4,1"}),
    ([513], {"per_cu": "5,4,2"}),
    ([100, 400, 1024, 1025], {"longest": 1100, "nonempty": 50}),
    ([100, 400, 1024], {"longest": 1100}),
    ([512] * 20, {"budget_bytes": MIB}),
    ([512] * 20, {}),
    ([100, 5000, 100], {"budget_bytes": MIB}),
    ([8, 8, 8], {"nonempty": 1 << 31}),
    ([8], {"nonempty": MAX_ITEMS}),
    ([8], {"nonempty": MAX_ITEMS + 1}),
    ([8], {"nonempty": 1}),
    ([8] * 3, {"nonempty": 1}),
    ([8] * 300, {"nonempty": 5}),
    ([512], {"nonempty": 200000}),
    ([8, 300, 600], {"nonempty": 2}),
    ([8], {"nonempty": 0}),
    (MIXED, {"nonempty": 13}),
    (MIXED, {"nonempty": 13, "max_items": 7}),
    (MIXED, {"nonempty": 13, "budget_bytes": MIB}),
    (MIXED, {"nonempty": 13, "max_items": 2, "budget_bytes": MIB, "per_cu": "5,4,1"}),
]


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the planner")
    exe = str(tmp_path_factory.mktemp("plan") / "search_multi_lanes_plan")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "search_multi_lanes_plan_driver.cpp"),
                    os.path.join(ROOT, "smith-waterman_amd", "csrc", "sw_plan.cpp")], check=True)

    def run(qlens, **kw):
        kw = {"longest": 400, "nonempty": 1000, "max_entry": 11, "gap_open": -11, "gap_extend": -1, "lanes": 16, **kw}
        line = "qlens=" + ",".join(str(q) for q in qlens) + " " + " ".join(f"{k}={v}" for k, v in kw.items())
        return json.loads(subprocess.run([exe], input=line + "\n", capture_output=True, text=True, check=True).stdout)
    return run


def check_launches(p, nonempty):
    """The shape of every launch; returns {entry: packed?}."""
    kind = {}
    for l in p["launches"]:
        assert l["kernel"] == l["C"] // 8 and l["nranks"] >= 1 and l["grid"] >= 1
        assert l["items"] == l["nq"] * (-(-l["nranks"] // 2) if l["packed"] else l["nranks"])
        if l["packed"]:
            assert l["rank0"] % 2 == 0 and (l["nranks"] % 2 == 0 or l["rank0"] + l["nranks"] == nonempty)   # only the last rank runs alone
        for t in range(l["q0"], l["q0"] + l["nq"]):
            assert kind.setdefault(t, l["packed"]) == l["packed"]
    return kind


@pytest.mark.parametrize("qlens,kw", MULTI_CASES)
def test_lanes_32_gives_the_launches_of_plan_search_multi(plan, qlens, kw):
    for extra in ({}, {"max_entry": 127, "gap_open": -40000}, {"packed_per_cu": "1,0,0"}):
        p = plan(qlens, lanes=32, **kw, **extra)
        assert p["launches"] == p["multi_launches"]                       # field for field, in order
        assert p["table"] == p["multi_table"] and p["groups"] == p["multi_groups"]
        assert p["prof_need"] == p["multi_prof_need"] and p["bnd_need"] == p["multi_bnd_need"] and p["packed_launches"] == 0


def test_score_bound_from_both_sides(plan):
    for qlen, longest, m, want in [(1057, 1100, 31, 1), (1058, 1100, 31, 0), (258, 1100, 127, 1), (259, 1100, 127, 0), (100000, 1100, -5, 1),
                                   (100000, 100000, -5, 1), (100000, 10, 127, 1), (5000, 258, 127, 1), (5000, 259, 127, 0), (100000, 100000, 0, 1)]:
        assert m <= 0 or (m * min(qlen, longest) <= 32767) == bool(want)
        p = plan([qlen], longest=longest, nonempty=4, max_entry=m)
        assert [l["packed"] for l in p["launches"]] == [want] and p["packed_launches"] == want, (qlen, longest, m)
        assert p["launches"][0]["items"] == (2 if want else 4)
        p = plan([qlen], longest=longest, nonempty=4, max_entry=m, lanes=32)
        assert [l["packed"] for l in p["launches"]] == [0] and p["packed_launches"] == 0


def test_gap_bound_from_both_sides(plan):
    """gap_open + 2 gap_extend >= -32768, call-wide: one step below it nothing is packed."""
    for go, ge, want in [(-32766, -1, 1), (-32767, -1, 0), (0, -16384, 1), (0, -16385, 0), (-32768, 0, 1), (-32769, 0, 0), (-11, -1, 1), (0, 0, 1),
                         (-(1 << 24) + 1, -1, 0)]:
        assert (go + 2 * ge >= -32768) == bool(want)
        p = plan([8, 300, 600], nonempty=5, gap_open=go, gap_extend=ge)
        assert [l["packed"] for l in p["launches"]] == [want] * 3 and p["packed_launches"] == 3 * want, (go, ge)
    p = plan([8, 300, 600], nonempty=5, gap_open=-32769, gap_extend=0)
    assert p["launches"] == p["multi_launches"]


def test_packed_entries_come_first_and_keep_their_profiles(plan):
    p = plan([100, 300, 200, 250, 40], longest=1000, nonempty=7, max_entry=127)          # 127 x qlen <= 32767: qlen <= 258
    assert [(l["C"], l["packed"], l["q0"], l["nq"], l["items"]) for l in p["launches"]] == [(4, 1, 0, 4, 16), (8, 0, 4, 1, 7)]
    assert [e[2] for e in p["table"]] == [0, 2, 3, 4, 1]
    p = plan([259, 100, 300, 258, 400], longest=1000, nonempty=7, max_entry=127)         # the 8-column class: 258 packed, the others not
    assert [(l["C"], l["packed"], l["q0"], l["nq"]) for l in p["launches"]] == [(4, 1, 0, 1), (8, 1, 1, 1), (8, 0, 2, 3)]
    assert [e[2] for e in p["table"]] == [1, 3, 0, 2, 4] and p["packed_launches"] == 2   # input order within either part
    assert sorted(p["table"]) == sorted(p["multi_table"])                                # every entry keeps its profile's place
    # the same under a budget that cuts groups, with a table whose maximum splits every class
    qlens = [400, 100, 300, 64, 1025, 258, 2049, 259, 20, 513, 1024]
    p = plan(qlens, longest=1100, nonempty=9, max_entry=127, budget_bytes=MIB, cover=1)
    assert len(p["groups"]) >= 2 and p["groups"] == p["multi_groups"] and p["cover"] == [1, 1, 1]
    assert sorted(p["table"]) == sorted(p["multi_table"])
    kind = check_launches(p, 9)
    for q0, nq, _ in p["groups"]:
        mine, theirs = p["table"][q0:q0 + nq], p["multi_table"][q0:q0 + nq]
        assert sorted(mine) == sorted(theirs)
        assert [e[4] // e[5] // 64 for e in mine] == [e[4] // e[5] // 64 for e in theirs]    # class after class, as there
        for C in (4, 8, 16):
            cls = [t for t in range(q0, q0 + nq) if p["table"][t][4] // p["table"][t][5] // 64 == C]
            flags = [kind[t] for t in cls]
            assert flags == sorted(flags, reverse=True)                                  # packed first
            for part in (1, 0):
                rows = [p["table"][t][2] for t in cls if kind[t] == part]
                assert rows == sorted(rows)                                              # input order within either part
    for t, pk in kind.items():
        assert pk == (127 * min(p["table"][t][3], 1100) <= 32767)


@pytest.mark.parametrize("nonempty", [1, 2, 12, 13])
@pytest.mark.parametrize("kw", [{}, {"max_items": 7}, {"budget_bytes": MIB}, {"max_items": 2, "budget_bytes": MIB, "per_cu": "5,4,1"},
                                {"max_entry": 127, "max_items": 5}, {"max_entry": 127, "budget_bytes": MIB}])
def test_every_pair_is_covered_exactly_once(plan, kw, nonempty):
    p = plan(MIXED, longest=1100, nonempty=nonempty, cover=1, **kw)
    assert p["cover"] == [1, 1, 1]
    kind = check_launches(p, nonempty)
    assert sorted(kind) == list(range(len(MIXED)))
    assert all(l["items"] <= kw.get("max_items", MAX_ITEMS) for l in p["launches"])
    assert p["packed_launches"] == sum(l["packed"] for l in p["launches"]) > 0
    if kw.get("max_entry", 11) == 11:
        assert all(l["packed"] for l in p["launches"])
    else:
        assert {l["packed"] for l in p["launches"]} == {0, 1}
    # a class cut into several launches: every packed launch starts at an even rank and only the last holds an odd one
    if "max_items" in kw and nonempty > 2:
        assert max(sum(1 for l in p["launches"] if (l["q0"], l["packed"]) == key) for key in {(l["q0"], l["packed"]) for l in p["launches"]}) > 1


def test_boundary_workspace_is_that_of_the_32_bit_launch(plan):
    qlens = [100, 400, 1024, 1025, 2049]
    p16 = plan(qlens, longest=1100, nonempty=50)
    p32 = plan(qlens, longest=1100, nonempty=50, lanes=32)
    assert [l["packed"] for l in p16["launches"]] == [1, 1, 1]
    assert [(l["q0"], l["nq"], l["bnd_per"]) for l in p16["launches"]] == [(l["q0"], l["nq"], l["bnd_per"]) for l in p32["launches"]]
    assert p16["launches"][2]["bnd_per"] == 2 * ((1100 + 160 + 3) // 4 * 4) and p16["launches"][0]["bnd_per"] == 0
    assert p16["bnd_need"] == p16["launches"][2]["grid"] * 4 * p16["launches"][2]["bnd_per"] <= p32["bnd_need"]
    # a class split by eligibility: either part is sized by its own queries' strips, as a 32-bit launch of those queries would be
    p = plan([1025, 2049, 520], longest=1100, nonempty=50, max_entry=31)                 # 31 x min(qlen, 1100) <= 32767: qlen <= 1057
    assert [(l["C"], l["packed"], l["nq"]) for l in p["launches"]] == [(16, 1, 2), (16, 0, 1)]
    alone = plan([1025, 520], longest=1100, nonempty=50, lanes=32)
    assert p["launches"][0]["bnd_per"] == alone["launches"][0]["bnd_per"] > 0
    assert p["launches"][1]["bnd_per"] == plan([2049], longest=1100, nonempty=50, lanes=32)["launches"][0]["bnd_per"]


def test_grids_and_occupancy(plan):
    p = plan([100, 400, 1024], longest=1100, nonempty=5000, per_cu="6,5,3", packed_per_cu="4,4,2")
    assert [l["packed"] for l in p["launches"]] == [1, 1, 1]
    assert [l["grid"] for l in p["launches"]] == [min(4 * 256, 625), min(4 * 256, 625), min(2 * 256, 625)]   # resident workgroups or a quarter of the items
    # a packed kernel that does not fit keeps its class on 32-bit lanes: 16 columns per lane need two workgroups per CU, as the 32-bit kernel
    p = plan([100, 400, 1024], longest=1100, nonempty=5000, per_cu="6,5,3", packed_per_cu="4,0,1")
    assert [(l["C"], l["packed"]) for l in p["launches"]] == [(4, 1), (8, 0), (16, 0)] and p["packed_launches"] == 1
    assert [l["grid"] for l in p["launches"]] == [625, 1250, 3 * 256]
    # the classes are those of the 32-bit occupancy, whatever the packed kernels'
    assert plan([513], per_cu="5,4,1", packed_per_cu="4,4,2")["launches"][0]["C"] == 8
    p = plan([8, 300], nonempty=1)
    assert [(l["packed"], l["rank0"], l["nranks"], l["items"], l["grid"]) for l in p["launches"]] == [(1, 0, 1, 1, 1)] * 2
    p = plan([8, 300], nonempty=0)
    assert p["launches"] == [] and p["packed_launches"] == 0 and len(p["table"]) == 2


def test_items_beyond_max_items_are_cut_by_arithmetic(plan):
    p = plan([300] * 64, nonempty=200_000_000)                          # 6.4 10^9 packed items
    assert all(l["packed"] and l["items"] <= MAX_ITEMS for l in p["launches"]) and len(p["launches"]) == -(-100_000_000 // (MAX_ITEMS // 64))
    assert sum(l["items"] for l in p["launches"]) == 64 * 100_000_000
    check_launches(p, 200_000_000)
    assert p["packed_launches"] == len(p["launches"])
    p = plan([8, 9, 10], nonempty=13, max_items=10)                     # three queries: 3 rank pairs a launch
    assert [(l["rank0"], l["nranks"]) for l in p["launches"]] == [(0, 6), (6, 6), (12, 1)]
