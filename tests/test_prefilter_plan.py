"""CPU: the planner of the ungapped pre-filter (swp::plan_prefilter, smith-waterman_amd/csrc/sw_plan.cpp), built with g++ and driven
through tests/prefilter_plan_driver.cpp: the groups and the table against plan_search_multi's, which kernel every query's items take
(the packed bound from both sides, "prefilter_lanes"), the pairing of the ranks, the grids, the boundary workspace and the cut of the
items -- by arithmetic, nothing is enumerated.  Occupancies are given, not measured: 3 workgroups per CU unless a case says otherwise."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = 257
MIB = 1 << 20
MIXED = [1, 4, 255, 256, 257, 512, 513, 1024, 1025, 2049]


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the planner")
    exe = str(tmp_path_factory.mktemp("plan") / "prefilter_plan")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "prefilter_plan_driver.cpp"),
                    os.path.join(ROOT, "smith-waterman_amd", "csrc", "sw_plan.cpp")], check=True)

    def run(qlens, **kw):
        kw = {"longest": 1100, "nonempty": 13, "max_entry": 11, **kw}
        line = "qlens=" + ",".join(str(q) for q in qlens) + " " + " ".join(f"{k}={v}" for k, v in kw.items())
        return json.loads(subprocess.run([exe], input=line + "\n", capture_output=True, text=True, check=True).stdout)
    return run


def covered(p, nonempty):
    """Every (table entry, rank) exactly once over the launches; returns {entry: packed?}."""
    seen, kind = {}, {}
    for l in p["launches"]:
        assert l["kernel"] == 2 * (l["C"] // 8) + l["packed"] and l["nranks"] >= 1 and l["grid"] >= 1
        assert l["items"] == l["nq"] * (-(-l["nranks"] // 2) if l["packed"] else l["nranks"])
        if l["packed"]:
            assert l["rank0"] % 2 == 0 and (l["nranks"] % 2 == 0 or l["rank0"] + l["nranks"] == nonempty)   # only the last rank runs alone
        for t in range(l["q0"], l["q0"] + l["nq"]):
            assert kind.setdefault(t, l["packed"]) == l["packed"]
            seen.setdefault(t, []).append((l["rank0"], l["nranks"]))
    for t, spans in seen.items():
        spans.sort()
        assert spans[0][0] == 0 and spans[-1][0] + spans[-1][1] == nonempty
        assert all(a[0] + a[1] == b[0] for a, b in zip(spans, spans[1:]))
    return kind


@pytest.mark.parametrize("qlens,kw", [
    (MIXED, {}),
    ([2049, 4, 300, 1, 600, 256, 512], {"max_entry": 100}),
    ([512] * 20, {"budget_bytes": MIB}),
    (MIXED + [8, 8, 8, 700, 300], {"budget_bytes": MIB, "per_cu": "5,5,4,4,1,1", "max_entry": 64}),
])
def test_groups_and_entries_are_those_of_the_many_query_search(plan, qlens, kw):
    p = plan(qlens, **kw)
    assert p["groups"] == p["multi_groups"] and p["prof_need"] == p["multi_prof_need"]
    assert sorted(p["table"]) == sorted(p["multi_table"])                                # every entry keeps its profile's place
    for q0, nq, _ in p["groups"]:
        mine, theirs = p["table"][q0:q0 + nq], p["multi_table"][q0:q0 + nq]
        assert sorted(mine) == sorted(theirs)
        assert [e[4] // e[5] // 64 for e in mine] == [e[4] // e[5] // 64 for e in theirs]    # class after class, as there
    kind = covered(p, 13)
    assert sorted(kind) == list(range(len(qlens)))
    longest, m = 1100, kw.get("max_entry", 11)
    for t, pk in kind.items():
        assert pk == (m * min(p["table"][t][3], longest) <= 32767)


def test_packed_bound_from_both_sides(plan):
    for qlen, longest, m, want in [(258, 5000, 127, 1), (259, 5000, 127, 0), (5000, 258, 127, 1), (5000, 259, 127, 0),
                                   (32767, 40000, 1, 1), (32768, 40000, 1, 0), (4681, 9000, 7, 1), (4682, 9000, 7, 0), (100000, 100000, 0, 1), (100000, 100000, -5, 1)]:
        assert m <= 0 or (m * min(qlen, longest) <= 32767) == bool(want)
        p = plan([qlen], longest=longest, nonempty=4, max_entry=m)
        assert [l["packed"] for l in p["launches"]] == [want] and p["packed_launches"] == want, (qlen, longest, m)
        assert p["launches"][0]["items"] == (2 if want else 4)
        p = plan([qlen], longest=longest, nonempty=4, max_entry=m, lanes=32)
        assert [l["packed"] for l in p["launches"]] == [0] and p["packed_launches"] == 0


def test_a_class_with_both_kinds_gets_a_launch_each(plan):
    p = plan([100, 300, 200, 250, 40], longest=1000, nonempty=7, max_entry=127)          # 127 x qlen <= 32767: qlen <= 258
    assert [(l["C"], l["packed"], l["q0"], l["nq"], l["items"]) for l in p["launches"]] == [(4, 1, 0, 4, 16), (8, 0, 4, 1, 7)]
    assert [e[2] for e in p["table"]] == [0, 2, 3, 4, 1]
    p = plan([259, 100, 300, 258, 400], longest=1000, nonempty=7, max_entry=127)         # the 8-column class: 258 packed, the others not
    assert [(l["C"], l["packed"], l["q0"], l["nq"]) for l in p["launches"]] == [(4, 1, 0, 1), (8, 1, 1, 1), (8, 0, 2, 3)]
    assert [e[2] for e in p["table"]] == [1, 3, 0, 2, 4] and p["packed_launches"] == 2
    covered(p, 7)


def test_odd_one_and_no_target(plan):
    p = plan([8, 300], nonempty=13)
    assert [(l["packed"], l["nranks"], l["items"]) for l in p["launches"]] == [(1, 13, 7), (1, 13, 7)]
    p = plan([8, 300], nonempty=1)
    assert [(l["packed"], l["rank0"], l["nranks"], l["items"], l["grid"]) for l in p["launches"]] == [(1, 0, 1, 1, 1)] * 2
    p = plan([8, 300], nonempty=0)
    assert p["launches"] == [] and len(p["table"]) == 2 and len(p["groups"]) == 1 and p["bnd_need"] == 0
    p = plan([8, 300], nonempty=13, lanes=32)
    assert [(l["packed"], l["items"]) for l in p["launches"]] == [(0, 13), (0, 13)]


def test_grids_and_boundary_workspace(plan):
    p = plan([100, 400, 1024, 1025], longest=1100, nonempty=5000, per_cu="6,5,5,4,3,2")
    l4, l8, l16 = p["launches"]
    assert (l4["grid"], l8["grid"], l16["grid"]) == (min(5 * 256, 625), min(4 * 256, 625), min(2 * 256, 1250))   # resident workgroups or a quarter of the items
    assert l4["bnd_per"] == 0 and l8["bnd_per"] == 0
    assert l16["bnd_per"] == 2 * ((1100 + 160 + 3) // 4 * 4)            # two columns of one int per row, sized by the longest target
    assert p["bnd_need"] == l16["grid"] * 4 * l16["bnd_per"]
    assert plan([100, 400, 1024], longest=1100, nonempty=50)["bnd_need"] == 0
    p = plan([100], nonempty=5, lanes=32)
    assert p["launches"][0]["grid"] == 2                                # five items: two workgroups of four waves


def test_several_groups_under_a_small_budget(plan):
    p = plan(MIXED, budget_bytes=MIB)
    assert len(p["groups"]) >= 3 and p["groups"] == p["multi_groups"]
    assert [l["group"] for l in p["launches"]] == sorted(l["group"] for l in p["launches"])
    for g, (q0, nq, _) in enumerate(p["groups"]):
        mine = [l for l in p["launches"] if l["group"] == g]
        assert mine and min(l["q0"] for l in mine) == q0 and max(l["q0"] + l["nq"] for l in mine) == q0 + nq
    assert sorted(covered(p, 13)) == list(range(10))
    assert p["prof_need"] == max(b for _, _, b in p["groups"])


def test_items_beyond_max_items_are_cut_by_arithmetic(plan):
    big = (1 << 31) - 1
    p = plan([300] * 64, nonempty=200_000_000)                          # 64 x 2 10^8 = 1.28 10^10 pairs, 6.4 10^9 packed items
    assert all(l["packed"] and l["items"] <= big for l in p["launches"]) and len(p["launches"]) == -(-100_000_000 // (big // 64))
    assert sum(l["items"] for l in p["launches"]) == 64 * 100_000_000
    covered(p, 200_000_000)
    p = plan([300] * 64, nonempty=200_000_001, lanes=32)
    assert all(l["items"] <= big for l in p["launches"]) and sum(l["items"] for l in p["launches"]) == 64 * 200_000_001
    covered(p, 200_000_001)
    for lanes, per in ((0, 6), (32, 3)):                                # max_items = 10, three queries: 3 rank pairs or 3 ranks a launch
        p = plan([8, 9, 10], nonempty=13, max_items=10, lanes=lanes)
        assert [l["nranks"] for l in p["launches"]] == [per] * (13 // per) + ([13 % per] if 13 % per else [])
        assert all(l["items"] <= 10 for l in p["launches"])
        covered(p, 13)
    p = plan([8] * 25, nonempty=3, max_items=10)                        # a class alone beyond the limit: cut by queries too
    assert sorted({(l["q0"], l["nq"]) for l in p["launches"]}) == [(0, 10), (10, 10), (20, 5)]
    covered(p, 3)
