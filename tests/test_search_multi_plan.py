"""CPU: the planner of the many-query search (swp::plan_search_multi, smith-waterman_amd/csrc/sw_plan.cpp), built with g++ and driven
through tests/search_multi_plan_driver.cpp: the class of every query, the groups a profile budget cuts, the launches and their work
items.  Occupancies are given, not measured: 3 workgroups per CU unless a case says otherwise."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = 257                      # profile rows (swk::SW_SEARCH_ROWS)
MIB = 1 << 20
MAX_ITEMS = (1 << 31) - 1


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the planner")
    exe = str(tmp_path_factory.mktemp("plan") / "search_multi_plan")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "search_multi_plan_driver.cpp"),
                    os.path.join(ROOT, "smith-waterman_amd", "csrc", "sw_plan.cpp")], check=True)

    def run(qlens, **kw):
        kw = {"longest": 400, "nonempty": 1000, **kw}
        line = "qlens=" + ",".join(str(q) for q in qlens) + " " + " ".join(f"{k}={v}" for k, v in kw.items())
        return json.loads(subprocess.run([exe], input=line + "\n", capture_output=True, text=True, check=True).stdout)
    return run


def by_row(p):
    """query -> (C of its launch, qpad, nstrips)"""
    out = {}
    for l in p["launches"]:
        for t in range(l["q0"], l["q0"] + l["nq"]):
            _, row, _, qpad, nstrips = p["table"][t]
            out[row] = (l["C"], qpad, nstrips)
    return out


def test_class_of_each_query(plan):
    qlens = [1, 256, 257, 512, 513, 1024, 1025, 2049]
    p = plan(qlens)
    assert by_row(p) == {0: (4, 256, 1), 1: (4, 256, 1), 2: (8, 512, 1), 3: (8, 512, 1), 4: (16, 1024, 1), 5: (16, 1024, 1), 6: (16, 2048, 2),
                         7: (16, 3072, 3)}
    assert len(p["groups"]) == 1 and [l["C"] for l in p["launches"]] == [4, 8, 16]           # at most three launches per group
    assert [l["kernel"] for l in p["launches"]] == [0, 1, 2]
    assert [(l["q0"], l["nq"]) for l in p["launches"]] == [(0, 2), (2, 2), (4, 4)]
    # the table: by class, input order within a class; the profiles back to back in table order
    assert [t[1] for t in p["table"]] == list(range(8))
    off = 0
    for prof_off, _, qlen, qpad, _ in p["table"]:
        assert prof_off == off and qpad >= qlen
        off += ROWS * qpad
    assert p["prof_need"] == off == p["groups"][0][2]


def test_table_is_sorted_by_class_with_input_order_kept(plan):
    p = plan([2049, 4, 300, 1, 600, 256, 512])
    assert [t[1] for t in p["table"]] == [1, 3, 5, 2, 6, 0, 4]
    assert [(l["C"], l["q0"], l["nq"]) for l in p["launches"]] == [(4, 0, 3), (8, 3, 2), (16, 5, 2)]


def test_sixteen_column_occupancy_fallback(plan):
    """Below two workgroups per CU at 16 columns per lane a long query runs at 8: twice the strips, the 8-column launch."""
    p = plan([512, 513, 2049], per_cu="5,4,1")
    assert by_row(p) == {0: (8, 512, 1), 1: (8, 1024, 2), 2: (8, 2560, 5)}
    assert [l["C"] for l in p["launches"]] == [8]
    assert by_row(plan([513], per_cu="5,4,2"))[0] == (16, 1024, 1)


def test_boundary_workspace_only_where_a_query_has_more_than_one_strip(plan):
    p = plan([100, 400, 1024, 1025], longest=1100, nonempty=50)
    l4, l8, l16 = p["launches"]
    assert l4["bnd_per"] == 0 and l8["bnd_per"] == 0
    assert l16["bnd_per"] == 2 * ((1100 + 160 + 3) // 4 * 4)           # H and F per row, sized by the longest target as for one query
    assert p["bnd_need"] == l16["grid"] * 4 * l16["bnd_per"]
    assert plan([100, 400, 1024], longest=1100)["bnd_need"] == 0


def test_groups_under_a_budget_of_one_mib_and_the_default(plan):
    one = ROWS * 512                                                       # 131 584 bytes: 7 fit 1 MiB, 8 do not
    p = plan([512] * 20, budget_bytes=MIB)
    assert p["groups"] == [[0, 7, 7 * one], [7, 7, 7 * one], [14, 6, 6 * one]]
    assert p["prof_need"] == 7 * one <= MIB
    assert [(l["group"], l["q0"], l["nq"]) for l in p["launches"]] == [(0, 0, 7), (1, 7, 7), (2, 14, 6)]
    assert [t[0] for t in p["table"][7:14]] == [k * one for k in range(7)]   # offsets start anew in every group
    p = plan([512] * 20)                                                   # default: 256 MiB
    assert p["groups"] == [[0, 20, 20 * one]]
    p = plan([512], repeat=2041)                                           # 2040 profiles of 131 584 bytes fit 256 MiB
    assert [g[1] for g in p["groups"]] == [2040, 1]


def test_an_over_budget_query_is_a_group_of_its_own(plan):
    p = plan([100, 5000, 100], budget_bytes=MIB)
    assert p["groups"] == [[0, 1, ROWS * 256], [1, 1, ROWS * 5120], [2, 1, ROWS * 256]]
    assert p["prof_need"] == ROWS * 5120 > MIB
    assert [(l["group"], l["C"]) for l in p["launches"]] == [(0, 4), (1, 16), (2, 4)]


def test_items_split_at_the_counter_width(plan):
    """Arithmetic on counts only: nothing is enumerated."""
    p = plan([8, 8, 8], nonempty=1 << 31)
    per = MAX_ITEMS // 3
    assert [(l["rank0"], l["nranks"]) for l in p["launches"]] == [(0, per), (per, per), (2 * per, per), (3 * per, (1 << 31) - 3 * per)]
    assert all(l["items"] == 3 * l["nranks"] <= MAX_ITEMS and l["nq"] == 3 for l in p["launches"])
    assert len(plan([8], nonempty=MAX_ITEMS)["launches"]) == 1
    assert [(l["rank0"], l["nranks"]) for l in plan([8], nonempty=MAX_ITEMS + 1)["launches"]] == [(0, MAX_ITEMS), (MAX_ITEMS, 1)]


def test_grid_never_above_items(plan):
    for qlens, nonempty, resident in [([8], 1, 1), ([8] * 3, 1, 1), ([8] * 300, 5, 375), ([512], 200000, 768), ([8, 300, 600], 2, 1)]:
        p = plan(qlens, nonempty=nonempty)
        for l in p["launches"]:
            assert l["items"] == l["nq"] * l["nranks"]
            assert l["grid"] == min(3 * 256, (l["items"] + 3) // 4) and 1 <= l["grid"] <= l["items"]   # workgroups of four waves
            assert 4 * l["grid"] < l["items"] + 4                                                  # no workgroup without an item
        assert p["launches"][0]["grid"] == resident
    assert plan([8], nonempty=0)["launches"] == []


@pytest.mark.parametrize("kw", [{}, {"max_items": 7}, {"budget_bytes": MIB}, {"max_items": 2, "budget_bytes": MIB, "per_cu": "5,4,1"}])
def test_every_pair_is_covered_exactly_once(plan, kw):
    qlens = [1, 4, 255, 256, 257, 512, 513, 1024, 1025, 2049, 8, 8, 8, 700, 300]
    p = plan(qlens, nonempty=13, cover=1, **kw)
    assert p["cover"] == [1, 1, 1]
    assert sorted(t[1] for t in p["table"]) == list(range(len(qlens)))
    assert all(l["items"] <= kw.get("max_items", MAX_ITEMS) for l in p["launches"])
