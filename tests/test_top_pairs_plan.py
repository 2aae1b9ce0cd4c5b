"""CPU: the planner of the selection from a pair list (swp::plan_top_pairs, smith-waterman_amd/csrc/sw_plan.cpp), built with g++ and
driven through tests/top_pairs_plan_driver.cpp: the key's target bits, where the LDS-aggregated count and scatter end, the items the sort
keeps between rounds, the workspace sizes, the grids and what is refused."""
import json
import math
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIB = 1 << 20


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the planner")
    exe = str(tmp_path_factory.mktemp("plan") / "top_pairs_plan")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "top_pairs_plan_driver.cpp"),
                    os.path.join(ROOT, "smith-waterman_amd", "csrc", "sw_plan.cpp")], check=True)

    def run(**kw):
        kw = {"npairs": 1000, "nqueries": 4, "ntargets": 1000, "top": 10, **kw}
        line = " ".join(f"{k}={v}" for k, v in kw.items())
        return json.loads(subprocess.run([exe], input=line + "\n", capture_output=True, text=True, check=True).stdout)
    return run


@pytest.mark.parametrize("nt", [1, 2, 3, 4, 5, 64, 65, 4096, 4097, 1 << 20, (1 << 20) + 1, 1 << 30, (1 << 30) + 1, (1 << 31) - 1])
def test_target_bits(plan, nt):
    p = plan(ntargets=nt)
    tbits = math.ceil(math.log2(nt)) if nt > 1 else 0
    assert p["refused"] is None and p["tbits"] == tbits
    assert (1 << tbits) >= nt and (tbits == 0 or (1 << (tbits - 1)) < nt)    # the smallest field that holds every target
    assert 24 + tbits < 63                                                   # bit 63 stays free for the mark of a real item
    assert plan(ntargets=0)["tbits"] == 0


def test_where_the_lds_form_ends(plan):
    edge = plan()["lds_queries"]
    assert edge * 4 <= 64 * 1024                                             # its counters fit the LDS a workgroup may always take
    assert plan(nqueries=1)["lds"] == 1 and plan(nqueries=edge)["lds"] == 1
    assert plan(nqueries=edge + 1)["lds"] == 0 and plan(nqueries=10**6)["lds"] == 0
    assert plan(nqueries=0)["lds"] == 1


@pytest.mark.parametrize("top,T", [(1, 1), (2, 2), (3, 4), (4, 4), (5, 8), (64, 64), (65, 128), (2048, 2048), (2049, 4096), (4096, 4096)])
def test_items_kept_between_rounds(plan, top, T):
    p = plan(top=top, npairs=100000)
    assert p["T"] == T and p["kernel"] == 1
    assert p["items"] == max(p["top_max"], 2 * T)                            # a round takes in at least as many new items as it keeps
    assert p["items"] - T >= T and p["items"] * 12 <= 160 * 1024             # ... and the items fit the LDS of a CU
    assert p["sort_kernel"] == (2 if p["items"] > p["top_max"] else 1)


def test_whole_sort_up_to_top_max_entries(plan):
    m = plan()["top_max"]
    for n in (0, 1, m - 1, m):
        p = plan(npairs=n, top=4096)
        assert p["kernel"] == 0 and p["sort_kernel"] == 0 and p["items"] == m  # every segment fits, whatever top
    p = plan(npairs=m + 1, top=4096)
    assert p["kernel"] == 1 and p["items"] == 2 * m
    assert plan(npairs=m + 1, top=2048)["items"] == m


@pytest.mark.parametrize("npairs,nq", [(0, 5), (1, 1), (1000, 64), (132253, 64), (10**6, 3), (12_800_000, 64), ((1 << 31) - 1, 100000), (1000, 0)])
def test_workspace_bytes(plan, npairs, nq):
    p = plan(npairs=npairs, nqueries=nq)
    assert p["keys_need"] == npairs and p["pos_need"] == npairs             # 8 + 4 bytes per entry
    assert p["segment_bytes"] == 12 * npairs <= 16 * npairs
    assert p["seg_need"] == 2 * (nq + 1)                                     # count / cursor and offset per query, one more offset
    assert p["entry_bytes"] == 56 and 40 * npairs + p["segment_bytes"] <= 56 * npairs


def test_cap_of_the_chained_call(plan):
    assert plan(budget_bytes=MIB)["prefiltered_cap"] == MIB // 56 == 18724
    assert plan(budget_bytes=1024 * MIB)["prefiltered_cap"] == (1 << 30) // 56


@pytest.mark.parametrize("npairs", [1, 255, 256, 257, 4096, 4097, 132253, 10**6, 12_800_000, (1 << 31) - 1])
@pytest.mark.parametrize("cus", [1, 256])
def test_slices_cover_the_list_once(plan, npairs, cus):
    p = plan(npairs=npairs, num_cus=cus)
    g, s = p["grid"], p["slice"]
    assert g >= 1 and s % 256 == 0
    assert (g - 1) * s < npairs <= g * s                                    # [w s, min(npairs, (w + 1) s)) for w < g: disjoint, none empty
    assert g <= 4 * cus                                                     # at most four workgroups per CU
    assert g == 1 or s >= p["min_slice"] // 2                               # no sliver of a slice
    assert g * s < (1 << 32)


def test_grids_and_launches(plan):
    p = plan(npairs=132253, nqueries=64)
    assert p["grid"] == 33 and p["slice"] == 4096 and p["sort_grid"] == 64 and p["launches"] == 4
    p = plan(npairs=0, nqueries=7)                                          # an empty list: the sort alone writes the empty rows
    assert p["grid"] == 0 and p["sort_grid"] == 7 and p["launches"] == 1
    p = plan(npairs=1000, nqueries=0)
    assert p["sort_grid"] == 0 and p["launches"] == 0
    p = plan(npairs=1000, nqueries=10**6)                                   # the sort's workgroups walk the queries in strides
    assert p["sort_grid"] == p["sort_grid_max"] == 65536


@pytest.mark.parametrize("kw", [{"npairs": -1}, {"npairs": 1 << 31}, {"nqueries": -1}, {"ntargets": -1}, {"ntargets": 1 << 31}, {"top": 0}, {"top": -3},
                                {"top": 4097}])
def test_refused(plan, kw):
    p = plan(**kw)
    assert isinstance(p["refused"], str) and p["refused"]
    assert p["grid"] == 0 and p["sort_grid"] == 0 and p["keys_need"] == 0    # nothing else of the plan is set


def test_accepted_at_the_edges(plan):
    for kw in ({"npairs": 0}, {"npairs": (1 << 31) - 1}, {"nqueries": 0}, {"ntargets": 0}, {"ntargets": (1 << 31) - 1}, {"top": 1}, {"top": 4096}):
        assert plan(**kw)["refused"] is None
