"""CPU: the planner of the per-query selection (swp::plan_search_top, smith-waterman_amd/csrc/sw_plan.cpp), built with g++ and driven
through tests/search_top_plan_driver.cpp: the chunks a result budget cuts, the workgroups of a row and their slices, the digit passes of
the radix select and the workspace sizes.  The occupancy is given, not measured."""
import json
import math
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIB = 1 << 20
RESULT = 24                     # sizeof(sw_result)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the planner")
    exe = str(tmp_path_factory.mktemp("plan") / "search_top_plan")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "search_top_plan_driver.cpp"),
                    os.path.join(ROOT, "smith-waterman_amd", "csrc", "sw_plan.cpp")], check=True)

    def run(**kw):
        kw = {"nqueries": 1, "ntargets": 1000, "top": 10, **kw}
        line = " ".join(f"{k}={v}" for k, v in kw.items())
        return json.loads(subprocess.run([exe], input=line + "\n", capture_output=True, text=True, check=True).stdout)
    return run


def test_chunks_under_a_budget_of_one_mib(plan):
    assert MIB // RESULT == 43690
    p = plan(nqueries=10, ntargets=20000, budget_bytes=MIB)             # 2 rows of 20 000 fit 43 690 results, 3 do not
    assert p["chunks"] == [[0, 2], [2, 2], [4, 2], [6, 2], [8, 2]] and p["chunk_queries"] == 2
    assert p["results_need"] == 2 * 20000 and p["results_need"] * RESULT <= MIB
    p = plan(nqueries=3, ntargets=50000, budget_bytes=MIB)              # a row larger than the budget is a chunk of its own
    assert p["chunks"] == [[0, 1], [1, 1], [2, 1]] and p["results_need"] == 50000
    p = plan(nqueries=7, ntargets=20000, budget_bytes=MIB)              # the last chunk takes what is left
    assert p["chunks"] == [[0, 2], [2, 2], [4, 2], [6, 1]]
    assert plan(nqueries=64, ntargets=200000)["chunks"] == [[0, 64]]    # the default of 1 GiB holds 223 such rows
    assert plan(nqueries=0, ntargets=20000)["chunks"] == []


@pytest.mark.parametrize("nq,nt,budget", [(1, 1, MIB), (10, 20000, MIB), (9000, 3, MIB), (5000, 0, MIB), (33, 4097, 10 * MIB), (4097, 5000, 1 << 40)])
def test_chunks_cover_every_query_once_in_order(plan, nq, nt, budget):
    p = plan(nqueries=nq, ntargets=nt, budget_bytes=budget)
    at = 0
    for q0, n in p["chunks"]:
        assert q0 == at and 1 <= n <= p["chunk_queries"]
        assert n == 1 or n * nt * RESULT <= budget
        at += n
    assert at == nq
    assert p["chunk_queries"] <= 4096                                   # bounds the histograms, whatever the budget
    assert p["results_need"] == p["chunk_queries"] * nt


@pytest.mark.parametrize("nt", [1, 63, 64, 65, 4097, 10**6])
@pytest.mark.parametrize("nq", [1, 64, 4096])
def test_slices_of_a_row_cover_the_targets_once(plan, nt, nq):
    p = plan(nqueries=nq, ntargets=nt, budget_bytes=1 << 40)
    assert p["kernel"] == (1 if nt > p["top_max"] else 0)
    if p["kernel"] == 0:
        return                                                          # one workgroup sorts the whole row: no slices
    w, s = p["wgs_row"], p["slice"]
    assert w >= 1 and s % 256 == 0
    assert (w - 1) * s < nt <= w * s                                    # [k s, min(nt, (k + 1) s)) for k < w: disjoint, none empty, all of 0..nt
    assert w == 1 or s >= 4096 // 2                                     # no sliver of a slice
    assert w * nq <= 8 * 256 + nq                                         # about one device full of workgroups at the given occupancy


def test_more_workgroups_per_row_with_fewer_rows(plan):
    one, many = plan(nqueries=1, ntargets=300000), plan(nqueries=64, ntargets=300000)
    assert one["wgs_row"] == 74 and one["slice"] == 4096                # bounded by the smallest slice: ceil(300000 / 4096)
    assert many["wgs_row"] == 32 and many["slice"] == 9472              # 8 x 256 workgroups over 64 rows; ceil(300000 / 32) in whole 256s
    assert plan(nqueries=64, ntargets=300000, per_cu=1, num_cus=64)["wgs_row"] == 1


@pytest.mark.parametrize("nt", [1, 2, 3, 64, 65, 4096, 4097, 300000, 10**6, (1 << 31) - 1])
def test_digit_passes_cover_every_bit_that_can_differ(plan, nt):
    p = plan(ntargets=nt, budget_bytes=1 << 40)
    tbits = math.ceil(math.log2(nt)) if nt > 1 else 0
    assert p["tbits"] == tbits and p["nbits"] == 24 + tbits and (1 << tbits) >= nt
    if p["kernel"] == 0:
        assert p["passes"] == []
        return
    hi = p["nbits"]
    for shift, bits in p["passes"]:                                      # highest bits first, back to back, down to bit 0
        assert 1 <= bits <= p["digit_bits"] and shift + bits == hi
        hi = shift
    assert hi == 0
    assert len(p["passes"]) == math.ceil(p["nbits"] / p["digit_bits"])


def test_workspace_sizes(plan):
    p = plan(nqueries=10, ntargets=20000, budget_bytes=MIB)
    assert p["hist_need"] == 2 * 2048 and p["state_need"] == 2 and p["results_need"] == 40000
    p = plan(nqueries=100000, ntargets=5000, budget_bytes=1 << 40)
    assert p["chunk_queries"] == 4096 and p["hist_need"] == 4096 * 2048 and p["state_need"] == 4096
    p = plan(nqueries=10, ntargets=4096)                                 # the sort alone needs neither
    assert p["kernel"] == 0 and p["hist_need"] == 0 and p["state_need"] == 0 and p["results_need"] == 40960
