"""CPU: the planner of the score histogram (swp::plan_score_hist, smith-waterman_amd/csrc/sw_plan.cpp), built with g++ and driven
through tests/score_hist_plan_driver.cpp: the work items cover every target of every query exactly once, no slice is empty, the LDS
copies stay inside 160 KiB, the slice count at 1, 64 and 4096 queries, every grid inside the cap of the many-query plans, and a call
without a query or a target launches nothing."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the planner")
    exe = str(tmp_path_factory.mktemp("plan") / "score_hist_plan")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "score_hist_plan_driver.cpp"),
                    os.path.join(ROOT, "smith-waterman_amd", "csrc", "sw_plan.cpp")], check=True)

    def run(cases):
        lines = "".join(f"nqueries={nq} ntargets={nt} num_cus={cus} copies={cp}\n" for nq, nt, cus, cp in cases)
        out = subprocess.run([exe], input=lines, capture_output=True, text=True, check=True).stdout
        return [json.loads(x) for x in out.splitlines()]
    return run


def test_items_cover_every_target_once(plan):
    cases = [(nq, nt, cus, 0) for nq in (1, 3, 64, 70, 4096) for nt in (1, 63, 64, 65, 257, 4095, 4096, 4097, 5000, 8191, 8192, 25000, 200000, (1 << 31) - 1)
             for cus in (1, 256, 304)]
    for (nq, nt, cus, _), p in zip(cases, plan(cases)):
        s, per = p["slices_per_query"], p["slice"]
        assert s >= 1 and per >= 1 and p["items"] == nq * s
        # item w = (query w // s, targets [k per, min(nt, (k + 1) per)) with k = w % s): the slices tile [0, nt), none empty
        assert (s - 1) * per < nt <= s * per
        assert per >= min(nt, p["min_slice"]) and s <= p["max_slices"]
        assert s <= max(1, cus * p["wgs_per_cu"] // nq)                       # no more slices than fill the device
        assert 1 <= p["grid"] == min(p["items"], p["grid_max"]) < (1 << 31) and p["launches"] == 1


def test_slice_count_at_1_64_and_4096_queries(plan):
    p1, p64, p4096 = plan([(1, 200000, 256, 0), (64, 200000, 256, 0), (4096, 200000, 256, 0)])
    assert p1["slices_per_query"] == 48 and p1["slice"] == 4167                # 200 000 // 4096 slices of at least 4096 targets
    assert p64["slices_per_query"] == 16 and p64["slice"] == 12500             # 4 workgroups per CU over 64 queries
    assert p4096["slices_per_query"] == 1 and p4096["slice"] == 200000 and p4096["grid"] == 4096


def test_lds_stays_inside_160_kib(plan):
    cases = [(64, 200000, 256, cp) for cp in (0, 1, 2, 3, 4, 5, 8, -1)]
    for (_, _, _, cp), p in zip(cases, plan(cases)):
        assert p["copies"] == (cp if cp in (1, 2, 4) else 1)
        assert p["cells"] == 40 * 256 and p["lds_bytes"] == p["copies"] * 40 * 256 * 4 <= p["lds_max"] == 160 << 10


def test_grids_stay_inside_the_cap(plan):
    cases = [(1 << 20, 100, 256, 0), ((1 << 20) + 5, 100, 256, 0), (1 << 24, 10000, 256, 0), (5000, 1 << 24, 256, 0)]
    for (nq, nt, _, _), p in zip(cases, plan(cases)):
        assert 1 <= p["grid"] == min(p["items"], p["grid_max"]) and p["threshold_grid"] == min(nq, p["grid_max"]) and p["threshold_launches"] == 1


def test_nothing_to_count_launches_nothing(plan):
    for p in plan([(0, 100, 256, 0), (5, 0, 256, 0), (0, 0, 256, 0)]):
        assert p["grid"] == 0 and p["items"] == 0 and p["launches"] == 0 and p["slices_per_query"] == 0
    p, = plan([(0, 100, 256, 0)])
    assert p["threshold_grid"] == 0 and p["threshold_launches"] == 0
