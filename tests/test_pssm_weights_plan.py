"""CPU: the planner of the hit weights (swp::plan_pssm_weights, smith-waterman_amd/csrc/sw_plan.cpp), built with g++ and driven through
tests/pssm_weights_plan_driver.cpp: the tile launch is cut exactly as the update's (one tile rule, not two), its LDS fits the device for
every number of letters, the accumulators hold one 64-bit word per entry of the table, the finish launch has one workgroup per query
inside the device's bounds, and a call without a query launches nothing."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_CU = 160 * 1024


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the planner")
    exe = str(tmp_path_factory.mktemp("plan") / "pssm_weights_plan")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "pssm_weights_plan_driver.cpp"),
                    os.path.join(ROOT, "smith-waterman_amd", "csrc", "sw_plan.cpp")], check=True)

    def run(cases):
        lines = "".join(f"qlens={','.join(map(str, q))} nletters={n} num_cus={cus} top={top}\n" for q, n, cus, top in cases)
        out = subprocess.run([exe], input=lines, capture_output=True, text=True, check=True).stdout
        return [json.loads(x) for x in out.splitlines()]
    return run


QUERY_SETS = [[1], [63], [64], [65], [513], [1, 63, 64, 65, 257, 513], [512] * 64, [1300, 2, 700], [(1 << 20) - 1], [40] * 1000]


def test_the_tile_launch_is_the_updates(plan):
    cases = [(q, n, cus, top) for q in QUERY_SETS for n in (1, 4, 24, 25, 255, 256) for cus in (1, 256) for top in (1, 4096)]
    for case, p in zip(cases, plan(cases)):
        for f in ("stride", "tile_cols", "tiles_per_query", "grid", "lds_bytes"):
            assert p[f] == p["hits_" + f], (case, f)
        assert p["tile_launches"] == 1 and p["launches"] == 2


def test_lds_fits_and_tiles_cover_every_column(plan):
    cases = [([513, 64], n, 256, 10) for n in range(1, 257)]
    for (qlens, n, cus, top), p in zip(cases, plan(cases)):
        assert p["stride"] > n and p["stride"] % 2 == 1                                 # a spare dword for k_j; odd: adjacent columns, other banks
        assert p["lds_bytes"] == p["code_bytes"] + 4 * p["tile_cols"] * p["stride"] <= p["lds_budget"] <= LDS_CU
        assert 1 <= p["tile_cols"] <= p["max_cols"]
        assert p["tiles_per_query"] * p["tile_cols"] >= max(qlens) > (p["tiles_per_query"] - 1) * p["tile_cols"]
    p, = plan([([513], 256, 256, 3)])
    assert p["tiles_per_query"] == 9                                                    # 256 letters: a 513-column query takes several tiles


def test_accumulators_and_finish_grid(plan):
    cases = [(q, 25, cus, top) for q in QUERY_SETS for cus in (1, 256) for top in (1, 10, 4095, 4096)]
    cases.append(([3] * ((1 << 20) + 5), 25, 256, 10))                                  # more queries than the grid may have workgroups
    for (qlens, n, cus, top), p in zip(cases, plan(cases)):
        assert p["acc_entry_bytes"] == 8
        assert p["acc_entries"] == len(qlens) * top and p["acc_bytes"] == 8 * p["acc_entries"]
        assert p["finish_grid"] == min(len(qlens), p["grid_max"]) and 1 <= p["finish_grid"] < (1 << 31)
        assert 1 <= p["grid"] <= p["grid_max"] < (1 << 31)


def test_no_query_launches_nothing(plan):
    p, = plan([([], 24, 256, 10)])
    assert p["grid"] == 0 and p["finish_grid"] == 0 and p["launches"] == 0 and p["acc_bytes"] == 0
