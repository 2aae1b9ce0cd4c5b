"""CPU: the planner of the PSSM update (swp::plan_pssm_hits, smith-waterman_amd/csrc/sw_plan.cpp), built with g++ and driven through
tests/pssm_hits_plan_driver.cpp: the tiles cover every column of every query once, a workgroup's LDS fits the device for every number of
letters, the column stride keeps adjacent columns in different banks, and the grid stays inside the device's bounds."""
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
    exe = str(tmp_path_factory.mktemp("plan") / "pssm_hits_plan")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "pssm_hits_plan_driver.cpp"),
                    os.path.join(ROOT, "smith-waterman_amd", "csrc", "sw_plan.cpp")], check=True)

    def run(cases):
        lines = "".join(f"qlens={','.join(map(str, q))} nletters={n} num_cus={cus}\n" for q, n, cus in cases)
        out = subprocess.run([exe], input=lines, capture_output=True, text=True, check=True).stdout
        return [json.loads(x) for x in out.splitlines()]
    return run


QUERY_SETS = [[1], [63], [64], [65], [513], [1, 63, 64, 65, 257, 513], [512] * 64, [1300, 2, 700], [(1 << 20) - 1], [40] * 1000]


def tiles_of(p, qlen):
    """The (first column, columns) of the tiles the kernel gives a query: tile i starts at i * tile_cols, surplus workgroups return."""
    return [(i * p["tile_cols"], min(p["tile_cols"], qlen - i * p["tile_cols"])) for i in range(p["tiles_per_query"]) if i * p["tile_cols"] < qlen]


def test_tiles_cover_every_column_once(plan):
    cases = [(q, n, cus) for q in QUERY_SETS for n in (1, 4, 24, 25, 255, 256) for cus in (1, 256)]
    for (qlens, n, cus), p in zip(cases, plan(cases)):
        for qlen in qlens:
            covered = [c for c0, cols in tiles_of(p, qlen) for c in range(c0, c0 + cols)] if qlen < 5000 else None
            if covered is not None:
                assert covered == list(range(qlen)), (qlens, n, cus)
            t = tiles_of(p, qlen)
            assert t[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(t, t[1:])) and t[-1][0] + t[-1][1] == qlen
            assert all(1 <= cols <= p["tile_cols"] for _, cols in t)
        assert p["launches"] == 1


def test_lds_fits_for_every_number_of_letters(plan):
    cases = [([513, 64], n, 256) for n in range(1, 257)] + [([(1 << 20) - 1], n, 1) for n in range(1, 257)]
    for (qlens, n, cus), p in zip(cases, plan(cases)):
        assert p["stride"] > n and p["stride"] % 2 == 1 and p["stride"] <= n + 2      # a spare dword for N[j]; odd: adjacent columns, other banks
        assert p["lds_bytes"] == p["code_bytes"] + 4 * p["tile_cols"] * p["stride"]
        assert p["lds_bytes"] <= p["lds_budget"] <= LDS_CU
        assert 1 <= p["tile_cols"] <= p["max_cols"]
        assert p["code_bytes"] + 4 * (p["max_cols"] + 1) * p["stride"] > p["lds_budget"]   # max_cols is what the budget holds, not less
    p25, p256 = plan([([512], 25, 256), ([513], 256, 256)])
    assert p25["max_cols"] == 604 >= 512                                               # a protein query of 512 columns fits one tile
    assert p256["tile_cols"] == 63 and p256["tiles_per_query"] == 9                    # 256 letters force tiles of a few dozen columns


def test_grid_stays_inside_the_device_bounds(plan):
    cases = [(q, n, cus) for q in QUERY_SETS + [[(1 << 20) - 1] * 50] for n in (1, 25, 256) for cus in (1, 256)]
    for (qlens, n, cus), p in zip(cases, plan(cases)):
        jobs = len(qlens) * p["tiles_per_query"]
        assert p["grid"] == min(jobs, p["grid_max"]) and 1 <= p["grid"] <= p["grid_max"] < (1 << 31)
        assert p["tiles_per_query"] == -(-max(qlens) // p["tile_cols"])
    p, = plan([([], 24, 256)])
    assert p["grid"] == 0 and p["launches"] == 0 and p["tiles_per_query"] == 0         # no query: nothing is launched


def test_tiles_spread_a_call_over_the_device(plan):
    p, = plan([([512] * 64, 25, 256)])                                                 # 32768 columns over 2 x 256 workgroups: 64 columns each
    assert p["tile_cols"] == 64 and p["grid"] == 512
    p, = plan([([512] * 64, 25, 1)])                                                   # one CU: whole queries, as many columns as the query has
    assert p["tile_cols"] == 512 and p["grid"] == 64
    p, = plan([([2000] * 3, 25, 1)])                                                   # ... or as the LDS holds
    assert p["tile_cols"] == p["max_cols"] == 604
