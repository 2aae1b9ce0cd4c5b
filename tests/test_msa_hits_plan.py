"""CPU: the planner of the query-anchored alignment (swp::plan_msa_hits, smith-waterman_amd/csrc/sw_plan.cpp), built with g++ and
driven through tests/msa_hits_plan_driver.cpp: the slices of launch A cover every entry of a query exactly once in whole rounds of the
four waves, every grid stays inside the cap of the many-query plans, the scan has the chunks, levels and rounds its entries need, and a
call without a query, or without the row table, launches nothing, or launch A alone."""
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
    exe = str(tmp_path_factory.mktemp("plan") / "msa_hits_plan")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "msa_hits_plan_driver.cpp"),
                    os.path.join(ROOT, "smith-waterman_amd", "csrc", "sw_plan.cpp")], check=True)

    def run(cases):
        lines = "".join(f"nqueries={nq} top={top} num_cus={cus} rows={int(rows)}\n" for nq, top, cus, rows in cases)
        out = subprocess.run([exe], input=lines, capture_output=True, text=True, check=True).stdout
        return [json.loads(x) for x in out.splitlines()]
    return run


TOPS = [1, 2, 3, 4, 5, 10, 63, 64, 100, 4095, 4096]


def test_slices_cover_every_entry_once(plan):
    cases = [(nq, top, cus, True) for nq in (1, 3, 64, 300, 5000) for top in TOPS for cus in (1, 256, 304)]
    for (nq, top, cus, _), p in zip(cases, plan(cases)):
        s, n = p["slice_entries"], p["slices_per_query"]
        assert s >= 4 and s % 4 == 0                                           # whole rounds of the four waves
        # slice k holds the entries [k s, min(top, (k + 1) s)): disjoint by construction; together 0 .. top - 1, none of them empty
        assert (n - 1) * s < top <= n * s
        assert p["entries"] == nq * top
        assert p["cols_grid"] == min(nq * n, p["grid_max"])
        # the device is filled where there is work for it: no slice is larger than the entries over 8 workgroups per CU, in rounds
        share = -(-nq * top // (8 * cus))
        assert s <= max(4, -(-share // 4) * 4)


def test_grids_stay_inside_the_cap(plan):
    cases = [(nq, top, 256, True) for nq, top in ((1 << 20, 1), ((1 << 20) + 5, 4096), (1 << 24, 1), (4096, 4096), (3, 4096))]
    for (nq, top, cus, _), p in zip(cases, plan(cases)):
        for g in ("cols_grid", "scan_grid", "rows_grid"):
            assert 1 <= p[g] <= p["grid_max"] < (1 << 31)
        assert p["rows_grid"] == min(-(-nq * top // 4), p["grid_max"])
        assert p["scan_grid"] == min(p["scan_chunks"], p["grid_max"])


def test_scan_levels(plan):
    entries = [1, 255, 256, 257, 4096 * 3, 1 << 24]
    cases = [(n, 1, 256, True) for n in entries] + [(3, 4096, 256, True), (1 << 12, 4096, 256, True)]
    want = {1: (1, 1, 1), 255: (1, 1, 1), 256: (1, 1, 1), 257: (2, 2, 1), 4096 * 3: (48, 2, 1), 1 << 24: (1 << 16, 2, 256)}
    for (nq, top, cus, _), p in zip(cases, plan(cases)):
        n = nq * top
        assert p["chunk"] == 256 and p["entries"] == n
        assert p["scan_chunks"] == -(-n // 256) and p["sums_bytes"] == 8 * p["scan_chunks"]
        assert p["scan_levels"] == (1 if n <= 256 else 2) and p["top_rounds"] == -(-p["scan_chunks"] // 256)
        if n in want:
            assert (p["scan_chunks"], p["scan_levels"], p["top_rounds"]) == want[n]
        assert p["launches"] == 4


def test_no_query_and_no_rows(plan):
    p, = plan([(0, 10, 256, True)])
    assert all(p[f] == 0 for f in ("entries", "cols_grid", "scan_chunks", "scan_grid", "rows_grid", "launches", "sums_bytes"))
    p, = plan([(7, 10, 256, False)])
    assert p["launches"] == 1 and p["cols_grid"] >= 7 and p["scan_grid"] == p["rows_grid"] == p["scan_chunks"] == p["scan_levels"] == 0
