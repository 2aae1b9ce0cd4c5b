"""CPU: the planner's choice of the prologue's alphabet scan (smith-waterman_amd/csrc/sw_plan.cpp, TilePlan::scan_all) from both sides
of its limit, kScanAllLetters = 48 Ki letters of cols + rows.  tests/fill_plan_driver.cpp shows that nothing else of a plan moves at
the limit; its output has no field for the scan itself, which tests/prologue_plan_driver.cpp prints."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 48 * 1024
BARRIER_SCAN, SCAN_ALL = 1 << 28, 1 << 29
PLAN_CPP = os.path.join(ROOT, "smith-waterman_amd", "csrc", "sw_plan.cpp")


def _build(tmp, name):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the planner")
    exe = str(tmp / name)
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", name + ".cpp"), PLAN_CPP], check=True)
    return exe


@pytest.fixture(scope="module")
def scan_of(tmp_path_factory):
    exe = _build(tmp_path_factory.mktemp("prologue_plan"), "prologue_plan_driver")

    def run(cols, rows, s2w=0, flags=0):
        out = subprocess.run([exe], input=f"{cols} {rows} {s2w} {flags}\n", capture_output=True, text=True, check=True).stdout.split()
        assert int(out[0]) == LIMIT and int(out[1]) == 1, "the two-column kernel was expected"
        tiles = [int(x) for x in out[3:]]
        assert len(tiles) == int(out[2]) >= 1
        return tiles
    return run


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = _build(tmp_path_factory.mktemp("fill_plan"), "fill_plan_driver")

    def run(**kw):
        line = " ".join(f"{k}={v}" for k, v in {"num_cus": 256, "xcd_round_robin": 1, "s2_per_cu": 1, **kw}.items())
        return json.loads(subprocess.run([exe], input=line + "\n", capture_output=True, text=True, check=True).stdout)
    return run


@pytest.mark.parametrize("cols,rows", [(16384, 16384), (20480, 20480), (2, LIMIT - 2), (LIMIT - 1, 1), (LIMIT - 16, 16), (LIMIT // 2, LIMIT // 2)])
def test_up_to_the_limit_every_workgroup_scans_for_itself(scan_of, cols, rows):
    assert cols + rows <= LIMIT
    assert set(scan_of(cols, rows)) == {1}


@pytest.mark.parametrize("cols,rows", [(2, LIMIT - 1), (LIMIT, 1), (LIMIT - 15, 16), (LIMIT // 2 + 1, LIMIT // 2), (65536, 65536), (1 << 19, 1 << 19)])
def test_beyond_the_limit_the_scan_is_shared(scan_of, cols, rows):
    assert cols + rows > LIMIT
    assert set(scan_of(cols, rows)) == {0}


@pytest.mark.parametrize("cols,rows", [(30001, 333), (30001, LIMIT - 30001), (30001, LIMIT - 30000), (40001, LIMIT - 40001), (40001, LIMIT - 40000), (250001, 16)])
def test_every_column_tile_decides_alike(scan_of, cols, rows):
    """the whole matrix' columns decide, not the tile's: every tile scans the whole a"""
    tiles = scan_of(cols, rows, s2w=126)
    assert len(tiles) >= 2 and set(tiles) == {1 if cols + rows <= LIMIT else 0}


def test_debug_bits_force_either_scan(scan_of):
    assert set(scan_of(1000, 1000, flags=BARRIER_SCAN)) == {0}
    assert set(scan_of(1 << 18, 1 << 18, flags=SCAN_ALL)) == {1}
    assert set(scan_of(30001, 333, s2w=126, flags=BARRIER_SCAN)) == {0}


@pytest.mark.parametrize("cols,rows", [(2, LIMIT - 2), (LIMIT - 16, 16), (LIMIT // 2, LIMIT // 2), (131072, 131072)])
def test_nothing_else_moves_at_the_limit(plan, cols, rows):
    """the rest of the plan is what the scan's debug bits leave it: the limit changes the prologue and nothing else"""
    base = plan(cols=cols, rows=rows)
    assert base["two_cols"] == 1
    assert plan(cols=cols, rows=rows, debug_flags=BARRIER_SCAN) == base
    assert plan(cols=cols, rows=rows, debug_flags=SCAN_ALL) == base
