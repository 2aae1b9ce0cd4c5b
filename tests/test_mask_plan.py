"""CPU: the planner of the low-complexity mask (swp::plan_mask, smith-waterman_amd/csrc/sw_plan.cpp), built with g++ and driven through
tests/mask_plan_driver.cpp: the tiles cover the positions exactly once, a workgroup's lanes cover a tile, the halo is W - 1, the
workspace holds the three bit arrays, the summaries and the carries without overlap, every grid stays inside the cap of the many-query
plans, from one letter to 2^31 - 1 letters at windows 2 and 64; a handle without letters launches only the count."""
import json
import os
import shutil
import subprocess

import pytest

import mask_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LETTERS = [1, 2, 63, 64, 65, 4095, 4096, 4097, 8192, 70_000_000, (1 << 31) - 4096, (1 << 31) - 1]


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the planner")
    exe = str(tmp_path_factory.mktemp("plan") / "mask_plan")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "mask_plan_driver.cpp"),
                    os.path.join(ROOT, "smith-waterman_amd", "csrc", "sw_plan.cpp")], check=True)

    def run(cases):
        lines = "".join(f"letters={n} ntargets={nt} window={w} count={int(c)}\n" for n, nt, w, c in cases)
        out = subprocess.run([exe], input=lines, capture_output=True, text=True, check=True).stdout
        return [json.loads(x) for x in out.splitlines()]
    return run


def test_tiles_cover_the_positions_once(plan):
    cases = [(n, 1, w, True) for n in LETTERS for w in (2, 12, 64)]
    for (n, _, w, _), p in zip(cases, plan(cases)):
        T = p["tile"]
        # tile i holds [i T, min(n, (i + 1) T)): the tiles are disjoint by construction and cover [0, n) iff the last one reaches n
        assert T == 4096 and p["tiles"] == -(-n // T) and (p["tiles"] - 1) * T < n <= p["tiles"] * T
        assert p["starts_per_lane"] * 256 == T and p["tile_words"] * 64 == T and p["halo"] == w - 1 <= 63
        assert p["g_window"] == mc.G[w]


def test_workspace_holds_the_bits(plan):
    cases = [(n, 5, w, True) for n in LETTERS for w in (2, 64)]
    for (n, _, w, _), p in zip(cases, plan(cases)):
        words = p["tiles"] * p["tile_words"]
        assert p["words"] == words and 64 * words >= n
        parts = [(p["low1_off"], 8 * words), (p["low2_off"], 8 * words), (p["mask_off"], 8 * words), (p["summary_off"], 4 * p["tiles"]),
                 (p["carry_off"], 4 * p["tiles"])]
        at = 0
        for off, size in parts:                       # in order, back to back, each aligned for its element
            assert off == at and off % 8 in (0, 4) and (size % 8 == 0 or off >= p["summary_off"])
            at = off + size
        assert p["workspace_bytes"] == at and p["low1_off"] % 8 == p["low2_off"] % 8 == p["mask_off"] % 8 == 0 and p["summary_off"] % 4 == 0


def test_grids_stay_inside_the_cap(plan):
    cases = [(n, nt, w, True) for n in LETTERS for nt in (1, 255, 256, 257, 100_000_000, (1 << 31) - 1) for w in (2, 64)]
    for (n, nt, w, _), p in zip(cases, plan(cases)):
        assert 1 <= p["window_grid"] == p["apply_grid"] == min(p["tiles"], p["grid_max"]) < (1 << 31)
        assert p["carry_grid"] == 1 and p["carry_threads"] == 1024
        assert 1 <= p["count_grid"] == min(-(-nt // p["count_targets"]), p["grid_max"]) and p["launches"] == 4
    p, = plan([(70_000_000, 200_000, 12, False)])
    assert p["count_grid"] == 0 and p["launches"] == 3


def test_without_letters_only_the_count_runs(plan):
    a, b, c = plan([(0, 7, 12, True), (0, 7, 12, False), (0, 0, 12, True)])
    assert a["tiles"] == a["window_grid"] == a["carry_grid"] == a["apply_grid"] == a["workspace_bytes"] == 0 and a["count_grid"] == 1 and a["launches"] == 1
    for p in (b, c):
        assert all(p[f] == 0 for f in ("tiles", "window_grid", "carry_grid", "apply_grid", "count_grid", "workspace_bytes", "launches"))
