"""CPU: the planner of the alignment filter (swp::plan_msa_filter, smith-waterman_amd/csrc/sw_plan.cpp), built with g++ and driven
through tests/msa_filter_plan_driver.cpp: the tiles cover every pair r' < r of a query's rows exactly once, the chunks of queries stay
inside the workspace budget from both sides of every threshold, one query of top 4096 is never refused, every grid stays inside the
cap of the many-query plans, and a call without a query launches nothing."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOPS = [1, 2, 63, 64, 65, 100, 4095, 4096]
MIB = 1 << 20


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the planner")
    exe = str(tmp_path_factory.mktemp("plan") / "msa_filter_plan")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "msa_filter_plan_driver.cpp"),
                    os.path.join(ROOT, "smith-waterman_amd", "csrc", "sw_plan.cpp")], check=True)

    def run(cases, tiles=False):
        lines = "".join(f"nqueries={nq} top={top} budget_bytes={budget} tiles={int(tiles)}\n" for nq, top, budget in cases)
        out = subprocess.run([exe], input=lines, capture_output=True, text=True, check=True).stdout
        return [json.loads(x) for x in out.splitlines()]
    return run


def test_tiles_cover_every_pair_once(plan):
    cases = [(3, top, 256 * MIB) for top in TOPS]
    for (_, top, _), p in zip(cases, plan(cases, tiles=True)):
        blocks = -(-top // 64)
        assert p["tile"] == 64 and p["blocks"] == blocks and p["tiles_per_query"] == blocks * (blocks + 1) // 2 == len(p["tiles"])
        tiles = [tuple(t) for t in p["tiles"]]
        # a tile (rb, cb) compares the rows of block rb with the rows r' of block cb, on the diagonal with r' < r only: the pair
        # (r', r) lies in (r // 64, r' // 64) alone, so the tiles cover every pair once exactly when they are the triangle cb <= rb, each once
        assert len(set(tiles)) == len(tiles) and set(tiles) == {(rb, cb) for rb in range(blocks) for cb in range(rb + 1)}
        if top <= 100:
            index = {t: k for k, t in enumerate(tiles)}
            seen = [0] * len(tiles)
            for r in range(top):
                for rp in range(r):
                    seen[index[(r // 64, rp // 64)]] += 1
            assert sum(seen) == top * (top - 1) // 2
        # every diagonal tile is there: it also holds its rows against the query
        assert all((b, b) in tiles for b in range(blocks))
        assert p["query_words"] == (blocks + 1) * blocks * 64 and p["query_bytes"] == 8 * p["query_words"] and p["chunk_cols"] % 4 == 0


def test_chunks_stay_inside_the_budget(plan):
    cases = []
    for top in TOPS:
        blocks = -(-top // 64)
        qb = 8 * (blocks + 1) * blocks * 64
        for k in (1, 2, 5, 64):
            for budget in (k * qb - 1, k * qb, k * qb + 1):
                for nq in (1, k - 1, k, k + 1, 2 * k, 2 * k + 1, 300):
                    if nq >= 1:
                        cases.append((nq, top, budget))
    for (nq, top, budget), p in zip(cases, plan(cases)):
        qb = p["query_bytes"]
        per = p["queries_per_chunk"]
        assert per == max(1, min(nq, budget // qb))
        assert p["workspace_bytes"] == per * qb and (p["workspace_bytes"] <= budget or per == 1)
        # as many as fit: one more query would not, unless the call has no more
        assert per == nq or (per + 1) * qb > budget
        assert p["chunks"] == -(-nq // per) and p["last_queries"] == nq - (p["chunks"] - 1) * per and 1 <= p["last_queries"] <= per
        assert p["launches"] == 2 * p["chunks"]


def test_one_query_of_top_4096_is_never_refused(plan):
    cases = [(1, 4096, b) for b in (0, 1, MIB, 3 * MIB, 256 * MIB)] + [(5, 4096, MIB)]
    for (nq, top, budget), p in zip(cases, plan(cases)):
        assert p["queries_per_chunk"] >= 1 and p["chunks"] == (nq if budget < p["query_bytes"] else -(-nq // (budget // p["query_bytes"])))
        assert p["pair_grid"] >= 1 and p["greedy_grid"] >= 1
        # the least value of the option holds one such query
        assert (p["min_mib"] - 1) * MIB < p["query_bytes"] <= p["min_mib"] * MIB


def test_grids_stay_inside_the_cap(plan):
    cases = [(1 << 20, 1, 1 << 40), ((1 << 20) + 5, 1, 1 << 40), (4096, 4096, 1 << 40), (3, 4096, 256 * MIB), (1000, 100, 3 * MIB), (1 << 24, 64, 1 << 50)]
    for (nq, top, budget), p in zip(cases, plan(cases)):
        for g, n in (("pair_grid", p["queries_per_chunk"] * p["tiles_per_query"]), ("greedy_grid", p["queries_per_chunk"]),
                     ("last_pair_grid", p["last_queries"] * p["tiles_per_query"]), ("last_greedy_grid", p["last_queries"])):
            assert 1 <= p[g] <= p["grid_max"] < (1 << 31) and p[g] == min(n, p["grid_max"])


def test_no_query_launches_nothing(plan):
    p, = plan([(0, 100, 256 * MIB)])
    assert all(p[f] == 0 for f in ("queries_per_chunk", "chunks", "workspace_bytes", "pair_grid", "greedy_grid", "last_queries", "last_pair_grid",
                                   "last_greedy_grid", "launches"))
