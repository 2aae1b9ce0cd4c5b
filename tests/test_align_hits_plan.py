"""CPU: the planner of the hit-table alignment (swp::plan_align_hits, smith-waterman_amd/csrc/sw_plan.cpp), built with g++ and driven
through tests/align_hits_plan_driver.cpp: groups under the profile budget and the item-list bound, the size tiers of every class, the
slots of every launch under the workspace budget, and the refusal of a worst case that does not fit.  The occupancies are given, not
measured; nothing here looks at a target or a hit."""
import itertools
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIB = 1 << 20
ROWS = 257                      # profile rows per query
SLOT_LIMIT = (1 << 31) - 256    # a slot is addressed through one buffer descriptor
BND_BYTES = 1 << 30             # the boundary columns of a launch


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the planner")
    exe = str(tmp_path_factory.mktemp("ahplan") / "align_hits_plan")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "align_hits_plan_driver.cpp"),
                    os.path.join(ROOT, "smith-waterman_amd", "csrc", "sw_plan.cpp")], check=True)

    def run(qlens, **kw):
        kw = {"top": 10, "longest": 700, "num_cus": 256, "per_cu": "5,4,2", **kw}
        line = "qlens=" + ",".join(str(q) for q in qlens) + " " + " ".join(f"{k}={v}" for k, v in kw.items())
        return json.loads(subprocess.run([exe], input=line + "\n", capture_output=True, text=True, check=True).stdout)
    return run


def lane_columns(qlen, per_cu):
    C = 4 if qlen <= 256 else 8 if qlen <= 512 else 16
    return 8 if C == 16 and per_cu[2] < 2 else C


def padded(qlen, per_cu):
    w = 64 * lane_columns(qlen, per_cu)
    return (qlen + w - 1) // w * w


QSETS = [[1], [256, 257, 512, 513], [1, 64, 256, 257, 512, 513, 1025, 2049], [2049, 7, 300, 5000, 64, 1024], [512] * 64]
GRID = list(itertools.product(QSETS, [0, 1, 500, 35000], [MIB, 64 * MIB, 1024 * MIB], ["5,4,2", "5,4,1", "1,1,1"], [1, 10, 4096]))


@pytest.mark.parametrize("qlens,longest,budget,per_cu,top", GRID)
def test_tiers_slots_and_groups(plan, qlens, longest, budget, per_cu, top):
    occ = [int(x) for x in per_cu.split(",")]
    p = plan(qlens, longest=longest, budget_bytes=budget, per_cu=per_cu, top=top, profile_budget_bytes=4 * MIB, max_items=30000)
    rows = max(1, longest)
    worst = rows * max(padded(q, occ) for q in qlens)
    assert p["worst_bytes"] == worst
    assert p["fits"] == (0 if worst > budget or worst > SLOT_LIMIT else 1)             # refused exactly when the worst case does not fit
    if not p["fits"]:
        assert p["groups"] == [] and p["launch"] == []
        return
    # groups: every query once, in order; under the profile budget and the item-list bound unless a single query
    assert p["in_order"] == 1 and p["covered"] == len(qlens) and p["entries"] == len(qlens) * top
    assert sorted(t[1] for t in p["table"]) == list(range(len(qlens)))
    for g in p["groups"]:
        members = p["table"][g["q0"]:g["q0"] + g["nq"]]
        assert sorted(t[1] for t in members) == list(range(g["q0"], g["q0"] + g["nq"]))   # consecutive queries
        assert g["prof_bytes"] == sum(ROWS * t[3] for t in members)
        assert g["nq"] == 1 or (g["prof_bytes"] <= 4 * MIB and g["nq"] * top <= 30000)
        assert g["nq"] * top <= p["items_need"] and g["prof_bytes"] <= p["prof_need"]
        at = off = 0
        for k, c in enumerate(g["cls"]):
            C = (4, 8, 16)[k]
            mine = p["table"][c["q0"]:c["q0"] + c["nq"]]
            assert c["q0"] == g["q0"] + at and c["item0"] == at * top and c["entries"] == c["nq"] * top
            at += c["nq"]
            for t in mine:                                                               # the class of every query, its table entry
                assert lane_columns(t[2], occ) == C and t[3] == padded(t[2], occ) and t[4] == t[3] // (64 * C) and t[0] == off
                off += ROWS * t[3]
            if not mine:
                assert c["bound"] == []
                continue
            b = c["bound"]
            assert 1 <= len(b) <= p["max_tiers"] and b == sorted(b)
            assert b[-1] == rows * max(t[3] for t in mine)                               # the top tier holds the class's worst case
            for lo, hi in zip(b, b[1:]):
                assert lo == hi // p["tier_ratio"]
            assert len(b) == 1 or b[0] >= p["tier_floor"]
            assert len(b) == p["max_tiers"] or b[0] // p["tier_ratio"] < p["tier_floor"]
            # every size an item of this class can have has a tier that holds it
            for t in mine:
                for n in {n for n in (1, 2, rows // 3 + 1, rows - 1, rows) if 1 <= n <= rows}:
                    assert any(n * t[3] <= x for x in b)
        assert at == g["nq"]
    # launches: one per tier, the largest first within a class; slots under the budget, at least one, at most the resident waves
    want = [(gi, k, t) for gi, g in enumerate(p["groups"]) for k, c in enumerate(g["cls"]) for t in reversed(range(len(c["bound"])))]
    assert [(l["group"], l["kernel"], l["tier"]) for l in p["launch"]] == want
    assert p["tiers"] == len(want) and p["slots"] == sum(l["slots"] for l in p["launch"])
    for l in p["launch"]:
        c = p["groups"][l["group"]]["cls"][l["kernel"]]
        assert l["C"] == (4, 8, 16)[l["kernel"]] and l["slot_bytes"] == c["bound"][l["tier"]]
        assert 1 <= l["slots"] <= max(1, min(occ[l["kernel"]] * 256 * 4, c["entries"]))
        assert l["slots"] * l["slot_bytes"] <= budget and l["slots"] * l["slot_bytes"] <= p["dir_need"]
        assert l["grid"] == (l["slots"] + 3) // 4
        if c["nstrips"] > 1:    # the boundary column holds every row an item of several strips can have in this tier, with the kernel's slack
            tier_rows = min(rows, l["slot_bytes"] // (2 * 64 * l["C"]))
            assert l["bnd_per"] >= 2 * (tier_rows + 70)
            assert l["slots"] == 1 or l["slots"] * l["bnd_per"] * 4 <= BND_BYTES
            assert l["slots"] * l["bnd_per"] <= p["bnd_need"]
        else:
            assert l["bnd_per"] == 0


def test_the_tiers_of_a_protein_database(plan):
    p = plan([512] * 64, longest=35000, budget_bytes=1024 * MIB, top=100)
    (g,) = p["groups"]
    assert g["cls"][1]["bound"] == [35000 * 512 // 64, 35000 * 512 // 16, 35000 * 512 // 4, 35000 * 512]
    assert [l["slots"] for l in p["launch"]] == [59, 239, 958, 3834]                    # budget / size, no more than the class's 6400 entries
    assert p["tiers"] == 4 and p["slots"] == 59 + 239 + 958 + 3834
    p = plan([512] * 64, longest=35000, budget_bytes=1024 * MIB, top=10)
    assert [l["slots"] for l in p["launch"]] == [59, 239, 640, 640]                     # ... no more than its 640
    p = plan([100], longest=300, top=5)
    assert p["groups"][0]["cls"][0]["bound"] == [300 * 256] and [l["slots"] for l in p["launch"]] == [5]


def test_refusal_depends_on_host_data_alone(plan):
    assert plan([1025], longest=500, budget_bytes=MIB)["fits"] == 1                     # 500 x 2048
    assert plan([1025], longest=513, budget_bytes=MIB)["fits"] == 0
    assert plan([1024, 7], longest=1024, budget_bytes=MIB)["fits"] == 1 and plan([1024, 7], longest=1025, budget_bytes=MIB)["fits"] == 0
    assert plan([5000], longest=(1 << 20) - 1, budget_bytes=1 << 40)["fits"] == 0       # beyond a buffer descriptor, whatever the budget
    assert plan([2049], longest=(1 << 20) - 1, budget_bytes=1 << 40)["fits"] == 0 and plan([2048], longest=(1 << 20) - 1, budget_bytes=1 << 40)["fits"] == 1


def test_groups_under_the_profile_budget(plan):
    prof = ROWS * 2048
    p = plan([1025] * 5, longest=100, profile_budget_bytes=2 * prof)
    assert [(g["q0"], g["nq"]) for g in p["groups"]] == [(0, 2), (2, 2), (4, 1)] and p["prof_need"] == 2 * prof
    p = plan([1025] * 3, longest=100, profile_budget_bytes=prof - 1)                    # a query too big for the budget is a group of its own
    assert [(g["q0"], g["nq"]) for g in p["groups"]] == [(0, 1), (1, 1), (2, 1)]
    p = plan([64] * 10, longest=100, top=7, max_items=21)                               # the item-list bound: 3 queries x 7
    assert [g["nq"] for g in p["groups"]] == [3, 3, 3, 1] and p["items_need"] == 21


@pytest.mark.parametrize("top,rep", [(4096, 1 << 18), (2047, 1 << 19), (1, 1 << 21)])
def test_item_counts_at_and_beyond_2_31(plan, top, rep):
    """2^20 / 2^21 queries: nqueries x top reaches 2^32, (2^31 - 1) x ~1 and 2^23 entries; the plan only ever multiplies counts."""
    qlens = [100, 300, 600, 64] if rep < (1 << 21) else [100]
    p = plan(qlens, rep=rep, top=top, longest=400, detail=0, profile_budget_bytes=1 << 40)
    nq = len(qlens) * rep
    assert p["fits"] == 1 and p["covered"] == nq and p["in_order"] == 1
    assert p["entries"] == nq * top and (top == 1 or p["entries"] >= (1 << 31) - 1)
    per_group = max(1, (1 << 22) // top)
    assert p["ngroups"] == -(-nq // per_group) and p["items_need"] == min(nq, per_group) * top <= 1 << 22
    assert p["nlaunches"] == p["tiers"] >= p["ngroups"]


@pytest.mark.parametrize("top", [(1 << 31) - 1, 1 << 31])
def test_one_row_of_2_31_entries(plan, top):
    """(The C-ABI bounds top by SW_TOP_MAX; the planner's arithmetic holds beyond it.)"""
    p = plan([100, 100], top=top, longest=400)
    assert p["entries"] == 2 * top and [g["nq"] for g in p["groups"]] == [1, 1] and p["items_need"] == top
    assert all(l["slots"] == min(5 * 256 * 4, (1 << 30) // l["slot_bytes"]) for l in p["launch"])
