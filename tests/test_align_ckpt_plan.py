"""CPU: the planners of checkpointed alignment (swp::plan_align_ckpt, swp::plan_align_hits_ckpt, swp::align_use_ckpt;
smith-waterman_amd/csrc/sw_plan.cpp), built with g++ and driven through tests/align_ckpt_plan_driver.cpp: the band height, the slot
formula, the refusal, the slots, and the tiers of the hit-table call.  The occupancies are given, not measured."""
import itertools
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIB = 1 << 20
SLOT_LIMIT = (1 << 31) - 256
BND_BYTES = 1 << 30
CANDIDATES = [1 << k for k in range(6, 21)]          # the 15 band heights there are
FLOOR = 256
PER_CU = [5, 4, 2]


def slot_bytes(n, qpad, B):
    """The formula of the issue, an empty hit counted as one row."""
    n = max(1, n)
    return qpad * (min(B, n) + 8 * (-(-n // B) - 1))


LENS = [0, 1, 63, 64, 65, 700, 4336, 35000, 5 * 10**6, (1 << 31) - 1]
QPADS = [256, 512, 1024, 4096]
BUDGETS = [MIB, 64 * MIB, 1024 * MIB]
FORCED = [0, 64, 4096]
GRID = list(itertools.product(LENS, QPADS, BUDGETS, FORCED))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the planner")
    exe = str(tmp_path_factory.mktemp("ckplan") / "align_ckpt_plan")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "align_ckpt_plan_driver.cpp"),
                    os.path.join(ROOT, "smith-waterman_amd", "csrc", "sw_plan.cpp")], check=True)

    def run(lines):
        out = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, check=True).stdout
        return [json.loads(ln) for ln in out.splitlines()]
    return run


@pytest.fixture(scope="module")
def grid(driver):
    """Every case of GRID in one run of the driver, 300 hits each."""
    lines = [f"what=one len={n} qlen={q} budget_bytes={b} forced={f} nhits=300 num_cus=256 per_cu=5,4,2" for n, q, b, f in GRID]
    return dict(zip(GRID, driver(lines)))


@pytest.mark.parametrize("n,qpad,budget,forced", GRID)
def test_band_slot_and_refusal(grid, n, qpad, budget, forced):
    p = grid[(n, qpad, budget, forced)]
    assert (p["floor"], p["min_rows"], p["max_rows"], p["slot_limit"]) == (FLOOR, CANDIDATES[0], CANDIDATES[-1], SLOT_LIMIT)
    assert p["qpad"] == qpad and p["C"] == {256: 4, 512: 8, 1024: 16, 4096: 16}[qpad] and p["nstrips"] == qpad // (64 * p["C"])
    B = p["band_rows"]
    assert B in CANDIDATES and B == 1 << p["log_band"]
    assert p["slot_bytes"] == p["formula"] == slot_bytes(n, qpad, B)
    # what the planner may choose from: the forced height alone, or every candidate at or above the floor
    admissible = [forced] if forced else [c for c in CANDIDATES if c >= FLOOR]
    assert B in admissible
    best = min(slot_bytes(n, qpad, c) for c in admissible)               # brute force over the candidates
    assert p["slot_bytes"] == best
    assert B == max(c for c in admissible if slot_bytes(n, qpad, c) == best)   # a tie goes to the larger band
    if max(1, n) <= FLOOR and not forced:
        assert p["slot_bytes"] == max(1, n) * qpad                       # one band, no checkpoint: the whole-matrix layout
    assert p["fits"] == (0 if best > budget or best > SLOT_LIMIT else 1)   # refused exactly when the smallest admissible slot does not fit
    if not p["fits"]:
        return
    resident = PER_CU[p["kernel"]] * 256 * 4
    slots = min(300, resident, budget // p["slot_bytes"])
    if p["nstrips"] > 1:                                                 # a boundary column is one band's, with the kernel's slack
        band = min(B, max(1, n))
        assert 2 * (band + 70) <= p["bnd_per"] <= 2 * (band + 164)
        slots = min(slots, BND_BYTES // (p["bnd_per"] * 4))
    else:
        assert p["bnd_per"] == 0
    assert p["slots"] == max(1, slots) and p["grid"] == (p["slots"] + 3) // 4
    assert p["dir_need"] == p["slots"] * p["slot_bytes"] <= max(budget, p["slot_bytes"]) and p["bnd_need"] == p["slots"] * p["bnd_per"]


def test_the_figures_of_the_issue(driver):
    a, b = driver(["what=one len=4336 qlen=512 nhits=100 per_cu=5,4,2", "what=one len=5000000 qlen=1024 nhits=1 per_cu=5,4,2"])
    assert (a["band_rows"], a["slot_bytes"]) == (256, 192 << 10)         # the protein hit of DESIGN 9e: 192 KiB against 2.2 MB
    assert b["band_rows"] == 8192 and b["slot_bytes"] == 1024 * (8192 + 8 * 610) and b["fits"] == 1    # 5 M rows x 1024: 13 MB against 5 GB
    c16, c8 = driver(["what=one len=700 qlen=1025 nhits=9 per_cu=5,4,2", "what=one len=700 qlen=1025 nhits=9 per_cu=5,4,1"])
    assert (c16["C"], c16["qpad"], c8["C"], c8["qpad"]) == (16, 2048, 8, 1536)   # an instantiation that does not hold two workgroups per CU is not picked


QSETS = [[1], [256, 257, 512, 513], [100, 300, 600], [2049, 7, 300, 5000, 64, 1024], [512] * 64]
HGRID = list(itertools.product(range(len(QSETS)), [0, 1, 700, 35000, 5 * 10**6], BUDGETS, FORCED, [0, 1, 2]))


def padded(qlen):
    w = 64 * (4 if qlen <= 256 else 8 if qlen <= 512 else 16)
    return (qlen + w - 1) // w * w


@pytest.fixture(scope="module")
def hgrid(driver):
    lines = [f"what=hits qlens={','.join(str(q) for q in QSETS[s])} longest={n} budget_bytes={b} forced={f} mode={m} top=10 num_cus=256 per_cu=5,4,2"
             for s, n, b, f, m in HGRID]
    return dict(zip(HGRID, driver(lines)))


@pytest.mark.parametrize("s,longest,budget,forced,mode", HGRID)
def test_hit_table_tiers_and_mode(hgrid, s, longest, budget, forced, mode):
    p = hgrid[(s, longest, budget, forced, mode)]
    qlens, rows = QSETS[s], max(1, longest)
    worst_qpad = max(padded(q) for q in qlens)
    whole = rows * worst_qpad
    whole_fits = whole <= budget and whole <= SLOT_LIMIT
    assert p["whole_fits"] == int(whole_fits)
    # mode 2 takes the whole-matrix plan exactly when that plan fits; mode 1 never does, mode 0 always
    assert p["ckpt"] == int(mode == 1 or (mode == 2 and not whole_fits))
    admissible = [forced] if forced else [c for c in CANDIDATES if c >= FLOOR]
    size = (lambda n, qpad, B: slot_bytes(n, qpad, B)) if p["ckpt"] else (lambda n, qpad, B: max(1, n) * qpad)
    worst = min(size(rows, worst_qpad, c) for c in admissible)
    assert p["worst_qpad"] == worst_qpad and p["worst_bytes"] == worst
    assert p["fits"] == int(worst <= budget and worst <= SLOT_LIMIT)
    if not p["fits"]:
        assert p["groups"] == [] and p["launch"] == []
        return
    for g in p["groups"]:
        for k, c in enumerate(g["cls"]):
            if c["nq"] == 0:
                assert c["bound"] == []
                continue
            b = c["bound"]
            B = 1 << c["log_band"] if p["ckpt"] else 0
            assert (B in admissible) if p["ckpt"] else c["log_band"] == 0
            top_tier = min(size(rows, c["qpad"], x) for x in admissible)
            assert b[-1] == top_tier == size(rows, c["qpad"], B)          # the top tier: the class's worst case under the size function
            if p["ckpt"]:
                assert B == max(x for x in admissible if slot_bytes(rows, c["qpad"], x) == top_tier)
            assert 1 <= len(b) <= p["max_tiers"] and b == sorted(b) and len(set(b)) == len(b)   # tiers ascend
            for lo, hi in zip(b, b[1:]):
                assert lo == hi // p["tier_ratio"]
            assert len(b) == 1 or b[0] >= p["tier_floor"]
            assert len(b) == p["max_tiers"] or b[0] // p["tier_ratio"] < p["tier_floor"]
            mine = [padded(q) for q in qlens if (4 if q <= 256 else 8 if q <= 512 else 16) == (4, 8, 16)[k]]
            for qpad in mine:                                             # every item the class can get has a tier that holds it
                for n in {n for n in (1, 2, 64, 65, rows // 3 + 1, rows - 1, rows) if 1 <= n <= rows}:
                    assert size(n, qpad, B) <= b[-1]
    for l in p["launch"]:
        c = p["groups"][l["group"]]["cls"][l["kernel"]]
        assert l["slot_bytes"] == c["bound"][l["tier"]] and l["log_band"] == c["log_band"]
        assert 1 <= l["slots"] <= max(1, min(PER_CU[l["kernel"]] * 256 * 4, c["entries"]))
        assert l["slots"] * l["slot_bytes"] <= budget and l["slots"] * l["slot_bytes"] <= p["dir_need"]
        assert l["grid"] == (l["slots"] + 3) // 4
        if c["nstrips"] > 1 and p["ckpt"]:
            band = min(1 << l["log_band"], rows)
            assert 2 * (band + 70) <= l["bnd_per"] <= 2 * (band + 164)
            assert l["slots"] == 1 or l["slots"] * l["bnd_per"] * 4 <= BND_BYTES
            assert l["slots"] * l["bnd_per"] <= p["bnd_need"]
        elif c["nstrips"] == 1:
            assert l["bnd_per"] == 0


def test_one_long_record_no_longer_turns_the_call_off(driver):
    """64 queries of 512 against a database whose longest record has 5 M letters: refused whole, a few MB per slot checkpointed."""
    whole, ck = driver([f"what=hits qlens={','.join(['512'] * 64)} longest=5000000 mode={m} top=10 per_cu=5,4,2" for m in (0, 2)])
    assert (whole["ckpt"], whole["fits"]) == (0, 0)
    assert (ck["ckpt"], ck["fits"]) == (1, 1) and ck["worst_bytes"] == 512 * (8192 + 8 * 610) < 8 * MIB
