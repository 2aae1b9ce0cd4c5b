"""CPU: the fill planner (smith-waterman_amd/csrc/sw_plan.cpp), built with g++ and driven through tests/fill_plan_driver.cpp.  Every
threshold of the policy from both sides, and the shapes whose plan the GPU tests see on the device (last_* options).

Device facts are the MI355X's: 256 CUs, workgroups dealt round-robin to the 8 XCDs, and ONE workgroup of sw_systolic2 per CU at 768
threads.  That occupancy is read from the code object's metadata (sw_systolic2<6, false>: 138 592 bytes of LDS against 160 KiB per
CU, 168 VGPRs), not measured here."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MI355X = {"num_cus": 256, "xcd_round_robin": 1, "s2_per_cu": 1}
NO_TILES, NO_TWO_COLUMNS, NO_SCOUTS, NO_XCD, NO_SPLIT, NO_PACING = 1 << 19, 1 << 14, 1 << 17, 1 << 23, 1 << 20, 1 << 27


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the planner")
    exe = str(tmp_path_factory.mktemp("plan") / "fill_plan")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "fill_plan_driver.cpp"),
                    os.path.join(ROOT, "smith-waterman_amd", "csrc", "sw_plan.cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def plan(driver):
    def run(**kw):
        line = " ".join(f"{k}={int(v) if isinstance(v, bool) else v}" for k, v in {**MI355X, **kw}.items())
        out = subprocess.run([driver], input=line + "\n", capture_output=True, text=True, check=True).stdout
        return json.loads(out)
    return run


def last(p):
    """what sw_get_option reports after the fill: last_strips2, last_scouts, last_xcd_mode, last_tiles, last_split_from"""
    t = p["tiles"][-1] if p["tiles"] else {"strips": 0, "nscout": 0, "xcd_mode": 0, "split_blk": 0}
    return t["strips"], t["nscout"], t["xcd_mode"], p["ntile"], t["split_from"] if t["split_blk"] else 0


def test_strips_per_workgroup_consumers_importers(plan):
    assert plan(cols=63 * 1152, rows=64)["NS"] == 1             # S <= 4.5 * CUs
    assert plan(cols=63 * 1152 + 1, rows=64)["NS"] == 2
    assert plan(cols=64, rows=64, npairs=256)["NS"] == 2        # a batch: S * npairs <= CUs
    assert plan(cols=63, rows=64, npairs=256)["NS"] == 1
    p = plan(cols=18708, rows=18708)                            # 3.5e8 cells: chain-bound
    assert (p["NC"], p["importers"], p["threads"]) == (4, 4, 768)
    p = plan(cols=18709, rows=18708)
    assert (p["NC"], p["importers"], p["threads"]) == (6, 2, 768)
    assert plan(cols=2000, rows=2000, consumers=5)["NC"] == 4   # no five-consumer one-column kernel
    assert plan(cols=2000, rows=2000, consumers=9)["NC"] == 7
    p = plan(cols=2000, rows=2000, strips_per_group=2, consumers=3)
    assert (p["NS"], p["NC"], p["threads"], p["two_cols"]) == (2, 3, 64 * 10, 0)
    assert plan(cols=63 * 300, rows=64, reserve_cus=16)["grid"] == 240
    assert plan(cols=63 * 300, rows=64, max_blocks=7)["grid"] == 7
    p = plan(cols=6400, rows=100, engine=1)                     # strip_scan
    assert (p["engine"], p["S"], p["grid"], p["threads"], p["two_cols"]) == (1, 100, 25, 256, 0)


def test_streaming_stores(plan):
    assert plan(cols=24494, rows=24494)["store_nt"] == 1        # 6.0e8 cells
    assert plan(cols=24495, rows=24495)["store_nt"] == 0
    assert plan(cols=24494, rows=24494, store_policy=1)["store_nt"] == 0
    assert plan(cols=24495, rows=24495, store_policy=2)["store_nt"] == 1
    assert plan(cols=1000, rows=1000, npairs=601)["store_nt"] == 0
    # per tile: 30000 x 30000 in two tiles of 15120 / 14880 columns (4.5e8 cells each), the whole matrix above the cut
    p = plan(cols=30000, rows=30000, s2w=126)
    assert p["store_nt"] == 0 and [t["store_nt"] for t in p["tiles"]] == [1, 1]
    p = plan(cols=30000, rows=30000, s2w=126, store_policy=1)
    assert p["ntile"] == 2 and [t["store_nt"] for t in p["tiles"]] == [0, 0]
    assert plan(cols=22000, rows=40)["tiles"][0]["store_nt"] == 1   # overlapping strips: whole lines streamed
    assert plan(cols=22000, rows=40, store_policy=1)["tiles"][0]["store_nt"] == 0


def test_perm_producer(plan):
    assert plan(cols=1000, rows=1000)["perm"] == 1
    assert plan(cols=1000, rows=1000, match=119, mismatch=-100, gap=-4)["perm"] == 1   # match - 2 gap = 127
    assert plan(cols=1000, rows=1000, match=120, mismatch=-100, gap=-4)["perm"] == 0
    assert plan(cols=1000, rows=1000, match=5, mismatch=-120, gap=-4)["perm"] == 1     # mismatch - 2 gap = -112
    assert plan(cols=1000, rows=1000, match=5, mismatch=-136, gap=-4)["perm"] == 0     # -128
    # every G value + 2^16 + 1024 below 2^24: 100 n + 10 (2 n + 2) < 2^24 - 66560
    n = (2 ** 24 - 0x10000 - 1024 - 20 - 1) // 120
    assert plan(cols=n, rows=n, match=100, mismatch=-100, gap=-10)["perm"] == 1
    assert plan(cols=n + 1, rows=n + 1, match=100, mismatch=-100, gap=-10)["perm"] == 0
    assert plan(cols=1000, rows=1000, has_top=1)["perm"] == 0                         # halo of unknown magnitude
    assert plan(cols=1000, rows=1000, has_top=1, total_rows=5000)["perm"] == 1
    assert plan(cols=1000, rows=1000, has_left=1)["perm"] == 0
    p = plan(cols=1000, rows=1000, debug_flags=16)
    assert p["perm"] == 0 and p["two_cols"] == 0 and p["edge4_need"] == 0
    assert plan(cols=1000, rows=1000)["e4stride"] == 1184 and plan(cols=1000, rows=1000)["edge4_need"] == 16 * 1184


def test_where_the_two_column_kernel_pays(plan):
    # P only, int8: the strip chain (3.1 us per strip) against 2 x the output volume at 3.2 TB/s
    assert plan(cols=6300, rows=78000, has_H=0, p_elem_bytes=1)["two_cols"] == 1
    assert plan(cols=6300, rows=79000, has_H=0, p_elem_bytes=1)["two_cols"] == 0
    # H only, int32: 0.5 x; and beyond 126 * 170 columns (even widths) always
    assert plan(cols=6300, rows=156000 // 2, has_P=0)["two_cols"] == 1
    assert plan(cols=6300, rows=80000, has_P=0)["two_cols"] == 0
    assert plan(cols=21420, rows=100000, has_P=0)["two_cols"] == 0
    assert plan(cols=21422, rows=100000, has_P=0)["two_cols"] == 1
    assert plan(cols=21420, rows=100000, p_elem_bytes=1)["two_cols"] == 0                # int32 H + int8 P
    assert plan(cols=21422, rows=100000, p_elem_bytes=1)["two_cols"] == 1
    assert plan(cols=6300, rows=200000, h_elem_bytes=8, p_elem_bytes=1)["two_cols"] == 1  # int64 H: always
    assert plan(cols=6300, rows=80000, has_P=0, debug_flags=1 << 15)["two_cols"] == 1


def test_two_column_exclusions(plan):
    assert plan(cols=1001, rows=304)["two_cols"] == 1                           # odd width: the base mode only
    assert plan(cols=1007, rows=304, h_elem_bytes=8)["two_cols"] == 0
    assert plan(cols=1001, rows=304, p_elem_bytes=1)["two_cols"] == 0
    assert plan(cols=1000, rows=304, p_elem_bytes=1)["two_cols"] == 1
    assert plan(cols=1000, rows=333, has_top_gran=1, has_bot_gran=1, total_rows=1000)["two_cols"] == 0   # a band's last row from a full block
    assert plan(cols=1000, rows=336, has_top_gran=1, has_bot_gran=1, total_rows=1000)["two_cols"] == 1
    assert plan(cols=1000, rows=333, has_top_gran=1, total_rows=1000)["two_cols"] == 1
    assert plan(cols=1000, rows=304, has_result=0)["two_cols"] == 0
    assert plan(cols=1000, rows=304, s2_per_cu=0)["two_cols"] == 0
    assert plan(cols=1000, rows=304, npairs=2)["two_cols"] == 0
    assert plan(cols=1000, rows=304, has_left=1, total_rows=304)["two_cols"] == 0
    assert plan(cols=1000, rows=304, has_right=1)["two_cols"] == 0
    assert plan(cols=1000, rows=304, full_stride=0)["two_cols"] == 0
    assert plan(cols=1000, rows=304, strips_per_group=1)["two_cols"] == 0
    assert plan(cols=1000, rows=304, consumers=3)["two_cols"] == 0
    assert plan(cols=1000, rows=304, consumers=4)["two_cols"] == 1
    for bit in (1, 3, 6, 7, 9, 14):
        assert plan(cols=1000, rows=304, debug_flags=1 << bit)["two_cols"] == 0, bit
    for bit in (0, 2, 5, 8, 10, 11, 12, 13):
        assert plan(cols=1000, rows=304, debug_flags=1 << bit)["two_cols"] == 1, bit


def test_strip_width(plan):
    assert plan(cols=21420, rows=64)["W2"] == 126                               # S126 = 170
    assert plan(cols=21421, rows=64)["W2"] == 110
    assert plan(cols=21421, rows=64, p_aligned=0)["W2"] == 126                  # no whole lines: no overlap
    assert plan(cols=21421, rows=64, h_aligned=0)["W2"] == 126
    assert plan(cols=18716, rows=64, h_elem_bytes=8)["W2"] == 126               # int64 H: S110 = 170
    assert plan(cols=18718, rows=64, h_elem_bytes=8)["W2"] == 110
    assert plan(cols=18717, rows=64)["W2"] == 126
    # one class of the HBM: from 2e8 cells, store probe ratio 1.7 and up
    assert plan(cols=14143, rows=14143, pair_ratio=1.7)["W2"] == 110
    assert plan(cols=14142, rows=14142, pair_ratio=1.7)["W2"] == 126
    assert plan(cols=14143, rows=14143, pair_ratio=1.69)["W2"] == 126
    assert plan(cols=14143, rows=14143)["W2"] == 126                            # unknown
    # option s2w
    assert plan(cols=22000, rows=64, s2w=126)["W2"] == 126
    assert plan(cols=1000, rows=64, s2w=110)["W2"] == 110
    assert plan(cols=1001, rows=64, s2w=110)["W2"] == 110                       # odd, but whole lines of int32 H + P
    assert plan(cols=1001, rows=64, s2w=110, p_aligned=0)["W2"] == 126
    assert plan(cols=1000, rows=64, s2w=110, has_top_gran=1, total_rows=640)["W2"] == 126   # bands keep 126


def test_column_tiles(plan):
    p = plan(cols=32768, rows=32768, s2w=126)
    assert (p["ntile"], p["tstrips"], [t["cols"] for t in p["tiles"]]) == (2, 131, [16506, 16262])
    assert plan(cols=35020, rows=35020, s2w=126)["ntile"] == 2                  # estimated 0.9797 x the untiled time
    assert plan(cols=35080, rows=35080, s2w=126)["ntile"] == 1                  # 0.9802 x: not 2 % faster
    assert plan(cols=49152, rows=49152, s2w=126)["ntile"] == 1
    assert plan(cols=21420, rows=64, s2w=126)["ntile"] == 1                     # 170 strips
    assert plan(cols=21421, rows=64, s2w=126)["ntile"] == 2
    assert plan(cols=21421, rows=64)["ntile"] == 1                              # the library's own overlap: one launch
    assert plan(cols=21421, rows=64, s2w=110)["ntile"] == 2                     # forced overlap tiles as well
    assert plan(cols=21421, rows=64, s2w=126, debug_flags=NO_TILES)["ntile"] == 1
    assert plan(cols=21422, rows=64, s2w=126, p_elem_bytes=1)["ntile"] == 1     # not the base mode
    assert plan(cols=21422, rows=64, s2w=126, has_top_gran=1, total_rows=640)["two_cols"] == 1   # nor a band
    assert plan(cols=21422, rows=64, s2w=126, has_top_gran=1, total_rows=640)["ntile"] == 1


def test_scouts_and_roles_per_xcd(plan):
    def at(strips, **kw):   # 126-column strips, one launch
        return plan(cols=126 * strips, rows=64, s2w=126, debug_flags=kw.pop("debug_flags", 0) | NO_TILES, **kw)["tiles"][0]
    assert at(3)["nscout"] == 0 and at(4)["nscout"] == 3 and at(4)["grid"] == 7
    t = at(171)                                                                 # 2 x doubles <= S2 - 1
    assert (t["nscout"], t["scout_double"], t["grid"], t["xcd_mode"]) == (85, 85, 256, 0)
    assert at(172)["nscout"] == 0 and at(172)["grid"] == 172
    assert at(100, debug_flags=NO_SCOUTS)["nscout"] == 0
    assert at(15)["xcd_mode"] == 0 and at(16)["xcd_mode"] == 1 and at(16)["grid"] == 256
    assert at(168)["xcd_mode"] == 1 and at(169)["xcd_mode"] == 0                # the scouts of an XCD no longer fit
    assert at(100, xcd_round_robin=0)["xcd_mode"] == 0
    assert at(100, max_blocks=255)["xcd_mode"] == 0                             # needs 256 workgroups
    assert at(100, debug_flags=NO_XCD)["xcd_mode"] == 0
    # the classic chain dealt per XCD: from 384 strips of 126 columns, or with option xcd_chain
    assert at(383)["xcd_mode"] == 0 and at(384)["xcd_mode"] == 2
    assert at(384, xcd_chain=2)["xcd_mode"] == 0 and at(200, xcd_chain=1)["xcd_mode"] == 2
    assert at(384, debug_flags=NO_XCD)["xcd_mode"] == 0
    assert plan(cols=110 * 400, rows=64, s2w=110, debug_flags=NO_TILES)["tiles"][0]["xcd_mode"] == 0   # not for overlapping strips
    assert at(200, xcd_chain=1, max_blocks=63)["xcd_mode"] == 0                 # grid >= 64


def test_split_strips(plan):
    t = plan(cols=8192, rows=8192)["tiles"][0]
    assert (t["strips"], t["xcd_mode"], t["split_blk"], t["split_from"], t["split_extra"]) == (66, 1, 449, 56, 1)
    assert (t["filler_end_steps"], t["filler_full_steps"], t["filler_hop_ps"]) == (7360, 8320, 2400000)
    assert plan(cols=8192, rows=4096)["tiles"][0]["split_blk"] == 224
    assert plan(cols=8192, rows=4080)["tiles"][0]["split_blk"] == 0              # rows >= 4096
    assert plan(cols=8192, rows=8192, filler_tau_ps=21500)["tiles"][0]["split_blk"] == 0   # tau <= scout lead: sblk = nblk
    assert plan(cols=8192, rows=4096, filler_tau_ps=21700)["tiles"][0]["split_blk"] == 0   # the split block ends as late: from = S2
    assert plan(cols=8192, rows=4096, filler_tau_ps=22000)["tiles"][0]["split_from"] == 65   # S2 = 66
    for flags in (NO_SPLIT, NO_PACING):
        assert plan(cols=8192, rows=8192, debug_flags=flags)["tiles"][0]["split_blk"] == 0
    assert plan(cols=8192, rows=8192, debug_flags=NO_PACING)["tiles"][0]["filler_hop_ps"] == 0
    assert plan(cols=8192, rows=8192, filler_hop_ps=0)["tiles"][0]["split_blk"] == 0
    assert plan(cols=8192, rows=8192, debug_flags=NO_XCD)["tiles"][0]["split_blk"] == 0
    # forced: any split block below the last, any first strip
    t = plan(cols=126 * 40, rows=333, s2w=126, split_blk=3, split_from=1)["tiles"][0]
    assert (t["split_blk"], t["split_from"], t["filler_end_steps"], t["filler_full_steps"]) == (3, 1, 192, 512)
    assert plan(cols=126 * 40, rows=333, split_blk=20)["tiles"][0]["split_blk"] == 20
    assert plan(cols=126 * 40, rows=333, split_blk=21)["tiles"][0]["split_blk"] == 0   # below nblk = 21
    assert plan(cols=126 * 40, rows=333, split_blk=3, split_from=0)["tiles"][0]["split_from"] == 1


def test_two_column_consumers(plan):
    assert plan(cols=2000, rows=2000)["tiles"][0]["consumers"] == 7              # behind scouts
    assert plan(cols=22000, rows=64)["tiles"][0]["consumers"] == 7               # overlapping strips
    assert plan(cols=126 * 200, rows=64, s2w=126, debug_flags=NO_TILES)["tiles"][0]["consumers"] == 5   # chain-bound classic chain
    assert plan(cols=126 * 200, rows=20000, s2w=126, debug_flags=NO_TILES)["tiles"][0]["consumers"] == 6
    assert plan(cols=2000, rows=2000, consumers=5)["tiles"][0]["consumers"] == 5
    assert plan(cols=2000, rows=2000, consumers=8)["tiles"][0]["consumers"] == 7


def test_probe_of_foreign_pairs(plan):
    n = 14143   # 2e8 cells
    assert plan(cols=n, rows=n, probe_foreign_pairs=1)["probe_pair_class"] == 1
    assert plan(cols=n - 1, rows=n - 1, probe_foreign_pairs=1)["probe_pair_class"] == 0
    assert plan(cols=n, rows=n)["probe_pair_class"] == 0
    assert plan(cols=n, rows=n, probe_foreign_pairs=1, pair_ratio=1.4)["probe_pair_class"] == 0
    assert plan(cols=n, rows=n, probe_foreign_pairs=1, s2w=126)["probe_pair_class"] == 0
    assert plan(cols=n, rows=n, probe_foreign_pairs=1, p_aligned=0)["probe_pair_class"] == 0
    assert plan(cols=21420, rows=10000, probe_foreign_pairs=1)["probe_pair_class"] == 1   # S126 = 170
    assert plan(cols=21421, rows=10000, probe_foreign_pairs=1)["probe_pair_class"] == 0
    assert plan(cols=n, rows=n, probe_foreign_pairs=1, has_P=0)["probe_pair_class"] == 0
    # what the probe is told: the real sizes of both matrices (an int8 P is a quarter of an int32 one)
    p = plan(cols=40000, rows=40000, p_elem_bytes=1, probe_foreign_pairs=1)
    assert p["probe_pair_class"] == 0 and (p["h_bytes"], p["p_bytes"]) == (40001 ** 2 * 4, 40001 ** 2)
    p = plan(cols=20000, rows=20000, p_elem_bytes=1, probe_foreign_pairs=1)
    assert p["probe_pair_class"] == 1 and (p["h_bytes"], p["p_bytes"]) == (20001 ** 2 * 4, 20001 ** 2)


def test_workspaces(plan):
    p = plan(cols=1000, rows=1000)
    assert p["edge_need"] == 16 * 1001 and p["cb_need"] == 1648 and p["priv_need"] == 3328 * 256
    p = plan(cols=1000, rows=1000, npairs=3)
    assert (p["edge_need"], p["cb_need"], p["edge4_need"], p["priv_need"]) == (3 * 16 * 1001, 3 * 1648, 3 * 16 * 1184, 0)
    p = plan(cols=1000, rows=1000, engine=1)
    assert (p["edge_need"], p["cb_need"], p["edge4_need"], p["priv_need"]) == (16 * 1001, 0, 0, 0)


@pytest.mark.parametrize("kw,want", [
    # (tests/test_overlap_strips_gpu.py: the library's choice beyond the scouts) -> (last_strips2, last_scouts, last_xcd_mode, last_tiles)
    ({"cols": 22000, "rows": 50}, (200, 0, 0, 1)), ({"cols": 22000, "rows": 50, "h_elem_bytes": 8}, (200, 0, 0, 1)),
    ({"cols": 21560, "rows": 17}, (196, 0, 0, 1)),
    ({"cols": 20000, "rows": 40, "h_elem_bytes": 8}, (182, 0, 0, 1)), ({"cols": 20000, "rows": 40}, (159, 97, 1, 1)),
    ({"cols": 22001, "rows": 40}, (200, 0, 0, 1)), ({"cols": 22001, "rows": 40, "p_elem_bytes": 1}, (0, 0, 0, 1)),
    ({"cols": 22000, "rows": 40, "p_elem_bytes": 1}, (200, 0, 0, 1)), ({"cols": 22000, "rows": 40, "p_elem_bytes": 1, "has_H": 0}, (175, 0, 0, 1)),
    # (test_two_columns_gpu.py)
    ({"cols": 9000, "rows": 1600, "max_blocks": 7}, (72, 0, 0, 1)), ({"cols": 9000, "rows": 1600, "debug_flags": NO_TWO_COLUMNS}, (0, 0, 0, 1)),
    ({"cols": 40000, "rows": 4096, "s2w": 126, "debug_flags": NO_TILES}, (318, 0, 0, 1)), ({"cols": 40000, "rows": 4096, "s2w": 126}, (159, 97, 1, 2)),
    ({"cols": 1260, "rows": 333, "h_elem_bytes": 8}, (10, 9, 0, 1)), ({"cols": 1007, "rows": 304, "h_elem_bytes": 8}, (0, 0, 0, 1)),
    # (test_column_tiles_gpu.py, test_xcd_roles_gpu.py)
    ({"cols": 30000, "rows": 2000, "s2w": 126}, (119, 118, 1, 2)), ({"cols": 35000, "rows": 300, "s2w": 126}, (139, 117, 1, 2)),
    ({"cols": 126 * 15, "rows": 64}, (15, 14, 0, 1)), ({"cols": 126 * 16, "rows": 64}, (16, 15, 1, 1)), ({"cols": 126 * 167, "rows": 64}, (167, 89, 1, 1)),
    ({"cols": 126 * 200, "rows": 64, "s2w": 126}, (100, 99, 1, 2)), ({"cols": 126 * 200, "rows": 64, "s2w": 126, "debug_flags": NO_TILES}, (200, 0, 0, 1)),
    ({"cols": 126 * 200, "rows": 64}, (229, 0, 0, 1)), ({"cols": 126 * 64 - 5, "rows": 272, "debug_flags": NO_XCD}, (64, 63, 0, 1)),
])
def test_plans_the_gpu_tests_see(plan, kw, want):
    assert last(plan(**kw))[:4] == want


def test_split_plans_the_gpu_tests_see(plan):
    assert last(plan(cols=8192, rows=8192))[4] > 0 and last(plan(cols=8192, rows=8192, debug_flags=NO_SPLIT))[4] == 0
    for strips, rows, blk, frm in ((40, 333, 3, 1), (131, 272, 9, 100), (64, 1000, 40, 30)):
        p = plan(cols=126 * strips - strips % 3, rows=rows, s2w=126, split_blk=blk, split_from=frm)
        assert last(p)[2] == 1 and last(p)[4] == frm
    assert last(plan(cols=110 * 60, rows=400, s2w=110, split_blk=7, split_from=1))[4] == 1
    assert last(plan(cols=30000, rows=600, s2w=110))[3] >= 2
