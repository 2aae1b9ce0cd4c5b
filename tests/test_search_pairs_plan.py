"""CPU: the planner of the pair-list search (swp::plan_search_pairs, smith-waterman_amd/csrc/sw_plan.cpp), built with g++ and driven
through tests/search_pairs_plan_driver.cpp: the query table and the groups against plan_search_multi's, the chunks of the list, the
launches of a (chunk, group), their grids and boundary workspaces, the weight buckets and the item workspace.  Occupancies are given,
not measured: 3 workgroups per CU unless a case says otherwise."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = 257                      # profile rows (swk::SW_SEARCH_ROWS)
MIB = 1 << 20
DEFAULT_CHUNK = 1 << 22
MIXED = [1, 4, 255, 256, 257, 512, 513, 1024, 1025, 2049]


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the planner")
    exe = str(tmp_path_factory.mktemp("plan") / "search_pairs_plan")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "search_pairs_plan_driver.cpp"),
                    os.path.join(ROOT, "smith-waterman_amd", "csrc", "sw_plan.cpp")], check=True)

    def run(qlens, **kw):
        kw = {"longest": 400, "npairs": 1000, **kw}
        line = "qlens=" + ",".join(str(q) for q in qlens) + " " + " ".join(f"{k}={v}" for k, v in kw.items())
        return json.loads(subprocess.run([exe], input=line + "\n", capture_output=True, text=True, check=True).stdout)
    return run


@pytest.mark.parametrize("qlens,kw", [
    (MIXED, {}),
    ([2049, 4, 300, 1, 600, 256, 512], {}),
    ([512] * 20, {"budget_bytes": MIB}),
    ([100, 5000, 100], {"budget_bytes": MIB}),
    ([512, 513, 2049], {"per_cu": "5,4,1"}),                      # 16 columns per lane below two workgroups per CU: the long queries run at 8
    (MIXED + [8, 8, 8, 700, 300], {"budget_bytes": MIB, "per_cu": "5,4,1"}),
])
def test_table_and_groups_are_those_of_the_many_query_search(plan, qlens, kw):
    p = plan(qlens, **kw)
    assert p["table"] == p["multi_table"] and len(p["table"]) == len(qlens)
    assert [[g["q0"], g["nq"], g["prof_bytes"]] for g in p["groups"]] == p["multi_groups"]
    assert p["prof_need"] == p["multi_prof_need"]
    # entry_of is the inverse of the table's rows; a group's classes tile its entries in order, each of one width
    assert [p["table"][t][2] for t in p["entry_of"]] == list(range(len(qlens)))
    for g in p["groups"]:
        c = g["cls_q0"]
        assert c[0] == g["q0"] and c[3] == g["q0"] + g["nq"] and c == sorted(c)
        for k in range(3):
            for t in range(c[k], c[k + 1]):
                _, _, _, qlen, qpad, nstrips = p["table"][t]
                assert qpad // nstrips // 64 == (4, 8, 16)[k] and qpad >= qlen


def chunks_of(plan, npairs, chunk, which):
    p = plan([8], npairs=npairs, **({} if chunk is None else {"chunk": chunk}), chunks=",".join(str(i) for i in which))
    return p, p["chunk_at"]


@pytest.mark.parametrize("npairs,chunk", [(150, 1), (150, 64), (128, 64), (64, 64), (1, 64), (150, None), (DEFAULT_CHUNK, None),
                                          (3 * DEFAULT_CHUNK, None), (3 * DEFAULT_CHUNK + 1, None)])
def test_chunks_tile_the_list(plan, npairs, chunk):
    size = DEFAULT_CHUNK if chunk is None else chunk
    n = -(-npairs // size)
    which = list(range(n)) if n <= 200 else [0, 1, n - 2, n - 1]
    p, at = chunks_of(plan, npairs, chunk, which)
    assert p["chunk"] == size and p["nchunks"] == n
    assert at[0][0] == 0 and at[-1][0] + at[-1][1] == npairs                                # from the first pair to the last
    for i, (p0, np_) in zip(which, at):
        assert p0 == i * size and 1 <= np_ <= size and np_ == min(size, npairs - p0)       # no gap, no overlap, never above the chunk size
    assert all(np_ == size for _, np_ in at[:-1])
    assert p["last_chunk_pairs"] == at[-1][1]


def test_chunks_of_a_list_beyond_two_to_the_31_by_arithmetic(plan):
    npairs = (1 << 31) + 5
    for size, n in ((DEFAULT_CHUNK, 513), ((1 << 31) - 1, 2), (1, npairs), (64, (1 << 25) + 1)):
        p, at = chunks_of(plan, npairs, size, [0, 1, n - 2, n - 1])
        assert p["nchunks"] == n
        assert [a[0] for a in at] == [0, size, (n - 2) * size, (n - 1) * size]
        assert at[0][1] == size and at[-2][1] == size and at[-1][1] == npairs - (n - 1) * size >= 1
        assert (n - 1) * size + at[-1][1] == npairs
        assert p["items_need"] == 24 * size                                                 # the workspace follows the chunk, not the list
    assert plan([8], npairs=npairs, chunk=1 << 40)["chunk"] == (1 << 31) - 1                # every counter stays inside 32 bits


def test_one_score_launch_per_class_present(plan):
    p = plan(MIXED, npairs=150)
    assert [(l["group"], l["C"], l["kernel"], l["q0"], l["nq"]) for l in p["launches"]] == [(0, 4, 0, 0, 4), (0, 8, 1, 4, 2), (0, 16, 2, 6, 4)]
    assert p["nchunks"] == 1 and p["launches_total"] == 1 + 2 + 3                           # profile, count, scatter, three classes
    p = plan([8, 300], npairs=150, chunk=64)                                                # two classes, three chunks
    assert [l["C"] for l in p["launches"]] == [4, 8] and p["nchunks"] == 3 and p["launches_total"] == 1 + 3 * (2 + 2)
    p = plan([100, 5000, 100], npairs=10, budget_bytes=MIB)                                 # three groups of one class each
    assert [(l["group"], l["C"]) for l in p["launches"]] == [(0, 4), (1, 16), (2, 4)] and p["launches_total"] == 3 + 3 * 2 + 3
    p = plan(MIXED, npairs=150, chunk=64, budget_bytes=MIB)
    per_group = [sum(1 for l in p["launches"] if l["group"] == g) for g in range(len(p["groups"]))]
    for g, grp in enumerate(p["groups"]):
        c = grp["cls_q0"]
        assert per_group[g] == sum(1 for k in range(3) if c[k + 1] > c[k])
    assert p["launches_total"] == len(p["groups"]) + 3 * (2 * len(p["groups"]) + len(p["launches"]))
    assert plan(MIXED, npairs=0)["nchunks"] == 0


def test_grid_is_the_lesser_of_the_resident_waves_and_the_pairs_of_the_chunk(plan):
    for npairs, chunk, per_cu in [(1, None, "3"), (5, None, "3"), (150, 64, "3"), (3071, None, "3"), (3072, None, "3"), (3073, None, "3"),
                                  (10 ** 6, None, "6,5,3"), (10 ** 6, 1000, "6,5,3")]:
        p = plan([8, 300, 600], npairs=npairs, per_cu=per_cu, **({} if chunk is None else {"chunk": chunk}))
        pcs = [int(x) for x in per_cu.split(",")] * (3 if "," not in per_cu else 1)
        full, last = min(npairs, p["chunk"]), p["last_chunk_pairs"]
        for l in p["launches"]:
            resident = 4 * pcs[l["kernel"]] * 256                                           # waves: four per workgroup, 256 CUs
            assert l["bnd_per"] == 0 and l["max_grid"] == resident // 4
            assert l["grid_full"] == -(-min(resident, full) // 4) and l["grid_last"] == -(-min(resident, last) // 4)
            assert 1 <= l["grid_last"] <= l["grid_full"]


def test_boundary_workspace_only_for_a_class_with_a_multi_strip_query(plan):
    p = plan([100, 400, 1024, 1025], longest=1100, npairs=50)
    l4, l8, l16 = p["launches"]
    assert l4["bnd_per"] == 0 and l8["bnd_per"] == 0
    assert l16["bnd_per"] == 2 * ((1100 + 160 + 3) // 4 * 4)           # H and F per row, sized by the handle's longest target
    assert p["bnd_need"] == l16["grid_full"] * 4 * l16["bnd_per"] and l16["grid_full"] == 13
    assert plan([100, 400, 1024], longest=1100, npairs=50)["bnd_need"] == 0
    p = plan([512, 513], longest=1100, npairs=50, per_cu="5,4,1")      # 513 at 8 columns per lane: two strips in the 8-column class
    assert [(l["C"], l["bnd_per"] > 0) for l in p["launches"]] == [(8, True)]


def test_bucket_is_the_floor_of_the_binary_logarithm_of_the_weight(plan):
    top = (1 << 20) - 1
    edges = [(1, 256), (top, 256), (1, 1 << 20), (top, 1 << 20)]
    ramp = [(1, 256), (2, 256), (3, 256), (4, 256), (5, 512), (63, 1024), (64, 1024), (1100, 3072), (4336, 512), (35000, 512), (top, 3072)]
    p = plan([8], buckets=",".join(f"{a}:{b}" for a, b in edges + ramp))
    assert p["buckets"][:4] == [8, 27, 20, 39]
    assert all(0 <= b < 41 for b in p["buckets"])
    got = dict(zip(edges + ramp, p["buckets"]))
    for (a, b), bucket in got.items():
        assert 1 << bucket <= a * b < 1 << (bucket + 1)
    order = sorted(got, key=lambda ab: ab[0] * ab[1])
    assert [got[x] for x in order] == sorted(got[x] for x in order)     # monotone in len x qpad


def test_item_workspace(plan):
    for npairs, chunk, want in [(150, None, 150), (150, 64, 64), (0, None, 0), (DEFAULT_CHUNK + 1, None, DEFAULT_CHUNK), (64, 64, 64)]:
        assert plan([8], npairs=npairs, **({} if chunk is None else {"chunk": chunk}))["items_need"] == 24 * want
