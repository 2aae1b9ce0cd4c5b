"""CPU: the host leg of the affine alignment (sw_align_affine_host) against the walk of the canonical alignment over the independent
checker's matrices (tests/align_cases.py over tests/affine_oracle.cpp), against the reference-generated paths of the fixtures, on
constructed gaps and ties; the argument rules; plan_align_affine.  No GPU is needed."""
import ctypes
import glob
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from affine_cases import GAPS, PROTEIN, ROOT, alphabets, checker, random_submat  # noqa: F401
from align_cases import expected, h_cells, indel_cases, pack, replay


def check_all(swamd, checker, query, targets, sub, go, ge, hits, what=""):  # noqa: F811
    packed, offs = pack(targets)
    aln, ops = swamd.align_affine_host(query, (packed, offs), sub, go, ge, hits)
    assert aln.shape == (len(hits), 7) and len(ops) == len(hits)
    memo = {}
    for h, k in enumerate(hits):
        if k not in memo:
            memo[k] = expected(checker, query, targets[k], sub, go, ge)
        row, eops, _ = memo[k]
        assert tuple(int(x) for x in aln[h]) == row, f"{what} hit {h} (target {k}, len {len(targets[k])}): {tuple(aln[h])} vs {row}"
        assert ops[h] == eops, f"{what} hit {h} (target {k}): ops differ"
        replay(query, targets[k], sub, go, ge, aln[h], ops[h])
    return aln, ops


@pytest.mark.parametrize("i,qlen", list(enumerate([1, 7, 64, 65, 130, 257])))
def test_exact_ops_against_the_rule(swamd, checker, i, qlen):  # noqa: F811
    rng = np.random.default_rng(900 + qlen)
    sub = random_submat(rng)
    for a in range(4):                                       # all four alphabets, every pair of GAPS
        qa, ta = alphabets(a)
        query = rng.choice(qa, qlen).astype(np.uint8)
        lens = [0, 1, 63, 64, 65] + list(rng.integers(2, 200, 5))
        targets = [rng.choice(ta, n).astype(np.uint8) for n in lens]
        # a target cut from the query with an indel, so that some alignments carry gaps whatever the alphabet
        if qlen >= 64:
            targets.append(np.concatenate([query[:30], query[34:]]))
            targets.append(np.concatenate([query[:40], rng.choice(ta, 3).astype(np.uint8), query[40:]]))
        hits = list(rng.permutation(len(targets))) + [2, 2, 0, len(targets) - 1]   # unordered, with duplicates
        for go, ge in GAPS:
            check_all(swamd, checker, query, targets, sub, go, ge, [int(h) for h in hits], f"qlen {qlen} alphabet {a} gaps {go, ge}")


FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "rand_*.npz"))) + [os.path.join(ROOT, "tests", "golden", "kat_builtin.npz")]


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_gap_open_zero_walks_the_reference_path(swamd, path):
    g = np.load(path)
    a, b, ref = g["a"], g["b"], [int(x) for x in g["path"]]
    aln, ops = swamd.align_affine_host(a, [b], swamd.submat_match(3, -3), 0, -2, [0])
    cols, rows, seed, maxpos, score, plen = (int(x) for x in g["meta"])
    assert plen == len(ref)
    assert (int(aln[0, 0]), int(aln[0, 1])) == (maxpos, score)
    assert int(aln[0, 6]) == plen == len(ops[0])
    assert h_cells(aln[0], ops[0], len(a)) == ref


def test_constructed_gaps_sit_where_they_were_built(swamd, checker):  # noqa: F811
    rng = np.random.default_rng(77)
    B = 150
    query = rng.choice(PROTEIN[:20], 300).astype(np.uint8)
    sub, go, ge, cases = indel_cases(swamd, rng, query, B, span=100)
    targets = [c[0] for c in cases]
    aln, ops = check_all(swamd, checker, query, targets, sub, go, ge, list(range(len(cases))), "indels")
    for k, (t, eops, score) in enumerate(cases):
        s, p, H, E, F = checker.matrices(query, t, sub, go, ge)
        assert s == score, f"case {k}: the best alignment is not the one built ({s} vs {score})"
        assert ops[k] == eops, f"case {k}: {ops[k]}"
        assert tuple(int(x) for x in aln[k, 2:6]) == (B - 100, 0, B + 100, len(t))


def test_tie_rule(swamd, checker):  # noqa: F811
    query = np.frombuffer(b"ACGT" * 40, np.uint8)
    targets = [np.frombuffer(s, np.uint8) for s in (b"ACGT" * 10, b"CGTA" * 12, b"ACG" * 30, b"ACGTT" * 20, b"GTAC" * 40, b"AACCGGTT" * 8)]
    seen, efties = set(), 0
    for (m, x), (go, ge) in [((1, 1), (0, 0)), ((2, 0), (-1, 0)), ((2, -1), (0, -1)), ((1, 0), (0, 0)), ((1, -1), (0, 0))]:
        sub = swamd.submat_match(m, x)
        _, ops = check_all(swamd, checker, query, targets, sub, go, ge, list(range(len(targets))), f"table {m, x} gaps {go, ge}")
        # the cases are ties: somewhere the diagonal equals E or F at a positive cell, and E equals F where neither is the diagonal's
        dtie = eftie = 0
        for t in targets:
            s, p, H, E, F = checker.matrices(query, t, sub, go, ge)
            D = H[:-1, :-1] + np.where(np.equal.outer(t, query), m, x)
            h, e, f = H[1:, 1:], E[1:, 1:], F[1:, 1:]
            dtie += int(((h > 0) & (h == D) & ((h == e) | (h == f))).sum())
            eftie += int(((h > 0) & (h == e) & (h == f)).sum())
        print(f"table {m, x} gaps {go, ge}: {dtie} diagonal ties, {eftie} E = F ties")
        assert dtie > 0
        efties += eftie
        seen |= set(b"".join(ops))
    assert seen == set(b"MID") and efties > 0


def test_argument_rules(swamd):
    L = swamd.lib()
    q = np.frombuffer(b"ACGTACGTAC", np.uint8).copy()
    db = np.frombuffer(b"ACGTTGCAAACCGGTT" * 4, np.uint8).copy()
    sub = swamd.submat_match(3, -3)
    cap = 32
    aln = np.zeros((4, 7), np.int64)
    ops = np.full((4, cap), 0x55, np.uint8)

    def call(hits=(1, 0), offs=(0, 5, 9), go=-3, ge=-1, hits_ptr=True, nhits=None, alnp=aln.ctypes.data, opsp=ops.ctypes.data, ops_cap=cap, qlen=10):
        o = np.array(offs, np.int64)
        h = np.array(hits, np.int64)
        sc = swamd._Affine(sub.ctypes.data, go, ge)
        return L.sw_align_affine_host(q.ctypes.data, qlen, db.ctypes.data, o.ctypes.data, len(o) - 1, h.ctypes.data if hits_ptr else None,
                                      len(h) if nhits is None else nhits, ctypes.byref(sc), alnp, opsp, ops_cap)

    assert call() == 0
    assert call(hits=(2,)) == -22 and b"out of range" in L.sw_last_error()
    assert call(hits=(-1,)) == -22
    assert call(hits_ptr=False) == -22 and b"hits" in L.sw_last_error()
    assert call(hits_ptr=False, nhits=0) == 0 and call(hits=(), nhits=0) == 0       # nothing to do
    assert call(alnp=None) == -22
    assert call(ops_cap=-1) == -22 and b"ops_cap" in L.sw_last_error()
    assert call(opsp=None, ops_cap=0) == 0                                            # coordinates only
    assert call(go=1) == -22 and call(qlen=0) == -22 and call(offs=(0, 5, 4)) == -22   # the search's own rules
    # nops > ops_cap: the true nops is reported, the neighbour's row stays as it was
    db2 = np.frombuffer(b"ACGTACGTAC" + b"ACGTAC", np.uint8).copy()
    o = np.array([0, 10, 16], np.int64)
    h = np.array([0, 1], np.int64)
    sc = swamd._Affine(sub.ctypes.data, -3, -1)
    ops[:] = 0x55
    assert L.sw_align_affine_host(q.ctypes.data, 10, db2.ctypes.data, o.ctypes.data, 2, h.ctypes.data, 2, ctypes.byref(sc), aln.ctypes.data,
                                  ops.ctypes.data, 6) == 0
    flat = ops.reshape(-1)
    assert aln[0, 6] == 10 and aln[1, 6] == 6
    assert flat[6:12].tobytes() == b"MMMMMM" and np.all(flat[12:] == 0x55)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the planner")
    exe = str(tmp_path_factory.mktemp("alplan") / "align_affine_plan")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "align_affine_plan_driver.cpp"),
                    os.path.join(ROOT, "smith-waterman_amd", "csrc", "sw_plan.cpp")], check=True)

    def run(**kw):
        kw = {"num_cus": 256, "per_cu": "5,4,2", "qlen": 512, "maxhit": 400, "nhits": 100, "budget_mib": 1024, **kw}
        line = " ".join(f"{k}={v}" for k, v in kw.items())
        return json.loads(subprocess.run([exe], input=line + "\n", capture_output=True, text=True, check=True).stdout)
    return run


def test_plan_align_affine(plan):
    # columns per lane on both sides of 256 and 512 columns; 16 only while its kernel keeps two workgroups per CU
    assert [plan(qlen=n)["C"] for n in (256, 257, 512, 513)] == [4, 8, 8, 16]
    assert [plan(qlen=n)["kernel"] for n in (256, 257, 513)] == [0, 1, 2]
    assert plan(qlen=513, per_cu="5,4,1")["C"] == 8
    # a slot: longest hit x padded query; the boundary column only beyond one strip
    p = plan(qlen=513, maxhit=700)
    assert (p["qpad"], p["slot_bytes"], p["bnd_per"]) == (1024, 700 * 1024, 0)
    assert plan(qlen=1025, maxhit=700)["bnd_per"] > 0 and plan(qlen=1025, maxhit=700)["qpad"] == 2048
    # slots = min(hits, resident waves, budget / slot); the grid holds them, four to a workgroup
    p = plan(qlen=512, maxhit=400, nhits=100)
    assert (p["slots"], p["grid"], p["dir_need"]) == (100, 25, 100 * 400 * 512)
    assert plan(nhits=100000)["slots"] == 4 * 256 * 4                         # resident waves of the 8-column kernel
    assert plan(nhits=100000, budget_mib=100)["slots"] == (100 << 20) // (400 * 512)
    assert plan(qlen=513, maxhit=700, nhits=40, budget_mib=1)["slots"] == 1   # fewer slots from a smaller budget
    assert plan(qlen=513, maxhit=500, nhits=40, budget_mib=1)["slots"] == 2
    assert plan(nhits=1)["grid"] == 1 and plan(nhits=5)["grid"] == 2
    # a single hit larger than the budget is refused, and so is one beyond a buffer descriptor
    assert plan(qlen=513, maxhit=1025, budget_mib=1)["fits"] == 0 and plan(qlen=513, maxhit=1024, budget_mib=1)["fits"] == 1
    assert plan(qlen=5000, maxhit=1 << 20, budget_mib=1 << 20)["fits"] == 0
    # the hits run longest first, ties in the caller's order
    assert plan(lens="5,9,0,9,7")["order"] == [1, 3, 4, 0, 2]
