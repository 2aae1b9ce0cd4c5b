"""CPU: the affine search's host leg (sw_search_affine_host) against the independent checker (tests/affine_oracle.cpp) and, with
gap_open = 0 and the match table, against the reference-pinned linear oracle; the matrix builders and reader; the argument rules;
plan_search_affine over its thresholds; the ISA audit of the affine kernels.  No GPU is needed."""
import ctypes
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from affine_cases import ALL_BYTES, DNA, GAPS, PROTEIN, ROOT, alphabets, assert_same, checker, database, random_submat  # noqa: F401

SCORINGS = [(3, -3, -2), (5, -3, -4), (1, 1, 0), (2, 0, -1)]   # those of tests/test_search_gpu.py


@pytest.mark.parametrize("i,qlen", list(enumerate([1, 7, 64, 65, 130, 257, 300, 513])))
def test_host_leg_matches_checker(swamd, checker, i, qlen):  # noqa: F811
    rng = np.random.default_rng(500 + qlen)
    qa, ta = alphabets(i)
    query = rng.choice(qa, qlen).astype(np.uint8)
    packed, offs = database(rng, qlen, ta, budget=2e6)       # empty, 1-letter targets, offsets[0] = 7
    assert offs[0] % 2 == 1 and 0 in np.diff(offs) and 1 in np.diff(offs)
    sub = random_submat(rng)
    assert not np.array_equal(sub, sub.T)
    for go, ge in GAPS:
        res = swamd.search_affine_host(query, (packed, offs), sub, go, ge)
        assert_same(res, checker.search(query, packed, offs, sub, go, ge), f"qlen {qlen} go {go} ge {ge}")
        assert np.all(res[np.diff(offs) == 0] == 0)


@pytest.mark.parametrize("scores", SCORINGS)
def test_gap_open_zero_with_match_table_is_the_linear_search(swamd, oracle, scores):
    match, mismatch, gap = scores
    rng = np.random.default_rng(match * 10 - gap)
    sub = swamd.submat_match(match, mismatch)
    for i, qlen in enumerate([5, 64, 200, 300]):
        qa, ta = alphabets(i)
        query = rng.choice(qa, qlen).astype(np.uint8)
        packed, offs = database(rng, qlen, ta, budget=1e6)
        res = swamd.search_affine_host(query, (packed, offs), sub, 0, gap)
        for k in range(len(offs) - 1):
            t = packed[offs[k]:offs[k + 1]]
            if len(t) == 0:
                assert tuple(res[k]) == (0, 0, 0)
                continue
            o = oracle.fill_streaming(query, t, scores)
            assert (res[k, 1], res[k, 0], res[k, 2]) == (o["max_score"], o["max_pos"], 0), f"target {k} (len {len(t)})"


def test_submat_builders(swamd):
    s = swamd.submat_match(5, -4)
    assert s.shape == (256, 256) and s.dtype == np.int8
    assert np.all(np.diag(s) == 5) and s.sum() == 256 * 5 - 4 * (65536 - 256)
    sc = np.array([[4, -1, -2], [0, 5, -3], [7, 1, 6]], np.int8)
    t = swamd.submat_from_letters(b"AC\x00", sc, -9)
    assert t[ord("A"), ord("C")] == -1 and t[ord("C"), ord("A")] == 0 and t[0, ord("A")] == 7 and t[0, 0] == 6
    assert t[ord("G"), ord("A")] == -9 and t[ord("A"), ord("G")] == -9 and t[255, 255] == -9
    assert (t != -9).sum() == 9
    with pytest.raises(swamd.SwError):
        swamd.submat_from_letters(b"AA", np.zeros((2, 2), np.int8), 0)      # a letter twice
    with pytest.raises(swamd.SwError):
        swamd.submat_from_letters(b"AC", np.zeros((2, 2), np.int8), 300)    # other beyond int8


MATRIX_TEXT = """# a comment line
#   another, then a blank line

   A  r  N  *
A  4 -1 -2 -4
R -1  5  0 -4

# a comment between the rows
n -2  0  6 -4
* -4 -4 -4  1
"""


def test_read_submat_round_trip(swamd, tmp_path):
    p = tmp_path / "m.txt"
    p.write_text(MATRIX_TEXT)
    s = swamd.read_submat(str(p))
    exp = np.full((256, 256), -4, np.int8)                  # other = the smallest entry
    letters = b"ARN*"
    vals = [[4, -1, -2, -4], [-1, 5, 0, -4], [-2, 0, 6, -4], [-4, -4, -4, 1]]
    for a, row in zip(letters, vals):
        for b, v in zip(letters, row):
            exp[a, b] = v
    assert np.array_equal(s, exp)
    assert s[ord("r"), ord("r")] == -4                      # lower case in the FILE is upper-cased; the byte 'r' itself is unlisted
    # a written file reads back: random asymmetric scores over the protein letters, rows in another order than the header
    rng = np.random.default_rng(1)
    n = len(PROTEIN)
    sc = rng.integers(-128, 128, (n, n)).astype(np.int8)
    order = rng.permutation(n)
    text = "# generated\n  " + " ".join(chr(c) for c in PROTEIN) + "\n"
    text += "".join(chr(PROTEIN[r]) + " " + " ".join(str(v) for v in sc[r]) + "\r\n" for r in order)
    q = tmp_path / "w.txt"
    q.write_text(text)
    assert np.array_equal(swamd.read_submat(str(q)), swamd.submat_from_letters(PROTEIN, sc, int(sc.min())))


@pytest.mark.parametrize("text,what", [
    ("A C\nA 1 2\nC 1\n", b"entries"),                      # ragged row
    ("A C\nA 1 2 3\nC 1 2\n", b"entries"),
    ("A C\nA 1 200\nC 1 2\n", b"int8"),
    ("A C\nA 1 -129\nC 1 2\n", b"int8"),
    ("A C\nA 1 2\n", b"rows"),
    ("A C\nA 1 2\nG 1 2\n", b"header"),
    ("A C\nA 1 x\nC 1 2\n", b"integer"),
    ("# nothing\n", b"header"),
])
def test_read_submat_rejects(swamd, tmp_path, text, what):
    p = tmp_path / "bad.txt"
    p.write_text(text)
    out = np.zeros((256, 256), np.int8)
    L = swamd.lib()
    assert L.sw_read_submat(os.fsencode(str(p)), out.ctypes.data) == -22
    assert what in L.sw_last_error(), L.sw_last_error()
    assert L.sw_read_submat(os.fsencode(str(tmp_path / "missing.txt")), out.ctypes.data) == -22


def test_argument_rules(swamd):
    L = swamd.lib()
    q = np.frombuffer(b"ACGTACGTAC", np.uint8).copy()
    db = np.frombuffer(b"ACGTTGCAAACCGGTT" * 4, np.uint8).copy()
    res = np.zeros((4, 3), np.int64)
    sub = swamd.submat_match(3, -3)

    def call(qlen=10, offs=(0, 5, 9), go=-3, ge=-1, table=sub, qp=q.ctypes.data, dbp=db.ctypes.data, rp=res.ctypes.data, offs_ptr=True, n=None,
             scoring=True):
        o = np.array(offs, np.int64)
        sc = swamd._Affine(table.ctypes.data if table is not None else None, go, ge)
        return L.sw_search_affine_host(qp, qlen, dbp, o.ctypes.data if offs_ptr else None, len(o) - 1 if n is None else n,
                                       ctypes.byref(sc) if scoring else None, rp)

    assert call() == 0
    assert call(qp=None) == -22 and call(dbp=None) == -22 and call(rp=None) == -22 and call(offs_ptr=False) == -22
    assert call(scoring=False) == -22 and call(table=None) == -22 and call(n=-1) == -22
    assert call(offs=(0, 5, 4)) == -22 and b"decrease" in L.sw_last_error()
    assert call(offs=(-1, 5)) == -22
    assert call(qlen=0) == -22 and call(qlen=1 << 20) == -22
    assert call(go=1) == -22 and b"gap_open" in L.sw_last_error()
    assert call(ge=1) == -22 and b"gap_extend" in L.sw_last_error()
    assert call(go=-(1 << 24), ge=0) == 0
    assert call(go=-(1 << 24), ge=-1) == -22 and b"2^24" in L.sw_last_error()
    assert call(go=-(1 << 23), ge=-(1 << 23) - 1) == -22
    # 24-bit score of the key: largest entry x min(qlen, longest target); the message names the entry
    big = swamd.submat_match(3, -3)
    big[ord("G"), ord("T")] = 127
    lo = -(-(1 << 24) // 127)                                # the first min(qlen, longest target) that reaches 2^24 with 127
    qbig = np.zeros(lo, np.uint8)
    dbig = np.zeros(lo, np.uint8)
    assert call(qlen=lo, offs=(0, 3, 3, 4), table=big, qp=qbig.ctypes.data, dbp=dbig.ctypes.data) == 0      # short targets: far below
    assert call(qlen=lo, offs=(0, 3, lo + 3), table=big, qp=qbig.ctypes.data, dbp=dbig.ctypes.data) == -22  # (rejected before any cell)
    assert b"s[71][84] = 127" in L.sw_last_error(), L.sw_last_error()
    assert call(qlen=lo, offs=(0, lo), table=sub, qp=qbig.ctypes.data, dbp=dbig.ctypes.data, n=0) == 0      # no targets: nothing to bound
    neg = np.full((256, 256), -5, np.int8)                   # nothing positive: max(entry, 0) = 0, any length goes
    assert call(qlen=10, offs=(0, 64), table=neg) == 0 and np.all(res[0] == 0)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the planner")
    exe = str(tmp_path_factory.mktemp("aplan") / "search_affine_plan")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "search_affine_plan_driver.cpp"),
                    os.path.join(ROOT, "smith-waterman_amd", "csrc", "sw_plan.cpp")], check=True)

    def run(**kw):
        kw = {"num_cus": 256, "per_cu": "6,5,3", "qlen": 512, "maxlen": 400, "ntargets": 100000, **kw}
        line = " ".join(f"{k}={v}" for k, v in kw.items())
        return json.loads(subprocess.run([exe], input=line + "\n", capture_output=True, text=True, check=True).stdout)
    return run


def test_plan_search_affine_thresholds(plan):
    # columns per lane by query length, as the linear search ...
    assert (plan(qlen=256)["C"], plan(qlen=257)["C"], plan(qlen=512)["C"], plan(qlen=513)["C"]) == (4, 8, 8, 16)
    assert [plan(qlen=n)["kernel"] for n in (1, 300, 5000)] == [0, 1, 2]
    # ... but 16 only while its kernel keeps two workgroups per CU
    assert plan(qlen=513, per_cu="6,5,2")["C"] == 16 and plan(qlen=513, per_cu="6,5,1")["C"] == 8
    assert plan(qlen=256, per_cu="6,5,1")["C"] == 4
    # strips and the padded profile row
    p = plan(qlen=1024)
    assert (p["nstrips"], p["qpad"], p["prof_need"]) == (1, 1024, 257 * 1024)
    p = plan(qlen=1025)
    assert (p["nstrips"], p["qpad"]) == (2, 2048)
    p = plan(qlen=513, per_cu="6,5,1")
    assert (p["nstrips"], p["qpad"]) == (2, 1024)
    # boundary column: none for one strip, two ints (H, F) per row of the longest target + slack otherwise
    assert plan(qlen=1024, maxlen=3000)["bnd_per"] == 0 and plan(qlen=1024, maxlen=3000)["bnd_need"] == 0
    p = plan(qlen=1025, maxlen=3000)
    assert p["bnd_row_ints"] == 2 and p["bnd_per"] == 2 * 3160 and p["bnd_need"] == p["grid"] * 4 * p["bnd_per"]
    assert plan(qlen=1025, maxlen=3001)["bnd_per"] == 2 * 3164
    # grid: resident workgroups, fewer for few targets, fewer where the boundary columns would pass 1 GiB
    assert plan(qlen=512)["grid"] == 5 * 256 and plan(qlen=100)["grid"] == 6 * 256 and plan(qlen=2000)["grid"] == 3 * 256
    assert plan(qlen=512, ntargets=9)["grid"] == 3 and plan(qlen=512, ntargets=8)["grid"] == 2 and plan(qlen=512, ntargets=1)["grid"] == 1
    per = 2 * ((1000000 + 160 + 3) // 4) * 4
    assert plan(qlen=2000, maxlen=1000000)["grid"] == (1 << 30) // (per * 16)
    assert (1 << 30) // (per * 16) < 3 * 256
    assert plan(qlen=1024, maxlen=1000000)["grid"] == 3 * 256            # one strip: no boundary column, no cap
    # profile blocks: one per 256 bytes, at most 4096
    assert plan(qlen=4)["prof_blocks"] == 257 and plan(qlen=5000)["prof_blocks"] == 4096


def test_check_isa_audits_affine_kernels():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_isa.py")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "search kernels without scratch" in out.stdout          # the text tests/test_search_host.py reads
    assert "3 affine search kernels without scratch" in out.stdout


def test_scores_beyond_a_signed_byte_are_refused_not_clamped(swamd, tmp_path):
    for m, x in [(200, -3), (3, -129), (128, 0)]:
        with pytest.raises(ValueError, match="int8"):
            swamd.submat_match(m, x)
    assert swamd.submat_match(127, -128)[0, 0] == 127 and swamd.submat_match(127, -128)[0, 1] == -128
    # the CLI refuses them, and flag values that are no integers, before it touches a device
    exe = os.path.join(ROOT, "smith-waterman_amd", "smithW")
    fa = tmp_path / "x.fa"
    fa.write_text(">x\nACGT\n")
    for extra, what in [(["--scores", "200", "-3", "-2", "--gap-open", "-5"], "-128..127"),
                        (["--gap-open", "five"], "--gap-open needs an integer"),
                        (["--gap-open", "-5", "--gap-extend", "1x"], "--gap-extend needs an integer")]:
        out = subprocess.run([exe, "--search", str(fa), str(fa)] + extra, capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and what in out.stderr, out.stderr
