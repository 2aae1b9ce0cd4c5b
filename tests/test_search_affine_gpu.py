"""GPU: database search with a substitution matrix and affine gaps (sw_search_affine_device / Engine.search_affine /
smithW --search --matrix) against the independent checker (tests/affine_oracle.cpp), and against Engine.search where the two must agree."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from affine_cases import DNA, GAPS, PROTEIN, ROOT, alphabets, assert_same, checker, database, random_submat  # noqa: F401

pytestmark = pytest.mark.gpu

SCORINGS = [(3, -3, -2), (5, -3, -4), (1, 1, 0), (2, 0, -1)]                                    # those of tests/test_search_gpu.py
QLENS = [1, 7, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049, 5000]          # likewise


@pytest.mark.parametrize("i,qlen", list(enumerate(QLENS)))
def test_search_affine_matches_checker(engine, checker, i, qlen):  # noqa: F811
    rng = np.random.default_rng(2000 + qlen)
    qa, ta = alphabets(i)
    go, ge = GAPS[i % len(GAPS)]
    query = rng.choice(qa, qlen).astype(np.uint8)
    packed, offs = database(rng, qlen, ta)                     # 3e7 cells
    sub = random_submat(rng)
    res = engine.search_affine(query, (packed, offs), sub, go, ge)
    assert_same(res, checker.search(query, packed, offs, sub, go, ge), f"qlen {qlen} go {go} ge {ge}")
    # the kernel is the planner's choice (index 0 / 1 / 2 = 4 / 8 / 16 columns per lane): beyond 512 columns it takes 16 per lane only while the
    # code object reports two workgroups per CU for that kernel, 8 otherwise -- either is a correct plan, QLENS brackets the strips of both
    assert engine.get_option("last_search_affine_kernel") in ((0,) if qlen <= 256 else (1,) if qlen <= 512 else (1, 2))


def _crisp_submat(rng):
    """Matches 5..9, mismatches -4..-1 over the protein letters: the diagonal is the largest entry of its row and column."""
    n = len(PROTEIN)
    sc = rng.integers(-4, 0, (n, n)).astype(np.int8)
    sc[np.arange(n), np.arange(n)] = rng.integers(5, 10, n).astype(np.int8)
    import importlib
    return importlib.import_module("smith-waterman_amd").submat_from_letters(PROTEIN, sc, -4)


def test_indels_open_gaps_across_strip_boundaries(engine, checker):  # noqa: F811
    """Targets cut from the query with runs deleted and inserted: affine scoring must differ from linear, and gaps must lie open across
    the strip boundary (column 1024 ends a strip at 16 columns per lane and at 8, whichever the planner takes).  Both are conditions of this TEST, asserted on the checker's matrices."""
    rng = np.random.default_rng(77)
    go, ge, B = -8, -1, 1024
    query = rng.choice(PROTEIN[:20], 2300).astype(np.uint8)
    sub = _crisp_submat(rng)
    diag = lambda seq: int(sum(int(sub[x, x]) for x in seq))  # noqa: E731
    targets, crossing = [], []
    # a run of the query missing from the target (F, a gap that consumes query letters) over columns B - d + 1 .. B + d: open across B | B + 1
    for d in (1, 5, 15):
        t = np.concatenate([query[B - 200:B - d], query[B + d:B + 200]])
        crossing.append((len(targets), "F", 200 - d, 2 * d, diag(t) + go + 2 * d * ge))
        targets.append(t)
    # a run inserted into the target (E, a gap that consumes target letters) in column B, the last of strip 0: H = E leaves through the boundary
    for n in (1, 15, 30):
        t = np.concatenate([query[B - 200:B], rng.choice(PROTEIN[20:], n).astype(np.uint8), query[B:B + 200]])
        crossing.append((len(targets), "E", 200 + n, n, diag(t[:200]) + diag(t[200 + n:]) + go + n * ge))
        targets.append(t)
    # slices anywhere with 1..4 runs of 1..30 letters deleted or inserted
    for _ in range(60):
        a = int(rng.integers(0, 1500))
        s = list(query[a:a + int(rng.integers(300, 800))])
        for _ in range(int(rng.integers(1, 5))):
            at, run = int(rng.integers(40, len(s) - 40)), int(rng.integers(1, 31))
            if rng.random() < 0.5:
                del s[at:at + run]
            else:
                s[at:at] = list(rng.choice(PROTEIN[:20], run))
        targets.append(np.array(s, np.uint8))
    offs = np.zeros(len(targets) + 1, np.int64)
    offs[1:] = np.cumsum([len(t) for t in targets])
    packed = np.concatenate(targets)
    exp = checker.search(query, packed, offs, sub, go, ge)
    # condition 1: affine differs from both linear scorings for at least a quarter of the targets
    lin_e = checker.search(query, packed, offs, sub, 0, ge)[:, 1]
    lin_oe = checker.search(query, packed, offs, sub, 0, go + ge)[:, 1]
    differs = (exp[:, 1] != lin_e) & (exp[:, 1] != lin_oe)
    assert differs.sum() * 4 >= len(targets), f"only {differs.sum()} of {len(targets)} targets tell affine from linear gaps"
    # condition 2: the best alignment of the built targets holds a gap open across the boundary column
    for k, kind, row, glen, score in crossing:
        s, p, H, E, F = checker.matrices(query, targets[k], sub, go, ge)
        assert s == score == exp[k, 1], f"target {k}: the best alignment is not the one built ({s} vs {score})"
        if kind == "F":      # in row `row` the gap runs through columns B and B + 1: extended, not opened, and it is what H holds there
            assert F[row, B + 1] == F[row, B] + ge > H[row, B] + go + ge
            assert H[row, B + 1] == F[row, B + 1] > 0 and H[row, B] == F[row, B]
        else:                # in column B the gap's last row: E extended from the row above, H = E, and the diagonal leaves from it into strip 1
            assert H[row, B] == E[row, B] > 0 and (glen == 1 or E[row, B] == E[row - 1, B] + ge > H[row - 1, B] + go + ge)
            assert H[row + 1, B + 1] == H[row, B] + sub[query[B], targets[k][row]]
    res = engine.search_affine(query, (packed, offs), sub, go, ge)
    assert engine.get_option("last_search_affine_kernel") in (1, 2)      # strips of 512 or 1024 columns: B is a boundary of both
    assert_same(res, exp, "indel targets")


@pytest.mark.parametrize("i,qlen", [(0, 64), (1, 257), (2, 513), (3, 1025), (4, 2049), (5, 5000)])
def test_gap_open_zero_match_table_equals_linear_search(engine, swamd, i, qlen):
    rng = np.random.default_rng(1000 + qlen)                   # the databases of tests/test_search_gpu.py
    qa, ta = alphabets(i)
    match, mismatch, gap = SCORINGS[i % len(SCORINGS)]
    query = rng.choice(qa, qlen).astype(np.uint8)
    packed, offs = database(rng, qlen, ta)
    lin = engine.search(query, (packed, offs), (match, mismatch, gap))
    aff = engine.search_affine(query, (packed, offs), swamd.submat_match(match, mismatch), 0, gap)
    assert np.array_equal(aff, lin)


def test_ties_pin_the_lowest_index(engine, checker, swamd):  # noqa: F811
    query = np.frombuffer(b"ACGT" * 300, np.uint8)             # periodic, two strips: the maximum is reached at many cells
    targets = [b"ACGT" * n for n in (1, 2, 16, 17, 100, 200, 300)] + [b"CGTA" * 40, b"GTAC" * 300, b"ACG" * 90]
    packed, offs = swamd._pack_targets(targets)
    for (m, x), (go, ge) in [((3, -3), (-4, -1)), ((1, 1), (0, 0)), ((2, 0), (-1, 0)), ((2, -1), (0, -1))]:
        sub = swamd.submat_match(m, x)
        res = engine.search_affine(query, targets, sub, go, ge)
        assert_same(res, checker.search(query, packed, offs, sub, go, ge), f"table {m, x} gaps {go, ge}")
    res = engine.search_affine(b"A" * 300, [b"C" * 10, b"G" * 1000, b"T" * 64], swamd.submat_match(3, -3), -2, -1)
    assert np.array_equal(res, np.zeros((3, 3), np.int64))     # nothing positive


def test_long_target_among_short(engine, checker):  # noqa: F811
    rng = np.random.default_rng(7)
    lens = list(rng.integers(1, 100, 5000))
    lens.insert(1234, 200_000)
    offs = np.zeros(len(lens) + 1, np.int64)
    offs[1:] = np.cumsum(lens)
    packed = rng.choice(DNA, int(offs[-1])).astype(np.uint8)
    query = rng.choice(DNA, 1100).astype(np.uint8)             # two strips: a boundary column of 200 000 rows
    sub = random_submat(rng, -6, 6)
    res = engine.search_affine(query, (packed, offs), sub, -5, -1)
    assert_same(res, checker.search(query, packed, offs, sub, -5, -1), "long among short")


def test_results_in_input_order(engine):
    rng = np.random.default_rng(3)
    targets = [rng.choice(PROTEIN, int(n)).astype(np.uint8) for n in rng.integers(0, 900, 300)]
    query = rng.choice(PROTEIN, 400).astype(np.uint8)
    sub = random_submat(rng)
    res = engine.search_affine(query, targets, sub, -6, -2)
    perm = rng.permutation(len(targets))
    res2 = engine.search_affine(query, [targets[p] for p in perm], sub, -6, -2)
    assert np.array_equal(res2, res[perm])
    _, top = engine.search_affine(query, targets, sub, -6, -2, top=5)
    assert list(res[top, 1]) == sorted(res[:, 1], reverse=True)[:5]


def test_repeated_calls_regrow_workspaces(checker, swamd):  # noqa: F811
    rng = np.random.default_rng(11)
    packed, offs = database(rng, 300, PROTEIN, budget=3e6)
    q1 = rng.choice(PROTEIN, 300).astype(np.uint8)
    q2 = rng.choice(PROTEIN, 2500).astype(np.uint8)
    s1, s2 = random_submat(rng), random_submat(rng)
    e1, e2 = checker.search(q1, packed, offs, s1, -7, -1), checker.search(q2, packed, offs, s2, -2, -2)
    eng = swamd.Engine(0)                                      # a fresh context: every workspace starts empty and grows
    try:
        for _ in range(3):
            assert_same(eng.search_affine(q1, (packed, offs), s1, -7, -1), e1, "short query")
            assert_same(eng.search_affine(q2, (packed, offs), s2, -2, -2), e2, "long query")
            lin = eng.search(q2, (packed, offs))               # the linear search shares the workspaces
            assert_same(eng.search_affine(q2, (packed, offs), swamd.submat_match(3, -3), 0, -2), lin, "after a linear search")
    finally:
        eng.close()


def test_three_families_interleaved_on_one_fresh_context(swamd, oracle, checker):  # noqa: F811
    """sw_search_device, sw_search_affine_device and sw_align_affine_device share the schedule, profile, boundary, counter and table
    workspaces and the pinned copies the schedule and the table are uploaded from.  A fresh context, no host synchronisation between the
    calls, every call with more targets or hits than the one before (3 -> 40 -> 60 hits -> 120 -> 200 on a second stream), then one with
    fewer: the workspaces are reallocated while earlier uploads may still be in flight, the table is first allocated between two plain
    searches, and every call brings a table of its own.  Every result bit for bit against the host references."""
    import torch
    rng = np.random.default_rng(41)
    dbs = {3: [5, 0, 5],                                                       # an empty target and a length tie
           40: [0, 90, 90] + list(rng.integers(0, 91, 37)),
           200: [90, 0, 1, 90] + list(rng.integers(0, 91, 196))}
    dbs = {n: swamd._pack_targets([rng.choice(PROTEIN, int(k)).astype(np.uint8) for k in lens]) for n, lens in dbs.items()}
    q63, q300 = (rng.choice(PROTEIN, n).astype(np.uint8) for n in (63, 300))   # one strip; more columns than one strip of 4 per lane
    subs = [random_submat(rng) for _ in range(4)]
    hits60 = np.concatenate([[0, 1, 2, 1], rng.integers(0, 40, 56)]).astype(np.int64)
    hits5 = np.array([2, 0, 39, 2, 1], np.int64)
    cap = 300 + 90
    eng = swamd.Engine(0)                                                      # a fresh context: every workspace starts empty
    try:
        dev = lambda x: torch.from_numpy(np.concatenate([x, np.zeros(16, np.uint8)])).to("cuda:0")  # noqa: E731
        d63, d300 = dev(q63), dev(q300)
        ddb = {n: dev(packed) for n, (packed, _) in dbs.items()}
        res = lambda n: torch.full((max(1, n), 3), 7, dtype=torch.int64, device="cuda:0")  # noqa: E731
        alns = lambda n: (torch.full((n, 7), 7, dtype=torch.int64, device="cuda:0"), torch.zeros((n, cap), dtype=torch.uint8, device="cuda:0"))  # noqa: E731
        r0, r1, r2, r4, r5, o3, o6 = res(0), res(3), res(40), res(120), res(200), alns(60), alns(5)
        second = torch.cuda.Stream()
        torch.cuda.synchronize()
        eng.search_device(d63, 63, ddb[3], dbs[3][1][:1], out=r0)                                   # no target at all: nothing happens
        eng.search_device(d63, 63, ddb[3], dbs[3][1], out=r1)
        eng.search_affine_device(d300, 300, ddb[40], dbs[40][1], subs[0], -10, -1, out=r2)
        eng.align_affine_device(d300, 300, ddb[40], dbs[40][1], subs[1], -3, -2, hits60, ops_cap=cap, out=o3)
        eng.search_device(d300, 300, ddb[200], dbs[200][1][:121], (5, -3, -4), out=r4)
        with torch.cuda.stream(second):
            eng.search_affine_device(d63, 63, ddb[200], dbs[200][1], subs[2], 0, -2, out=r5)
        eng.align_affine_device(d300, 300, ddb[40], dbs[40][1], subs[3], -4, 0, hits5, ops_cap=cap, out=o6)
        torch.cuda.synchronize()
    finally:
        eng.close()
    assert (r0.cpu().numpy() == 7).all()

    def linear(query, n, ntargets, scores, got):
        packed, offs = dbs[n]
        exp = np.zeros((ntargets, 3), np.int64)
        for k in range(ntargets):
            if offs[k + 1] > offs[k]:
                o = oracle.fill_streaming(query, packed[offs[k]:offs[k + 1]], scores)
                exp[k] = (o["max_pos"], o["max_score"], 0)
        assert_same(got.cpu().numpy(), exp, f"linear search, {ntargets} targets")

    def affine(query, n, sub, go, ge, got):
        exp = checker.search(query, *dbs[n], sub, go, ge)
        assert np.array_equal(swamd.search_affine_host(query, dbs[n], sub, go, ge), exp)
        assert_same(got.cpu().numpy(), exp, f"affine search, {n} targets")

    def aligned(query, n, sub, go, ge, hits, got):
        exp_aln, exp_ops = swamd.align_affine_host(query, dbs[n], sub, go, ge, hits)
        assert np.array_equal(exp_aln[:, :2], checker.search(query, *dbs[n], sub, go, ge)[hits, :2])
        aln = got[0].cpu().numpy()
        assert np.array_equal(aln, exp_aln), f"alignment of {len(hits)} hits: rows {np.nonzero((aln != exp_aln).any(axis=1))[0][:5]} differ"
        assert swamd._ops_list(aln, got[1].cpu().numpy(), cap) == exp_ops, f"alignment of {len(hits)} hits: ops differ"

    linear(q63, 3, 3, (3, -3, -2), r1)
    affine(q300, 40, subs[0], -10, -1, r2)
    aligned(q300, 40, subs[1], -3, -2, hits60, o3)
    linear(q300, 200, 120, (5, -3, -4), r4)
    affine(q63, 200, subs[2], 0, -2, r5)
    aligned(q300, 40, subs[3], -4, 0, hits5, o6)


def test_scores_just_below_the_limit_and_one_step_over(engine, swamd):
    L = -(-(1 << 24) // 127) - 1                               # 127 L < 2^24 <= 127 (L + 1)
    assert 127 * L < (1 << 24) <= 127 * (L + 1)
    sub = swamd.submat_match(127, -128)
    query = np.full(L + 1, ord("A"), np.uint8)
    res = engine.search_affine(query, [b"A" * L, b"A" * 100, b"C" * 50], sub, -20, -3)
    # all letters equal: H[i][j] = 127 min(i, j); the maximum first at (L, L), again at (L, L + 1): the lowest index is pinned
    assert tuple(res[0]) == (L * (L + 2) + L, 127 * L, 0)
    assert tuple(res[1]) == (100 * (L + 2) + 100, 12700, 0) and tuple(res[2]) == (0, 0, 0)
    with pytest.raises(swamd.SwError) as e:
        engine.search_affine(query, [b"A" * (L + 1)], sub, -20, -3)
    assert e.value.code == -22 and "s[0][0] = 127" in str(e.value)


def test_rejects_bad_input(engine, swamd):
    import torch
    lib = swamd.lib()
    dq = torch.zeros(64, dtype=torch.uint8, device="cuda")
    ddb = torch.zeros(256, dtype=torch.uint8, device="cuda")
    dres = torch.zeros((8, 3), dtype=torch.int64, device="cuda")
    sub = swamd.submat_match(3, -3)

    def call(qlen=10, offs=(0, 5, 9), go=-3, ge=-1, table=sub, q=dq.data_ptr(), db=ddb.data_ptr(), res=dres.data_ptr(), n=None, offs_ptr=True, scoring=True):
        o = np.array(offs, np.int64)
        sc = swamd._Affine(table.ctypes.data if table is not None else None, go, ge)
        return lib.sw_search_affine_device(engine._h, q, qlen, db, o.ctypes.data if offs_ptr else None, len(o) - 1 if n is None else n,
                                           ctypes.byref(sc) if scoring else None, res, None)

    assert call() == 0
    engine.synchronize()
    assert call(offs=(0, 5, 4)) == -22 and b"decrease" in lib.sw_last_error()
    assert call(qlen=0) == -22 and call(qlen=1 << 20) == -22 and call(offs=(0, 1 << 20)) == -22
    assert call(go=1) == -22 and call(ge=1) == -22
    assert call(go=-(1 << 24), ge=-1) == -22
    assert call(q=None) == -22 and call(db=None) == -22 and call(res=None) == -22 and call(offs_ptr=False) == -22
    assert call(n=-1) == -22 and call(scoring=False) == -22 and call(table=None) == -22
    assert call(go=-(1 << 24), ge=0) == 0
    engine.synchronize()


def test_cli_search_with_matrix_matches_checker(swamd, checker, tmp_path):  # noqa: F811
    rng = np.random.default_rng(5)
    letters = PROTEIN[:20]
    n = len(letters)
    sc = rng.integers(-4, 3, (n, n)).astype(np.int8)
    sc[np.arange(n), np.arange(n)] = rng.integers(4, 12, n).astype(np.int8)
    mf = tmp_path / "m.txt"
    mf.write_text("# test matrix\n   " + "  ".join(chr(c) for c in letters) + "\n" +
                  "".join(chr(letters[r]) + " " + " ".join(f"{v:3d}" for v in sc[r]) + "\n" for r in range(n)))
    sub = swamd.submat_from_letters(letters, sc, int(sc.min()))
    q = rng.choice(letters, 300).astype(np.uint8)
    recs = [rng.choice(letters, int(k)).astype(np.uint8) for k in rng.integers(0, 700, 40)]
    recs[7] = np.concatenate([recs[7], q[50:120], q[135:200]])          # the query with 15 letters missing: found through a gap
    qf, dbf = tmp_path / "q.fa", tmp_path / "db.fa"
    qf.write_bytes(b">decoy\nAAAA\n>query\n" + bytes(q) + b"\n")
    dbf.write_bytes(b"".join(b">t%d\n" % k + bytes(r) + b"\n" for k, r in enumerate(recs)))
    exe = os.path.join(ROOT, "smith-waterman_amd", "smithW")
    out = subprocess.run([exe, "--search", str(qf), str(dbf), "--record-a", "1", "--top", "12", "--matrix", str(mf), "--gap-open", "-9",
                          "--gap-extend", "-1"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert lines[0].startswith("#") and any(ln.startswith("Elapsed time") for ln in lines)
    hits = [tuple(int(x) for x in ln.split("\t")) for ln in lines[1:13]]
    packed, offs = swamd._pack_targets(recs)
    exp = checker.search(q, packed, offs, sub, -9, -1)
    order = sorted(range(len(recs)), key=lambda k: (-exp[k, 1], k))
    for rank, (hit, k) in enumerate(zip(hits, order[:12])):
        assert hit == (rank + 1, k, exp[k, 1], exp[k, 0] // 301, exp[k, 0] % 301)
    assert hits[0][1] == 7
    # without --matrix: the match / mismatch table of --scores
    out = subprocess.run([exe, "--search", str(qf), str(dbf), "--record-a", "1", "--top", "3", "--scores", "5", "-3", "-4", "--gap-open", "-6",
                          "--gap-extend", "-1"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    hit = tuple(int(x) for x in [ln for ln in out.stdout.splitlines() if ln.strip()][1].split("\t"))
    exp = checker.search(q, packed, offs, swamd.submat_match(5, -3), -6, -1)
    best = min(range(len(recs)), key=lambda k: (-exp[k, 1], k))
    assert hit == (1, best, exp[best, 1], exp[best, 0] // 301, exp[best, 0] % 301)
