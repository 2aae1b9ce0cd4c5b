"""GPU: the alignment of hits under affine scoring (sw_align_affine_device / Engine.align_affine / smithW --search --align) against
the walk of the canonical alignment over the independent checker's matrices (tests/align_cases.py), the host leg, the affine
search's arg-max and, with gap_open = 0, the linear fill's traceback."""
import os
import subprocess

import numpy as np
import pytest

from affine_cases import DNA, GAPS, PROTEIN, ROOT, alphabets, checker, random_submat  # noqa: F401
from align_cases import expected, h_cells, indel_cases, pack, replay

pytestmark = pytest.mark.gpu

QLENS = [1, 7, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049]


def assert_exact(checker, query, targets, sub, go, ge, hits, aln, ops, what=""):  # noqa: F811
    assert aln.shape == (len(hits), 7) and len(ops) == len(hits)
    memo = {}
    for h, k in enumerate(hits):
        if k not in memo:
            memo[k] = expected(checker, query, targets[k], sub, go, ge)
        row, eops, _ = memo[k]
        assert tuple(int(x) for x in aln[h]) == row, f"{what} hit {h} (target {k}, len {len(targets[k])}): {tuple(aln[h])} vs {row}"
        assert ops[h] == eops, f"{what} hit {h} (target {k}, len {len(targets[k])}): ops differ"
        replay(query, targets[k], sub, go, ge, aln[h], ops[h])


@pytest.mark.parametrize("i,qlen", list(enumerate(QLENS)))
def test_align_matches_the_rule(engine, checker, i, qlen):  # noqa: F811
    rng = np.random.default_rng(3000 + qlen)
    qa, ta = alphabets(i)
    go, ge = GAPS[i % len(GAPS)]
    query = rng.choice(qa, qlen).astype(np.uint8)
    lens = [0, 1, 63, 64, 65] + list(rng.integers(2, 701, 19))
    targets = [rng.choice(ta, n).astype(np.uint8) for n in lens]
    order = rng.permutation(len(targets))
    targets = [targets[k] for k in order]
    packed, offs = pack(targets)
    sub = random_submat(rng)
    hits = list(range(len(targets)))
    aln, ops = engine.align_affine(query, (packed, offs), sub, go, ge, hits)
    assert_exact(checker, query, targets, sub, go, ge, hits, aln, ops, f"qlen {qlen} gaps {go, ge}")
    res = engine.search_affine(query, (packed, offs), sub, go, ge)
    assert np.array_equal(aln[:, :2], res[:, :2])
    assert engine.get_option("last_align_affine_kernel") in ((0,) if qlen <= 256 else (1,) if qlen <= 512 else (1, 2))
    assert engine.get_option("last_align_affine_slots") == len(hits)


def test_gaps_across_the_strip_boundary_sit_where_they_were_built(engine, checker, swamd):  # noqa: F811
    rng = np.random.default_rng(77)
    B = 1024                                   # ends a strip at 16 columns per lane and at 8, whichever the planner takes
    query = rng.choice(PROTEIN[:20], 2300).astype(np.uint8)
    sub, go, ge, cases = indel_cases(swamd, rng, query, B, span=200)
    targets = [c[0] for c in cases]
    hits = list(range(len(targets)))
    aln, ops = engine.align_affine(query, targets, sub, go, ge, hits)
    assert engine.get_option("last_align_affine_kernel") in (1, 2)
    for k, (t, eops, score) in enumerate(cases):
        s, p, H, E, F = checker.matrices(query, t, sub, go, ge)
        assert s == score, f"case {k}: the best alignment is not the one built ({s} vs {score})"
        assert int(aln[k, 1]) == score and ops[k] == eops, f"case {k}: {ops[k]}"
        assert tuple(int(x) for x in aln[k, 2:6]) == (B - 200, 0, B + 200, len(t))
    assert_exact(checker, query, targets, sub, go, ge, hits, aln, ops, "indels")


def test_slots_are_reused(swamd, checker):  # noqa: F811
    """40 hits through one or two direction matrices: every hit but the first walks a slot whose lines an earlier hit left behind."""
    rng = np.random.default_rng(5)
    query = rng.choice(PROTEIN, 513).astype(np.uint8)
    # related targets, so that the alignments are long: slices of the query with substitutions and indels
    targets = []
    for n in rng.integers(300, 701, 40):
        a = int(rng.integers(0, 100))
        s = list(query[a:a + 400])
        for _ in range(3):
            at, run = int(rng.integers(20, len(s) - 20)), int(rng.integers(1, 10))
            if rng.random() < 0.5:
                del s[at:at + run]
            else:
                s[at:at] = list(rng.choice(PROTEIN, run))
        s = (list(rng.choice(PROTEIN, n)) + s)[-int(n):] if len(s) < n else s[:int(n)]
        targets.append(np.array(s, np.uint8))
    assert min(len(t) for t in targets) >= 300 and max(len(t) for t in targets) <= 700
    sub = random_submat(rng)
    hits = list(range(40))
    eng = swamd.Engine(0)
    try:
        ref_aln, ref_ops = eng.align_affine(query, targets, sub, -10, -1, hits)
        assert eng.get_option("last_align_affine_slots") == 40
        eng.set_option("align_workspace_mib", 1)
        aln, ops = eng.align_affine(query, targets, sub, -10, -1, hits)
        assert eng.get_option("last_align_affine_slots") in (1, 2)
        assert np.array_equal(aln, ref_aln) and ops == ref_ops
        assert_exact(checker, query, targets, sub, -10, -1, hits, aln, ops, "one slot")
        assert max(len(o) for o in ops) > 200                        # long walks, not begin corners next to the end
        with pytest.raises(swamd.SwError, match="align_workspace_mib"):
            eng.align_affine(query, [rng.choice(PROTEIN, 1100).astype(np.uint8)], sub, -10, -1, [0])
    finally:
        eng.close()


def test_device_equals_host(engine, swamd):
    rng = np.random.default_rng(11)
    query = rng.choice(PROTEIN[:20], 300).astype(np.uint8)
    targets = []
    for k in range(200):
        t = rng.choice(PROTEIN[:20], int(rng.integers(20, 500))).astype(np.uint8)
        if k % 3 == 0:                                                   # a third of them related to the query
            a = int(rng.integers(0, 150))
            t = np.concatenate([t[:20], query[a:a + 60], t[20:25], query[a + 63:a + 120]])
        targets.append(t)
    packed, offs = pack(targets)
    sub = random_submat(rng, -6, 9)
    res, top = engine.search_affine(query, (packed, offs), sub, -7, -1, top=50)
    aln, ops = engine.align_affine(query, (packed, offs), sub, -7, -1, top)
    haln, hops = swamd.align_affine_host(query, (packed, offs), sub, -7, -1, top)
    assert np.array_equal(aln, haln) and ops == hops
    assert np.array_equal(aln[:, :2], res[top][:, :2])
    for h, k in enumerate(top):
        replay(query, targets[k], sub, -7, -1, aln[h], ops[h])


@pytest.mark.parametrize("qlen,rows", [(65, 600), (513, 580), (1025, 333)])
def test_gap_open_zero_walks_the_linear_traceback(engine, swamd, qlen, rows):
    rng = np.random.default_rng(qlen)
    a = rng.choice(DNA, qlen).astype(np.uint8)
    b = rng.choice(DNA, rows).astype(np.uint8)
    out = engine.fill(a, b, (3, -3, -2))
    r = out.result()
    path = engine.traceback(out, r["max_pos"])
    aln, ops = engine.align_affine(a, [b], swamd.submat_match(3, -3), 0, -2, [0])
    assert (int(aln[0, 0]), int(aln[0, 1])) == (r["max_pos"], r["max_score"])
    assert h_cells(aln[0], ops[0], qlen) == [int(x) for x in path]


def test_empty_alignments(engine, swamd):
    t = engine.torch
    sub = swamd.submat_match(3, -3)
    targets = [b"C" * 10, b"", b"G" * 1000, b"T" * 64]
    aln, ops = engine.align_affine(b"A" * 300, targets, sub, -2, -1, [0, 1, 2, 3, 1])
    assert np.array_equal(aln, np.zeros((5, 7), np.int64)) and ops == [b""] * 5
    # coordinates only: d_ops = NULL with ops_cap = 0
    packed, offs = swamd._pack_targets(targets + [b"GGAAAATT"])
    d_q = t.from_numpy(np.frombuffer(b"A" * 300, np.uint8).copy()).to(f"cuda:{engine.device}")
    d_db = t.from_numpy(packed.copy()).to(f"cuda:{engine.device}")
    out = (t.full((5, 7), -1, dtype=t.int64, device=d_q.device), None)
    aln, none = engine.align_affine_device(d_q, 300, d_db, offs, sub, -2, -1, [4, 0, 1, 2, 3], ops_cap=0, out=out)
    engine.synchronize()
    aln = aln.cpu().numpy()
    assert none is None and np.array_equal(aln[1:], np.zeros((4, 7), np.int64))
    assert tuple(aln[0]) == (6 * 301 + 4, 12, 0, 2, 4, 6, 4)
    assert engine.align_affine(b"ACGT", targets, sub, -2, -1, [])[0].shape == (0, 7)      # nhits == 0: nothing launched


def test_cli_align(engine, swamd, tmp_path):
    rng = np.random.default_rng(3)
    letters = PROTEIN[:20]
    query = rng.choice(letters, 150).astype(np.uint8)
    targets = [rng.choice(letters, int(n)).astype(np.uint8) for n in rng.integers(50, 300, 12)]
    targets[4] = np.concatenate([targets[4][:30], query[10:70], query[75:140], targets[4][30:50]])
    targets[9] = np.concatenate([query[20:80], rng.choice(letters, 4).astype(np.uint8), query[80:130]])
    n = len(letters)
    sc = rng.integers(-4, 0, (n, n)).astype(np.int8)
    sc[np.arange(n), np.arange(n)] = rng.integers(5, 10, n).astype(np.int8)
    mpath = tmp_path / "m.txt"
    mpath.write_text("  " + " ".join(chr(c) for c in letters) + "\n" + "".join(chr(letters[r]) + " " + " ".join(str(v) for v in sc[r]) + "\n" for r in range(n)))
    qfa, dfa = tmp_path / "q.fa", tmp_path / "db.fa"
    qfa.write_text(">q\n" + query.tobytes().decode() + "\n")
    dfa.write_text("".join(f">t{k}\n{t.tobytes().decode()}\n" for k, t in enumerate(targets)))
    exe = os.path.join(ROOT, "smith-waterman_amd", "smithW")
    base = [exe, "--search", str(qfa), str(dfa), "--matrix", str(mpath), "--gap-open", "-8", "--gap-extend", "-1", "--top", "3"]
    plain = subprocess.run(base, capture_output=True, text=True, timeout=120)
    with_align = subprocess.run(base + ["--align"], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and with_align.returncode == 0, plain.stderr + with_align.stderr
    strip = lambda text: [ln for ln in text.split("\n") if not ln.startswith("Elapsed")]  # noqa: E731
    lines, plines = strip(with_align.stdout), strip(plain.stdout)
    # without --align: today's format -- the header, three hit lines of five fields, nothing else
    assert plines[0].startswith("# query 150 letters, 12 targets") and [len(ln.split("\t")) for ln in plines[1:4]] == [5, 5, 5]
    assert not any(ln.startswith(("align", "Q ", "T ")) for ln in plines)
    # with it: the same lines, each hit followed by its four
    assert [ln for i, ln in enumerate(lines) if not (1 <= i <= 15 and (i - 1) % 5 != 0)] == plines
    sub = swamd.read_submat(str(mpath))
    res, top = engine.search_affine(query, targets, sub, -8, -1, top=3)
    aln, ops = engine.align_affine(query, targets, sub, -8, -1, top)
    assert set(top) >= {4, 9}
    for h, k in enumerate(top):
        hit, al, lq, lm, lt = lines[1 + 5 * h:6 + 5 * h]
        assert [int(x) for x in hit.split("\t")[:3]] == [h + 1, k, int(res[k, 1])]
        assert al.split("\t") == ["align"] + [str(int(aln[h, c])) for c in (2, 4, 3, 5, 6)]
        assert (lq[:2], lm[:2], lt[:2]) == ("Q ", "  ", "T ")
        assert (lq[2:], lm[2:], lt[2:]) == swamd.format_alignment(query, targets[k], aln[h], ops[h])
        # the three lines rebuild to the library's ops
        rebuilt = bytes(ord("I") if b == "-" else ord("D") if a == "-" else ord("M") for a, b in zip(lq[2:], lt[2:]))
        assert rebuilt == ops[h]
    assert b"I" in b"".join(ops) and b"D" in b"".join(ops)
