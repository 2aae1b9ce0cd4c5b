"""GPU: smithW --search Q.fa DB.fa --all-queries --prefilter S (one handle: sw_db_prefilter_ungapped, then sw_db_search_affine_pairs on
its device list): stdout but for the line of timings equals, byte for byte, the rendering built from the Python host legs
(prefilter_ungapped_host + search_affine_pairs_host); the flags --prefilter excludes, and S < 1."""
import os
import subprocess

import numpy as np
import pytest

from affine_cases import PROTEIN
from oracle_lib import ROOT

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "smith-waterman_amd", "smithW")


def run(*args):
    return subprocess.run([CLI, *[str(a) for a in args]], capture_output=True, text=True, timeout=120)


def fasta(path, seqs, name):
    with open(path, "w") as f:
        for k, s in enumerate(seqs):
            f.write(f">{name}{k} some description\n")
            s = bytes(s).decode()
            f.write("\n".join(s[i:i + 60] for i in range(0, len(s), 60)) + "\n")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    rng = np.random.default_rng(43)
    d = tmp_path_factory.mktemp("cli_prefilter")
    letters = PROTEIN[:20]
    queries = [rng.choice(letters, n).astype(np.uint8) for n in (30, 300, 600)]
    targets = [rng.choice(letters, int(n)).astype(np.uint8) for n in (50, 7, 200, 64, 400, 33, 90)]
    targets[2] = np.concatenate([targets[2][:40], queries[1][20:200], targets[2][40:]])       # a related pair: a long diagonal
    targets[6][10:50] = queries[2][500:540]                                                  # and a short one
    fasta(d / "q.fa", queries, "query")
    fasta(d / "db.fa", targets, "rec")
    with open(d / "m.txt", "w") as f:                              # a small NCBI-format table: matches 5, mismatches -2 .. -4
        ls = [chr(c) for c in letters]
        f.write("# test table\n   " + "  ".join(ls) + "\n")
        for i, a in enumerate(ls):
            f.write(a + " " + " ".join(str(5 if i == j else -2 - (i + 2 * j) % 3) for j in range(len(ls))) + "\n")
    return d, str(d / "q.fa"), str(d / "db.fa"), str(d / "m.txt"), queries, targets


def rendering(swamd, files, sub, go, ge, s):
    """What the tool prints before its line of timings."""
    _, _, _, _, queries, targets = files
    pairs, n, u = swamd.prefilter_ungapped_host(queries, targets, sub, s)
    pairs = pairs[:n]
    res = swamd.search_affine_pairs_host(queries, targets, (sub, go, ge), pairs)
    out = [f"# {n} pairs of {len(queries)} queries and {len(targets)} targets pass the ungapped pre-filter at {s}; query\ttarget\tname\tscore\ttarget_end\tquery_end"]
    for (q, k), (pos, score, _) in zip(pairs.tolist(), res.tolist()):
        m = len(queries[q]) + 1
        out.append(f"{q}\t{k}\trec{k}\t{score}\t{pos // m}\t{pos % m} ungapped={u[q, k]}")
    return "\n".join(out) + "\n\n"


def before_timings(text):
    at = text.index("Elapsed time for database search:")
    assert text[at:].count("\n") == 2 and text.endswith("\n\n")                         # the line of timings and a blank line end the output
    return text[:at]


def test_stdout_equals_the_rendering_of_the_host_legs(swamd, files):
    d, q, db, m, _, _ = files
    sub = swamd.read_submat(m)
    for s, least in ((25, 3), (60, 2), (1, 21), (100000, 0)):
        r = run("--search", q, db, "--all-queries", "--matrix", m, "--gap-open", -6, "--gap-extend", -1, "--prefilter", s)
        assert r.returncode == 0, r.stderr
        want = rendering(swamd, files, sub, -6, -1, s)
        assert before_timings(r.stdout) == want, s
        assert want.count("ungapped=") >= least and (s != 100000 or want.count("ungapped=") == 0)
    want = rendering(swamd, files, sub, -6, -1, 60)
    assert "1\t2\trec2\t" in want and "2\t6\trec6\t" in want                              # the planted pairs pass
    r = run("--search", q, db, "--all-queries", "--scores", 3, -3, -2, "--prefilter", 20)  # linear gaps through the match table, gap_open 0
    assert r.returncode == 0, r.stderr
    assert before_timings(r.stdout) == rendering(swamd, files, swamd.submat_match(3, -3), 0, -2, 20)


def test_excluded_flags_and_a_threshold_below_one(files):
    d, q, db, m, _, _ = files
    (d / "one.txt").write_text("0 0\n")
    for flags, word in ((("--top", 3), "--top"), (("--min-score", 5), "--min-score"), (("--align",), "--align"), (("--pairs", d / "one.txt"), "--pairs")):
        r = run("--search", q, db, "--all-queries", "--prefilter", 20, *flags)
        assert r.returncode == 2 and f"--prefilter does not go with {word}" in r.stderr and "usage:" not in r.stderr and r.stdout == "", (flags, r.stderr)
    for s in (0, -4):
        r = run("--search", q, db, "--all-queries", "--prefilter", s)
        assert r.returncode == 2 and "S >= 1" in r.stderr and r.stdout == ""
    r = run("--search", q, db, "--prefilter", 20)
    assert r.returncode == 2 and "--prefilter goes with --search --all-queries" in r.stderr
    r = run("40", "30", "--prefilter", 20)
    assert r.returncode == 2 and "--prefilter goes with --search --all-queries" in r.stderr
    r = run("--search", q, db, "--all-queries", "--prefilter", 20, "--scores", 300, -3, -2)
    assert r.returncode == 2 and "--prefilter without --matrix" in r.stderr
