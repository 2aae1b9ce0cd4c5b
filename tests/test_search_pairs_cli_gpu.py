"""GPU: smithW --search Q.fa DB.fa --pairs FILE (one handle, one sw_db_search_affine_pairs call): the pair lines against the Python host
leg line by line, comment and blank lines in the list, a malformed line (exit status 2, the line number in the message), and the flags
--pairs excludes."""
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
    rng = np.random.default_rng(41)
    d = tmp_path_factory.mktemp("cli_pairs")
    letters = PROTEIN[:20]
    queries = [rng.choice(letters, n).astype(np.uint8) for n in (30, 300, 600)]
    targets = [rng.choice(letters, int(n)).astype(np.uint8) for n in (50, 7, 200, 64, 400, 33)]
    targets[2] = np.concatenate([targets[2][:40], queries[1][20:200], targets[2][40:]])       # a related pair: a long alignment
    fasta(d / "q.fa", queries, "query")
    fasta(d / "db.fa", targets, "rec")
    with open(d / "m.txt", "w") as f:                              # a small NCBI-format table: matches 5, mismatches -2 .. -4
        ls = [chr(c) for c in letters]
        f.write("# test table\n   " + "  ".join(ls) + "\n")
        for i, a in enumerate(ls):
            f.write(a + " " + " ".join(str(5 if i == j else -2 - (i + 2 * j) % 3) for j in range(len(ls))) + "\n")
    return d, str(d / "q.fa"), str(d / "db.fa"), str(d / "m.txt"), queries, targets


PAIRS = [(1, 2), (0, 0), (2, 4), (1, 2), (0, 5), (2, 1), (7, 0), (1, 6), (-1, 3), (2, 5)]


def pair_lines(text):
    return [ln for ln in text.split("\n") if ln and not ln.startswith("#") and not ln.startswith("Elapsed")]


def expected(swamd, files, scoring):
    _, _, _, _, queries, targets = files
    res = swamd.search_affine_pairs_host(queries, targets, scoring, PAIRS)
    out = []
    for (q, k), (pos, score, _) in zip(PAIRS, res):
        m = len(queries[q]) + 1 if 0 <= q < len(queries) else 1
        name = f"rec{k}" if 0 <= k < len(targets) else "-"
        out.append(f"{q}\t{k}\t{name}\t{score}\t{pos // m}\t{pos % m}")
    return out


def test_pair_lines_equal_the_host_leg(swamd, files):
    d, q, db, m, _, _ = files
    with open(d / "pairs.txt", "w") as f:
        f.write("# candidate pairs\n\n")
        for i, (a, b) in enumerate(PAIRS):
            f.write(f"{a} {b}\n" if i % 2 else f"  {a}\t{b}  \n")
            if i == 4:
                f.write("   \n# another comment\n")
    r = run("--search", q, db, "--pairs", d / "pairs.txt", "--matrix", m, "--gap-open", -6, "--gap-extend", -1)
    assert r.returncode == 0, r.stderr
    want = expected(swamd, files, (swamd.read_submat(m), -6, -1))
    assert pair_lines(r.stdout) == want
    assert int(want[0].split("\t")[3]) > 500 and want[6].split("\t")[2:] == ["rec0", "0", "0", "0"] and want[7].split("\t")[2:] == ["-", "0", "0", "0"]
    r = run("--search", q, db, "--pairs", d / "pairs.txt", "--scores", 3, -3, -2)         # linear gaps through the match table, gap_open 0
    assert r.returncode == 0, r.stderr
    assert pair_lines(r.stdout) == expected(swamd, files, (swamd.submat_match(3, -3), 0, -2))


def test_a_malformed_line_names_its_number(files):
    d, q, db, m, _, _ = files
    for k, text in enumerate(["1 2\n# fine\n\n3 x\n", "1 2\n0 1\n4\n", "1 2 3\n", "1.5 2\n", "0 0\n\n\n\n1,2\n"]):
        path = d / f"bad{k}.txt"
        path.write_text(text)
        r = run("--search", q, db, "--pairs", path)
        lineno = (4, 3, 1, 1, 5)[k]
        assert r.returncode == 2 and f"line {lineno}:" in r.stderr and "bad" in r.stderr and pair_lines(r.stdout) == [], (text, r.stderr)
    r = run("--search", q, db, "--pairs", d / "missing.txt")
    assert r.returncode == 2 and "cannot open" in r.stderr


def test_excluded_flags(files):
    d, q, db, m, _, _ = files
    (d / "one.txt").write_text("0 0\n")
    for flags, word in ((("--all-queries",), "--all-queries"), (("--top", 3), "--top"), (("--all-queries", "--min-score", 5), "--all-queries"),
                        (("--min-score", 5), "--min-score"), (("--align",), "--align")):
        r = run("--search", q, db, "--pairs", d / "one.txt", *flags)
        assert r.returncode == 2 and f"--pairs does not go with {word}" in r.stderr and "usage:" not in r.stderr, (flags, r.stderr)
    r = run("40", "30", "--pairs", d / "one.txt")
    assert r.returncode == 2 and "--pairs goes with --search" in r.stderr
    r = run("--search", q, db, "--pairs", d / "one.txt", "--scores", 300, -3, -2)
    assert r.returncode == 2 and "--pairs without --matrix" in r.stderr
