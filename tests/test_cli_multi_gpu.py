"""GPU: smithW --search Q.fa DB.fa --all-queries (every record of Q.fa through one prepared database handle) against one
single-query run per record: the hit blocks are equal line for line."""
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


def fasta(path, seqs):
    with open(path, "w") as f:
        for k, s in enumerate(seqs):
            f.write(f">rec{k}\n")
            s = bytes(s).decode()
            f.write("\n".join(s[i:i + 60] for i in range(0, len(s), 60)) + "\n")


def blocks(text):
    """The hit blocks of an output: from every '# query' line to the blank line in front of 'Elapsed time'."""
    out, cur = [], None
    for ln in text.splitlines():
        if ln.startswith("# query"):
            cur = [ln]
            out.append(cur)
        elif ln.startswith("##") or not ln.strip() or ln.startswith("Elapsed"):
            cur = None
        elif cur is not None:
            cur.append(ln)
    return out


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    rng = np.random.default_rng(8)
    d = tmp_path_factory.mktemp("cli_multi")
    letters = PROTEIN[:20]
    queries = [rng.choice(letters, n).astype(np.uint8) for n in (40, 300, 700)]
    targets = [rng.choice(letters, int(n)).astype(np.uint8) for n in rng.integers(20, 400, 30)]
    for k, q in enumerate(queries):                                # related targets: the alignments are long
        t = q[5:].copy()
        t[::9] = letters[3]
        targets.insert(4 * k + 1, np.concatenate([t[:len(t) // 2], rng.choice(letters, 3).astype(np.uint8), t[len(t) // 2:]]))
    fasta(d / "q.fa", queries)
    fasta(d / "db.fa", targets)
    with open(d / "m.txt", "w") as f:                              # a small NCBI-format table: matches 5, mismatches -2 .. -4
        ls = [chr(c) for c in letters]
        f.write("# test table\n   " + "  ".join(ls) + "\n")
        for i, a in enumerate(ls):
            f.write(a + " " + " ".join(str(5 if i == j else -2 - (i + 2 * j) % 3) for j in range(len(ls))) + "\n")
    return str(d / "q.fa"), str(d / "db.fa"), str(d / "m.txt")


@pytest.mark.parametrize("extra", [("--top", 5), ("--top", 4, "--matrix", "M", "--gap-open", -6, "--gap-extend", -1, "--align"),
                                   ("--top", 3, "--gap-extend", -3), ("--top", 3, "--scores", 2, -1, -2, "--align")])
def test_all_queries_equals_three_single_runs(files, extra):
    q, db, m = files
    extra = [m if x == "M" else x for x in extra]
    r = run("--search", q, db, "--all-queries", *extra)
    assert r.returncode == 0, r.stderr
    got = blocks(r.stdout)
    assert len(got) == 3 and r.stdout.count("## query record") == 3 and f"## query record 1 of {q}" in r.stdout
    assert r.stdout.count("Elapsed time for database search:") == 1
    for k in range(3):
        one = run("--search", q, db, "--record-a", k, *extra)
        assert one.returncode == 0, one.stderr
        want = blocks(one.stdout)
        assert len(want) == 1 and len(want[0]) > 3 and got[k] == want[0], f"record {k}"


def test_all_queries_usage(files):
    q, db, _ = files
    for args in (("--all-queries",), ("40", "30", "--all-queries")):
        r = run(*args)
        assert r.returncode == 2 and "--all-queries goes with --search" in r.stderr and "usage:" not in r.stderr
    r = run("--search", q, db, "--all-queries", "--scores", 300, -3, -2)              # a table of signed bytes cannot hold 300
    assert r.returncode == 2 and "--all-queries without --matrix needs --scores" in r.stderr
