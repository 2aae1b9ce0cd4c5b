"""GPU: smithW --pairs-lanes 16|32 (option "search_pairs_lanes"): with --pairs and with --prefilter-hits the lines printed under 16 are
the lines of the same command without the flag; other values and other modes are refused with a message before any device work."""
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
    rng = np.random.default_rng(54)
    d = tmp_path_factory.mktemp("cli_pairs_lanes")
    letters = PROTEIN[:20]
    queries = [rng.choice(letters, n).astype(np.uint8) for n in (30, 300, 600, 1100)]          # all three classes
    targets = [rng.choice(letters, int(n)).astype(np.uint8) for n in (50, 7, 200, 64, 400, 33, 90, 70, 100)]
    targets[2] = np.concatenate([targets[2][:40], queries[1][20:200], targets[2][40:]])        # a related pair: a long diagonal
    targets[6][10:50] = queries[2][500:540]                                                   # and two short ones, of similar lengths
    targets[8][30:80] = queries[2][100:150]
    fasta(d / "q.fa", queries, "query")
    fasta(d / "db.fa", targets, "rec")
    with open(d / "m.txt", "w") as f:                              # a small NCBI-format table: matches 5, mismatches -2 .. -4
        ls = [chr(c) for c in letters]
        f.write("# test table\n   " + "  ".join(ls) + "\n")
        for i, a in enumerate(ls):
            f.write(a + " " + " ".join(str(5 if i == j else -2 - (i + 2 * j) % 3) for j in range(len(ls))) + "\n")
    with open(d / "pairs.txt", "w") as f:                          # every pair in a shuffled order, some twice, some outside the files
        f.write("# query target\n")
        lines = [f"{q} {k}" for q in range(4) for k in range(9)] + ["2 6", "2 8", "2 6", "4 0", "0 9", "-1 3"]
        for i in rng.permutation(len(lines)):
            f.write(lines[i] + "\n")
    return str(d / "q.fa"), str(d / "db.fa"), str(d / "m.txt"), str(d / "pairs.txt")


def before_timings(text):
    at = text.index("Elapsed time for database search:")
    assert text[at:].count("\n") == 2 and text.endswith("\n\n")                         # the line of timings and a blank line end the output
    return text[:at]


def test_pairs_prints_the_same_lines(files):
    q, db, m, pairs = files
    base = ("--search", q, db, "--pairs", pairs, "--matrix", m, "--gap-open", -11, "--gap-extend", -1)
    plain = run(*base)
    assert plain.returncode == 0, plain.stderr
    want = before_timings(plain.stdout)
    assert want.count("\n") >= 42 and "\n1\t2\trec2" in "\n" + want
    for lanes in (16, 32):
        r = run(*base, "--pairs-lanes", lanes)
        assert r.returncode == 0, r.stderr
        assert before_timings(r.stdout) == want, lanes


def test_prefilter_hits_prints_the_same_lines(files):
    q, db, m, _ = files
    base = ("--search", q, db, "--all-queries", "--matrix", m, "--gap-open", -11, "--gap-extend", -1, "--prefilter-hits", 30, "--top", 3, "--align")
    plain = run(*base)
    assert plain.returncode == 0, plain.stderr
    want = before_timings(plain.stdout)
    assert want.count("## query record") == 4 and "align\t" in want
    for lanes in (16, 32):
        r = run(*base, "--pairs-lanes", lanes)
        assert r.returncode == 0, r.stderr
        assert before_timings(r.stdout) == want, lanes


def test_refusals_come_before_any_device_work(files):
    q, db, m, pairs = files
    scoring = ("--matrix", m, "--gap-open", -11, "--gap-extend", -1)
    env_without_a_device = {**os.environ, "HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"}

    def refused(*args):
        r = subprocess.run([CLI, *[str(a) for a in args]], capture_output=True, text=True, timeout=120, env=env_without_a_device)
        assert r.returncode == 2 and r.stdout == "" and "usage:" not in r.stderr, (args, r.stderr)
        return r.stderr

    for v in (8, 0, 64):
        assert f"--pairs-lanes takes 16 or 32, got {v}" in refused("--search", q, db, "--pairs", pairs, *scoring, "--pairs-lanes", v)
        assert f"--pairs-lanes takes 16 or 32, got {v}" in refused("--search", q, db, "--all-queries", *scoring, "--prefilter-hits", 30, "--pairs-lanes", v)
    assert "--pairs-lanes needs an integer" in refused("--search", q, db, "--pairs", pairs, *scoring, "--pairs-lanes", "wide")
    goes_with = "--pairs-lanes goes with --search --pairs or --search --all-queries --prefilter-hits"
    assert goes_with in refused("--search", q, db, *scoring, "--pairs-lanes", 16)
    assert goes_with in refused("--search", q, db, "--all-queries", *scoring, "--pairs-lanes", 16)
    assert goes_with in refused("--search", q, db, "--all-queries", *scoring, "--prefilter", 30, "--pairs-lanes", 16)
    assert goes_with in refused(100, 100, "--pairs-lanes", 16)
    assert goes_with in refused("--fasta", q, db, "--pairs-lanes", 32)
    assert goes_with in refused("--pairs", pairs, "--pairs-lanes", 16)
    # --search-lanes keeps its refusals beside the new flag
    not_with = "--search-lanes does not go with --prefilter / --prefilter-hits / --pairs"
    assert not_with in refused("--search", q, db, "--all-queries", "--pairs", pairs, *scoring, "--search-lanes", 16, "--pairs-lanes", 16)
    assert not_with in refused("--search", q, db, "--all-queries", *scoring, "--prefilter-hits", 30, "--search-lanes", 16, "--pairs-lanes", 16)
