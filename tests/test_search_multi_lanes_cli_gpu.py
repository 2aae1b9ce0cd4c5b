"""GPU: smithW --search-lanes 16|32 (option "search_lanes"): with --all-queries and with --pssm the lines printed under 16 are the lines
of the same command without the flag; other values and other modes are refused with a message before any device work."""
import os
import subprocess

import numpy as np
import pytest

import pssm_cases
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
    rng = np.random.default_rng(53)
    d = tmp_path_factory.mktemp("cli_lanes")
    letters = PROTEIN[:20]
    queries = [rng.choice(letters, n).astype(np.uint8) for n in (30, 300, 600, 1100)]          # all three classes
    targets = [rng.choice(letters, int(n)).astype(np.uint8) for n in (50, 7, 200, 64, 400, 33, 90)]   # an odd number: the last rank runs alone
    targets[2] = np.concatenate([targets[2][:40], queries[1][20:200], targets[2][40:]])        # a related pair: a long diagonal
    targets[6][10:50] = queries[2][500:540]                                                   # and a short one
    fasta(d / "q.fa", queries, "query")
    fasta(d / "db.fa", targets, "rec")
    with open(d / "m.txt", "w") as f:                              # a small NCBI-format table: matches 5, mismatches -2 .. -4
        ls = [chr(c) for c in letters]
        f.write("# test table\n   " + "  ".join(ls) + "\n")
        for i, a in enumerate(ls):
            f.write(a + " " + " ".join(str(5 if i == j else -2 - (i + 2 * j) % 3) for j in range(len(ls))) + "\n")
    m = rng.integers(-6, 3, (70, 20)).astype(np.int8)
    residue = rng.integers(0, 20, 70)
    m[np.arange(70), residue] = rng.integers(4, 10, 70).astype(np.int8)
    pssm_cases.write_ascii_pssm(d / "p.pssm", letters, m, letters[residue])
    return str(d / "q.fa"), str(d / "db.fa"), str(d / "m.txt"), str(d / "p.pssm")


def before_timings(text):
    at = text.index("Elapsed time for database search:")
    assert text[at:].count("\n") == 2 and text.endswith("\n\n")                         # the line of timings and a blank line end the output
    return text[:at]


def test_all_queries_prints_the_same_lines(files):
    q, db, m, _ = files
    base = ("--search", q, db, "--all-queries", "--matrix", m, "--gap-open", -11, "--gap-extend", -1, "--top", 3)
    plain = run(*base)
    assert plain.returncode == 0, plain.stderr
    want = before_timings(plain.stdout)
    assert want.count("## query record") == 4 and "\n1\t2\t" in want                    # the planted target leads its query's block
    for lanes in (16, 32):
        r = run(*base, "--search-lanes", lanes)
        assert r.returncode == 0, r.stderr
        assert before_timings(r.stdout) == want, lanes
    r = run(*base, "--align", "--search-lanes", 16)                                     # the hit table under 16 feeds the alignments unchanged
    assert r.returncode == 0 and before_timings(r.stdout) == before_timings(run(*base, "--align").stdout)


def test_pssm_prints_the_same_lines(files):
    _, db, _, p = files
    base = ("--search", "--pssm", p, db, "--gap-open", -11, "--gap-extend", -1, "--top", 3)
    plain = run(*base)
    assert plain.returncode == 0, plain.stderr
    for lanes in (16, 32):
        r = run(*base, "--search-lanes", lanes)
        assert r.returncode == 0, r.stderr
        assert before_timings(r.stdout) == before_timings(plain.stdout), lanes


def test_refusals_come_before_any_device_work(files):
    q, db, m, p = files
    scoring = ("--matrix", m, "--gap-open", -11, "--gap-extend", -1)
    env_without_a_device = {**os.environ, "HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"}

    def refused(*args):
        r = subprocess.run([CLI, *[str(a) for a in args]], capture_output=True, text=True, timeout=120, env=env_without_a_device)
        assert r.returncode == 2 and r.stdout == "" and "usage:" not in r.stderr, (args, r.stderr)
        return r.stderr

    for v in (8, 0, 64):
        assert f"--search-lanes takes 16 or 32, got {v}" in refused("--search", q, db, "--all-queries", *scoring, "--search-lanes", v)
        assert f"--search-lanes takes 16 or 32, got {v}" in refused("--search", "--pssm", p, db, "--gap-open", -11, "--gap-extend", -1, "--search-lanes", v)
    assert "--search-lanes needs an integer" in refused("--search", q, db, "--all-queries", *scoring, "--search-lanes", "wide")
    goes_with = "--search-lanes goes with --search --all-queries or --search --pssm"
    assert goes_with in refused("--search", q, db, *scoring, "--search-lanes", 16)      # one query: its own kernel and schedule
    assert goes_with in refused(100, 100, "--search-lanes", 16)
    assert goes_with in refused("--fasta", q, db, "--search-lanes", 32)
    not_with = "--search-lanes does not go with --prefilter / --prefilter-hits / --pairs"
    assert not_with in refused("--search", q, db, "--all-queries", *scoring, "--prefilter", 5, "--search-lanes", 16)
    assert not_with in refused("--search", q, db, "--all-queries", *scoring, "--prefilter-hits", 5, "--search-lanes", 16)
    assert not_with in refused("--search", q, db, "--all-queries", "--pairs", m, *scoring, "--search-lanes", 16)
    assert goes_with in refused("--search", q, db, "--pairs", m, *scoring, "--search-lanes", 16)      # a pair list is not a many-query search
