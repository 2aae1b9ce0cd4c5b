"""GPU: smithW --search Q.fa DB.fa --all-queries --prefilter-hits S prints the blocks of --all-queries with
sw_db_search_affine_top_prefiltered in the place of sw_db_search_affine_top.  With S = 1 and --min-score 1 the two print the same hit
and alignment lines; with a real threshold the hits are those of the Python chain.  A count beyond the list is left to
tests/test_top_pairs_gpu.py: the command line has no switch that makes the list smaller than queries x records, short of 19 million
pairs."""
import os
import subprocess

import numpy as np
import pytest

from affine_cases import PROTEIN
from oracle_lib import ROOT

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "smith-waterman_amd", "smithW")
GAPS = ("--gap-open", -5, "--gap-extend", -1)


def run(*args):
    return subprocess.run([CLI, *[str(a) for a in args]], capture_output=True, text=True, timeout=120)


def fasta(path, seqs):
    with open(path, "w") as f:
        for k, s in enumerate(seqs):
            f.write(f">rec{k}\n{bytes(s).decode()}\n")


def body(text):
    """Everything but the elapsed line."""
    return [ln for ln in text.splitlines() if not ln.startswith("Elapsed")]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Four queries against 24 targets among which every target occurs twice: ties at every rank."""
    rng = np.random.default_rng(37)
    d = tmp_path_factory.mktemp("cli_top_pairs")
    letters = PROTEIN[:20]
    queries = [rng.choice(letters, n).astype(np.uint8) for n in (12, 40, 90, 300)]
    distinct = [rng.choice(letters, int(n)).astype(np.uint8) for n in rng.integers(10, 120, 9)] + [q[2:].copy() for q in queries[1:]]
    targets = distinct + distinct[::-1]
    fasta(d / "q.fa", queries)
    fasta(d / "db.fa", targets)
    return str(d / "q.fa"), str(d / "db.fa"), queries, targets


@pytest.mark.parametrize("extra", [(), ("--align",), ("--align", "--align-checkpoint")], ids=["hits", "align", "align-checkpoint"])
def test_threshold_one_prints_what_all_queries_prints(files, extra):
    q, db, queries, targets = files
    for top in (3, len(targets)):
        want = run("--search", q, db, "--all-queries", "--top", top, "--min-score", 1, *GAPS, *extra)
        got = run("--search", q, db, "--all-queries", "--prefilter-hits", 1, "--top", top, "--min-score", 1, *GAPS, *extra)
        assert want.returncode == 0 and got.returncode == 0, got.stderr
        assert body(got.stdout) == body(want.stdout)
        assert sum(ln.startswith("## query record") for ln in body(got.stdout)) == len(queries)
        assert (sum(ln.startswith("align\t") for ln in body(got.stdout)) > len(queries)) == bool(extra)
    line = [ln for ln in got.stdout.splitlines() if ln.startswith("Elapsed")]
    assert len(line) == 1 and "pairs passed the pre-filter U >= 1" in line[0]


def test_a_real_threshold_prints_the_hits_of_the_python_chain(files, swamd, engine):
    q, db, queries, targets = files
    sub = swamd.submat_match(3, -3)
    scoring = (sub, -5, -1)
    with engine.prepare_db([t.tobytes() for t in targets]) as handle:
        _, u = handle.prefilter_ungapped([x.tobytes() for x in queries], sub, 1)
        S = int(np.sort(u[u > 0])[(u > 0).sum() * 3 // 4])                        # a quarter of the scoring pairs pass
        hits, nhits, npairs = handle.search_affine_top_prefiltered([x.tobytes() for x in queries], scoring, S, 5, 2)
    assert 0 < npairs == int((u >= S).sum()) < (u > 0).sum()
    r = run("--search", q, db, "--all-queries", "--prefilter-hits", S, "--top", 5, "--min-score", 2, *GAPS)
    assert r.returncode == 0, r.stderr
    rows, k = [], -1
    for ln in body(r.stdout):
        if ln.startswith("## query record"):
            k += 1
            rows.append([])
        elif ln[:1].isdigit():
            rank, rec, score, te, qe = (int(x) for x in ln.split("\t"))
            rows[k].append((rec, te * (len(queries[k]) + 1) + qe, score))
            assert rank == len(rows[k])
    assert len(rows) == len(queries)
    for k in range(len(queries)):
        assert rows[k] == [tuple(h) for h in hits[k, :nhits[k]].tolist()], f"record {k}"
    assert f"{npairs} of {len(queries) * len(targets)} pairs passed the pre-filter U >= {S}" in r.stdout


def test_usage_errors(files):
    q, db, _, targets = files
    bad = [
        (("--search", q, db, "--all-queries", "--prefilter-hits", 0), "--prefilter-hits S needs S >= 1"),
        (("--search", q, db, "--all-queries", "--prefilter-hits", -4), "--prefilter-hits S needs S >= 1"),
        (("--search", q, db, "--prefilter-hits", 5), "--prefilter-hits goes with --search --all-queries"),
        (("100", "100", "--prefilter-hits", 5), "--prefilter-hits goes with --search --all-queries"),
        (("--search", q, db, "--all-queries", "--prefilter-hits", 5, "--prefilter", 5), "--prefilter-hits does not go with --prefilter"),
        (("--search", q, db, "--all-queries", "--prefilter-hits", 5, "--pairs", q), "--prefilter-hits does not go with --pairs"),
        (("--search", q, db, "--prefilter-hits", 5, "--pairs", q), "--prefilter-hits goes with --search --all-queries"),
    ]
    for args, word in bad:
        r = run(*args)
        assert r.returncode == 2 and word in r.stderr and "usage:" not in r.stderr and r.stdout == "", (args, r.stderr)
    assert run("--search", q, db, "--all-queries", "--prefilter-hits", "x").returncode == 2


def test_more_hits_than_the_device_selects(tmp_path):
    """min(K, records) above SW_TOP_MAX: the long way of --all-queries has no pair list to select from."""
    rng = np.random.default_rng(4)
    fasta(tmp_path / "q.fa", [rng.choice(PROTEIN[:20], 8).astype(np.uint8)])
    fasta(tmp_path / "db.fa", [rng.choice(PROTEIN[:20], 4).astype(np.uint8) for _ in range(4097)])
    r = run("--search", tmp_path / "q.fa", tmp_path / "db.fa", "--all-queries", "--prefilter-hits", 3, "--top", 5000)
    assert r.returncode == 2 and "4097 is above 4096" in r.stderr and "usage:" not in r.stderr and r.stdout == ""
    r = run("--search", tmp_path / "q.fa", tmp_path / "db.fa", "--all-queries", "--prefilter-hits", 3, "--top", 4096)
    assert r.returncode == 0 and "## query record 0" in r.stdout
