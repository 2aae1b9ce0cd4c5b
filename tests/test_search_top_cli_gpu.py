"""GPU: smithW --search Q.fa DB.fa --all-queries selects its hits on the device (sw_db_search_affine_top).  The existing tests pin the
format; this pins the new path against the one-query path, which sorts the whole row on the host, and --min-score against it."""
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
            f.write(f">rec{k}\n{bytes(s).decode()}\n")


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
    """Four queries against 24 targets among which every target occurs twice: ties at every rank."""
    rng = np.random.default_rng(31)
    d = tmp_path_factory.mktemp("cli_top")
    letters = PROTEIN[:20]
    queries = [rng.choice(letters, n).astype(np.uint8) for n in (12, 40, 90, 300)]
    distinct = [rng.choice(letters, int(n)).astype(np.uint8) for n in rng.integers(10, 120, 9)] + [q[2:].copy() for q in queries[1:]]
    targets = distinct + distinct[::-1]
    fasta(d / "q.fa", queries)
    fasta(d / "db.fa", targets)
    return str(d / "q.fa"), str(d / "db.fa"), len(queries), len(targets)


@pytest.mark.parametrize("extra", [(), ("--gap-open", -5, "--gap-extend", -1, "--align")])
def test_all_queries_top_3_equals_one_query_runs(files, extra):
    q, db, nq, _ = files
    r = run("--search", q, db, "--all-queries", "--top", 3, *extra)
    assert r.returncode == 0, r.stderr
    got = blocks(r.stdout)
    assert len(got) == nq
    for k in range(nq):
        one = run("--search", q, db, "--record-a", k, "--top", 3, *extra)
        assert one.returncode == 0, one.stderr
        want = blocks(one.stdout)
        assert len(want) == 1 and len(want[0]) == (1 + 3 * (5 if extra else 1)) and got[k] == want[0], f"record {k}"


def test_min_score_drops_exactly_the_hits_below_it(files):
    q, db, nq, nt = files
    full = blocks(run("--search", q, db, "--all-queries", "--top", nt).stdout)
    assert len(full) == nq and all(len(b) == 1 + nt for b in full)
    scores = sorted(int(ln.split("\t")[2]) for b in full for ln in b[1:])
    cut = scores[len(scores) // 2]
    assert scores[0] < cut <= scores[-1]
    r = run("--search", q, db, "--all-queries", "--top", nt, "--min-score", cut)
    assert r.returncode == 0, r.stderr
    got = blocks(r.stdout)
    for k in range(nq):
        want = [full[k][0]] + [ln for ln in full[k][1:] if int(ln.split("\t")[2]) >= cut]
        assert got[k] == want, f"record {k}"
    assert sum(len(b) - 1 for b in got) < nq * nt
    none = blocks(run("--search", q, db, "--all-queries", "--top", 5, "--min-score", scores[-1] + 1).stdout)
    assert [len(b) for b in none] == [1] * nq                                  # only the header lines


def test_min_score_usage(files):
    q, db, _, _ = files
    r = run("--search", q, db, "--min-score", 5)
    assert r.returncode == 2 and "--all-queries" in r.stderr
    assert run("--search", q, db, "--all-queries", "--min-score", "x").returncode == 2
    assert run("100", "100", "--min-score", 5).returncode == 2
