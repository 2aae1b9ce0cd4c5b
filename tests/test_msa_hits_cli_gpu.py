"""GPU: smithW --out-a3m PREFIX (with --search Q.fa DB.fa --all-queries, with and without --iterations 2, and with --search --pssm FILE
DB.fa) on a 3-query, 40-target FASTA written here: every PREFIX.<query>.a3m, parsed back, is the query's record (none for a matrix)
and, per hit at or above --include-score, the header and the A3M row Database.msa_from_hits gives for the tables of the Python chain of
host legs; every row has one byte that is not lower case per query column; stdout is what it is without the flag."""
import os
import subprocess

import numpy as np
import pytest

import pssm_cases
from affine_cases import PROTEIN
from oracle_lib import ROOT
from pssm_hits_cases import mutate

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "smith-waterman_amd", "smithW")
GO, GE, TOP, INCLUDE = -6, -1, 6, 40


def run(*args):
    return subprocess.run([CLI, *[str(a) for a in args]], capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    rng = np.random.default_rng(71)
    d = tmp_path_factory.mktemp("cli_a3m")
    alpha = PROTEIN[:20]
    queries = [rng.choice(alpha, n).astype(np.uint8) for n in (63, 130, 40)]
    targets = [rng.choice(alpha, int(n)).astype(np.uint8) for n in rng.integers(2, 300, 31)]
    for qs in queries:
        for _ in range(3):
            targets.append(np.concatenate([rng.choice(alpha, int(rng.integers(0, 40))).astype(np.uint8), mutate(rng, qs, alpha),
                                           rng.choice(alpha, int(rng.integers(0, 40))).astype(np.uint8)]))
    targets = [targets[k] for k in rng.permutation(len(targets))]
    assert len(queries) == 3 and len(targets) == 40
    for name, tag, seqs in (("q.fa", "qry", queries), ("db.fa", "rec", targets)):
        with open(d / name, "w") as f:
            for k, s in enumerate(seqs):
                f.write(f">{tag}{k} some description\n" + bytes(s).decode() + "\n")
    return d, str(d / "q.fa"), str(d / "db.fa"), queries, targets


def chain(swamd, m0, qoffs, targets, scoring, sub, iterations):
    """The tables of the last round of the host legs chained: (hits, counts, alignments, ops)."""
    m = m0
    for it in range(iterations):
        if it > 0:
            m = swamd.pssm_from_hits_host((m0, qoffs), targets, scoring, (sub, 10, INCLUDE), hits, nhits, aln, ops)
        hits, nhits = pssm_cases.rank_order(swamd.search_pssm_multi_host((m, qoffs), targets, scoring), TOP, 0)
        aln, ops = swamd.align_pssm_hits_host((m, qoffs), targets, scoring, hits, nhits)
    return hits, nhits, aln, ops


def expected_files(engine, queries_or_qoffs, records, targets, tables):
    """Per query the lines of its file, from Database.msa_from_hits on the chain's tables."""
    hits, nhits, aln, ops = tables
    with engine.prepare_db(targets) as db:
        cols, rows, a3m = db.msa_from_hits(queries_or_qoffs, INCLUDE, hits, nhits, aln, ops)
    out = []
    for q in range(len(rows)):
        lines = list(records[q])
        for r in range(rows.shape[1]):
            off, ln, nm, ni, nins = (int(x) for x in rows[q, r])
            if ln:
                a = aln[q, r]
                lines += [f">rec{int(hits[q, r, 0])} score={a[1]} q={a[2]}-{a[4]} t={a[3]}-{a[5]} ident={ni}/{nm}", bytes(a3m[off:off + ln]).decode()]
        out.append(lines)
    assert sum(len(x) for x in out) - sum(len(x) for x in records) >= 6      # hits were written ...
    assert (rows["len"] == 0).any() and (rows["ninsert"] > 0).any()          # ... some were left out, and some rows hold inserts
    return out


def check_files(d, prefix, exp, qlens, with_record):
    for q, lines in enumerate(exp):
        got = open(d / f"{prefix}.{q}.a3m").read()
        assert got.endswith("\n") and got[:-1].split("\n") == lines, (prefix, q)
        body = got[:-1].split("\n")[1::2]
        assert len(body) == (len(lines) // 2) and (not with_record or body[0].isupper())
        for row in body:                                                     # every non-lower-case row length equals the query length
            assert sum(not c.islower() for c in row) == qlens[q]


def sequence_world(swamd, files):
    d, qfa, dbfa, queries, targets = files
    letters = np.unique(np.concatenate(queries + targets))
    sub = swamd.submat_match(3, -3)
    m0, qoffs = swamd.pssm_from_queries(queries, sub, letters)
    return sub, m0, qoffs, (letters, -3, 3, GO, GE)


@pytest.mark.parametrize("iterations", [None, 2])
def test_sequence_queries(swamd, engine, files, iterations):
    d, qfa, dbfa, queries, targets = files
    sub, m0, qoffs, scoring = sequence_world(swamd, files)
    tables = chain(swamd, m0, qoffs, targets, scoring, sub, iterations or 1)
    records = [[f">qry{q}", bytes(s).decode()] for q, s in enumerate(queries)]
    exp = expected_files(engine, queries, records, targets, tables)
    assert all(int(ident.split("=")[-1].split("/")[0]) > 0 for lines in exp for ident in lines[2::2])     # identities are counted against the letters
    base = ["--search", qfa, dbfa, "--all-queries", "--gap-open", GO, "--gap-extend", GE, "--top", TOP, "--align", "--include-score", INCLUDE]
    base += ["--iterations", iterations] if iterations else []
    prefix = f"seq{iterations}"
    r, plain = run(*base, "--out-a3m", d / prefix), run(*base)
    assert r.returncode == 0 and plain.returncode == 0, (r.stderr, plain.stderr)
    cut = lambda text: text[:text.index("Elapsed time for database search:")]
    assert cut(r.stdout) == cut(plain.stdout)                                # the flag adds files, not lines
    check_files(d, prefix, exp, [len(s) for s in queries], True)


def test_a_pssm_file_has_no_query_record(swamd, engine, files):
    d, qfa, dbfa, queries, targets = files
    letters0 = np.unique(np.concatenate(queries + targets))
    m0, qoffs0 = swamd.pssm_from_queries(queries, swamd.submat_match(3, -3), letters0)
    p = str(d / "q1.pssm")
    swamd.write_pssm(p, letters0, m0[qoffs0[1]:qoffs0[2]], queries[1])
    letters, m = swamd.read_pssm(p)
    scoring = (letters, min(int(m.min()), 0), max(int(m.max()), 0), GO, GE)
    qoffs = np.array([0, len(m)], np.int64)
    tables = chain(swamd, m, qoffs, targets, scoring, swamd.submat_match(2, -4), 2)
    exp = expected_files(engine, qoffs, [[]], targets, tables)
    assert all(ident.endswith("ident=0/" + ident.split("/")[-1]) for ident in exp[0][0::2])               # a matrix has no letters: no identities
    r = run("--search", "--pssm", p, dbfa, "--gap-open", GO, "--gap-extend", GE, "--top", TOP, "--iterations", 2, "--scores", 2, -4, -2, "--align",
            "--include-score", INCLUDE, "--out-a3m", d / "pssm")
    assert r.returncode == 0, r.stderr
    got = open(d / "pssm.0.a3m").read()
    assert got[:-1].split("\n") == exp[0] and got.startswith(">rec")
    for row in exp[0][1::2]:
        assert sum(not c.islower() for c in row) == len(m)


def test_refused_flags(files):
    d, qfa, dbfa, _, _ = files
    r = run("--search", qfa, dbfa, "--all-queries", "--gap-open", GO, "--gap-extend", GE, "--out-a3m", d / "x")
    assert r.returncode == 2 and "--align" in r.stderr and r.stdout == ""
    r = run("--search", qfa, dbfa, "--align", "--out-a3m", d / "x")
    assert r.returncode == 2 and "go with --search --all-queries or --search --pssm" in r.stderr
