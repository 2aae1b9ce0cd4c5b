"""GPU: smithW --iterations N (with --search Q.fa DB.fa --all-queries and with --search --pssm FILE DB.fa): stdout but for the line of
timings equals, byte for byte, the rendering of the Python chain of host legs -- pssm_from_queries, then per round search_pssm_multi_host,
the rank order, align_pssm_hits_host and pssm_from_hits_host with the iteration-0 matrix as prior --, the files of --out-pssm read back
equal to the chain's matrices, and --iterations 1 prints the lines of today."""
import os
import subprocess

import numpy as np
import pytest

import pssm_cases
import pssm_hits_cases as cases
from affine_cases import PROTEIN
from oracle_lib import ROOT

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "smith-waterman_amd", "smithW")
GO, GE, TOP = -6, -1, 5


def run(*args):
    return subprocess.run([CLI, *[str(a) for a in args]], capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    rng = np.random.default_rng(61)
    d = tmp_path_factory.mktemp("cli_iter")
    queries = [rng.choice(PROTEIN[:20], n).astype(np.uint8) for n in (63, 130, 40)]
    packed, offs = cases.homologue_database(rng, queries, 30)
    targets = [packed[offs[k]:offs[k + 1]] for k in range(len(offs) - 1) if offs[k + 1] > offs[k]]   # (a FASTA file has no empty record)
    for name, seqs in (("q.fa", queries), ("db.fa", targets)):
        with open(d / name, "w") as f:
            for k, s in enumerate(seqs):
                f.write(f">rec{k}\n" + bytes(s).decode() + "\n")
    return d, str(d / "q.fa"), str(d / "db.fa"), queries, targets


def chain(swamd, m0, qoffs, targets, scoring, sub, iterations, prior_weight, include_score):
    """(matrix of the last search, its hits, counts, alignments, ops) of the host legs chained."""
    m = m0
    for it in range(iterations):
        if it > 0:
            m = swamd.pssm_from_hits_host((m0, qoffs), targets, scoring, (sub, prior_weight, include_score), hits, nhits, aln, ops)
        hits, nhits = pssm_cases.rank_order(swamd.search_pssm_multi_host((m, qoffs), targets, scoring), min(TOP, len(targets)), 0)
        aln, ops = swamd.align_pssm_hits_host((m, qoffs), targets, scoring, hits, nhits)
    return m, hits, nhits, aln, ops


def rendering(swamd, path, lines_q, qoffs, targets, hits, nhits, aln, ops, align):
    out = []
    for q in range(len(qoffs) - 1):
        qlen = int(qoffs[q + 1] - qoffs[q])
        out += [f"## query record {q} of {path}",
                f"# query {qlen} letters, {len(targets)} targets, {sum(len(t) for t in targets)} letters; rank\trecord\tscore\ttarget_end\tquery_end"]
        for r in range(int(nhits[q])):
            k, pos, score = (int(x) for x in hits[q, r])
            out.append(f"{r + 1}\t{k}\t{score}\t{pos // (qlen + 1)}\t{pos % (qlen + 1)}")
            if align:
                a = aln[q, r]
                out.append(f"align\t{a[2]}\t{a[4]}\t{a[3]}\t{a[5]}\t{a[6]}")
                lq, lm, lt = swamd.format_alignment(lines_q[q], targets[k], a, ops[q][r])
                out += [f"Q {lq}", f"  {lm}", f"T {lt}"]
    return "\n".join(out) + "\n\n"


def before_timings(text):
    at = text.index("Elapsed time for database search:")
    assert text[at:].count("\n") == 2 and text.endswith("\n\n")
    return text[:at]


def sequence_world(swamd, files):
    d, qfa, dbfa, queries, targets = files
    letters = np.unique(np.concatenate(queries + targets))                 # the distinct bytes of database and queries, ascending
    sub = swamd.submat_match(3, -3)
    m0, qoffs = swamd.pssm_from_queries(queries, sub, letters)
    s = np.asarray(sub, np.int64).reshape(256, 256)[np.ix_(letters, letters)]
    return letters, sub, m0, qoffs, (letters, min(int(s.min()), 0), max(int(s.max()), 0), GO, GE)


def test_two_iterations_print_the_lines_of_the_python_chain(swamd, files):
    d, qfa, dbfa, queries, targets = files
    letters, sub, m0, qoffs, scoring = sequence_world(swamd, files)
    first = chain(swamd, m0, qoffs, targets, scoring, sub, 1, 10, 1)
    m1, hits, nhits, aln, ops = chain(swamd, m0, qoffs, targets, scoring, sub, 2, 10, 1)
    assert (m1 != m0).any() and (hits != first[1]).any()                   # the second round is another search
    for align in (False, True):
        r = run("--search", qfa, dbfa, "--all-queries", "--gap-open", GO, "--gap-extend", GE, "--top", TOP, "--iterations", 2, "--out-pssm", d / "it2",
                *(["--align"] if align else []))
        assert r.returncode == 0, r.stderr
        assert before_timings(r.stdout) == rendering(swamd, qfa, queries, qoffs, targets, hits, nhits, aln, ops, align), align
    for q in range(len(queries)):                                           # the files read back equal to the chain's matrices
        lt, back = swamd.read_pssm(str(d / f"it2.{q}.pssm"))
        assert (lt == letters).all() and (back == m1[qoffs[q]:qoffs[q + 1]]).all(), q
        assert [x.split()[1] for x in open(d / f"it2.{q}.pssm").read().splitlines()[3:3 + len(back)]] == [chr(b) for b in queries[q]]
    # other weights, another threshold, three rounds
    m2, hits, nhits, aln, ops = chain(swamd, m0, qoffs, targets, scoring, sub, 3, 2, 40)
    r = run("--search", qfa, dbfa, "--all-queries", "--gap-open", GO, "--gap-extend", GE, "--top", TOP, "--iterations", 3, "--prior-weight", 2, "--include-score", 40,
            "--align")
    assert r.returncode == 0, r.stderr
    assert before_timings(r.stdout) == rendering(swamd, qfa, queries, qoffs, targets, hits, nhits, aln, ops, True)


def test_one_iteration_prints_the_lines_of_today(swamd, files):
    d, qfa, dbfa, queries, targets = files
    base = ["--search", qfa, dbfa, "--all-queries", "--gap-open", GO, "--gap-extend", GE, "--top", TOP, "--align"]
    today, one = run(*base), run(*base, "--iterations", 1)
    assert today.returncode == 0 and one.returncode == 0, (today.stderr, one.stderr)
    assert before_timings(one.stdout) == before_timings(today.stdout)
    # ... and they are the lines of the chain's first round, also through the iterating path (--out-pssm writes the iteration-0 matrix)
    letters, sub, m0, qoffs, scoring = sequence_world(swamd, files)
    m, hits, nhits, aln, ops = chain(swamd, m0, qoffs, targets, scoring, sub, 1, 10, 1)
    assert before_timings(today.stdout) == rendering(swamd, qfa, queries, qoffs, targets, hits, nhits, aln, ops, True)
    r = run(*base, "--iterations", 1, "--out-pssm", d / "it1")
    assert r.returncode == 0 and before_timings(r.stdout) == before_timings(today.stdout), r.stderr
    assert (swamd.read_pssm(str(d / "it1.1.pssm"))[1] == m0[qoffs[1]:qoffs[2]]).all()


def test_a_pssm_file_iterates_too(swamd, files):
    d, qfa, dbfa, queries, targets = files
    letters0, sub, m0, qoffs0, _ = sequence_world(swamd, files)
    p = str(d / "q1.pssm")
    swamd.write_pssm(p, letters0, m0[qoffs0[1]:qoffs0[2]], queries[1])
    letters, m = swamd.read_pssm(p)
    scoring = (letters, min(int(m.min()), 0), max(int(m.max()), 0), GO, GE)
    qoffs = np.array([0, len(m)], np.int64)
    m1, hits, nhits, aln, ops = chain(swamd, m, qoffs, targets, scoring, swamd.submat_match(2, -4), 2, 10, 1)
    r = run("--search", "--pssm", p, dbfa, "--gap-open", GO, "--gap-extend", GE, "--top", TOP, "--iterations", 2, "--scores", 2, -4, -2, "--align", "--out-pssm",
            d / "p2")
    assert r.returncode == 0, r.stderr
    consensus = bytes(letters[np.argmax(m1, axis=1)])
    assert before_timings(r.stdout) == rendering(swamd, p, [consensus], qoffs, targets, hits, nhits, aln, ops, True)
    assert (swamd.read_pssm(str(d / "p2.0.pssm"))[1] == m1).all()


def test_refused_flags(files):
    d, qfa, dbfa, _, _ = files
    base = ["--search", qfa, dbfa, "--all-queries", "--gap-open", GO, "--gap-extend", GE]
    for flags, word in ((("--iterations", 0), "N >= 1"), (("--iterations", 2, "--prior-weight", 65536), "0..65535"), (("--iterations", 2, "--prefilter-hits", 5), "does not go with"),
                        (("--iterations", 2, "--top", 0), "device hit table")):
        r = run(*base, *flags)
        assert r.returncode == 2 and word in r.stderr and r.stdout == "", (flags, r.stderr)
    r = run("--search", qfa, dbfa, "--iterations", 2)
    assert r.returncode == 2 and "go with --search --all-queries or --search --pssm" in r.stderr
