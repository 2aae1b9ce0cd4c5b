"""GPU: smithW --weight-hits P (with --iterations N / --out-pssm): stdout but for the line of timings equals, byte for byte, the
rendering of the Python chain of host legs with pssm_hit_weights_host between the alignment and the update of every round, the files of
--out-pssm read back equal to the chain's matrices and differ from the unweighted run's, the flag is refused outside 1..65535 and
without the iteration flags, and without it the program prints what it printed before."""
import numpy as np
import pytest

import pssm_cases
import pssm_hits_cases as hc
from affine_cases import PROTEIN
from test_pssm_hits_cli_gpu import GE, GO, TOP, before_timings, rendering, run, sequence_world
from test_pssm_hits_cli_gpu import chain as unweighted_chain

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Three queries; per query a family of three copies of one homologue beside one distinct homologue, in random targets."""
    rng = np.random.default_rng(62)
    d = tmp_path_factory.mktemp("cli_weights")
    alpha = PROTEIN[:20]
    queries = [rng.choice(alpha, n).astype(np.uint8) for n in (63, 130, 40)]
    packed, offs = hc.homologue_database(rng, queries, 30, copies=1)
    targets = [packed[offs[k]:offs[k + 1]] for k in range(len(offs) - 1) if offs[k + 1] > offs[k]]   # (a FASTA file has no empty record)
    for qs in queries:
        targets += [hc.mutate(rng, qs, alpha)] * 3
    for name, seqs in (("q.fa", queries), ("db.fa", targets)):
        with open(d / name, "w") as f:
            for k, s in enumerate(seqs):
                f.write(f">rec{k}\n" + bytes(s).decode() + "\n")
    return d, str(d / "q.fa"), str(d / "db.fa"), queries, targets


def chain(swamd, m0, qoffs, targets, scoring, sub, iterations, prior_weight, include_score, per_hit):
    """(matrix of the last search, its hits, counts, alignments, ops, the weights of the last update) of the host legs chained."""
    m, w = m0, None
    for it in range(iterations):
        if it > 0:
            w = swamd.pssm_hit_weights_host(qoffs, targets, scoring, (per_hit, include_score), hits, nhits, aln, ops)
            m = swamd.pssm_from_hits_host((m0, qoffs), targets, scoring, (sub, prior_weight, include_score), hits, nhits, aln, ops, weights=w)
        hits, nhits = pssm_cases.rank_order(swamd.search_pssm_multi_host((m, qoffs), targets, scoring), min(TOP, len(targets)), 0)
        aln, ops = swamd.align_pssm_hits_host((m, qoffs), targets, scoring, hits, nhits)
    return m, hits, nhits, aln, ops, w


def test_weighted_iterations_print_the_lines_of_the_python_chain(swamd, files):
    d, qfa, dbfa, queries, targets = files
    letters, sub, m0, qoffs, scoring = sequence_world(swamd, files)
    m1, hits, nhits, aln, ops, w = chain(swamd, m0, qoffs, targets, scoring, sub, 2, 160, 1, 16)
    plain = unweighted_chain(swamd, m0, qoffs, targets, scoring, sub, 2, 10, 1)[0]
    assert len(set(w[w > 0].tolist())) > 1 and (m1 != plain).any()          # the weights differ among the hits and change the matrix
    base = ["--search", qfa, dbfa, "--all-queries", "--gap-open", GO, "--gap-extend", GE, "--top", TOP]
    for align in (False, True):
        r = run(*base, "--iterations", 2, "--weight-hits", 16, "--prior-weight", 160, "--out-pssm", d / "w2", *(["--align"] if align else []))
        assert r.returncode == 0, r.stderr
        assert before_timings(r.stdout) == rendering(swamd, qfa, queries, qoffs, targets, hits, nhits, aln, ops, align), align
    for q in range(len(queries)):
        lt, back = swamd.read_pssm(str(d / f"w2.{q}.pssm"))
        assert (lt == letters).all() and (back == m1[qoffs[q]:qoffs[q + 1]]).all(), q
    # three rounds, another threshold and unit
    m2, hits, nhits, aln, ops, _ = chain(swamd, m0, qoffs, targets, scoring, sub, 3, 7, 40, 3)
    r = run(*base, "--iterations", 3, "--weight-hits", 3, "--prior-weight", 7, "--include-score", 40, "--align")
    assert r.returncode == 0, r.stderr
    assert before_timings(r.stdout) == rendering(swamd, qfa, queries, qoffs, targets, hits, nhits, aln, ops, True)


def test_without_the_flag_the_output_is_unchanged(swamd, files):
    """The unweighted run equals the unweighted chain -- what the program printed before the flag existed --, --out-pssm included; and
    --weight-hits with --out-pssm alone (one round: no update happens) prints the lines of that one round."""
    d, qfa, dbfa, queries, targets = files
    letters, sub, m0, qoffs, scoring = sequence_world(swamd, files)
    base = ["--search", qfa, dbfa, "--all-queries", "--gap-open", GO, "--gap-extend", GE, "--top", TOP, "--align"]
    m1, hits, nhits, aln, ops = unweighted_chain(swamd, m0, qoffs, targets, scoring, sub, 2, 10, 1)
    r = run(*base, "--iterations", 2, "--out-pssm", d / "plain")
    assert r.returncode == 0, r.stderr
    assert before_timings(r.stdout) == rendering(swamd, qfa, queries, qoffs, targets, hits, nhits, aln, ops, True)
    assert all((swamd.read_pssm(str(d / f"plain.{q}.pssm"))[1] == m1[qoffs[q]:qoffs[q + 1]]).all() for q in range(len(queries)))
    one, flagged = run(*base, "--out-pssm", d / "one"), run(*base, "--out-pssm", d / "one_w", "--weight-hits", 16)
    assert one.returncode == 0 and flagged.returncode == 0, (one.stderr, flagged.stderr)
    assert before_timings(one.stdout) == before_timings(flagged.stdout)


def test_refused_flags(files):
    d, qfa, dbfa, _, _ = files
    base = ["--search", qfa, dbfa, "--all-queries", "--gap-open", GO, "--gap-extend", GE]
    for flags, word in ((("--iterations", 2, "--weight-hits", 0), "1..65535"), (("--iterations", 2, "--weight-hits", 65536), "1..65535"),
                        (("--iterations", 2, "--weight-hits", -4), "1..65535"), (("--weight-hits", 16), "goes with --iterations"),
                        (("--iterations", 1, "--weight-hits", 16), "goes with --iterations")):
        r = run(*base, *flags)
        assert r.returncode == 2 and word in r.stderr and r.stdout == "", (flags, r.stderr)
    r = run("--search", qfa, dbfa, "--weight-hits", 16, "--iterations", 2)
    assert r.returncode == 2 and r.stdout == ""
