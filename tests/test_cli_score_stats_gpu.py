"""GPU: smithW --evalue E and --include-evalue E.  --evalue prints, per query, exactly the hits of the plain run whose E-value under
the Python chain's fit is at most E, each line with its " E=" field, ranks recounted, alignments following their hits; with
--include-evalue the files of --out-pssm hold the bytes of the Python chain of host legs that thresholds a copy of every round's hit
table (score_hist_host, score_fit, score_thresholds, hits_threshold_host) and builds the next matrix from it with include_min_score
at its minimum; --score-shift takes the histogram at that shift; with --pssm the same; a command line without the new flags prints
what it printed before (the rendering of the unweighted chain)."""
import numpy as np
import pytest

import pssm_cases
import pssm_hits_cases as hc
from affine_cases import PROTEIN
from test_pssm_hits_cli_gpu import GE, GO, before_timings, rendering, run, sequence_world

pytestmark = pytest.mark.gpu

TOP = 12
INCLUDE_MIN = -(1 << 63)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Three queries with three mutated copies each among 150 random targets."""
    rng = np.random.default_rng(63)
    d = tmp_path_factory.mktemp("cli_score_stats")
    queries = [rng.choice(PROTEIN[:20], n).astype(np.uint8) for n in (63, 130, 40)]
    packed, offs = hc.homologue_database(rng, queries, 150)
    targets = [packed[offs[k]:offs[k + 1]] for k in range(len(offs) - 1) if offs[k + 1] > offs[k]]   # (a FASTA file has no empty record)
    for name, seqs in (("q.fa", queries), ("db.fa", targets)):
        with open(d / name, "w") as f:
            for k, s in enumerate(seqs):
                f.write(f">rec{k}\n" + bytes(s).decode() + "\n")
    return d, str(d / "q.fa"), str(d / "db.fa"), queries, targets


def search_round(swamd, m, qoffs, targets, scoring, shift):
    table = swamd.search_pssm_multi_host((m, qoffs), targets, scoring)
    hits, nhits = pssm_cases.rank_order(table, min(TOP, len(targets)), 0)
    aln, ops = swamd.align_pssm_hits_host((m, qoffs), targets, scoring, hits, nhits)
    fit = swamd.score_fit(swamd.score_hist_host(table, targets, shift), shift)
    return hits, nhits, aln, ops, fit


def chain(swamd, m0, qoffs, targets, scoring, sub, iterations, prior_weight, evalue, shift=0):
    """(matrix of the last search, its hits, counts, alignments, ops, fit) of the host legs chained, the inclusion by E-value."""
    m = m0
    for it in range(iterations):
        if it > 0:
            included = swamd.hits_threshold_host(targets, swamd.score_thresholds(fit, evalue), hits, nhits)[2]
            m = swamd.pssm_from_hits_host((m0, qoffs), targets, scoring, (sub, prior_weight, INCLUDE_MIN), included, nhits, aln, ops)
        hits, nhits, aln, ops, fit = search_round(swamd, m, qoffs, targets, scoring, shift)
    return m, hits, nhits, aln, ops, fit


def evalue_rendering(swamd, path, lines_q, qoffs, targets, hits, nhits, aln, ops, fit, evalue, align):
    """The rendering of --evalue: the lines of test_pssm_hits_cli_gpu.rendering for the kept hits, ranks recounted, " E=" appended."""
    keep = swamd.hits_threshold_host(targets, swamd.score_thresholds(fit, evalue), hits, nhits)[0]
    out = []
    for q in range(len(qoffs) - 1):
        qlen = int(qoffs[q + 1] - qoffs[q])
        out += [f"## query record {q} of {path}",
                f"# query {qlen} letters, {len(targets)} targets, {sum(len(t) for t in targets)} letters; rank\trecord\tscore\ttarget_end\tquery_end"]
        rank = 0
        for r in range(int(nhits[q])):
            if not keep[q, r]:
                continue
            rank += 1
            k, pos, score = (int(x) for x in hits[q, r])
            e = swamd.score_evalue(fit[q], len(targets[k]), score)
            assert e <= evalue
            out.append(f"{rank}\t{k}\t{score}\t{pos // (qlen + 1)}\t{pos % (qlen + 1)} E={e:.2e}")
            if align:
                a = aln[q, r]
                out.append(f"align\t{a[2]}\t{a[4]}\t{a[3]}\t{a[5]}\t{a[6]}")
                lq, lm, lt = swamd.format_alignment(lines_q[q], targets[k], a, ops[q][r])
                out += [f"Q {lq}", f"  {lm}", f"T {lt}"]
    return "\n".join(out) + "\n\n", keep


def test_evalue_prints_the_hits_below_the_cut(swamd, files):
    d, qfa, dbfa, queries, targets = files
    letters, sub, m0, qoffs, scoring = sequence_world(swamd, files)
    hits, nhits, aln, ops, fit = search_round(swamd, m0, qoffs, targets, scoring, 0)
    assert (fit["valid"] == 1).all()
    base = ["--search", qfa, dbfa, "--all-queries", "--gap-open", GO, "--gap-extend", GE, "--top", TOP]
    for evalue, align in ((1e-3, False), (1e-3, True), (5.0, True)):
        exp, keep = evalue_rendering(swamd, qfa, queries, qoffs, targets, hits, nhits, aln, ops, fit, evalue, align)
        assert (0 < keep.sum(axis=1)).all() and (keep.sum(axis=1) < TOP).all()         # some hits fall, some stay, for every query
        r = run(*base, "--evalue", evalue, *(["--align"] if align else []))
        assert r.returncode == 0, r.stderr
        assert before_timings(r.stdout) == exp, (evalue, align)
    # ... through the iterative path (--iterations 1 with --out-pssm) and at another shift
    exp, _ = evalue_rendering(swamd, qfa, queries, qoffs, targets, hits, nhits, aln, ops, fit, 1e-3, True)
    r = run(*base, "--evalue", 1e-3, "--align", "--out-pssm", d / "one")
    assert r.returncode == 0 and before_timings(r.stdout) == exp, r.stderr
    fit2 = search_round(swamd, m0, qoffs, targets, scoring, 2)[4]
    assert (fit2["a"] != fit["a"]).all()
    exp, _ = evalue_rendering(swamd, qfa, queries, qoffs, targets, hits, nhits, aln, ops, fit2, 1e-3, False)
    r = run(*base, "--evalue", 1e-3, "--score-shift", 2)
    assert r.returncode == 0 and before_timings(r.stdout) == exp, r.stderr


def test_include_evalue_writes_the_matrices_of_the_python_chain(swamd, files):
    d, qfa, dbfa, queries, targets = files
    letters, sub, m0, qoffs, scoring = sequence_world(swamd, files)
    base = ["--search", qfa, dbfa, "--all-queries", "--gap-open", GO, "--gap-extend", GE, "--top", TOP]
    for iterations, evalue, pw in ((2, 1e-3, 10), (3, 1.0, 4)):
        m, hits, nhits, aln, ops, fit = chain(swamd, m0, qoffs, targets, scoring, sub, iterations, pw, evalue)
        r = run(*base, "--iterations", iterations, "--include-evalue", evalue, "--prior-weight", pw, "--out-pssm", d / f"e{iterations}", "--align")
        assert r.returncode == 0, r.stderr
        assert before_timings(r.stdout) == rendering(swamd, qfa, queries, qoffs, targets, hits, nhits, aln, ops, True)
        for q in range(len(queries)):
            lt, back = swamd.read_pssm(str(d / f"e{iterations}.{q}.pssm"))
            assert (lt == letters).all() and (back == m[qoffs[q]:qoffs[q + 1]]).all(), (iterations, q)
    # the inclusion by E-value is another one than --include-score 1, which includes every hit (a threshold no hit misses): at prior
    # weight 1 the matrices differ
    everything = chain(swamd, m0, qoffs, targets, scoring, sub, 2, 1, 1e9)[0]
    m_e = chain(swamd, m0, qoffs, targets, scoring, sub, 2, 1, 1e-3)[0]
    assert (m_e != everything).any()
    for flags, m in ((("--include-score", 1), everything), (("--include-evalue", 1e-3), m_e)):
        r = run(*base, "--iterations", 2, "--prior-weight", 1, "--out-pssm", d / "s2", *flags)
        assert r.returncode == 0, r.stderr
        assert all((swamd.read_pssm(str(d / f"s2.{q}.pssm"))[1] == m[qoffs[q]:qoffs[q + 1]]).all() for q in range(len(queries))), flags
    # both flags: the last round's hits by --evalue, the rounds by --include-evalue
    m, hits, nhits, aln, ops, fit = chain(swamd, m0, qoffs, targets, scoring, sub, 2, 10, 1e-3)
    exp, _ = evalue_rendering(swamd, qfa, queries, qoffs, targets, hits, nhits, aln, ops, fit, 0.5, False)
    r = run(*base, "--iterations", 2, "--include-evalue", 1e-3, "--evalue", 0.5)
    assert r.returncode == 0 and before_timings(r.stdout) == exp, r.stderr


def test_without_the_flags_the_output_is_unchanged(swamd, files):
    d, qfa, dbfa, queries, targets = files
    letters, sub, m0, qoffs, scoring = sequence_world(swamd, files)
    base = ["--search", qfa, dbfa, "--all-queries", "--gap-open", GO, "--gap-extend", GE, "--top", TOP, "--align"]
    hits, nhits, aln, ops, _ = search_round(swamd, m0, qoffs, targets, scoring, 0)
    r = run(*base)
    assert r.returncode == 0, r.stderr
    assert before_timings(r.stdout) == rendering(swamd, qfa, queries, qoffs, targets, hits, nhits, aln, ops, True)
    # an E-value no hit misses drops nothing: the lines of the plain run with their E= fields
    loose = run(*base, "--evalue", 1e6)
    assert loose.returncode == 0, loose.stderr
    strip = lambda text: "\n".join(ln.split(" E=")[0] if ln[:1].isdigit() else ln for ln in text.split("\n"))
    assert strip(before_timings(loose.stdout)) == before_timings(r.stdout) and " E=" in loose.stdout
