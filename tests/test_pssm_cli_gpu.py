"""GPU: smithW --search --pssm FILE DB.fa (sw_read_pssm, then one handle: sw_db_search_pssm_top and, with --align, sw_db_align_pssm_hits on
its device hit table): stdout but for the line of timings equals, byte for byte, the rendering built from the Python host legs
(read_pssm, search_pssm_multi_host, align_pssm_hits_host, format_alignment with the matrix's consensus); the flags --pssm excludes."""
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


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    rng = np.random.default_rng(47)
    d = tmp_path_factory.mktemp("cli_pssm")
    letters = PROTEIN[:20]
    m = rng.integers(-6, 3, (70, 20)).astype(np.int8)
    residue = rng.integers(0, 20, 70)
    m[np.arange(70), residue] = rng.integers(4, 10, 70).astype(np.int8)           # one favoured letter per column
    pssm_cases.write_ascii_pssm(d / "p.pssm", letters, m, letters[residue])
    targets = [rng.choice(np.concatenate([letters, [ord("X")]]), int(n)).astype(np.uint8) for n in (50, 7, 200, 64, 400, 33, 90)]
    targets[2][40:100] = letters[residue[5:65]]                                    # related targets: a long diagonal,
    targets[4] = np.concatenate([targets[4][:100], letters[residue[:30]], targets[4][100:103], letters[residue[30:]], targets[4][103:]]).astype(np.uint8)   # a gap
    with open(d / "db.fa", "w") as f:
        for k, s in enumerate(targets):
            f.write(f">rec{k} some description\n" + bytes(s).decode() + "\n")
    return d, str(d / "p.pssm"), str(d / "db.fa"), targets


def rendering(swamd, files, go, ge, top, min_score, align):
    """What the tool prints before its line of timings."""
    _, p, _, targets = files
    letters, m = swamd.read_pssm(p)
    scoring = (letters, min(int(m.min()), 0), max(int(m.max()), 0), go, ge)
    consensus = bytes(letters[np.argmax(m, axis=1)])                               # per column the first letter with the largest entry
    res = swamd.search_pssm_multi_host([m], targets, scoring)
    hits, nhits = pssm_cases.rank_order(res, min(top, len(targets)), min_score)
    aln, ops = swamd.align_pssm_hits_host([m], targets, scoring, hits, nhits)
    out = [f"## query record 0 of {p}",
           f"# query {len(m)} letters, {len(targets)} targets, {sum(len(t) for t in targets)} letters; rank\trecord\tscore\ttarget_end\tquery_end"]
    for r in range(int(nhits[0])):
        k, pos, score = (int(x) for x in hits[0, r])
        out.append(f"{r + 1}\t{k}\t{score}\t{pos // (len(m) + 1)}\t{pos % (len(m) + 1)}")
        if align:
            a = aln[0, r]
            out.append(f"align\t{a[2]}\t{a[4]}\t{a[3]}\t{a[5]}\t{a[6]}")
            lq, lm, lt = swamd.format_alignment(consensus, targets[k], a, ops[0][r])
            out += [f"Q {lq}", f"  {lm}", f"T {lt}"]
    return "\n".join(out) + "\n\n"


def before_timings(text):
    at = text.index("Elapsed time for database search:")
    assert text[at:].count("\n") == 2 and text.endswith("\n\n")
    return text[:at]


def test_stdout_equals_the_rendering_of_the_host_legs(swamd, files):
    d, p, db, targets = files
    for top, min_score, align in ((10, 0, False), (3, 0, True), (5, 40, True), (5, 100000, True)):
        flags = ["--top", top] + (["--min-score", min_score] if min_score else []) + (["--align"] if align else [])
        r = run("--search", "--pssm", p, db, "--gap-open", -6, "--gap-extend", -1, *flags)
        assert r.returncode == 0, r.stderr
        want = rendering(swamd, files, -6, -1, top, min_score, align)
        assert before_timings(r.stdout) == want, (top, min_score, align)
    want = rendering(swamd, files, -6, -1, 3, 0, True)
    assert "\n1\t2\t" in want or "\n1\t4\t" in want                                # a planted target leads
    assert any(x.startswith("Q ") and "-" in x for x in want.split("\n"))           # and the planted gap is there


def test_excluded_flags(files):
    d, p, db, _ = files
    for flags, word in ((("--matrix", p), "--matrix"), (("--all-queries",), "--all-queries"), (("--pairs", p), "--pairs"), (("--prefilter", 5), "--prefilter")):
        r = run("--search", "--pssm", p, db, "--gap-open", -6, "--gap-extend", -1, *flags)
        assert r.returncode == 2 and f"--pssm does not go with {word}" in r.stderr and "usage:" not in r.stderr and r.stdout == "", (flags, r.stderr)
    r = run("--search", "--pssm", p, db, "--gap-open", -6)
    assert r.returncode == 2 and "--pssm needs --gap-open O and --gap-extend E" in r.stderr
    r = run("--search", "--pssm", db, db, "--gap-open", -6, "--gap-extend", -1)      # not a PSSM
    assert r.returncode == 1 and "sw_read_pssm" in r.stderr and r.stdout == ""
