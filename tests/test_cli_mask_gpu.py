"""GPU: smithW --mask on a 3-query, 40-target FASTA written here, with planted poly-Q stretches: `--search Q.fa DB.fa --all-queries
--top 5 --mask` prints what the CLI without --mask prints for a FASTA masked beforehand by the Python host leg, and says on stderr
how much was masked; with --align the T lines show the mask byte, again as for the file masked beforehand; with --out-a3m the files
hold the ORIGINAL letters where the alignment crossed masked ones, and are otherwise the files of the run on the masked file."""
import os
import re
import subprocess

import numpy as np
import pytest

from affine_cases import PROTEIN
from oracle_lib import ROOT

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "smith-waterman_amd", "smithW")


def run(*args):
    return subprocess.run([CLI, *[str(a) for a in args]], capture_output=True, text=True, timeout=120)


def body(stdout):
    """stdout without the line that holds the time."""
    return [x for x in stdout.split("\n") if not x.startswith("Elapsed time")]


@pytest.fixture(scope="module")
def files(swamd, tmp_path_factory):
    rng = np.random.default_rng(83)
    d = tmp_path_factory.mktemp("cli_mask")
    alpha = np.array([c for c in PROTEIN[:20] if c != ord("Q")], np.uint8)
    rnd = lambda n: rng.choice(alpha, int(n)).astype(np.uint8).tobytes()
    q0 = rnd(60) + b"Q" * 14 + rnd(60)            # long flanks: an alignment with a copy of q0 crosses the masked stretch
    queries = [q0, rnd(90), b"Q" * 30 + rnd(40)]
    targets = [rnd(n) for n in rng.integers(20, 300, 30)]
    targets += [rnd(30) + q0 + rnd(10), rnd(5) + q0[:70] + b"QQ" + q0[70:], rnd(40) + queries[1] + rnd(40)]
    targets += [rnd(n) + b"Q" * 25 + rnd(n) for n in (10, 50, 90, 120, 33, 71, 8)]
    targets = [targets[k] for k in rng.permutation(len(targets))]
    assert len(targets) == 40
    masked, nmasked = swamd.mask_low_complexity_host(targets)
    offs = np.concatenate([[0], np.cumsum([len(t) for t in targets])])
    masked_targets = [masked[offs[k]:offs[k + 1]].tobytes() for k in range(40)]
    assert (nmasked > 0).sum() >= 9 and all(len(a) == len(b) for a, b in zip(targets, masked_targets))
    for name, tag, seqs in (("q.fa", "qry", queries), ("db.fa", "rec", targets), ("db_masked.fa", "rec", masked_targets)):
        with open(d / name, "w") as f:
            for k, s in enumerate(seqs):
                f.write(f">{tag}{k} some description\n" + s.decode() + "\n")
    return d, str(d / "q.fa"), str(d / "db.fa"), str(d / "db_masked.fa"), nmasked


def test_hit_lines_are_those_of_a_file_masked_beforehand(files):
    d, q, db, dbm, nmasked = files
    base = ["--all-queries", "--top", 5]
    a, b, plain = run("--search", q, db, *base, "--mask"), run("--search", q, dbm, *base), run("--search", q, db, *base)
    assert a.returncode == b.returncode == plain.returncode == 0
    assert body(a.stdout) == body(b.stdout) and body(a.stdout) != body(plain.stdout)
    total = sum(len(x) for x in open(db).read().split("\n")[1::2])
    assert a.stderr == f"smithW: --mask: {int(nmasked.sum())} letters of {int((nmasked > 0).sum())} targets masked (of {total} letters, 40 targets)\n"
    assert b.stderr == ""
    # the sub-flags reach the rule: a window nothing here is low under masks nothing
    c = run("--search", q, db, *base, "--mask", "--mask-trigger", 0, "--mask-extend", 0, "--mask-letters", "W")
    assert c.returncode == 0 and body(c.stdout) == body(plain.stdout) and c.stderr.startswith("smithW: --mask: 0 letters of 0 targets")
    # the single-query mode and the matrix-free affine mode take the flag too
    for extra in ([], ["--gap-open", -6, "--gap-extend", -1, "--all-queries"]):
        a, b = run("--search", q, db, "--top", 5, "--mask", *extra), run("--search", q, dbm, "--top", 5, *extra)
        assert a.returncode == b.returncode == 0 and body(a.stdout) == body(b.stdout)


def test_align_shows_the_mask_byte(files):
    d, q, db, dbm, _ = files
    base = ["--all-queries", "--top", 5, "--align"]
    a, b = run("--search", q, db, *base, "--mask"), run("--search", q, dbm, *base)
    assert a.returncode == b.returncode == 0 and body(a.stdout) == body(b.stdout)
    tlines = [x for x in a.stdout.split("\n") if x.startswith("T ")]
    assert any("X" in x for x in tlines)
    a = run("--search", q, db, *base, "--mask", "--mask-byte", "#")
    assert a.returncode == 0 and any("#" in x for x in a.stdout.split("\n") if x.startswith("T ")) and "X" not in a.stdout


def test_out_a3m_holds_the_original_letters(files):
    d, q, db, dbm, _ = files
    base = ["--all-queries", "--top", 5, "--align"]
    a = run("--search", q, db, *base, "--mask", "--out-a3m", d / "m")
    b = run("--search", q, dbm, *base, "--out-a3m", d / "b")
    assert a.returncode == b.returncode == 0 and body(a.stdout) == body(b.stdout)
    restored = 0
    for k in range(3):
        la, lb = (open(d / f"{p}.{k}.a3m").read().split("\n") for p in "mb")
        assert len(la) == len(lb) and la[:2] == lb[:2]                         # the query's record
        for x, y in zip(la[2:], lb[2:]):
            if x.startswith(">"):
                assert re.sub(r" ident=\S+", "", x) == re.sub(r" ident=\S+", "", y)      # (identities are counted on the letters written)
                continue
            assert len(x) == len(y) and "X" not in x and "x" not in x
            for cx, cy in zip(x, y):
                assert cx == cy or cy in "Xx"
                restored += cx != cy
    assert restored >= 10
