"""GPU: smithW --search Q.fa DB.fa --all-queries --align --align-checkpoint (option "align_checkpoint" = 2): the output is that of the
run without the flag, byte for byte -- on a small database, where the flag changes nothing, and on one with a long record, where the
unflagged run falls back to one alignment call per query and the flagged run aligns the whole table in one checkpointed call."""
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
            f.write(f">rec{k}\n")
            s = bytes(s).decode()
            f.write("\n".join(s[i:i + 60] for i in range(0, len(s), 60)) + "\n")


def untimed(text):
    return [ln for ln in text.split("\n") if not ln.startswith("Elapsed")]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    rng = np.random.default_rng(18)
    d = tmp_path_factory.mktemp("cli_ckpt")
    letters = PROTEIN[:20]
    queries = [rng.choice(letters, n).astype(np.uint8) for n in (40, 300, 1100)]
    targets = [rng.choice(letters, int(n)).astype(np.uint8) for n in rng.integers(20, 400, 30)]
    for k, q in enumerate(queries):                                # related targets: the alignments are long and carry a gap
        t = q[5:].copy()
        t[::9] = letters[3]
        targets.insert(4 * k + 1, np.concatenate([t[:len(t) // 2], rng.choice(letters, 3).astype(np.uint8), t[len(t) // 2:]]))
    fasta(d / "q.fa", queries)
    fasta(d / "db.fa", targets)
    # one long record: 600 000 rows x 2048 padded columns of the longest query do not fit the default workspace of 1 GiB.  It is one
    # letter repeated, so it scores a single match and is nobody's hit: the per-query calls of the unflagged run never see it
    fasta(d / "db_long.fa", targets[:7] + [np.full(600_000, letters[0], np.uint8)] + targets[7:])
    with open(d / "m.txt", "w") as f:                              # a small NCBI-format table: matches 5, mismatches -2 .. -4
        ls = [chr(c) for c in letters]
        f.write("# test table\n   " + "  ".join(ls) + "\n")
        for i, a in enumerate(ls):
            f.write(a + " " + " ".join(str(5 if i == j else -2 - (i + 2 * j) % 3) for j in range(len(ls))) + "\n")
    return str(d / "q.fa"), str(d / "db.fa"), str(d / "db_long.fa"), str(d / "m.txt")


@pytest.mark.parametrize("long_record", [False, True])
def test_the_flag_changes_no_byte_of_the_output(files, long_record):
    q, db, db_long, m = files
    args = ("--search", q, db_long if long_record else db, "--all-queries", "--top", 4, "--matrix", m, "--gap-open", -6, "--gap-extend", -1, "--align")
    plain, flagged = run(*args), run(*args, "--align-checkpoint")
    assert plain.returncode == 0 and flagged.returncode == 0, plain.stderr + flagged.stderr
    assert untimed(flagged.stdout) == untimed(plain.stdout)
    # which route was taken: the per-query fallback says so on stderr, the one call says nothing
    assert ("aligning query by query" in plain.stderr) == long_record and ("align_workspace_mib" in plain.stderr) == long_record
    assert "aligning query by query" not in flagged.stderr
    lines = untimed(flagged.stdout)
    assert sum(ln.startswith("align\t") for ln in lines) == 3 * 4                      # every alignment is printed
    assert max(int(ln.split("\t")[5]) for ln in lines if ln.startswith("align\t")) > 1000
    if long_record:                                                                    # the long record is no hit: the blocks are the small database's, one record on
        small = untimed(run(*[db if a == db_long else a for a in args]).stdout)
        assert [ln for ln in lines if ln[:2] in ("Q ", "T ", "  ")] == [ln for ln in small if ln[:2] in ("Q ", "T ", "  ")]


def test_one_query_and_the_usage_errors(files):
    q, db, db_long, m = files
    args = ("--search", q, db, "--record-a", 2, "--top", 2, "--matrix", m, "--gap-open", -6, "--gap-extend", -1, "--align")
    plain, flagged = run(*args), run(*args, "--align-checkpoint")
    assert plain.returncode == 0 and flagged.returncode == 0, plain.stderr + flagged.stderr
    assert untimed(flagged.stdout) == untimed(plain.stdout)
    for bad in (("--search", q, db, "--align-checkpoint"), ("--search", q, db, "--all-queries", "--align-checkpoint"), ("40", "30", "--align-checkpoint")):
        r = run(*bad)
        assert r.returncode == 2 and "--align-checkpoint goes with --search --align" in r.stderr and "usage:" not in r.stderr
