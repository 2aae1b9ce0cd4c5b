#!/usr/bin/env python3
"""Does the smithW of this tree answer every command line as the smithW of another revision does?

    python scripts/diff_cli.py REV [--out REPORT.json] [--parent-bin FILE]

builds the CLI twice with the Makefile's g++ line -- from smith-waterman_amd/cli/ and include/swhip.h as `git show REV:` gives them (in a
temporary directory laid out as the repository) and from the working tree --, both linked against the working tree's libswhip.so, runs
both over one list of command lines (every mode, every flag at least once; GPU) and compares exit status, stdout, stderr and every file
written (PREFIX.<i>.pssm, PREFIX.<i>.a3m) as bytes.  Two things are masked: the floating-point numbers on the lines that begin
"Elapsed time", and in a "smithW: <call> -> N:" line the text of the call down to the function's name.  One process at a time, each
under 120 s; a process that ends with a signal, with 134 / 139 or at the limit ends the run.  Prints every differing item; the exit
status is 1 if any differs.  --parent-bin: a CLI of REV built earlier (with --build-parent FILE, on a machine that has the history).

    python scripts/diff_cli.py REV --export tests/golden/cli_usage.json

runs USAGE_CASES -- the refusals and early errors, none of which gets as far as sw_create -- through REV's CLI alone and writes
{"files": {name: text}, "cases": [{"args": [...], "expect": [status, stdout, stderr]}]} with the temporary paths replaced by {NAME}
(tests/test_cli_usage_host.py holds the tree's CLI to it).  No GPU.
"""
import argparse
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "smith-waterman_amd")
PROTEIN = "ARNDCQEGHILKMFPSTWYV"
LIMIT_S = 120


def build_cli(tree, exe):
    """The Makefile's smithW rule on the sources under `tree`, against the working tree's library."""
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(tree, "smith-waterman_amd", "cli", "smithW.cpp"), "-L" + PKG, "-lswhip",
                    "-Wl,-rpath," + PKG], check=True)
    return exe


def tree_at(rev, tmp):
    """A directory with cli/ and include/swhip.h of `rev`, laid out as the repository."""
    cli = "smith-waterman_amd/cli/"
    names = subprocess.run(["git", "-C", ROOT, "ls-tree", "--name-only", rev, cli], capture_output=True, text=True, check=True).stdout.split()
    for rel in names + ["include/swhip.h"]:
        path = os.path.join(tmp, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as out:
            out.write(subprocess.run(["git", "-C", ROOT, "show", f"{rev}:{rel}"], capture_output=True, check=True).stdout)
    return tmp


def mask(text):
    lines = []
    for ln in text.split("\n"):
        if ln.startswith("Elapsed time"):
            ln = re.sub(r"-?\d+\.\d+(e[-+]?\d+)?", "<t>", ln)
        lines.append(re.sub(r"^smithW: (\w+)\(.*\) -> (-?\d+):", r"smithW: \1(...) -> \2:", ln))
    return "\n".join(lines)


def elapsed(text):
    return [float(x.group(0)) for ln in text.split("\n") if ln.startswith("Elapsed time") for x in [re.search(r"-?\d+\.\d+", ln)] if x]


class Fatal(Exception):
    pass


def run(exe, args):
    env = dict(os.environ, LD_LIBRARY_PATH=PKG + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))   # (a CLI built where the tree lay elsewhere)
    try:
        p = subprocess.run([exe, *args], capture_output=True, timeout=LIMIT_S, env=env)
    except subprocess.TimeoutExpired:
        raise Fatal(f"{' '.join(args)}: no end within {LIMIT_S} s")
    if p.returncode < 0 or p.returncode in (134, 139):
        raise Fatal(f"{' '.join(args)}: ended with status {p.returncode}\n{p.stderr.decode(errors='replace')[-2000:]}")
    return p.returncode, p.stdout.decode(errors="replace"), p.stderr.decode(errors="replace")


# ---- the inputs: the small files the CLI tests make
def fasta(path, seqs, width=60):
    with open(path, "w") as f:
        for k, s in enumerate(seqs):
            f.write(f">rec{k} record {k}\n")
            f.write("\n".join(s[i:i + width] for i in range(0, len(s), width)) + "\n")


def matrix_text():
    """A small NCBI-format table: matches 5, mismatches -2 .. -4."""
    ls = list(PROTEIN)
    rows = [a + " " + " ".join(str(5 if i == j else -2 - (i + 2 * j) % 3) for j in range(len(ls))) for i, a in enumerate(ls)]
    return "# test table\n   " + "  ".join(ls) + "\n" + "\n".join(rows) + "\n"


def pssm_text(rng, ncols, consensus=None):
    """PSI-BLAST's ASCII layout: a title, the alphabet printed twice, one line per column, a blank line and the statistics."""
    hdr = "   ".join(PROTEIN)
    lines = ["", "Last position-specific scoring matrix computed, weighted observed percentages rounded down, information per position",
             "            " + hdr + "   " + hdr]
    for g in range(ncols):
        row = [int(v) for v in rng.integers(-6, 3, 20)]
        best = PROTEIN.index(consensus[g]) if consensus else int(rng.integers(0, 20))
        row[best] = int(rng.integers(4, 10))
        lines.append(f"{g + 1:5d} {PROTEIN[best]}   " + " ".join(f"{v:3d}" for v in row) + "   " + " ".join("  0" for _ in row) + "  0.55 0.12")
    lines += ["", "                      K         Lambda", "Standard Ungapped    0.1350     0.3166"]
    return "\n".join(lines) + "\n"


def make_inputs(d):
    import numpy as np
    rng = np.random.default_rng(71)
    word = lambda n: "".join(rng.choice(list(PROTEIN), int(n)))
    queries = [word(n) for n in (12, 57, 130, 300)]
    half = [word(n) for n in rng.integers(10, 121, 12)]
    for k, q in enumerate(queries):   # related targets: a long diagonal with a gap in it
        t = q[3:113]
        half[3 * k] = (t[:len(t) // 2] + word(2) + t[len(t) // 2:])[:120]
    targets = half + half             # every target occurs twice: ties in every ranking
    f = {name: os.path.join(d, name) for name in ("q.fa", "q_long.fa", "db.fa", "db_long.fa", "big.fa", "m.txt", "p.pssm", "pairs.txt")}
    fasta(f["q.fa"], queries)
    fasta(f["db.fa"], targets)
    # one record of one letter repeated, nobody's hit: 600 000 rows x the 2048 padded columns of a 1100-letter query pass the default
    # workspace of 1 GiB (the files of tests/test_cli_align_ckpt_gpu.py)
    fasta(f["q_long.fa"], [queries[1], queries[3] + word(800)])
    fasta(f["db_long.fa"], targets[:7] + ["A" * 600_000] + targets[7:])
    fasta(f["big.fa"], [word(10) for _ in range(4097)])
    with open(f["m.txt"], "w") as out:
        out.write(matrix_text())
    with open(f["p.pssm"], "w") as out:
        out.write(pssm_text(rng, 110, queries[3][3:113]))
    with open(f["pairs.txt"], "w") as out:
        out.write("# query target\n0 0\n\n3 9\n  2 21  \n# outside the files\n4 0\n1 24\n-1 3\n\n1 12\n3 0\n")
    return f


def commands(f):
    q, db, m = f["q.fa"], f["db.fa"], f["m.txt"]
    aff = ["--matrix", m, "--gap-open", "-6", "--gap-extend", "-1"]
    one, many, pssm = ["--search", q, db], ["--search", q, db, "--all-queries"], ["--search", "--pssm", f["p.pssm"], db, "--gap-open", "-6", "--gap-extend", "-1"]
    many_long = ["--search", f["q_long.fa"], f["db_long.fa"], "--all-queries", "--top", "3", *aff, "--align"]
    return [
        # one query
        one, one + ["--record-a", "1", "--top", "5", *aff], one + ["--record-a", "2", "--gap-open", "-5", "--gap-extend", "-1"], one + ["--gap-extend", "-3"],
        one + ["--record-a", "2", "--align", "--top", "3"], one + ["--record-a", "3", "--top", "4", "--align", *aff],
        ["--search", f["q_long.fa"], f["db_long.fa"], "--record-a", "1", "--top", "3", *aff, "--align", "--align-checkpoint"],
        # every query through one handle
        many + ["--top", "3"], many + ["--top", "0"], many + ["--min-score", "40", *aff], many + ["--top", "3", "--align", *aff], many + ["--top", "3", "--align", "--scores", "2", "-1", "-2"],
        many + ["--search-lanes", "16", *aff], many + ["--prefilter-hits", "20", "--top", "4", *aff], many + ["--prefilter-hits", "20", "--pairs-lanes", "16", "--align", *aff],
        ["--search", q, f["big.fa"], "--all-queries", "--top", "4097"], ["--search", q, f["big.fa"], "--all-queries", "--top", "4097", "--min-score", "12", "--align"],
        many + ["--prefilter", "20", *aff], many + ["--prefilter", "9"], many_long, many_long + ["--align-checkpoint"],
        # a list of pairs
        one + ["--pairs", f["pairs.txt"], *aff], one + ["--pairs", f["pairs.txt"], "--pairs-lanes", "16"],
        # one matrix as the query
        pssm, pssm + ["--align", "--top", "3"], pssm + ["--search-lanes", "16", "--min-score", "30"], ["--search", "--pssm", f["p.pssm"], f["big.fa"], "--gap-open", "-6", "--gap-extend", "-1", "--top", "4097"],
        # iterations
        many + ["--iterations", "1", "--top", "5", *aff], many + ["--iterations", "1", "--out-pssm", "{OUT}/s1", *aff], many + ["--iterations", "2", "--align", "--top", "4", *aff],
        many + ["--iterations", "3", "--align", "--out-a3m", "{OUT}/s3", "--include-score", "30", *aff],
        many + ["--iterations", "2", "--weight-hits", "16", "--prior-weight", "160", "--out-pssm", "{OUT}/sw", "--search-lanes", "16", *aff],
        many + ["--align", "--out-a3m", "{OUT}/s0", "--top", "6"],
        pssm + ["--iterations", "1"], pssm + ["--iterations", "2", "--align", "--top", "4", "--out-pssm", "{OUT}/p2"],
        pssm + ["--iterations", "3", "--align", "--out-a3m", "{OUT}/p3", "--out-pssm", "{OUT}/p3"],
        pssm + ["--iterations", "2", "--weight-hits", "16", "--prior-weight", "160", "--align", "--align-checkpoint"],
        # the fill
        [], ["100", "90"], ["100", "90", "--dump"], ["--dump-labels", "40", "30", "--seed", "7"], ["--h64", "100", "90"], ["100", "--no-backtrack", "90"], ["--dump"],
        ["1000", "900", "--p8", "--gpus", "2"], ["300", "200", "--devices", "0,0"], ["--fasta", q, db, "--record-a", "1", "--record-b", "2", "--scores", "2", "-1", "-1"],
    ]


def outcome(exe, args, out_dir):
    os.makedirs(out_dir)
    status, so, se = run(exe, [a.replace("{OUT}", out_dir) for a in args])
    files = {}
    for name in sorted(os.listdir(out_dir)):
        with open(os.path.join(out_dir, name), "rb") as fh:
            files[name] = fh.read()
    return {"status": status, "stdout": mask(so), "stderr": mask(se), "files": files, "elapsed": elapsed(so)}


def digest(x):
    return hashlib.sha256(x if isinstance(x, bytes) else x.encode()).hexdigest()[:16]


def compare(parent, tree, tmp, rev):
    f = make_inputs(tmp)
    report, differing = [], 0
    for k, args in enumerate(commands(f)):
        a, b = outcome(parent, args, os.path.join(tmp, f"out_parent_{k}")), outcome(tree, args, os.path.join(tmp, f"out_tree_{k}"))
        items = [x for x in ("status", "stdout", "stderr") if a[x] != b[x]] + [f"file {n}" for n in sorted(set(a["files"]) | set(b["files"])) if a["files"].get(n) != b["files"].get(n)]
        shown = " ".join(os.path.basename(x) if os.sep in x else x for x in args)
        print(f"[{k:2d}] {'same' if not items else 'DIFFERS in ' + ', '.join(items)}: status {a['status']}, {len(a['files'])} files: smithW {shown}", flush=True)
        if a["status"] or a["stderr"]:
            print("     stderr: " + a["stderr"].split("\n")[0][:300])
        for x in items:
            if x in ("stdout", "stderr"):
                pa, pb = a[x].split("\n"), b[x].split("\n")
                at = next((i for i in range(min(len(pa), len(pb))) if pa[i] != pb[i]), min(len(pa), len(pb)))
                print(f"     {x} line {at + 1}:\n       {rev}: {pa[at][:300] if at < len(pa) else '<end>'}\n       tree: {pb[at][:300] if at < len(pb) else '<end>'}")
        differing += len(items)
        side = lambda o: {"status": o["status"], "stdout": digest(o["stdout"]), "stderr": digest(o["stderr"]), "stderr_text": o["stderr"][:600],
                          "files": {n: digest(v) for n, v in o["files"].items()}, "elapsed": o["elapsed"]}
        report.append({"args": shown, "differing": items, "parent": side(a), "tree": side(b)})
    return {"rev": rev, "commands": len(report), "differing_items": differing, "masked": ["floats on 'Elapsed time' lines", "call text in 'smithW: <call> -> N:' lines"],
            "note": "elapsed: seconds as printed, recorded, not compared (at these sizes they are launch noise)", "runs": report}


# ---- the refusals and early errors: every message of main() and what the modes refuse before sw_create
S, P = ["--search", "{Q}", "{DB}"], ["--search", "--pssm", "{PSSM}", "{DB}", "--gap-open", "-6", "--gap-extend", "-1"]
A = S + ["--all-queries"]
BIG_SCORES = ["--scores", "300", "-3", "-2"]
USAGE_CASES = [
    # parsing
    ["--bogus"], ["5"], ["5", "--dump"], ["--top"], S + ["--min-score"], ["--search", "{Q}"], ["--search", "--pssm", "{PSSM}"], ["--scores", "1", "2"], ["--fasta", "{Q}"],
    ["--min-score", "3k"], ["--gap-open", "-x"], ["--iterations", ""], ["--prefilter", "1e3"], ["--weight-hits", "99999999999"], ["40", "30", "20"],
    # --align-checkpoint, the lanes
    ["40", "30", "--align-checkpoint"], S + ["--align-checkpoint"], A + ["--align-checkpoint"],
    A + ["--search-lanes", "8"], ["--search-lanes", "16"], S + ["--search-lanes", "16"], A + ["--search-lanes", "16", "--prefilter", "5"], A + ["--search-lanes", "32", "--prefilter-hits", "5"],
    S + ["--search-lanes", "16", "--pairs", "{PAIRS}"], P + ["--search-lanes", "16", "--pairs", "{PAIRS}"],
    A + ["--pairs-lanes", "8"], A + ["--pairs-lanes", "16"], ["--pairs-lanes", "16", "--pairs", "{PAIRS}"], P + ["--pairs-lanes", "16", "--pairs", "{PAIRS}"], S + ["--pairs-lanes", "32"],
    # the iterative search
    ["--iterations", "2"], S + ["--iterations", "2"], S + ["--out-pssm", "x"], ["40", "30", "--include-score", "3"], A + ["--iterations", "0"], A + ["--prior-weight", "70000"],
    A + ["--prior-weight", "-1"], A + ["--iterations", "2", "--prefilter", "5"], A + ["--iterations", "2", "--prefilter-hits", "5"], S + ["--pairs", "{PAIRS}", "--all-queries", "--iterations", "2"],
    A + ["--out-a3m", "x"], P + ["--out-a3m", "x", "--iterations", "2"],
    A + ["--weight-hits", "16"], A + ["--weight-hits", "16", "--iterations", "1"], S + ["--weight-hits", "16"], A + ["--iterations", "2", "--weight-hits", "0"],
    A + ["--out-pssm", "x", "--weight-hits", "70000"],
    # --pssm
    P + ["--matrix", "{PSSM}"], P + ["--all-queries"], P + ["--pairs", "{PAIRS}"], P + ["--prefilter", "5"], P + ["--prefilter-hits", "5"], P[:-2], P[:4] + ["--gap-extend", "-1"],
    P + ["--iterations", "2", *BIG_SCORES], P + ["--out-pssm", "x", "--scores", "3", "-129", "-2"],
    # --search and its scores
    S + ["--gap-open", "-5", *BIG_SCORES], S + ["--align", "--scores", "3", "-300", "-2"], A + ["--gap-open", "-5", "--align", "--scores", "128", "0", "0"],
    # --prefilter-hits, --prefilter
    S + ["--prefilter-hits", "5"], ["--prefilter-hits", "5"], A + ["--prefilter-hits", "5", "--prefilter", "5"], A + ["--prefilter-hits", "5", "--pairs", "{PAIRS}"], A + ["--prefilter-hits", "0"],
    S + ["--prefilter", "5"], ["--prefilter", "5"], ["--all-queries", "--prefilter", "5"], A + ["--prefilter", "5", "--top", "3"], A + ["--prefilter", "5", "--min-score", "3"], A + ["--prefilter", "5", "--align"],
    A + ["--prefilter", "5", "--pairs", "{PAIRS}"], A + ["--prefilter", "0"], A + ["--prefilter", "5", *BIG_SCORES],
    # --pairs
    ["--pairs", "{PAIRS}"], S + ["--pairs", "{PAIRS}", "--all-queries"], S + ["--pairs", "{PAIRS}", "--top", "3"], S + ["--pairs", "{PAIRS}", "--min-score", "3"], S + ["--pairs", "{PAIRS}", "--align", "--gap-open", "-3"],
    S + ["--pairs", "{PAIRS}", *BIG_SCORES], S + ["--pairs", "{PAIRS_TOKEN}"], S + ["--pairs", "{PAIRS_THREE}"], S + ["--pairs", "{PAIRS_LONG}"], S + ["--pairs", "{MISSING}"],
    # --all-queries, --min-score and what goes with --search alone
    ["--all-queries"], A + BIG_SCORES, S + ["--min-score", "5"], ["--min-score", "5"], ["--align"], ["40", "30", "--matrix", "{PSSM}"], ["--gap-open", "-3"], ["--gap-extend", "-3"],
    # several rules at once: the first in the order of the checks answers
    ["5", "--align-checkpoint", "--search-lanes", "8"], A + ["--search-lanes", "8", "--pairs-lanes", "8", "--iterations", "0"], ["--align-checkpoint", "--search-lanes", "16", "--iterations", "2"],
    ["--pairs-lanes", "8", "--weight-hits", "0", "--out-a3m", "x"], A + ["--iterations", "0", "--prior-weight", "-1", "--prefilter", "5"], A + ["--out-a3m", "x", "--weight-hits", "0", "--iterations", "1"],
    P + ["--matrix", "{PSSM}", "--all-queries", "--pairs", "{PAIRS}"], P[:-2] + ["--prefilter", "0", "--iterations", "2", *BIG_SCORES], A + ["--prefilter", "0", "--top", "3", "--align", *BIG_SCORES],
    A + ["--gap-open", "-5", "--align", "--prefilter-hits", "0", *BIG_SCORES], A + ["--prefilter-hits", "0", "--prefilter", "0", "--pairs", "{PAIRS}"],
    S + ["--pairs", "{PAIRS_TOKEN}", "--all-queries", "--top", "3", *BIG_SCORES], S + ["--pairs", "{PAIRS}", "--min-score", "3", "--align", *BIG_SCORES],
    ["--min-score", "5", "--align", "--matrix", "{PSSM}", "--pairs", "{PAIRS}", "--all-queries"], ["--align", "--gap-extend", "-1", "--min-score", "2"], ["--prefilter", "5", "--prefilter-hits", "5", "--pairs", "{PAIRS}"],
    # files that are not there or not what they should be, and what the modes refuse before they open a device
    ["--search", "{MISSING}", "{DB}"], ["--search", "{Q}", "{MISSING}"], ["--search", "{MISSING}", "{DB}", "--all-queries"], ["--search", "{Q}", "{MISSING}", "--all-queries", "--prefilter", "5"],
    ["--search", "{Q}", "{MISSING}", "--pairs", "{PAIRS}"], ["--fasta", "{MISSING}", "{DB}"], ["--fasta", "{Q}", "{MISSING}", "--record-b", "2"],
    ["--fasta", "{Q}", "{DB}", "--record-a", "9"], ["--search", "{Q}", "{DB}", "--record-a", "9"],
    ["--search", "--pssm", "{DB}", "{DB}", "--gap-open", "-6", "--gap-extend", "-1"], ["--search", "--pssm", "{PSSM_SHORT}", "{DB}", "--gap-open", "-6", "--gap-extend", "-1", "--iterations", "2"],
    ["--search", "--pssm", "{MISSING}", "{DB}", "--gap-open", "-6", "--gap-extend", "-1"], P[:3] + ["{MISSING}"] + P[4:],
    A + ["--iterations", "2", "--matrix", "{MISSING}"], A + ["--iterations", "2", "--top", "0"], P + ["--iterations", "2", "--top", "0"], P + ["--out-pssm", "x", "--top", "-4"],
    ["--search", "{EMPTY}", "{DB}", "--all-queries", "--iterations", "2"],
]


def usage_files():
    import numpy as np
    rng = np.random.default_rng(5)
    word = lambda n: "".join(rng.choice(list(PROTEIN), int(n)))
    fa = lambda seqs: "".join(f">s{k}\n{s}\n" for k, s in enumerate(seqs))
    pssm = pssm_text(rng, 9)
    return {"Q": fa([word(12), word(30)]), "DB": fa([word(n) for n in (10, 25, 40)]), "EMPTY": "", "PSSM": pssm, "PSSM_SHORT": "\n".join(pssm.split("\n")[:3]) + "\n",
            "PAIRS": "0 0\n1 2\n", "PAIRS_TOKEN": "0 0\n1 x\n", "PAIRS_THREE": "# three numbers\n\n0 1 2\n", "PAIRS_LONG": "0 0\n" + " " * 600 + "1 1\n"}


def run_usage(exe, golden_files, cases, d):
    """[[status, stdout, stderr], ...] of `cases` under `exe`, the paths under `d` written back as {NAME}."""
    paths = {name: os.path.join(d, name.lower()) for name in golden_files}
    for name, text in golden_files.items():
        with open(paths[name], "w") as f:
            f.write(text)
    paths["MISSING"] = os.path.join(d, "missing")
    got = []
    for args in cases:
        real = [a.format(**paths) if "{" in a else a for a in args]
        status, so, se = run(exe, real)
        for name in sorted(paths, key=len, reverse=True):   # (PAIRS_TOKEN before PAIRS)
            so, se = so.replace(paths[name], "{" + name + "}"), se.replace(paths[name], "{" + name + "}")
        got.append([status, mask(so), mask(se)])
    return got


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("rev")
    ap.add_argument("--out", help="the report as JSON (profiles/cli_refactor_ab.json is one)")
    ap.add_argument("--export", metavar="FILE", help="write the golden of the usage cases from REV's CLI; no GPU")
    ap.add_argument("--parent-bin", help="REV's CLI, built earlier")
    ap.add_argument("--build-parent", metavar="FILE", help="build REV's CLI into FILE and stop")
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="diff_cli_")
    try:
        if a.build_parent:
            build_cli(tree_at(a.rev, os.path.join(tmp, "rev")), a.build_parent)
            return 0
        parent = a.parent_bin or build_cli(tree_at(a.rev, os.path.join(tmp, "rev")), os.path.join(tmp, "smithW_rev"))
        if a.export:
            files = usage_files()
            got = run_usage(parent, files, USAGE_CASES, tmp)
            for c, g in zip(USAGE_CASES, got):   # a case that gets as far as the device is no case for a machine without one
                if g[0] not in (1, 2) or g[1] or "sw_create" in g[2]:
                    raise SystemExit(f"not a refusal or an early error: {c} -> {g}")
            with open(a.export, "w") as f:
                json.dump({"rev": subprocess.run(["git", "-C", ROOT, "rev-parse", a.rev], capture_output=True, text=True).stdout.strip() or a.rev, "files": files,
                           "cases": [{"args": c, "expect": g} for c, g in zip(USAGE_CASES, got)]}, f, indent=1)
                f.write("\n")
            print(f"{len(got)} cases: statuses {sorted(set(g[0] for g in got))}")
            return 0
        tree = build_cli(ROOT, os.path.join(tmp, "smithW_tree"))
        report = compare(os.path.abspath(parent), tree, tmp, a.rev)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(report, f, indent=1)
                f.write("\n")
        print(f"{report['commands']} command lines, {report['differing_items']} differing items")
        return 1 if report["differing_items"] else 0
    except Fatal as e:
        print(f"STOPPED, nothing further started: {e}")
        return 3
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
