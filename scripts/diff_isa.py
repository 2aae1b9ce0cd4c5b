#!/usr/bin/env python3
"""Are the gfx950 instructions of these kernels those of another revision?

    python scripts/diff_isa.py REV FILE.hip ...

puts smith-waterman_amd/csrc/* and include/swhip.h as `git show REV:` gives them into a temporary directory laid out as the repository
(sw_kernels.h includes ../../include/swhip.h), compiles every named file of csrc/ from that directory and from the working tree,
device-only, to gfx950 assembly, and compares the two as text: the instruction lines (comments stripped; labels and directives left
out) and, per kernel, VGPRs, SGPRs, LDS and scratch bytes from the code object's metadata.  Prints both per file and per kernel; the
exit status is 1 if anything differs.  A plain text diff -- it looks for no particular instruction.  No GPU.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("smith-waterman_amd", "csrc")
HEADER = os.path.join("include", "swhip.h")
RESOURCES = [("VGPRs", ".vgpr_count"), ("SGPRs", ".sgpr_count"), ("LDS", ".group_segment_fixed_size"), ("scratch", ".private_segment_fixed_size")]


def tree_at(rev, tmp):
    """A directory with csrc/ and include/swhip.h of `rev`, laid out as the repository."""
    names = subprocess.run(["git", "-C", ROOT, "ls-tree", "--name-only", rev, CSRC.replace(os.sep, "/") + "/"], capture_output=True, text=True, check=True).stdout.split()
    for rel in names + [HEADER.replace(os.sep, "/")]:
        path = os.path.join(tmp, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as out:
            out.write(subprocess.run(["git", "-C", ROOT, "show", f"{rev}:{rel}"], capture_output=True, check=True).stdout)
    return tmp


def assembly(tree, name, out):
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++20", "-S", "--cuda-device-only", os.path.join(tree, CSRC, name), "-o", out],
                   check=True, stderr=subprocess.DEVNULL)
    with open(out) as f:
        return f.read()


def instructions(asm):
    """The instruction lines: comments stripped, and no blank lines, labels or directives."""
    out = []
    for ln in asm[:asm.find(".amdgpu_metadata")].splitlines():
        t = ln.split(";")[0].strip()
        if t and not t.startswith(".") and not t.endswith(":"):
            out.append(t)
    return out


def resources(asm):
    """{kernel: {field: value}} from the amdhsa.kernels metadata, in the order of the file."""
    out = {}
    for entry in re.split(r"^  - ", asm[asm.find("amdhsa.kernels:"):], flags=re.M)[1:]:
        fields = dict(re.findall(r"^\s*(\.\w+):\s+(\S+)\s*$", entry, flags=re.M))
        if ".name" in fields:
            out[fields[".name"]] = {label: fields.get(key) for label, key in RESOURCES}
    return out


def differing(a, b, tmp, tag):
    """Lines that `diff` reports as changed, added or removed between two lists of lines."""
    if a == b:
        return 0
    paths = []
    for side, lines in (("old", a), ("new", b)):
        paths.append(os.path.join(tmp, f"{tag}.{side}.txt"))
        with open(paths[-1], "w") as f:
            f.write("".join(ln + "\n" for ln in lines))
    text = subprocess.run(["diff", *paths], capture_output=True, text=True).stdout
    return sum(ln[:1] in "<>" for ln in text.splitlines())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("rev", help="the revision to compare the working tree's instructions with")
    ap.add_argument("files", nargs="+", metavar="FILE.hip", help="files of smith-waterman_amd/csrc")
    a = ap.parse_args()
    files = [os.path.basename(f) for f in a.files]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        old = tree_at(a.rev, os.path.join(tmp, "old"))
        jobs = [(tree, f, os.path.join(tmp, f"{side}.{f}.s")) for f in files for side, tree in (("old", old), ("new", ROOT))]
        with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
            asm = list(pool.map(lambda j: assembly(*j), jobs))
        for n, f in enumerate(files):
            was, now = asm[2 * n], asm[2 * n + 1]
            iw, inow = instructions(was), instructions(now)
            d = differing(iw, inow, tmp, f)
            print(f"{f}: {len(iw)} instruction lines at {a.rev}, {len(inow)} in the tree, {d} differ")
            bad += d
            rw, rn = resources(was), resources(now)
            for k in list(rw) + [k for k in rn if k not in rw]:
                x, y = rw.get(k), rn.get(k)
                same = x == y
                bad += not same
                side = lambda r: "absent" if r is None else " ".join(f"{label} {r[label]}" for label, _ in RESOURCES)
                print(f"  {k}: {side(x)}" + ("" if same else f"  ->  {side(y)}  DIFFERS"))
    print(f"total: {'identical' if not bad else 'DIFFERENT'} ({len(files)} files compared with {a.rev})")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
