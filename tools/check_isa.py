#!/usr/bin/env python3
"""Post-build audit of the gfx950 ISA of sw_kernels.hip (run by `make check_isa`):
  * v126/v127 (landing registers of the hand-tracked edge prefetch) appear ONLY in the two asm
    statements that own them;
  * no scratch (spills) in the fill kernels, none at all in the search kernels (sw_search.hip, sw_search_affine.hip, sw_search_multi.hip, sw_search_multi16.hip)
    and the alignment kernels (sw_align_affine.hip, sw_align_hits.hip, sw_align_ckpt.hip), whose work counter is a vector buffer atomic."""
import re, subprocess, sys, os, tempfile
here = os.path.dirname(os.path.abspath(__file__))
src = os.path.join(here, "..", "smith-waterman_amd", "csrc", "sw_kernels.hip")
with tempfile.TemporaryDirectory() as td:
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++20", "-S", "--cuda-device-only", src,
                    "-o", os.path.join(td, "k.s")], check=True)
    s = open(os.path.join(td, "k.s")).read()
bad = []
for ln in s.splitlines():
    t = ln.split(";")[0]
    if re.search(r"\bv12[67]\b|v\[12[0-7]:12[67]\]|v\[126:", t):
        if not (("global_load_dwordx2 v[126:127]" in t) or re.match(r"\s*v_mov_b32(_e32)? v\d+, v12[67]\s*$", t)):
            bad.append(ln)
if bad:
    print("v126/v127 used outside the prefetch asm:\n" + "\n".join(bad)); sys.exit(1)
src2 = os.path.join(here, "..", "smith-waterman_amd", "csrc", "sw_systolic.hip")
with tempfile.TemporaryDirectory() as td:
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++20", "-S", "--cuda-device-only", src2,
                    "-o", os.path.join(td, "k.s")], check=True, stderr=subprocess.DEVNULL)
    s2 = open(os.path.join(td, "k.s")).read()
# (the systolic producer keeps literal registers strictly inside single asm statements, so there is
#  nothing to audit there besides scratch)
nprod = s2.count("SW_PRODUCER_PATH_BEGIN")
# (sw_systolic2 carries its prologue / epilogue since round 4: up to 64 bytes of spills in the per-strip set-up code are tolerated -- none may
#  sit in a loop: the producer / consumer loops are single asm statements, and every scratch access must lie outside any `Loop:` annotation)
for m in re.finditer(r"\.private_segment_fixed_size:\s*(\d+)", s2):
    if int(m.group(1)) > 64:
        print("scratch in use (systolic):", m.group(0)); sys.exit(1)
depth = 0
for ln in s2.splitlines():
    if "scratch_" in ln and "Loop" in ln:
        print("scratch access inside a loop (systolic):", ln.strip()); sys.exit(1)
# sw_traceback.hip keeps a 64-row window of P in the LITERAL registers v64..v127 (+ v62 / v63) ACROSS asm statements: no
# compiler-generated instruction may touch them; sw_batch.hip must not spill
def dev_asm(name):
    with tempfile.TemporaryDirectory() as td:
        subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++20", "-S", "--cuda-device-only",
                        os.path.join(here, "..", "smith-waterman_amd", "csrc", name), "-o", os.path.join(td, "k.s")], check=True, stderr=subprocess.DEVNULL)
        return open(os.path.join(td, "k.s")).read()
s3 = dev_asm("sw_traceback.hip")
inasm, bad3 = False, []
for ln in s3.splitlines():
    t = ln.strip()
    if t.startswith(";;#ASMSTART"): inasm = True; continue
    if t.startswith(";;#ASMEND"): inasm = False; continue
    if inasm or not t or t[0] in ";." or t.endswith(":"): continue
    regs = [int(x) for x in re.findall(r"\bv(\d+)\b", t)]
    for a, b in re.findall(r"v\[(\d+):(\d+)\]", t): regs += list(range(int(a), int(b) + 1))
    if any(62 <= r <= 127 for r in regs): bad3.append(ln)   # (the packed-matrix loader may use v128+ for its addresses)
if bad3:
    print("compiler code touches the traceback window registers v62..v127:\n" + "\n".join(bad3[:10])); sys.exit(1)
# (sw_batch_wave16<true> is held to 128 VGPRs -- four waves per SIMD -- and parks one address pair in scratch while it sets up a strip: 16 bytes allowed)
for txt, what, lim in ((s3, "traceback", 0), (dev_asm("sw_batch.hip"), "batch", 16)):
    for m in re.finditer(r"\.private_segment_fixed_size:\s*(\d+)", txt):
        if int(m.group(1)) > lim:
            print(f"scratch in use ({what}):", m.group(0)); sys.exit(1)
# sw_search.hip (database search): no scratch at all in the search kernels, and the work counter is taken with a VECTOR buffer atomic
s4 = dev_asm("sw_search.hip")
for m in re.finditer(r"\.private_segment_fixed_size:\s*(\d+)", s4):
    if int(m.group(1)) > 0:
        print("scratch in use (search):", m.group(0)); sys.exit(1)
nsearch = len(re.findall(r"^\s*\.name:\s+\S*sw_search_wave", s4, flags=re.M))
if nsearch < 6 or len(re.findall(r"^\s*buffer_atomic_add ", s4, flags=re.M)) < nsearch:
    print(f"search kernels: expected a vector buffer atomic work counter in each of {nsearch} kernels"); sys.exit(1)
# sw_search_affine.hip (affine search): the same two rules for its kernels
s5 = dev_asm("sw_search_affine.hip")
for m in re.finditer(r"\.private_segment_fixed_size:\s*(\d+)", s5):
    if int(m.group(1)) > 0:
        print("scratch in use (affine search):", m.group(0)); sys.exit(1)
naffine = len(re.findall(r"^\s*\.name:\s+\S*sw_search_affine_wave", s5, flags=re.M))
# (per kernel: the text from a kernel's label to its .Lfunc_end is that kernel's body)
bodies = re.findall(r"^(\S*sw_search_affine_wave\S*):[^\n]*\n(.*?)^\.Lfunc_end\d+:", s5, flags=re.M | re.S)
without = [name for name, body in bodies if not re.search(r"^\s*buffer_atomic_add ", body, flags=re.M)]
if naffine < 3 or len(bodies) != naffine or without:
    print(f"affine search kernels: expected a vector buffer atomic work counter in each of {naffine} kernels ({len(bodies)} bodies found, none in {without})"); sys.exit(1)
# sw_search_multi.hip (many queries against a prepared database): the same two rules for its three kernels
s7 = dev_asm("sw_search_multi.hip")
for m in re.finditer(r"\.private_segment_fixed_size:\s*(\d+)", s7):
    if int(m.group(1)) > 0:
        print("scratch in use (many-query search):", m.group(0)); sys.exit(1)
nmulti = len(re.findall(r"^\s*\.name:\s+\S*sw_search_affine_multi_wave", s7, flags=re.M))
bodies7 = re.findall(r"^(\S*sw_search_affine_multi_wave\S*):[^\n]*\n(.*?)^\.Lfunc_end\d+:", s7, flags=re.M | re.S)
without7 = [name for name, body in bodies7 if not re.search(r"^\s*buffer_atomic_add ", body, flags=re.M)]
if nmulti != 3 or len(bodies7) != nmulti or without7:
    print(f"many-query search kernels: expected a vector buffer atomic work counter in each of 3 kernels ({nmulti} kernels, {len(bodies7)} bodies found, none in {without7})"); sys.exit(1)
# sw_align_affine.hip (alignment of hits): no scratch at all
s6 = dev_asm("sw_align_affine.hip")
for m in re.finditer(r"\.private_segment_fixed_size:\s*(\d+)", s6):
    if int(m.group(1)) > 0:
        print("scratch in use (affine alignment):", m.group(0)); sys.exit(1)
nalign = len(re.findall(r"^\s*\.name:\s+\S*sw_align_affine_wave", s6, flags=re.M))
if nalign < 3:
    print(f"affine alignment kernels: expected 3, found {nalign}"); sys.exit(1)
# sw_align_hits.hip (alignment of a device hit table): no scratch at all in its three alignment kernels and two binning kernels, and the
# work counter of every alignment kernel is taken with a vector buffer atomic
s8 = dev_asm("sw_align_hits.hip")
for m in re.finditer(r"\.private_segment_fixed_size:\s*(\d+)", s8):
    if int(m.group(1)) > 0:
        print("scratch in use (hit-table alignment):", m.group(0)); sys.exit(1)
nhits = len(re.findall(r"^\s*\.name:\s+\S*sw_align_hits_wave", s8, flags=re.M))
nbin = len(re.findall(r"^\s*\.name:\s+\S*sw_align_hits_bin", s8, flags=re.M))
bodies8 = re.findall(r"^(\S*sw_align_hits_wave\S*):[^\n]*\n(.*?)^\.Lfunc_end\d+:", s8, flags=re.M | re.S)
without8 = [name for name, body in bodies8 if not re.search(r"^\s*buffer_atomic_add ", body, flags=re.M)]
if nhits != 3 or nbin != 2 or len(bodies8) != nhits or without8:
    print(f"hit-table alignment kernels: expected 3 alignment kernels with a vector buffer atomic work counter and 2 binning kernels ({nhits} + {nbin} kernels, {len(bodies8)} bodies found, none in {without8})"); sys.exit(1)
# sw_align_ckpt.hip (checkpointed alignment): the alignment kernels' two rules for its three kernels per item source
s9 = dev_asm("sw_align_ckpt.hip")
for m in re.finditer(r"\.private_segment_fixed_size:\s*(\d+)", s9):
    if int(m.group(1)) > 0:
        print("scratch in use (checkpointed alignment):", m.group(0)); sys.exit(1)
nckpt = len(re.findall(r"^\s*\.name:\s+\S*sw_align_ckpt_wave", s9, flags=re.M))
nckpth = len(re.findall(r"^\s*\.name:\s+\S*sw_align_hits_ckpt_wave", s9, flags=re.M))
bodies9 = re.findall(r"^(\S*sw_align_(?:hits_)?ckpt_wave\S*):[^\n]*\n(.*?)^\.Lfunc_end\d+:", s9, flags=re.M | re.S)
without9 = [name for name, body in bodies9 if not re.search(r"^\s*buffer_atomic_add ", body, flags=re.M)]
if nckpt != 3 or nckpth != 3 or len(bodies9) != 6 or without9:
    print(f"checkpointed alignment kernels: expected 3 + 3 kernels with a vector buffer atomic work counter ({nckpt} + {nckpth} kernels, {len(bodies9)} bodies found, none in {without9})"); sys.exit(1)
# sw_search_multi16.hip (the many-query search on packed 16-bit lanes): the same two rules for its three kernels
s10 = dev_asm("sw_search_multi16.hip")
for m in re.finditer(r"\.private_segment_fixed_size:\s*(\d+)", s10):
    if int(m.group(1)) > 0:
        print("scratch in use (packed many-query search):", m.group(0)); sys.exit(1)
npacked = len(re.findall(r"^\s*\.name:\s+\S*sw_search_multi_pk_wave", s10, flags=re.M))
bodies10 = re.findall(r"^(\S*sw_search_multi_pk_wave\S*):[^\n]*\n(.*?)^\.Lfunc_end\d+:", s10, flags=re.M | re.S)
without10 = [name for name, body in bodies10 if not re.search(r"^\s*buffer_atomic_add ", body, flags=re.M)]
if npacked != 3 or len(bodies10) != npacked or without10:
    print(f"packed many-query search kernels: expected a vector buffer atomic work counter in each of 3 kernels ({npacked} kernels, {len(bodies10)} bodies found, none in {without10})"); sys.exit(1)
n = len(re.findall(r"global_load_dwordx2 v\[126:127\]", s))
print(f"check_isa ok: {n} prefetch sites, v126/v127 private; {nprod} producer paths keep v100..v120 private; traceback window v62..v127 private; no scratch; {nsearch} search kernels without scratch; {naffine} affine search kernels without scratch; {nmulti} many-query search kernels without scratch; {nalign} affine alignment kernels without scratch; {nhits} + {nbin} hit-table alignment kernels without scratch; {nckpt} + {nckpth} checkpointed alignment kernels without scratch; {npacked} packed many-query search kernels without scratch")
