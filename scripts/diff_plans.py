#!/usr/bin/env python3
"""Are the plans of this tree those of another revision?

    python scripts/diff_plans.py REV [--random N] [--seed S]

builds every tests/*_plan_driver.cpp twice with g++ -- against sw_plan.cpp, sw_plan.h and sw_debug.h as `git show REV:` gives them (in a
temporary directory) and against the working tree --, feeds both builds the same job lines and compares their output lines as text.
The job lines: every line the plan tests give their drivers, recorded while the tests run (so they are the tests' own cases, not a
copy), and per driver a seeded random set drawn around the planners' thresholds.  Prints the lines compared and every differing line;
the exit status is 1 if any line differs.  A driver that does not build against REV's planner -- it drives a planner REV does not have
yet -- is run against the working tree alone and reported as such.  No GPU.

    python scripts/diff_plans.py --export FILE

writes the recorded job lines alone as JSON, {driver: [line, ...]} (tests/test_plan_sanitizers.py runs them under the sanitizers).
"""
import argparse
import glob
import json
import os
import random
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("smith-waterman_amd", "csrc")
PLAN_FILES = ["sw_plan.cpp", "sw_plan.h", "sw_debug.h"]
MIB = 1 << 20


def drivers():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(ROOT, "tests", "*_plan_driver.cpp")))


def build(tree, out_dir, flags=("-O1",), may_fail=False):
    """Every driver of the working tree against the planner under `tree`; returns {driver: executable}.  may_fail: a driver that does
    not build -- one whose planner `tree` does not have yet -- maps to None."""
    os.makedirs(out_dir, exist_ok=True)

    def one(name):
        exe = os.path.join(out_dir, name)
        p = subprocess.run(["g++", "-std=c++20", *flags, "-Wall", "-Werror", "-o", exe, os.path.join(tree, "tests", name + ".cpp"),
                            os.path.join(tree, CSRC, "sw_plan.cpp")], check=not may_fail, capture_output=may_fail)
        return name, exe if p.returncode == 0 else None
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        return dict(pool.map(one, drivers()))


def tree_at(rev, tmp):
    """A directory with the planner of `rev` and the drivers of the working tree, laid out as the repository."""
    os.makedirs(os.path.join(tmp, CSRC))
    os.makedirs(os.path.join(tmp, "tests"))
    for f in PLAN_FILES:
        text = subprocess.run(["git", "-C", ROOT, "show", f"{rev}:{CSRC}/{f}"], capture_output=True, check=True).stdout
        with open(os.path.join(tmp, CSRC, f), "wb") as out:
            out.write(text)
    for name in drivers():
        with open(os.path.join(ROOT, "tests", name + ".cpp"), "rb") as src, open(os.path.join(tmp, "tests", name + ".cpp"), "wb") as out:
            out.write(src.read())
    return tmp


def export_cases():
    """Runs the CPU tests that drive a plan driver and records every line they feed one: {driver: [line, ...]}, duplicates dropped."""
    import pytest
    files = []
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "test_*.py"))):
        with open(path) as f:
            text = f.read()
        if "_plan_driver" in text and "diff_plans" not in text:
            files.append(path)
    cases, exe_driver, real_run = {}, {}, subprocess.run

    def run(cmd, *args, **kw):
        if isinstance(cmd, (list, tuple)) and cmd:
            if cmd[0] == "g++" and "-o" in cmd:
                for src in cmd:
                    if os.path.basename(src)[:-4] in drivers() and src.endswith(".cpp"):
                        exe_driver[cmd[cmd.index("-o") + 1]] = os.path.basename(src)[:-4]
            elif cmd[0] in exe_driver and isinstance(kw.get("input"), str):
                seen = cases.setdefault(exe_driver[cmd[0]], {})
                for line in kw["input"].splitlines():
                    if line.strip():
                        seen.setdefault(line, None)
        return real_run(cmd, *args, **kw)

    class OnlyPlanTests:   # of a file that tests more than plans, the tests that take its `plan` fixture
        @staticmethod
        def pytest_collection_modifyitems(config, items):
            keep = [it for it in items if "plan" in os.path.basename(str(it.fspath)) or "plan" in getattr(it, "fixturenames", ())]
            config.hook.pytest_deselected(items=[it for it in items if it not in keep])
            items[:] = keep
    subprocess.run = run
    try:
        rc = pytest.main(["-q", "-m", "not gpu", "-p", "no:cacheprovider", *files], plugins=[OnlyPlanTests()])
    finally:
        subprocess.run = real_run
    if rc != 0:
        raise SystemExit(f"the plan tests did not pass (pytest exit {rc}): no cases exported")
    return {d: list(lines) for d, lines in cases.items()}


# ---- the random sets: drawn around the thresholds of the planners (columns per lane at 256 / 512, strips at 1024 / 2048, the 16-column
# occupancy rule, the packed bounds, the gap bound, the 32-bit item counter, small budgets and item limits)
QLENS = [1, 2, 8, 63, 64, 255, 256, 257, 300, 511, 512, 513, 700, 1023, 1024, 1025, 2047, 2048, 2049, 5000]
PER_CU = ["3", "5,4,3", "5,4,2", "5,4,1", "6,5,3", "2,2,2", "1,1,1"]
PER_CU6 = ["3", "5,5,4,4,2,2", "5,5,4,4,3,1", "5,5,4,4,1,3", "6,4,5,4,3,2"]
NONEMPTY = [0, 1, 2, 3, 7, 13, 40]
NONEMPTY_BIG = [1000, 200001, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, (1 << 33) + 5]


def kv(**fields):
    return " ".join(f"{k}={v}" for k, v in fields.items() if v is not None)


def queries(r, most=24):
    return ",".join(str(r.choice(QLENS)) for _ in range(r.randint(1, most)))


def ranks(r):
    """nonempty and max_items: a small item limit only with few targets (a launch per limit's worth of items is planned)."""
    if r.random() < 0.5:
        return {"nonempty": r.choice(NONEMPTY), "max_items": r.choice([2, 3, 5, 7, 10, 50, None])}
    return {"nonempty": r.choice(NONEMPTY + NONEMPTY_BIG), "max_items": None}


def budget(r):
    return r.choice([None, MIB, MIB, 4 * MIB])


def lanes_fields(r):
    return {"max_entry": r.choice([-5, 0, 1, 11, 31, 32, 127]), "gap_open": r.choice([-11, 0, -32766, -32767, -32768, -32769, -40000]),
            "gap_extend": r.choice([-1, 0, -2]), "lanes": r.choice([16, 16, 32]), "packed_per_cu": r.choice(PER_CU + ["4,0,1", "1,0,0"])}


def gen_search_multi(r):
    return kv(qlens=queries(r), per_cu=r.choice(PER_CU), longest=r.choice([1, 258, 259, 400, 1100, 100000]), budget_bytes=budget(r), **ranks(r))


def gen_search_multi_lanes(r):
    return kv(qlens=queries(r), per_cu=r.choice(PER_CU), longest=r.choice([1, 258, 259, 400, 1057, 1058, 1100, 100000]), budget_bytes=budget(r),
              **ranks(r), **lanes_fields(r))


def gen_prefilter(r):
    return kv(qlens=queries(r), per_cu=r.choice(PER_CU6), longest=r.choice([1, 258, 259, 400, 1100, 100000]), budget_bytes=budget(r),
              max_entry=r.choice([-5, 0, 1, 11, 31, 32, 126, 127]), lanes=r.choice([0, 0, 32]), **ranks(r))


def gen_search_pairs(r):
    return kv(qlens=queries(r), per_cu=r.choice(PER_CU), longest=r.choice([1, 400, 1100, 100000]), budget_bytes=budget(r),
              npairs=r.choice([0, 1, 63, 64, 65, 150, 1 << 22, (1 << 22) + 1, 1 << 31, (1 << 33) + 7]), chunk=r.choice([None, 1, 64, 1000, (1 << 31) - 1]))


def gen_search_pairs_lanes(r):
    return gen_search_pairs(r) + " " + kv(**lanes_fields(r))


def gen_align_hits(r):
    return kv(qlens=queries(r, 12), rep=r.choice([None, 1, 3, 50]), top=r.choice([1, 2, 5, 64, 4096]), longest=r.choice([0, 1, 300, 1100, 36000, 1 << 20]),
              budget_bytes=r.choice([None, MIB, 64 * MIB, 1 << 32]), profile_budget_bytes=budget(r), max_items=r.choice([None, 2, 7, 100, 1 << 31]),
              per_cu=r.choice(["3,3,3", "5,4,2", "5,4,1", "1,1,1"]), detail=r.choice([None, 1]))


def gen_align_ckpt(r):
    forced = r.choice([0, 0, 64, 256, 1024, 1 << 20])
    per_cu = r.choice(["3,3,3", "5,4,2", "5,4,1"])
    if r.random() < 0.5:
        return kv(what="one", len=r.choice([0, 1, 255, 256, 257, 5000, 36000, 1 << 20]), qlen=r.choice(QLENS), nhits=r.choice([1, 3, 1000, 100000]),
                  budget_bytes=r.choice([MIB, 64 * MIB, 1 << 30, 1 << 32]), forced=forced, per_cu=per_cu)
    return kv(what="hits", qlens=queries(r, 12), longest=r.choice([1, 300, 1100, 36000, 1 << 20]), top=r.choice([1, 5, 64]),
              budget_bytes=r.choice([MIB, 64 * MIB, 1 << 30, 1 << 32]), forced=forced, per_cu=per_cu, mode=r.choice([0, 1, 2]))


def gen_align_affine(r):
    return kv(qlen=r.choice(QLENS), maxhit=r.choice([0, 1, 300, 1100, 36000, 1 << 20]), nhits=r.choice([1, 3, 1000, 100000]),
              budget_mib=r.choice([1, 64, 1024, 4096]), per_cu=r.choice(PER_CU), lens=",".join(str(r.randint(0, 50)) for _ in range(r.randint(0, 8))) or None)


def gen_search_affine(r):
    return kv(qlen=r.choice(QLENS), maxlen=r.choice([1, 300, 1100, 36000, 1 << 20]), ntargets=r.choice([0, 1, 3, 4, 5, 1000, 1 << 22]),
              per_cu=r.choice(PER_CU), num_cus=r.choice([None, 1, 304]))


def gen_fill(r):
    kind = r.choice(["fill", "fill", "batch", "search"])
    if kind == "batch":
        return kv(kind=kind, cols=r.choice(QLENS), rows=r.choice(QLENS + [65000, 70000]), npairs=r.choice([1, 2, 64, 20000]), has_H=r.choice([0, 1]),
                  has_P=r.choice([0, 1]), p_elem_bytes=r.choice([1, 4]), match=r.choice([3, 4, 127, 128]), nletters=r.choice([4, 5, 8, 9]), n=r.choice([1, 2, 3]))
    if kind == "search":
        return kv(kind=kind, qlen=r.choice(QLENS), maxlen=r.choice([1, 300, 36000]), ntargets=r.choice([1, 4, 5, 1000, 1 << 22]), match=r.choice([3, 127, 128]),
                  search_per_cu=r.choice(["4", "8,8,6,6,4,4"]))
    n = r.choice([1000, 4096, 8192, 16384, 20480, 24576, 32768, 40000, 65536, 131072])
    return kv(cols=n + r.choice([0, 0, 1, 2]), rows=r.choice([n, 333, 4096, 2 * n]), h_elem_bytes=r.choice([4, 8]), p_elem_bytes=r.choice([1, 4]),
              has_H=r.choice([0, 1, 1]), has_P=r.choice([0, 1, 1]), has_result=1, full_stride=1, h_aligned=1, p_aligned=1, xcd_round_robin=r.choice([0, 1]),
              s2_per_cu=r.choice([0, 1]), s2w=r.choice([0, 0, 110, 126]), store_policy=r.choice([0, 1, 2]), filler_hop_ps=r.choice([0, 2400000]))


def gen_prologue(r):
    return f"{r.choice([2, 16384, 30001, 49151, 49152, 65536])} {r.choice([1, 16, 333, 16384, 49150, 65536])} {r.choice([0, 110, 126])} {r.choice([0, 1 << 28, 1 << 29])}"


def gen_search_top(r):
    return kv(nqueries=r.choice([0, 1, 64, 4096, 4097, 9000]), ntargets=r.choice([0, 1, 63, 4096, 4097, 300000, (1 << 31) - 1]), top=r.choice([1, 10, 4096]),
              budget_bytes=r.choice([MIB, 10 * MIB, 1 << 30, 1 << 40]), per_cu=r.choice([1, 4, 8]), num_cus=r.choice([None, 1, 304]))


def gen_top_pairs(r):
    return kv(npairs=r.choice([-1, 0, 1, 255, 256, 257, 4096, 4097, 132253, 12800000, (1 << 31) - 1, 1 << 31]), nqueries=r.choice([0, 1, 64, 8192, 8193, 100000]),
              ntargets=r.choice([0, 1, 5, 4097, (1 << 31) - 1, 1 << 31]), top=r.choice([0, 1, 3, 64, 65, 2049, 4096, 4097]), num_cus=r.choice([None, 1, 256]))


def gen_pssm_hits(r):
    return kv(qlens=queries(r), nletters=r.choice([1, 4, 20, 21, 25, 64, 255, 256]), num_cus=r.choice([None, 1, 256, 304]))


def gen_pssm_weights(r):
    return gen_pssm_hits(r) + " " + kv(top=r.choice([1, 2, 10, 100, 4095, 4096]))


def gen_msa_hits(r):
    return kv(nqueries=r.choice([0, 1, 3, 64, 255, 256, 257, 5000, 1 << 20, (1 << 20) + 5]), top=r.choice([1, 2, 4, 5, 10, 100, 4095, 4096]),
              num_cus=r.choice([None, 1, 256, 304]), rows=r.choice([0, 1, 1]))


def gen_msa_filter(r):
    return kv(nqueries=r.choice([0, 1, 3, 64, 300, 5000, 1 << 20, (1 << 20) + 5]), top=r.choice([1, 2, 63, 64, 65, 100, 1000, 4095, 4096]),
              budget_bytes=r.choice([0, 1 << 20, 3 << 20, (3 << 20) + 1, 256 << 20, 1 << 40]), tiles=r.choice([0, 0, 1]))


def gen_score_hist(r):
    return kv(nqueries=r.choice([0, 1, 3, 64, 70, 4096, 1 << 20, (1 << 20) + 5]), ntargets=r.choice([0, 1, 63, 64, 65, 257, 4095, 4096, 4097, 5000, 25000, 200000, (1 << 31) - 1]),
              num_cus=r.choice([1, 256, 304]), copies=r.choice([0, 0, 1, 2, 4]))


def gen_mask(r):
    return kv(letters=r.choice([0, 1, 63, 64, 4095, 4096, 4097, 70_000_000, (1 << 31) - 1, 1 << 33]), ntargets=r.choice([0, 1, 255, 256, 257, 200_000, 1 << 30]),
              window=r.choice([2, 12, 63, 64]), count=r.choice([0, 1]))


GENERATORS = {"search_multi_plan_driver": gen_search_multi, "search_multi_lanes_plan_driver": gen_search_multi_lanes, "prefilter_plan_driver": gen_prefilter,
              "search_pairs_plan_driver": gen_search_pairs, "search_pairs_lanes_plan_driver": gen_search_pairs_lanes, "align_hits_plan_driver": gen_align_hits,
              "align_ckpt_plan_driver": gen_align_ckpt, "align_affine_plan_driver": gen_align_affine, "search_affine_plan_driver": gen_search_affine,
              "fill_plan_driver": gen_fill, "prologue_plan_driver": gen_prologue, "search_top_plan_driver": gen_search_top,
              "top_pairs_plan_driver": gen_top_pairs, "pssm_hits_plan_driver": gen_pssm_hits,
              "pssm_weights_plan_driver": gen_pssm_weights, "msa_hits_plan_driver": gen_msa_hits,
              "msa_filter_plan_driver": gen_msa_filter, "mask_plan_driver": gen_mask, "score_hist_plan_driver": gen_score_hist}


def random_cases(n, seed):
    out = {}
    for name in drivers():
        r = random.Random(f"{seed}:{name}")
        out[name] = [GENERATORS[name](r) for _ in range(n)]
    return out


def run_lines(exe, lines):
    p = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True)
    if p.returncode != 0:
        raise SystemExit(f"{exe} exited with {p.returncode}: {p.stderr[-2000:]}")
    return p.stdout.splitlines()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("rev", nargs="?", help="the revision to compare the working tree's plans with")
    ap.add_argument("--export", metavar="FILE", help="write the job lines of the plan tests as JSON and stop")
    ap.add_argument("--random", type=int, default=1500, help="random job lines per driver (default 1500)")
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    missing = [d for d in drivers() if d not in GENERATORS]
    if missing:
        raise SystemExit(f"no random set for {missing}: add a generator")
    cases = export_cases()
    if a.export:
        with open(a.export, "w") as f:
            json.dump(cases, f)
        return 0
    if not a.rev:
        ap.error("REV or --export is needed")
    rnd = random_cases(a.random, a.seed)
    differing = compared = 0
    with tempfile.TemporaryDirectory() as tmp:
        old = build(tree_at(a.rev, os.path.join(tmp, "old")), os.path.join(tmp, "bin_old"), may_fail=True)
        new = build(ROOT, os.path.join(tmp, "bin_new"))
        for name in drivers():
            lines = cases.get(name, []) + rnd[name]
            if old[name] is None:
                print(f"{name}: does not build against the planner of {a.rev} (a planner that revision lacks): {len(run_lines(new[name], lines))} lines run, none compared")
                continue
            was, now = run_lines(old[name], lines), run_lines(new[name], lines)
            if len(was) != len(now) or len(was) != len(lines):
                raise SystemExit(f"{name}: {len(lines)} job lines gave {len(was)} and {len(now)} output lines")
            bad = [i for i in range(len(lines)) if was[i] != now[i]]
            for i in bad[:5]:
                print(f"{name}: DIFFERS for `{lines[i]}`\n  {a.rev}: {was[i][:400]}\n  tree: {now[i][:400]}")
            print(f"{name}: {len(lines)} lines compared ({len(cases.get(name, []))} from the tests, {len(rnd[name])} random), {len(bad)} differ")
            compared += len(lines)
            differing += len(bad)
    print(f"total: {compared} lines compared with {a.rev}, {differing} differ")
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
