"""CPU: the planners (smith-waterman_amd/csrc/sw_plan.cpp) under the sanitizers.  Every tests/*_plan_driver.cpp, a program of its own,
is built with sw_plan.cpp under -fsanitize=address,undefined and fed every job line the plan tests give that driver
(scripts/diff_plans.py --export records them while those tests run, so the lines are theirs).  A clean exit is the test: the plans
themselves are checked by the plan tests and, against another revision, by scripts/diff_plans.py.  Nothing is loaded into Python."""
import importlib.util
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def test_planners_are_clean_under_the_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the plan drivers")
    spec = importlib.util.spec_from_file_location("diff_plans", os.path.join(ROOT, "scripts", "diff_plans.py"))
    diff_plans = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(diff_plans)
    cases_file = str(tmp_path / "cases.json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "diff_plans.py"), "--export", cases_file], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with open(cases_file) as f:
        cases = json.load(f)
    exes = diff_plans.build(ROOT, str(tmp_path / "bin"), SANITIZE)
    assert sorted(cases) == sorted(exes) == diff_plans.drivers()      # every driver has cases of the tests
    for name, exe in exes.items():
        lines = cases[name]
        assert lines, name
        p = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True)
        assert p.returncode == 0 and p.stderr == "", (name, p.returncode, p.stderr[-2000:])
        assert len(p.stdout.splitlines()) == len(lines), name
