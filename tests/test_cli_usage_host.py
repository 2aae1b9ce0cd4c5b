"""No GPU: what smithW answers to a command line it refuses, and to input files it cannot read -- every message of main() and what the
modes refuse before they open a device -- is what the CLI before "The CLI's shared parts"  answered: exit status, stdout and
stderr as bytes, for command lines that break one rule and for ones that break several, where the order of the checks decides the
message.  tests/golden/cli_usage.json holds the command lines, the small input files and the answers, recorded from that CLI by
scripts/diff_cli.py REV --export; temporary paths stand as {NAME}, and in a "smithW: <call> -> N:" line the text of the call is cut
down to the function's name, as the script cuts it."""
import json
import os
import sys

import pytest

from oracle_lib import ROOT

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import diff_cli  # noqa: E402

CLI = os.path.join(ROOT, "smith-waterman_amd", "smithW")
with open(os.path.join(ROOT, "tests", "golden", "cli_usage.json")) as f:
    GOLDEN = json.load(f)
CASES = GOLDEN["cases"]


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """Every case run once, one process at a time."""
    assert os.path.exists(CLI), "build() makes the CLI"
    return diff_cli.run_usage(CLI, GOLDEN["files"], [c["args"] for c in CASES], str(tmp_path_factory.mktemp("cli_usage")))


@pytest.mark.parametrize("k", range(len(CASES)), ids=lambda k: f"{k}:" + " ".join(CASES[k]["args"])[:70])
def test_the_answer_is_that_of_the_cli_before(answers, k):
    status, out, err = CASES[k]["expect"]
    assert answers[k] == [status, out, err]
    assert status in (1, 2) and out == "" and err.count("\n") == 1 and (err.startswith("smithW: ") or err.startswith("usage: smithW "))


def test_the_cases_trip_every_refusal_of_main():
    """Every 'smithW: ...' message main() can print stands in the golden at least once (read from the source, so a new rule needs a case)."""
    import re
    with open(os.path.join(ROOT, "smith-waterman_amd", "cli", "smithW.cpp")) as f:
        text = f.read()
    text = text[text.index("static Mode refuse("):]
    messages = re.findall(r'refuse\("((?:[^"\\]|\\.)*)"', text) + re.findall(r'byte_scores\(o\.sc, "([^"]*)"', text)
    assert len(messages) >= 40
    said = "\n".join(c["expect"][2] for c in CASES)
    for m in messages:
        fixed = re.split(r"%lld|%d|%s", m.replace('\\"', '"'))   # the message around its numbers
        assert all(part in said for part in fixed if part.strip()), m
