"""No GPU: what smithW answers to the command lines --mask and its sub-flags are refused on -- exit status 2, nothing on stdout, one
line on stderr --, in the manner of tests/test_cli_score_stats_host.py: every rule of mask_rule (smith-waterman_amd/cli/cli_parts.h),
for command lines that break one rule and for ones that break several, where the order of the rules decides the message; and the
values that are no integers."""
import os
import re
import sys

import pytest

from oracle_lib import ROOT

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import diff_cli  # noqa: E402

CLI = os.path.join(ROOT, "smith-waterman_amd", "smithW")
ONE = ["--search", "{Q}", "{DB}"]
MANY = ONE + ["--all-queries"]
SUB = "smithW: --mask-window / --mask-trigger / --mask-extend / --mask-byte / --mask-letters go with --mask\n"
WHERE = "smithW: --mask goes with --search\n"
CASES = [
    # a sub-flag without --mask
    (MANY + ["--mask-window", "12"], SUB),
    (ONE + ["--mask-trigger", "2200"], SUB),
    (ONE + ["--mask-extend", "2500"], SUB),
    (MANY + ["--mask-byte", "X"], SUB),
    (["--mask-letters", "ACGT"], SUB),
    # --mask without --search
    (["--mask"], WHERE),
    (["100", "100", "--mask"], WHERE),
    (["--fasta", "{Q}", "{DB}", "--mask", "--mask-window", "8"], WHERE),
    # values out of range
    (ONE + ["--mask", "--mask-window", "1"], "smithW: --mask-window W needs W within 2..64, got 1\n"),
    (MANY + ["--mask", "--mask-window", "65"], "smithW: --mask-window W needs W within 2..64, got 65\n"),
    (MANY + ["--mask", "--mask-trigger", "-1"], "smithW: --mask-trigger MB needs MB >= 0 (thousandths of a bit), got -1\n"),
    (MANY + ["--mask", "--mask-extend", "2199"], "smithW: --mask-extend MB needs MB >= the trigger's 2200, got 2199\n"),
    (MANY + ["--mask", "--mask-trigger", "3000"], "smithW: --mask-extend MB needs MB >= the trigger's 3000, got 2500\n"),
    (ONE + ["--mask", "--mask-byte", "XY"], "smithW: --mask-byte C takes one character, got \"XY\"\n"),
    (ONE + ["--mask", "--mask-byte", ""], "smithW: --mask-byte C takes one character, got \"\"\n"),
    (MANY + ["--mask", "--mask-letters", ""], "smithW: --mask-letters STR takes 1..32 letters, got 0\n"),
    (MANY + ["--mask", "--mask-letters", "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefg"], "smithW: --mask-letters STR takes 1..32 letters, got 33\n"),
    (MANY + ["--mask", "--mask-letters", "ACGTA"], "smithW: --mask-letters names 'A' twice\n"),
    # several rules broken: the first one speaks
    (["--mask-window", "1"], SUB),
    (["--mask", "--mask-window", "1"], WHERE),
    (MANY + ["--mask", "--mask-window", "0", "--mask-trigger", "-5"], "smithW: --mask-window W needs W within 2..64, got 0\n"),
    (MANY + ["--mask", "--mask-trigger", "-5", "--mask-letters", "AA"], "smithW: --mask-trigger MB needs MB >= 0 (thousandths of a bit), got -5\n"),
    # the rules of the flags that were there before still speak where the new ones hold, and before them
    (MANY + ["--mask", "--search-lanes", "8"], "smithW: --search-lanes takes 16 or 32, got 8\n"),
    (MANY + ["--mask", "--mask-window", "1", "--evalue", "0"], "smithW: --evalue E needs E > 0, got 0\n"),
    (MANY + ["--mask", "--iterations", "0"], "smithW: --iterations N needs N >= 1, got 0\n"),
    # values that are no integers
    (MANY + ["--mask", "--mask-window", "x"], "smithW: --mask-window needs an integer, got \"x\"\n"),
    (MANY + ["--mask", "--mask-trigger", "2.2"], "smithW: --mask-trigger needs an integer, got \"2.2\"\n"),
    (MANY + ["--mask", "--mask-extend", ""], "smithW: --mask-extend needs an integer, got \"\"\n"),
]


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """Every case run once, one process at a time."""
    assert os.path.exists(CLI), "build() makes the CLI"
    return diff_cli.run_usage(CLI, diff_cli.usage_files(), [args for args, _ in CASES], str(tmp_path_factory.mktemp("cli_mask")))


@pytest.mark.parametrize("k", range(len(CASES)), ids=lambda k: f"{k}:" + " ".join(CASES[k][0])[:70])
def test_the_refusal(answers, k):
    assert answers[k] == [2, "", CASES[k][1]]


def test_the_cases_trip_every_rule():
    """Every message mask_rule can return stands in the expectations at least once (read from the source, so a new rule needs a case)."""
    with open(os.path.join(ROOT, "smith-waterman_amd", "cli", "cli_parts.h")) as f:
        text = f.read()
    text = text[text.index("static std::string mask_rule("):]
    text = text[:text.index("\n}\n")]
    messages = re.findall(r'"(--(?:[^"\\]|\\.)*)"', text)
    assert len(messages) >= 8
    said = "\n".join(err for _, err in CASES)
    for m in messages:
        fixed = re.split(r"%lld|%d|%s|%c", m.replace('\\"', '"'))
        assert all(part in said for part in fixed if part.strip()), m
