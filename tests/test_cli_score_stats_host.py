"""No GPU: what smithW answers to the command lines the statistics flags (--evalue, --include-evalue, --score-shift) are refused on --
exit status 2, nothing on stdout, one line on stderr --, in the manner of tests/test_cli_usage_host.py but with the expectations here:
every rule of score_stats_rule (smith-waterman_amd/cli/cli_parts.h), for command lines that break one rule and for ones that break
several, where the order of the rules decides the message; and the flags' values that are no numbers."""
import os
import re
import sys

import pytest

from oracle_lib import ROOT

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import diff_cli  # noqa: E402

CLI = os.path.join(ROOT, "smith-waterman_amd", "smithW")
MANY = ["--search", "{Q}", "{DB}", "--all-queries"]
PSSM = ["--search", "--pssm", "{PSSM}", "{DB}", "--gap-open", "-6", "--gap-extend", "-1"]
CENSORED = "smithW: --evalue / --include-evalue do not go with --prefilter / --prefilter-hits / --pairs (the fit needs every score, not a censored sample)\n"
WHERE = "smithW: --evalue / --include-evalue go with --search --all-queries or --search --pssm\n"
CASES = [
    # E <= 0
    (MANY + ["--evalue", "0"], "smithW: --evalue E needs E > 0, got 0\n"),
    (MANY + ["--evalue", "-1e-3"], "smithW: --evalue E needs E > 0, got -0.001\n"),
    (MANY + ["--evalue", "nan"], "smithW: --evalue E needs E > 0, got nan\n"),
    (MANY + ["--iterations", "2", "--include-evalue", "0"], "smithW: --include-evalue E needs E > 0, got 0\n"),
    (PSSM + ["--evalue", "-2"], "smithW: --evalue E needs E > 0, got -2\n"),
    # a shift outside 0..16, and a shift alone
    (MANY + ["--evalue", "1", "--score-shift", "17"], "smithW: --score-shift N needs N within 0..16, got 17\n"),
    (MANY + ["--evalue", "1", "--score-shift", "-1"], "smithW: --score-shift N needs N within 0..16, got -1\n"),
    (MANY + ["--score-shift", "3"], "smithW: --score-shift goes with --evalue or --include-evalue\n"),
    (["--score-shift", "3"], "smithW: --score-shift goes with --evalue or --include-evalue\n"),
    # either flag with --prefilter, --prefilter-hits or --pairs
    (MANY + ["--evalue", "1", "--prefilter", "20"], CENSORED),
    (MANY + ["--evalue", "1", "--prefilter-hits", "20"], CENSORED),
    (["--search", "{Q}", "{DB}", "--evalue", "1", "--pairs", "{PAIRS}"], CENSORED),
    (MANY + ["--iterations", "2", "--include-evalue", "1", "--prefilter-hits", "20"], CENSORED),
    (MANY + ["--iterations", "2", "--include-evalue", "1", "--prefilter", "20"], CENSORED),
    (["--search", "{Q}", "{DB}", "--iterations", "2", "--include-evalue", "1", "--pairs", "{PAIRS}"], CENSORED),
    # either flag without --all-queries / --pssm
    (["--search", "{Q}", "{DB}", "--evalue", "1"], WHERE),
    (["--search", "{Q}", "{DB}", "--include-evalue", "1"], WHERE),
    (["--evalue", "1"], WHERE),
    (["--fasta", "{Q}", "{DB}", "--evalue", "1"], WHERE),
    (["100", "100", "--include-evalue", "1"], WHERE),
    # --include-evalue with --include-score, and without --iterations
    (MANY + ["--iterations", "2", "--include-evalue", "1", "--include-score", "30"], "smithW: --include-evalue does not go with --include-score\n"),
    (PSSM + ["--iterations", "3", "--include-score", "30", "--include-evalue", "1"], "smithW: --include-evalue does not go with --include-score\n"),
    (MANY + ["--include-evalue", "1"], "smithW: --include-evalue goes with --iterations N (N > 1)\n"),
    (MANY + ["--include-evalue", "1", "--iterations", "1"], "smithW: --include-evalue goes with --iterations N (N > 1)\n"),
    (MANY + ["--include-evalue", "1", "--out-pssm", "{MISSING}"], "smithW: --include-evalue goes with --iterations N (N > 1)\n"),
    (PSSM + ["--include-evalue", "1", "--evalue", "1"], "smithW: --include-evalue goes with --iterations N (N > 1)\n"),
    # several rules broken: the first one speaks
    (["--search", "{Q}", "{DB}", "--evalue", "0", "--pairs", "{PAIRS}"], "smithW: --evalue E needs E > 0, got 0\n"),
    (MANY + ["--evalue", "1", "--score-shift", "40", "--prefilter", "3"], "smithW: --score-shift N needs N within 0..16, got 40\n"),
    (["--search", "{Q}", "{DB}", "--include-evalue", "1", "--include-score", "3", "--prefilter-hits", "3"], CENSORED),
    (["--search", "{Q}", "{DB}", "--include-evalue", "1", "--include-score", "3"], WHERE),
    # the rules of the flags that were there before still speak where the new ones hold
    (MANY + ["--evalue", "1", "--search-lanes", "8"], "smithW: --search-lanes takes 16 or 32, got 8\n"),
    (MANY + ["--evalue", "1", "--iterations", "0"], "smithW: --iterations N needs N >= 1, got 0\n"),
    # values that are no numbers
    (MANY + ["--evalue", "x"], "smithW: --evalue needs a number, got \"x\"\n"),
    (MANY + ["--evalue", "1e"], "smithW: --evalue needs a number, got \"1e\"\n"),
    (MANY + ["--iterations", "2", "--include-evalue", ""], "smithW: --include-evalue needs a number, got \"\"\n"),
    (MANY + ["--evalue", "1", "--score-shift", "2k"], "smithW: --score-shift needs an integer, got \"2k\"\n"),
]


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """Every case run once, one process at a time."""
    assert os.path.exists(CLI), "build() makes the CLI"
    return diff_cli.run_usage(CLI, diff_cli.usage_files(), [args for args, _ in CASES], str(tmp_path_factory.mktemp("cli_score_stats")))


@pytest.mark.parametrize("k", range(len(CASES)), ids=lambda k: f"{k}:" + " ".join(CASES[k][0])[:70])
def test_the_refusal(answers, k):
    assert answers[k] == [2, "", CASES[k][1]]


def test_the_cases_trip_every_rule():
    """Every message score_stats_rule can return stands in the expectations at least once (read from the source, so a new rule needs a case)."""
    with open(os.path.join(ROOT, "smith-waterman_amd", "cli", "cli_parts.h")) as f:
        text = f.read()
    text = text[text.index("static std::string score_stats_rule("):]
    text = text[:text.index("\n}\n")]
    messages = re.findall(r'"(--(?:[^"\\]|\\.)*)"', text)
    assert len(messages) >= 8
    said = "\n".join(err for _, err in CASES)
    for m in messages:
        fixed = re.split(r"%lld|%d|%s|%g", m)
        assert all(part in said for part in fixed if part.strip()), m
