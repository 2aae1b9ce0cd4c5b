"""CPU: the PSSM update and the hit weights at their full size -- the cases tests/test_pssm_full_size_gpu.py runs on the device, held
here to the numpy rules (tests/pssm_hits_cases.py, tests/pssm_weights_cases.py), to their closed forms and to the planner before
anything runs on a GPU.
  * The 40-bit field (field_case): one query of 2^20 - 1 columns whose T_0 is (L - 3) 2^20 + 3 x 2^19, and 2^40 - 2^20 -- the largest
    the accumulator's low field can hold -- with one entry; the weights [21, 11] and [per_hit, 0]; the update on the same tables.
  * SUM = 2^32 (sum_case): 4096 entries of A_r = 2^20 at per_hit 1, 16 and 65535 (numerator 2^49), and the sibling at 2^32 - 2^20.
  * The second turn (second_turn_case): 2^20 + 3 queries of 9 tiles over a grid capped at 2^20 workgroups.  The planner is asked
    (through the two plan drivers) that there ARE more jobs than workgroups; the numpy rules walk the queries with a used entry, the
    rest is closed form; the host legs over the whole call are held to both.
The host legs are compared with the numpy rules on every case, so the GPU tests may take them as the expected values."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import pssm_hits_cases as hc
import pssm_weights_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, LMAX = wc.F, wc.LMAX


@pytest.mark.parametrize("second", [True, False])
def test_the_40_bit_field_closed_forms(swamd, second):
    c, T, A = wc.field_case(second)
    w, A_r, used = wc.reference(c, 16, 0)
    assert used[0].tolist() == [True, second]
    assert [int(a) for a in A_r[0]] == A                                  # the numpy rule gives the closed forms ...
    assert w[0].tolist() == wc.shares(A, 16) == ([21, 11] if second else [16, 0])
    assert T[0] >> 30 == 0x3FF                                            # the top ten bits of the field are all set
    if not second:
        assert T[0] == 2**40 - 2**20 and (wc.reference(c, 65535, 0)[0][0] == [65535, 0]).all()
    for per_hit in (1, 16, 65535):                                        # ... and the host leg equals the numpy rule
        assert (wc.host_leg(swamd, c, per_hit, 0) == wc.reference(c, per_hit, 0)[0]).all()


@pytest.mark.parametrize("second", [True, False])
def test_the_update_on_the_field_case(swamd, second):
    c, _, _ = wc.field_case(second)
    w = wc.host_leg(swamd, c, 16, 0)
    front = int(c.qoffs[0])
    for pw, weights in [(32, w), (0, None)]:
        exp_out, exp_cnt, used = hc.reference(c, pw, 0, weights)
        out, cnt = hc.host_leg(swamd, c, pw, 0, weights)
        assert (cnt == exp_cnt).all() and (out == exp_out[front:]).all()
        assert (hc.host_leg(swamd, c, pw, 0, weights, want_counts=False, in_place=True)[0] == out).all()
        wt = w[0].tolist() if weights is not None else [1, int(second)]   # every column was observed: the columns 5 .. 7 by both entries
        assert (exp_cnt.sum(axis=1)[[0, 5, 7, 8, LMAX - 1]] == [wt[0], wt[0] + wt[1], wt[0] + wt[1], wt[0], wt[0]]).all()


@pytest.mark.parametrize("sibling", [False, True])
def test_sum_2_to_the_32(swamd, sibling):
    c, A = wc.sum_case(sibling)
    S = sum(A)
    assert S == (2**32 - 2**20 if sibling else 2**32) and S >= 2**32 - 2**20 > 2**31
    for per_hit in (1, 16, 65535):
        exp = wc.shares(A, per_hit)
        w, A_r, used = wc.reference(c, per_hit, 0)
        assert used.all() and [int(a) for a in A_r[0]] == A and w[0].tolist() == exp
        if not sibling:
            assert exp == [per_hit] * 4096
        else:
            assert exp[0] == exp[1] and len(set(exp[2:])) == 1
            assert (exp[0], exp[2]) == {1: (1, 1), 16: (8, 16), 65535: (32776, 65535)}[per_hit]          # (32767.5 x (1 + 2^-12) + 1/2; 65551 before the clamp)
        assert (wc.host_leg(swamd, c, per_hit, 0) == w).all()
    assert 2**49 - 2**34 < 2 * 65535 * 4096 * F + S < 2**50                # the numerator: about 2^49, the header's "below 2^50"


# ---- the second turn ----

def _plan(tmp, driver, lines):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the planner")
    exe = str(tmp / driver)
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", driver + "_driver.cpp"),
                    os.path.join(ROOT, "smith-waterman_amd", "csrc", "sw_plan.cpp")], check=True)
    out = subprocess.run([exe], input=lines, capture_output=True, text=True, check=True).stdout
    return json.loads(out.splitlines()[0])


def test_the_planner_gives_every_workgroup_nine_jobs(tmp_path):
    """The premise of the second-turn case, from the planner itself: 9 tiles of 63 columns per query, a grid of 2^20 workgroups for nine
    times as many jobs (and 27 more), a finish grid of 2^20 for 2^20 + 3 queries."""
    c, used_q, _ = hc.second_turn_case()
    nq = len(c.qoffs) - 1
    qlens = ",".join(map(str, np.diff(c.qoffs).tolist()))
    h = _plan(tmp_path, "pssm_hits_plan", f"qlens={qlens} nletters=256 num_cus=256\n")
    w = _plan(tmp_path, "pssm_weights_plan", f"qlens={qlens} nletters=256 num_cus=256 top=1\n")
    for p in (h, w):
        assert p["tile_cols"] == hc.TURN_TILE and p["tiles_per_query"] == 9 and p["grid"] == hc.GRID_MAX
        assert nq * p["tiles_per_query"] == 9 * p["grid"] + 27
    assert w["finish_grid"] == hc.GRID_MAX == nq - 3 and w["acc_entries"] == nq


def test_second_turn_case_pairs_jobs_and_equals_the_rules(swamd):
    """second_turn_case() asserts the pairing of jobs inside the workgroups.  Here: the host legs on the queries with a used entry equal
    the numpy rules; the host legs over the WHOLE call equal those results placed into the closed form of every other query -- weight 0,
    counts 0, min(prior, smax)."""
    c, used_q, s = hc.second_turn_case()
    nq, inc = len(c.qoffs) - 1, hc.TURN_INCLUDE_MIN
    assert nq == hc.GRID_MAX + 3 and len(used_q) > 1500
    # the weights: top = 1, so per_hit where the entry has a counted pair
    ws, _, used = wc.reference(s, 16, inc)
    assert used.all() and (wc.host_leg(swamd, s, 16, inc) == ws).all() and (ws == 16).all()
    w = wc.host_leg(swamd, c, 16, inc)
    exp_w = np.zeros((nq, 1), np.int32)
    exp_w[used_q] = ws
    assert (w == exp_w).all()
    # the update on the queries with a used entry, weighted, with and without a prior weight
    front = int(s.qoffs[0])
    for pw in (32, 0):
        ro, rc, used = hc.reference(s, pw, inc, ws)
        ho, hcnt = hc.host_leg(swamd, s, pw, inc, ws)
        assert used.all() and (hcnt == rc).all() and (ho == ro[front:]).all()
        assert (rc.sum(axis=1) > 0).sum() == len(used_q) + 3 * 15          # one column per one-column query, sixteen per long one
    # the whole call (prior_weight 0: a column without counts costs the host leg nothing)
    out, cnt = hc.host_leg(swamd, c, 0, inc, w)
    exp_out, rows, exp_cnt = hc.second_turn_expected(c, used_q, ho, hcnt)
    assert (out == exp_out).all()
    assert (cnt[rows] == exp_cnt).all() and np.count_nonzero(cnt) == np.count_nonzero(exp_cnt)
