"""No GPU: sw_traceback_host_ex on hand-made predecessor matrices (tests/traceback_cases.py, families 1-6; int32 and int8) against the
plain reference walk, and the reference walk itself against the oracle's backtrack() on every generated case."""
import ctypes

import numpy as np
import pytest

import traceback_cases as tc

FAMILIES = {"runs": tc.family_runs(), "alignments": tc.family_alignments(), "edges": tc.family_edges(), "shapes": tc.family_shapes(),
            "random": tc.family_random()}
ALL = [c for f in FAMILIES.values() for c in f]


def test_ref_walk_is_the_oracles_backtrack(oracle):
    """The new reference pinned to the existing one: same path, same negated matrix, on every small case of every family."""
    for case in ALL + tc.family_caps():
        P, pos = case.build(np.int32)
        Q = P.copy()
        path = tc.ref_walk(P, pos)
        assert np.array_equal(path, oracle.backtrack(Q, pos)) and np.array_equal(P, Q), case.name
        assert np.array_equal(np.abs(P), case.build(np.int32)[0]) and np.array_equal(np.flatnonzero(P.reshape(-1) < 0), np.sort(path)), case.name


def test_random_family_reaches_every_exit_with_both_walkers():
    """Family 5 on the reference alone: at least 200 cases, LEFT and UP runs of a whole window and more, and every way out of a window
    (top, left by DIAGONAL, left by LEFT, the end of the path) from windows with the cursor in row 63 and from windows clamped at the top."""
    cases = FAMILIES["random"]
    assert len(cases) >= 200
    seen, longest = set(), {tc.LEFT: 0, tc.UP: 0, tc.DIAGONAL: 0}
    for case in cases:
        P, pos = case.build(np.int32)
        path = tc.ref_walk(P, pos)
        codes = tc.path_codes(P, path)
        for code in longest:
            longest[code] = max(longest[code], tc.longest_run(codes, code))
        seen |= {(w["exit"], w["ti"] == 63) for w in tc.windows_of(path, codes, case.m)}
    assert min(longest.values()) >= 300
    assert seen >= {(e, r) for e in ("end", "top", "left-diag", "left-left") for r in (True, False)} - {("top", False)}


def test_shape_family_covers_every_corner_phase():
    assert {c.m % 4 for c in FAMILIES["shapes"]} == {0, 1, 2, 3} and len(FAMILIES["shapes"]) == len(tc.SHAPES) ** 2
    assert {(c.rows1 < 64, c.m < 64) for c in FAMILIES["shapes"]} == {(a, b) for a in (True, False) for b in (True, False)}


def test_alignment_family_clamps_first_windows_every_way():
    got = {(c.start[0] < 63, c.start[1] < 63) for c in FAMILIES["alignments"] if c.start[0] and c.start[1]}
    assert got == {(a, b) for a in (True, False) for b in (True, False)}
    assert {(c.start[0] % 64, c.start[1] % 64) for c in FAMILIES["alignments"]} == {(a, b) for a in (0, 1, 62, 63) for b in (0, 1, 62, 63)}


@pytest.mark.parametrize("dtype", [np.int32, np.int8], ids=["int32", "int8"])
@pytest.mark.parametrize("case", ALL, ids=str)
def test_host_traceback_on_a_hand_made_matrix(swamd, case, dtype):
    P, pos = case.build(dtype)
    ref = P.copy()
    want = tc.ref_walk(ref, pos)
    tc.check_property(case, ref, want)
    got = swamd.traceback_host(P, pos)
    assert len(got) == len(want) and np.array_equal(got, want)
    assert np.array_equal(P, ref), "every decoy untouched, every path cell negated"


@pytest.mark.parametrize("dtype", [np.int32, np.int8], ids=["int32", "int8"])
@pytest.mark.parametrize("case", tc.family_caps(), ids=str)
def test_host_traceback_path_cap(swamd, case, dtype):
    """path_cap smaller than, equal to and larger than the path: the first min(cap, n) entries, nothing after them, the full length
    and the whole path negated all the same."""
    P0, pos = case.build(dtype)
    ref = P0.copy()
    want = tc.ref_walk(ref, pos)
    tc.check_property(case, ref, want)
    n = len(want)
    L = swamd.lib()
    for cap in tc.cap_values(n):
        P = P0.copy()
        buf = np.full(n + 80, tc.SENTINEL, np.int64)
        plen = ctypes.c_int64(-7)
        assert L.sw_traceback_host_ex(P.ctypes.data, P.dtype.itemsize, case.m - 1, case.rows1 - 1, pos, buf.ctypes.data, cap, ctypes.byref(plen)) == 0
        k = min(cap, n)
        assert plen.value == n, f"cap {cap}"
        assert np.array_equal(buf[:k], want[:k]) and (buf[k:] == tc.SENTINEL).all(), f"cap {cap}"
        assert np.array_equal(P, ref), f"cap {cap}"
    # no path buffer at all
    P = P0.copy()
    plen = ctypes.c_int64(-7)
    assert L.sw_traceback_host_ex(P.ctypes.data, P.dtype.itemsize, case.m - 1, case.rows1 - 1, pos, None, 0, ctypes.byref(plen)) == 0
    assert plen.value == n and np.array_equal(P, ref)
