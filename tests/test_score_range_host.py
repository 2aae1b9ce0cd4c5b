"""CPU: what entitles tests/test_score_range_gpu.py (the case table of tests/score_range_cases.py) to its verdicts.

1. The oracle is exact over the whole range check_dims accepts: an independent restatement of the recurrence, written here over
   anti-diagonals in NumPy int64 (tie order diagonal, up, left with strict >; the lowest linear index wins the arg-max), agrees with
   oracle.fill in H, P and max_pos for every scoring of the case table, and oracle.fill_streaming agrees with oracle.fill.
2. Every case's expected route is what the planners (sw_plan.cpp, through tests/fill_plan_driver.cpp) decide for it.
3. The cases sit on their edges: the G-space peak of every inside case of B, the best score of the packed batch cases, the recipes
   of A."""
import json
import subprocess

import numpy as np
import pytest

import score_range_cases as T
from test_fill_plan import MI355X, driver  # noqa: F401  (the planner driver, built once per module)

FILLS, BATCHES, SEARCHES = T.fill_cases(), T.batch_cases(), T.search_cases()


def reference_fill(a, b, scores):
    match, mismatch, gap = (int(x) for x in scores)
    cols, rows = len(a), len(b)
    H = np.zeros((rows + 1, cols + 1), np.int64)
    P = np.zeros((rows + 1, cols + 1), np.int32)
    S = np.where(b[:, None] == a[None, :], match, mismatch).astype(np.int64)
    for d in range(2, rows + cols + 1):
        i = np.arange(max(1, d - cols), min(rows, d - 1) + 1)
        j = d - i
        best = np.zeros(len(i), np.int64)
        pred = np.zeros(len(i), np.int32)
        for cand, code in ((H[i - 1, j - 1] + S[i - 1, j - 1], 3), (H[i - 1, j] + gap, 1), (H[i, j - 1] + gap, 2)):
            m = cand > best
            best[m] = cand[m]
            pred[m] = code
        H[i, j] = best
        P[i, j] = pred
    return H, P, int(np.argmax(H))   # (the first of equal maxima in row-major order; 0 where nothing is positive)


def _scorings():
    """every scoring of the table that check_dims takes on 300 x 200, the near-2^24 search recipe included"""
    out = {c.scores for c in FILLS if c.valid} | {c.scores for c in BATCHES} | {c.scores for c in SEARCHES if c.scores}
    m = T.kScoreBits // 200 - 1
    out.add((m, -m // 3, -m // 5))
    return sorted(s for s in out if T.dims_ok(300, 200, s))


def _agree(oracle, a, b, scores, what):
    H, P, mp = reference_fill(a, b, scores)
    assert H.max() < T.kScoreBits and H.min() >= 0
    oH, oP, omp = oracle.fill(a, b, scores)
    assert np.array_equal(oH, H) and np.array_equal(oP, P) and omp == mp, what
    st = oracle.fill_streaming(a, b, scores)
    assert (st["max_pos"], st["max_score"]) == (mp, int(H.flat[mp])) and np.array_equal(st["bottom"], H[-1]), what
    assert np.array_equal(st["csH"], oracle.row_checksums(oH)) and np.array_equal(st["csP"], oracle.row_checksums(oP)), what


@pytest.mark.parametrize("scores", _scorings(), ids=lambda s: "m%d_x%d_g%d" % s)
def test_oracle_equals_the_int64_reference(oracle, scores):
    for recipe, cols, rows in (("corner", 300, 200), ("allmatch", 300, 200), ("random", 150, 200), ("periodic", 150, 200)):
        a, b = T.make_pair(recipe, cols, rows, T.seed_of(recipe) + abs(scores[0]))
        _agree(oracle, a, b, scores, (scores, recipe))


def test_oracle_equals_the_int64_reference_at_the_outer_limits(oracle):
    """the cases of C themselves: scores of 2^24 - 1, G-space of 2^31"""
    seen = set()
    for c in FILLS:
        key = (c.cols, c.rows, c.scores, c.recipe)
        if c.group != "C" or not c.valid or key in seen:
            continue
        seen.add(key)
        _agree(oracle, *c.pair(), c.scores, c.name)
    assert len(seen) >= 9


# ---- routes
def _run(driver, kind, kw):  # noqa: F811
    line = f"kind={kind} " + " ".join(f"{k}={int(v) if isinstance(v, bool) else v}" for k, v in kw.items())
    return json.loads(subprocess.run([driver], input=line + "\n", capture_output=True, text=True, check=True).stdout)


def _planned_last_cols(p):
    t = p["tiles"][-1]
    return t["cols"] if t["strips"] == 1 else t["cols"] - T.S2_W - (t["strips"] - 2) * p["W2"]


def test_fill_routes(driver):  # noqa: F811
    for c in FILLS:
        assert T.dims_ok(c.cols, c.rows, c.scores) == c.valid, c.name
        if not c.valid:
            continue
        p = _run(driver, "fill", {**MI355X, **c.plan_kw()})
        assert (p["perm"], p["two_cols"]) == (int(c.perm), int(c.two_cols)), c.name
        if c.w2:
            assert p["W2"] == c.w2, c.name
        if c.last_cols:
            assert _planned_last_cols(p) == c.last_cols, c.name
    cols, total, cuts, scores = T.band_case()
    kw = {**MI355X, "rows": cuts[0], "total_rows": total, "has_top_gran": 1, "has_bot_gran": 1, "match": scores[0], "mismatch": scores[1], "gap": scores[2]}
    p = _run(driver, "fill", {**kw, "cols": cols})
    assert (p["perm"], p["two_cols"]) == (1, 1)
    assert _run(driver, "fill", {**kw, "cols": cols + 2})["perm"] == 0


def test_fill_cases_cover_what_they_claim():
    names = {c.name for c in FILLS}
    for cols, rows in T.A_SHAPES:
        for sc in T.A_INSIDE:   # the match byte and the mismatch byte both at work
            assert {f"A-{cols}x{rows}-m{sc[0]}_x{sc[1]}_g{sc[2]}-{r}" for r in ("random", "corner", "allmatch")} <= names
    b_in = [c for c in FILLS if c.group == "B" and c.inside]
    assert {(c.w2, c.last_cols) for c in b_in} >= {(126, n) for n in T.B_LAST_126} | {(110, n) for n in T.B_LAST_110}
    assert T.widest_perm_cols(16, T.B_SCORES) == 265230 and 325000 < T.widest_perm_cols(T.B_STREAM_ROWS, T.B_STREAM_SCORES) < 326000
    assert all(c.perm and c.two_cols for c in b_in) and all(not c.perm for c in FILLS if c.group == "B" and not c.inside)


def test_tag_boundary_cases_peak_at_the_boundary(oracle):
    """G = H - gap (row + col) never decreases along a row or down a column (G[i][j] >= G[i-1][j], G[i][j-1]: the gap terms of the
    recurrence), so its largest value over the matrix is the bottom-right cell's: the streaming oracle's bottom row has it.  It must lie
    within 128 (-gap) + match rows of 2^24 - 1024: at most 125 columns given up to shape the last strip (one more for an even width),
    two gap steps that gmax counts and no cell has, and less than one column of rounding."""
    for c in FILLS:
        if c.group != "B" or not c.inside:
            continue
        match, _, gap = c.scores
        st = oracle.fill_streaming(*c.pair(), c.scores)
        peak = int(st["bottom"][-1]) - gap * (c.rows + c.cols) + T.kGBias
        room = T.kTagBit - T.kPermSlack - peak
        assert 0 < room <= 128 * -gap + match * c.rows, (c.name, peak, room)
        if c.recipe == "corner":   # ... and the diagonal really climbs into the corner
            assert st["bottom"][-1] >= match * c.rows // 2, c.name
    widest = next(c for c in FILLS if c.name == "B-16r-widest-random")
    assert widest.cols == 265230
    # the monotonicity itself, on whole matrices of the oracle: the largest G is the last cell's, and no G decreases to the right or downwards
    for c in (next(c for c in FILLS if c.name == n) for n in ("B-16r-widest-corner", "B-17r-s126-last1-random", "A-1007x304-m1_x-1_g-63-corner")):
        H = oracle.fill(*c.pair(), c.scores)[0].astype(np.int64)
        G = H - c.scores[2] * np.add.outer(np.arange(c.rows + 1), np.arange(c.cols + 1))
        assert G.max() == G[-1, -1] and (np.diff(G, axis=0) >= 0).all() and (np.diff(G, axis=1) >= 0).all(), c.name


def test_batch_routes(driver, oracle):  # noqa: F811
    for c in BATCHES:
        p = _run(driver, "batch", c.plan_kw())
        kernel = T.BATCH_FALLBACK if not p["wave"] else T.BATCH_WAVE16 if p["kernel"] >= 9 else T.BATCH_WAVE
        assert (bool(p["wave"]), kernel) == (c.wave, c.kernel), c.name
        assert p["C"] == T.lane_columns(c.cols)
        if c.score_line:
            A, B = c.pairs()
            best = max(oracle.fill_streaming(A[k], B[k], c.scores)["max_score"] for k in range(c.npairs))
            assert best >= 31800, c.name
    kernels = {(c.kernel, T.lane_columns(c.cols), c.mode) for c in BATCHES}
    assert {(T.BATCH_WAVE, C, m) for C in (4, 8, 16) for m in ("hp", "p8")} <= kernels
    assert {(T.BATCH_WAVE16, 16, "score"), (T.BATCH_WAVE16, 16, "p8"), (T.BATCH_FALLBACK, 8, "hp")} <= kernels
    assert all(c.npairs % 2 == 1 for c in BATCHES)


def test_search_routes(driver):  # noqa: F811
    for c in SEARCHES:
        _, _, offs = c.data()
        sc = c.scores_for(offs)
        p = _run(driver, "search", {"num_cus": 256, "search_per_cu": 8, "qlen": c.qlen, "maxlen": int(np.diff(offs).max()),
                                    "ntargets": int((np.diff(offs) > 0).sum()), "match": sc[0], "mismatch": sc[1], "gap": sc[2]})
        assert (p["C"], bool(p["wide"]), p["kernel"]) == (c.C, c.wide, c.kernel), c.name
        assert T.dims_ok(c.qlen, int(np.diff(offs).max()), sc), c.name
    assert {(c.C, c.wide) for c in SEARCHES} == {(C, w) for C in (4, 8, 16) for w in (False, True)}
