"""Hand-made predecessor matrices for the traceback kernels, and a plain reference walk (a helper module, not a conftest).

The traceback entry points take P as plain input, so a test can write any matrix it likes instead of waiting for a fill of random
sequences to produce one -- such fills give almost pure diagonals.  make_case() draws a matrix of random codes (the decoys: a walk
that takes one wrong step lands on a random code and goes visibly astray) and writes a path into it as a list of (code, count) runs;
ref_walk() is backtrack() (serial_smithW.c:262-277) as a Python loop.  The families below are the case lists that the host tests
(test_traceback_host.py) and the GPU tests (test_traceback_synthetic_gpu.py) share; every case is a `Case` whose matrix is built on
demand from its seed, so collecting the tests costs nothing."""
from dataclasses import dataclass

import numpy as np

NONE, UP, LEFT, DIAGONAL = 0, 1, 2, 3
W = 64   # the window of csrc/sw_traceback.hip: 64 rows x 64 columns, the cursor in its bottom-right part
BORDER = "border"   # last element of a plan: do not end the path with a NONE cell, let it run into row 0 / column 0


def np_pack(P):
    """The 2-bit format by definition: cell k in bits 2 (k & 3) of byte k >> 2; path bitmap bit k & 31 of word k >> 5."""
    flat = P.reshape(-1).astype(np.int64)
    n = flat.size
    pad = (-n) % 32
    codes = np.concatenate([np.abs(flat), np.zeros(pad, np.int64)]).astype(np.uint8).reshape(-1, 4)
    p2 = (codes[:, 0] | (codes[:, 1] << 2) | (codes[:, 2] << 4) | (codes[:, 3] << 6)).astype(np.uint8)
    neg = np.concatenate([flat < 0, np.zeros(pad, bool)]).reshape(-1, 32)
    bits = (neg.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)
    return p2, bits


def pack_codes(flat):
    """np_pack's code bytes for a flat array of codes 0..3 without the int64 detour (the big matrices of family 7)."""
    n = flat.size
    nbytes = ((n + 31) // 32) * 8
    src = flat
    if n != nbytes * 4:
        src = np.zeros(nbytes * 4, flat.dtype)
        src[:n] = flat
    q = src.reshape(-1, 4).view(np.uint8)
    out = q[:, 0] | (q[:, 1] << 2)
    out |= q[:, 2] << 4
    out |= q[:, 3] << 6
    return out


def path_bitmap(path, ncells):
    """The path bitmap of a walk over `path` (linear indices), word for word as the kernel must leave it."""
    bits = np.zeros((ncells + 31) // 32, np.uint32)
    path = np.asarray(path, np.int64)
    np.bitwise_or.at(bits, path >> 5, (np.uint32(1) << (path & 31).astype(np.uint32)))
    return bits


def ref_walk(P, pos, cap=None):
    """backtrack() on a numpy matrix of any integer dtype, in place: DIAGONAL -> pos - m - 1, UP -> pos - m, else pos - 1; negate;
    stop when the next cell is NONE.  P[pos] == NONE gives the empty path.  Returns the FULL path whatever `cap` is: a capped path
    buffer holds its first min(cap, n) entries, and the caller slices."""
    m = P.shape[1]
    flat = P.reshape(-1)
    assert np.shares_memory(flat, P), "P must be contiguous: the walk negates in place"
    path = []
    pos = int(pos)
    if flat[pos] == NONE:
        return np.zeros(0, np.int64)
    while True:
        c = int(flat[pos])
        pred = pos - m - 1 if c == DIAGONAL else pos - m if c == UP else pos - 1
        flat[pos] = -c
        path.append(pos)
        pos = pred
        if flat[pos] == NONE:
            break
    return np.asarray(path, np.int64)


def make_case(rows1, m, start, plan, seed):
    """A (rows1, m) int8 matrix of uniformly random codes 0..3 with row 0 and column 0 NONE (the contract of a real P: the walk
    never leaves the matrix), the path written from `start` = (i, j) as (code, count) runs, clipped at row 1 / column 1 (a run that
    would step into row 0 or column 0 ends there, and so does the plan), and the cell after the last run set to NONE unless the
    plan ends with BORDER.  Returns (P, start position)."""
    rng = np.random.default_rng(seed)
    P = rng.integers(0, 4, (rows1, m), dtype=np.int8)
    P[0, :] = NONE
    P[:, 0] = NONE
    i, j = start
    assert 0 <= i < rows1 and 0 <= j < m
    pos = i * m + j
    if i == 0 or j == 0:
        return P, pos
    border = bool(plan) and plan[-1] == BORDER
    runs = plan[:-1] if border else plan
    clipped = False
    for code, count in runs:
        for _ in range(count):
            P[i, j] = code
            i -= code & 1
            j -= code >> 1
            if i == 0 or j == 0:
                clipped = True
                break
        if clipped:
            break
    if not clipped:
        assert not border, "a BORDER plan must reach row 0 or column 0"
        P[i, j] = NONE
    return P, pos


@dataclass(frozen=True)
class Case:
    name: str
    rows1: int
    m: int
    start: tuple
    plan: tuple
    seed: int

    def build(self, dtype=np.int8):
        P, pos = make_case(self.rows1, self.m, self.start, list(self.plan), self.seed)
        return np.ascontiguousarray(P.astype(dtype)), pos

    def __str__(self):
        return self.name


# ---- properties of a reference path, asserted by the families on the reference alone ---------------------------------------------------
def path_codes(P_after, path):
    return -P_after.reshape(-1)[path].astype(np.int64)


def longest_run(codes, code):
    best = cur = 0
    for c in codes:
        cur = cur + 1 if c == code else 0
        best = max(best, cur)
    return best


def windows_of(path, codes, m):
    """Replays the kernel's windowing on a reference path (codes: the code of every path cell): a window is anchored at the cursor
    (rows gi-63..gi, columns gj-63..gj, clamped at 0) and kept until the next cursor falls outside it.  One dict per window:
    clamp_top / clamp_left, ti / tj (the cursor inside the window), cells (path cells inside), exit ('end': the path stopped inside,
    'top', 'left-diag', 'left-left'), row / col (window coordinates of the cell the exit step was taken from) and, for
    'left-left', left_cells: the LEFT cells of that row inside the window."""
    out = []
    k, n = 0, len(path)
    while k < n:
        gi, gj = divmod(int(path[k]), m)
        r0, c0 = max(gi - (W - 1), 0), max(gj - (W - 1), 0)
        w = dict(clamp_top=gi < W - 1, clamp_left=gj < W - 1, ti=gi - r0, tj=gj - c0, cells=0, exit="end")
        while k < n and path[k] // m >= r0 and path[k] % m >= c0:
            w["cells"] += 1
            k += 1
        pi, pj = divmod(int(path[k - 1]), m)
        c = int(codes[k - 1])
        ni, nj = pi - (c & 1), pj - (c >> 1)
        w["row"], w["col"] = pi - r0, pj - c0
        if nj < c0:
            w["exit"] = "left-diag" if c == DIAGONAL else "left-left"
            if c == LEFT:
                q = k - 1
                while q >= 0 and codes[q] == LEFT and path[q] // m == pi and path[q] % m >= c0:
                    q -= 1
                w["left_cells"] = k - 1 - q
        elif ni < r0:
            w["exit"] = "top"
        out.append(w)
    return out


# ---- family 1: runs around the window size ----------------------------------------------------------------------------------------------
RUN_COUNTS = (1, 2, 62, 63, 64, 65, 127, 128, 129, 300)


def family_runs():
    cases = []
    for code, cname in ((UP, "up"), (LEFT, "left"), (DIAGONAL, "diag")):
        for n in RUN_COUNTS:
            dr, dc = (code & 1) * n, (code >> 1) * n
            seed = 1000 * code + n
            # (a) a few DIAGONAL steps, the run, a few DIAGONAL steps, NONE
            i, j = dr + 3 + 4 + 9, dc + 3 + 4 + 11
            cases.append(Case(f"run-{cname}{n}-mid", i + 7, j + 5, (i, j), ((DIAGONAL, 3), (code, n), (DIAGONAL, 4)), seed))
            # (b) the path ends (NONE) right after the run
            cases.append(Case(f"run-{cname}{n}-end", i + 7, j + 5, (i, j), ((DIAGONAL, 3), (code, n)), seed + 1))
            # (c) the run reaches row 1 / column 1 and steps into the border
            i, j = (dr if dr else 40) + 3, (dc if dc else 45) + 3
            cases.append(Case(f"run-{cname}{n}-border", i + 2, j + 3, (i, j), ((DIAGONAL, 3), (code, n), BORDER), seed + 2))
    return cases


# ---- family 2: every alignment of the start cell ---------------------------------------------------------------------------------------
def family_alignments():
    cases = []
    plan = ((DIAGONAL, 5), (LEFT, 3), (UP, 2), (DIAGONAL, 70), (UP, 66), (LEFT, 67), (DIAGONAL, 1000), BORDER)
    for bi in (0, 1, 2):         # i below 64 / above (i or j == 0: the start on the border, the empty path)
        for bj in (0, 1, 2):
            for ri in (0, 1, 62, 63):
                for rj in (0, 1, 62, 63):
                    i, j = bi * W + ri, bj * W + rj
                    cases.append(Case(f"align-i{i}-j{j}", 2 * W + 66, 2 * W + 69, (i, j), plan, 50000 + i * 1000 + j))
    return cases


# ---- family 3: edge exits ----------------------------------------------------------------------------------------------------------------
def family_edges():
    cases = []
    R, C = 400, 420
    si, sj = 300, 330          # first window: rows 237..300, columns 267..330
    # a LEFT run in row q of the window (reached by 63 - q DIAGONAL steps, so at window column q) that stops AT the window's
    # column 0 (over = -1: no exit, the path goes UP there), or crosses its left edge by exactly 0 cells (the exit step lands on
    # a cell that is not LEFT), 1 cell and 63 cells
    for q in (63, 40, 1, 0):
        for over in (-1, 0, 1, 63):
            n = q + 1 + over
            plan = ((DIAGONAL, 63 - q),) + (((LEFT, n),) if n else ()) + ((UP, 3), (DIAGONAL, 30))
            cases.append(Case(f"edge-left-row{q}-over{over}", R, C, (si, sj), plan, 60000 + q * 100 + over + 1))
    # a DIAGONAL step across the left edge from rows 63, 1 and 0 of the window
    for q in (63, 1, 0):
        u = 63 - q
        plan = ((LEFT, 63), (UP, u), (DIAGONAL, 5), (LEFT, 2), (DIAGONAL, 20)) if u else ((LEFT, 63), (DIAGONAL, 5), (LEFT, 2), (DIAGONAL, 20))
        cases.append(Case(f"edge-diag-row{q}", R, C, (si, sj), plan, 61000 + q))
    # UP across the top edge from columns 0 and 63 of the window
    cases.append(Case("edge-up-col63", R, C, (si, sj), ((UP, 70), (DIAGONAL, 3), (LEFT, 5)), 62000))
    cases.append(Case("edge-up-col0", R, C, (si, sj), ((LEFT, 63), (UP, 70), (DIAGONAL, 3), (LEFT, 5)), 62001))
    # staircases over several windows
    cases.append(Case("edge-stairs-1", R, C, (si, sj), ((LEFT, 1), (UP, 1)) * 280, 63000))
    cases.append(Case("edge-stairs-63", R, C, (250, 415), ((LEFT, 63), (UP, 1)) * 6 + ((DIAGONAL, 10),), 63001))
    cases.append(Case("edge-stairs-63-up63", 400, 420, (399, 419), ((LEFT, 63), (UP, 63)) * 5 + ((LEFT, 40),), 63002))
    return cases


# ---- family 4: small and odd shapes --------------------------------------------------------------------------------------------------
SHAPES = (2, 3, 5, 63, 64, 65, 66, 129, 130, 131, 517)


def family_shapes():
    cases = []
    for rows1 in SHAPES:
        for m in SHAPES:
            plan = ((DIAGONAL, 2), (LEFT, m // 3), (UP, rows1 // 3), (DIAGONAL, 7), (LEFT, 66), (UP, 67), (DIAGONAL, 1000), BORDER)
            cases.append(Case(f"shape-{rows1}x{m}", rows1, m, (rows1 - 1, m - 1), plan, 70000 + rows1 * 1000 + m))
    return cases


# ---- family 5: random plans ----------------------------------------------------------------------------------------------------------------
def family_random(n=240):
    cases = []
    for s in range(n):
        rng = np.random.default_rng(80000 + s)
        rows1, m = int(rng.integers(2, 701)), int(rng.integers(2, 901))
        i, j = int(rng.integers(1, rows1)), int(rng.integers(1, m))
        plan = []
        for _ in range(int(rng.integers(1, 40))):
            cls = int(rng.integers(0, 3))
            n_ = int(rng.integers(1, 5)) if cls == 0 else int(rng.integers(60, 71)) if cls == 1 else int(rng.integers(100, 401))
            plan.append((int(rng.integers(1, 4)), n_))
        cases.append(Case(f"rand-{s}-{rows1}x{m}", rows1, m, (i, j), tuple(plan), 90000 + s))
    return cases


# ---- family 6: path_cap ---------------------------------------------------------------------------------------------------------------
def family_caps():
    """Two paths (one with LEFT / UP runs through the row walk's flush, one that starts in the step walker); the caps are derived
    from the reference path's length in the tests: 1, 63, 64, 65, n - 1, n, n + 1."""
    return [Case("cap-runs", 300, 350, (299, 349), ((DIAGONAL, 10), (LEFT, 70), (UP, 66), (DIAGONAL, 20), (LEFT, 5), (UP, 3), (DIAGONAL, 80)), 95000),
            Case("cap-top", 80, 400, (50, 399), ((LEFT, 100), (DIAGONAL, 20), (LEFT, 130), (UP, 10), (DIAGONAL, 30), BORDER), 95001)]


def cap_values(n):
    return [1, 63, 64, 65, n - 1, n, n + 1]


SENTINEL = -0x5A5A5A5A5A5A5A5A


# ---- family 7: the read-ahead wave and big offsets ----------------------------------------------------------------------------------------
def big_plan(seed):
    """A mix of the runs of family 1, several thousand steps long, that runs far from the diagonal through its start (which the
    read-ahead wave expects): a LEFT-heavy half, then an UP-heavy half, each with a run of every length of RUN_COUNTS."""
    rng = np.random.default_rng(seed)
    short = (1, 2, 62, 63, 64, 65)
    plan = []
    for main, other in ((LEFT, UP), (UP, LEFT)):
        for n in rng.permutation(RUN_COUNTS):
            plan += [(main, int(n)), (DIAGONAL, int(rng.choice(short))), (main, int(rng.choice(RUN_COUNTS))), (other, int(rng.choice(short))),
                     (main, int(rng.choice(RUN_COUNTS)))]
    return tuple(plan)


def write_path(P, start, plan, background):
    """make_case's path writer on an existing matrix with a constant background: row 0 / column 0 NONE, the path from `start`,
    NONE after the last run unless it was clipped at the border."""
    P[...] = background
    P[0, :] = NONE
    P[:, 0] = NONE
    i, j = start
    for code, count in plan:
        for _ in range(count):
            P[i, j] = code
            i -= code & 1
            j -= code >> 1
            if i == 0 or j == 0:
                return
    P[i, j] = NONE


def ref_walk_sparse(P, pos):
    """ref_walk without the in-place negation (family 7 keeps one host copy): returns (path, codes)."""
    m = P.shape[1]
    flat = P.reshape(-1)
    path, codes = [], []
    pos = int(pos)
    if flat[pos] == NONE:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    while True:
        c = int(flat[pos])
        path.append(pos)
        codes.append(c)
        pos = pos - m - 1 if c == DIAGONAL else pos - m if c == UP else pos - 1
        if flat[pos] == NONE:
            break
    return np.asarray(path, np.int64), np.asarray(codes, np.int64)


# ---- what each family exists for, asserted on the reference path alone ----------------------------------------------------------------
def check_property(case, P_after, path):
    """Fails if `case` has quietly stopped exercising what its family is for.  P_after: the reference matrix after ref_walk."""
    m = case.m
    codes = path_codes(P_after, path)
    wins = windows_of(path, codes, m)
    fam, _, rest = case.name.partition("-")
    if fam == "run":
        kind, where = rest.split("-")
        cname = kind.rstrip("0123456789")
        n, code = int(kind[len(cname):]), {"up": UP, "left": LEFT, "diag": DIAGONAL}[cname]
        # (a DIAGONAL run merges with the DIAGONAL steps before and after it)
        assert longest_run(codes, code) == n + (0 if code != DIAGONAL else 7 if where == "mid" else 3)
        assert codes[0] == DIAGONAL and len(path) == 3 + n + (4 if where == "mid" else 0)
        if where == "end":
            assert codes[-1] == code
        if where == "border":
            li, lj = divmod(int(path[-1]), m)
            assert codes[-1] == code and (li == 1 if code & 1 else True) and (lj == 1 if code >> 1 else True)
    elif fam == "align":
        i, j = case.start
        if i == 0 or j == 0:
            assert len(path) == 0
        else:
            w = wins[0]
            assert (w["clamp_top"], w["clamp_left"]) == (i < W - 1, j < W - 1) and (w["ti"], w["tj"]) == (min(i, W - 1), min(j, W - 1))
            assert divmod(int(path[0]), m) == (i, j)
    elif fam == "edge":
        w = wins[0]
        if rest.startswith("left-row"):
            q, over = int(rest[8:rest.index("-over")]), int(rest[rest.index("-over") + 5:])
            assert longest_run(codes, LEFT) == q + 1 + over
            if over < 0:         # the run stops AT the window's column 0 and the path goes UP there: no exit by a LEFT step
                assert w["exit"] in ("top", "left-diag") and w["col"] == 0 and w["cells"] == 64 + min(q, 3)
            else:
                assert w["exit"] == "left-left" and w["row"] == q and w["left_cells"] == q + 1 and w["cells"] == 64
        elif rest.startswith("diag-row"):
            q = int(rest[8:])
            assert w["exit"] == "left-diag" and w["row"] == q and w["col"] == 0
        elif rest.startswith("up-col"):
            assert w["exit"] == "top" and w["row"] == 0 and w["col"] == int(rest[6:]) and longest_run(codes, UP) == 70
        else:
            assert len(wins) >= 5 and longest_run(codes, LEFT) == (1 if rest == "stairs-1" else 63)
            if rest != "stairs-1":
                assert sum(x["exit"] == "left-left" for x in wins) >= 3
    elif fam == "shape":
        assert len(path) >= 1 and int(path[0]) == case.rows1 * m - 1
        li, lj = divmod(int(path[-1]), m)
        assert li == 1 or lj == 1, "the plan runs into the border"
    elif fam == "cap":
        assert len(path) > 130
    return wins, codes
