"""The score-range case table: fills, batches and searches whose scores sit on both sides of every line at which the library changes
its arithmetic (plain data and small helpers; nothing here touches a GPU).  tests/test_score_range_host.py checks the table on a CPU;
tests/test_score_range_gpu.py runs it: every output of every case bit for bit against the oracle, then the route ("last_perm",
"last_strips2", "last_batch_kernel", "last_search_kernel").

The lines, with the constants quoted BY NAME from smith-waterman_amd/csrc/sw_plan.cpp (plan_fill, plan_batch, plan_search) and from
check_dims in sw_ctx.h.  The sizes of the cases are computed from these copies; test_score_range_host.py holds every case's expected
route against what the planners decide, so a constant that moves in sw_plan.cpp makes a route assertion fail instead of moving a
case off its edge unnoticed."""
import zlib
from dataclasses import dataclass, field

import numpy as np

# plan_fill: f.perm
kPermByte = 127                 # match - 2 gap and mismatch - 2 gap in -127 .. 127 (the perm producer's signed-byte profile)
kTagBit = 1 << 24               # G values share a word with the 8-bit launch tag in the top byte
kGBias = 0x10000                # the bias every G value carries
kPermSlack = 1024               # gmax + kGBias + kPermSlack < kTagBit
kScoutStrips = 170              # more 126-column strips than this: the library's own choice is overlapping strips every 110 columns
S2_W, S2_OV = 126, 110          # columns a strip of the two-column kernel computes; distance of overlapping strips
# plan_batch / plan_search
kWaveScore = 127                # match, mismatch in -127 .. 127: the signed-byte profiles of sw_batch_wave / sw_search_wave
kWave16Score, kWave16Rows = 32000, 65000   # packed 16-bit lanes: match * min(cols, rows) and -gap below 32000, fewer than 65000 rows
kKeyedScore = 4096              # keyed arg-max
kC4Cols, kC8Cols = 256, 512     # columns per lane: 4 up to 256 columns, 8 up to 512, 16 beyond
# check_dims
kScoreBits, kCellBits = 1 << 24, 1 << 31   # match * min(cols, rows) and the per-step constant below 2^24; gmax + step below 2^31

DNA = np.frombuffer(b"ACGT", np.uint8)
BATCH_FALLBACK, BATCH_WAVE, BATCH_WAVE16 = 0, 1, 2   # sw_get_option "last_batch_kernel"


def gmax_of(cols, rows, scores, total_rows=0):
    """plan_fill's bound of every G value (H - gap (row + col)) of a fill; total_rows: a band's whole matrix"""
    match, _, gap = scores
    return match * max(min(cols, rows), min(cols, total_rows)) + (-gap) * (rows + cols + 2)


def perm_ok(cols, rows, scores, total_rows=0):
    match, mismatch, gap = scores
    mm, xm = match - 2 * gap, mismatch - 2 * gap
    return -kPermByte <= mm <= kPermByte and -kPermByte <= xm <= kPermByte and gmax_of(cols, rows, scores, total_rows) + kGBias + kPermSlack < kTagBit


def widest_perm_cols(rows, scores, total_rows=0):
    """the largest cols (> rows) at which perm_ok holds"""
    match, _, gap = scores
    cols = (kTagBit - kGBias - kPermSlack - 1 - match * max(rows, total_rows)) // (-gap) - rows - 2
    assert cols > max(rows, total_rows) and perm_ok(cols, rows, scores, total_rows) and not perm_ok(cols + 1, rows, scores, total_rows)
    return cols


def dims_ok(cols, rows, scores):
    """check_dims (sw_ctx.h) for a whole matrix"""
    match, mismatch, gap = scores
    if gap > 0 or match < 0 or mismatch > match:
        return False
    lo = min(cols, rows)
    gmax = match * lo + (-gap) * (rows + cols + 2)
    step = max(abs(mismatch), match) + 2 * (-gap)
    return gmax + step < kCellBits and step < kScoreBits and match * lo < kScoreBits


def last_strip_cols(cols, w2):
    """columns that only the last strip of the two-column kernel computes (column tiles own whole multiples of the strip distance)"""
    if cols <= S2_W:
        return cols
    return (cols - 1) % S2_W + 1 if w2 == S2_W else (cols - S2_W - 1) % S2_OV + 1


def auto_strip_distance(cols):
    """the strip distance the library itself picks for a whole int32 H + P matrix in aligned buffers -- plan_fill:
    `S126 = cols <= 126 ? 1 : (cols - 126 + 125) / 126 + 1` and `W2 = 110` where `S126 > kScoutStrips` (wl_fmt holds, option s2w = 0)"""
    s126 = 1 if cols <= S2_W else (cols - S2_W + S2_W - 1) // S2_W + 1
    return S2_OV if s126 > kScoutStrips else S2_W


def lane_columns(cols):
    return 4 if cols <= kC4Cols else 8 if cols <= kC8Cols else 16


def seed_of(name):
    return zlib.crc32(name.encode())


def make_pair(recipe, cols, rows, seed):
    """(a, b) as uint8 arrays.  corner: b is the tail of a with ~2 % substitutions -- the diagonal ends in the bottom-right cell, so H
    climbs to nearly match * rows exactly where -gap (row + col) is largest; allmatch: one letter; periodic: ACGT repeated."""
    rng = np.random.default_rng(seed)
    if recipe == "allmatch":
        return np.full(cols, 65, np.uint8), np.full(rows, 65, np.uint8)
    if recipe == "periodic":
        return np.resize(DNA, cols).copy(), np.resize(DNA, rows).copy()
    a = DNA[rng.integers(0, 4, cols)]
    if recipe == "random":
        return a, DNA[rng.integers(0, 4, rows)]
    assert recipe == "corner"
    b = a[-rows:].copy() if rows <= cols else np.concatenate([DNA[rng.integers(0, 4, rows - cols)], a])
    sub = rng.random(rows) < 0.02
    b[sub] = DNA[rng.integers(0, 4, int(sub.sum()))]
    return a, b


@dataclass
class FillCase:
    name: str
    group: str                       # "A", "B", "C"
    cols: int
    rows: int
    scores: tuple
    recipe: str
    fmt: str = "h32p32"              # h32p32, h32p8, h64p32, none (score-only)
    options: dict = field(default_factory=dict)   # sw_set_option values for the fill (s2w, engine)
    inside: bool = True              # inside the line this case sits at
    perm: bool = True                # expected FillPlan::perm ("last_perm")
    two_cols: bool = True            # expected FillPlan::two_cols ("last_strips2" > 0)
    last_cols: int = 0               # expected columns of the last strip (0: not asserted)
    w2: int = 0                      # expected strip distance (0: not asserted)
    streamed: bool = False           # too big for whole matrices on the host: row checksums, bottom row, arg-max
    valid: bool = True               # check_dims accepts it (False: the call must return -22 and write nothing)

    def pair(self):
        return make_pair(self.recipe, self.cols, self.rows, seed_of(self.name))

    def plan_kw(self):
        """the fields of the planner driver's fill job"""
        hb, pb = {"h32p32": (4, 4), "h32p8": (4, 1), "h64p32": (8, 4), "none": (4, 4)}[self.fmt]
        kw = {"cols": self.cols, "rows": self.rows, "match": self.scores[0], "mismatch": self.scores[1], "gap": self.scores[2],
              "h_elem_bytes": hb, "p_elem_bytes": pb}
        if self.fmt == "none":
            kw.update(has_H=0, has_P=0)
        kw.update(self.options)
        return kw


# ---- A: the signed-byte corners of the perm producer
A_SHAPES = [(1007, 304), (2520, 333), (126, 16)]
A_INSIDE = [(127, -127, 0), (1, -1, -63), (125, -129, -1), (0, -127, 0), (127, 127, 0)]
A_OUTSIDE = [(128, -127, 0), (127, -128, 0), (1, -1, -64)]
A_RECIPES = ["random", "corner", "allmatch"]

# ---- B: the 24-bit tag boundary
B_SCORES = (1, -1, -63)
B_ROWS = [16, 17, 31, 144]
B_LAST_126, B_LAST_110 = [126, 125, 63, 2, 1], [109, 1]
B_STREAM_SCORES, B_STREAM_ROWS = (25, -25, -51), 1296
B_BAND_TOTAL_ROWS, B_BAND_CUTS = 144, (48, 96)


def _sc(scores):
    return "m%d_x%d_g%d" % scores


def _widest_with(wmax, w2, last):
    w = wmax
    while last_strip_cols(w, w2) != last:
        w -= 1
    assert wmax - w <= 125
    return w


def gap_limit(cols, rows, match):
    """the most negative gap check_dims accepts with scores (match, -match, gap) on cols x rows"""
    gap = -(kCellBits // (rows + cols + 4))
    while dims_ok(cols, rows, (match, -match, gap - 1)):
        gap -= 1
    while not dims_ok(cols, rows, (match, -match, gap)):
        gap += 1
    return gap


def fill_cases():
    out = []
    for cols, rows in A_SHAPES:
        for sc in A_INSIDE:
            assert perm_ok(cols, rows, sc)
            for recipe in A_RECIPES:
                out.append(FillCase(f"A-{cols}x{rows}-{_sc(sc)}-{recipe}", "A", cols, rows, sc, recipe))
            # an odd width with an int8 P (an even one at 126 and 2520 columns): the one-column kernel, whose producer only "last_perm" shows
            out.append(FillCase(f"A-{cols}x{rows}-{_sc(sc)}-corner-p8", "A", cols, rows, sc, "corner", fmt="h32p8", two_cols=cols % 2 == 0))
        for sc in A_OUTSIDE:
            assert not perm_ok(cols, rows, sc)
            for recipe in A_RECIPES[:2]:
                out.append(FillCase(f"A-{cols}x{rows}-{_sc(sc)}-{recipe}", "A", cols, rows, sc, recipe, inside=False, perm=False, two_cols=False))
    for rows in B_ROWS:
        wmax = widest_perm_cols(rows, B_SCORES)
        auto = auto_strip_distance(wmax)
        for recipe in ("corner", "random"):
            out.append(FillCase(f"B-{rows}r-widest-{recipe}", "B", wmax, rows, B_SCORES, recipe, w2=auto, last_cols=last_strip_cols(wmax, auto)))
            for last in B_LAST_126:
                w = _widest_with(wmax, S2_W, last)
                out.append(FillCase(f"B-{rows}r-s126-last{last}-{recipe}", "B", w, rows, B_SCORES, recipe, options={"s2w": S2_W}, w2=S2_W, last_cols=last))
            for last in B_LAST_110:
                w = _widest_with(wmax, S2_OV, last)
                out.append(FillCase(f"B-{rows}r-s110-last{last}-{recipe}", "B", w, rows, B_SCORES, recipe, options={"s2w": S2_OV}, w2=S2_OV, last_cols=last))
            out.append(FillCase(f"B-{rows}r-beyond-{recipe}", "B", wmax + 1, rows, B_SCORES, recipe, inside=False, perm=False, two_cols=False))
        even = wmax - wmax % 2
        for fmt in ("h32p8", "h64p32", "none"):
            out.append(FillCase(f"B-{rows}r-even-{fmt}", "B", even, rows, B_SCORES, "corner", fmt=fmt))
    wmax = widest_perm_cols(B_STREAM_ROWS, B_STREAM_SCORES)
    out.append(FillCase("B-streamed", "B", wmax, B_STREAM_ROWS, B_STREAM_SCORES, "corner", w2=S2_OV, last_cols=last_strip_cols(wmax, S2_OV), streamed=True))
    # ---- C: the outer limits of check_dims (none of them perm: the character-compare producer, sw_strip_scan, sw_fill_host)
    m1000 = (kScoreBits - 1) // 1000
    g1100 = gap_limit(1000, 1100, 3)
    c_inside = [("16e6", 1000, 1048, (16000, -16000, -8000), "allmatch"), ("score24", 1000, 1000, (m1000, -m1000, -2), "allmatch"),
                ("gap31-random", 1000, 1100, (3, -3, -1000000), "random"), ("gap31-corner", 1000, 1100, (3, -3, -1000000), "corner"),
                ("gap31-last-random", 1000, 1100, (3, -3, g1100), "random"), ("gap31-last-corner", 1000, 1100, (3, -3, g1100), "corner"),
                ("2cols", 2, 2000, (8000000, -8000000, -100), "allmatch"), ("2cols-last", 2, 2000, (kScoreBits // 2 - 1, -8000000, -100), "allmatch"),
                ("step24", 100, 100, (3, -3, -(kScoreBits // 2 - 2)), "corner")]
    c_outside = [("score24", 1000, 1000, (m1000 + 1, -m1000, -2), "allmatch"), ("16e6", 1000, 1048, (m1000 + 1, -16000, -8000), "allmatch"),
                 ("gap31", 1000, 1100, (3, -3, g1100 - 1), "random"), ("2cols", 2, 2000, (kScoreBits // 2, -8000000, -100), "allmatch"),
                 ("step24", 100, 100, (3, -3, -(kScoreBits // 2 - 1)), "corner")]
    for name, cols, rows, sc, recipe in c_inside:
        assert dims_ok(cols, rows, sc) and not perm_ok(cols, rows, sc), name
        for fmt in ("h32p32", "h64p32"):
            for eng in (0, 1):
                out.append(FillCase(f"C-{name}-{fmt}-engine{eng}", "C", cols, rows, sc, recipe, fmt=fmt, options={"engine": eng}, perm=False, two_cols=False))
    for name, cols, rows, sc, recipe in c_outside:
        assert not dims_ok(cols, rows, sc), name
        for eng in (0, 1):
            out.append(FillCase(f"C-{name}-rejected-engine{eng}", "C", cols, rows, sc, recipe, options={"engine": eng}, inside=False, perm=False,
                                two_cols=False, valid=False))
    assert len({c.name for c in out}) == len(out)
    return out


def band_case():
    """(cols, total rows, cuts, scores): stacked bands of a corner input, every band as wide as the perm producer takes it"""
    rows = B_BAND_CUTS[0]
    assert all(b - a == rows for a, b in zip((0,) + B_BAND_CUTS, B_BAND_CUTS + (B_BAND_TOTAL_ROWS,)))
    cols = widest_perm_cols(rows, B_SCORES, B_BAND_TOTAL_ROWS)
    return cols - cols % 2, B_BAND_TOTAL_ROWS, B_BAND_CUTS, B_SCORES


# ---- D: the batch kernels
@dataclass
class BatchCase:
    name: str
    cols: int
    rows: int
    scores: tuple
    recipes: tuple                   # one per pair
    mode: str                        # "hp" (int32 H + P), "p8" (int8 P alone), "score"
    wave: bool                       # expected BatchPlan::wave
    kernel: int                      # expected "last_batch_kernel"
    score_line: bool = False         # a packed case placed at the score line: the oracle's best score must reach 31 800

    @property
    def npairs(self):
        return len(self.recipes)

    def pairs(self):
        ab = [make_pair(r, self.cols, self.rows, seed_of(self.name) + k) for k, r in enumerate(self.recipes)]
        return np.stack([a for a, _ in ab]), np.stack([b for _, b in ab])

    def plan_kw(self):
        kw = {"cols": self.cols, "rows": self.rows, "npairs": self.npairs, "match": self.scores[0], "mismatch": self.scores[1], "gap": self.scores[2],
              "has_H": int(self.mode == "hp"), "has_P": int(self.mode != "score"), "p_elem_bytes": 1 if self.mode == "p8" else 4}
        # (two pairs of driver fields that must agree: plan_batch reads npairs and has_P / p_elem_bytes, batch_kernel the pairs of the
        #  chunk n and the bytes of a P element pb, 0 without P)
        kw["pb"] = {"hp": 4, "p8": 1, "score": 0}[self.mode]
        kw["n"] = self.npairs
        return kw


def batch_route(cols, rows, npairs, scores, mode):
    """(wave, last_batch_kernel) from the lines of plan_batch"""
    match, mismatch, gap = scores
    wave = -kWaveScore <= match <= kWaveScore and -kWaveScore <= mismatch <= kWaveScore
    fits16 = npairs >= 2 and lane_columns(cols) == 16 and match * min(cols, rows) < kWave16Score and -gap < kWave16Score and rows < kWave16Rows
    return wave, (BATCH_WAVE16 if fits16 and mode != "hp" else BATCH_WAVE) if wave else BATCH_FALLBACK


MIXED = ("random", "corner", "allmatch", "periodic", "random")   # an odd number of pairs: the last one runs in both halves of a wave


def batch_cases():
    out = []

    def add(name, cols, rows, sc, recipes, modes, score_line=False):
        assert dims_ok(cols, rows, sc), name
        for mode in modes:
            wave, kernel = batch_route(cols, rows, len(recipes), sc, mode)
            out.append(BatchCase(f"D-{name}-{cols}x{rows}-{_sc(sc)}-{mode}", cols, rows, sc, tuple(recipes), mode, wave, kernel, score_line))
    for sc in [(127, -127, -2), (127, 127, 0), (0, -127, -1), (5, -3, -1000000)]:
        for cols, rows in [(200, 90), (400, 110), (700, 100), (1500, 130), (2049, 40)]:   # 4, 8, 16 columns per lane; two and three strips (check_dims takes a gap of -1000000 up to rows + cols of 2140)
            add("wave", cols, rows, sc, MIXED, ("hp", "p8", "score"))
    for sc in [(128, -3, -2), (3, -128, -2)]:
        add("fallback", 300, 120, sc, MIXED, ("hp", "score"))
    # packed lanes: the score line, the gap line; mismatch = -127 beside a score of 31 900
    line = ("allmatch", "random", "allmatch", "corner", "allmatch")
    for name, cols, rows, sc in [("score16", 600, 319, (100, -100, -2)), ("score16", 600, 320, (100, -100, -2)),
                                 ("score16", 600, 251, (127, -127, -3)), ("score16", 600, 252, (127, -127, -3)),
                                 ("borrow16", 600, 319, (100, -127, -1))]:
        add(name, cols, rows, sc, line, ("score", "p8"), score_line=True)
    for gap in (-(kWave16Score - 1), -kWave16Score):
        add("gap16", 600, 100, (3, -3, gap), MIXED, ("score", "p8"))
    assert len({c.name for c in out}) == len(out)
    return out


# ---- E: search
SEARCH_QLENS = [200, 400, 513, 1100, 2100]   # 4, 8, 16 columns per lane; two and three strips
SEARCH_SCORES = [(127, -127, -1), (128, -127, -1), (127, -128, -1), (255, -255, -3), (256, -1, -2), (5, -1, -2), (0, -5, -1)]
SEARCH_FIXED_LENS = [0, 1, 63, 64, 65]


@dataclass
class SearchCase:
    name: str
    qlen: int
    scores: tuple                    # None: the near-2^24 recipe, scores from the longest target
    wide: bool
    C: int
    long_target: int = 0             # one target of this many letters among 2000 short ones

    def data(self):
        """(query, packed targets, offsets)"""
        rng = np.random.default_rng(seed_of(self.name))
        query = DNA[rng.integers(0, 4, self.qlen)]
        if self.long_target:
            lens = list(rng.integers(1, 100, 2000))
            lens.insert(777, self.long_target)
        else:
            lens = SEARCH_FIXED_LENS + list(rng.integers(2, 3001, 10)) + [0]
        seqs = [DNA[rng.integers(0, 4, int(n))] for n in lens]
        if not self.long_target:   # one target holds a slice of the query, so that scores climb
            seqs[7] = np.concatenate([seqs[7][:50], query[self.qlen // 4:], seqs[7][50:]])
        offs = np.zeros(len(seqs) + 1, np.int64)
        offs[0] = 7
        offs[1:] = 7 + np.cumsum([len(s) for s in seqs])
        packed = np.concatenate([DNA[rng.integers(0, 4, 7)]] + seqs).astype(np.uint8)
        return query, packed, offs

    def scores_for(self, offs):
        if self.scores is not None:
            return self.scores
        match = kScoreBits // min(self.qlen, int(np.diff(offs).max())) - 1   # match * min(cols, rows) just below 2^24
        return (match, -match // 3, -match // 5)

    @property
    def kernel(self):
        return 2 * (self.C // 8) + int(self.wide)


def search_cases():
    out = []
    for qlen in SEARCH_QLENS:
        for sc in SEARCH_SCORES:
            out.append(SearchCase(f"E-{qlen}-{_sc(sc)}", qlen, sc, sc[0] > kWaveScore or sc[1] < -kWaveScore, lane_columns(qlen)))
    out.append(SearchCase("E-400-near24", 400, None, True, lane_columns(400)))
    out.append(SearchCase("E-1100-long-target", 1100, (127, -127, -1), False, 16, long_target=300000))
    out.append(SearchCase("E-1100-long-target-wide", 1100, (128, -127, -1), True, 16, long_target=300000))
    return out
