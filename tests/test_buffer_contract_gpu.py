"""GPU: every entry point's BUFFER contract (include/swhip.h) -- where the kernels write and on what memory state they depend.  Every
output is a view into a poisoned arena (tests/buffer_cases.py) at a chosen address skew with 256 KiB guards on both sides, every input
sits at an odd address (b at a multiple of 16, as the header asks) between live-letter padding, and after each call
  * the payload equals the oracle / the checker bit for bit, row 0 and column 0 included (left-over poison fails here),
  * assert_guards finds every byte outside the outputs unchanged, the inputs and their padding included,
  * the kernel or geometry that ran is the one the case was built for (sw_get_option "last_*").
The padding tests prove that results do not depend on the bytes around the inputs; they cannot prove that those bytes are never read."""
import numpy as np
import pytest

from affine_cases import DNA, PROTEIN, checker, random_submat  # noqa: F401
from align_cases import expected, pack
import pssm_hits_cases as hc
import pssm_weights_cases as wc
from buffer_cases import POISON, POISON8, POISON32, POISON64, Arena, arena_bytes, assert_guards, live_head, live_tail

pytestmark = pytest.mark.gpu

NO_TWO_COLUMNS = 16384


def _dev(engine):
    return f"cuda:{engine.device}"


def _out(ar, shape, dtype, skew, name, align=256):
    n = int(np.prod(shape)) * ar.buf.new_empty(0, dtype=dtype).element_size()
    c = ar.carve(n, align, skew, name=name)
    return ar.view(c, dtype, tuple(shape)), c


def _inp(ar, seq, align, skew, name, front=None, back=None):
    seq = np.ascontiguousarray(seq, np.uint8).reshape(-1)
    t, _ = ar.place(seq, align, skew, front=live_head(seq, 64) if front is None else front, back=live_tail(seq, 64) if back is None else back, name=name)
    return t


def _result(ar, n=1, name="result"):
    """n sw_result at an address with % 16 == 8"""
    t, _ = _out(ar, (n, 3) if n > 1 else (3,), ar.torch.int64, 8, name, align=16)
    return t


# ---- fill (sw_fill_device_ex) ---------------------------------------------------------------------------------------------------------
def _formats(torch):
    return {"hp32": (torch.int32, torch.int32), "h64": (torch.int64, torch.int32), "p8": (torch.int32, torch.int8), "h_only": (torch.int32, None),
            "p_only": (None, torch.int32), "p8_only": (None, torch.int8), "score_only": (None, None)}


ALL_FORMATS = ("hp32", "h64", "p8", "h_only", "p_only", "p8_only", "score_only")


def _skews(fmt):
    """(H, P) base skews: 4 for int32, 8 for an int64 H (the planner tests & 15), 1, 3, 4, 7 for an int8 P"""
    hs = {"hp32": (0, 4), "h64": (0, 8), "p8": (0, 4), "h_only": (0, 4)}.get(fmt, (0,))
    ps = {"hp32": (0, 4), "h64": (0, 4), "p_only": (0, 4), "p8": (0, 1, 3, 4, 7), "p8_only": (0, 1, 3, 4, 7)}.get(fmt, (0,))
    if fmt == "p8":
        return [(0, 0), (4, 0), (0, 1), (4, 3), (0, 4), (4, 7), (0, 7), (4, 1)]
    return [(h, p) for h in hs for p in ps]


def _strips(cols, w):
    return 1 if cols <= 126 else -(-(cols - 126) // w) + 1


def _two_columns(cols, fmt):
    """the two-column kernel takes an odd width only with int32 H + int32 P (sw_plan.cpp)"""
    return fmt == "hp32" or cols % 2 == 0


def _run_fills(engine, swamd, oracle, a, b, formats, check_kernel, what):
    torch = engine.torch
    cols, rows = len(a), len(b)
    H, P, mp = oracle.fill(a, b)
    score = int(H.flat[mp])
    cells = (rows + 1) * (cols + 1)
    inp = Arena(torch, _dev(engine), arena_bytes(cols + 128, rows + 128))
    d_a = _inp(inp, a, 64, 3, "a")                  # an odd address
    d_b = _inp(inp, b, 256, 48, "b")                # 16-byte aligned, as the header asks, and no more than that
    out = Arena(torch, _dev(engine), arena_bytes(cells * 8, cells * 4, 24))
    fm = _formats(torch)
    for fmt in formats:
        hd, pd = fm[fmt]
        for hs, ps in _skews(fmt):
            out.reset()
            Ht = _out(out, (rows + 1, cols + 1), hd, hs, "H")[0] if hd is not None else None
            Pt = _out(out, (rows + 1, cols + 1), pd, ps, "P")[0] if pd is not None else None
            res = _result(out)
            case = f"{what} {cols}x{rows} {fmt}, H base % 256 = {hs}, P base % 256 = {ps}"
            engine.fill_into(swamd.Fill(Ht, Pt, res, cols, rows), d_a, d_b)
            engine.synchronize()
            assert res.cpu().tolist() == [mp, score, 0], case
            if Ht is not None:
                assert np.array_equal(Ht.cpu().numpy().astype(np.int64), H.astype(np.int64)), case + ": H"
            if Pt is not None:
                assert np.array_equal(Pt.cpu().numpy().astype(np.int32), P), case + ": P"
            assert_guards(out)
            assert_guards(inp)
            check_kernel(fmt, hs, ps, case)


@pytest.mark.parametrize("cols,rows", [(1, 16), (127, 40), (253, 80), (1007, 304)])
def test_fill_two_columns_126(engine, swamd, oracle, cols, rows):
    """the default kernel family: strips every 126 columns; the last shape is an odd width with a ragged last block"""
    a, b = oracle.generate(cols, rows, 900 + cols)

    def kernel(fmt, hs, ps, case):
        assert engine.get_option("last_strips2") == (_strips(cols, 126) if _two_columns(cols, fmt) else 0), case

    _run_fills(engine, swamd, oracle, a, b, ALL_FORMATS, kernel, "two columns")


@pytest.mark.parametrize("cols,rows", [(2, 16), (236, 33), (346, 17), (1001, 1000)])
def test_fill_overlapping_strips_whole_lines(engine, swamd, oracle, cols, rows):
    """option s2w = 110: whole 64-byte lines from overlapping strips; an odd width stores every row shifted.  Bases that are not 8-byte
    (16-byte: int64 H) aligned cannot take whole lines: an even width keeps the 110-column strips with pair stores, an odd one falls
    back to 126 (tests/test_fill_plan.py: test_strip_width)."""
    a, b = oracle.generate(cols, rows, 910 + cols)

    def kernel(fmt, hs, ps, case):
        aligned = hs % (16 if fmt == "h64" else 8) == 0 and ps % 8 == 0
        if not _two_columns(cols, fmt):
            want = 0
        elif cols % 2 == 0:
            want = _strips(cols, 110)
        else:
            want = _strips(cols, 110 if aligned else 126)
        assert engine.get_option("last_strips2") == want, case

    engine.set_option("s2w", 110)
    try:
        _run_fills(engine, swamd, oracle, a, b, ALL_FORMATS, kernel, "overlapping strips")
    finally:
        engine.set_option("s2w", 0)


def test_fill_one_column_kernel_by_alphabet(engine, swamd, oracle):
    """8 letters: the two-column launch leaves at once and the one-column kernel behind it fills, row 0 / column 0 included"""
    rng = np.random.default_rng(5)
    a = rng.choice(np.frombuffer(b"ABCDEFGH", np.uint8), size=640).astype(np.uint8)
    b = rng.choice(np.frombuffer(b"ABCDEFGH", np.uint8), size=160).astype(np.uint8)
    assert len(set(a.tolist()) | set(b.tolist())) == 8

    def kernel(fmt, hs, ps, case):
        assert engine.get_option("last_strips2") == _strips(640, 126) and engine.get_option("last_strips") == -(-640 // 63), case

    _run_fills(engine, swamd, oracle, a, b, ALL_FORMATS, kernel, "one column (8 letters)")


def test_fill_one_column_kernel_forced(engine, swamd, oracle):
    a, b = oracle.generate(1007, 304, 921)

    def kernel(fmt, hs, ps, case):
        assert engine.get_option("last_strips2") == 0 and engine.get_option("last_strips") == -(-1007 // 63), case

    engine.set_option("debug_flags", NO_TWO_COLUMNS)
    try:
        _run_fills(engine, swamd, oracle, a, b, ALL_FORMATS, kernel, "one column (forced)")
    finally:
        engine.set_option("debug_flags", 0)


def test_fill_second_engine(engine, swamd, oracle):
    a, b = oracle.generate(300, 200, 922)

    def kernel(fmt, hs, ps, case):
        assert engine.get_option("engine") == 1 and engine.get_option("last_grid") >= 1, case

    engine.set_option("engine", 1)
    try:
        _run_fills(engine, swamd, oracle, a, b, ("hp32",), kernel, "strip_scan")
    finally:
        engine.set_option("engine", 0)


def test_fill_split_strips(engine, swamd, oracle):
    """forced split strips (the scouts write the lower blocks); needs the roles dealt per XCD, and runs unsplit elsewhere"""
    a, b = oracle.generate(6600, 400, 923)
    want = 1 if engine.get_option("xcd_round_robin") else 0

    def kernel(fmt, hs, ps, case):
        assert engine.get_option("last_strips2") == _strips(6600, 126) and engine.get_option("last_split_from") == want, case

    engine.set_option("s2w", 126); engine.set_option("split_blk", 7); engine.set_option("split_from", 1)
    try:
        _run_fills(engine, swamd, oracle, a, b, ALL_FORMATS, kernel, "split strips")
    finally:
        engine.set_option("split_blk", 0); engine.set_option("split_from", 0); engine.set_option("s2w", 0)


def test_fill_column_tiles(engine, swamd, oracle):
    """171 strips of 126 columns, the smallest width that is cut into column tiles (int32 H + P only): a tile's left halo is read from H
    itself, so a tile must not touch the column its neighbour wrote"""
    cols, rows = 21421, 48
    a, b = oracle.generate(cols, rows, 924)

    def kernel(fmt, hs, ps, case):
        assert engine.get_option("last_tiles") >= 2 and engine.get_option("last_scouts") > 0, case

    engine.set_option("s2w", 126)
    try:
        _run_fills(engine, swamd, oracle, a, b, ("hp32",), kernel, "column tiles")
    finally:
        engine.set_option("s2w", 0)


@pytest.mark.parametrize("cols,rows", [(504, 64), (2016, 64)])
def test_fill_behind_scouts(engine, swamd, oracle, cols, rows):
    """4 strips: the fewest that get scout workgroups; 16 strips: the fewest whose roles are dealt per XCD (tests/test_xcd_roles_gpu.py)"""
    a, b = oracle.generate(cols, rows, 925)

    def kernel(fmt, hs, ps, case):
        assert engine.get_option("last_strips2") == cols // 126 and engine.get_option("last_scouts") > 0, case
        if cols == 2016 and engine.get_option("xcd_round_robin"):
            assert engine.get_option("last_xcd_mode") == 1, case

    _run_fills(engine, swamd, oracle, a, b, ALL_FORMATS, kernel, "scouts")


# ---- tiles and bands ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("halo", [True, False], ids=["halo", "no_halo"])
@pytest.mark.parametrize("tcols,trows", [(130, 48), (257, 33)])
def test_one_interior_tile(engine, oracle, tcols, trows, halo):
    """One interior tile of a 6 x 5-block matrix, filled alone into poison with row_stride > cols + 1: every cell outside the tile's
    rectangle stays poison; its row 0 / column 0 stay poison when d_top / d_left say a neighbour owns them and are zero when not, in H
    and in P; d_right is the tile's last column."""
    torch = engine.torch
    cols, rows = 6 * tcols, 5 * 48
    i0, j0 = 2 * 48, 2 * tcols
    a, b = oracle.generate(cols, rows, 930 + tcols)
    if halo:
        H, P, _ = oracle.fill(a, b)
        eH, eP = H[i0:i0 + trows + 1, j0:j0 + tcols + 1], P[i0:i0 + trows + 1, j0:j0 + tcols + 1]
    else:
        eH, eP, _ = oracle.fill(a[j0:j0 + tcols], b[i0:i0 + trows])
    inp = Arena(torch, _dev(engine), arena_bytes(cols + 128, rows + 128, 4 * tcols + 4, 4 * trows + 4))
    d_a = _inp(inp, a, 64, 1, "a")
    d_b = _inp(inp, b, 256, 16, "b")
    top = left = None
    if halo:
        top = _inp(inp, np.ascontiguousarray(eH[0]).view(np.uint8), 16, 4, "top", front=np.zeros(0, np.uint8), back=np.zeros(0, np.uint8)).view(torch.int32)
        left = _inp(inp, np.ascontiguousarray(eH[:, 0]).view(np.uint8), 16, 12, "left", front=np.zeros(0, np.uint8), back=np.zeros(0, np.uint8)).view(torch.int32)
    out = Arena(torch, _dev(engine), arena_bytes((rows + 1) * (cols + 1) * 4, (rows + 1) * (cols + 1) * 4, 4 * trows + 4, 24))
    Ht, _ = _out(out, (rows + 1, cols + 1), torch.int32, 4, "H")
    Pt, _ = _out(out, (rows + 1, cols + 1), torch.int32, 0, "P")
    right, _ = _out(out, (trows + 1,), torch.int32, 4, "right", align=16)
    res = _result(out)
    engine.fill_tile(Ht, Pt, i0, j0, trows, tcols, d_a, d_b, res, top=top, left=left, right=right)
    engine.synchronize()
    assert engine.get_option("last_strips2") == 0 and engine.get_option("last_strips") == -(-tcols // 63)
    wantH = np.full((rows + 1, cols + 1), POISON32, np.int32)
    wantP = wantH.copy()
    lo = 1 if halo else 0
    wantH[i0 + lo:i0 + trows + 1, j0 + lo:j0 + tcols + 1] = eH[lo:, lo:]
    wantP[i0 + lo:i0 + trows + 1, j0 + lo:j0 + tcols + 1] = eP[lo:, lo:]
    gotH, gotP = Ht.cpu().numpy(), Pt.cpu().numpy()
    for name, got, want in (("H", gotH, wantH), ("P", gotP, wantP)):
        bad = np.argwhere(got != want)
        assert len(bad) == 0, f"{name}: {len(bad)} cells differ, first at {bad[0].tolist()} (tile rows {i0}..{i0 + trows}, columns {j0}..{j0 + tcols}): {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"
    assert np.array_equal(right.cpu().numpy(), eH[:, -1])
    inner = eH[1:, 1:]
    mp = int(np.argmax(inner))                       # lowest index among ties, relative to the corner with the full stride
    r = res.cpu().tolist()
    assert r[2] == 0 and r[1] == int(inner.max())
    if r[1] > 0:
        assert r[0] == (mp // tcols + 1) * (cols + 1) + mp % tcols + 1
    assert_guards(out)
    assert_guards(inp)


@pytest.mark.parametrize("cols,rows,p8,one_column", [(252, 96, False, False), (1000, 64, True, False), (252, 96, True, True), (1000, 64, False, True)])
def test_one_band(engine, oracle, cols, rows, p8, one_column):
    """The lower of two stacked bands as one band-resident launch: H row 0 receives the halo values, P row 0 stays poison, d_bot_gran has
    exactly cols + 1 granules and d_bot_done exactly ceil(cols / 63) words."""
    torch = engine.torch
    a, b = oracle.generate(cols, 2 * rows, 940 + cols)
    H, P, _ = oracle.fill(a, b)
    lo, hi = rows, 2 * rows
    nstrips = -(-cols // 63)
    inp = Arena(torch, _dev(engine), arena_bytes(cols + 128, rows + 128, 8 * cols + 8))
    d_a = _inp(inp, a, 64, 5, "a")
    d_b = _inp(inp, b[lo:], 256, 32, "b")
    gran = (np.int64(7) << 32) | H[lo].astype(np.int64)
    top_gran = _inp(inp, gran.view(np.uint8), 16, 8, "top_gran", front=np.zeros(0, np.uint8), back=np.zeros(0, np.uint8)).view(torch.int64)
    out = Arena(torch, _dev(engine), arena_bytes((rows + 1) * (cols + 1) * 4, (rows + 1) * (cols + 1) * 4, 8 * cols + 8, 4 * nstrips, 24))
    Ht, _ = _out(out, (rows + 1, cols + 1), torch.int32, 4, "H")
    Pt, _ = _out(out, (rows + 1, cols + 1), torch.int8 if p8 else torch.int32, 3 if p8 else 4, "P")
    bot, _ = _out(out, (cols + 1,), torch.int64, 8, "bot_gran", align=16)
    done, _ = _out(out, (nstrips,), torch.int32, 4, "bot_done", align=16)
    res = _result(out)
    engine.set_option("band_wait_ms", 5000)
    engine.set_option("debug_flags", NO_TWO_COLUMNS if one_column else 0)
    try:
        engine.fill_band(d_a, cols, d_b, rows, 2 * rows, Ht, Pt, res, top_gran=top_gran, top_tag=7, bot_gran=bot, bot_tag=8, bot_done=done)
        engine.synchronize()
        assert engine.get_option("last_strips2") == (0 if one_column else _strips(cols, 126))
    finally:
        engine.set_option("debug_flags", 0)
        engine.set_option("band_wait_ms", 0)
    r = res.cpu().tolist()
    assert r[2] == 0, "the band aborted"
    assert np.array_equal(Ht.cpu().numpy(), H[lo:hi + 1]), "H (row 0 = the halo values)"
    gotP = Pt.cpu().numpy()
    assert np.array_equal(gotP[1:].astype(np.int32), P[lo + 1:hi + 1]), "P"
    assert (gotP[0] == (POISON8 if p8 else POISON32)).all(), "P row 0 belongs to the band above"
    g = bot.cpu().numpy()
    assert np.array_equal(g >> 32, np.full(cols + 1, 8)) and np.array_equal((g & 0xffffffff).astype(np.int32), H[hi])
    assert (done.cpu().numpy() == 8).all()
    body = H[lo + 1:hi + 1]
    assert r[1] == int(body.max())
    if body.max() > H[lo].max():
        assert r[0] == int(np.argmax(body)) + cols + 1
    assert_guards(out)
    assert_guards(inp)


# ---- batch (sw_batch_device_ex, sw_batch_traceback_device) ----------------------------------------------------------------------------
def _batch_inputs(engine, inp, A, B, padded):
    """(d_a, d_b) as (npairs, stride) views; tight strides (cols, round16(rows)) or cols + 37 and round16(rows) + 48, every gap holding
    the tail of the pair in front of it again (live letters of a neighbouring pair's own alphabet)"""
    npairs, cols = A.shape
    rows = B.shape[1]
    astr = cols + (37 if padded else 0)
    bstr = (rows + 15) // 16 * 16 + (48 if padded else 0)
    Ab, Bb = np.empty((npairs, astr), np.uint8), np.empty((npairs, bstr), np.uint8)
    for k in range(npairs):
        Ab[k] = np.concatenate([A[k], live_tail(A[k], astr - cols)])
        Bb[k] = np.concatenate([B[k], live_tail(B[k], bstr - rows)])
    d_a = _inp(inp, Ab, 64, 1, "a", front=live_head(A[0], 64), back=live_tail(A[-1], 64)).view(npairs, astr)
    d_b = _inp(inp, Bb, 256, 32, "b", front=live_head(B[0], 64), back=live_tail(B[-1], 64)).view(npairs, bstr)
    return d_a, d_b


def _pairs(seed, npairs, cols, rows, letters=4):
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(b"ACGTNRYKMSWBDHVU", np.uint8)[:letters]
    return np.ascontiguousarray(alpha[rng.integers(0, letters, (npairs, cols))]), np.ascontiguousarray(alpha[rng.integers(0, letters, (npairs, rows))])


# (kernel, cols, rows, npairs, letters, output modes): a mode is (H?, P dtype or None, H skew, P skew)
BATCH_CASES = [
    (1, 300, 17, 5, 4, [(True, "i32", 0, 0), (True, "i32", 4, 4), (True, "i8", 4, 1), (False, "i32", 0, 4)]),
    (1, 1025, 50, 3, 4, [(True, "i32", 4, 0), (True, "i8", 0, 3), (True, "i8", 0, 7)]),
    (2, 777, 129, 3, 4, [(False, None, 0, 0), (False, "i8", 0, 0), (False, "i8", 0, 1), (False, "i8", 0, 4)]),
    (2, 528, 33, 5, 4, [(False, None, 0, 0), (False, "i8", 0, 3), (False, "i8", 0, 7)]),
    (0, 200, 150, 3, 12, [(True, "i32", 0, 0), (True, "i32", 4, 4), (True, "i8", 4, 3)]),
]


@pytest.mark.parametrize("kernel,cols,rows,npairs,letters,modes", BATCH_CASES, ids=[f"k{c[0]}-{c[1]}x{c[2]}x{c[3]}" for c in BATCH_CASES])
def test_batch(engine, oracle, kernel, cols, rows, npairs, letters, modes):
    """32-bit lanes (1), packed 16-bit lanes (2, odd pair counts: the last pair is stored once) and the fall-back (0), each with tight and
    with padded strides; the padded run must equal the oracle per pair AND the tight run."""
    torch = engine.torch
    A, B = _pairs(950 + cols, npairs, cols, rows, letters)
    ref = [oracle.fill(A[k], B[k]) for k in range(npairs)]
    want_res = np.array([[mp, int(h.flat[mp]), 0] for h, p, mp in ref], np.int64)
    cells = (rows + 1) * (cols + 1)
    inp = Arena(torch, _dev(engine), arena_bytes(npairs * (cols + 37) + 128, npairs * (rows + 64) + 128))
    out = Arena(torch, _dev(engine), arena_bytes(npairs * cells * 4, npairs * cells * 4, npairs * 24))
    for want_h, pk, hs, ps in modes:
        tight = None
        for padded in (False, True):
            inp.reset(); out.reset()
            d_a, d_b = _batch_inputs(engine, inp, A, B, padded)
            Ht = _out(out, (npairs, rows + 1, cols + 1), torch.int32, hs, "H")[0] if want_h else None
            Pt = _out(out, (npairs, rows + 1, cols + 1), torch.int8 if pk == "i8" else torch.int32, ps, "P")[0] if pk else None
            res = _result(out, npairs, "results")
            case = f"kernel {kernel}, {npairs} x {cols}x{rows}, H {want_h} (skew {hs}), P {pk} (skew {ps}), {'padded' if padded else 'tight'} strides"
            engine.batch_device(d_a, d_b, cols, rows, out=(res, Ht, Pt))
            assert engine.get_option("last_batch_kernel") == kernel, case
            got = [res.cpu().numpy(), Ht.cpu().numpy() if want_h else None, Pt.cpu().numpy().astype(np.int32) if pk else None]
            assert np.array_equal(got[0], want_res), case
            for k in range(npairs):
                assert not want_h or np.array_equal(got[1][k], ref[k][0]), f"{case}: H of pair {k}"
                assert not pk or np.array_equal(got[2][k], ref[k][1]), f"{case}: P of pair {k}"
            assert_guards(out)
            assert_guards(inp)
            if padded:
                assert all(x is None or np.array_equal(x, y) for x, y in zip(got, tight)), case + ": differs from the tight-stride run"
            tight = got


def test_batch_traceback_paths_between_guards(engine, oracle):
    torch = engine.torch
    npairs, cols, rows = 5, 300, 17
    A, B = _pairs(960, npairs, cols, rows)
    cells, cap = (rows + 1) * (cols + 1), cols + rows + 2
    inp = Arena(torch, _dev(engine), arena_bytes(npairs * (cols + 37) + 128, npairs * (rows + 64) + 128))
    out = Arena(torch, _dev(engine), arena_bytes(npairs * cells, npairs * cap * 8, npairs * 24))
    d_a, d_b = _batch_inputs(engine, inp, A, B, True)
    Pt, _ = _out(out, (npairs, rows + 1, cols + 1), torch.int8, 3, "P")
    paths, _ = _out(out, (npairs, cap), torch.int64, 8, "paths", align=16)
    res = _result(out, npairs, "results")
    engine.batch_device(d_a, d_b, cols, rows, traceback=True, want_paths=True, out=(res, None, Pt), paths=paths)
    assert engine.get_option("last_batch_kernel") == 1
    res, paths, Pn = res.cpu().numpy(), paths.cpu().numpy(), Pt.cpu().numpy().astype(np.int32)
    for k in range(npairs):
        h, p, mp = oracle.fill(A[k], B[k])
        opath = oracle.backtrack(p, mp)
        assert tuple(res[k]) == (mp, int(h.flat[mp]), len(opath)) and np.array_equal(paths[k, :len(opath)], opath) and np.array_equal(Pn[k], p), f"pair {k}"
    assert_guards(out)
    assert_guards(inp)


# ---- search, linear and affine --------------------------------------------------------------------------------------------------------
def _database(rng, alpha):
    """30 targets: empty, one letter, lane edges, random lengths up to 300; offsets[0] = 7 (the letters in front are live padding)"""
    lens = [0, 1, 63, 64, 65] + list(rng.integers(2, 301, 25))
    rng.shuffle(lens)
    offs = np.zeros(len(lens) + 1, np.int64)
    offs[0] = 7
    offs[1:] = 7 + np.cumsum(lens)
    return rng.choice(alpha, int(offs[-1])).astype(np.uint8), offs


def _search_inputs(engine, query, packed, qskew):
    inp = Arena(engine.torch, _dev(engine), arena_bytes(len(query) + 128, len(packed) + 128))
    d_q = _inp(inp, query, 64, qskew, "query")
    d_db = _inp(inp, packed, 64, 1, "db")            # (packed[:7] lies in front of offsets[0]: more live letters)
    return inp, d_q, d_db


@pytest.mark.parametrize("qlen,qskew", [(63, 1), (257, 2), (1025, 3)])
def test_search(engine, oracle, qlen, qskew):
    torch = engine.torch
    rng = np.random.default_rng(970 + qlen)
    query = rng.choice(DNA, qlen).astype(np.uint8)
    packed, offs = _database(rng, DNA)
    n = len(offs) - 1
    want = np.zeros((n, 3), np.int64)
    for k in range(n):
        if offs[k + 1] > offs[k]:
            st = oracle.fill_streaming(query, packed[offs[k]:offs[k + 1]])
            want[k] = (st["max_pos"], st["max_score"], 0)
    inp, d_q, d_db = _search_inputs(engine, query, packed, qskew)
    out = Arena(torch, _dev(engine), arena_bytes(n * 24))
    res = _result(out, n, "results")
    got = engine.search_device(d_q, qlen, d_db, offs, out=res)
    engine.synchronize()
    assert got.shape == (n, 3) and np.array_equal(got.cpu().numpy(), want)
    assert engine.get_option("last_search_kernel") == 2 * ((4 if qlen <= 256 else 8 if qlen <= 512 else 16) // 8)
    assert_guards(out)
    assert_guards(inp)


@pytest.mark.parametrize("qlen,qskew", [(63, 1), (257, 2), (1025, 3)])
def test_search_affine_twice(engine, checker, qlen, qskew):  # noqa: F811
    """two queries one after the other on the same engine: the profile and boundary workspaces are reused, the outputs are fresh poison"""
    torch = engine.torch
    rng = np.random.default_rng(980 + qlen)
    packed, offs = _database(rng, PROTEIN)
    n = len(offs) - 1
    sub = random_submat(rng)
    out = Arena(torch, _dev(engine), arena_bytes(n * 24))
    for go, ge in ((-10, -1), (-3, -2)):
        query = rng.choice(PROTEIN, qlen).astype(np.uint8)
        inp, d_q, d_db = _search_inputs(engine, query, packed, qskew)
        out.reset()
        res = _result(out, n, "results")
        got = engine.search_affine_device(d_q, qlen, d_db, offs, sub, go, ge, out=res)
        engine.synchronize()
        assert np.array_equal(got.cpu().numpy(), checker.search(query, packed, offs, sub, go, ge)), (go, ge)
        assert engine.get_option("last_search_affine_kernel") in ((0,) if qlen <= 256 else (1,) if qlen <= 512 else (1, 2))
        assert_guards(out)
        assert_guards(inp)


# ---- align ----------------------------------------------------------------------------------------------------------------------------
def _related_targets(rng, query, count):
    """slices of the query with substitutions and indels: the walks are long"""
    targets = []
    for _ in range(count):
        s = list(query[int(rng.integers(0, max(1, len(query) // 8))):])
        for _ in range(3):
            if len(s) > 50:
                at, run = int(rng.integers(20, len(s) - 20)), int(rng.integers(1, 8))
                if rng.random() < 0.5:
                    del s[at:at + run]
                else:
                    s[at:at] = list(rng.choice(PROTEIN, run))
        for at in rng.integers(0, len(s), len(s) // 12):
            s[int(at)] = int(rng.choice(PROTEIN))
        targets.append(np.array(s, np.uint8))
    return targets


def _align_case(rng, checker, qlen):  # noqa: F811
    query = rng.choice(PROTEIN, qlen).astype(np.uint8)
    targets = _related_targets(rng, query, 8)
    hits = [0, 1, 2, 3, 4, 5, 6, 7, 2, 2, 5, 0]
    sub, go, ge = random_submat(rng), -10, -1
    exp = [expected(checker, query, t, sub, go, ge) for t in targets]
    return query, targets, hits, sub, go, ge, exp


def _check_align(engine, query, targets, hits, sub, go, ge, exp, cap, qskew):
    torch = engine.torch
    packed, offs = pack(targets)
    packed = np.concatenate([live_head(packed, 7), packed])
    offs = offs + 7
    inp, d_q, d_db = _search_inputs(engine, query, packed, qskew)
    nh = len(hits)
    out = Arena(torch, _dev(engine), arena_bytes(nh * 56, nh * cap))
    aln, _ = _out(out, (nh, 7), torch.int64, 8, "aln", align=16)
    ops, _ = _out(out, (nh, cap), torch.uint8, 1, "ops", align=64)
    engine.align_affine_device(d_q, len(query), d_db, offs, sub, go, ge, hits, ops_cap=cap, out=(aln, ops))
    engine.synchronize()
    aln, ops = aln.cpu().numpy(), ops.cpu().numpy()
    for h, k in enumerate(hits):
        row, eops, _ = exp[k]
        assert tuple(int(x) for x in aln[h]) == row, f"ops_cap {cap}, hit {h} (target {k})"
        if row[6] <= cap:   # the ops, then poison; a row with nops > ops_cap may hold anything -- inside itself
            assert ops[h, :row[6]].tobytes() == eops and (ops[h, row[6]:] == POISON).all(), f"ops_cap {cap}, hit {h} (target {k}): ops"
    assert_guards(out)
    assert_guards(inp)


@pytest.mark.parametrize("qlen,qskew", [(65, 1), (513, 2), (1025, 3)])
def test_align_ops_capacities(engine, checker, qlen, qskew):  # noqa: F811
    """ops_cap exactly sufficient, about half of the median nops, and 1: nops is always the true length, and a hit that does not fit
    writes nothing outside its own row (the header's promise)"""
    rng = np.random.default_rng(990 + qlen)
    query, targets, hits, sub, go, ge, exp = _align_case(rng, checker, qlen)
    nops = sorted(exp[k][0][6] for k in hits)
    assert nops[0] >= 1 and nops[-1] > qlen // 2, "the walks were meant to be long"
    for cap in (nops[-1], max(2, nops[len(nops) // 2] // 2), 1):
        _check_align(engine, query, targets, hits, sub, go, ge, exp, cap, qskew)
        assert engine.get_option("last_align_affine_kernel") in ((0,) if qlen <= 256 else (1,) if qlen <= 512 else (1, 2))
        assert engine.get_option("last_align_affine_slots") == len(hits)


def test_align_one_slot_reused_under_poison(swamd, checker):  # noqa: F811
    rng = np.random.default_rng(995)
    query, targets, hits, sub, go, ge, exp = _align_case(rng, checker, 513)
    eng = swamd.Engine(0)
    try:
        eng.set_option("align_workspace_mib", 1)
        _check_align(eng, query, targets, hits, sub, go, ge, exp, max(exp[k][0][6] for k in hits), 1)
        assert eng.get_option("last_align_affine_slots") in (1, 2)
    finally:
        eng.close()


# ---- side stream ----------------------------------------------------------------------------------------------------------------------
def _side_stream(engine, staged, call):
    """On a stream of its own: ~10 ms of device work (a fill_ over 2 GiB), then the device-to-device copies that bring the real inputs
    from their staging tensors into buffers that hold poison until then, then the library call; only that stream is synchronised.  A
    helper launch or memset the library put on another stream would read the poison, or write before the copies."""
    torch = engine.torch
    busy = torch.empty(2 << 30, dtype=torch.uint8, device=_dev(engine))
    torch.cuda.synchronize()                                        # (the poison is in place)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        busy.fill_(1)
        for dst, src in staged:
            dst.copy_(src, non_blocking=True)
        call()
        s.synchronize()
    del busy


def _staged(engine, arr):
    """(a poisoned device buffer of the array's size + 64, the staging tensor with the data and live padding behind it)"""
    torch = engine.torch
    arr = np.ascontiguousarray(arr, np.uint8)
    flat = np.concatenate([arr.reshape(-1), live_tail(arr.reshape(-1), 64)])
    dst = torch.full((len(flat),), POISON, dtype=torch.uint8, device=_dev(engine))
    return dst, torch.from_numpy(flat).to(_dev(engine))


def test_side_stream_fill(engine, swamd, oracle):
    torch = engine.torch
    cols, rows = 1007, 304
    a, b = oracle.generate(cols, rows, 1001)
    H, P, mp = oracle.fill(a, b)
    (d_a, s_a), (d_b, s_b) = _staged(engine, a), _staged(engine, b)
    out = Arena(torch, _dev(engine), arena_bytes((rows + 1) * (cols + 1) * 4, (rows + 1) * (cols + 1) * 4, 24))
    Ht, _ = _out(out, (rows + 1, cols + 1), torch.int32, 0, "H")
    Pt, _ = _out(out, (rows + 1, cols + 1), torch.int32, 0, "P")
    res = _result(out)
    _side_stream(engine, [(d_a, s_a), (d_b, s_b)], lambda: engine.fill_into(swamd.Fill(Ht, Pt, res, cols, rows), d_a, d_b))
    assert res.cpu().tolist() == [mp, int(H.flat[mp]), 0]
    assert np.array_equal(Ht.cpu().numpy(), H) and np.array_equal(Pt.cpu().numpy(), P)
    assert_guards(out)


def test_side_stream_batch(engine, oracle):
    torch = engine.torch
    npairs, cols, rows = 5, 300, 32
    A, B = _pairs(1002, npairs, cols, rows)
    (d_a, s_a), (d_b, s_b) = _staged(engine, A), _staged(engine, B)
    cells = (rows + 1) * (cols + 1)
    out = Arena(torch, _dev(engine), arena_bytes(npairs * cells * 4, npairs * cells * 4, npairs * 24))
    Ht, _ = _out(out, (npairs, rows + 1, cols + 1), torch.int32, 0, "H")
    Pt, _ = _out(out, (npairs, rows + 1, cols + 1), torch.int32, 0, "P")
    res = _result(out, npairs, "results")
    _side_stream(engine, [(d_a, s_a), (d_b, s_b)],
                 lambda: engine.batch_device(d_a[:npairs * cols].view(npairs, cols), d_b[:npairs * rows].view(npairs, rows), cols, rows, out=(res, Ht, Pt)))
    assert engine.get_option("last_batch_kernel") == 1
    got = res.cpu().numpy()
    for k in range(npairs):
        h, p, mp = oracle.fill(A[k], B[k])
        assert tuple(got[k]) == (mp, int(h.flat[mp]), 0) and np.array_equal(Ht[k].cpu().numpy(), h) and np.array_equal(Pt[k].cpu().numpy(), p), f"pair {k}"
    assert_guards(out)


def test_side_stream_search_affine(engine, checker):  # noqa: F811
    torch = engine.torch
    rng = np.random.default_rng(1003)
    query = rng.choice(PROTEIN, 1025).astype(np.uint8)
    packed, offs = _database(rng, PROTEIN)
    sub = random_submat(rng)
    n = len(offs) - 1
    (d_q, s_q), (d_db, s_db) = _staged(engine, query), _staged(engine, packed)
    out = Arena(torch, _dev(engine), arena_bytes(n * 24))
    res = _result(out, n, "results")
    _side_stream(engine, [(d_q, s_q), (d_db, s_db)], lambda: engine.search_affine_device(d_q, 1025, d_db, offs, sub, -10, -1, out=res))
    assert np.array_equal(res.cpu().numpy(), checker.search(query, packed, offs, sub, -10, -1))
    assert_guards(out)


def test_side_stream_align_affine(engine, checker):  # noqa: F811
    torch = engine.torch
    rng = np.random.default_rng(1004)
    query, targets, hits, sub, go, ge, exp = _align_case(rng, checker, 513)
    packed, offs = pack(targets)
    cap = max(exp[k][0][6] for k in hits)
    (d_q, s_q), (d_db, s_db) = _staged(engine, query), _staged(engine, packed)
    out = Arena(torch, _dev(engine), arena_bytes(len(hits) * 56, len(hits) * cap))
    aln, _ = _out(out, (len(hits), 7), torch.int64, 8, "aln", align=16)
    ops, _ = _out(out, (len(hits), cap), torch.uint8, 1, "ops", align=64)
    _side_stream(engine, [(d_q, s_q), (d_db, s_db)],
                 lambda: engine.align_affine_device(d_q, 513, d_db, offs, sub, go, ge, hits, ops_cap=cap, out=(aln, ops)))
    aln, ops = aln.cpu().numpy(), ops.cpu().numpy()
    for h, k in enumerate(hits):
        row, eops, _ = exp[k]
        assert tuple(int(x) for x in aln[h]) == row and ops[h, :row[6]].tobytes() == eops, f"hit {h} (target {k})"
    assert_guards(out)
    assert POISON64 < 0


# ---- the PSSM update and the hit weights ----------------------------------------------------------------------------------------------
def _table(ar, arr, skew, name):
    """An int32 / int64 input table at its natural alignment plus an odd multiple of it, must-stay, between poison."""
    arr = np.ascontiguousarray(arr)
    t, c = ar.place(arr.reshape(-1).view(np.uint8), 256, skew, name=name)
    assert skew % arr.itemsize == 0 and (skew // arr.itemsize) % 2 == 1
    return ar.view(c, {4: ar.torch.int32, 8: ar.torch.int64}[arr.itemsize], (arr.size,))


@pytest.mark.parametrize("skew", [0, 1, 3])
@pytest.mark.parametrize("kind", ["synthetic", "garbage"])
def test_pssm_hit_weights_and_update(engine, swamd, kind, skew):
    """sw_db_pssm_hit_weights, then sw_db_pssm_from_hits out of place with counts and in place without, every buffer carved out of one
    poisoned arena per direction: the database, the ops, the prior and the matrix at base % 64 = skew, the int64 tables (hits, nhits,
    alignments) at 8 x 3 and the int32 ones (weights, counts) at 4 x 3 past a 256-byte line.  After each call the inputs hold their bytes,
    every guard is whole and only the outputs of THAT call changed.  24 letters, top 9; the garbage table trips every guard of the rule
    (tests/pssm_hits_cases.py: garbage).  Expected: the host legs (held to the numpy rules in tests/test_pssm_*_host.py)."""
    torch = engine.torch
    rng = np.random.default_rng(1200 + skew)
    c = hc.synthetic(rng, 24, 9)
    if kind == "garbage":
        c = hc.garbage(rng, c)
    else:
        c.nhits = np.array([9, 0, 4, 9, 8, 9], np.int64)
    per_hit, pw, inc = 16, 3, 20
    nl, nq, top = len(c.letters), len(c.qoffs) - 1, 9
    front, total = int(c.qoffs[0]) * nl, int(c.qoffs[-1]) * nl
    exp_w = wc.host_leg(swamd, c, per_hit, inc)
    exp_out, exp_cnt = hc.host_leg(swamd, c, pw, inc, exp_w)
    assert exp_w.any() and exp_cnt.any() and (exp_out != np.minimum(c.prior[int(c.qoffs[0]):], c.smax)).any()
    prior_bytes = np.ascontiguousarray(c.prior).reshape(-1).view(np.uint8)

    inp = Arena(torch, _dev(engine), arena_bytes(len(c.packed) + 128, c.ops.size + 128, total + 128, c.hits.size * 8, nq * 8, c.aln.size * 8))
    d_db = _inp(inp, c.packed, 64, skew, "db")
    d_ops = _inp(inp, c.ops, 64, skew, "ops")
    d_prior = _inp(inp, prior_bytes, 64, skew, "prior").view(torch.int8)
    d_hits = _table(inp, c.hits, 24, "hits")
    d_nhits = _table(inp, c.nhits, 24, "nhits")
    d_aln = _table(inp, c.aln, 24, "aln")
    out = Arena(torch, _dev(engine), arena_bytes(nq * top * 4, (total - front) * 4, total, total))
    d_w, c_w = _out(out, (nq * top,), torch.int32, 12, "weights")
    d_cnt, c_cnt = _out(out, (total - front,), torch.int32, 12, "counts")
    d_m, c_m = _out(out, (total,), torch.int8, skew, "matrix", align=64)
    c_in = out.carve(total, 64, skew, name="in place")
    d_in = out.view(c_in, torch.int8, (total,))
    d_in.copy_(d_prior)
    for cv in (c_cnt, c_m):
        out.must_stay(cv)
    out.must_stay(c_in, prior_bytes)

    def unchanged(case):
        assert_guards(out)
        assert_guards(inp)

    with engine.prepare_db(d_db, c.offs) as db:
        # the weights: only their carve changes
        got = db.pssm_hit_weights_device(c.qoffs, hc.scoring(c), (per_hit, inc), d_hits, d_nhits, d_aln, d_ops, c.cap, out=d_w, top=top)
        assert got.data_ptr() == d_w.data_ptr() and engine.get_option("last_pssm_weights_launches") == 2
        engine.synchronize()
        assert np.array_equal(d_w.cpu().numpy().reshape(nq, top), exp_w), "weights"
        unchanged("weights")
        # the update out of place, with counts, reading the weights: the weights are an input now
        out.must_stay(c_w, exp_w.reshape(-1).view(np.uint8))
        c_cnt.expect = c_m.expect = None
        db.pssm_from_hits_device(d_prior, c.qoffs, hc.scoring(c), (c.sub, pw, inc), d_hits, d_nhits, d_aln, d_ops, c.cap, weights=d_w, out=d_m, top=top,
                                 counts=d_cnt)
        assert engine.get_option("last_pssm_hits_launches") == 1
        engine.synchronize()
        m = d_m.cpu().numpy()
        assert (m[:front] == POISON8).all(), "the columns in front of the first query were written"
        assert np.array_equal(m[front:].reshape(-1, nl), exp_out), "matrix"
        assert np.array_equal(d_cnt.cpu().numpy().reshape(-1, nl), exp_cnt), "counts"
        unchanged("update")
        # in place, matrix only: the counts and the matrix of the call before are must-stay now
        out.must_stay(c_cnt, exp_cnt.reshape(-1).view(np.uint8))
        out.must_stay(c_m, m.view(np.uint8))
        c_in.expect = None
        db.pssm_from_hits_device(d_in, c.qoffs, hc.scoring(c), (c.sub, pw, inc), d_hits, d_nhits, d_aln, d_ops, c.cap, weights=d_w, out=d_in, top=top)
        assert engine.get_option("last_pssm_hits_launches") == 1
        engine.synchronize()
        m2 = d_in.cpu().numpy()
        assert np.array_equal(m2[:front].view(np.uint8), prior_bytes[:front]), "the columns in front of the first query changed"
        assert np.array_equal(m2[front:].reshape(-1, nl), exp_out), "matrix in place"
        unchanged("update in place")
