"""GPU: the prologue of the two-column kernel (sw_systolic2.inc) -- the alphabet scan, shared behind a grid barrier or done by every
workgroup for itself (the planner's limit kScanAllLetters: cols + rows <= 48 Ki letters scan for themselves), the code table, every
workgroup's padded copy of b and its letter codes, the cleared row 0 / column 0 -- against the oracle, cell for cell, on the shapes
that stress it, and the two scans against each other.  Debug bits 28 / 29 force the shared / the private scan."""
import numpy as np
import pytest

from test_fill_gpu import check_against_oracle

pytestmark = pytest.mark.gpu

BARRIER_SCAN, SCAN_ALL, WRAP_EARLY = 1 << 28, 1 << 29, 1 << 10
LIMIT = 48 * 1024     # swp::kScanAllLetters
SCANS = [pytest.param((BARRIER_SCAN, 0), id="barrier"), pytest.param((SCAN_ALL, 1), id="scan_all")]


@pytest.fixture
def scan(engine, request):
    """the scan forced by the parametrisation: (debug flags, what last_scan_all must report)"""
    yield request.param
    engine.set_option("debug_flags", 0)


def _letters(rng, letters, n):
    return rng.choice(np.frombuffer(letters, np.uint8), size=n).astype(np.uint8)


def _check(engine, oracle, a, b, want_scan, two_cols=True, **kw):
    out = check_against_oracle(engine, oracle, a, b, **kw)
    if two_cols:
        assert engine.get_option("last_strips2") > 0, "the two-column kernel was expected to run"
        assert engine.get_option("last_scan_all") == want_scan
    return out


@pytest.mark.parametrize("scan", SCANS, indirect=True)
@pytest.mark.parametrize("cols,rows", [(500, 1), (500, 5), (500, 15), (500, 17), (1000, 333), (127, 1295), (2000, 12289), (1, 1), (1, 3000), (3000, 1),
                                       (2, 4097), (4097, 2)])
def test_shapes_that_stress_the_prologue(engine, oracle, scan, cols, rows):
    """rows not a multiple of 16, fewer rows than one 16-byte piece of the coded copy, one more row than a whole pass of the workgroup
    (768 threads x 16 bytes), 1 x N and N x 1"""
    flags, want = scan
    engine.set_option("debug_flags", flags)
    a, b = oracle.generate(cols, rows, 91)
    _check(engine, oracle, a, b, want)


@pytest.mark.parametrize("scan", SCANS, indirect=True)
def test_seven_and_eight_letters(engine, oracle, scan):
    """exactly 7 letters: the two-column kernel fills; exactly 8: it leaves the shared padded copies and the one-column kernel fills"""
    flags, want = scan
    engine.set_option("debug_flags", flags)
    rng = np.random.default_rng(7)
    a, b = _letters(rng, b"ACGTNRY", 900), _letters(rng, b"ACGTNRY", 330)
    a[:7] = np.frombuffer(b"ACGTNRY", np.uint8)
    _check(engine, oracle, a, b, want)
    a8, b8 = _letters(rng, b"ACGTNRYK", 900), _letters(rng, b"ACGTNRYK", 330)
    a8[:8] = np.frombuffer(b"ACGTNRYK", np.uint8)
    _check(engine, oracle, a8, b8, want)


@pytest.mark.parametrize("scan", SCANS, indirect=True)
@pytest.mark.parametrize("where", ["last_of_b", "last_of_a"])
@pytest.mark.parametrize("cols,rows", [(900, 330), (1003, 4099)])
def test_eighth_letter_in_the_last_byte(engine, oracle, scan, where, cols, rows):
    """the letter that decides who fills sits in the very last byte a scan reads (of b, of a): missed, the two-column kernel would fill
    with a code table of seven letters"""
    flags, want = scan
    engine.set_option("debug_flags", flags)
    rng = np.random.default_rng(8)
    a, b = _letters(rng, b"ACGTNRY", cols), _letters(rng, b"ACGTNRY", rows)
    a[:7] = np.frombuffer(b"ACGTNRY", np.uint8)
    (b if where == "last_of_b" else a)[-1] = ord("K")
    _check(engine, oracle, a, b, want)


@pytest.mark.parametrize("scan", SCANS, indirect=True)
def test_b_rewritten_on_the_device_between_fills(engine, oracle, scan):
    """the same device buffers and outputs: 4 letters, then 20 letters written into d_b on the device, then 4 again -- every fill finds
    its own alphabet (nothing about it may be remembered on the host)"""
    import torch
    flags, want = scan
    engine.set_option("debug_flags", flags)
    rng = np.random.default_rng(9)
    cols, rows = 1500, 700
    a = _letters(rng, b"ACGT", cols)
    b4, b20, b4b = _letters(rng, b"ACGT", rows), _letters(rng, b"ACDEFGHIKLMNPQRSTVWY", rows), _letters(rng, b"ACGT", rows)
    d_a, _ = engine.to_device(a)
    d_b, _ = engine.to_device(b4)
    out = engine.alloc(cols, rows)
    for b in (b4, b20, b4b):
        d_b[:rows] = torch.from_numpy(b.copy()).to(d_b.device)
        engine.fill_into(out, d_a, d_b)
        engine.synchronize()
        assert engine.get_option("last_strips2") > 0 and engine.get_option("last_scan_all") == want
        H, P, mp = oracle.fill(a, b)
        assert np.array_equal(out.H.cpu().numpy(), H) and np.array_equal(out.P.cpu().numpy(), P)
        r = out.result()
        assert r["max_pos"] == mp and r["max_score"] == int(H.flat[mp])


@pytest.mark.parametrize("scan", SCANS, indirect=True)
def test_column_tiles(engine, oracle, swamd, scan):
    """30001 columns in strips every 126: column tiles, one launch each -- every tile scans the whole a and decides alike"""
    flags, want = scan
    engine.set_option("debug_flags", flags)
    engine.set_option("s2w", 126)
    try:
        a, b = swamd.generate(30001, 333, 5)
        b[-1] = ord("N")
        out = engine.fill(a, b)
        assert engine.get_option("last_tiles") >= 2 and engine.get_option("last_scan_all") == want
    finally:
        engine.set_option("s2w", 0)
    H, P, mp = oracle.fill(a, b)
    assert np.array_equal(out.H.cpu().numpy(), H) and np.array_equal(out.P.cpu().numpy(), P)
    r = out.result()
    assert r["max_pos"] == mp and r["max_score"] == int(H.flat[mp])


@pytest.mark.parametrize("scan", SCANS, indirect=True)
def test_band_with_a_top_halo(engine, oracle, swamd, scan):
    """stacked bands on the two-column kernel: the lower band's row 0 is its halo row (it arrives as granules while the kernel runs) --
    the prologue clears column 0 and leaves that row alone"""
    from test_band_gpu import _bands
    flags, want = scan
    engine.set_option("debug_flags", flags)
    _bands(engine, oracle, swamd, 1300, 640, (320,))
    assert engine.get_option("last_strips2") == 11 and engine.get_option("last_scan_all") == want
    _bands(engine, oracle, swamd, 2520, 912, (304, 608), p8=True, want_h=False)
    assert engine.get_option("last_strips2") == 20 and engine.get_option("last_scan_all") == want


@pytest.mark.parametrize("scan", SCANS, indirect=True)
def test_launch_tag_wrap(engine, oracle, scan):
    """debug bit 10: the 8-bit launch tag wraps after three launches (the edge values are wiped in between)"""
    flags, want = scan
    engine.set_option("debug_flags", flags | WRAP_EARLY)
    for k, (cols, rows) in enumerate([(2000, 300), (700, 1000), (2000, 300), (5000, 77), (700, 1000), (2000, 300), (127, 40), (2000, 300)]):
        a, b = oracle.generate(cols, rows, 20 + k)
        H, P, mp = oracle.fill(a, b)
        out = engine.fill(a, b)
        assert engine.get_option("last_scan_all") == want
        assert np.array_equal(out.H.cpu().numpy(), H) and np.array_equal(out.P.cpu().numpy(), P), (k, cols, rows)
        assert out.result()["max_pos"] == mp


@pytest.mark.parametrize("cols,rows", [(2, LIMIT - 2), (2, LIMIT - 1), (LIMIT - 1, 1), (LIMIT, 1), (LIMIT - 2, 2), (LIMIT - 1, 2)])
def test_both_sides_of_the_planners_limit(engine, oracle, swamd, cols, rows):
    """cols + rows at the limit and one letter beyond it: the planner's own choice of the scan, then the other one forced -- the same
    matrices, the oracle's"""
    import torch
    a, b = swamd.generate(cols, rows, 12)
    want = 1 if cols + rows <= LIMIT else 0
    H, P, mp = oracle.fill(a, b)
    outs = []
    try:
        for flags, w in ((0, want), (BARRIER_SCAN if want else SCAN_ALL, 1 - want)):
            engine.set_option("debug_flags", flags)
            out = engine.fill(a, b)
            assert engine.get_option("last_strips2") > 0 and engine.get_option("last_scan_all") == w
            assert np.array_equal(out.H.cpu().numpy(), H) and np.array_equal(out.P.cpu().numpy(), P)
            assert out.result()["max_pos"] == mp and out.result()["max_score"] == int(H.flat[mp])
            outs.append(out)
    finally:
        engine.set_option("debug_flags", 0)
    assert torch.equal(outs[0].H, outs[1].H) and torch.equal(outs[0].P, outs[1].P) and outs[0].result() == outs[1].result()
