"""CPU: the host leg of the PSSM update (sw_pssm_from_hits_host) against the numpy restatement of its rule (tests/pssm_hits_cases.py),
byte for byte on counts and matrix -- synthetic tables around every 64-op chunk edge, real tables from the host legs of the search and
the alignment, garbage tables between guard bytes, and the arithmetic edges the GPU test shares (sums beyond 2^32, the rounding table
at numerators of 1e10, both clamps, unobserved columns, 3 to 256 letters, full-range S and prior) --, its refusals, the writer sw_write_pssm read back by sw_read_pssm, and both in a
stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import pssm_hits_cases as cases
from affine_cases import ROOT

EINVAL = -22


def weights_of(rng, kind, nq, top):
    if kind == "none":
        return None
    if kind == "zeros":                                  # small weights, zeros among them
        return rng.integers(0, 4, (nq, top)).astype(np.int32)
    w = rng.integers(-3, 9, (nq, top)).astype(np.int32)  # "wild": negative values and values above 65535, taken as 0 and 65535
    w.reshape(-1)[::5] = 70000
    w.reshape(-1)[1::7] = -2**31
    return w


def check(swamd, c, pw, inc, w):
    exp_out, exp_counts, used = cases.reference(c, pw, inc, w)
    front = int(c.qoffs[0])
    out, counts = cases.host_leg(swamd, c, pw, inc, w)
    assert (counts == exp_counts).all()
    assert (out == exp_out[front:]).all()
    return exp_out[front:], exp_counts, used


@pytest.mark.parametrize("top", [1, 3, 64])
@pytest.mark.parametrize("nletters", [1, 4, 24, 256])
def test_synthetic_tables(swamd, nletters, top):
    rng = np.random.default_rng(100 * nletters + top)
    c = cases.synthetic(rng, nletters, top)
    assert (c.prior > c.smax).any()                      # prior entries above smax: taken as smax
    nq = len(cases.QLENS)
    seen_den0 = False
    for pw, kind in [(0, "none"), (1, "zeros"), (65535, "wild"), (0, "zeros"), (2, "wild")]:
        out, counts, used = check(swamd, c, pw, 0, weights_of(rng, kind, nq, top))
        seen_den0 |= pw == 0 and (counts.sum(axis=1) == 0).any()
        assert used.any()
    assert seen_den0                                     # columns with den == 0 occurred: they keep the clamped prior
    # in place, counts only, matrix only: the same bytes
    w = weights_of(rng, "wild", nq, top)
    out, counts = cases.host_leg(swamd, c, 2, 0, w)
    assert (cases.host_leg(swamd, c, 2, 0, w, in_place=True, want_counts=False)[0] == out).all()
    assert (cases.host_leg(swamd, c, 2, 0, w, want_out=False)[1] == counts).all()


def test_nothing_included_gives_the_clamped_prior(swamd):
    rng = np.random.default_rng(7)
    c = cases.synthetic(rng, 24, 3)
    front = int(c.qoffs[0])
    for pw in (0, 1, 65535):
        out, counts = cases.host_leg(swamd, c, pw, int(c.aln[:, :, 1].max()) + 1, None)
        assert (counts == 0).all() and (out == np.minimum(c.prior[front:], c.smax)).all()
        check(swamd, c, pw, int(c.aln[:, :, 1].max()) + 1, None)
    out, counts = cases.host_leg(swamd, c, 1, int(c.aln[:, :, 1].max()), None)   # ... and AT the best score that entry counts
    assert counts.sum() > 0


@pytest.mark.parametrize("pw,prior,s,w,exp", [
    (1, -3, 0, 1, -1),       # (-3 + 0) / 2 = -1.5, a tie: half up is -1
    (1, -5, 0, 1, -2),       # -2.5 -> -2
    (1, -5, 0, 2, -2),       # -5 / 3 = -1.67 -> -2; truncating (2 num + den) / (2 den) = -7 / 6 would give -1
    (2, -1, 0, 1, -1),       # -2 / 3 = -0.67 -> -1; truncating -1 / 6 would give 0
    (1, 5, 0, 1, 3),         # 2.5 -> 3
    (1, 4, -7, 2, -3),       # (4 - 14) / 3 = -3.33 -> -3
    (0, 9, -128, 1, -128),   # the observed row alone
    (1, 100, 127, 65535, 127),
])
def test_round_half_up_with_floor_division(swamd, pw, prior, s, w, exp):
    """One column, one letter, one 'M': out = round_half_up((pw * prior + w * s) / (pw + w)) with negative numerators."""
    rng = np.random.default_rng(1)
    c = cases.synthetic(rng, 1, 1, qlens=[1], smax=127, dup_targets=[1])
    c.packed[:] = c.letters[0]
    c.prior[:] = prior
    c.sub[:] = s
    c.aln[0, 0] = (0, 5, 0, 0, 0, 0, 1)
    c.ops[0, 0] = cases.M
    out, counts, _ = check(swamd, c, pw, 0, np.array([[w]], np.int32))
    assert counts[0, 0] == w and out[0, 0] == exp


@pytest.mark.parametrize("row", cases.ROUNDING, ids=lambda r: f"pw{r[0]}_p{r[1]}_s{r[2][0]}_{r[2][1]}_n{r[3][0]}")
def test_rounding_at_numerators_of_1e10(swamd, row):
    """The rounding table at N[j] = 4096 x 65535: exact halves of both signs, a hair on either side of one, floor against truncation."""
    c, w = cases.rounding_case(*row)
    out, counts, _ = check(swamd, c, row[0], 0, w)
    assert counts.sum() >= 4095 * 65535 and (out == row[5]).all()


@pytest.mark.parametrize("first", [2048, 3072])
def test_products_beyond_32_bits(swamd, first):
    """C x S = 1.7e10 (the builder asserts it): equal halves, and the twin whose sum itself passes 2^32."""
    c, w = cases.overflow_case(first)
    for pw in (0, 1, 65535):
        out, _, _ = check(swamd, c, pw, 0, w)
        want = [63, 63, 63] if first == 3072 else [0, 0, 0] if pw == 0 else [-1, 0, -1]
        assert (out == want).all(), (pw, out[0])


@pytest.mark.parametrize("smax", [0, 127])
@pytest.mark.parametrize("s", [127, -128])
def test_both_clamps(swamd, s, smax):
    c = cases.clamp_case(s, smax)
    for pw in (0, 1, 65535):
        out, counts, _ = check(swamd, c, pw, 0, None)
        seen = counts.sum(axis=1) > 0
        assert (out[~seen] == -128).all()                # min(-128, smax), observed or not
    out, counts, _ = check(swamd, c, 0, 0, None)
    assert (out[counts.sum(axis=1) > 0] == s).all()


@pytest.mark.parametrize("smax", [0, 1, 127])
def test_an_unobserved_column_keeps_its_clamped_prior_exactly(swamd, smax):
    """den == 0 (prior_weight 0) and den == prior_weight (the kernel's shortcut): P itself, negative and odd P among them."""
    rng = np.random.default_rng(40 + smax)
    c = cases.full_range_case(rng, 5, 3, smax)
    front, nothing = int(c.qoffs[0]), int(c.aln[:, :, 1].max()) + 1
    want = np.minimum(c.prior[front:], smax)
    assert (want % 2 == 1).any() and (want < 0).any()
    for pw in (0, 1, 2, 65535):
        out, counts, _ = check(swamd, c, pw, nothing, None)
        assert not counts.any() and (out == want).all()
        out, counts, _ = check(swamd, c, pw, 0, None)    # ... and with entries used: the columns no entry reaches
        assert (out[counts.sum(axis=1) == 0] == want[counts.sum(axis=1) == 0]).all() and (counts.sum(axis=1) == 0).any()


@pytest.mark.parametrize("nletters", [3, 5, 255, 256])
def test_alphabets_of_3_5_255_and_256_letters(swamd, nletters):
    rng = np.random.default_rng(7000 + nletters)
    c, _ = cases.alphabet_case(rng, nletters, 9)
    for pw, kind in [(0, "none"), (2, "wild")]:
        check(swamd, c, pw, 0, weights_of(rng, kind, len(cases.QLENS), 9))


@pytest.mark.parametrize("smax", [0, 1, 127])
@pytest.mark.parametrize("nletters", [5, 256])
def test_full_range_inputs(swamd, nletters, smax):
    rng = np.random.default_rng(8000 + nletters + smax)
    c = cases.full_range_case(rng, nletters, 9, smax)
    clamps = set()
    for pw, kind in [(0, "none"), (1, "zeros"), (3, "wild"), (65535, "wild")]:
        out, _, _ = check(swamd, c, pw, 0, weights_of(rng, kind, len(cases.QLENS), 9))
        clamps |= {int(out.min()), int(out.max())}
    assert {-128, 127} <= clamps or smax < 127


def test_real_tables(swamd):
    rng = np.random.default_rng(11)
    c = cases.real(swamd, rng, top=8)
    for pw, inc in [(1, 1), (10, 1), (0, 30)]:
        out, counts, used = check(swamd, c, pw, inc, None)
    out, counts, used = check(swamd, c, 10, 1, None)
    front = int(c.qoffs[0])
    assert (out != np.minimum(c.prior[front:], c.smax)).any()              # the update moved the matrix
    # the Python mirror: the alignment call's own outputs go straight in
    aln, ops = swamd.align_pssm_hits_host((c.prior, c.qoffs), (c.packed, c.offs), cases.scoring(c), c.hits, c.nhits)
    m, cnt = swamd.pssm_from_hits_host((c.prior, c.qoffs), (c.packed, c.offs), cases.scoring(c), (c.sub, 10, 1), c.hits, c.nhits, aln, ops, want_counts=True)
    assert (m[front:] == out).all() and (cnt == counts).all() and (m[:front] == c.prior[:front]).all()


@pytest.mark.parametrize("nletters,top", [(4, 3), (24, 64), (256, 9)])
def test_garbage_tables_give_defined_results_inside_the_buffers(swamd, nletters, top):
    rng = np.random.default_rng(3 * nletters + top)
    c = cases.garbage(rng, cases.synthetic(rng, nletters, top))
    for pw, kind in [(1, "none"), (0, "wild")]:
        out, counts, used = check(swamd, c, pw, 0, weights_of(rng, kind, len(cases.QLENS), top))   # (host_leg checks the guard bytes)
    assert not used[0].any()                             # nhits = -5: no entry
    assert used[1:].any() and not used.all()


def test_refusals(swamd):
    rng = np.random.default_rng(5)
    c = cases.synthetic(rng, 4, 3)
    L = swamd.lib()
    nl, nq, top = 4, len(c.qoffs) - 1, 3
    out = np.full(int(c.qoffs[-1]) * nl, 0x55, np.int8)
    cnt = np.full(int(c.qoffs[-1] - c.qoffs[0]) * nl, 0x55555555, np.int32)
    hits, aln, ops = np.ascontiguousarray(c.hits), np.ascontiguousarray(c.aln), np.ascontiguousarray(c.ops)

    def call(**kw):
        a = dict(prior=c.prior.ctypes.data, qoffs=c.qoffs, nq=nq, db=c.packed.ctypes.data, offs=c.offs, scoring=cases.scoring(c), sub=c.sub, pw=1, upd=True,
                 hits=hits.ctypes.data, top=top, aln=aln.ctypes.data, ops=ops.ctypes.data, cap=c.cap, out=out.ctypes.data, cnt=cnt.ctypes.data)
        a.update(kw)
        lt, sc = swamd._pssm_scoring(a["scoring"])
        sub, up = swamd._pssm_update((c.sub, a["pw"], 0))
        if a["sub"] is None:
            up.sub = None
        qo, of = np.ascontiguousarray(a["qoffs"], np.int64), np.ascontiguousarray(a["offs"], np.int64)
        return L.sw_pssm_from_hits_host(a["prior"], qo.ctypes.data, a["nq"], a["db"], of.ctypes.data, len(of) - 1, ctypes.byref(sc) if a["scoring"] else None,
                                        ctypes.byref(up) if a["upd"] else None, a["hits"], None, a["top"], a["aln"], a["ops"], a["cap"], None, a["out"], a["cnt"])

    assert call() == 0
    good_out, good_cnt = out.copy(), cnt.copy()
    lt, other, smax, go, ge = cases.scoring(c)
    bad_q = c.qoffs.copy()
    bad_q[2] = bad_q[1]                                  # an empty query
    bad_t = c.offs.copy()
    bad_t[3] = bad_t[2] - 1                              # offsets that decrease
    for name, kw in {
        "upd": dict(upd=False), "sub": dict(sub=None), "hits": dict(hits=None), "aln": dict(aln=None), "ops": dict(ops=None), "prior": dict(prior=None),
        "ops_cap 0": dict(cap=0), "ops_cap -1": dict(cap=-1), "prior_weight -1": dict(pw=-1), "prior_weight 65536": dict(pw=65536),
        "both outputs": dict(out=None, cnt=None), "top 0": dict(top=0), "top 4097": dict(top=4097),
        "letter twice": dict(scoring=(np.frombuffer(b"ACCA", np.uint8), other, smax, go, ge)), "nletters 0": dict(scoring=(np.zeros(0, np.uint8), other, smax, go, ge)),
        "smax 128": dict(scoring=(lt, other, 128, go, ge)), "other above smax": dict(scoring=(lt, smax + 1, smax, go, ge)),
        "gap_open 1": dict(scoring=(lt, other, smax, 1, ge)), "empty query": dict(qoffs=bad_q), "qoffsets[0] -1": dict(qoffs=c.qoffs - 4),
        "offsets decrease": dict(offs=bad_t), "nqueries -1": dict(nq=-1),
    }.items():
        assert call(**kw) == EINVAL, name
        assert L.sw_last_error().decode(), name
        assert (out == good_out).all() and (cnt == good_cnt).all(), name    # a refusal writes nothing
    assert call(pw=0) == 0 and call(pw=65535) == 0 and call(top=top, cnt=None) == 0 and call(out=None) == 0
    assert call(nq=0) == 0                               # no query: nothing to do


def test_write_pssm_round_trip(swamd, tmp_path):
    rng = np.random.default_rng(9)
    letters = np.frombuffer(b"ARNDCQEGHILKMFPSTWYV*xz", np.uint8)
    m = rng.integers(-128, 128, (37, len(letters))).astype(np.int8)
    m[0, 0], m[0, 1], m[36, -1] = -128, 127, -128
    path = str(tmp_path / "out.pssm")
    swamd.write_pssm(path, letters, m)
    lt, back = swamd.read_pssm(path)
    assert (lt == letters).all() and back.dtype == np.int8 and (back == m).all()
    assert all(line.split()[1] == "X" for line in open(path).read().splitlines()[3:3 + 37])
    cons = rng.choice(np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8), 37)
    swamd.write_pssm(path, letters, m, cons)
    lt, back = swamd.read_pssm(path)
    assert (lt == letters).all() and (back == m).all()
    rows = open(path).read().splitlines()[3:3 + 37]
    assert [r.split()[:2] for r in rows] == [[str(g + 1), chr(cons[g])] for g in range(37)]
    assert all(r.split()[2 + len(letters):] == ["0"] * len(letters) for r in rows)     # the zero percentages
    one = np.array([[-128], [127], [0]], np.int8)                                       # a one-letter alphabet
    swamd.write_pssm(path, b"A", one)
    lt, back = swamd.read_pssm(path)
    assert bytes(lt) == b"A" and (back == one).all()
    # what the reader could not read back is refused, and the file of the last good call stays
    before = open(path).read()
    for bad_letters in (np.arange(256, dtype=np.uint8), b"AC-", b"ACA", b"A1", b""):
        n = max(1, len(bad_letters))
        with pytest.raises(swamd.SwError):
            swamd.write_pssm(path, bad_letters, np.zeros((2, n), np.int8))
    with pytest.raises(swamd.SwError):
        swamd.write_pssm(path, b"AC", np.zeros((0, 2), np.int8))
    with pytest.raises(swamd.SwError):
        swamd.write_pssm(path, b"AC", np.zeros((2, 2), np.int8), b"A ")
    with pytest.raises(swamd.SwError):
        swamd.write_pssm(str(tmp_path / "no_such_dir" / "x.pssm"), b"AC", np.zeros((2, 2), np.int8))
    assert open(path).read() == before


def test_host_leg_and_writer_are_clean_under_the_sanitizers(tmp_path):
    """tests/pssm_hits_driver.cpp, a program of its own, with the sources that hold the host leg and the writer, all under
    -fsanitize=address,undefined: garbage tables in heap blocks of exactly their sizes.  A clean exit is the test."""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the driver")
    exe = str(tmp_path / "pssm_hits_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "pssm_hits_driver.cpp"), os.path.join(ROOT, "smith-waterman_amd", "csrc", "sw_hits_host.cpp"),
                    os.path.join(ROOT, "smith-waterman_amd", "csrc", "sw_pssm_read.cpp")], check=True)
    r = subprocess.run([exe, str(tmp_path / "driver.pssm")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "" and r.stdout.startswith("ok "), (r.returncode, r.stdout, r.stderr)
