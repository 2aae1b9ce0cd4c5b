"""CPU: the host legs of the PSSM calls (sw_search_pssm_multi_host, sw_align_pssm_hits_host) against the independent checker, the bridge
from sequence queries (sw_pssm_from_queries), the clamp, `other`, the argument errors the device calls share with them, and the reader of
PSI-BLAST's ASCII PSSM (sw_read_pssm) -- also under the address and undefined-behaviour sanitizers, in a stand-alone program."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import align_cases
import pssm_cases
from affine_cases import GAPS, PROTEIN, ROOT, assert_same, checker, random_submat  # noqa: F401

EINVAL = -22


@pytest.fixture(scope="module")
def case():
    """The shapes of the GPU tests: every query length of one call against the database of the affine tests."""
    rng = np.random.default_rng(2024)
    packed, offs = pssm_cases.small_database(rng, PROTEIN)
    return rng, packed, offs


@pytest.mark.parametrize("nletters", pssm_cases.NLETTERS)
def test_search_host_equals_the_checker(swamd, checker, case, nletters):  # noqa: F811
    rng, packed, offs = case
    go, ge = GAPS[pssm_cases.NLETTERS.index(nletters) % len(GAPS)]
    ty = pssm_cases.Typed(rng, pssm_cases.letters_of(rng, nletters), -3, 9, pssm_cases.QLENS)
    res = swamd.search_pssm_multi_host((ty.matrix, ty.qoffs), (packed, offs), ty.scoring(go, ge))
    exp = ty.expected(checker, packed, offs, go, ge)
    assert res.shape == exp.shape
    for q in range(len(exp)):
        assert_same(res[q], exp[q], f"nletters {nletters}, query {q} of {len(ty.query(q))} columns")
    assert (res[:, np.diff(offs) == 0, :] == 0).all()


def test_from_queries_reproduces_the_sequence_search(swamd):
    rng = np.random.default_rng(5)
    qlens = [1, 40, 7, 130, 64]
    qoffs = np.concatenate([[5], 5 + np.cumsum(qlens)]).astype(np.int64)
    qpacked = rng.choice(PROTEIN, int(qoffs[-1])).astype(np.uint8)
    tlens = [0, 1, 63, 64, 65, 0, 127, 300, 1, 90]
    offs = np.concatenate([[3], 3 + np.cumsum(tlens)]).astype(np.int64)
    packed = rng.choice(PROTEIN, int(offs[-1])).astype(np.uint8)
    sub = random_submat(rng)
    for go, ge in GAPS[:2]:
        exp = swamd.search_affine_multi_host((qpacked, qoffs), (packed, offs), (sub, go, ge))
        m, moffs = swamd.pssm_from_queries((qpacked, qoffs), sub, PROTEIN)
        assert m.shape == (sum(qlens), len(PROTEIN)) and moffs[0] == 0
        assert (m[0] == sub[qpacked[5], PROTEIN]).all()
        res = swamd.search_pssm_multi_host((m, moffs), (packed, offs), (PROTEIN, -128, 127, go, ge))
        assert (res == exp).all()
        hits = np.argsort(-exp[:, :, 1], axis=1, kind="stable")[:, :4]
        a0, o0 = swamd.align_affine_hits_host((qpacked, qoffs), (packed, offs), (sub, go, ge), hits)
        a1, o1 = swamd.align_pssm_hits_host((m, moffs), (packed, offs), (PROTEIN, -128, 127, go, ge), hits)
        assert (a0 == a1).all() and o0 == o1


def test_clamp_entries_of_100_with_smax_7(swamd, checker):  # noqa: F811
    rng = np.random.default_rng(6)
    packed, offs = align_cases.pack([rng.choice(PROTEIN, n).astype(np.uint8) for n in (50, 0, 200, 77)])
    ty = pssm_cases.Typed(rng, PROTEIN, -5, 7, [90, 300], lo=-6, hi=6)
    ty.types[rng.random(ty.types.shape) < 0.2] = 100
    ty.table[:, ty.letters] = np.minimum(ty.types, 7)              # the clamped table
    assert (ty.matrix == 100).any() and ty.table.max() == 7
    res = swamd.search_pssm_multi_host((ty.matrix, ty.qoffs), (packed, offs), ty.scoring(-4, -1))
    assert (res == ty.expected(checker, packed, offs, -4, -1)).all()
    unclamped = swamd.search_pssm_multi_host((ty.matrix, ty.qoffs), (packed, offs), (ty.letters, -5, 127, -4, -1))
    assert (unclamped[:, :, 1] > res[:, :, 1]).any()               # the clamp is what made the difference


def test_other_scores_the_bytes_that_are_not_listed(swamd, checker):  # noqa: F811
    rng = np.random.default_rng(7)
    letters = PROTEIN[:4]
    packed, offs = align_cases.pack([rng.choice(PROTEIN, n).astype(np.uint8) for n in (64, 130, 1)])   # mostly unlisted bytes
    for other in (-128, -2, 3):
        ty = pssm_cases.Typed(rng, letters, other, 5, [70, 20])
        res = swamd.search_pssm_multi_host((ty.matrix, ty.qoffs), (packed, offs), ty.scoring(-3, -2))
        assert (res == ty.expected(checker, packed, offs, -3, -2)).all(), other
    # a positive `other`: a target of unlisted bytes alone aligns end to end
    ty = pssm_cases.Typed(rng, letters, 3, 5, [10])
    res = swamd.search_pssm_multi_host((ty.matrix, ty.qoffs), [b"WWWWWWWWWWWW"], ty.scoring(-3, -2))
    assert res[0, 0, 1] == 30


@pytest.mark.parametrize("go,ge", [(-10, -1), (0, 0)])
def test_align_host_equals_the_walk_of_the_checker(swamd, checker, go, ge):  # noqa: F811
    rng = np.random.default_rng(8)
    targets = [rng.choice(PROTEIN, n).astype(np.uint8) for n in (120, 0, 64, 300, 1)]
    packed, offs = align_cases.pack(targets)
    ty = pssm_cases.Typed(rng, PROTEIN, -4, 8, [1, 65, 257])
    hits = np.array([[0, 3, 1, 7], [3, 2, 0, 4], [4, 3, 3, -1]], np.int64)
    nhits = np.array([4, 3, 4], np.int64)
    aln, ops = swamd.align_pssm_hits_host((ty.matrix, ty.qoffs), (packed, offs), ty.scoring(go, ge), hits, nhits)
    for q in range(3):
        for r in range(4):
            k = int(hits[q, r])
            if r >= nhits[q] or not 0 <= k < len(targets):
                assert (aln[q, r] == 0).all() and ops[q][r] == b""
                continue
            row, exp_ops, _ = align_cases.expected(checker, ty.query(q), targets[k], ty.table, go, ge)
            assert tuple(aln[q, r]) == row and ops[q][r] == exp_ops, (q, r)
            align_cases.replay(ty.query(q), targets[k], ty.table, go, ge, aln[q, r], ops[q][r])


def test_format_alignment_takes_a_consensus(swamd):
    top, mid, bot = swamd.format_alignment("MKV", b"AMKAV", (0, 0, 0, 1, 3, 5, 4), b"MMDM")
    assert (top, mid, bot) == ("MK-V", "|| |", "MKAV")


def _call(swamd, fn, qoffs, nq, scoring, offs=(0, 4), null=None, top=2):
    """A host leg on 64 columns and a 4-letter database, every output poisoned; `null` names an argument passed as NULL."""
    L = swamd.lib()
    lt, sc = swamd._pssm_scoring(scoring)
    m, db = np.full((64, max(1, len(lt))), 2, np.int8), np.full(8, 65, np.uint8)
    qoffs, offs = np.asarray(qoffs, np.int64), np.asarray(offs, np.int64)
    res = np.full((max(1, nq) * max(1, len(offs) - 1), 3), -7, np.int64)
    hits = np.zeros((max(1, nq) * top, 3), np.int64)
    aln, ops = np.full((max(1, nq) * top, 7), -7, np.int64), np.full((max(1, nq) * top, 16), 0x5A, np.uint8)
    a = {"pssm": m.ctypes.data, "qoffsets": qoffs.ctypes.data, "db": db.ctypes.data, "offsets": offs.ctypes.data, "scoring": ctypes.byref(sc),
         "results": res.ctypes.data, "hits": hits.ctypes.data, "aln": aln.ctypes.data}
    if null == "letters":
        sc.letters = None
    elif null:
        a[null] = None
    if fn == "search":
        rc = L.sw_search_pssm_multi_host(a["pssm"], a["qoffsets"], nq, a["db"], a["offsets"], len(offs) - 1, a["scoring"], a["results"])
        outs = [res]
    else:
        rc = L.sw_align_pssm_hits_host(a["pssm"], a["qoffsets"], nq, a["db"], a["offsets"], len(offs) - 1, a["scoring"], a["hits"], None, top, a["aln"],
                                       ops.ctypes.data, 16)
        outs = [aln, ops]
    return rc, outs, L.sw_last_error().decode()


@pytest.mark.parametrize("fn", ["search", "align"])
def test_einval_list_leaves_the_outputs_untouched(swamd, fn):
    good = (b"ACGT", -2, 5, -2, -1)
    rc, outs, _ = _call(swamd, fn, [0, 4, 10], 2, good)
    assert rc == 0 and (outs[0][:, 1] == 8).all()                  # 4 x entry 2 against AAAA
    nulls = ["pssm", "qoffsets", "db", "offsets", "scoring", "letters"] + (["results"] if fn == "search" else ["hits", "aln"])
    for null in nulls:
        rc, outs, msg = _call(swamd, fn, [0, 4, 10], 2, good, null=null)
        assert rc == EINVAL, null
        assert (outs[0] == -7).all(), null
    bad = [
        ([0, 4, 10], -1, good, "negative query count"),
        ([0, 10, 4], 2, good, "decrease"),
        ([-1, 4, 10], 2, good, "negative"),
        ([0, 4, 4], 2, good, "length 0"),
        ([0, 4, 4 + (1 << 20)], 2, good, "length 1048576"),
        ([0, 4, 10], 2, (b"", -2, 5, -2, -1), "nletters = 0"),
        ([0, 4, 10], 2, (bytes(range(256)) + b"A", -2, 5, -2, -1), "nletters = 257"),
        ([0, 4, 10], 2, (b"ACGA", -2, 5, -2, -1), "listed twice"),
        ([0, 4, 10], 2, (b"ACGT", -2, -1, -2, -1), "smax = -1"),
        ([0, 4, 10], 2, (b"ACGT", -2, 128, -2, -1), "smax = 128"),
        ([0, 4, 10], 2, (b"ACGT", -129, 5, -2, -1), "other = -129"),
        ([0, 4, 10], 2, (b"ACGT", 6, 5, -2, -1), "other = 6"),
        ([0, 4, 10], 2, (b"ACGT", -2, 5, 1, -1), "gap_open"),
        ([0, 4, 10], 2, (b"ACGT", -2, 5, -2, 1), "gap_extend"),
        ([0, 4, 10], 2, (b"ACGT", -2, 5, -(1 << 24), -1), "2^24"),
    ]
    who = "sw_search_pssm_multi_host" if fn == "search" else "sw_align_pssm_hits_host"
    for qoffs, nq, scoring, word in bad:
        rc, outs, msg = _call(swamd, fn, qoffs, nq, scoring)
        assert rc == EINVAL and word in msg and who in msg, (qoffs, nq, scoring[1:], msg)
        assert (outs[0] == -7).all() and (fn == "search" or (outs[1] == 0x5A).all()), msg
    assert _call(swamd, fn, [0, 4, 10], 2, good, offs=(0, 4, 2))[0] == EINVAL       # the offsets errors of sw_search_device
    assert _call(swamd, fn, [0, 4, 10], 2, good, offs=(-1, 4))[0] == EINVAL
    if fn == "align":
        assert _call(swamd, fn, [0, 4, 10], 2, good, top=0)[0] == EINVAL
        assert _call(swamd, fn, [0, 4, 10], 2, good, top=swamd.SW_TOP_MAX + 1)[0] == EINVAL


def test_score_bound_is_smax_times_the_shorter_side(swamd):
    """smax x min(longest query, longest target) < 2^24, from both sides: 132 200 columns against 132 200 letters pass at 126, not at 127."""
    L = swamd.lib()
    n = 132200
    assert 126 * n < (1 << 24) <= 127 * n
    m, db = np.zeros((n + 8, 1), np.int8), np.full(n, 65, np.uint8)
    offs = np.array([0, n], np.int64)
    res = np.full((2, 3), -7, np.int64)

    def call(smax, qoffs, t=1):
        lt, sc = swamd._pssm_scoring((b"A", -1, smax, -2, -1))
        return L.sw_search_pssm_multi_host(m.ctypes.data, np.asarray(qoffs, np.int64).ctypes.data, 2, db.ctypes.data, offs.ctypes.data, t, ctypes.byref(sc),
                                           res.ctypes.data)

    assert call(127, [0, 4, 4 + n]) == EINVAL and "2^24" in L.sw_last_error().decode() and (res == -7).all()
    offs[1] = 100                                                  # a short longest target: min(...) is small again
    assert call(127, [0, 4, 4 + n], t=1) == 0 and res[1, 1] == 0   # (all-zero entries: nothing aligns)
    offs[1] = n
    assert call(127, [0, 4, 8]) == 0                               # short queries against the long target


def test_device_entry_points_refuse_null_without_a_device(swamd):
    L = swamd.lib()
    assert L.sw_db_search_pssm(None, None, None, None, 0, None, None, None) == EINVAL
    assert L.sw_db_search_pssm_top(None, None, None, None, 0, None, 1, 0, None, None, None) == EINVAL
    assert L.sw_db_align_pssm_hits(None, None, None, None, 0, None, None, None, 1, None, None, 0, None) == EINVAL


# ---- sw_read_pssm

def _files(tmp_path):
    """A well-formed file and the malformed ones: name -> (path, the word its error message holds, or None)."""
    rng = np.random.default_rng(9)
    letters = PROTEIN[:20]
    m = rng.integers(-9, 12, (37, 20)).astype(np.int8)
    m[3, 5], m[4, 6] = -128, 127
    cons = rng.choice(letters, 37).astype(np.uint8)
    good = tmp_path / "good.pssm"
    pssm_cases.write_ascii_pssm(good, letters, m, cons)
    text = good.read_text().split("\n")
    files = {"good": (good, None)}

    def variant(name, lines, word):
        p = tmp_path / f"{name}.pssm"
        p.write_text("\n".join(lines) + "\n")
        files[name] = (p, word)

    row = text[5].split()
    variant("truncated_row", text[:5] + [" ".join(row[:12])] + text[6:], "needs a position")
    variant("entry_128", text[:5] + [" ".join(row[:4] + ["128"] + row[5:])] + text[6:], "does not fit int8")
    variant("not_an_integer", text[:5] + [" ".join(row[:4] + ["4x"] + row[5:])] + text[6:], "not an integer")
    variant("no_header", text[:2] + text[3:], "no header")
    variant("letter_twice", text[:2] + ["   A R N R D   A R N R D"] + text[3:], "listed twice")
    variant("no_column", text[:3], "no column")
    variant("empty", [], "no header")
    (tmp_path / "empty.pssm").write_bytes(b"")
    variant("last_line_unterminated", text[:10], None)
    (tmp_path / "last_line_unterminated.pssm").write_bytes("\n".join(text[:10]).encode())
    files["good_crlf"] = (tmp_path / "good_crlf.pssm", None)      # CRLF line ends: the same table, not its first column
    files["good_crlf"][0].write_bytes(good.read_bytes().replace(b"\n", b"\r\n"))
    return files, letters, m


def test_read_pssm(swamd, tmp_path):
    files, letters, m = _files(tmp_path)
    lt, got = swamd.read_pssm(str(files["good"][0]))
    assert (lt == letters).all() and got.dtype == np.int8 and (got == m).all()
    lt, got = swamd.read_pssm(str(files["good_crlf"][0]))
    assert b"\r\n" in files["good_crlf"][0].read_bytes() and (lt == letters).all() and got.shape == m.shape and (got == m).all()
    lt, got = swamd.read_pssm(str(files["last_line_unterminated"][0]))
    assert (lt == letters).all() and (got == m[:7]).all()
    for name, (path, word) in files.items():
        if word is None:
            continue
        with pytest.raises(swamd.SwError) as e:
            swamd.read_pssm(str(path))
        assert e.value.code == EINVAL and word in str(e.value), (name, str(e.value))
    with pytest.raises(swamd.SwError):
        swamd.read_pssm(str(tmp_path / "missing.pssm"))
    # a cap too small: SW_EINVAL, and not one byte written
    L = swamd.lib()
    lo = np.zeros(256, np.uint8)
    nl, nc = ctypes.c_int32(-7), ctypes.c_int64(-7)
    buf = np.full(m.size, 0x5A, np.uint8)
    rc = L.sw_read_pssm(os.fsencode(str(files["good"][0])), lo.ctypes.data, ctypes.byref(nl), buf.ctypes.data, m.size - 1, ctypes.byref(nc))
    assert rc == EINVAL and "too small" in L.sw_last_error().decode() and (buf == 0x5A).all() and nl.value == -7 and nc.value == -7
    assert L.sw_read_pssm(None, lo.ctypes.data, ctypes.byref(nl), None, 0, ctypes.byref(nc)) == EINVAL


def test_read_pssm_is_clean_under_the_sanitizers(tmp_path):
    """tests/pssm_read_driver.cpp, a program of its own, with the source that holds the reader, both under -fsanitize=address,undefined:
    every file above through both calls of the two-call pattern, with buffers of exactly the size asked for.  A clean exit is the test."""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the reader's driver")
    files, letters, m = _files(tmp_path)
    exe = str(tmp_path / "pssm_read_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "pssm_read_driver.cpp"), os.path.join(ROOT, "smith-waterman_amd", "csrc", "sw_pssm_read.cpp")], check=True)
    for name, (path, word) in files.items():
        r = subprocess.run([exe, str(path)], capture_output=True, text=True)
        assert r.returncode == (0 if word is None else 3), (name, r.returncode, r.stdout, r.stderr)
        assert r.stderr == "", (name, r.stderr)
        if word is None:
            n = 37 if name.startswith("good") else 7
            assert r.stdout.split()[:3] == ["20", str(n), str(int(m[:n].astype(np.int64).sum()))], (name, r.stdout)
        else:
            assert word in r.stdout, (name, r.stdout)
