"""Shared by the affine-search tests (test_search_affine_host.py, test_search_affine_gpu.py): the independent checker
(tests/affine_oracle.cpp, built with g++ and loaded through ctypes), random tables and the databases of the linear search tests."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DNA = np.frombuffer(b"ACGT", np.uint8)
PROTEIN = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWYBZX*", np.uint8)
ALL_BYTES = np.arange(256, dtype=np.uint8)
# (gap_open, gap_extend): the usual protein pair, a dear opening, and the degenerate corners (0, ge), (go, 0), (0, 0)
GAPS = [(-10, -1), (-3, -2), (0, -2), (-4, 0), (0, 0)]


class Checker:
    def __init__(self, so):
        L = ctypes.CDLL(so)
        vp, i64 = ctypes.c_void_p, ctypes.c_int64
        L.affine_oracle_pair.argtypes = [vp, i64, vp, i64, vp, i64, i64, ctypes.POINTER(i64), ctypes.POINTER(i64), vp, vp, vp]
        L.affine_oracle_search.argtypes = [vp, i64, vp, vp, i64, vp, i64, i64, vp]
        self.L = L

    def search(self, query, packed, offs, submat, go, ge):
        """(ntargets, 3) int64: max_pos, max_score, 0 per target."""
        q = np.ascontiguousarray(query, np.uint8)
        db = np.ascontiguousarray(packed, np.uint8) if len(packed) else np.zeros(1, np.uint8)
        offs = np.ascontiguousarray(offs, np.int64)
        sub = np.ascontiguousarray(submat, np.int8)
        assert sub.shape == (256, 256)
        res = np.zeros((len(offs) - 1, 3), np.int64)
        self.L.affine_oracle_search(q.ctypes.data, len(q), db.ctypes.data, offs.ctypes.data, len(offs) - 1, sub.ctypes.data, go, ge, res.ctypes.data)
        return res

    def matrices(self, query, target, submat, go, ge):
        """max_score, max_pos and the whole H, E, F of one pair ((len + 1) x (qlen + 1) int64)."""
        q = np.ascontiguousarray(query, np.uint8)
        t = np.ascontiguousarray(target, np.uint8)
        sub = np.ascontiguousarray(submat, np.int8)
        shape = (len(t) + 1, len(q) + 1)
        H, E, F = (np.zeros(shape, np.int64) for _ in range(3))
        s, p = ctypes.c_int64(), ctypes.c_int64()
        self.L.affine_oracle_pair(q.ctypes.data, len(q), t.ctypes.data, len(t), sub.ctypes.data, go, ge, ctypes.byref(s), ctypes.byref(p),
                                  H.ctypes.data, E.ctypes.data, F.ctypes.data)
        return int(s.value), int(p.value), H, E, F


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the affine checker")
    so = str(tmp_path_factory.mktemp("affine") / "libaffine_oracle.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "affine_oracle.cpp")],
                   check=True)
    return Checker(so)


def random_submat(rng, lo=-8, hi=12):
    """A random ASYMMETRIC table over all 256 x 256 byte pairs, the diagonal lifted so that alignments grow."""
    s = rng.integers(lo, hi + 1, (256, 256)).astype(np.int8)
    d = np.arange(256)
    s[d, d] = rng.integers(4, hi + 1, 256).astype(np.int8)
    return s


def alphabets(i):
    """(query alphabet, target alphabet) of tests/test_search_gpu.py: DNA, protein, every byte value, target letters absent from the query."""
    return [(DNA, DNA), (PROTEIN, PROTEIN), (ALL_BYTES, ALL_BYTES), (DNA, PROTEIN)][i % 4]


def database(rng, qlen, alpha, budget=3e7):
    """The database of tests/test_search_gpu.py: empty, 1-letter and lane-edge targets among random lengths, an odd offsets[0]."""
    lens = [0, 1, 63, 64, 65, 0]
    n_rand = int(np.clip(budget / (qlen * 1500), 4, 194))
    lens += list(rng.integers(2, 3001, n_rand))
    rng.shuffle(lens)
    front = 7
    offs = np.zeros(len(lens) + 1, np.int64)
    offs[0] = front
    offs[1:] = front + np.cumsum(lens)
    packed = rng.choice(alpha, int(offs[-1])).astype(np.uint8)
    return packed, offs


def assert_same(res, exp, what=""):
    res, exp = np.asarray(res), np.asarray(exp)
    assert res.shape == exp.shape, f"{what}: shape {res.shape} vs {exp.shape}"
    bad = np.nonzero((res != exp).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} targets differ, first {bad[0]}: {tuple(res[bad[0]])} vs {tuple(exp[bad[0]])}"
