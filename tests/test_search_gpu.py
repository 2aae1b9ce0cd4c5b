"""GPU: database search (sw_search_device / Engine.search / smithW --search) -- one query against many targets of any length;
every target's (max_score, max_pos) against the oracle's streaming fill of (query, target)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle_lib import ROOT

pytestmark = pytest.mark.gpu

DNA = np.frombuffer(b"ACGT", np.uint8)
PROTEIN = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWYBZX*", np.uint8)
ALL_BYTES = np.arange(256, dtype=np.uint8)
SCORINGS = [(3, -3, -2), (5, -3, -4), (1, 1, 0), (2, 0, -1)]
QLENS = [1, 7, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049, 5000]


def _alphabets(i):
    """(query alphabet, target alphabet): DNA, protein, every byte value (0 included), target letters absent from the query."""
    return [(DNA, DNA), (PROTEIN, PROTEIN), (ALL_BYTES, ALL_BYTES), (DNA, PROTEIN)][i % 4]


def _database(rng, qlen, alpha, budget=3e7):
    lens = [0, 1, 63, 64, 65, 0]
    n_rand = int(np.clip(budget / (qlen * 1500), 4, 194))
    lens += list(rng.integers(2, 3001, n_rand))
    rng.shuffle(lens)
    front = 7                                                  # offsets[0] > 0 and odd: no alignment anywhere
    offs = np.zeros(len(lens) + 1, np.int64)
    offs[0] = front
    offs[1:] = front + np.cumsum(lens)
    packed = rng.choice(alpha, int(offs[-1])).astype(np.uint8)
    return packed, offs


def _check_against_oracle(oracle, query, packed, offs, scores, res):
    assert res.shape == (len(offs) - 1, 3)
    for k in range(len(offs) - 1):
        t = packed[offs[k]:offs[k + 1]]
        if len(t) == 0:
            assert tuple(res[k]) == (0, 0, 0), f"empty target {k}"
            continue
        o = oracle.fill_streaming(query, t, scores)
        assert (res[k, 1], res[k, 0]) == (o["max_score"], o["max_pos"]), f"target {k} (len {len(t)}): {tuple(res[k])} vs {o['max_score'], o['max_pos']}"
        assert res[k, 2] == 0


@pytest.mark.parametrize("i,qlen", list(enumerate(QLENS)))
def test_search_matches_oracle(engine, oracle, swamd, i, qlen):
    rng = np.random.default_rng(1000 + qlen)
    qa, ta = _alphabets(i)
    scores = SCORINGS[i % len(SCORINGS)]
    query = rng.choice(qa, qlen).astype(np.uint8)
    packed, offs = _database(rng, qlen, ta)
    res = engine.search(query, (packed, offs), scores)
    _check_against_oracle(oracle, query, packed, offs, scores, res)


@pytest.mark.parametrize("qlen", [100, 700, 2100])
def test_search_scores_near_the_limit(engine, oracle, qlen):
    rng = np.random.default_rng(qlen)
    query = rng.choice(DNA, qlen).astype(np.uint8)
    packed, offs = _database(rng, qlen, DNA, budget=5e6)
    lo = min(qlen, int(np.diff(offs).max()))
    match = (1 << 24) // lo - 1                                # match * min(cols, rows) just below 2^24: far beyond a byte
    scores = (match, -match // 3, -match // 5)
    res = engine.search(query, (packed, offs), scores)
    _check_against_oracle(oracle, query, packed, offs, scores, res)
    assert res[:, 1].max() > 127


def test_search_ties_pin_the_lowest_index(engine, oracle):
    query = np.frombuffer(b"ACGT" * 150, np.uint8)             # periodic: the maximum is reached at many cells
    targets = [b"ACGT" * n for n in (1, 2, 16, 17, 100, 200)] + [b"CGTA" * 40, b"GTAC" * 300, b"ACG" * 90]
    for scores in [(3, -3, -2), (1, 1, 0), (2, 0, -1)]:
        res = engine.search(query, targets, scores)
        _check_against_oracle(oracle, query, *swamd_pack(targets), scores, res)
    # all-mismatch targets: no positive cell
    res = engine.search(b"A" * 300, [b"C" * 10, b"G" * 1000, b"T" * 64], (3, -3, -2))
    assert np.array_equal(res, np.zeros((3, 3), np.int64))


def swamd_pack(targets):
    import importlib
    return importlib.import_module("smith-waterman_amd")._pack_targets(targets)


def test_search_load_balance_long_target_among_short(engine, oracle):
    rng = np.random.default_rng(7)
    lens = list(rng.integers(1, 100, 5000))
    lens.insert(1234, 200_000)
    offs = np.zeros(len(lens) + 1, np.int64)
    offs[1:] = np.cumsum(lens)
    packed = rng.choice(DNA, int(offs[-1])).astype(np.uint8)
    query = rng.choice(DNA, 1000).astype(np.uint8)
    res = engine.search(query, (packed, offs), (3, -3, -2))
    _check_against_oracle(oracle, query, packed, offs, (3, -3, -2), res)


def test_search_results_in_input_order(engine, swamd):
    # the same targets in two orders: the results follow the targets
    rng = np.random.default_rng(3)
    targets = [rng.choice(PROTEIN, int(n)).astype(np.uint8) for n in rng.integers(0, 900, 300)]
    query = rng.choice(PROTEIN, 400).astype(np.uint8)
    res = engine.search(query, targets)
    perm = rng.permutation(len(targets))
    res2 = engine.search(query, [targets[p] for p in perm])
    assert np.array_equal(res2, res[perm])


@pytest.mark.parametrize("npairs,n", [(20000, 256), (2000, 1024)])
def test_search_equals_batch_on_equal_lengths(engine, npairs, n):
    rng = np.random.default_rng(n)
    query = rng.choice(DNA, n).astype(np.uint8)
    b_all = rng.choice(DNA, (npairs, n)).astype(np.uint8)
    res_b, _, _ = engine.batch(np.broadcast_to(query, (npairs, n)), b_all, store=False)
    offs = np.arange(npairs + 1, dtype=np.int64) * n
    res_s = engine.search(query, (b_all.reshape(-1), offs))
    assert np.array_equal(res_s, res_b.cpu().numpy())


def test_search_repeated_calls_reuse_workspaces(engine, oracle):
    rng = np.random.default_rng(11)
    packed, offs = _database(rng, 300, PROTEIN, budget=3e6)
    q1 = rng.choice(PROTEIN, 300).astype(np.uint8)
    q2 = rng.choice(PROTEIN, 2500).astype(np.uint8)
    r1 = engine.search(q1, (packed, offs))
    r2 = engine.search(q2, (packed, offs))
    _check_against_oracle(oracle, q2, packed, offs, (3, -3, -2), r2)
    assert np.array_equal(engine.search(q1, (packed, offs)), r1)
    assert np.array_equal(engine.search(q2, (packed, offs)), r2)
    _check_against_oracle(oracle, q1, packed, offs, (3, -3, -2), r1)


def test_search_rejects_bad_input(engine, swamd):
    import torch
    L = swamd.lib()
    dq = torch.zeros(64, dtype=torch.uint8, device="cuda")
    ddb = torch.zeros(256, dtype=torch.uint8, device="cuda")
    dres = torch.zeros((8, 3), dtype=torch.int64, device="cuda")
    sc = swamd._Scores(3, -3, -2)

    def call(qlen=10, offs=(0, 5, 9), scores=sc, q=dq.data_ptr(), db=ddb.data_ptr(), res=dres.data_ptr(), n=None, offs_ptr=True):
        o = np.array(offs, np.int64)
        return L.sw_search_device(engine._h, q, qlen, db, o.ctypes.data if offs_ptr else None, len(o) - 1 if n is None else n,
                                  ctypes.byref(scores), res, None)

    assert call() == 0
    engine.synchronize()
    assert call(offs=(0, 5, 4)) == -22 and b"decrease" in L.sw_last_error()
    assert call(qlen=0) == -22
    assert call(qlen=1 << 20) == -22
    assert call(offs=(0, 1 << 20)) == -22
    assert call(scores=swamd._Scores(3, -3, 1)) == -22                 # gap > 0
    assert call(scores=swamd._Scores(1 << 22, -3, -2), qlen=10, offs=(0, 64)) == -22   # match * min(dims) beyond 2^24
    assert call(q=None) == -22
    assert call(db=None) == -22
    assert call(res=None) == -22
    assert call(offs_ptr=False) == -22
    assert call(n=-1) == -22


def test_search_top_k_order(engine):
    query = b"ACGTACGTTTGACCA"
    targets = [b"A", b"ACGTACGTTTGACCA", b"", b"GG", b"ACGTACGT", b"ACGTACGTTTGACCA", b"TTGACCA"]
    res, top = engine.search(query, targets, top=4)
    assert list(top) == [1, 5, 4, 6]
    assert list(res[top, 1]) == sorted(res[:, 1], reverse=True)[:4]
    _, top = engine.search(query, targets, top=100)
    assert len(top) == len(targets)


def test_cli_search_matches_oracle(swamd, oracle, tmp_path):
    rng = np.random.default_rng(5)
    q = rng.choice(PROTEIN, 300).astype(np.uint8)
    recs = [rng.choice(PROTEIN, int(n)).astype(np.uint8) for n in rng.integers(0, 700, 40)]
    recs[7] = np.concatenate([recs[7], q[50:200]]) if len(recs[7]) else q[50:200]
    qf, dbf = tmp_path / "q.fa", tmp_path / "db.fa"
    qf.write_bytes(b">decoy\nAAAA\n>query\n" + bytes(q) + b"\n")
    dbf.write_bytes(b"".join(b">t%d\n" % k + bytes(r) + b"\n" for k, r in enumerate(recs)))
    exe = os.path.join(ROOT, "smith-waterman_amd", "smithW")
    out = subprocess.run([exe, "--search", str(qf), str(dbf), "--record-a", "1", "--top", "12", "--scores", "5", "-3", "-4"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert lines[0].startswith("#")
    hits = [tuple(int(x) for x in ln.split("\t")) for ln in lines[1:13]]
    assert any(ln.startswith("Elapsed time") for ln in lines)
    expect = []
    for k, r in enumerate(recs):
        o = oracle.fill_streaming(q, r, (5, -3, -4)) if len(r) else {"max_score": 0, "max_pos": 0}
        expect.append((k, o["max_score"], o["max_pos"]))
    expect.sort(key=lambda e: (-e[1], e[0]))
    for rank, (hit, e) in enumerate(zip(hits, expect[:12])):
        k, score, mp = e
        assert hit == (rank + 1, k, score, mp // 301, mp % 301)
    assert hits[0][1] == 7
