"""GPU: checkpointed alignment ("align_checkpoint", csrc/sw_align_ckpt.hip) against the whole-matrix path on the same engine (aln and
ops bit for bit), the walk of the canonical alignment over the independent checker's matrices, and the host leg.  Bands of 64 rows
("align_checkpoint_rows") put a checkpoint row every 64 target letters, so that a few hundred letters cross several of them."""
import numpy as np
import pytest

from affine_cases import GAPS, PROTEIN, alphabets, checker, random_submat  # noqa: F401
from align_cases import _crisp_submat, expected, indel_cases, pack, replay

pytestmark = pytest.mark.gpu

QLENS = [1, 63, 65, 256, 257, 513, 1025, 2049]
SEAMS = [0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257]


@pytest.fixture()
def eng(swamd):
    """An engine of its own (the options it sets stay with it), bands of 64 rows."""
    e = swamd.Engine(0)
    e.set_option("align_checkpoint_rows", 64)
    yield e
    e.close()


def assert_exact(checker, query, targets, sub, go, ge, hits, aln, ops, what=""):  # noqa: F811
    assert aln.shape == (len(hits), 7) and len(ops) == len(hits)
    memo = {}
    for h, k in enumerate(hits):
        if k not in memo:
            memo[k] = expected(checker, query, targets[k], sub, go, ge)
        row, eops, _ = memo[k]
        assert tuple(int(x) for x in aln[h]) == row, f"{what} hit {h} (target {k}, len {len(targets[k])}): {tuple(aln[h])} vs {row}"
        assert ops[h] == eops, f"{what} hit {h} (target {k}, len {len(targets[k])}): ops differ"
        replay(query, targets[k], sub, go, ge, aln[h], ops[h])


def both_modes(eng, query, targets, sub, go, ge, hits, rows=64):
    """Mode 1, then mode 0 on the same engine; asserts that they agree bit for bit and returns mode 1's (aln, ops)."""
    aln, ops = eng.align_affine(query, targets, sub, go, ge, hits, checkpoint=1)
    assert eng.get_option("last_align_affine_checkpointed") == 1 and eng.get_option("last_align_affine_band_rows") == rows
    assert eng.get_option("align_checkpoint") == 0                       # the keyword holds for its call alone
    ref_aln, ref_ops = eng.align_affine(query, targets, sub, go, ge, hits, checkpoint=0)
    assert eng.get_option("last_align_affine_checkpointed") == 0 and eng.get_option("last_align_affine_band_rows") == 0
    bad = np.nonzero((aln != ref_aln).any(axis=1))[0]
    assert len(bad) == 0, f"{len(bad)} rows differ from the whole-matrix path, first {bad[0]}: {tuple(aln[bad[0]])} vs {tuple(ref_aln[bad[0]])}"
    assert ops == ref_ops
    return aln, ops


@pytest.mark.parametrize("i,qlen", list(enumerate(QLENS)))
def test_the_rule_at_every_seam(eng, checker, swamd, i, qlen):  # noqa: F811
    rng = np.random.default_rng(4100 + qlen)
    qa, ta = alphabets(i)
    go, ge = GAPS[i % len(GAPS)]
    query = rng.choice(qa, qlen).astype(np.uint8)
    lens = SEAMS + list(rng.integers(2, 701, 12))
    targets = [rng.choice(ta, n).astype(np.uint8) for n in lens]
    targets = [targets[k] for k in rng.permutation(len(targets))]
    packed, offs = pack(targets)
    sub = random_submat(rng)
    hits = list(range(len(targets)))
    aln, ops = both_modes(eng, query, (packed, offs), sub, go, ge, hits)
    assert_exact(checker, query, targets, sub, go, ge, hits, aln, ops, f"qlen {qlen} gaps {go, ge}")
    haln, hops = swamd.align_affine_host(query, (packed, offs), sub, go, ge, hits)
    assert np.array_equal(aln, haln) and ops == hops


def planted(swamd, rng):
    """Alignments built around the checkpoint rows 64 and 128 of a 300-letter query's hits: a prefix of foreign letters shifts the piece
    so that the named event falls on target row R - 1, R, R + 1, R + 2.  (target, ops, score, q_begin, t_begin, q_end, t_end) each."""
    a = 40
    query = rng.choice(PROTEIN[:20], 300).astype(np.uint8)
    while query[a + 29] == query[a + 34] or query[a + 30] == query[a + 35]:      # (the I run must not be free to slide along equal letters)
        query = rng.choice(PROTEIN[:20], 300).astype(np.uint8)
    sub = _crisp_submat(swamd, rng)
    go, ge = -8, -1
    foreign = lambda n: rng.choice(PROTEIN[20:], n).astype(np.uint8)  # noqa: E731
    diag = lambda seq: int(sum(int(sub[x, x]) for x in seq))  # noqa: E731
    cases = []
    for R in (64, 128):
        for r in (R - 1, R, R + 1, R + 2):
            for n in (1, 15, 70):        # D x n whose first row is r, after 30 pairs: opens below / on / above the checkpoint, 70 spans a band
                P = r - 1 - 30
                t = np.concatenate([foreign(P), query[a:a + 30], foreign(n), query[a + 30:a + 130]])
                cases.append((t, b"M" * 30 + b"D" * n + b"M" * 100, diag(query[a:a + 130]) + go + n * ge, a, P, a + 130, len(t)))
            P = r - 30                   # I x 5 in row r, the row of the 30th pair
            t = np.concatenate([foreign(P), query[a:a + 30], query[a + 35:a + 135]])
            cases.append((t, b"M" * 30 + b"I" * 5 + b"M" * 100, diag(t[P:]) + go + 5 * ge, a, P, a + 135, len(t)))
            P = r - 1                    # the begin corner: the first pair in row r
            t = np.concatenate([foreign(P), query[a:a + 100]])
            cases.append((t, b"M" * 100, diag(query[a:a + 100]), a, P, a + 100, len(t)))
            P = r - 40                   # the end cell in row r, ten foreign rows behind it
            t = np.concatenate([foreign(P), query[a:a + 40], foreign(10)])
            cases.append((t, b"M" * 40, diag(query[a:a + 40]), a, P, a + 40, r))
    return query, sub, go, ge, cases


def test_gaps_and_corners_on_a_checkpoint_row(eng, checker, swamd):  # noqa: F811
    rng = np.random.default_rng(64128)
    query, sub, go, ge, cases = planted(swamd, rng)
    targets = [c[0] for c in cases]
    hits = list(range(len(targets)))
    aln, ops = both_modes(eng, query, targets, sub, go, ge, hits)
    M = len(query) + 1
    for k, (t, eops, score, qb, tb, qe, te) in enumerate(cases):
        assert ops[k] == eops, f"case {k}: {ops[k]}"
        assert tuple(int(x) for x in aln[k]) == (te * M + qe, score, qb, tb, qe, te, len(eops)), f"case {k}: {tuple(aln[k])}"
        replay(query, t, sub, go, ge, aln[k], ops[k])
    assert_exact(checker, query, targets, sub, go, ge, hits, aln, ops, "planted")


def test_strip_boundary_times_checkpoint(eng, checker, swamd):  # noqa: F811
    rng = np.random.default_rng(77)
    B = 1024
    query = rng.choice(PROTEIN[:20], 2300).astype(np.uint8)
    sub, go, ge, cases = indel_cases(swamd, rng, query, B, span=200)
    targets = [c[0] for c in cases]
    hits = list(range(len(targets)))
    aln, ops = both_modes(eng, query, targets, sub, go, ge, hits)
    for k, (t, eops, score) in enumerate(cases):
        assert int(aln[k, 1]) == score and ops[k] == eops, f"case {k}: {ops[k]}"
    assert_exact(checker, query, targets, sub, go, ge, hits, aln, ops, "indels")


def related_targets(rng, query, count):
    """The targets of test_slots_are_reused (test_align_affine_gpu.py): slices of the query with substitutions and indels, 300..700 letters."""
    targets = []
    for n in rng.integers(300, 701, count):
        a = int(rng.integers(0, 100))
        s = list(query[a:a + 400])
        for _ in range(3):
            at, run = int(rng.integers(20, len(s) - 20)), int(rng.integers(1, 10))
            if rng.random() < 0.5:
                del s[at:at + run]
            else:
                s[at:at] = list(rng.choice(PROTEIN, run))
        s = (list(rng.choice(PROTEIN, n)) + s)[-int(n):] if len(s) < n else s[:int(n)]
        targets.append(np.array(s, np.uint8))
    return targets


def test_refused_today_aligned_now(eng, checker, swamd):  # noqa: F811
    rng = np.random.default_rng(5)
    query = rng.choice(PROTEIN, 513).astype(np.uint8)
    targets = related_targets(rng, query, 40)
    sub = random_submat(rng)
    long_t = np.concatenate([rng.choice(PROTEIN, 350).astype(np.uint8), query[20:500], rng.choice(PROTEIN, 270).astype(np.uint8)])
    assert len(long_t) == 1100
    ref_aln, ref_ops = eng.align_affine(query, targets, sub, -10, -1, list(range(40)))
    assert eng.get_option("last_align_affine_checkpointed") == 0
    eng.set_option("align_workspace_mib", 1)
    with pytest.raises(swamd.SwError, match="align_workspace_mib"):          # 1100 rows x 1024 bytes: refused as it always was
        eng.align_affine(query, [long_t], sub, -10, -1, [0])
    aln, ops = eng.align_affine(query, [long_t], sub, -10, -1, [0], checkpoint=2)
    assert eng.get_option("last_align_affine_checkpointed") == 1
    assert 0 < eng.get_option("last_align_affine_slot_bytes") <= 1 << 20
    haln, hops = swamd.align_affine_host(query, [long_t], sub, -10, -1, [0])
    assert np.array_equal(aln, haln) and ops == hops and len(ops[0]) > 400
    replay(query, long_t, sub, -10, -1, aln[0], ops[0])
    # 40 hits through the one or two slots that fit
    aln, ops = eng.align_affine(query, targets, sub, -10, -1, list(range(40)), checkpoint=1)
    assert eng.get_option("last_align_affine_slots") == (1 << 20) // eng.get_option("last_align_affine_slot_bytes") < 40
    assert np.array_equal(aln, ref_aln) and ops == ref_ops
    assert max(len(o) for o in ops) > 200


def test_beyond_a_descriptor(swamd):
    """The longest target a call of the search family accepts (2^20 - 1 letters) against a 2100-letter query: 3.2 GB of direction bytes at 3072 padded columns, more than the workspace
    holds and more than a descriptor addresses, so no option makes the whole-matrix path take it.  Every off-diagonal entry of the
    table is negative, so the cells of the background hold H = 0, E = F = goe: the state above the planted rows is row 0's state, and
    the alignment inside the slice 50 letters either side of the copy is the whole target's."""
    rng = np.random.default_rng(4300)
    sub = _crisp_submat(swamd, rng)
    go, ge = -8, -1
    query = rng.choice(PROTEIN[:10], 2100).astype(np.uint8)
    copy = list(query[1020:1280])                                      # 260 letters across the boundary of the first two strips
    copy[40], copy[200] = PROTEIN[10], PROTEIN[11]                     # two substitutions
    del copy[100:105]                                                  # a 5-letter deletion
    copy[150:150] = list(rng.choice(PROTEIN[10:20], 4))               # a 4-letter insertion
    copy = np.array(copy, np.uint8)

    def build(total):
        t = rng.choice(PROTEIN[10:20], total).astype(np.uint8)
        at = total - 3000 - len(copy)
        t[at:at + len(copy)] = copy
        return t, at

    def sliced(t, at):
        lo, hi = at - 50, at + len(copy) + 50
        aln, ops = swamd.align_affine_host(query, [t[lo:hi]], sub, go, ge, [0])
        row = [int(x) for x in aln[0]]
        te, qe = divmod(row[0], len(query) + 1)
        row[0] = (te + lo) * (len(query) + 1) + qe
        row[3] += lo
        row[5] += lo
        return tuple(row), ops[0]

    small, at = build(20000)                                            # the slice argument itself, where the host leg on the whole target is cheap
    haln, hops = swamd.align_affine_host(query, [small], sub, go, ge, [0])
    assert (tuple(int(x) for x in haln[0]), hops[0]) == sliced(small, at)
    big, at = build((1 << 20) - 1)
    erow, eops = sliced(big, at)
    assert b"D" in eops and b"I" in eops and len(eops) > 250
    eng = swamd.Engine(0)
    try:
        with pytest.raises(swamd.SwError, match="align_workspace_mib"):
            eng.align_affine(query, [big], sub, go, ge, [0])
        aln, ops = eng.align_affine(query, [big], sub, go, ge, [0], checkpoint=2)
        assert eng.get_option("last_align_affine_checkpointed") == 1
        rows = eng.get_option("last_align_affine_band_rows")
        assert rows >= 256 and rows & (rows - 1) == 0 and eng.get_option("last_align_affine_slot_bytes") < 64 << 20
        assert len(big) * 3072 > (1 << 31)
        assert (tuple(int(x) for x in aln[0]), ops[0]) == (erow, eops)
        res = eng.search_affine(query, [big], sub, go, ge)
        assert (int(res[0, 0]), int(res[0, 1])) == erow[:2]
        replay(query, big, sub, go, ge, aln[0], ops[0])
    finally:
        eng.close()
