"""GPU: checkpointed alignment ("align_checkpoint") of a device hit table (sw_db_align_affine_hits) against the whole-matrix path on
the same engine, byte for byte, and the host leg; and the buffer contract of sw_align_affine_device under it: guard regions around
every buffer, an odd base for d_ops, ops_cap one below, at and one above a hit's nops.  Bands of 64 rows throughout."""
import numpy as np
import pytest

from affine_cases import PROTEIN, checker, random_submat  # noqa: F401
from align_cases import expected, pack
from buffer_cases import POISON, POISON64, Arena, arena_bytes, assert_guards, live_head, live_tail

pytestmark = pytest.mark.gpu

GUARD = 64           # int64 words before and behind d_aln, and 8 x that many bytes around d_ops
TOP = 8


@pytest.fixture()
def eng(swamd):
    e = swamd.Engine(0)
    e.set_option("align_checkpoint_rows", 64)
    yield e
    e.close()


def to_dev(eng, arr):
    return eng.torch.from_numpy(np.ascontiguousarray(arr).copy()).to(f"cuda:{eng.device}")


def run_table(eng, db, queries, scoring, table, nhits, cap, mode):
    """One call on poisoned, guarded outputs under `mode`.  Returns every byte of d_aln and d_ops as numpy, guards checked."""
    t = eng.torch
    dev = f"cuda:{eng.device}"
    qp, qo = pack(queries)
    n = len(queries) * TOP
    arena = Arena(t, dev, arena_bytes(len(qp) + 128))
    d_q, _ = arena.place(qp, 64, 3, front=live_head(qp, 64), back=live_tail(qp, 64), name="queries")
    abuf = t.full((GUARD + n * 7 + GUARD,), POISON64, dtype=t.int64, device=dev)
    obuf = t.full((8 * GUARD + n * cap + 8 * GUARD,), POISON, dtype=t.uint8, device=dev)
    out = (abuf[GUARD:GUARD + n * 7], obuf[8 * GUARD:8 * GUARD + n * cap])
    aln, ops = db.align_affine_hits_device(d_q, qo, scoring, to_dev(eng, table), to_dev(eng, nhits), ops_cap=cap, out=out, top=TOP, checkpoint=mode)
    eng.synchronize()
    a, o = abuf.cpu().numpy(), obuf.cpu().numpy()
    assert np.all(a[:GUARD] == POISON64) and np.all(a[-GUARD:] == POISON64), "a guard region of d_aln was written"
    assert np.all(o[:8 * GUARD] == POISON) and np.all(o[-8 * GUARD:] == POISON), "a guard region of d_ops was written"
    assert_guards(arena)
    return aln.cpu().numpy(), ops.cpu().numpy()


def table_case(rng):
    queries = [rng.choice(PROTEIN, n).astype(np.uint8) for n in (100, 300, 600)]         # one of each class
    targets = [rng.choice(PROTEIN, int(n)).astype(np.uint8) for n in [0, 1, 64, 65, 700] + list(rng.integers(2, 701, 55))]
    # related targets, so that alignments are long, carry gaps and cross several checkpoint rows
    targets[10] = np.concatenate([rng.choice(PROTEIN, 130).astype(np.uint8), queries[2][20:300], queries[2][304:590]])
    targets[11] = np.concatenate([queries[1][:140], rng.choice(PROTEIN, 6).astype(np.uint8), queries[1][140:290], rng.choice(PROTEIN, 90).astype(np.uint8)])
    targets[12] = np.concatenate([rng.choice(PROTEIN, 60).astype(np.uint8), queries[0][5:95]])
    nt = len(targets)
    assert nt == 60 and max(len(t) for t in targets) <= 700
    hits = rng.integers(0, nt, (3, TOP)).astype(np.int64)
    hits[:, 0] = [12, 11, 10]
    hits[:, 1] = [10, 12, 11]
    hits[0, 2], hits[1, 2], hits[2, 2] = -1, nt, 4                                       # outside the database on either side, inside used parts
    table = np.stack([hits, np.full_like(hits, 3), np.full_like(hits, 9)], axis=-1)       # only `target` is read
    return queries, targets, (random_submat(rng), -10, -1), table


def test_hit_table(eng, swamd):
    rng = np.random.default_rng(6001)
    queries, targets, scoring, table = table_case(rng)
    cap = 600 + 700
    with eng.prepare_db(targets) as db:
        for nhits in ([0, 3, 8], [8, 0, 3], [3, 8, 0]):
            nhits = np.array(nhits, np.int64)
            aln, ops = run_table(eng, db, queries, scoring, table, nhits, cap, 1)
            assert eng.get_option("last_align_hits_checkpointed") == 1 and eng.get_option("last_align_hits_band_rows") == 64
            ref_aln, ref_ops = run_table(eng, db, queries, scoring, table, nhits, cap, 0)
            assert eng.get_option("last_align_hits_checkpointed") == 0 and eng.get_option("last_align_hits_band_rows") == 0
            assert np.array_equal(aln, ref_aln)                                          # every byte of d_aln
            used = 0
            for q in range(3):
                for r in range(TOP):
                    inside = r < nhits[q] and 0 <= table[q, r, 0] < len(targets)
                    if inside:
                        n = int(aln[q, r, 6])
                        assert np.array_equal(ops[q, r], ref_ops[q, r]) and np.all(ops[q, r, n:] == POISON), f"entry {q, r}: ops"
                        used += n > 0
                    else:
                        assert not aln[q, r].any() and np.all(ops[q, r] == POISON), f"entry {q, r}: an unused entry"
            assert used >= 3 and int(aln[:, :, 6].max()) > 250
            haln, hops = swamd.align_affine_hits_host(queries, targets, scoring, table, nhits)
            assert np.array_equal(aln, haln)
            assert all(ops[q, r, :aln[q, r, 6]].tobytes() == hops[q][r] for q in range(3) for r in range(TOP))
    # one long record that no hit names: the whole-matrix call is refused for it, whatever the table says; mode 2 is not
    eng.set_option("align_workspace_mib", 1)
    nhits = np.array([8, 3, 8], np.int64)
    longer = targets + [rng.choice(PROTEIN, 3000).astype(np.uint8)]
    table = table.copy()
    table[1, 2, 0] = len(longer)                                                         # (still outside: no entry names the new record)
    with eng.prepare_db(longer) as db:
        with pytest.raises(swamd.SwError, match="align_workspace_mib"):
            run_table(eng, db, queries, scoring, table, nhits, cap, 0)
        aln, ops = run_table(eng, db, queries, scoring, table, nhits, cap, 2)
        assert eng.get_option("last_align_hits_checkpointed") == 1
        haln, hops = swamd.align_affine_hits_host(queries, longer, scoring, table, nhits)
        assert np.array_equal(aln, haln) and int(aln[:, :, 6].max()) > 250
        assert all(ops[q, r, :aln[q, r, 6]].tobytes() == hops[q][r] for q in range(3) for r in range(TOP))
        # a workspace that holds the long record's whole matrix: mode 2 is the whole-matrix path, unchanged
        eng.set_option("align_workspace_mib", 64)
        aln2, ops2 = run_table(eng, db, queries, scoring, table, nhits, cap, 2)
        assert eng.get_option("last_align_hits_checkpointed") == 0
        assert np.array_equal(aln2, aln) and np.array_equal(ops2, ops)


def related(rng, query, count):
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


@pytest.mark.parametrize("qlen,qskew", [(129, 1), (513, 2), (1025, 3)])
def test_buffer_contract(eng, checker, qlen, qskew):  # noqa: F811
    """Guards around d_aln, d_ops, the query and the database; d_ops at an odd address; ops_cap one below, at and one above the nops of
    one hit: nops is always the true length, a hit whose ops do not fit writes no op byte, nothing leaves a hit's own row."""
    torch = eng.torch
    dev = f"cuda:{eng.device}"
    rng = np.random.default_rng(7700 + qlen)
    query = rng.choice(PROTEIN, qlen).astype(np.uint8)
    targets = related(rng, query, 8)
    hits = [0, 1, 2, 3, 4, 5, 6, 7, 2, 2, 5, 0]
    sub, go, ge = random_submat(rng), -10, -1
    exp = [expected(checker, query, t, sub, go, ge) for t in targets]
    nops = sorted(exp[k][0][6] for k in hits)
    assert nops[0] >= 1 and nops[-1] > qlen // 2 and max(len(t) for t in targets) > 64, "the walks were meant to be long and to cross checkpoint rows"
    packed, offs = pack(targets)
    packed = np.concatenate([live_head(packed, 7), packed])
    offs = offs + 7
    mid = nops[len(nops) // 2]
    for cap in (mid - 1, mid, mid + 1):
        inp = Arena(torch, dev, arena_bytes(len(query) + 128, len(packed) + 128))
        d_q, _ = inp.place(query, 64, qskew, front=live_head(query, 64), back=live_tail(query, 64), name="query")
        d_db, _ = inp.place(packed, 64, 1, front=live_head(packed, 64), back=live_tail(packed, 64), name="db")
        nh = len(hits)
        out = Arena(torch, dev, arena_bytes(nh * 56, nh * cap))
        ca = out.carve(nh * 56, 16, 8, name="aln")
        co = out.carve(nh * cap, 64, 1, name="ops")                                      # an odd base
        aln, ops = out.view(ca, torch.int64, (nh, 7)), out.view(co, torch.uint8, (nh, cap))
        eng.align_affine_device(d_q, len(query), d_db, offs, sub, go, ge, hits, ops_cap=cap, out=(aln, ops), checkpoint=1)
        eng.synchronize()
        assert eng.get_option("last_align_affine_checkpointed") == 1 and eng.get_option("last_align_affine_band_rows") == 64
        a, o = aln.cpu().numpy(), ops.cpu().numpy()
        for h, k in enumerate(hits):
            row, eops, _ = exp[k]
            assert tuple(int(x) for x in a[h]) == row, f"ops_cap {cap}, hit {h} (target {k})"
            if row[6] <= cap:
                assert o[h, :row[6]].tobytes() == eops and (o[h, row[6]:] == POISON).all(), f"ops_cap {cap}, hit {h} (target {k}): ops"
            else:
                assert (o[h] == POISON).all(), f"ops_cap {cap}, hit {h} (target {k}): op bytes written that do not fit"
        assert_guards(out)
        assert_guards(inp)
