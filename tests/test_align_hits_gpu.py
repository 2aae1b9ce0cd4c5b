"""GPU: the alignments of a device hit table (sw_db_align_affine_hits / Database.align_affine_hits_device) against Engine.align_affine
per query (held to the independent checker by test_align_affine_gpu.py) and the host leg: all three classes of queries and their
edges in one call, hand-built tables and the output of the device selection fed straight in, size tiers and slot reuse under a small
workspace, two groups, gaps across a strip boundary, small and absent ops rows.  Every output lies between poisoned guard regions."""
import numpy as np
import pytest

from affine_cases import DNA, GAPS, PROTEIN, random_submat
from align_cases import h_cells, indel_cases, pack

pytestmark = pytest.mark.gpu

POISON = 0x5A
POISON64 = 0x5A5A5A5A5A5A5A5A
GUARD = 64           # int64 words before and behind d_aln, and 8 x that many bytes around d_ops
TIER_RATIO, TIER_FLOOR, MAX_TIERS = 4, 32 << 10, 4      # swp::kAlignHitsTier* (smith-waterman_amd/csrc/sw_plan.h)


def run_table(eng, db, queries, scoring, d_hits, d_nhits, top, cap):
    """One call on poisoned, guarded outputs.  Returns (aln (nq, top, 7), ops (nq, top, cap) or None) as numpy, guards checked."""
    t = eng.torch
    dev = f"cuda:{eng.device}"
    qp, qo = pack(queries)
    nq = len(queries)
    n = nq * top
    d_q = t.from_numpy(qp.copy()).to(dev)
    abuf = t.full((GUARD + n * 7 + GUARD,), POISON64, dtype=t.int64, device=dev)
    obuf = t.full((8 * GUARD + n * cap + 8 * GUARD,), POISON, dtype=t.uint8, device=dev) if cap > 0 else None
    out = (abuf[GUARD:GUARD + n * 7], obuf[8 * GUARD:8 * GUARD + n * cap] if cap > 0 else None)
    aln, ops = db.align_affine_hits_device(d_q, qo, scoring, d_hits, d_nhits, ops_cap=cap, out=out, top=top)
    eng.synchronize()
    a = abuf.cpu().numpy()
    assert np.all(a[:GUARD] == POISON64) and np.all(a[-GUARD:] == POISON64), "a guard region of d_aln was written"
    assert aln.shape == (nq, top, 7)
    if cap > 0:
        o = obuf.cpu().numpy()
        assert np.all(o[:8 * GUARD] == POISON) and np.all(o[-8 * GUARD:] == POISON), "a guard region of d_ops was written"
        assert ops.shape == (nq, top, cap)
    return aln.cpu().numpy(), (ops.cpu().numpy() if cap > 0 else None)


def reference(eng, queries, targets, scoring, table, nhits):
    """Engine.align_affine per query over the used entries inside the database: {(q, r): (aln row, ops bytes)}."""
    sub, go, ge = scoring
    packed, offs = pack(targets)
    nq, top = table.shape[:2]
    ref = {}
    for q in range(nq):
        used = top if nhits is None else int(np.clip(nhits[q], 0, top))
        rs = [r for r in range(used) if 0 <= table[q, r, 0] < len(targets)]
        if rs:
            aln, ops = eng.align_affine(queries[q], (packed, offs), sub, go, ge, [int(table[q, r, 0]) for r in rs])
            ref.update({(q, r): (aln[i], ops[i]) for i, r in enumerate(rs)})
    return ref


def assert_table(aln, ops, cap, ref, what=""):
    nq, top = aln.shape[:2]
    for q in range(nq):
        for r in range(top):
            if (q, r) in ref:
                ea, eo = ref[(q, r)]
                assert tuple(aln[q, r]) == tuple(ea), f"{what} entry {q, r}: {tuple(aln[q, r])} vs {tuple(ea)}"
                if ops is not None and ea[6] <= cap:
                    assert ops[q, r, :ea[6]].tobytes() == eo, f"{what} entry {q, r}: ops differ"
                    assert np.all(ops[q, r, ea[6]:] == POISON), f"{what} entry {q, r}: bytes behind nops were written"
            else:
                assert not aln[q, r].any(), f"{what} entry {q, r} must be all zeros: {tuple(aln[q, r])}"
                assert ops is None or np.all(ops[q, r] == POISON), f"{what} entry {q, r}: the ops row of an unused entry was written"


def to_dev(eng, arr):
    return eng.torch.from_numpy(np.ascontiguousarray(arr).copy()).to(f"cuda:{eng.device}")


QLENS = [513, 1, 2049, 256, 64, 1025, 257, 512]       # all three classes, their edges, two and three strips at 16 columns per lane
TOP = 5


@pytest.fixture(scope="module")
def mixed(engine):
    rng = np.random.default_rng(4242)
    queries = [rng.choice(PROTEIN, n).astype(np.uint8) for n in QLENS]
    lens = [0, 1, 63, 64, 65] + list(rng.integers(2, 701, 19))
    targets = [rng.choice(PROTEIN, int(n)).astype(np.uint8) for n in lens]
    # a few targets related to the long queries, so that some alignments are long and carry gaps
    targets[7] = np.concatenate([queries[2][100:400], queries[2][404:700]])
    targets[9] = np.concatenate([queries[5][:300], rng.choice(PROTEIN, 5).astype(np.uint8), queries[5][300:600]])
    targets[11] = queries[0][50:450].copy()
    related = [targets[7], targets[9], targets[11]]
    targets = [targets[k] for k in rng.permutation(len(targets))]
    where = [next(i for i, t in enumerate(targets) if t is x) for x in related]
    nt = len(targets)
    scoring = (random_submat(rng), *GAPS[0])
    hits = rng.integers(0, nt, (len(queries), TOP)).astype(np.int64)
    hits[0, 1] = hits[0, 0]                                                            # a duplicate
    hits[2, 1], hits[5, 0], hits[0, 2] = where                                          # each related target under its query
    hits[1, 2], hits[2, 0], hits[6, 4] = -1, -7, nt                                     # outside the database, inside a used part
    nhits = np.array([TOP, TOP, 3, 0, TOP + 2, 1, TOP, 4], np.int64)                    # one row unused, full rows, one above top
    table = np.stack([hits, np.full_like(hits, 3), np.full_like(hits, 9)], axis=-1)     # only `target` is read
    ref = reference(engine, queries, targets, scoring, table, nhits)
    return dict(queries=queries, targets=targets, scoring=scoring, table=table, nhits=nhits, ref=ref, cap=2049 + 700)


def test_hand_built_table(engine, swamd, mixed):
    m = mixed
    with engine.prepare_db(m["targets"]) as db:
        aln, ops = run_table(engine, db, m["queries"], m["scoring"], to_dev(engine, m["table"]), to_dev(engine, m["nhits"]), TOP, m["cap"])
        assert_table(aln, ops, m["cap"], m["ref"], "table (a)")
        assert len(m["ref"]) == 5 + 4 + 2 + 0 + 5 + 1 + 4 + 4 and max(int(a[6]) for a, _ in m["ref"].values()) > 250
        # the host leg gives the same table
        haln, hops = swamd.align_affine_hits_host(m["queries"], m["targets"], m["scoring"], m["table"], m["nhits"])
        assert np.array_equal(aln, haln)
        assert all(ops[q, r, :aln[q, r, 6]].tobytes() == hops[q][r] for q in range(len(QLENS)) for r in range(TOP))
        assert engine.get_option("last_align_hits_tiers") >= 3 and engine.get_option("last_align_hits_launches") == 3 + engine.get_option("last_align_hits_tiers")
        assert 3 <= engine.get_option("last_align_hits_lists") <= engine.get_option("last_align_hits_tiers")   # every class has items
        # NULL counts: every entry of every row is used
        aln2, ops2 = run_table(engine, db, m["queries"], m["scoring"], to_dev(engine, m["table"]), None, TOP, m["cap"])
        assert_table(aln2, ops2, m["cap"], reference(engine, m["queries"], m["targets"], m["scoring"], m["table"], None), "NULL nhits")
        # twice the same call: identical bytes
        aln3, ops3 = run_table(engine, db, m["queries"], m["scoring"], to_dev(engine, m["table"]), None, TOP, m["cap"])
        assert np.array_equal(aln2, aln3) and np.array_equal(ops2, ops3)


def test_table_of_the_device_selection_goes_straight_in(engine, mixed):
    m = mixed
    t = engine.torch
    qp, qo = pack(m["queries"])
    with engine.prepare_db(m["targets"]) as db:
        d_q = to_dev(engine, qp)
        d_hits, d_nhits = db.search_affine_top_device(d_q, qo, m["scoring"], TOP, min_score=1)      # no host copy in between
        aln, ops = run_table(engine, db, m["queries"], m["scoring"], d_hits, d_nhits, TOP, m["cap"])
        table, nhits = d_hits.cpu().numpy(), d_nhits.cpu().numpy()
        assert nhits.min() >= 1 and (table[:, :, 0] >= 0).sum() == nhits.sum()
        assert_table(aln, ops, m["cap"], reference(engine, m["queries"], m["targets"], m["scoring"], table, nhits), "table (b)")
        for q in range(len(QLENS)):                                                      # the search's arg-max, found again by the re-fill
            assert np.array_equal(aln[q, :nhits[q], :2], table[q, :nhits[q], 1:3])
        assert isinstance(d_hits, t.Tensor)


def test_small_ops_rows_and_no_ops(engine, mixed):
    m = mixed
    cap = 40
    with engine.prepare_db(m["targets"]) as db:
        aln, ops = run_table(engine, db, m["queries"], m["scoring"], to_dev(engine, m["table"]), to_dev(engine, m["nhits"]), TOP, cap)
        nops = np.array([int(a[6]) for a, _ in m["ref"].values()])
        assert (nops > cap).any() and ((nops > 0) & (nops <= cap)).any()
        assert_table(aln, ops, cap, m["ref"], "ops_cap 40")                              # the true nops everywhere; rows that fit are exact, none spills
        aln, none = run_table(engine, db, m["queries"], m["scoring"], to_dev(engine, m["table"]), to_dev(engine, m["nhits"]), TOP, 0)
        assert none is None
        assert_table(aln, None, 0, m["ref"], "d_ops NULL")


def test_two_groups(engine, mixed):
    m = mixed
    with engine.prepare_db(m["targets"]) as db:
        d_table, d_n = to_dev(engine, m["table"]), to_dev(engine, m["nhits"])
        one = run_table(engine, db, m["queries"], m["scoring"], d_table, d_n, TOP, m["cap"])
        tiers_one = engine.get_option("last_align_hits_tiers")
        engine.set_option("search_profile_mib", 1)                                       # 257 x (3072 + 2048) bytes alone exceed it
        try:
            two = run_table(engine, db, m["queries"], m["scoring"], d_table, d_n, TOP, m["cap"])
            assert engine.get_option("last_align_hits_launches") - engine.get_option("last_align_hits_tiers") >= 3 * 2   # at least two groups
            assert engine.get_option("last_align_hits_tiers") > tiers_one
        finally:
            engine.set_option("search_profile_mib", 256)
        assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1])
        assert_table(two[0], two[1], m["cap"], m["ref"], "two groups")


def planned_bounds(longest, qpad):
    b = [longest * qpad]
    while len(b) < MAX_TIERS and b[-1] // TIER_RATIO >= TIER_FLOOR:
        b.append(b[-1] // TIER_RATIO)
    return b[::-1]


def test_tiers_and_slot_reuse(swamd):
    """A 1 MiB workspace: 120 items through far fewer direction matrices, in tiers of different sizes; every item but the first of a
    slot walks lines an earlier item left behind, of another row stride where the queries differ."""
    rng = np.random.default_rng(5)
    long_q = rng.choice(PROTEIN, 1025).astype(np.uint8)
    queries = [long_q[100:300].copy(), long_q[350:750].copy(), long_q]                   # 4, 8 and 16 columns per lane
    targets = []
    for i, n in enumerate(rng.integers(100, 501, 40)):
        n = 500 if i == 0 else 100 if i == 1 else int(n)
        a = int(rng.integers(0, 500))
        s = list(long_q[a:a + n])
        for _ in range(3):
            at, run = int(rng.integers(20, len(s) - 20)), int(rng.integers(1, 10))
            if rng.random() < 0.5:
                del s[at:at + run]
            else:
                s[at:at] = list(rng.choice(PROTEIN, run))
        s = (list(rng.choice(PROTEIN, n)) + s)[-n:] if len(s) < n else s[:n]
        targets.append(np.array(s, np.uint8))
    lens = [len(t) for t in targets]
    assert min(lens) == 100 and max(lens) == 500
    scoring = (random_submat(rng), -10, -1)
    table = np.zeros((3, 40, 3), np.int64)
    table[:, :, 0] = np.stack([rng.permutation(40) for _ in range(3)])
    eng = swamd.Engine(0)
    try:
        with eng.prepare_db(targets) as db:
            ref = run_table(eng, db, queries, scoring, to_dev(eng, table), None, 40, 1025 + 500)
            eng.set_option("align_workspace_mib", 1)                                     # 500 x 2048 bytes just fit
            aln, ops = run_table(eng, db, queries, scoring, to_dev(eng, table), None, 40, 1025 + 500)
            assert np.array_equal(aln, ref[0]) and np.array_equal(ops, ref[1])
            assert_table(aln, ops, 1525, reference(eng, queries, targets, scoring, table, None), "1 MiB")
            assert aln[:, :, 6].max() > 200                                              # long walks, not begin corners next to the end
            # the planned tiers, by the rule of sw_plan.h, and the items they receive
            bounds = [planned_bounds(500, qpad) for qpad in (256, 512, 2048)]
            assert eng.get_option("last_align_hits_tiers") == sum(len(b) for b in bounds) == 1 + 2 + 3
            filled = sum(len({min(t for t, x in enumerate(b) if n * qpad <= x) for n in lens}) for b, qpad in zip(bounds, (256, 512, 2048)))
            assert filled == 1 + 2 + 2                                                   # by those bounds: two tiers of the 8- and of the 16-column class
            assert eng.get_option("last_align_hits_lists") == filled                     # ... and that many lists received items on the device
            slots = sum(min(40, (1 << 20) // x) for b in bounds for x in b)
            assert eng.get_option("last_align_hits_slots") == slots < 120
        # one 1100-letter target in the handle: 1100 x 2048 bytes could be asked for, whatever the table says
        with eng.prepare_db(targets + [rng.choice(PROTEIN, 1100).astype(np.uint8)]) as db:
            with pytest.raises(swamd.SwError, match="align_workspace_mib"):
                run_table(eng, db, queries, scoring, to_dev(eng, np.full((3, 40, 3), -1, np.int64)), None, 40, 0)
    finally:
        eng.close()


def test_gaps_across_the_strip_boundary(engine, swamd):
    rng = np.random.default_rng(77)
    B = 1024
    query = rng.choice(PROTEIN[:20], 2300).astype(np.uint8)
    sub, go, ge, cases = indel_cases(swamd, rng, query, B, span=200)
    targets = [c[0] for c in cases]
    queries = [rng.choice(PROTEIN[:20], 100).astype(np.uint8), query, rng.choice(PROTEIN[:20], 700).astype(np.uint8)]
    table = np.zeros((3, len(cases), 3), np.int64)
    table[:, :, 0] = np.arange(len(cases))
    with engine.prepare_db(targets) as db:
        aln, ops = run_table(engine, db, queries, (sub, go, ge), to_dev(engine, table), None, len(cases), 2300 + 500)
    for k, (t, eops, score) in enumerate(cases):
        assert int(aln[1, k, 1]) == score and ops[1, k, :aln[1, k, 6]].tobytes() == eops, f"case {k}"
        assert tuple(int(x) for x in aln[1, k, 2:6]) == (B - 200, 0, B + 200, len(t))
    assert_table(aln, ops, 2800, reference(engine, queries, targets, (sub, go, ge), table, None), "indels")


def test_gap_open_zero_walks_the_linear_traceback(engine, swamd):
    rng = np.random.default_rng(513)
    a, b = rng.choice(DNA, 513).astype(np.uint8), rng.choice(DNA, 580).astype(np.uint8)
    out = engine.fill(a, b, (3, -3, -2))
    r = out.result()
    path = engine.traceback(out, r["max_pos"])
    with engine.prepare_db([rng.choice(DNA, 50).astype(np.uint8), b]) as db:
        aln, ops = db.align_affine_hits([a], (swamd.submat_match(3, -3), 0, -2), np.array([[1, 0]], np.int64), np.array([1], np.int64))
    assert (int(aln[0, 0, 0]), int(aln[0, 0, 1])) == (r["max_pos"], r["max_score"])
    assert h_cells(aln[0, 0], ops[0][0], 513) == [int(x) for x in path]
    assert not aln[0, 1].any() and ops[0][1] == b""


def test_empty_handle_and_no_queries(engine, swamd):
    t = engine.torch
    sub = swamd.submat_match(3, -3)
    with engine.prepare_db([]) as db:                                                   # ntargets == 0: d_aln is zeroed, nothing else
        aln, ops = run_table(engine, db, [np.frombuffer(b"ACGT", np.uint8)], (sub, -2, -1), to_dev(engine, np.zeros((1, 3, 3), np.int64)), None, 3, 8)
        assert not aln.any() and np.all(ops == POISON)
        assert [engine.get_option("last_align_hits_" + x) for x in ("launches", "tiers", "slots", "lists")] == [0, 0, 0, 0]
    with engine.prepare_db([b"ACGT", b""]) as db:
        d_q = t.zeros(1, dtype=t.uint8, device=f"cuda:{engine.device}")
        out = (t.full((7,), POISON64, dtype=t.int64, device=d_q.device), None)
        aln, _ = db.align_affine_hits_device(d_q, np.zeros(1, np.int64), (sub, -2, -1), t.zeros(3, dtype=t.int64, device=d_q.device), None, out=out, top=1)
        engine.synchronize()
        assert aln.shape == (0, 1, 7) and np.all(out[0].cpu().numpy() == POISON64)       # nqueries == 0: nothing launched
        aln, ops = db.align_affine_hits([b"ACGT"], (sub, -2, -1), np.array([[1, 0, 2]], np.int64))   # an empty target, a hit, ntargets itself
        assert not aln[0, 0].any() and not aln[0, 2].any() and tuple(aln[0, 1]) == (4 * 5 + 4, 12, 0, 0, 4, 4, 4) and ops[0] == [b"", b"MMMM", b""]


def test_cli_aligns_query_by_query_where_the_one_call_refuses(engine, swamd, tmp_path):
    """A 30 000-letter query and one 35 000-letter target in the database: 35 000 x 30 720 bytes are above the default workspace of
    1 GiB, so the call on the whole table refuses -- it cannot know that the two hits are short -- and smithW aligns them per query."""
    import os
    import subprocess
    from affine_cases import ROOT
    rng = np.random.default_rng(9)
    query = rng.choice(DNA, 30000).astype(np.uint8)
    targets = [rng.choice(DNA, 35000).astype(np.uint8), query[100:400].copy(), np.concatenate([query[5000:5100], query[5103:5200]])]
    qfa, dfa = tmp_path / "q.fa", tmp_path / "db.fa"
    qfa.write_text(">q\n" + query.tobytes().decode() + "\n")
    dfa.write_text("".join(f">t{k}\n{t.tobytes().decode()}\n" for k, t in enumerate(targets)))
    exe = os.path.join(ROOT, "smith-waterman_amd", "smithW")
    run = subprocess.run([exe, "--search", str(qfa), str(dfa), "--all-queries", "--top", "2", "--align", "--gap-open", "-12", "--gap-extend", "-3"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    aln, ops = engine.align_affine(query, targets, swamd.submat_match(3, -3), -12, -3, [1, 2])   # (dear gaps: the long random target scores far below the two related ones)
    lines = run.stdout.split("\n")
    got = [ln.split("\t")[1:] for ln in lines if ln.startswith("align\t")]
    assert got == [[str(int(aln[h, c])) for c in (2, 4, 3, 5, 6)] for h in range(2)]
    assert [ln.split("\t")[1] for ln in lines if ln[:1].isdigit()] == ["1", "2"]
