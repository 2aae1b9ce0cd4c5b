"""GPU: the many-query affine family at the edges of its score range and its alphabet -- the case table of tests/affine_range_cases.py,
whose expectations come from the independent checkers alone (tests/test_affine_range_host.py asserts the table's conditions on them).
Every call writes into poisoned outputs, equality is exact, and after each comparison the route is asserted from the "last_*"
options so that no case passes on a path it was not meant for.

The near-limit alignment is out of scope: the whole direction matrix of the (L + 1) x L pair exceeds kAlignSlotLimit, and a
checkpointed re-fill would multiply the run time of a sweep of 1.7e10 cells."""
import numpy as np
import pytest

import affine_range_cases as arc
from affine_cases import checker  # noqa: F401
from align_cases import replay
from top_cases import numpy_top
from ungapped_cases import passing

pytestmark = pytest.mark.gpu

EINVAL = -22
POISON64 = -0x5A5A5A5A5A5A5A5B
POISON32 = -0x5A5A5A5B
POISON8 = 0x5A
CASES = [(name, gaps) for name in arc.TABLES for gaps in arc.GAPS]
NONEMPTY = np.array(arc.TLENS) > 0


def case_id(c):
    return f"{c[0]}{c[1][0]}_{c[1][1]}"


def to_dev(engine, packed, skew):
    """The bytes on the device at an address with addr % 2 == skew % 2 (torch aligns allocations to 512 bytes)."""
    t = engine.torch
    buf = t.zeros(len(packed) + skew + 16, dtype=t.uint8, device=f"cuda:{engine.device}")
    buf[skew:skew + len(packed)] = t.from_numpy(np.array(packed))
    d = buf[skew:skew + len(packed)]
    assert d.data_ptr() % 2 == skew % 2
    return d


def full(engine, shape, value, dtype="int64"):
    t = engine.torch
    return t.full(shape, value, dtype=getattr(t, dtype), device=f"cuda:{engine.device}")


def differ(got, want):
    got, want = np.asarray(got).reshape(-1, 3), np.asarray(want).reshape(-1, 3)
    bad = np.nonzero((got != want).any(axis=1))[0]
    return f"{len(bad)} entries differ, first {bad[0]}: {tuple(got[bad[0]])} vs {tuple(want[bad[0]])}" if len(bad) else ""


@pytest.fixture(scope="module")
def dev(engine):
    """Per table: the queries (odd base, so that query letters start at an odd address) and the database on the device, and its handle."""
    out = {}
    for name in arc.TABLES:
        s = arc.sequences(name)
        d_q, d_db = to_dev(engine, s["qpacked"], 1), to_dev(engine, s["packed"], 0)
        assert (d_q.data_ptr() + arc.QFRONT) % 2 == 1 and (d_db.data_ptr() + arc.FRONT) % 2 == 1
        out[name] = {"d_q": d_q, "d_db": d_db, "db": engine.prepare_db(d_db, s["offs"]), **s}
    yield out
    for d in out.values():
        d["db"].close()


# ---- 1, 2, 3: the search calls ----

@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_many_query_search(engine, checker, dev, case):  # noqa: F811
    name, gaps = case
    d, want = dev[name], arc.checked(checker, name, gaps)
    res = d["db"].search_affine_device(d["d_q"], d["qoffs"], (arc.table(name), *gaps), out=full(engine, (7 * 11 * 3,), POISON64))
    engine.synchronize()
    got = res.cpu().numpy()
    assert got.shape == (7, 11, 3) and not differ(got, want), f"{name} {gaps}: " + differ(got, want) + " (entry = query * 11 + target)"
    assert engine.get_option("last_search_multi_groups") == 1 and engine.get_option("last_search_multi_launches") >= 3


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_one_query_search_gives_the_same_rows(engine, checker, dev, case):  # noqa: F811
    name, gaps = case
    d, want = dev[name], arc.checked(checker, name, gaps)
    for q in (1, 4, 6):
        qlen = arc.QLENS[q]
        assert qlen in (63, 513, 2049)
        res = engine.search_affine_device(d["d_q"][int(d["qoffs"][q]):], qlen, d["d_db"], d["offs"], arc.table(name), *gaps, out=full(engine, (11, 3), POISON64))
        engine.synchronize()
        assert not differ(res.cpu().numpy(), want[q]), f"{name} {gaps} query {q}: " + differ(res.cpu().numpy(), want[q])
        assert engine.get_option("last_search_affine_kernel") in ((0,) if qlen <= 256 else (1,) if qlen <= 512 else (1, 2))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_pair_list_search(engine, checker, dev, case):  # noqa: F811
    name, gaps = case
    d, want = dev[name], arc.checked(checker, name, gaps)
    pairs = arc.pair_list()
    assert len(pairs) == 77 + 10 + 5 and (pairs[-5:] == -1).all() and len({tuple(p) for p in pairs[:87].tolist()}) == 77
    d_pairs = engine.torch.from_numpy(pairs.copy()).to(f"cuda:{engine.device}")
    res = d["db"].search_affine_pairs_device(d["d_q"], d["qoffs"], (arc.table(name), *gaps), d_pairs, out=full(engine, (len(pairs) * 3,), POISON64))
    engine.synchronize()
    got = res.cpu().numpy()
    gathered = want[pairs[:87, 0], pairs[:87, 1]]
    assert not differ(got[:87], gathered), f"{name} {gaps}: " + differ(got[:87], gathered) + f" (pairs {pairs[:87].tolist()})"
    assert not got[87:].any()                                                           # the {-1, -1} tail: zero over the poison
    assert engine.get_option("last_search_pairs_groups") == 1 and engine.get_option("last_search_pairs_chunks") == 1
    assert engine.get_option("last_search_pairs_launches") >= 1 + 2 + 3                 # profiles, two binning launches, a score launch per class


# ---- 4, 5: the pre-filter ----

def prefilter(engine, db, d_q, qoffs, sub, min_score, cap, lanes):
    """One call into poisoned outputs under prefilter_lanes = lanes: numpy (pairs (cap, 2), npairs, scores) and what the options say."""
    nq = len(qoffs) - 1
    out = (full(engine, (cap, 2), POISON64), full(engine, (1,), POISON64), full(engine, (nq, db.ntargets), POISON32, "int32"))
    engine.set_option("prefilter_lanes", lanes)
    try:
        pairs, n, scores = db.prefilter_ungapped_device(d_q, qoffs, sub, min_score, cap, want_scores=True, out=out)
        engine.synchronize()
        said = {k: engine.get_option("last_prefilter_" + k) for k in ("groups", "launches", "packed_launches")}
    finally:
        engine.set_option("prefilter_lanes", 0)
    return pairs.cpu().numpy(), int(n.item()), scores.cpu().numpy(), said


def check_list(pairs, n, want_pairs, cap):
    """n is the true count; the first min(n, cap) rows are distinct passing pairs; the rest is {-1, -1}."""
    assert n == len(want_pairs)
    k = min(n, cap)
    got, want = {tuple(p) for p in pairs[:k].tolist()}, {tuple(p) for p in want_pairs.tolist()}
    assert len(got) == k and got <= want and (n > cap or got == want)
    assert (pairs[k:] == -1).all()


def median_positive(want):
    pos = np.sort(want[want > 0])
    return int(pos[len(pos) // 2]) if len(pos) else 1


@pytest.mark.parametrize("lanes", [0, 32])
@pytest.mark.parametrize("name", arc.TABLES)
def test_prefilter(engine, dev, name, lanes):
    d, want, sub = dev[name], arc.ungapped(name), arc.table(name)
    m = median_positive(want)
    pairs, n, scores, said = prefilter(engine, d["db"], d["d_q"], d["qoffs"], sub, m, 77, lanes)
    assert scores.shape == (7, 11) and np.array_equal(scores, want), f"{name} lanes {lanes}: first (query, target) {np.argwhere(scores != want)[:3].tolist()}"
    check_list(pairs, n, passing(want, d["offs"], m), 77)
    assert said["groups"] == 1 and said["launches"] >= 3
    if lanes == 32:
        assert said["packed_launches"] == 0
    elif name == "floor":                                                               # no positive entry: max(largest, 0) = 0 packs every query
        assert said["packed_launches"] == said["launches"] and n == 0 and (pairs == -1).all() and not scores.any()
    else:                                                                               # 127 x min(qlen, 1100) <= 32767 for 1, 63, 256 and 257 letters alone
        assert 0 < said["packed_launches"] < said["launches"]
    # the second witness: gaps no alignment can pay leave Gotoh's H on the diagonals
    h = d["db"].search_affine_device(d["d_q"], d["qoffs"], (sub, -arc.LIMIT, 0)).cpu().numpy()[:, :, 1]
    assert np.array_equal(scores, h)


@pytest.mark.parametrize("lanes", [0, 32])
@pytest.mark.parametrize("name", ["full8", "corners", "ceiling"])
def test_prefilter_cuts_a_class_into_a_packed_and_a_32_bit_side(engine, dev, name, lanes):
    """Four queries of the 8-column class, two of which fit 16 bits (tests/affine_range_cases.py, cut_case)."""
    qpacked, qoffs, want = arc.cut_case(name)
    d = dev[name]
    m = median_positive(want)
    pairs, n, scores, said = prefilter(engine, d["db"], to_dev(engine, qpacked, 0), qoffs, arc.table(name), m, 44, lanes)
    assert np.array_equal(scores, want), f"{name} lanes {lanes}: first (query, target) {np.argwhere(scores != want)[:3].tolist()}"
    check_list(pairs, n, passing(want, d["offs"], m), 44)
    assert (said["launches"], said["packed_launches"]) == ((2, 1) if lanes == 0 else (1, 0))   # one class: a launch side per kind


@pytest.mark.parametrize("lanes", [0, 32])
@pytest.mark.parametrize("qlen", [258, 259])
def test_prefilter_halves(engine, qlen, lanes):
    """One 16-bit half at 127 x 258 = 32766 while the other half takes -128 at every cell, and the same with the halves swapped."""
    qpacked, qoffs, packed, offs, want = arc.halves_case(qlen)
    with engine.prepare_db(to_dev(engine, packed, 0), offs) as db:
        pairs, n, scores, said = prefilter(engine, db, to_dev(engine, qpacked, 0), qoffs, arc.table("corners"), 1, 4, lanes)
    assert np.array_equal(scores, want), (qlen, lanes, scores.tolist(), want.tolist())
    check_list(pairs, n, np.array([[0, 1], [0, 2]], np.int64), 4)
    assert said["launches"] == 1 and said["packed_launches"] == (1 if (qlen, lanes) == (258, 0) else 0)


# ---- 6: the selections ----

@pytest.mark.parametrize("top", [1, 4, 12])
@pytest.mark.parametrize("gaps", [(-11, -1), (0, 0)])
@pytest.mark.parametrize("name", ["full8", "corners", "ceiling"])
def test_top_and_top_prefiltered(engine, checker, dev, name, gaps, top):  # noqa: F811
    d, want, u = dev[name], arc.checked(checker, name, gaps), arc.ungapped(name)
    scoring = (arc.table(name), *gaps)
    for min_score in (0, 1):
        out = (full(engine, (7 * top * 3,), POISON64), full(engine, (7,), POISON64))
        hits, nhits = d["db"].search_affine_top_device(d["d_q"], d["qoffs"], scoring, top, min_score, out=out)
        engine.synchronize()
        want_hits, want_nhits = numpy_top(want, top, min_score)
        assert np.array_equal(hits.cpu().numpy(), want_hits) and np.array_equal(nhits.cpu().numpy(), want_nhits), (name, gaps, top, min_score)
        assert engine.get_option("last_search_top_chunks") == 1 and engine.get_option("last_search_top_kernel") == 0
    if name == "ceiling" and top >= 4:                                                  # ties between the two 300-letter and the two 64-letter targets
        assert want_hits[6, :4, 0].tolist() == [6, 5, 10, 9] and want_hits[1, :4, 0].tolist() == [2, 3, 4, 5]
    # a pair with an alignment of score >= 1 holds a positive entry, so its U is >= 1: the filter at 1 drops none of the hits above
    assert ((want[:, :, 1] >= 1) <= (u >= 1)).all()
    out = (full(engine, (7 * top * 3,), POISON64), full(engine, (7,), POISON64))
    hits, nhits, npairs = d["db"].search_affine_top_prefiltered_device(d["d_q"], d["qoffs"], scoring, 1, 77, top, 1, out=out)
    engine.synchronize()
    assert np.array_equal(hits.cpu().numpy(), want_hits) and np.array_equal(nhits.cpu().numpy(), want_nhits), (name, gaps, top)
    assert int(npairs.item()) == len(passing(u, d["offs"], 1))
    assert 0 < engine.get_option("last_prefilter_packed_launches") < engine.get_option("last_prefilter_launches")
    assert engine.get_option("last_top_pairs_kernel") == 0 and engine.get_option("last_top_pairs_launches") >= 1


# ---- 7: the alignments ----

def assert_alignment(query, target, sub, gaps, row, ops_row, want, what):
    erow, eops = want
    assert tuple(int(x) for x in row) == erow, f"{what}: {tuple(int(x) for x in row)} vs {erow}"
    ops = ops_row[:erow[6]].tobytes()
    assert ops == eops, f"{what}: ops differ"
    assert (ops_row[erow[6]:] == POISON8).all(), f"{what}: bytes behind nops were written"
    replay(query, target, sub, *gaps, row, ops)
    if gaps == (-arc.LIMIT, 0):
        assert set(ops) == {ord("M")}, what


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("gaps", arc.ALIGN_GAPS, ids=lambda g: f"{g[0]}_{g[1]}")
@pytest.mark.parametrize("name", arc.ALIGN_TABLES)
def test_alignments_whole_and_checkpointed(engine, checker, dev, name, gaps, mode):  # noqa: F811
    """mode 0: whole direction matrices; mode 1: checkpoint rows every 64 target letters, so that the 300- and 1100-letter hits cross
    several of them."""
    d, want, sub = dev[name], arc.aligned(checker, name, gaps), arc.table(name)
    rows_before = engine.get_option("align_checkpoint_rows")
    ckpt_before = engine.get_option("align_checkpoint")
    engine.set_option("align_checkpoint_rows", 64 if mode else 0)
    try:
        for q in arc.ALIGN_QUERIES:
            qlen = arc.QLENS[q]
            cap = qlen + 1100
            out = (full(engine, (4, 7), POISON64), full(engine, (4, cap), POISON8, "uint8"))
            aln, ops = engine.align_affine_device(d["d_q"][int(d["qoffs"][q]):], qlen, d["d_db"], d["offs"], sub, *gaps, arc.ALIGN_TARGETS, ops_cap=cap, out=out, checkpoint=mode)
            engine.synchronize()
            assert engine.get_option("last_align_affine_checkpointed") == mode and engine.get_option("last_align_affine_band_rows") == (64 if mode else 0)
            aln, ops = aln.cpu().numpy(), ops.cpu().numpy()
            for h, t in enumerate(arc.ALIGN_TARGETS):
                assert_alignment(d["queries"][q], d["targets"][t], sub, gaps, aln[h], ops[h], want[(q, t)], f"{name} {gaps} mode {mode} query {q} target {t}")
        # the same alignments from a (4, 4) hit table with one -1 entry
        hits = arc.hit_table()
        table = np.stack([hits, np.full_like(hits, 3), np.full_like(hits, 9)], axis=-1)  # only `target` is read
        qpacked, qoffs = arc.packed_of([d["queries"][q] for q in arc.ALIGN_QUERIES], 1, [0])
        cap = 2049 + 1100
        out = (full(engine, (16 * 7,), POISON64), full(engine, (16 * cap,), POISON8, "uint8"))
        d_hits = engine.torch.from_numpy(table.copy()).to(f"cuda:{engine.device}")
        aln, ops = d["db"].align_affine_hits_device(to_dev(engine, qpacked, 0), qoffs, (sub, *gaps), d_hits, None, ops_cap=cap, out=out, checkpoint=mode)
        engine.synchronize()
        assert engine.get_option("last_align_hits_checkpointed") == mode and engine.get_option("last_align_hits_band_rows") == (64 if mode else 0)
        assert engine.get_option("last_align_hits_launches") > 3
        aln, ops = aln.cpu().numpy(), ops.cpu().numpy()
        for a, q in enumerate(arc.ALIGN_QUERIES):
            for r in range(4):
                t = int(hits[a, r])
                if t < 0:
                    assert not aln[a, r].any() and (ops[a, r] == POISON8).all()
                else:
                    assert_alignment(d["queries"][q], d["targets"][t], sub, gaps, aln[a, r], ops[a, r], want[(q, t)], f"{name} {gaps} mode {mode} table entry {a, r}")
    finally:
        engine.set_option("align_checkpoint_rows", rows_before)
        engine.set_option("align_checkpoint", ckpt_before)
    assert engine.get_option("align_checkpoint") == ckpt_before and engine.get_option("align_checkpoint_rows") == rows_before


# ---- 8: scores just below 2^24, max_pos beyond 2^32 ----

@pytest.fixture(scope="module")
def near(engine):
    qpacked, qoffs, packed, offs, want, u = arc.near_limit_case()
    assert want[0, 0, 0] > 1 << 32 and arc.LIMIT - 127 <= want[0, 0, 1] < arc.LIMIT
    d_q, d_db = to_dev(engine, qpacked, 1), to_dev(engine, packed, 0)
    db = engine.prepare_db(d_db, offs)
    yield {"d_q": d_q, "qoffs": qoffs, "db": db, "want": want, "u": u, "scoring": (arc.near_table(), *arc.NEAR_GAPS)}
    db.close()


def test_near_limit_many_query_search(engine, near):
    res = near["db"].search_affine_device(near["d_q"], near["qoffs"], near["scoring"], out=full(engine, (2 * 3 * 3,), POISON64))
    engine.synchronize()
    assert not differ(res.cpu().numpy(), near["want"]), differ(res.cpu().numpy(), near["want"])
    assert engine.get_option("last_search_multi_launches") == 2                         # 7 letters and 132105: two classes


def test_near_limit_pair_list_search(engine, near):
    pairs = np.array([(0, 0), (1, 1), (0, 2), (0, 0)], np.int64)
    d_pairs = engine.torch.from_numpy(pairs).to(f"cuda:{engine.device}")
    res = near["db"].search_affine_pairs_device(near["d_q"], near["qoffs"], near["scoring"], d_pairs, out=full(engine, (4 * 3,), POISON64))
    engine.synchronize()
    want = near["want"][pairs[:, 0], pairs[:, 1]]
    assert not differ(res.cpu().numpy(), want), differ(res.cpu().numpy(), want)
    assert engine.get_option("last_search_pairs_launches") == 1 + 2 + 2


def test_near_limit_prefilter(engine, near):
    pairs, n, scores, said = prefilter(engine, near["db"], near["d_q"], near["qoffs"], near["scoring"][0], 1, 6, 0)
    assert np.array_equal(scores, near["u"]) and scores[0, 0] == 127 * arc.NEAR_L, scores.tolist()
    check_list(pairs, n, np.array([[0, 0], [0, 1], [1, 0], [1, 1]], np.int64), 6)
    assert said["launches"] == 2 and said["packed_launches"] == 1                       # 127 x 7 fits 16 bits; the long query's launch runs on 32-bit lanes


def test_near_limit_one_step_over(engine, swamd):
    """A handle whose longest target has L + 1 letters: 127 (L + 1) reaches 2^24, every call refuses and writes nothing."""
    qpacked, qoffs, packed, offs, _, _ = arc.near_limit_case(arc.NEAR_L + 1)
    d_q = to_dev(engine, qpacked, 1)
    scoring = (arc.near_table(), *arc.NEAR_GAPS)
    res = full(engine, (2 * 3 * 3,), POISON64)
    out = (full(engine, (6, 2), POISON64), full(engine, (1,), POISON64), full(engine, (2, 3), POISON32, "int32"))
    d_pairs = engine.torch.from_numpy(np.array([(0, 0), (1, 1)], np.int64)).to(f"cuda:{engine.device}")
    with engine.prepare_db(to_dev(engine, packed, 0), offs) as db:
        for call in (lambda: db.search_affine_device(d_q, qoffs, scoring, out=res),
                     lambda: db.search_affine_pairs_device(d_q, qoffs, scoring, d_pairs, out=res),
                     lambda: db.prefilter_ungapped_device(d_q, qoffs, scoring[0], 1, 6, want_scores=True, out=out)):
            with pytest.raises(swamd.SwError) as e:
                call()
            assert e.value.code == EINVAL and "reaches 2^24" in str(e.value)
        engine.synchronize()
    assert bool((res == POISON64).all()) and bool((out[0] == POISON64).all()) and bool((out[1] == POISON64).all()) and bool((out[2] == POISON32).all())


def test_one_step_over_the_gap_limit(engine, swamd, dev):
    """gap_open + gap_extend = -2^24 - 1: refused by every call that takes gap costs, nothing written (-2^24 itself runs in the cases above)."""
    d = dev["full8"]
    res = full(engine, (92 * 3,), POISON64)
    hits_out = (full(engine, (7 * 2 * 3,), POISON64), full(engine, (7,), POISON64))
    aln_out = (full(engine, (7 * 2 * 7,), POISON64), None)
    d_pairs = engine.torch.from_numpy(arc.pair_list()).to(f"cuda:{engine.device}")
    d_hits = full(engine, (7, 2, 3), 4)
    for go, ge in [(-arc.LIMIT, -1), (-1, -arc.LIMIT), (-arc.LIMIT - 1, 0), (0, -arc.LIMIT - 1)]:
        scoring = (arc.table("full8"), go, ge)
        for call in (lambda: d["db"].search_affine_device(d["d_q"], d["qoffs"], scoring, out=res),
                     lambda: d["db"].search_affine_pairs_device(d["d_q"], d["qoffs"], scoring, d_pairs, out=res),
                     lambda: d["db"].search_affine_top_device(d["d_q"], d["qoffs"], scoring, 2, 0, out=hits_out),
                     lambda: d["db"].search_affine_top_prefiltered_device(d["d_q"], d["qoffs"], scoring, 1, 77, 2, 0, out=hits_out),
                     lambda: d["db"].align_affine_hits_device(d["d_q"], d["qoffs"], scoring, d_hits, None, out=aln_out)):
            with pytest.raises(swamd.SwError) as e:
                call()
            assert e.value.code == EINVAL and "below -2^24" in str(e.value)
    engine.synchronize()
    assert bool((res == POISON64).all()) and all(bool((x == POISON64).all()) for x in hits_out) and bool((aln_out[0] == POISON64).all())
