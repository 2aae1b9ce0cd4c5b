"""GPU: the position-specific calls at the edges of their value range and of their alphabet -- the case table of
tests/pssm_range_cases.py, whose expectations come from the independent checker alone (tests/test_pssm_range_host.py asserts the
table's conditions on it).  Every matrix lies at an odd address between pads of 127, every output is carved out of a poisoned arena
(tests/buffer_cases.py) whose guards are checked, equality is exact, and the route of every call is read from the "last_*" options."""
import numpy as np
import pytest

import pssm_cases
import pssm_range_cases as prc
from affine_cases import checker  # noqa: F401
from align_cases import replay
from buffer_cases import POISON, POISON64, Arena, arena_bytes, assert_guards

pytestmark = pytest.mark.gpu

EINVAL = -22
PAD = 4096                         # bytes of 127 in front of and behind the matrix
NQ, NT = len(prc.QLENS), len(prc.TLENS)


def _dev(engine):
    return f"cuda:{engine.device}"


def place_matrix(engine, m, front):
    """The matrix in an arena of its own at an ODD address, 127s in front of it, behind it and in the `front` unused columns before
    qoffsets[0]; all of it must stay as it is.  Returns (arena, int8 tensor that starts at column 0)."""
    t = engine.torch
    m = m.copy()
    m[:front] = 127
    inp = Arena(t, _dev(engine), arena_bytes(m.size + 2 * PAD))
    d, _ = inp.place(m.view(np.uint8).reshape(-1), align=64, skew=1, front=np.full(PAD, 127, np.uint8), back=np.full(PAD, 127, np.uint8), name="pssm")
    assert d.data_ptr() % 2 == 1
    return inp, d.view(t.int8)


def carve_i64(arena, n, name):
    c = arena.carve(n * 8, align=8, name=name)
    return arena.view(c, arena.torch.int64, (n,))


def differ(got, want):
    got, want = np.asarray(got).reshape(-1, 3), np.asarray(want).reshape(-1, 3)
    if got.shape != want.shape:
        return f"shape {got.shape} vs {want.shape}"
    bad = np.nonzero((got != want).any(axis=1))[0]
    return f"{len(bad)} entries differ, first {bad[0]}: {tuple(got[bad[0]])} vs {tuple(want[bad[0]])}" if len(bad) else ""


@pytest.fixture(scope="module")
def dev(engine):
    """Per (matrix kind, letters), on first use: the matrix at its odd address, the database behind an odd offsets[0] and its handle."""
    made = {}

    def get(kind, n):
        if (kind, n) not in made:
            w = prc.world(kind, n)
            inp, d_pssm = place_matrix(engine, w.matrix, prc.QFRONT)
            d_db = engine.torch.from_numpy(w.packed.copy()).to(_dev(engine))
            assert (d_db.data_ptr() + prc.FRONT) % 2 == 1
            made[(kind, n)] = {"w": w, "inp": inp, "d_pssm": d_pssm, "d_db": d_db, "db": engine.prepare_db(d_db, w.offs),
                               "out": Arena(engine.torch, _dev(engine), arena_bytes(NQ * NT * 24, NQ * 12 * 24, NQ * 8))}
        return made[(kind, n)]
    yield get
    for d in made.values():
        d["db"].close()


def search(engine, d, qoffs, scoring, lanes, d_pssm=None, nq=NQ):
    """sw_db_search_pssm under search_lanes = lanes into a fresh carve of d's arena: (numpy table, what the options say)."""
    out = d["out"]
    out.reset()
    engine.set_option("search_lanes", lanes)
    try:
        res = d["db"].search_pssm_device(d["d_pssm"] if d_pssm is None else d_pssm, qoffs, scoring, out=carve_i64(out, nq * NT * 3, "results"))
        engine.synchronize()
        said = {k: engine.get_option("last_search_multi_" + k) for k in ("launches", "packed_launches", "groups")}
    finally:
        engine.set_option("search_lanes", 32)
    got = res.cpu().numpy()
    assert_guards(out)
    return got, said


# ---- the search, on both kinds of lanes ----

@pytest.mark.parametrize("case", prc.CASES, ids=prc.case_id)
def test_search_equals_the_checker_under_both_lanes(engine, checker, dev, case):  # noqa: F811
    kind, sc, n = case
    d = dev(kind, n)
    w = d["w"]
    routes = set()
    for gaps in prc.GAPS:
        want = prc.checked(checker, case, gaps)
        for lanes in (32, 16):
            got, said = search(engine, d, w.qoffs, w.scoring(sc, gaps), lanes)
            assert got.shape == (NQ, NT, 3) and not differ(got, want), f"{prc.case_id(case)} {gaps} lanes {lanes}: " + differ(got, want) + " (entry = query * 11 + target)"
            launches, packed = prc.lane_sides(prc.QLENS, sc[1], gaps) if lanes == 16 else (3, 0)
            assert (said["launches"], said["packed_launches"], said["groups"]) == (launches, packed, 1), (gaps, lanes, said)
            routes.add((lanes, packed > 0, packed < launches))
    # condition 6 of the table: packed launches alone, both kinds in one call (smax = 127), and 32-bit lanes under search_lanes = 16
    assert (16, True, sc[1] == 127) in routes and (16, False, True) in routes and (32, False, True) in routes
    assert_guards(d["inp"])


@pytest.mark.parametrize("n", prc.MAIN_NLETTERS)
@pytest.mark.parametrize("kind", ["full8", "corners", "ceiling"])
def test_search_cuts_a_class_into_a_packed_and_a_32_bit_side(engine, checker, dev, kind, n):  # noqa: F811
    """Four queries of the 8-column class, two of which fit 16 bits under smax = 127 (tests/pssm_range_cases.py, cut_case)."""
    d = dev(kind, n)
    w = d["w"]
    names, qoffs = prc.cut_case(kind, n)
    inp, d_pssm = place_matrix(engine, w.types[names], 1)
    for sc in ((-128, 127), prc.CLAMPING):
        gaps = prc.GAPS[0]
        want = prc.cut_checked(checker, kind, n, sc, gaps)
        for lanes in (32, 16):
            got, said = search(engine, d, qoffs, w.scoring(sc, gaps), lanes, d_pssm=d_pssm, nq=4)
            assert not differ(got, want), f"{kind} {n} {sc} lanes {lanes}: " + differ(got, want)
            assert (said["launches"], said["packed_launches"]) == ((1, 0) if lanes == 32 else (2, 1) if sc[1] == 127 else (1, 1))
    assert_guards(inp)


@pytest.mark.parametrize("case", [c for c in prc.CASES if c[0] == "full8" and c[1] == (-128, 127)], ids=prc.case_id)
def test_search_in_several_groups(engine, checker, dev, case):  # noqa: F811
    """search_profile_mib = 1: the profiles of 2115 columns do not fit one group."""
    kind, sc, n = case
    d = dev(kind, n)
    w = d["w"]
    gaps = prc.GAPS[0]
    want = prc.checked(checker, case, gaps)
    try:
        engine.set_option("search_profile_mib", 1)
        for lanes in (32, 16):
            got, said = search(engine, d, w.qoffs, w.scoring(sc, gaps), lanes)
            assert not differ(got, want), f"{prc.case_id(case)} lanes {lanes}: " + differ(got, want)
            assert said["groups"] > 1 and (said["packed_launches"] > 0) == (lanes == 16)
    finally:
        engine.set_option("search_profile_mib", 256)
    assert_guards(d["inp"])


# ---- the selection ----

@pytest.mark.parametrize("top", [1, 4, 12])
@pytest.mark.parametrize("case", prc.TOP_CASES, ids=prc.case_id)
def test_top_equals_the_rank_order_of_the_checkers_table(engine, checker, dev, case, top):  # noqa: F811
    kind, sc, n = case
    d = dev(kind, n)
    w, out = d["w"], d["out"]
    assert top in (1, 4) or top > NT
    for gaps in prc.TOP_GAPS:
        full = prc.checked(checker, case, gaps)
        positive = int(np.median(full[:, :, 1][full[:, :, 1] > 0]))
        assert positive > 0
        for min_score in (0, positive):
            want_hits, want_n = pssm_cases.rank_order(full, top, min_score)
            assert min_score == 0 or 0 < (full[:, :, 1] >= min_score).sum() < NQ * NT      # the positive value keeps some and drops some
            for lanes in (32, 16):
                out.reset()
                o = (carve_i64(out, NQ * top * 3, "hits"), carve_i64(out, NQ, "nhits"))
                engine.set_option("search_lanes", lanes)
                try:
                    hits, nhits = d["db"].search_pssm_top_device(d["d_pssm"], w.qoffs, w.scoring(sc, gaps), top, min_score, out=o)
                    engine.synchronize()
                    assert engine.get_option("last_search_top_chunks") == 1
                    assert (engine.get_option("last_search_multi_packed_launches") > 0) == (lanes == 16)
                finally:
                    engine.set_option("search_lanes", 32)
                assert np.array_equal(hits.cpu().numpy().reshape(NQ, top, 3), want_hits) and np.array_equal(nhits.cpu().numpy(), want_n), (gaps, min_score, lanes)
                assert_guards(out)
    assert_guards(d["inp"])


# ---- the alignments ----

@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("gaps", prc.ALIGN_GAPS, ids=lambda g: f"{g[0]}_{g[1]}")
@pytest.mark.parametrize("case", prc.ALIGN_CASES, ids=prc.case_id)
def test_alignments_whole_and_checkpointed(engine, checker, dev, case, gaps, mode):  # noqa: F811
    """mode 0: whole direction matrices; mode 1: checkpoint rows every 64 target letters, so that the 300- and 1100-letter hits cross
    several of them."""
    kind, sc, n = case
    d = dev(kind, n)
    w, want = d["w"], prc.aligned(checker, case, gaps)
    table = w.table(*sc)
    t = engine.torch
    hits = prc.hit_table()
    hit_rows = np.stack([hits, np.full_like(hits, 3), np.full_like(hits, 9)], axis=-1)     # only `target` is read
    m, qoffs = prc.align_matrix(w)
    inp, d_pssm = place_matrix(engine, m, 1)
    cap = max(prc.QLENS) + max(prc.TLENS)
    out = Arena(t, _dev(engine), arena_bytes(16 * 56, 16 * cap))
    d_aln = carve_i64(out, 16 * 7, "aln")
    c = out.carve(16 * cap, name="ops")
    rows_before, ckpt_before = engine.get_option("align_checkpoint_rows"), engine.get_option("align_checkpoint")
    engine.set_option("align_checkpoint_rows", 64 if mode else 0)
    try:
        aln, ops = d["db"].align_pssm_hits_device(d_pssm, qoffs, w.scoring(sc, gaps), t.from_numpy(hit_rows.copy()).to(_dev(engine)), None, ops_cap=cap,
                                                  out=(d_aln, out.view(c, t.uint8, (16 * cap,))), checkpoint=mode)
        engine.synchronize()
        assert engine.get_option("last_align_hits_checkpointed") == mode and engine.get_option("last_align_hits_band_rows") == (64 if mode else 0)
        assert engine.get_option("last_align_hits_launches") > 3
    finally:
        engine.set_option("align_checkpoint_rows", rows_before)
        engine.set_option("align_checkpoint", ckpt_before)
    aln, ops = aln.cpu().numpy().reshape(4, 4, 7), ops.cpu().numpy().reshape(4, 4, cap)
    for a, q in enumerate(prc.ALIGN_QUERIES):
        for r in range(4):
            k = int(hits[a, r])
            if k < 0:
                assert not aln[a, r].any() and (ops[a, r] == POISON).all(), (a, r)
                continue
            row, eops = want[(q, k)]
            assert tuple(int(x) for x in aln[a, r]) == row, (a, r, tuple(aln[a, r]), row)
            assert ops[a, r, :row[6]].tobytes() == eops and (ops[a, r, row[6]:] == POISON).all(), (a, r)
            replay(w.query(q), w.targets[k], table, *gaps, row, eops)
    assert_guards(out)
    assert_guards(inp)


# ---- one step outside the scoring object ----

def test_a_scoring_outside_its_range_is_refused_without_a_write(engine, swamd, dev):
    d = dev("full8", 4)
    w, t = d["w"], engine.torch
    out = Arena(t, _dev(engine), arena_bytes(NQ * NT * 24, NQ * 24, NQ * 8, NQ * 56, NQ * 64))
    res, hits, nhits, aln = carve_i64(out, NQ * NT * 3, "results"), carve_i64(out, NQ * 3, "hits"), carve_i64(out, NQ, "nhits"), carve_i64(out, NQ * 7, "aln")
    c_ops = out.carve(NQ * 64, name="ops")
    ops = out.view(c_ops, t.uint8, (NQ * 64,))
    for c in out.carves:
        out.must_stay(c)
    d_hits = t.zeros((NQ, 1, 3), dtype=t.int64, device=_dev(engine))
    d_hits[:, :, 0] = 5
    for other, smax in [(-128, -1), (-128, 128), (-129, 127), (2, 1), (128, 127), (1, 0)]:
        scoring = (w.letters, other, smax, -11, -1)
        for call in (lambda: d["db"].search_pssm_device(d["d_pssm"], w.qoffs, scoring, out=res),
                     lambda: d["db"].search_pssm_top_device(d["d_pssm"], w.qoffs, scoring, 1, 0, out=(hits, nhits)),
                     lambda: d["db"].align_pssm_hits_device(d["d_pssm"], w.qoffs, scoring, d_hits, None, ops_cap=64, out=(aln, ops))):
            with pytest.raises(swamd.SwError) as e:
                call()
            assert e.value.code == EINVAL and ("smax" in str(e.value) or "other" in str(e.value)), (other, smax, str(e.value))
    engine.synchronize()
    assert_guards(out)                                             # every output is still poison
    assert int(res[0]) == POISON64 and int(ops[0]) == POISON
    assert_guards(d["inp"])
