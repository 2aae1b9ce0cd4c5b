"""GPU: many queries against a prepared database (sw_db_create / sw_db_search_affine, Engine.prepare_db / Database.search_affine) against
sw_search_affine_device query by query ON THE SAME DEVICE BUFFERS and against the host leg (sw_search_affine_multi_host, which
tests/test_search_multi_host.py holds against the independent checker) -- exact equality everywhere."""
import numpy as np
import pytest

from affine_cases import PROTEIN
from buffer_cases import POISON, Arena, arena_bytes, assert_guards, live_head, live_tail

pytestmark = pytest.mark.gpu

QLENS = [1, 4, 255, 256, 257, 512, 513, 1024, 1025, 2049]        # every class (4 / 8 / 16 columns per lane), one strip and several
TLENS = [0, 1, 63, 64, 65, 127, 300, 1100, 64, 0, 1, 300, 65, 127, 63]
QFRONT, FRONT = 4, 3                                             # qoffsets[0], offsets[0]


def pack(lens, front, rng, alpha):
    offs = np.zeros(len(lens) + 1, np.int64)
    offs[0] = front
    offs[1:] = front + np.cumsum(lens)
    return rng.choice(alpha, max(1, int(offs[-1]))).astype(np.uint8), offs


def to_dev(engine, packed, skew):
    """The bytes on the device at an address with addr % 2 == skew % 2 (torch aligns allocations to 512 bytes)."""
    t = engine.torch
    buf = t.zeros(len(packed) + skew + 16, dtype=t.uint8, device=f"cuda:{engine.device}")
    buf[skew:skew + len(packed)] = t.from_numpy(packed.copy())
    d = buf[skew:skew + len(packed)]
    assert d.data_ptr() % 2 == skew % 2
    return d


def singles(engine, d_q, qoffs, d_db, offs, scoring):
    """sw_search_affine_device query by query on the same buffers: (nqueries, ntargets, 3)"""
    out = [engine.search_affine_device(d_q[int(qoffs[q]):], int(qoffs[q + 1] - qoffs[q]), d_db, offs, *scoring) for q in range(len(qoffs) - 1)]
    engine.synchronize()
    return np.stack([o.cpu().numpy() for o in out])


def poisoned(engine, nq, nt):
    t = engine.torch
    return t.full((max(3, nq * nt * 3),), -0x5A5A5A5A5A5A5A5B, dtype=t.int64, device=f"cuda:{engine.device}")


def differ(got, want):
    bad = np.argwhere((got != want).any(axis=2))
    return f"{len(bad)} pairs differ, first (query, target) {tuple(bad[0])}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}" if len(bad) else ""


@pytest.fixture(scope="module")
def scorings(swamd):
    rng = np.random.default_rng(5)
    n = len(PROTEIN)
    sc = rng.integers(-8, 13, (n, n)).astype(np.int8)            # asymmetric over the 24 letters
    sc[np.arange(n), np.arange(n)] = rng.integers(4, 13, n).astype(np.int8)
    assert not np.array_equal(sc, sc.T)
    return {"affine": (swamd.submat_from_letters(PROTEIN, sc, -8), -11, -1), "linear": (swamd.submat_match(3, -3), 0, -2)}


@pytest.fixture(scope="module")
def case(engine, swamd, scorings):
    """The mixed case: the ten query lengths shuffled, the targets, both on the device (query base odd), the handle, and per scoring the
    host leg's results -- computed once, never changed."""
    rng = np.random.default_rng(2024)
    qlens = list(QLENS)
    rng.shuffle(qlens)
    assert qlens != QLENS
    qpacked, qoffs = pack(qlens, QFRONT, rng, PROTEIN[:20])
    packed, offs = pack(TLENS, FRONT, rng, PROTEIN[:20])
    d_q, d_db = to_dev(engine, qpacked, 1), to_dev(engine, packed, 0)
    assert (d_q.data_ptr() + QFRONT) % 2 == 1
    db = engine.prepare_db(d_db, offs)
    host = {k: swamd.search_affine_multi_host((qpacked, qoffs), (packed, offs), s) for k, s in scorings.items()}
    yield {"qlens": qlens, "qpacked": qpacked, "qoffs": qoffs, "packed": packed, "offs": offs, "d_q": d_q, "d_db": d_db, "db": db, "host": host}
    db.close()


def test_info(case):
    assert case["db"].info() == {"ntargets": len(TLENS), "nonempty": sum(1 for x in TLENS if x), "longest": 1100, "letters": sum(TLENS)}


@pytest.mark.parametrize("which", ["affine", "linear"])
def test_mixed_queries_equal_single_calls_and_host_leg(engine, case, scorings, which):
    res = case["db"].search_affine_device(case["d_q"], case["qoffs"], scorings[which], out=poisoned(engine, len(QLENS), len(TLENS)))
    engine.synchronize()
    got = res.cpu().numpy()
    assert got.shape == (len(QLENS), len(TLENS), 3)
    # one launch per class: the 16-column kernel keeps two workgroups per CU on gfx950 (136 VGPRs), so the long queries do not fall back to 8
    assert engine.get_option("last_search_multi_groups") == 1 and engine.get_option("last_search_multi_launches") == 3
    assert not differ(got, case["host"][which]), "host leg: " + differ(got, case["host"][which])
    one = singles(engine, case["d_q"], case["qoffs"], case["d_db"], case["offs"], scorings[which])
    assert not differ(got, one), "single calls: " + differ(got, one)
    assert (got[:, [k for k, x in enumerate(TLENS) if x == 0], :] == 0).all()       # empty targets over the poison
    assert (got[:, :, 1] > 0).sum() > len(QLENS) * 8


def test_gap_open_zero_match_table_equals_linear_search(engine, case, scorings):
    got = case["db"].search_affine_device(case["d_q"], case["qoffs"], scorings["linear"]).cpu().numpy()
    qoffs = case["qoffs"]
    for q in range(len(QLENS)):
        lin = engine.search_device(case["d_q"][int(qoffs[q]):], int(qoffs[q + 1] - qoffs[q]), case["d_db"], case["offs"], (3, -3, -2)).cpu().numpy()
        assert np.array_equal(got[q], lin), f"query {q} of length {case['qlens'][q]}"


@pytest.mark.parametrize("q", [0, 5, 9])
def test_one_query(engine, case, scorings, q):
    qoffs = case["qoffs"][q:q + 2]
    got = case["db"].search_affine_device(case["d_q"], qoffs, scorings["affine"], out=poisoned(engine, 1, len(TLENS))).cpu().numpy()
    assert got.shape == (1, len(TLENS), 3) and not differ(got, case["host"]["affine"][q:q + 1])
    assert engine.get_option("last_search_multi_launches") == 1


def test_many_short_queries_against_few_targets(engine, swamd, scorings):
    """300 queries of length 8 against 5 targets: 1500 items in one launch, more than any single search of this file has."""
    rng = np.random.default_rng(300)
    qpacked, qoffs = pack([8] * 300, 0, rng, PROTEIN[:20])
    packed, offs = pack([40, 9, 300, 64, 17], FRONT, rng, PROTEIN[:20])
    d_q, d_db = to_dev(engine, qpacked, 1), to_dev(engine, packed, 0)
    with engine.prepare_db(d_db, offs) as db:
        got = db.search_affine_device(d_q, qoffs, scorings["affine"], out=poisoned(engine, 300, 5)).cpu().numpy()
        assert engine.get_option("last_search_multi_launches") == 1 and engine.get_option("last_search_multi_grid") == 375
    want = swamd.search_affine_multi_host((qpacked, qoffs), (packed, offs), scorings["affine"])
    assert not differ(got, want), differ(got, want)
    one = singles(engine, d_q, qoffs, d_db, offs, scorings["affine"])
    assert not differ(got, one), differ(got, one)


@pytest.mark.parametrize("name,qlo,qhi,nq,tlens", [
    ("4 columns per lane, one strip", 1, 256, 300, [40, 9, 300, 64, 17, 1, 0, 65] * 5),            # 300 x 35 = 10 500 items
    ("8 columns per lane, one strip", 257, 512, 120, [30, 7, 64, 65, 0, 120] * 10),               # 120 x 50 = 6 000 items
    ("16 columns per lane, one to three strips", 513, 2100, 60, [33, 5, 64, 0, 65, 90, 17] * 10),  # 60 x 60 = 3 600 items
])
def test_every_wave_takes_several_items(engine, swamd, scorings, name, qlo, qhi, nq, tlens):
    """More items in ONE launch than the launch has waves, query lengths mixed inside the class and target lengths mixed: every wave
    runs the loop around the sweep again with another query descriptor and another target -- the arg-max state, the profile descriptor,
    M, the strips and the boundary column all start anew per item.  (Resident waves on 256 CUs: 6144 / 5120 / 3072 at 4 / 8 / 16
    columns per lane; the assertion below does not depend on those figures.)"""
    rng = np.random.default_rng(nq)
    qlens = [qlo, qhi] + list(rng.integers(qlo, qhi + 1, nq - 2))
    rng.shuffle(qlens)
    qpacked, qoffs = pack(qlens, QFRONT, rng, PROTEIN[:20])
    packed, offs = pack(tlens, FRONT, rng, PROTEIN[:20])
    d_q, d_db = to_dev(engine, qpacked, 1), to_dev(engine, packed, 0)
    with engine.prepare_db(d_db, offs) as db:
        got = db.search_affine_device(d_q, qoffs, scorings["affine"], out=poisoned(engine, nq, len(tlens))).cpu().numpy()
        items = nq * db.info()["nonempty"]
        assert engine.get_option("last_search_multi_launches") == 1, name
        assert items > 4 * engine.get_option("last_search_multi_grid") > 0, name     # four waves per workgroup: more items than waves
    want = swamd.search_affine_multi_host((qpacked, qoffs), (packed, offs), scorings["affine"])
    assert not differ(got, want), name + ": " + differ(got, want)


def test_two_queries_against_many_targets(engine, swamd, scorings):
    rng = np.random.default_rng(3000)
    lens = rng.integers(0, 90, 3000)
    qpacked, qoffs = pack([130, 600], QFRONT, rng, PROTEIN[:20])
    packed, offs = pack(lens, FRONT, rng, PROTEIN[:20])
    d_q, d_db = to_dev(engine, qpacked, 1), to_dev(engine, packed, 1)
    with engine.prepare_db(d_db, offs) as db:
        got = db.search_affine_device(d_q, qoffs, scorings["affine"], out=poisoned(engine, 2, 3000)).cpu().numpy()
    one = singles(engine, d_q, qoffs, d_db, offs, scorings["affine"])
    assert not differ(got, one), differ(got, one)
    want = swamd.search_affine_multi_host((qpacked, qoffs), (packed, offs), scorings["affine"])
    assert not differ(got, want), differ(got, want)


def test_profile_budget_of_one_mib_cuts_groups(engine, case, scorings):
    """The ten profiles take 257 x 9216 bytes = 2.3 MiB (2.0 MiB and a little where the long queries run at 8 columns per lane): under a
    budget of 1 MiB that is at least three groups, whatever the order; the results do not change."""
    assert engine.get_option("search_profile_mib") == 256
    engine.set_option("search_profile_mib", 1)
    try:
        got = case["db"].search_affine_device(case["d_q"], case["qoffs"], scorings["affine"], out=poisoned(engine, len(QLENS), len(TLENS))).cpu().numpy()
        assert engine.get_option("last_search_multi_groups") >= 3
    finally:
        engine.set_option("search_profile_mib", 256)
    assert not differ(got, case["host"]["affine"]), differ(got, case["host"]["affine"])
    got = case["db"].search_affine_device(case["d_q"], case["qoffs"], scorings["affine"]).cpu().numpy()      # the default again
    assert engine.get_option("last_search_multi_groups") == 1 and not differ(got, case["host"]["affine"])
    with pytest.raises(Exception):
        engine.set_option("search_profile_mib", 0)


def test_two_handles_alive_at_once(engine, swamd, case, scorings):
    rng = np.random.default_rng(22)
    packed2, offs2 = pack([200, 0, 31, 700, 64], 9, rng, PROTEIN[:20])
    d_db2 = to_dev(engine, packed2, 1)
    want2 = swamd.search_affine_multi_host((case["qpacked"], case["qoffs"]), (packed2, offs2), scorings["affine"])
    db2 = engine.prepare_db(d_db2, offs2)
    try:
        for _ in range(2):
            a = case["db"].search_affine_device(case["d_q"], case["qoffs"], scorings["affine"], out=poisoned(engine, len(QLENS), len(TLENS)))
            b = db2.search_affine_device(case["d_q"], case["qoffs"], scorings["affine"], out=poisoned(engine, len(QLENS), 5))
            engine.synchronize()
            assert not differ(a.cpu().numpy(), case["host"]["affine"]) and not differ(b.cpu().numpy(), want2)
    finally:
        db2.close()
    got = case["db"].search_affine_device(case["d_q"], case["qoffs"], scorings["affine"]).cpu().numpy()      # the other handle lives on
    assert not differ(got, case["host"]["affine"])


def test_one_handle_on_two_streams_one_after_the_other(engine, case, scorings):
    t = engine.torch
    s1, s2 = t.cuda.Stream(device=engine.device), t.cuda.Stream(device=engine.device)
    o1, o2 = poisoned(engine, len(QLENS), len(TLENS)), poisoned(engine, len(QLENS), len(TLENS))
    t.cuda.synchronize()
    with t.cuda.stream(s1):
        r1 = case["db"].search_affine_device(case["d_q"], case["qoffs"], scorings["affine"], out=o1)
    with t.cuda.stream(s2):
        r2 = case["db"].search_affine_device(case["d_q"], case["qoffs"], scorings["linear"], out=o2)
    s1.synchronize()
    s2.synchronize()
    assert not differ(r1.cpu().numpy(), case["host"]["affine"]) and not differ(r2.cpu().numpy(), case["host"]["linear"])


def test_handle_reused_after_the_results_are_poisoned_again(engine, case, scorings):
    out = poisoned(engine, len(QLENS), len(TLENS))
    for which in ("affine", "linear", "affine"):
        out.fill_(-0x5A5A5A5A5A5A5A5B)
        got = case["db"].search_affine_device(case["d_q"], case["qoffs"], scorings[which], out=out).cpu().numpy()
        assert not differ(got, case["host"][which]), which


def test_empty_handle(engine, case, scorings):
    with engine.prepare_db(case["d_db"], np.array([7], np.int64)) as db:
        assert db.info() == {"ntargets": 0, "nonempty": 0, "longest": 0, "letters": 0}
        out = poisoned(engine, len(QLENS), 0)
        got = db.search_affine_device(case["d_q"], case["qoffs"], scorings["affine"], out=out)
        engine.synchronize()
        assert got.shape == (len(QLENS), 0, 3) and bool((out == -0x5A5A5A5A5A5A5A5B).all())     # nothing launched, nothing written
    with engine.prepare_db(case["d_db"], case["offs"]) as db:                                      # and no query
        out = poisoned(engine, 1, len(TLENS))
        assert db.search_affine_device(case["d_q"], np.array([4], np.int64), scorings["affine"], out=out).shape == (0, len(TLENS), 3)
        engine.synchronize()
        assert bool((out == -0x5A5A5A5A5A5A5A5B).all())


def test_handle_of_only_empty_targets(engine, case, scorings):
    with engine.prepare_db(case["d_db"], np.array([5, 5, 5, 5], np.int64)) as db:
        assert db.info() == {"ntargets": 3, "nonempty": 0, "longest": 0, "letters": 0}
        got = db.search_affine_device(case["d_q"], case["qoffs"], scorings["affine"], out=poisoned(engine, len(QLENS), 3)).cpu().numpy()
        assert got.shape == (len(QLENS), 3, 3) and (got == 0).all()


def test_argument_errors_on_the_device(engine, swamd, case, scorings):
    db, d_q = case["db"], case["d_q"]
    for qoffs in ([4, 4], [4, 2], [-1, 3], [0, 1 << 20]):
        with pytest.raises(swamd.SwError) as e:
            db.search_affine_device(d_q, np.array(qoffs, np.int64), scorings["affine"])
        assert e.value.code == -22
    sub = scorings["affine"][0]
    for go, ge in ((1, -1), (-1, 1), (-(1 << 24), -1)):
        with pytest.raises(swamd.SwError):
            db.search_affine_device(d_q, case["qoffs"], (sub, go, ge))
    with pytest.raises(ValueError, match="out must be"):                         # a result tensor too small for nqueries x ntargets: refused before the call
        db.search_affine_device(d_q, case["qoffs"], scorings["affine"], out=poisoned(engine, len(QLENS) - 1, len(TLENS)))
    with pytest.raises(swamd.SwError):                                           # the offsets errors of sw_search_device, at sw_db_create
        engine.prepare_db(case["d_db"], np.array([3, 9, 5], np.int64))
    got = db.search_affine_device(d_q, case["qoffs"], scorings["affine"]).cpu().numpy()          # the handle is as good as before
    assert not differ(got, case["host"]["affine"])


def test_buffer_contract(engine, case, scorings):
    """Guard bytes before and after d_results and the query buffer stay untouched, the inputs keep their letters, every poisoned result
    entry is overwritten.  The queries sit between live letters at an odd address, the database likewise."""
    torch = engine.torch
    dev = f"cuda:{engine.device}"
    qpacked, qoffs, packed, offs = case["qpacked"], case["qoffs"], case["packed"], case["offs"]
    nq, nt = len(QLENS), len(TLENS)
    inp = Arena(torch, dev, arena_bytes(len(qpacked) + 128, len(packed) + 128))
    d_q, _ = inp.place(qpacked, 64, 3, front=live_head(qpacked[QFRONT:], 64), back=live_tail(qpacked, 64), name="queries")
    d_db, _ = inp.place(packed, 64, 1, front=live_head(packed[FRONT:], 64), back=live_tail(packed, 64), name="db")
    out = Arena(torch, dev, arena_bytes(nq * nt * 24))
    c = out.carve(nq * nt * 24, 8, 0, name="results")
    res = out.view(c, torch.int64, (nq * nt * 3,))
    with engine.prepare_db(d_db, offs) as db:
        got = db.search_affine_device(d_q, qoffs, scorings["affine"], out=res)
        engine.synchronize()
        got = got.cpu().numpy()
    assert not differ(got, case["host"]["affine"]), differ(got, case["host"]["affine"])
    raw = out.bytes_of(c).cpu().numpy().reshape(nq * nt, 24)
    assert not (raw == POISON).all(axis=1).any() and (got[:, :, 2] == 0).all()   # every entry written, path_len included
    assert_guards(out)
    assert_guards(inp)


def test_score_edges_last_column_last_row_and_ties(engine, swamd):
    """The maximum planted in the LAST cell of the largest matrix (last column of the longest query, last row of the longest target), and
    periodic sequences whose maximum is reached at many cells: the lowest index wins, in every class and across strips."""
    rng = np.random.default_rng(99)
    scoring = (swamd.submat_match(3, -3), -4, -1)
    letters = PROTEIN[:20]
    long_q = rng.choice(letters, 2049).astype(np.uint8)
    long_t = np.concatenate([rng.choice(letters, 900).astype(np.uint8), long_q[-200:]])             # 1100 rows, the last 200 = the query's end
    long_t[899] = letters[0] if long_q[-201] != letters[0] else letters[1]                          # (the planted run does not extend by chance)
    queries = [rng.choice(letters, 300).astype(np.uint8), long_q, np.frombuffer(b"ACGT" * 300, np.uint8), np.frombuffer(b"ACGT" * 50, np.uint8),
               np.frombuffer(b"ACGT" * 100, np.uint8)]
    targets = [np.frombuffer(b"ACGT" * n, np.uint8) for n in (1, 16, 17, 100, 275)] + [long_t, np.frombuffer(b"GTAC" * 200, np.uint8)]
    qpacked, qoffs = swamd._pack_targets(queries)
    packed, offs = swamd._pack_targets(targets)
    want = swamd.search_affine_multi_host((qpacked, qoffs), (packed, offs), scoring)
    assert tuple(want[1, 5]) == (1100 * 2050 + 2049, 600, 0)                                     # conditions of this test: the planted corner ...
    assert tuple(want[2, 3]) == (400 * 1201 + 400, 1200, 0) and tuple(want[3, 4]) == (200 * 201 + 200, 600, 0)   # ... and the first of many equal cells
    d_q, d_db = to_dev(engine, qpacked, 1), to_dev(engine, packed, 1)
    with engine.prepare_db(d_db, offs) as db:
        got = db.search_affine_device(d_q, qoffs, scoring, out=poisoned(engine, len(queries), len(targets))).cpu().numpy()
    assert not differ(got, want), differ(got, want)
    assert np.array_equal(engine.prepare_db(targets).search_affine(queries, scoring), want)       # the list interface, host memory in and out
