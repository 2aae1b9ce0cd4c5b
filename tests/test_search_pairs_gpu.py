"""GPU: a device list of (query, target) pairs against a prepared database (sw_db_search_affine_pairs, Database.search_affine_pairs_device)
against the gathered table of sw_db_search_affine ON THE SAME DEVICE BUFFERS and against the host leg (sw_search_affine_pairs_host, which
tests/test_search_pairs_host.py holds against the independent checker) -- exact equality everywhere.  The item workspace is read
through the accessor option "debug_search_pairs_items_ptr" (the heaviest-first test)."""
import ctypes

import numpy as np
import pytest

from affine_cases import PROTEIN
from buffer_cases import POISON, Arena, arena_bytes, assert_guards, live_head, live_tail

pytestmark = pytest.mark.gpu

QLENS = [1, 4, 255, 256, 257, 512, 513, 1024, 1025, 2049]        # every class (4 / 8 / 16 columns per lane), one strip and several
TLENS = [0, 1, 63, 64, 65, 127, 300, 1100, 64, 0, 1, 300, 65, 127, 63]
QFRONT, FRONT = 4, 3                                             # qoffsets[0], offsets[0]
POISON_RESULT = -0x5A5A5A5A5A5A5A5B
INT64_MIN = -(1 << 63)
EINVAL = -22
ITEM = np.dtype([("start", "<i8"), ("out", "<i8"), ("len", "<i4"), ("entry", "<i4")])   # swk::SearchPairItem, 24 bytes


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


def pairs_dev(engine, pairs):
    t = engine.torch
    pr = np.ascontiguousarray(np.asarray(pairs, np.int64).reshape(-1, 2))
    return t.from_numpy(pr.copy() if len(pr) else np.zeros((1, 2), np.int64)).to(f"cuda:{engine.device}")[:len(pr)]


def poisoned(engine, npairs):
    t = engine.torch
    return t.full((max(3, npairs * 3),), POISON_RESULT, dtype=t.int64, device=f"cuda:{engine.device}")


def run(engine, db, d_q, qoffs, scoring, pairs):
    """The call on a host list, into poisoned results: (npairs, 3) numpy."""
    pr = np.asarray(pairs, np.int64).reshape(-1, 2)
    res = db.search_affine_pairs_device(d_q, qoffs, scoring, pairs_dev(engine, pr), out=poisoned(engine, len(pr)))
    engine.synchronize()
    return res.cpu().numpy()


def differ(got, want):
    bad = np.nonzero((got != want).any(axis=1))[0]
    return f"{len(bad)} pairs differ, first entry {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}" if len(bad) else ""


def cross(nq, nt, seed):
    pairs = np.array([(q, k) for q in range(nq) for k in range(nt)], np.int64)
    return pairs[np.random.default_rng(seed).permutation(len(pairs))]


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
    """The mixed case: the ten query lengths shuffled, the targets, both on the device (query base odd), the handle, all 150 pairs in a
    fixed shuffled order, and per scoring the table of sw_db_search_affine on the same buffers and the host leg's results -- computed
    once, never changed."""
    rng = np.random.default_rng(2024)
    qlens = list(QLENS)
    rng.shuffle(qlens)
    qpacked, qoffs = pack(qlens, QFRONT, rng, PROTEIN[:20])
    packed, offs = pack(TLENS, FRONT, rng, PROTEIN[:20])
    d_q, d_db = to_dev(engine, qpacked, 1), to_dev(engine, packed, 0)
    assert (d_q.data_ptr() + QFRONT) % 2 == 1
    db = engine.prepare_db(d_db, offs)
    pairs = cross(len(QLENS), len(TLENS), 7)
    table, host = {}, {}
    for k, s in scorings.items():
        table[k] = db.search_affine_device(d_q, qoffs, s).cpu().numpy()
        host[k] = swamd.search_affine_pairs_host((qpacked, qoffs), (packed, offs), s, pairs)
    classes = engine.get_option("last_search_multi_launches")     # one launch per class of queries there: what this device's occupancy makes of QLENS
    assert engine.get_option("last_search_multi_groups") == 1 and 2 <= classes <= 3
    yield {"qlens": qlens, "qpacked": qpacked, "qoffs": qoffs, "packed": packed, "offs": offs, "d_q": d_q, "d_db": d_db, "db": db, "pairs": pairs,
           "table": table, "host": host, "classes": classes}
    db.close()


def gathered(case, which, pairs):
    return case["table"][which][pairs[:, 0], pairs[:, 1]]


@pytest.mark.parametrize("which", ["affine", "linear"])
def test_mixed_list_equals_the_gathered_table_and_the_host_leg(engine, case, scorings, which):
    pairs = case["pairs"]
    got = run(engine, case["db"], case["d_q"], case["qoffs"], scorings[which], pairs)
    assert got.shape == (150, 3)
    assert engine.get_option("last_search_pairs_groups") == 1 and engine.get_option("last_search_pairs_chunks") == 1
    # the plan of one group and one chunk: a profile launch, two binning launches, one score launch per class of queries (three where the
    # 16-column kernel keeps two workgroups per CU, as on gfx950; the planner's arithmetic is tests/test_search_pairs_plan.py's)
    assert engine.get_option("last_search_pairs_launches") == 1 + 2 + case["classes"]
    assert not differ(got, gathered(case, which, pairs)), "table: " + differ(got, gathered(case, which, pairs))
    assert not differ(got, case["host"][which]), "host leg: " + differ(got, case["host"][which])
    empty = np.diff(case["offs"])[pairs[:, 1]] == 0
    assert empty.sum() == 20 and (got[empty] == 0).all()                                # empty targets: zero over the poison
    assert (got[:, 1] > 0).sum() > 80 and (got[:, 2] == 0).all()


def test_reversed_list_gives_reversed_results_and_two_runs_the_same_bytes(engine, case, scorings):
    pairs = case["pairs"]
    a = run(engine, case["db"], case["d_q"], case["qoffs"], scorings["affine"], pairs)
    b = run(engine, case["db"], case["d_q"], case["qoffs"], scorings["affine"], pairs)
    assert a.tobytes() == b.tobytes()
    r = run(engine, case["db"], case["d_q"], case["qoffs"], scorings["affine"], pairs[::-1])
    assert np.array_equal(r, a[::-1]) and not differ(a, case["host"]["affine"])


def test_bad_and_duplicate_entries(engine, case, scorings):
    rng = np.random.default_rng(31)
    pairs = case["pairs"].copy()
    nq, nt = len(QLENS), len(TLENS)
    where = rng.choice(150, 30 + 10, replace=False)
    bad_at, dup_at = where[:30], where[30:]
    bad_values = [(-1, -1), (nq, nt), (1 << 40, 1 << 40), (INT64_MIN, INT64_MIN)]
    for i, p in enumerate(bad_at):                                                      # the query, the target, or both, each bad value in turn
        bq, bt = bad_values[i % 4]
        field = (i // 4) % 3
        pairs[p] = (bq if field != 1 else pairs[p, 0], bt if field != 0 else pairs[p, 1])
    rest = np.setdiff1d(np.arange(150), where)
    src = rest[np.nonzero(gathered(case, "affine", pairs[rest])[:, 1] > 0)[0][:5]]      # five pairs with a score, each written three times
    for i, s in enumerate(src):
        pairs[dup_at[2 * i]] = pairs[dup_at[2 * i + 1]] = pairs[s]
    got = run(engine, case["db"], case["d_q"], case["qoffs"], scorings["affine"], pairs)
    assert (got[bad_at] == 0).all()
    for i, s in enumerate(src):
        assert got[s, 1] > 0 and np.array_equal(got[dup_at[2 * i]], got[s]) and np.array_equal(got[dup_at[2 * i + 1]], got[s])
    good = np.setdiff1d(np.arange(150), bad_at)
    assert not differ(got[good], gathered(case, "affine", pairs[good]))
    assert np.array_equal(got[rest], case["host"]["affine"][rest])                      # the rest is unchanged


def test_a_list_of_only_unusable_pairs(engine, case, scorings):
    nq, nt = len(QLENS), len(TLENS)
    pairs = [(q, k) for q in range(nq) for k in (0, 9)]                                 # the two empty targets
    pairs += [(-1, 3), (nq, 3), (1 << 40, 3), (INT64_MIN, 3), (2, -1), (2, nt), (2, 1 << 40), (2, INT64_MIN), (-1, -1), (INT64_MIN, INT64_MIN)]
    got = run(engine, case["db"], case["d_q"], case["qoffs"], scorings["affine"], pairs)
    assert got.shape == (len(pairs), 3) and (got == 0).all()
    assert engine.get_option("last_search_pairs_launches") == 3 + case["classes"]       # every launch ran, every list was empty
    after = run(engine, case["db"], case["d_q"], case["qoffs"], scorings["affine"], case["pairs"])
    assert not differ(after, case["host"]["affine"])                                    # the device is as good as before


def test_sparse_list(engine, swamd, scorings):
    """500 random pairs over 300 short queries, 100 of which no pair names: their profiles are built and never read."""
    rng = np.random.default_rng(300)
    qpacked, qoffs = pack([8] * 300, 0, rng, PROTEIN[:20])
    packed, offs = pack([40, 9, 300, 64, 17, 1, 0, 65] * 5, FRONT, rng, PROTEIN[:20])
    named = rng.choice(300, 200, replace=False)
    pairs = np.stack([rng.choice(named, 500), rng.integers(0, 40, 500)], axis=1).astype(np.int64)
    assert len(np.unique(pairs[:, 0])) <= 200
    d_q, d_db = to_dev(engine, qpacked, 1), to_dev(engine, packed, 0)
    with engine.prepare_db(d_db, offs) as db:
        got = run(engine, db, d_q, qoffs, scorings["affine"], pairs)
        assert engine.get_option("last_search_pairs_launches") == 4                     # one class
    want = swamd.search_affine_pairs_host((qpacked, qoffs), (packed, offs), scorings["affine"], pairs)
    assert not differ(got, want), differ(got, want)


@pytest.mark.parametrize("name,qlo,qhi,nq,tlens", [
    ("4 columns per lane, one strip", 1, 256, 300, [40, 9, 300, 64, 17, 1, 0, 65] * 5),            # 300 x 35 = 10 500 items
    ("8 columns per lane, one strip", 257, 512, 120, [30, 7, 64, 65, 0, 120] * 10),               # 120 x 50 = 6 000 items
    ("16 columns per lane, one to three strips", 513, 2100, 60, [33, 5, 64, 0, 65, 90, 17] * 10),  # 60 x 60 = 3 600 items
])
def test_every_wave_takes_several_items(engine, scorings, name, qlo, qhi, nq, tlens):
    """The shapes of test_search_multi_gpu's test of the same name as full explicit lists in random order: more items in the ONE launch
    of the class than it has waves (6144 / 5120 / 3072 resident on 256 CUs), so every wave runs the loop around the sweep again with
    another item -- a wrong list base, a wrong cursor or state kept from the previous item shows against the table."""
    rng = np.random.default_rng(nq)
    qlens = [qlo, qhi] + list(rng.integers(qlo, qhi + 1, nq - 2))
    rng.shuffle(qlens)
    qpacked, qoffs = pack(qlens, QFRONT, rng, PROTEIN[:20])
    packed, offs = pack(tlens, FRONT, rng, PROTEIN[:20])
    d_q, d_db = to_dev(engine, qpacked, 1), to_dev(engine, packed, 0)
    pairs = cross(nq, len(tlens), nq)
    with engine.prepare_db(d_db, offs) as db:
        table = db.search_affine_device(d_q, qoffs, scorings["affine"]).cpu().numpy()
        got = run(engine, db, d_q, qoffs, scorings["affine"], pairs)
        assert engine.get_option("last_search_pairs_launches") == 4, name
    want = table[pairs[:, 0], pairs[:, 1]]
    assert not differ(got, want), name + ": " + differ(got, want)
    assert (got[:, 1] > 0).sum() > len(pairs) // 2, name


def test_chunks_and_groups(engine, case, scorings):
    """150 pairs in chunks of 64 and the ten profiles (2.3 MiB) under a budget of 1 MiB: three chunks, the groups of sw_db_search_affine
    under the same budget, the bytes of the uncut call."""
    whole = run(engine, case["db"], case["d_q"], case["qoffs"], scorings["affine"], case["pairs"])
    assert engine.get_option("search_pairs_chunk") == 1 << 22 and engine.get_option("search_profile_mib") == 256
    engine.set_option("search_pairs_chunk", 64)
    engine.set_option("search_profile_mib", 1)
    try:
        case["db"].search_affine_device(case["d_q"], case["qoffs"], scorings["affine"])
        groups = engine.get_option("last_search_multi_groups")
        cut = run(engine, case["db"], case["d_q"], case["qoffs"], scorings["affine"], case["pairs"])
        assert engine.get_option("last_search_pairs_chunks") == 3
        assert engine.get_option("last_search_pairs_groups") == groups >= 3
        assert engine.get_option("last_search_pairs_launches") > 3 * 3 * groups         # count, scatter and a class at least per (chunk, group)
    finally:
        engine.set_option("search_pairs_chunk", 1 << 22)
        engine.set_option("search_profile_mib", 256)
    assert cut.tobytes() == whole.tobytes() and not differ(cut, case["host"]["affine"])
    for bad in (0, -1, 1 << 31):
        with pytest.raises(Exception):
            engine.set_option("search_pairs_chunk", bad)
    assert engine.get_option("search_pairs_chunk") == 1 << 22


def test_heaviest_first(engine, swamd, scorings):
    """One class: 4 targets of length 1100 among 400 of length 5, each paired with one query of 300.  len x qpad is 1100 x 512 (bucket 19)
    and 5 x 512 (bucket 11): after the scatter launch the four long items lead the class's list, whatever their places in the caller's."""
    rng = np.random.default_rng(1100)
    tlens = [5] * 404
    for k in (17, 150, 151, 399):
        tlens[k] = 1100
    qpacked, qoffs = pack([300], 0, rng, PROTEIN[:20])
    packed, offs = pack(tlens, FRONT, rng, PROTEIN[:20])
    pairs = cross(1, 404, 404)
    d_q, d_db = to_dev(engine, qpacked, 1), to_dev(engine, packed, 0)
    with engine.prepare_db(d_db, offs) as db:
        got = run(engine, db, d_q, qoffs, scorings["affine"], pairs)
        ptr = engine.get_option("debug_search_pairs_items_ptr")
        assert ptr > 0
        items = np.zeros(404, ITEM)
        assert swamd.lib().sw_memcpy_d2h(engine._h, items.ctypes.data, ptr, items.nbytes) == 0
    want = swamd.search_affine_pairs_host((qpacked, qoffs), (packed, offs), scorings["affine"], pairs)
    assert not differ(got, want), differ(got, want)
    assert items["len"][:4].tolist() == [1100] * 4 and (items["len"][4:] == 5).all()
    assert sorted(items["out"].tolist()) == list(range(404)) and (items["entry"] == 0).all()
    assert np.array_equal(items["start"], offs[pairs[items["out"], 1]])                 # every item names its pair's target


def test_buffer_contract(engine, case, scorings):
    """Guard bytes before and after d_results and d_pairs stay untouched, the pair list keeps its bytes, every poisoned result entry is
    overwritten.  d_pairs lies at an odd multiple of 8."""
    torch = engine.torch
    dev = f"cuda:{engine.device}"
    pairs = case["pairs"]
    n = len(pairs)
    raw_pairs = np.ascontiguousarray(pairs).view(np.uint8).reshape(-1)
    inp = Arena(torch, dev, arena_bytes(len(raw_pairs) + 128))
    d_raw, cp = inp.place(raw_pairs, 16, 8, name="pairs")
    assert d_raw.data_ptr() % 16 == 8
    d_pairs = d_raw.view(torch.int64).view(n, 2)
    out = Arena(torch, dev, arena_bytes(n * 24))
    c = out.carve(n * 24, 8, 0, name="results")
    res = out.view(c, torch.int64, (n * 3,))
    got = case["db"].search_affine_pairs_device(case["d_q"], case["qoffs"], scorings["affine"], d_pairs, out=res)
    engine.synchronize()
    got = got.cpu().numpy()
    assert not differ(got, case["host"]["affine"]), differ(got, case["host"]["affine"])
    raw = out.bytes_of(c).cpu().numpy().reshape(n, 24)
    assert not (raw == POISON).all(axis=1).any() and (got[:, 2] == 0).all()             # every entry written, path_len included
    assert_guards(out)
    assert_guards(inp)


def test_empty_handle_and_handle_of_only_empty_targets(engine, case, scorings):
    pairs = [(0, 0), (3, 1), (-1, 0), (9, 2)]
    with engine.prepare_db(case["d_db"], np.array([7], np.int64)) as db:                  # no target: no index is inside
        got = run(engine, db, case["d_q"], case["qoffs"], scorings["affine"], pairs)
        assert got.shape == (4, 3) and (got == 0).all() and engine.get_option("last_search_pairs_launches") == 0
    with engine.prepare_db(case["d_db"], np.array([5, 5, 5, 5], np.int64)) as db:
        got = run(engine, db, case["d_q"], case["qoffs"], scorings["affine"], pairs)
        assert (got == 0).all() and engine.get_option("last_search_pairs_launches") == 0


def test_no_pair_one_pair_and_no_query(engine, case, scorings):
    out = poisoned(engine, 1)
    res = case["db"].search_affine_pairs_device(case["d_q"], case["qoffs"], scorings["affine"], pairs_dev(engine, []), out=out)
    engine.synchronize()
    assert res.shape == (0, 3) and bool((out == POISON_RESULT).all())                    # nothing launched, nothing written
    assert engine.get_option("last_search_pairs_launches") == 0
    one = case["pairs"][np.nonzero(case["host"]["affine"][:, 1] > 0)[0][:1]]
    got = run(engine, case["db"], case["d_q"], case["qoffs"], scorings["affine"], one)
    assert got.shape == (1, 3) and np.array_equal(got, gathered(case, "affine", one)) and got[0, 1] > 0
    assert engine.get_option("last_search_pairs_launches") == 3 + case["classes"]       # the plan follows the queries: every class gets its launch
    got = run(engine, case["db"], case["d_q"], np.array([4], np.int64), scorings["affine"], [(0, 3), (1, 1)])   # no query: no entry names one
    assert (got == 0).all() and engine.get_option("last_search_pairs_launches") == 0


def test_two_calls_on_two_streams_one_after_the_other(engine, case, scorings):
    t = engine.torch
    s1, s2 = t.cuda.Stream(device=engine.device), t.cuda.Stream(device=engine.device)
    o1, o2 = poisoned(engine, 150), poisoned(engine, 150)
    d_pairs = pairs_dev(engine, case["pairs"])
    t.cuda.synchronize()
    with t.cuda.stream(s1):
        r1 = case["db"].search_affine_pairs_device(case["d_q"], case["qoffs"], scorings["affine"], d_pairs, out=o1)
    with t.cuda.stream(s2):
        r2 = case["db"].search_affine_pairs_device(case["d_q"], case["qoffs"], scorings["linear"], d_pairs, out=o2)
    s1.synchronize()
    s2.synchronize()
    assert not differ(r1.cpu().numpy(), case["host"]["affine"]) and not differ(r2.cpu().numpy(), case["host"]["linear"])


def test_list_interface(engine, swamd, scorings):
    queries, targets = [b"ACDEFGHIKL", b"MNPQ", b"ACDEFG" * 50], [b"ACDEFGHIKL", b"", b"KLMNPQRST", b"ACDEFG" * 20]
    pairs = [(2, 3), (0, 0), (1, 2), (0, 1), (5, 0), (2, 3)]
    with engine.prepare_db(targets) as db:
        got = db.search_affine_pairs(queries, scorings["affine"], pairs)
        assert db.search_affine_pairs(queries, scorings["affine"], []).shape == (0, 3)
    want = swamd.search_affine_pairs_host(queries, targets, scorings["affine"], pairs)
    assert got.shape == (6, 3) and np.array_equal(got, want) and (got[[3, 4]] == 0).all() and got[0, 1] > 0


def test_argument_errors_leave_the_results_poisoned(engine, swamd, case, scorings):
    L = swamd.lib()
    t = engine.torch
    db, d_q, qoffs = case["db"], case["d_q"], case["qoffs"]
    d_pairs = pairs_dev(engine, case["pairs"])
    out = poisoned(engine, 150)
    sub, sc = swamd._affine(*scorings["affine"])

    def call(**kw):
        a = {"ctx": engine._h, "db": db._h, "queries": d_q.data_ptr(), "qoffs": qoffs, "nq": len(QLENS), "sc": ctypes.byref(sc), "pairs": d_pairs.data_ptr(),
             "npairs": 150, "results": out.data_ptr(), **kw}
        qo = None if a["qoffs"] is None else np.ascontiguousarray(a["qoffs"], np.int64)
        rc = L.sw_db_search_affine_pairs(a["ctx"], a["db"], a["queries"], None if qo is None else qo.ctypes.data, a["nq"], a["sc"], a["pairs"], a["npairs"],
                                         a["results"], engine._stream())
        engine.synchronize()
        return rc

    bad = [{"ctx": None}, {"db": None}, {"queries": None}, {"qoffs": None}, {"sc": None}, {"pairs": None}, {"npairs": -1}, {"nq": -1},
           {"qoffs": [4, 4], "nq": 1}, {"qoffs": [4, 2], "nq": 1}, {"qoffs": [-1, 3], "nq": 1}, {"qoffs": [0, 1 << 20], "nq": 1}]
    keep = [swamd._affine(sub, go, ge)[1] for go, ge in ((1, -1), (-1, 1), (-(1 << 24), -1))]   # the scoring errors
    bad += [{"sc": ctypes.byref(s)} for s in keep]
    for kw in bad:
        assert call(**kw) == EINVAL, kw
        assert bool((out == POISON_RESULT).all()), kw                                   # an error leaves the results untouched
    assert call(results=None) == EINVAL and bool((out == POISON_RESULT).all())
    assert call(pairs=None, results=None, npairs=0) == 0 and bool((out == POISON_RESULT).all())   # neither is looked at without a pair
    with pytest.raises(ValueError, match="out must be"):                               # a result tensor too small for the list: refused before the call
        db.search_affine_pairs_device(d_q, qoffs, scorings["affine"], d_pairs, out=poisoned(engine, 149))
    with pytest.raises(ValueError, match="d_pairs must be"):
        db.search_affine_pairs_device(d_q, qoffs, scorings["affine"], d_pairs.view(-1))
    with pytest.raises(ValueError, match="d_pairs must be"):
        db.search_affine_pairs_device(d_q, qoffs, scorings["affine"], d_pairs.to(t.int32))
    assert call() == 0                                                                  # the handle is as good as before
    assert not differ(out.view(150, 3).cpu().numpy(), case["host"]["affine"])
