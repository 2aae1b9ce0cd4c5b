"""GPU: the pair list on packed 16-bit lanes ("search_pairs_lanes" = 16; smith-waterman_amd/csrc/sw_search_pairs16.hip).  Every
comparison is bitwise and three-way: search_pairs_lanes = 16 against 32 on the same device buffers, and against the host leg
(sw_search_affine_pairs_host); the scoring edges go against tests/affine_oracle.cpp as well.  Every call writes into poisoned results,
and after each call the route is asserted from "last_search_pairs_packed_launches", so that no case passes on a path it was not meant
for.  The scoring cases are tests/lanes_cases.py's."""
import numpy as np
import pytest

import affine_range_cases as arc
import buffer_cases as bc
import lanes_cases as lc
from affine_cases import PROTEIN, checker  # noqa: F401

pytestmark = pytest.mark.gpu

EINVAL = -22
POISON64 = -0x5A5A5A5A5A5A5A5B
INT64_MAX = (1 << 63) - 1


def to_dev(engine, packed, skew):
    """The bytes on the device at an address with addr % 2 == skew % 2 (torch aligns allocations to 512 bytes)."""
    t = engine.torch
    buf = t.zeros(len(packed) + skew + 16, dtype=t.uint8, device=f"cuda:{engine.device}")
    buf[skew:skew + len(packed)] = t.from_numpy(np.array(packed))
    return buf[skew:skew + len(packed)]


def pairs_dev(engine, pairs):
    t = engine.torch
    pr = np.ascontiguousarray(np.asarray(pairs, np.int64).reshape(-1, 2))
    return t.from_numpy(pr.copy()).to(f"cuda:{engine.device}")


def poisoned(engine, npairs):
    t = engine.torch
    return t.full((max(3, npairs * 3),), POISON64, dtype=t.int64, device=f"cuda:{engine.device}")


def differ(got, want):
    got, want = np.asarray(got).reshape(-1, 3), np.asarray(want).reshape(-1, 3)
    if got.shape != want.shape:
        return f"shape {got.shape} vs {want.shape}"
    bad = np.nonzero((got != want).any(axis=1))[0]
    return f"{len(bad)} entries differ, first {bad[0]}: {tuple(got[bad[0]])} vs {tuple(want[bad[0]])}" if len(bad) else ""


def under(engine, lanes, call):
    """call() under search_pairs_lanes = lanes: (what it returned, as numpy, what the context says of the call); the option is 32 again afterwards."""
    engine.set_option("search_pairs_lanes", lanes)
    try:
        assert engine.get_option("search_pairs_lanes") == lanes
        out = call()
        engine.synchronize()
        said = {"launches": engine.get_option("last_search_pairs_launches"), "packed": engine.get_option("last_search_pairs_packed_launches"),
                "items": engine.get_option("last_search_pairs_packed_items"), "groups": engine.get_option("last_search_pairs_groups"),
                "chunks": engine.get_option("last_search_pairs_chunks")}
    finally:
        engine.set_option("search_pairs_lanes", 32)
    out = tuple(x.cpu().numpy() for x in out) if isinstance(out, tuple) else out.cpu().numpy()
    return out, said


def qpad_of(qlen):
    """The profile row length of a query where the 16-column kernels keep two workgroups per CU (gfx950)."""
    w = 64 * (4 if qlen <= 256 else 8 if qlen <= 512 else 16)
    return -(-qlen // w) * w


def two_pair_items(case, pairs, chunk=None, packed=None):
    """What the device has to count: per chunk and cell (query, bucket) of the valid pairs of packed queries, ceil(n / 2)."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    lens, qlens = np.diff(case["offs"]), np.diff(case["qoffs"])
    nq, nt = len(qlens), len(lens)
    chunk = chunk or max(1, len(pairs))
    total = 0
    for p0 in range(0, len(pairs), chunk):
        cells = {}
        for q, k in pairs[p0:p0 + chunk].tolist():
            if 0 <= q < nq and 0 <= k < nt and lens[k] > 0 and (packed is None or packed[q]):
                key = (q, int(lens[k] * qpad_of(int(qlens[q]))).bit_length() - 1)
                cells[key] = cells.get(key, 0) + 1
        total += sum(-(-n // 2) for n in cells.values())
    return total


class OnDevice:
    """A case ({"qpacked", "qoffs", "packed", "offs", ...}) on the device: queries at an odd base, the database and its handle."""

    def __init__(self, engine, case):
        self.case, self.engine = case, engine
        self.d_q, self.d_db = to_dev(engine, case["qpacked"], 1), to_dev(engine, case["packed"], 0)
        self.db = engine.prepare_db(self.d_db, case["offs"])
        self.nq, self.nt = len(case["qoffs"]) - 1, len(case["offs"]) - 1

    def close(self):
        self.db.close()

    def cross(self, seed):
        pairs = np.array([(q, k) for q in range(self.nq) for k in range(self.nt)], np.int64)
        return pairs[np.random.default_rng(seed).permutation(len(pairs))]

    def run(self, scoring, pairs, lanes, d_pairs=None, out=None):
        pr = np.asarray(pairs, np.int64).reshape(-1, 2)
        d_pairs = pairs_dev(self.engine, pr) if d_pairs is None else d_pairs
        out = poisoned(self.engine, len(pr)) if out is None else out
        return under(self.engine, lanes, lambda: self.db.search_affine_pairs_device(self.d_q, self.case["qoffs"], scoring, d_pairs, out=out))


def three_way(swamd, d, scoring, pairs, what, host=None):
    """The list under 32, under 16 and on the host, byte for byte: (the results, what the call under 16 said, under 32)."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    r32, said32 = d.run(scoring, pairs, 32)
    r16, said16 = d.run(scoring, pairs, 16)
    if host is None:
        host = swamd.search_affine_pairs_host((d.case["qpacked"], d.case["qoffs"]), (d.case["packed"], d.case["offs"]), scoring, pairs)
    assert said32["packed"] == 0 and said32["items"] == 0, what
    assert r16.shape == (len(pairs), 3)
    assert r16.tobytes() == r32.tobytes(), f"{what}: 16 vs 32: " + differ(r16, r32)
    assert r16.tobytes() == host.tobytes(), f"{what}: 16 vs host: " + differ(r16, host)
    return r16, said16, said32


@pytest.fixture(scope="module")
def world(engine, swamd):
    """lc.QLENS against 200 targets of 0 .. 1100 letters (ten empty ones; 256 and 511, the ends of one bucket of every query whose
    profile row is a power of two long; 300 and 301), every pair in a fixed shuffled order, the table of Database.search_affine on
    the same buffers and the host leg's results of the list -- computed once, never changed."""
    rng = np.random.default_rng(1600)
    lens = [int(n) for n in rng.integers(1, 150, 170)] + [int(n) for n in rng.integers(150, 1100, 12)] + [1, 1100, 256, 511, 255, 512, 300, 301] + [0] * 10
    rng.shuffle(lens)
    assert len(lens) == 200
    case = lc.case_of([rng.choice(PROTEIN, n) for n in lc.QLENS], [rng.choice(PROTEIN, n) for n in lens])
    d = OnDevice(engine, case)
    scoring = (lc.table24(), -11, -1)
    pairs = d.cross(16)
    table = d.db.search_affine_device(d.d_q, case["qoffs"], scoring).cpu().numpy()
    host = swamd.search_affine_pairs_host((case["qpacked"], case["qoffs"]), (case["packed"], case["offs"]), scoring, pairs)
    hosttab = np.zeros_like(table)
    hosttab[pairs[:, 0], pairs[:, 1]] = host
    yield {"d": d, "case": case, "scoring": scoring, "pairs": pairs, "table": table, "host": host, "hosttab": hosttab, "lens": np.array(lens)}
    d.close()


def checked(checker, case, sub, gaps, pairs):  # noqa: F811
    full = np.stack([checker.search(q, case["packed"], case["offs"], sub, *gaps) for q in case["queries"]])
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    return full[pairs[:, 0], pairs[:, 1]]


# ---- the whole cross product ----

def test_cross_product(swamd, checker, world):  # noqa: F811
    w = world
    got, said16, said32 = three_way(swamd, w["d"], w["scoring"], w["pairs"], "cross", host=w["host"])
    assert not differ(got, w["table"][w["pairs"][:, 0], w["pairs"][:, 1]])              # the table of search_affine at the list's indices
    want = checked(checker, w["case"], lc.table24(), (-11, -1), w["pairs"])
    assert not differ(got, want), differ(got, want)
    # one group, one chunk: a profile launch, three binning launches, a packed launch per class; two binning launches under 32
    assert (said16["launches"], said16["packed"]) == (1 + 3 + 3, 3) and (said32["launches"], said32["packed"]) == (1 + 2 + 3, 0)
    assert said16["items"] == two_pair_items(w["case"], w["pairs"]) > 600
    empty = w["lens"][w["pairs"][:, 1]] == 0
    assert empty.sum() == 70 and not got[empty].any() and (got[~empty, 1] > 0).sum() > 1000


@pytest.mark.parametrize("gaps", lc.GAPS[1:], ids=lambda g: f"{g[0]}_{g[1]}")
def test_other_gap_costs(swamd, world, gaps):
    w = world
    pairs = w["pairs"][:400]
    _, said16, _ = three_way(swamd, w["d"], (lc.table24(), *gaps), pairs, f"gaps {gaps}")
    assert said16["packed"] == 3 and said16["items"] == two_pair_items(w["case"], pairs)


# ---- cells of one, two and three pairs ----

def test_cells_of_one_two_and_three(swamd, world):
    w = world
    lens = w["lens"]
    live = np.nonzero(lens > 0)[0]
    one = [(3, int(live[0]))]
    got, said, _ = three_way(swamd, w["d"], w["scoring"], one, "one pair alone")
    assert said["items"] == 1 and said["packed"] == 3 and got[0, 1] > 0
    each = [(q, int(live[q])) for q in range(7)]                                         # every query has exactly one pair: singles only
    _, said, _ = three_way(swamd, w["d"], w["scoring"], each, "one pair per query")
    assert said["items"] == 7
    # targets of 100 .. 127 letters share the bucket of any query: a pair of them, three of them
    same = [int(k) for k in np.nonzero((lens >= 100) & (lens <= 127))[0][:3]]
    assert len(same) == 3
    for n, items in ((2, 1), (3, 2)):
        lst = [(4, k) for k in same[:n]]
        _, said, _ = three_way(swamd, w["d"], w["scoring"], lst, f"a cell of {n}")
        assert said["items"] == items == two_pair_items(w["case"], lst)
    mixed = [(4, same[0]), (1, same[0]), (4, same[1]), (6, same[2]), (4, same[2]), (1, same[1])]   # cells of 3, 2 and 1 in one list
    _, said, _ = three_way(swamd, w["d"], w["scoring"], mixed, "cells of 3, 2, 1")
    assert said["items"] == 2 + 1 + 1


def test_duplicates_are_partners(swamd, world):
    w = world
    k = int(np.nonzero(w["lens"] == 300)[0][0])
    for q in (2, 5):
        for n in (2, 3):
            got, said, _ = three_way(swamd, w["d"], w["scoring"], [(q, k)] * n, f"({q}, {k}) x {n}")
            assert said["items"] == (n + 1) // 2 and got[0, 1] > 0 and (got == got[0]).all()  # every copy's entry is written
    lst = [(5, k), (0, 3), (5, k), (5, k + 1), (5, k)]
    got, _, _ = three_way(swamd, w["d"], w["scoring"], lst, "copies among others")
    assert np.array_equal(got[0], got[2]) and np.array_equal(got[0], got[4])


# ---- entries that never become an item ----

def test_bad_indices_and_empty_targets_between_live_pairs(engine, swamd, world):
    w = world
    d, case = w["d"], w["case"]
    nq, nt = d.nq, d.nt
    empties = [int(k) for k in np.nonzero(w["lens"] == 0)[0]]
    bad = [(-1, 5), (2, -1), (nq, 5), (2, nt), (INT64_MAX, 5), (2, INT64_MAX), (-1, -1), (INT64_MAX, INT64_MAX), (3, empties[0]), (6, empties[1])]
    pairs = w["pairs"][:300].tolist()
    where = []
    for i, b in enumerate(bad * 3):                                                      # interleaved with the live pairs
        where.append(7 + 9 * i)
        pairs.insert(where[-1], b)
    # ... and the tail of a real pre-filter run: the rows behind its count are (-1, -1)
    cap = nq * nt
    fp, fn, _ = d.db.prefilter_ungapped_device(d.d_q, case["qoffs"], lc.table24(), 60, cap)
    engine.synchronize()
    n = int(fn.item())
    assert 0 < n < cap
    tail = fp.cpu().numpy()
    assert (tail[n:] == -1).all() and (tail[:n] >= 0).all()
    pairs = np.array(pairs + tail.tolist(), np.int64)
    got, said, _ = three_way(swamd, d, w["scoring"], pairs, "bad entries")
    assert not got[where].any() and not got[len(pairs) - (cap - n):].any()
    valid = (pairs[:, 0] >= 0) & (pairs[:, 0] < nq) & (pairs[:, 1] >= 0) & (pairs[:, 1] < nt)
    good = np.nonzero(valid)[0]
    assert not differ(got[good], w["table"][pairs[good, 0], pairs[good, 1]])
    assert said["items"] == two_pair_items(case, pairs) and said["packed"] == 3
    # a list of nothing but such entries: every launch runs, every list is empty
    got, said, _ = three_way(swamd, d, w["scoring"], bad, "only bad entries")
    assert not got.any() and said["items"] == 0 and said["packed"] == 3


# ---- partners ----

def test_partners_at_the_ends_of_one_bucket(swamd, world):
    w = world
    at = {n: int(np.nonzero(w["lens"] == n)[0][0]) for n in (256, 511, 255, 512, 300, 301)}
    for q in (1, 2, 3, 4, 5):                                                            # profile rows of 256, 256, 512, 1024 and 2048: 256 and 511 share a bucket
        assert qpad_of(lc.QLENS[q]) & (qpad_of(lc.QLENS[q]) - 1) == 0
        for lst, items in (([(q, at[256]), (q, at[511])], 1), ([(q, at[511]), (q, at[256])], 1), ([(q, at[255]), (q, at[256])], 2), ([(q, at[511]), (q, at[512])], 2),
                           ([(q, at[300]), (q, at[301])], 1), ([(q, at[301]), (q, at[300])], 1)):
            got, said, _ = three_way(swamd, w["d"], w["scoring"], lst, f"query {q}: {lst}")
            assert said["items"] == items == two_pair_items(w["case"], lst)
            assert not differ(got, w["table"][[p[0] for p in lst], [p[1] for p in lst]])


def test_one_half_at_the_floor_while_the_other_climbs(engine, swamd, checker):  # noqa: F811
    """Under arc.table("corners") a query of 258 letters against itself (127 x 258 = 32766, the most the rule lets a half hold under this
    table) beside a target of 257 letters that mismatches everywhere, in either order of the list."""
    rng = np.random.default_rng(1601)
    q = rng.choice(np.array([0x00, 0xFF], np.uint8), 258)
    case = lc.case_of([q], [np.full(257, 0x01, np.uint8), q.copy()], filler=[0x01])
    sub = arc.table("corners")
    d = OnDevice(engine, case)
    try:
        for gaps in ((-11, -1), (0, 0), (-4, 0)):
            for lst in ([(0, 0), (0, 1)], [(0, 1), (0, 0)]):
                got, said, _ = three_way(swamd, d, (sub, *gaps), lst, f"corners {gaps} {lst}")
                assert said["packed"] == 1 and said["items"] == 1
                want = checked(checker, case, sub, gaps, lst)
                assert not differ(got, want), differ(got, want)
                assert got[lst.index((0, 1)), 1] == 127 * 258 and got[lst.index((0, 0)), 1] == 0
    finally:
        d.close()


@pytest.mark.parametrize("gaps", [(0, 0), (-1, 0)], ids=lambda g: f"{g[0]}_{g[1]}")
def test_ties_take_the_lowest_index_in_either_half(engine, swamd, checker, gaps):  # noqa: F811
    case, sub = lc.ties_case(), swamd.submat_match(1, -1)
    d = OnDevice(engine, case)
    try:
        pairs = np.concatenate([d.cross(5), d.cross(6)[:5]])                            # every pair, five of them twice
        got, said, _ = three_way(swamd, d, (sub, *gaps), pairs, f"ties {gaps}")
    finally:
        d.close()
    assert said["packed"] == 2 and said["items"] == two_pair_items(case, pairs)        # 257 and 1025 letters: two classes
    want = checked(checker, case, sub, gaps, pairs)
    assert not differ(got, want), differ(got, want)


# ---- the edges of the rule ----

def test_eligible_and_other_queries_in_one_call(engine, swamd, checker):  # noqa: F811
    case, sub = lc.ceiling_edge_case(), arc.table("ceiling")                            # queries of 258 and 259 letters, one class; targets of 300, 258, 64
    d = OnDevice(engine, case)
    try:
        pairs = np.concatenate([d.cross(8), d.cross(9)])
        got, said16, said32 = three_way(swamd, d, (sub, -11, -1), pairs, "ceiling")
    finally:
        d.close()
    assert (said16["launches"], said16["packed"]) == (1 + 3 + 2, 1) and said32["launches"] == 1 + 2 + 1   # 258 packed, 259 on 32-bit lanes in the same call
    assert said16["items"] == two_pair_items(case, pairs, packed=[True, False]) == 3
    want = checked(checker, case, sub, (-11, -1), pairs)
    assert not differ(got, want), differ(got, want)
    first = {tuple(p): i for i, p in reversed(list(enumerate(pairs.tolist())))}
    assert got[first[(0, 0)], 1] == 127 * 258 == 32766 and got[first[(1, 0)], 1] == 127 * 259


def test_the_score_32767(engine, swamd, checker):  # noqa: F811
    case, sub = lc.upper_edge_case(), np.full((256, 256), 31, np.int8)                  # queries of 1057 and 1058 letters, targets of 1100 and 1057
    d = OnDevice(engine, case)
    try:
        pairs = [(0, 0), (1, 1), (0, 1), (1, 0)]
        got, said16, said32 = three_way(swamd, d, (sub, -11, -1), pairs, "table 31")
    finally:
        d.close()
    assert (said16["launches"], said16["packed"], said16["items"]) == (1 + 3 + 2, 1, 1) and said32["launches"] == 1 + 2 + 1
    assert got[:, 1].tolist() == [32767, 31 * 1057, 32767, 31 * 1058]
    want = checked(checker, case, sub, (-11, -1), pairs)
    assert not differ(got, want), differ(got, want)


@pytest.mark.parametrize("gaps", lc.PACKED_GAPS + lc.FALLBACK_GAPS[:1] + [(-32769, 0)], ids=lambda g: f"{g[0]}_{g[1]}")
def test_lower_edge(engine, swamd, gaps):
    """gap_open + 2 gap_extend = -32768 runs packed, -32769 launches nothing packed; the bytes are the same."""
    case = lc.strips_case()
    d = OnDevice(engine, case)
    try:
        pairs = d.cross(11)
        got, said16, said32 = three_way(swamd, d, (lc.table24(), *gaps), pairs, f"table24 {gaps}")
    finally:
        d.close()
    assert np.array_equal(got[:, 1], lc.strips_ungapped()[pairs[:, 0], pairs[:, 1]])       # no alignment can pay such a gap
    packed = gaps[0] + 2 * gaps[1] >= -32768
    assert packed == (gaps in lc.PACKED_GAPS)
    assert said32["launches"] == 1 + 2 + 3 and said16["launches"] == 1 + (3 if packed else 2) + 3
    assert said16["packed"] == (3 if packed else 0) and said16["items"] == (two_pair_items(case, pairs) if packed else 0)


# ---- chunks, groups, workspaces ----

def test_cells_cut_by_chunk_borders(engine, swamd, world):
    w = world
    pairs = w["pairs"][:300]
    host = w["host"][:300]
    engine.set_option("search_pairs_chunk", 7)
    try:
        got, said16, said32 = three_way(swamd, w["d"], w["scoring"], pairs, "chunks of 7", host=host)
    finally:
        engine.set_option("search_pairs_chunk", 1 << 22)
    assert said16["chunks"] == said32["chunks"] == 43
    assert said16["packed"] == 43 * 3 and said16["launches"] == 1 + 43 * 6 and said32["launches"] == 1 + 43 * 5
    assert said16["items"] == two_pair_items(w["case"], pairs, chunk=7) > two_pair_items(w["case"], pairs)


def test_several_groups(engine, swamd, world):
    w = world
    pairs = w["pairs"][:300]
    engine.set_option("search_profile_mib", 1)
    try:
        got, said16, said32 = three_way(swamd, w["d"], w["scoring"], pairs, "1 MiB of profiles", host=w["host"][:300])
    finally:
        engine.set_option("search_profile_mib", 256)
    assert said16["groups"] == said32["groups"] >= 3
    assert said16["launches"] == said32["launches"] + said16["groups"] and said16["packed"] >= 3   # a third binning launch per group
    assert said16["items"] == two_pair_items(w["case"], pairs)                          # a cell belongs to one query, so to one group


def test_the_empty_half_comes_from_the_call_itself(swamd, world):
    """A large call, a call of singles only on the same context -- their items lie where the large call left full halves --, the large one again."""
    w = world
    live = np.nonzero(w["lens"] > 0)[0]
    singles = [(q, int(live[10 + q])) for q in range(7)]
    for _ in range(2):
        got, said, _ = three_way(swamd, w["d"], w["scoring"], w["pairs"], "large", host=w["host"])
        assert said["items"] > 600
        got, said, _ = three_way(swamd, w["d"], w["scoring"], singles, "singles")
        assert said["items"] == 7 and not differ(got, w["table"][[p[0] for p in singles], [p[1] for p in singles]])


def test_three_runs_give_the_same_bytes(world):
    w = world
    d_pairs = pairs_dev(w["d"].engine, w["pairs"])
    runs = [w["d"].run(w["scoring"], w["pairs"], 16, d_pairs=d_pairs)[0].tobytes() for _ in range(3)]
    assert runs[0] == runs[1] == runs[2] == w["host"].tobytes()


def test_buffer_contract(engine, world):
    """Guard bytes before and after d_results and d_pairs stay untouched, the pair list keeps its bytes, every poisoned result entry is
    overwritten.  d_pairs lies at an odd multiple of 8."""
    w = world
    torch = engine.torch
    dev = f"cuda:{engine.device}"
    pairs = np.concatenate([w["pairs"][:500], np.array([(-1, -1), (INT64_MAX, 0), (0, INT64_MAX)], np.int64)])
    n = len(pairs)
    raw_pairs = np.ascontiguousarray(pairs).view(np.uint8).reshape(-1)
    inp = bc.Arena(torch, dev, bc.arena_bytes(len(raw_pairs) + 128))
    d_raw, _ = inp.place(raw_pairs, 16, 8, name="pairs")
    assert d_raw.data_ptr() % 16 == 8
    d_pairs = d_raw.view(torch.int64).view(n, 2)
    out = bc.Arena(torch, dev, bc.arena_bytes(n * 24))
    c = out.carve(n * 24, 8, 0, name="results")
    res = out.view(c, torch.int64, (n * 3,))
    got, said = w["d"].run(w["scoring"], pairs, 16, d_pairs=d_pairs, out=res)
    assert said["packed"] == 3
    assert not differ(got[:500], w["host"][:500]) and not got[500:].any()
    raw = out.bytes_of(c).cpu().numpy().reshape(n, 24)
    assert not (raw == bc.POISON).all(axis=1).any() and (got[:, 2] == 0).all()           # every entry written, path_len included
    bc.assert_guards(out)
    bc.assert_guards(inp)


# ---- the one-call pipeline ----

def test_top_prefiltered_follows_the_option(engine, swamd, world):
    w = world
    d, case = w["d"], w["case"]
    S, top, min_score, cap = 60, 10, 1, d.nq * d.nt
    fp, fn, _ = swamd.prefilter_ungapped_host((case["qpacked"], case["qoffs"]), (case["packed"], case["offs"]), lc.table24(), S, want_scores=False)
    assert 0 < fn < (w["hosttab"][:, :, 1] > 0).sum()                                   # a strict, non-empty subset passes
    want_hits, want_nhits = swamd.top_hits_pairs_host(fp[:fn], w["hosttab"][fp[:fn, 0], fp[:fn, 1]], d.nq, d.nt, top, min_score)

    def call():
        t = engine.torch
        out = (t.full((d.nq * top * 3,), POISON64, dtype=t.int64, device=f"cuda:{engine.device}"), t.full((d.nq,), POISON64, dtype=t.int64, device=f"cuda:{engine.device}"))
        return d.db.search_affine_top_prefiltered_device(d.d_q, case["qoffs"], w["scoring"], S, cap, top, min_score, out=out)
    (h32, n32, c32), said32 = under(engine, 32, call)
    (h16, n16, c16), said16 = under(engine, 16, call)
    assert said32["packed"] == 0 and said16["packed"] == 3 and said16["items"] > 0
    assert h16.tobytes() == h32.tobytes() and n16.tobytes() == n32.tobytes() and int(c16[0]) == int(c32[0]) == fn
    assert np.array_equal(h16, want_hits) and np.array_equal(n16, want_nhits) and 0 < n16.max() <= top


# ---- the option ----

def test_option_values(engine, swamd, world):
    assert engine.get_option("search_pairs_lanes") == 32                                # the default
    for v in (0, 8, 64, -16):
        with pytest.raises(swamd.SwError) as e:
            engine.set_option("search_pairs_lanes", v)
        assert e.value.code == EINVAL and "search_pairs_lanes must be" in str(e.value)
        assert engine.get_option("search_pairs_lanes") == 32
    engine.set_option("search_pairs_lanes", 16)
    try:
        assert engine.get_option("search_pairs_lanes") == 16 and engine.get_option("search_lanes") == 32   # an option of its own
    finally:
        engine.set_option("search_pairs_lanes", 32)
    w = world
    pairs = w["pairs"][:50]
    # the counters read 0 after a call under 32 and after a call that launched nothing
    for lanes, packed in ((16, 3), (32, 0), (16, 3)):
        _, said = w["d"].run(w["scoring"], pairs, lanes)
        assert said["packed"] == packed and (said["items"] > 0) == (packed > 0)
    t = engine.torch
    _, said = under(engine, 16, lambda: w["d"].db.search_affine_pairs_device(w["d"].d_q, w["case"]["qoffs"], w["scoring"],
                                                                             t.zeros((0, 2), dtype=t.int64, device=f"cuda:{engine.device}")))
    assert said["packed"] == 0 and said["items"] == 0 and said["launches"] == 0
    # "search_lanes" does not reach the pair list
    engine.set_option("search_lanes", 16)
    try:
        _, said = w["d"].run(w["scoring"], pairs, 32)
    finally:
        engine.set_option("search_lanes", 32)
    assert said["packed"] == 0 and said["launches"] == 1 + 2 + 3
