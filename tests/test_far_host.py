"""CPU: the self-checks of tests/far_cases.py, and the host legs of the database-search family with their inputs beyond 4 GiB --
offsets[0] = FAR, qoffsets[0] = FAR, and PSSM columns whose index times nletters passes 2^32.  The arrays are numpy.empty and only the
pages of the payload and of the decoy 2^32 bytes below it are written, so resident memory stays a few MiB.  Expected values are the
checker's and the numpy reference's on the small arrays; the host legs run through the package's public functions, which hand the big
arrays on without a copy."""
import numpy as np
import pytest

import far_cases as fc
from affine_cases import checker  # noqa: F401


def far_array(desc, dtype=np.uint8):
    try:
        return fc.realise_numpy(desc, dtype)
    except MemoryError as e:                                                          # an address-space limit of this machine
        pytest.skip(f"numpy.empty({desc['size']}) was refused: {e}")


def placed(kind):
    p = fc.placement(kind)
    return p, far_array(p["q"]), far_array(p["db"])


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} words differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


# ---- self-checks ----

def test_every_far_constant_wraps_to_a_small_positive_offset():
    for name, v in fc.FAR_CONSTANTS.items():
        lo = v & 0xFFFFFFFF
        assert 2**32 <= v < 2**32 + 2**31 and lo == v - 2**32, name
        assert int(np.uint32(lo)) == int(np.int32(lo)) > 0, name                       # the same number as u32 and as int32
    for kind, (at, qat) in fc.PLACEMENTS.items():
        for v in (at, qat):
            assert v < 2**16 or v == fc.STRADDLE or v in fc.FAR_CONSTANTS.values(), kind


def test_far_buffer_puts_the_decoy_two_to_the_32_below():
    pay, dec = np.arange(1, 401, dtype=np.uint16).view(np.uint8), np.arange(1001, 1401, dtype=np.uint16).view(np.uint8)
    d = fc.far_buffer(pay, fc.FAR, dec)
    assert [at for at, _ in d["pieces"]] == [fc.FAR - 2**32, fc.FAR] and d["size"] == fc.FAR + 800 + fc.TAIL
    buf = far_array(d)
    assert np.array_equal(buf[fc.FAR:fc.FAR + 800], pay) and np.array_equal(buf[fc.FAR - 2**32:fc.FAR - 2**32 + 800], dec)
    d = fc.far_buffer(pay, fc.STRADDLE, dec)                                           # the decoy's first 150 bytes would lie below 0
    assert d["pieces"][0][0] == 0 and np.array_equal(d["pieces"][0][1], dec[150:]) and d["pieces"][1][0] == fc.STRADDLE
    d = fc.far_buffer(pay, 3, dec)                                                     # near: no decoy
    assert len(d["pieces"]) == 1 and d["size"] == 3 + 800 + fc.TAIL


def test_placements_keep_the_world_and_move_only_its_bytes():
    w = fc.world()
    for kind in fc.PLACEMENTS:
        p = fc.placement(kind)
        assert p["offs"][0] == fc.PLACEMENTS[kind][0] and p["qoffs"][0] == fc.PLACEMENTS[kind][1]
        assert np.diff(p["offs"]).tolist() == [fc.TLENS[k] for k in p["order"]] and np.diff(p["qoffs"]).tolist() == fc.QLENS
        at, pay = p["db"]["pieces"][-1]
        assert at == p["offs"][0] and np.array_equal(pay, np.concatenate([w["targets"][k] for k in p["order"]]))
    p = fc.placement("db_straddle")
    assert p["offs"][0] < 2**32 < p["offs"][1] and p["offs"][1] - p["offs"][0] == 300


def test_the_decoy_changes_every_result(checker):  # noqa: F811
    bad = fc.decoy_failures(checker)
    assert not bad, f"{len(bad)} (kind, mixture, query, target) keep their result under the decoy, first {bad[:5]}: change DECOY_SEED"


def test_expected_values_are_read_only_and_complete(checker):  # noqa: F811
    exp = fc.expected(checker)
    assert exp is fc.expected(checker)
    for g in fc.GAPS:
        assert exp["R"][g].shape == (fc.NQ, fc.NT, 3) and not exp["R"][g].flags.writeable
        live = np.array(fc.TLENS) > 0
        assert (exp["R"][g][:, live, 1] > 0).all() and not exp["R"][g][:, ~live].any()
        assert (exp["U"] <= exp["R"][g][:, :, 1]).all()                               # a gapless alignment is a local alignment
    hits, nhits = fc.hit_table(exp, fc.GAPS[0])
    assert nhits.tolist() == [fc.TOP] * fc.NQ
    fh, fn = fc.prefiltered_table(exp, fc.GAPS[0])
    assert 0 < fn.sum() < nhits.sum() or not np.array_equal(fh, hits)                  # the threshold removes something
    pr = fc.pair_list()
    assert (pr[:, 0] < 0).any() and (pr[:, 1] == fc.NT).any() and any(fc.TLENS[t] == 0 for q, t in pr if 0 <= t < fc.NT and q >= 0)


def test_pssm_layouts_cross_by_the_product(checker):  # noqa: F811
    for nl, col in fc.PSSM_FAR.items():
        desc, offs = fc.pssm_layout(nl, col)
        assert offs[0] == col < 2**32 <= col * nl and desc["size"] % nl == 0
        assert [at for at, _ in desc["pieces"]] == [col * nl - 2**32, col * nl]
        m = fc.pssm_of(fc.world()["queries"], nl)
        assert m.shape == (sum(fc.QLENS), nl) and m.max() <= fc.SMAX


def test_the_decoy_condition_excuses_one_query_of_the_weights_only():
    """sw_db_pssm_hit_weights and sw_db_pssm_from_hits are part of fc.decoy_failures() (empty, above).  One query is excused, by name:
    query 0 of the weights has one column, and four residues on one column weigh the same whenever they are four different letters
    -- in the world and in the decoy alike.  Its update is NOT excused, nor is any other query of either call."""
    assert fc.HITS_EXCUSED == [("pssm_hit_weights", 0)] and fc.QLENS[0] == 1
    assert (fc.PRIOR_WEIGHT, fc.PRIOR_WEIGHT_WEIGHTED, fc.PER_HIT, fc.INCLUDE_MIN) == (2, 512, 256, 1)


def test_hits_case_host_legs_equal_the_rules(swamd, checker):  # noqa: F811
    """The small world's update and weights: the host legs equal the numpy rules that the GPU tests take as expected."""
    import pssm_hits_cases as hc
    import pssm_weights_cases as wc
    exp = fc.expected(checker)
    for g in fc.GAPS:
        for nl in (24, 256):
            for order in (fc.NATURAL_ORDER, fc.STRADDLE_ORDER):
                c = fc.hits_case(exp, g, order, nl)
                w, m, counts = fc.hits_want(c, True)
                assert w.any() and counts.any()
                same(wc.host_leg(swamd, c, fc.PER_HIT, fc.INCLUDE_MIN), w, "weights")
                out, cnt = hc.host_leg(swamd, c, fc.PRIOR_WEIGHT_WEIGHTED, fc.INCLUDE_MIN, w)
                same(out, m, "matrix")
                same(cnt, counts, "counts")


def test_count_case_crosses_4gib_and_its_windows_equal_the_rule(swamd):
    import pssm_hits_cases as hc
    cc = fc.count_case()
    m, counts = fc.count_want()
    c = cc["compact"]
    out, cnt = hc.host_leg(swamd, c, fc.COUNT_PW, fc.COUNT_INC, c.weights)
    same(out, m, "matrix")
    same(cnt, counts, "counts")
    L, nl = fc.COUNT_QLEN, fc.COUNT_NL
    assert int(cc["qoffs"][-1]) * nl * 4 > 2**32 > int(cc["qoffs"][-2]) * nl * 4
    last = [(q * L + c0) * nl * 4 for q, c0, n, r in cc["windows"] if q == fc.COUNT_NQ - 1]
    assert len(last) == 4 and min(last) > 2**32                                        # every live count of the last query lies beyond the line
    assert counts[-62:].sum() > 0 and cc["windows"][-1][1] + 62 == L                   # ... up to its last column


# ---- the host legs ----

KINDS = ["db_far", "db_straddle", "q_far", "both_far"]


@pytest.mark.parametrize("kind", KINDS)
def test_search_pairs_and_prefilter_host(swamd, checker, kind):  # noqa: F811
    exp = fc.expected(checker)
    p, q, db = placed(kind)
    order = p["order"]
    for g in fc.GAPS:
        got = swamd.search_affine_multi_host((q, p["qoffs"]), (db, p["offs"]), (fc.table24(), *g))
        same(got, exp["R"][g][:, order], f"{kind} {g}: sw_search_affine_multi_host")
        pr = fc.pair_list()
        got = swamd.search_affine_pairs_host((q, p["qoffs"]), (db, p["offs"]), (fc.table24(), *g), pr)
        same(got, fc.pair_results(exp, g, pr, order), f"{kind} {g}: sw_search_affine_pairs_host")
    pairs, n, scores = swamd.prefilter_ungapped_host((q, p["qoffs"]), (db, p["offs"]), fc.table24(), fc.PREFILTER_MIN)
    u = exp["U"][:, order]
    same(scores, u, f"{kind}: sw_prefilter_ungapped_host scores")
    want = np.argwhere((u >= fc.PREFILTER_MIN) & (np.diff(p["offs"]) > 0)[None, :])
    assert n == len(want) and np.array_equal(pairs[:n], want) and (pairs[n:] == -1).all(), kind


@pytest.mark.parametrize("kind", KINDS)
def test_align_hits_host(swamd, checker, kind):  # noqa: F811
    exp = fc.expected(checker)
    p, q, db = placed(kind)
    for g in fc.GAPS:
        hits, nhits = fc.hit_table(exp, g, p["order"])
        aln, ops = swamd.align_affine_hits_host((q, p["qoffs"]), (db, p["offs"]), (fc.table24(), *g), hits, nhits)
        want, wops = fc.alignments(exp, g, hits, nhits, p["order"])
        same(aln, want, f"{kind} {g}: sw_align_affine_hits_host")
        assert ops == wops, f"{kind} {g}: ops"


@pytest.mark.parametrize("db_kind", ["near", "db_far"])
@pytest.mark.parametrize("nletters", [256, 24])
def test_pssm_host_columns_cross_by_the_product(swamd, checker, nletters, db_kind):  # noqa: F811
    exp = fc.expected(checker)
    p = fc.placement(db_kind)
    db = far_array(p["db"])
    desc, moffs = fc.pssm_layout(nletters, fc.PSSM_FAR[nletters])
    m = far_array(desc, np.int8)
    for g in fc.GAPS:
        scoring = fc.pssm_scoring(nletters, g)
        got = swamd.search_pssm_multi_host((m, moffs), (db, p["offs"]), scoring)
        same(got, exp["R"][g], f"nletters {nletters} {db_kind} {g}: sw_search_pssm_multi_host")
        hits, nhits = fc.hit_table(exp, g)
        aln, ops = swamd.align_pssm_hits_host((m, moffs), (db, p["offs"]), scoring, hits, nhits)
        want, wops = fc.alignments(exp, g, hits, nhits)
        same(aln, want, f"nletters {nletters} {db_kind} {g}: sw_align_pssm_hits_host")
        assert ops == wops
