"""CPU: the sessions of tests/session_cases.py before any GPU sees them.  Every step's expectation comes from the independent
references alone and the library's host leg of the same call must equal it; then the conditions that keep a step of the GPU test from
passing on stale state -- what an earlier call of another shape or scoring left in a shared buffer -- are asserted on the references:

  * scores: a step's table, recomputed under the scoring of the step before it in its context (whatever its kind: a table, a PSSM read
    as the checker's table, the match and mismatch scores of a linear search) and, where that is another step, under the scoring of
    the last earlier step of its own kind (a 64 KiB table, or a PSSM's letters), differs from its own in at least one entry of every
    query that has a non-empty target, and holds a non-zero score;
  * a table call whose table is the first upload behind a PSSM call's code table: with row 0 of its table replaced by that code table
    the step's expected table changes for every query that holds the byte 0 (every query of more than one letter does), and the
    table differs from the last table before it inside those 256 bytes and beyond them;
  * every selecting step selects something and `top` cuts at least one row; the pre-filter passes a strict, non-empty subset;
  * the packed steps are eligible for 16-bit lanes;
  * the growing session grows.

Growth is taken of the running maxima of session_cases.Step.measures(), which is what a workspace's size follows: the session ends on
its small first call and runs the one-query calls behind the forty queries, so the values of the steps themselves are not monotone.
What is asserted: each of the maxima rises strictly at least once behind the first step, and every step raises at least one of them
or is the first to use one of session_cases.WORKSPACES -- but for the four steps of session_cases.REUSING, exactly.  No GPU is needed.

The fourth session (session_cases.ITERATING: five sw_db_pssm_from_hits calls back to back) has tests of its own at the end: the tables
its first two steps leave are the checker's, every update's host leg equals the numpy rule, and no update could pass on the S, the
code table or the offsets of the update before it or of the one two before it, whose pinned copy it rewrites.

The fifth session (session_cases.WEIGHTED: sw_db_pssm_hit_weights and sw_db_pssm_from_hits in turn on two streams) likewise: the host
legs chained equal the numpy rules, the shared table and the accumulators grow where the session says they do, and no weights call or
update could pass on the code table, the offsets, the S or the accumulators of any other step of the session."""
import ctypes

import numpy as np
import pytest

import pairs_top_cases as ptc
import pssm_cases
import session_cases as sc
from affine_cases import checker  # noqa: F401
from align_cases import replay


@pytest.fixture(scope="module")
def expect(checker, oracle, swamd):  # noqa: F811
    return sc.Expect(checker, oracle, swamd)


def contexts():
    """{name: the steps one context runs, in enqueue order}."""
    a, b = sc.two_contexts()
    return {"growing": sc.growing(0) + sc.growing(1), "shrinking": sc.shrinking(0) + sc.shrinking(1), "two_a": a, "two_b": b}


ALL_STEPS = sc.growing(0) + sc.growing(1)


def sets_of(step):
    d = sc.databases()[step.db]
    if step.ty is not None:
        return (step.ty.matrix, step.ty.qoffs), (d["packed"], d["offs"])
    qs = sc.query_sets()[step.q]
    return (qs["qpacked"], qs["qoffs"]), (d["packed"], d["offs"])


def check_alignments(step, e, full, table, counts):
    """Every used entry inside the database: the ops replay over the letters to the alignment's own score, which is the checker's;
    every other entry is the zero alignment."""
    d = sc.databases()[step.db]
    nt, seen = len(d["targets"]), 0
    for q, query in enumerate(step.queries):
        used = table.shape[1] if counts is None else int(np.clip(counts[q], 0, table.shape[1]))
        for r in range(table.shape[1]):
            k = int(table[q, r, 0])
            if r < used and 0 <= k < nt:
                assert tuple(e["aln"][q, r, :2]) == tuple(full[q, k, :2]), (step.name, q, r)
                replay(query, d["targets"][k], step.checker_table, *step.gaps, e["aln"][q, r], e["ops"][q][r])
                seen += e["aln"][q, r, 1] > 0
            else:
                assert not e["aln"][q, r].any() and e["ops"][q][r] == b"", (step.name, q, r)
    assert seen > 0, step.name


@pytest.mark.parametrize("step", ALL_STEPS, ids=lambda s: f"{s.name}-{s.p}")
def test_host_leg_equals_the_references(swamd, oracle, expect, step):
    e = expect.of(step, sc.by_name(sc.growing(step.p)))
    c = step.call
    if c == "fill":
        a, b = sc.fill_pair()
        H, P = np.zeros_like(e["H"]), np.zeros_like(e["P"])
        r = swamd._Result()
        scores = swamd._Scores(*swamd.DEFAULT_SCORES)
        aa, bb = np.concatenate([a, np.zeros(1, np.uint8)]), np.concatenate([b, np.zeros(1, np.uint8)])
        assert swamd.lib().sw_fill_cpu(aa.ctypes.data, len(a), bb.ctypes.data, len(b), ctypes.byref(scores), H.ctypes.data, P.ctypes.data, ctypes.byref(r)) == 0
        assert np.array_equal(H, e["H"]) and np.array_equal(P, e["P"]) and (r.max_pos, r.max_score) == (e["max_pos"], e["max_score"]) and r.max_score > 0
        return
    queries, targets = sets_of(step)
    d = sc.databases()[step.db]
    nq, nt = len(step.queries), len(d["targets"])
    empty = np.diff(d["offs"]) == 0
    if c == "search_affine":
        got = swamd.search_affine_multi_host(queries, targets, (step.sub, *step.gaps))
        assert np.array_equal(got, e["results"]) and not got[:, empty].any() and got[:, :, 1].max() > 0
    elif c == "search_pssm":
        got = swamd.search_pssm_multi_host(queries, targets, step.ty.scoring(*step.gaps))
        assert np.array_equal(got, e["results"]) and not got[:, empty].any() and got[:, :, 1].max() > 0
    elif c == "search_affine_top":
        hits, nhits = swamd.search_affine_multi_top_host(queries, targets, (step.sub, *step.gaps), step.top, step.min_score)
        assert np.array_equal(hits, e["hits"]) and np.array_equal(nhits, e["nhits"])
    elif c == "search_pssm_top":
        full = swamd.search_pssm_multi_host(queries, targets, step.ty.scoring(*step.gaps))
        hits, nhits = pssm_cases.rank_order(full, step.top, step.min_score)
        assert np.array_equal(full, expect.full(step)) and np.array_equal(hits, e["hits"]) and np.array_equal(nhits, e["nhits"])
    elif c == "prefilter":
        pairs, n, scores = swamd.prefilter_ungapped_host(queries, targets, step.sub, step.min_score, step.cap)
        assert n == e["npairs"] and np.array_equal(pairs[:n], e["pairs"]) and (pairs[n:] == -1).all() and np.array_equal(scores, e["scores"])
        assert 0 < n < int((~empty).sum()) * nq                                         # a strict, non-empty subset
    elif c == "search_pairs":
        got = swamd.search_affine_pairs_host(queries, targets, (step.sub, *step.gaps), e["pairs"])
        assert np.array_equal(got, e["results"]) and got[:, 1].max() > 0
    elif c == "top_pairs":
        names = sc.by_name(sc.growing(step.p))
        src = expect.of(names[step.source], names)
        hits, nhits = swamd.top_hits_pairs_host(src["pairs"], src["results"], nq, nt, step.top, step.min_score)
        assert np.array_equal(hits, e["hits"]) and np.array_equal(nhits, e["nhits"])
    elif c == "top_prefiltered":
        pairs, n, _ = swamd.prefilter_ungapped_host(queries, targets, step.sub, sc.PREFILTER_MIN, step.cap, want_scores=False)
        res = swamd.search_affine_pairs_host(queries, targets, (step.sub, *step.gaps), pairs[:n])
        hits, nhits = swamd.top_hits_pairs_host(pairs[:n], res, nq, nt, step.top, step.min_score)
        assert n == e["npairs"] and 0 < n < int((~empty).sum()) * nq
        assert np.array_equal(hits, e["hits"]) and np.array_equal(nhits, e["nhits"])
    elif c in ("align_affine_hits", "align_pssm_hits"):
        check_alignments(step, e, expect.full(step), e["table"], e["counts"])
    elif c == "align_affine_one":
        full = expect.full(step)
        assert (e["aln"][:, 6] > 0).any()
        for h, k in enumerate(step.hits):
            assert tuple(e["aln"][h, :2]) == tuple(full[0, k, :2]), (step.name, h)
            replay(step.queries[0], d["targets"][k], step.sub, *step.gaps, e["aln"][h], e["ops"][h])
    elif c == "search_linear":
        got = swamd.search_affine_host(step.queries[0], targets, swamd.submat_match(*step.linear[:2]), 0, step.linear[2])
        assert np.array_equal(got, e["results"]) and got[:, 1].max() > 0
        for k in (1, 77, 198):                                                          # the fill oracle says the same of the linear recurrence
            o = oracle.fill_streaming(step.queries[0], d["targets"][k], step.linear)
            assert (o["max_pos"], o["max_score"]) == tuple(e["results"][k, :2]), k
    elif c == "search_affine_one":
        got = swamd.search_affine_host(step.queries[0], targets, step.sub, *step.gaps)
        assert np.array_equal(got, e["results"]) and got[:, 1].max() > 0
    else:
        raise AssertionError(c)
    if c in sc.SELECTING_CALLS:
        if c in ("top_pairs", "top_prefiltered"):
            pr = expect.of(sc.by_name(sc.growing(step.p))["prefilter"])["pairs"] if c == "top_pairs" else expect.ungapped(step)[1]
            candidates = np.bincount(pr[:, 0], minlength=nq)
        else:
            candidates = (expect.full(step)[:, :, 1] >= step.min_score).sum(axis=1)
        assert e["nhits"].sum() > 0 and (candidates > step.top).any(), f"{step.name}: nothing selected, or top cuts no row"
        assert (e["nhits"] <= np.minimum(candidates, step.top)).all() and (e["nhits"] == step.top).any()


def scored(step):
    return step.checker_table is not None and step.call not in ("fill", "top_pairs")


@pytest.mark.parametrize("name", list(contexts()))
def test_no_step_passes_on_the_previous_scoring(expect, name):
    steps = contexts()[name]
    last = {"table": None, "pssm": None}           # the last step that uploaded a 64 KiB table / a PSSM's code table
    before = None                                  # the last step with a scoring of any kind: its profiles are what the workspace holds
    uploaded = None                                # what the scoring table's two copies hold last: "table" or "pssm"
    same_kind = across = row0 = 0
    for step in steps:
        if not scored(step):
            continue                               # the selection of a list and the fill have no scoring
        kind = step.kind                           # (None: the linear search uploads no table)
        filters = step.call in ("prefilter", "top_prefiltered")
        own = expect.full(step) if step.call != "prefilter" else None
        offs = sc.databases()[step.db]["offs"]
        if own is not None:
            assert own[:, :, 1].max() > 0, step.name

        def differs(tab, gaps, only=None):
            ok = True
            if filters:
                ok = sc.ungapped_differs(step, tab, expect.ungapped(step)[0], only)
            if own is not None:
                ok = ok and sc.differs_per_query(own, expect.full_under(step, tab, gaps), offs, only)
            return ok

        if before is not None:                     # the step before it, whatever its kind
            gaps = before.checker_gaps if before.call != "prefilter" else step.checker_gaps
            assert differs(before.checker_table, gaps), (step.name, before.name)
            across += 1
        prev = last[kind] if kind else None
        if prev is not None and prev is not before:
            if kind == "table":
                assert not np.array_equal(step.sub, prev.sub), (step.name, prev.name)
                assert differs(prev.sub, prev.gaps if prev.call != "prefilter" else step.gaps), (step.name, prev.name)
            else:                                  # the step's matrix read through the previous PSSM's letters, clamp and gaps
                alt = np.full((256, 256), prev.ty.other, np.int8)
                alt[:, prev.ty.letters] = np.minimum(step.ty.types, prev.ty.smax)
                assert not np.array_equal(step.ty.letters, prev.ty.letters)
                assert differs(alt, prev.gaps), (step.name, prev.name)
            same_kind += 1
        if kind == "table" and uploaded == "pssm":  # row 0 of the table's copies holds the PSSM's code table until this call's upload
            alt = step.sub.copy()
            alt[0] = sc.code_row(last["pssm"].ty)
            holds0 = [k for k, q in enumerate(step.queries) if (q == 0).any()]
            assert holds0 == [k for k, q in enumerate(step.queries) if len(q) > 1], step.name
            assert differs(alt, step.gaps, holds0), (step.name, last["pssm"].name)
            if last["table"] is not None:
                new, old = step.sub.reshape(-1), last["table"].sub.reshape(-1)
                assert (new[:256] != old[:256]).any() and (new[256:] != old[256:]).any(), step.name
            row0 += 1
        if kind:
            last[kind], uploaded = step, kind
        before = step
    nscored = len([s for s in steps if scored(s)])
    assert across == nscored - 1 and same_kind >= 3
    assert row0 >= (3 if name == "growing" else 2) * len({s.p for s in steps})   # table calls per pass that take over from a PSSM's code table


# ---- the fourth session: updates back to back ----

def test_iterating_first_world_holds_the_checkers_tables(swamd, checker):  # noqa: F811
    """Steps 1 and 2 of the session (search_pssm_top, align_pssm_hits) leave the tables of worlds[0]: they are the rank order of the
    checker's scores and the rule's alignments over the checker's matrices."""
    from align_cases import expected
    import pssm_hits_cases as phc
    c = sc.iterating(swamd)["worlds"][0]
    tab = sc.sequence_table(c.sub, c.letters, c.other, c.smax)
    full = np.stack([checker.search(q, c.packed, c.offs, tab, -10, -1) for q in c.queries])
    hits, nhits = pssm_cases.rank_order(full, sc.UPDATE_TOPS[0], sc.ITER_MIN_SCORE)
    assert np.array_equal(hits, c.hits) and np.array_equal(nhits, c.nhits) and nhits.min() >= 1 and (nhits == sc.UPDATE_TOPS[0]).any()
    top = sc.UPDATE_TOPS[0]
    for q, query in enumerate(c.queries):
        for r in range(top):
            if r < nhits[q]:
                k = int(hits[q, r, 0])
                row, ops, _ = expected(checker, query, c.packed[c.offs[k]:c.offs[k + 1]], tab, -10, -1)
                assert tuple(c.aln[q, r]) == row and c.ops[q * top + r, :row[6]].tobytes() == ops, (q, r)
            else:
                assert not c.aln[q, r].any()
    assert phc.scoring(c)[3:] == (-10, -1)


def test_iterating_updates_equal_the_rule_and_their_shapes_differ(swamd):
    import pssm_hits_cases as phc
    worlds = sc.iterating(swamd)["worlds"]
    assert [len(c.letters) for c in worlds] == sc.UPDATE_NLETTERS == [4, 24, 256, 4, 24]
    assert [n for n, _ in sc.ITERATING[4:9]] == [f"update{k}" for k in range(5)] and [s for _, s in sc.ITERATING[4:9]] == [0, 1, 0, 1, 0]
    assert len({len(c.qoffs) for c in worlds}) == 5 and len({c.pw for c in worlds}) == 5 and len({c.hits.shape[1] for c in worlds}) == 5
    for c in worlds:
        out, _ = phc.host_leg(swamd, c, c.pw, c.inc)
        want = sc.update_expected(c)
        front = int(c.qoffs[0])
        assert np.array_equal(out, want[front:]) and (want[front:] != np.minimum(c.prior[front:], c.smax)).any()


def rows_differ_in_every_query(c, a, b):
    return all((a[c.qoffs[q]:c.qoffs[q + 1]] != b[c.qoffs[q]:c.qoffs[q + 1]]).any() for q in range(len(c.qoffs) - 1))


def test_iterating_no_update_could_pass_on_stale_state(swamd):
    """For every update and the updates one and two before it (two before: the one whose pinned copy it rewrites): its expected matrix
    differs in every query under the other's S and under the other's code table, and differs under the other's offsets wherever
    the other has as many queries and its columns fit."""
    worlds = sc.iterating(swamd)["worlds"]
    fits = 0
    for k, c in enumerate(worlds):
        own = sc.update_expected(c)
        for back in (1, 2):
            if k - back < 0:
                continue
            o = worlds[k - back]
            assert rows_differ_in_every_query(c, own, sc.update_expected(c, sub=o.sub)), (k, back, "S")
            assert rows_differ_in_every_query(c, own, sc.update_expected(c, code=sc.code_of(o.letters))), (k, back, "letters")
            assert not np.array_equal(c.qoffs, o.qoffs[:len(c.qoffs)])
        if k >= 1:
            o = worlds[k - 1]
            if len(o.qoffs) >= len(c.qoffs) and o.qoffs[len(c.qoffs) - 1] <= c.qoffs[-1]:
                fits += 1
                assert not np.array_equal(own, sc.update_expected(c, qoffs=o.qoffs)), (k, "offsets")
    assert fits >= 3


def test_iterating_search_on_the_fifth_matrix(swamd, checker):  # noqa: F811
    import pssm_hits_cases as phc
    c = sc.iterating(swamd)["worlds"][4]
    m = sc.update_expected(c)
    want = sc.iterating_search_again(checker, c, m)
    got = swamd.search_pssm_multi_host((m, c.qoffs), (c.packed, c.offs), phc.scoring(c))
    assert np.array_equal(got, want) and want[:, :, 1].max() > 0
    hits, nhits = pssm_cases.rank_order(want, sc.ITER_TOP_AGAIN, sc.ITER_MIN_SCORE)
    assert nhits.min() >= 1
    # the search reads the NEW matrix: under the prior the table is another
    assert not np.array_equal(want, sc.iterating_search_again(checker, c, c.prior))


def test_iterating_packed_steps_are_eligible_and_select(swamd, expect):
    it = sc.iterating(swamd)
    d, qs = sc.databases()["db200"], sc.query_sets()["seven"]
    longest = int(np.diff(d["offs"]).max())
    sub = sc.packed_table(0)
    assert all(max(int(sub.max()), 0) * min(len(q), longest) <= 32767 for q in qs["queries"]) and sc.lc.GAPS[0][0] + 2 * sc.lc.GAPS[0][1] >= -32768
    pairs = it["pairs"]
    assert (pairs[140:] == -1).all() and (pairs[:140] >= 0).all() and np.array_equal(pairs[100:110], pairs[:10])
    u, pr = sc.iterating_prefilter()
    assert 0 < len(pr) < (np.diff(sc.databases()["db40"]["offs"]) > 0).sum() * 40


def test_the_packed_steps_are_eligible():
    packed = [s for s in ALL_STEPS if s.packed]
    assert len(packed) == sc.PASSES and all(s.lanes == 16 for s in packed) and all(s.lanes == 32 for s in ALL_STEPS if not s.packed)
    for s in packed:
        longest = int(np.diff(sc.databases()[s.db]["offs"]).max())
        assert all(int(s.sub.max()) * min(len(q), longest) <= 32767 for q in s.queries)
        assert s.gaps[0] + 2 * s.gaps[1] >= -32768


def test_the_growing_session_grows():
    steps = sc.growing(0)
    names = [s.name for s in steps]
    m = np.array([s.measures() for s in steps])
    running = np.maximum.accumulate(m, axis=0)
    assert (running[-1] > running[0]).all()                                             # each of the measures rises strictly at least once
    used, reusing = set(sc.WORKSPACES[steps[0].call]), []
    for i in range(1, len(steps)):
        first_use = set(sc.WORKSPACES[steps[i].call]) - used
        used |= first_use
        if not (m[i] > running[i - 1]).any() and not first_use:
            reusing.append(names[i])
    assert tuple(reusing) == sc.REUSING, f"steps that need no more of anything and use nothing first: {reusing}"
    assert (m[1:names.index("prefilter") + 1, :4] > running[:names.index("prefilter"), :4]).any(axis=1).all()   # up to the pre-filter by size alone
    assert tuple(m[-1]) == tuple(m[0]) and (m[-1] <= running[-2]).all()                 # the small call on workspaces far larger than it needs
    assert [s.stream for s in steps].count(1) == 1 and steps[names.index("align_hits")].stream == 1


def test_the_other_sessions_are_the_same_steps():
    for p in range(sc.PASSES):
        g, s = sc.growing(p), sc.shrinking(p)
        assert sorted(x.key for x in g) == sorted(x.key for x in s) and s[0].name == "top_packed"
        assert [x.stream for x in s] == [i % 2 for i in range(len(s))]
        order = [x.name for x in s]
        assert [n for n in order if n in sc.CHAIN] == list(sc.CHAIN)                    # producers stay in front of their consumers
    a, b = sc.two_contexts()
    assert {x.stream for x in a} == {0} and {x.stream for x in b} == {1} and len(a) == len(b)


# ---- the fifth session ----

def test_weighted_host_legs_equal_the_rules_and_the_workspaces_grow(swamd):
    import pssm_hits_cases as phc
    import pssm_weights_cases as pwc
    worlds = sc.weighted(swamd)["worlds"]
    steps, (hits, nhits), full = sc.weighted_expected(swamd)
    assert [len(c.letters) for c in worlds] == sc.WEIGHT_NLETTERS == [4, 24, 256]
    assert [n for n, _ in sc.WEIGHTED] == ["pssm_top", "align", "weights0", "update0", "weights1", "update1", "weights2", "update2", "pssm_top_again"]
    assert [st for _, st in sc.WEIGHTED] == [0, 1, 0, 1, 0, 1, 0, 1, 0]
    nqs = [len(c.qoffs) - 1 for c in worlds]
    assert nqs == sorted(set(nqs)) and len({c.hits.shape[1] for c in worlds}) == 3 and len({c.per_hit for c in worlds}) == 3
    for c, (w, m) in zip(worlds, steps):
        front = int(c.qoffs[0])
        rw, _, used = pwc.reference(c, c.per_hit, c.inc)
        assert np.array_equal(w, rw)
        assert sum(len(set(w[q][used[q]].tolist())) > 1 for q in range(len(w))) >= 3          # the rule is at work: the hits of a query weigh differently
        rm, _, _ = phc.reference(c, c.pw, c.inc, w)
        assert np.array_equal(m[front:], rm[front:]) and (m[front:] != np.minimum(c.prior[front:], c.smax)).any()
        assert not np.array_equal(rm, phc.reference(c, c.pw, c.inc)[0])                 # the weights matter to the matrix
    # the table's need in call order: the two layouts in turn, a larger table before update0, update1 and update2; the accumulators grow twice
    needs, cap, grew = [], 0, []
    for k, c in enumerate(worlds):
        wn, un, acc = sc.table_needs(c)
        needs += [(f"weights{k}", wn), (f"update{k}", un)]
    for name, n in needs:
        if n > cap:
            grew.append(name)
            cap = n
    assert grew == ["weights0", "update0", "update1", "update2"]
    accs = [sc.table_needs(c)[2] for c in worlds]
    assert accs[0] < accs[1] < accs[2]
    # the search on the last matrix reads the NEW matrix
    c = worlds[-1]
    assert nhits.min() >= 0 and nhits.max() >= 1 and full[:, :, 1].max() > 0
    assert not np.array_equal(full, swamd.search_pssm_multi_host((c.prior, c.qoffs), (c.packed, c.offs), phc.scoring(c)))


def test_weighted_no_step_could_pass_on_another_steps_state(swamd):
    """For every world and every OTHER world of the session (the table a call reads may be the one an earlier call left or the one a
    later call on the other stream has already written): the weights differ in every query with more than two used entries under the
    other's code table (but where that table merely relabels the residues, once: the 256 letters under the 24), and differ under the
    other's offsets and on top of the other's accumulators; the matrix differs in every query
    under the other's S and code table and differs under its offsets where they fit."""
    import pssm_hits_cases as phc
    import pssm_weights_cases as pwc
    worlds = sc.weighted(swamd)["worlds"]
    steps, _, _ = sc.weighted_expected(swamd)
    checked = [0, 0]
    for k, c in enumerate(worlds):
        w, m = steps[k]
        used = pwc.reference(c, c.per_hit, c.inc)[2]
        varied = [q for q in range(len(w)) if used[q].sum() > 2]
        assert len(varied) >= 3
        upd = lambda **kw: phc.reference(_with(c, **kw), c.pw, c.inc, w, code=kw.get("code"))[0]  # noqa: E731
        for j, o in enumerate(worlds):
            if j == k:
                continue
            code = sc.code_of(o.letters)
            wc_ = sc.weights_under(c, code=code)
            places = code[np.unique(c.packed[int(c.offs[0]):])]
            if (places >= 0).all() and places.max() < len(c.letters) and len(set(places.tolist())) == len(places):
                # the other table only relabels the bytes of this world's targets: the weights cannot tell (the rule counts which residues
                # coincide, not which they are); the update of the same step, which reads the same table, can -- below
                assert np.array_equal(wc_, w) and (k, j) == (2, 1)
            else:
                assert wc_ is None or all((wc_[q] != w[q]).any() for q in varied), (k, j, "weights: code table")
            assert not np.array_equal(c.qoffs, o.qoffs[:len(c.qoffs)])
            if len(o.qoffs) >= len(c.qoffs):
                wo = sc.weights_under(c, qoffs=o.qoffs)
                assert wo is None or not np.array_equal(wo, w), (k, j, "weights: offsets")
                checked[0] += 1
            wa = sc.weights_under(c, acc=pwc.accumulators(o, o.inc)[:2])
            assert wa is None or not np.array_equal(wa, w), (k, j, "weights: accumulators")
            assert rows_differ_in_every_query(c, m, upd(sub=o.sub)), (k, j, "update: S")
            assert rows_differ_in_every_query(c, m, upd(code=code)), (k, j, "update: code table")
            if len(o.qoffs) >= len(c.qoffs) and o.qoffs[len(c.qoffs) - 1] <= c.qoffs[-1]:
                assert not np.array_equal(m, upd(qoffs=np.ascontiguousarray(o.qoffs[:len(c.qoffs)]))), (k, j, "update: offsets")
                checked[1] += 1
    assert checked == [3, 2]                                  # every world under each later one; the matrix where the later one's columns fit


def _with(c, sub=None, code=None, qoffs=None):
    import types
    v = types.SimpleNamespace(**vars(c))
    if sub is not None:
        v.sub = sub
    if qoffs is not None:
        v.qoffs = qoffs
    return v
