"""GPU: the sessions of tests/session_cases.py -- every search and alignment family of one context enqueued back to back on a fresh
context.  Every call stages through the same pinned copies (schedule, query table, scoring table) and device workspaces, so what
keeps one call's state from another's is the library's own ordering alone: the event wait before a pinned copy is rewritten, the drain
before a workspace is freed, the wait behind the device's previous call on another stream, the memsets in front of every launch.

A test allocates every input, handle and output first (outputs poisoned, the hit tables and alignments carved out of a guarded arena),
synchronises once, enqueues all steps without synchronising, copying to the host or reading a device value in between -- options are
host state and so are the "last_*" routes read here: sw_get_option reads fields of the context for all of them but
"last_align_hits_lists", which is not used --, synchronises once more and compares every output bit for bit with the expectation of
test_session_host.py.  The growing session runs twice on its context, the second time with a second set of tables on warm workspaces.

Each test prints what it observed of the overlap (whether the first step's event and which others were still pending when the last
enqueue returned, which steps were still running when the enqueue of the next returned, the time of the enqueue loop and of the
drain); nothing of that is asserted: DESIGN section 9o records the figures.  The references of all three tests are computed once, by
the first test that needs them.

The fourth session (session_cases.ITERATING) puts sw_db_pssm_from_hits into such a row: five updates back to
back on alternating streams behind the search and the alignment that feed the first, with the packed pair-list and pre-filter
routes in between.

The fifth (session_cases.WEIGHTED) alternates sw_db_pssm_hit_weights on stream 0 with the sw_db_pssm_from_hits on stream 1 that takes
its output as d_weights: the two calls share one device table and two pinned copies but lay the table out differently, and only the
library's ordering keeps the weights call of the next world from overwriting the table the update of this world is still reading."""
import time

import numpy as np
import pytest

import session_cases as sc
from affine_cases import checker  # noqa: F401
from buffer_cases import POISON, POISON32, POISON64, Arena, arena_bytes, assert_guards

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def expect(checker, oracle, swamd):  # noqa: F811
    return sc.Expect(checker, oracle, swamd)


def to_dev(t, data):
    """The bytes on the device with 16 zeroed spare bytes behind them."""
    data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    buf = t.zeros(len(data) + 16, dtype=t.uint8, device=DEV)
    buf[:len(data)] = t.from_numpy(data.copy())
    return buf[:len(data)]


def ops_cap(step):
    return max(len(q) for q in step.queries) + int(np.diff(sc.databases()[step.db]["offs"]).max())


class Run:
    """One fresh context and everything its steps need, allocated before the first call."""

    def __init__(self, swamd, torch, steps):
        t = self.t = torch
        self.steps = steps
        self.eng = swamd.Engine(0)
        self.second = t.cuda.Stream()
        self.d_db = {n: to_dev(t, d["packed"]) for n, d in sc.databases().items()}
        self.db = {n: self.eng.prepare_db(self.d_db[n], d["offs"]) for n, d in sc.databases().items()}
        self.d_q = {n: to_dev(t, q["qpacked"]) for n, q in sc.query_sets().items()}
        self.d_pssm = {id(s.ty): to_dev(t, s.ty.matrix).view(t.int8) for s in steps if s.ty is not None}
        a, b = sc.fill_pair()
        self.d_a, self.d_b = self.eng.to_device(a)[0], self.eng.to_device(b)[0]
        full = lambda n, dtype=t.int64, v=POISON64: t.full((n,), v, dtype=dtype, device=DEV)  # noqa: E731
        # the arena of the hit tables and the alignments
        sizes = []
        for s in steps:
            nq = len(s.queries) if s.call != "fill" else 0
            if s.call in sc.SELECTING_CALLS:
                sizes += [nq * s.top * 24, nq * 8]
            elif s.call in ("align_affine_hits", "align_pssm_hits"):
                sizes += [nq * s.top * 56, nq * s.top * ops_cap(s)]
            elif s.call == "align_affine_one":
                sizes += [len(s.hits) * 56, len(s.hits) * ops_cap(s)]
        self.arena = Arena(t, DEV, arena_bytes(*sizes))
        i64 = lambda n, name: self.arena.view(self.arena.carve(n * 8, align=8, name=name), t.int64, (n,))  # noqa: E731
        u8 = lambda n, name: self.arena.view(self.arena.carve(n, name=name), t.uint8, (n,))  # noqa: E731
        self.buf, self.out, self.events = {}, {}, {}
        for s in steps:
            nq = len(s.queries) if s.call != "fill" else 0
            nt = len(sc.databases()[s.db]["targets"]) if s.db else 0
            tag = f"{s.name}-{s.p}"
            if s.call in ("search_affine", "search_pssm"):
                self.buf[s.key] = full(nq * nt * 3)
            elif s.call in ("search_linear", "search_affine_one"):
                self.buf[s.key] = full(nt * 3).view(nt, 3)
            elif s.call in sc.SELECTING_CALLS:
                self.buf[s.key] = (i64(nq * s.top * 3, tag + " hits"), i64(nq, tag + " nhits"))
            elif s.call == "prefilter":
                self.buf[s.key] = (full(s.cap * 2).view(s.cap, 2), full(1), full(nq * nt, t.int32, POISON32).view(nq, nt))
            elif s.call == "search_pairs":
                self.buf[s.key] = full(s.cap * 3)
            elif s.call in ("align_affine_hits", "align_pssm_hits"):
                self.buf[s.key] = (i64(nq * s.top * 7, tag + " aln"), u8(nq * s.top * ops_cap(s), tag + " ops"))
                if s.hits is not None:
                    self.buf[s.key] += (t.from_numpy(s.hits.copy()).to(DEV), t.from_numpy(s.nhits.copy()).to(DEV))
            elif s.call == "align_affine_one":
                n = len(s.hits)
                self.buf[s.key] = (i64(n * 7, tag + " aln").view(n, 7), u8(n * ops_cap(s), tag + " ops").view(n, ops_cap(s)))
            elif s.call == "fill":
                f = self.eng.alloc(len(a), len(b))
                f.H.fill_(POISON32)
                f.P.fill_(POISON32)
                f.res.fill_(POISON64)
                self.buf[s.key] = f
        t.zeros(1, dtype=t.int64, device=DEV)                       # (the one-call search allocates its count: the allocator is warm)
        with t.cuda.stream(self.second):
            t.zeros(1, dtype=t.int64, device=DEV)

    def close(self):
        for db in self.db.values():
            db.close()
        self.eng.close()

    def enqueue(self, s):
        """The step's call on its stream, the routes it reports read from the host's fields, an event behind it.  Nothing waits."""
        t, eng = self.t, self.eng
        if s.stream:
            with t.cuda.stream(self.second):
                self._call(s)
                ev = t.cuda.Event()
                ev.record()
        else:
            self._call(s)
            ev = t.cuda.Event()
            ev.record()
        self.events[s.key] = ev
        if s.call in sc.MULTI_SEARCH_CALLS:
            packed = eng.get_option("last_search_multi_packed_launches")
            assert (packed > 0) if s.packed else (packed == 0), (s.name, packed)
        elif s.call in ("align_affine_hits", "align_pssm_hits"):
            assert eng.get_option("last_align_hits_checkpointed") == s.checkpoint, s.name
        elif s.call == "align_affine_one":
            assert eng.get_option("last_align_affine_checkpointed") == s.checkpoint, s.name

    def _call(self, s):
        eng, buf = self.eng, self.buf.get(s.key)
        eng.set_option("search_lanes", s.lanes)
        eng.set_option("align_checkpoint", s.checkpoint)
        c = s.call
        if c == "fill":
            self.out[s.key] = eng.fill_into(buf, self.d_a, self.d_b)
            return
        db, d = self.db[s.db], sc.databases()[s.db]
        if s.ty is not None:
            d_src, qoffs, scoring = self.d_pssm[id(s.ty)], s.ty.qoffs, s.ty.scoring(*s.gaps)
        else:
            qs = sc.query_sets()[s.q]
            d_src, qoffs, scoring = self.d_q[s.q], qs["qoffs"], (s.sub, *s.gaps)
            if s.one is not None:
                d_one, qlen = d_src[int(qoffs[s.one]):], len(s.queries[0])
        if c == "search_affine":
            self.out[s.key] = db.search_affine_device(d_src, qoffs, scoring, out=buf)
        elif c == "search_pssm":
            self.out[s.key] = db.search_pssm_device(d_src, qoffs, scoring, out=buf)
        elif c == "search_affine_top":
            self.out[s.key] = db.search_affine_top_device(d_src, qoffs, scoring, s.top, s.min_score, out=buf)
        elif c == "search_pssm_top":
            self.out[s.key] = db.search_pssm_top_device(d_src, qoffs, scoring, s.top, s.min_score, out=buf)
        elif c == "prefilter":
            self.out[s.key] = db.prefilter_ungapped_device(d_src, qoffs, s.sub, s.min_score, s.cap, want_scores=True, out=buf)
        elif c == "search_pairs":
            pairs = self.out[(s.source, s.p)][0]
            self.out[s.key] = (pairs, db.search_affine_pairs_device(d_src, qoffs, scoring, pairs, out=buf))
        elif c == "top_pairs":
            pairs, res = self.out[(s.source, s.p)]
            self.out[s.key] = eng.top_hits_pairs_device(pairs, res, s.cap, len(s.queries), len(d["targets"]), s.top, s.min_score, out=buf)
        elif c == "top_prefiltered":
            self.out[s.key] = db.search_affine_top_prefiltered_device(d_src, qoffs, scoring, sc.PREFILTER_MIN, s.cap, s.top, s.min_score, out=buf)
        elif c == "align_affine_hits":
            hits, nhits = self.out[(s.source, s.p)]
            self.out[s.key] = db.align_affine_hits_device(d_src, qoffs, scoring, hits, nhits, ops_cap=ops_cap(s), out=buf[:2])
        elif c == "align_pssm_hits":
            self.out[s.key] = db.align_pssm_hits_device(d_src, qoffs, scoring, buf[2], buf[3], ops_cap=ops_cap(s), out=buf[:2])
        elif c == "search_linear":
            self.out[s.key] = eng.search_device(d_one, qlen, self.d_db[s.db], d["offs"], s.linear, out=buf)
        elif c == "search_affine_one":
            self.out[s.key] = eng.search_affine_device(d_one, qlen, self.d_db[s.db], d["offs"], s.sub, *s.gaps, out=buf)
        elif c == "align_affine_one":
            self.out[s.key] = eng.align_affine_device(d_one, qlen, self.d_db[s.db], d["offs"], s.sub, *s.gaps, s.hits, ops_cap=ops_cap(s), out=buf)
        else:
            raise AssertionError(c)

    def pending(self):
        """The steps whose event has not completed (a query, not a wait)."""
        return [s.name for s in self.steps if s.key in self.events and not self.events[s.key].query()]

    # ---- after the final synchronisation ----

    def check(self, expect):
        """Every step against its expectation; all the steps that differ are reported, not the first alone."""
        wrong = []
        for s in self.steps:
            try:
                self._check(s, expect.of(s), self.out[s.key])
            except AssertionError as err:
                wrong.append(str(err).splitlines()[0])
        assert not wrong, f"{len(wrong)} of {len(self.steps)} steps differ:\n  " + "\n  ".join(wrong)
        assert_guards(self.arena)

    def _check(self, s, e, out):
        what = f"{s.name} (pass {s.p}, stream {s.stream})"
        host = lambda x: x.cpu().numpy()  # noqa: E731
        c = s.call
        if c == "fill":
            assert np.array_equal(host(out.H), e["H"]) and np.array_equal(host(out.P), e["P"]), what
            assert host(out.res).tolist()[:2] == [e["max_pos"], e["max_score"]], what
            return
        empty = np.diff(sc.databases()[s.db]["offs"]) == 0
        if c in ("search_affine", "search_pssm", "search_linear", "search_affine_one"):
            got = host(out)
            bad = np.argwhere((got != e["results"]).any(axis=-1))
            assert len(bad) == 0, f"{what}: {len(bad)} entries differ, first {tuple(bad[0])}: {got[tuple(bad[0])]} vs {e['results'][tuple(bad[0])]}"
            assert empty.any() and not got[..., empty, :].any(), what                  # {0, 0, 0} over the poison
        elif c in sc.SELECTING_CALLS:
            hits, nhits = host(out[0]), host(out[1])
            assert np.array_equal(nhits, e["nhits"]), f"{what}: nhits {nhits.tolist()} vs {e['nhits'].tolist()}"
            bad = np.argwhere((hits != e["hits"]).any(axis=-1))
            assert len(bad) == 0, f"{what}: {len(bad)} hits differ, first {tuple(bad[0])}: {hits[tuple(bad[0])]} vs {e['hits'][tuple(bad[0])]}"
            if c == "top_prefiltered":
                assert int(host(out[2])[0]) == e["npairs"], what
        elif c == "prefilter":
            pairs, n, scores = host(out[0]), int(host(out[1])[0]), host(out[2])
            assert n == e["npairs"], f"{what}: {n} pairs pass, expected {e['npairs']}"
            pr = pairs[:n]
            assert np.array_equal(pr[np.lexsort((pr[:, 1], pr[:, 0]))], e["pairs"]) and (pairs[n:] == -1).all(), what
            assert np.array_equal(scores, e["scores"]) and not scores[:, empty].any(), what
        elif c == "search_pairs":
            pairs, got = host(out[0]), host(out[1])
            want = np.zeros_like(got)
            valid = pairs[:, 0] >= 0
            want[valid] = e["full"][pairs[valid, 0], pairs[valid, 1]]
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert len(bad) == 0, f"{what}: {len(bad)} entries differ, first {bad[0]} {tuple(pairs[bad[0]])}: {got[bad[0]]} vs {want[bad[0]]}"
            assert valid.sum() == len(e["pairs"]) and got[valid, 1].max() > 0, what
        else:                                                                           # the three alignment calls
            aln, ops = host(out[0]), host(out[1])
            bad = np.argwhere((aln != e["aln"]).any(axis=-1))
            assert len(bad) == 0, f"{what}: {len(bad)} alignments differ, first {tuple(bad[0])}: {aln[tuple(bad[0])]} vs {e['aln'][tuple(bad[0])]}"
            flat_aln, flat_ops = aln.reshape(-1, 7), ops.reshape(len(aln.reshape(-1, 7)), -1)
            want_ops = e["ops"] if c == "align_affine_one" else [o for row in e["ops"] for o in row]
            for h, o in enumerate(want_ops):
                n = int(flat_aln[h, 6])
                assert flat_ops[h, :n].tobytes() == o and (flat_ops[h, n:] == POISON).all(), f"{what}: ops of entry {h}"


def run_sessions(runs, order, label):
    """Enqueues `order` -- (run, step) pairs -- with nothing in between, drains once, and says what it saw of the overlap."""
    import torch
    torch.cuda.synchronize()
    first, before, overlapped = None, None, []
    t0 = time.perf_counter()
    for run, s in order:
        run.enqueue(s)
        if before is not None and not before[0].events[before[1].key].query():      # (a query of the event, not a wait)
            overlapped.append(before[1].name)
        before = (run, s)
        if first is None:
            first = run.events[s.key]
    first_pending = not first.query()
    t1 = time.perf_counter()
    pending = [n for run in runs for n in run.pending()]
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print(f"\n[{label}] {len(order)} calls enqueued in {1e3 * (t1 - t0):.1f} ms, drained in {1e3 * (t2 - t1):.1f} ms; the first step's event was "
          f"{'still pending' if first_pending else 'complete'} when the last enqueue returned; pending then: {pending}; "
          f"{len(overlapped)} steps were still running when the enqueue of the next returned: {overlapped}")


@pytest.fixture
def runs(swamd):
    made = []

    def make(steps):
        import torch
        made.append(Run(swamd, torch, steps))
        return made[-1]

    yield make
    for r in made:
        r.close()


def test_growing_session_twice_on_one_fresh_context(runs, expect):
    steps = sc.growing(0) + sc.growing(1)
    run = runs(steps)
    run_sessions([run], [(run, s) for s in steps], "growing, two passes")
    run.check(expect)


def test_shrinking_session_on_two_streams(runs, expect):
    """The largest search first; the second pass finds every workspace at its final size, so nothing is reallocated in it."""
    run = runs(sc.shrinking(0) + sc.shrinking(1))
    assert run.steps[0].name == "top_packed"
    run_sessions([run], [(run, s) for s in sc.shrinking(0)], "shrinking, cold")
    run_sessions([run], [(run, s) for s in sc.shrinking(1)], "shrinking, warm")
    run.check(expect)


def test_iterating_session_updates_back_to_back(swamd, expect, checker):  # noqa: F811
    """session_cases.ITERATING on one fresh context: search_pssm_top and align_pssm_hits, five sw_db_pssm_from_hits in a row on
    alternating streams -- worlds of 4, 24, 256, 4 and 24 letters, so the device table grows twice and the fourth and fifth calls
    rewrite the pinned copies of the second and third --, a search on the fifth matrix, and the packed pair-list and pre-filter
    steps in between.  Every input is uploaded first; nothing is synchronised, copied or read between the calls; the updates are
    compared with the numpy rule, the searches and alignments with the checker's tables (tests/test_session_host.py)."""
    import torch as t

    import pssm_cases
    import pssm_hits_cases as phc
    it = sc.iterating(swamd)
    worlds, pairs = it["worlds"], it["pairs"]
    eng = swamd.Engine(0)
    second = t.cuda.Stream()
    dbs = []
    try:
        i8 = lambda a: t.from_numpy(np.ascontiguousarray(a).reshape(-1).copy()).to(DEV)  # noqa: E731
        w_db = [eng.prepare_db(to_dev(t, c.packed), c.offs) for c in worlds]
        dbs += w_db
        d_prior = [i8(c.prior) for c in worlds]
        c0, c4 = worlds[0], worlds[4]
        nq0, top0, cap0 = len(c0.qoffs) - 1, sc.UPDATE_TOPS[0], c0.cap
        nq4 = len(c4.qoffs) - 1
        sizes = [nq0 * top0 * 24, nq0 * 8, nq0 * top0 * 56, nq0 * top0 * cap0, nq4 * sc.ITER_TOP_AGAIN * 24, nq4 * 8] + [c.prior.size for c in worlds]
        arena = Arena(t, DEV, arena_bytes(*sizes))
        i64 = lambda n, name: arena.view(arena.carve(n * 8, align=8, name=name), t.int64, (n,))  # noqa: E731
        hits0, nhits0, aln0 = i64(nq0 * top0 * 3, "hits"), i64(nq0, "nhits"), i64(nq0 * top0 * 7, "aln")
        ops0 = arena.view(arena.carve(nq0 * top0 * cap0, name="ops"), t.uint8, (nq0 * top0 * cap0,))
        hits4, nhits4 = i64(nq4 * sc.ITER_TOP_AGAIN * 3, "hits again"), i64(nq4, "nhits again")
        d_new = [arena.view(arena.carve(c.prior.size, name=f"matrix {k}"), t.int8, (c.prior.size,)) for k, c in enumerate(worlds)]
        tables = [None] + [(t.from_numpy(c.hits.copy()).to(DEV), t.from_numpy(c.aln.copy()).to(DEV), t.from_numpy(c.ops.copy()).to(DEV)) for c in worlds[1:]]
        # the packed steps
        db200, db40 = (eng.prepare_db(to_dev(t, sc.databases()[n]["packed"]), sc.databases()[n]["offs"]) for n in ("db200", "db40"))
        dbs += [db200, db40]
        seven, forty = sc.query_sets()["seven"], sc.query_sets()["forty"]
        d_seven, d_forty, d_pairs = to_dev(t, seven["qpacked"]), to_dev(t, forty["qpacked"]), t.from_numpy(pairs.copy()).to(DEV)
        res_pairs = t.full((len(pairs) * 3,), POISON64, dtype=t.int64, device=DEV)
        cap = 40 * 40
        pre = (t.full((cap, 2), POISON64, dtype=t.int64, device=DEV), t.full((1,), POISON64, dtype=t.int64, device=DEV),
               t.full((40, 40), POISON32, dtype=t.int32, device=DEV))
        with t.cuda.stream(second):
            t.zeros(1, dtype=t.int64, device=DEV)
        out, said = {}, {}

        def call(name):
            if name == "pssm_top":
                out[name] = w_db[0].search_pssm_top_device(d_prior[0], c0.qoffs, phc.scoring(c0), top0, sc.ITER_MIN_SCORE, out=(hits0, nhits0))
            elif name == "align":
                out[name] = w_db[0].align_pssm_hits_device(d_prior[0], c0.qoffs, phc.scoring(c0), hits0, nhits0, ops_cap=cap0, out=(aln0, ops0), top=top0)
            elif name.startswith("update"):
                k = int(name[6:])
                c = worlds[k]
                h, n, a, o = (hits0, nhits0, aln0, ops0) if k == 0 else (tables[k][0], None, tables[k][1], tables[k][2])
                out[name] = w_db[k].pssm_from_hits_device(d_prior[k], c.qoffs, phc.scoring(c), (c.sub, c.pw, c.inc), h, n, a, o, c.cap, out=d_new[k],
                                                          top=c.hits.shape[1])
                said[name] = eng.get_option("last_pssm_hits_launches")
            elif name == "pssm_top_again":
                out[name] = w_db[4].search_pssm_top_device(d_new[4], c4.qoffs, phc.scoring(c4), sc.ITER_TOP_AGAIN, sc.ITER_MIN_SCORE, out=(hits4, nhits4))
            elif name == "pairs16":
                eng.set_option("search_pairs_lanes", 16)
                try:
                    out[name] = db200.search_affine_pairs_device(d_seven, seven["qoffs"], (sc.packed_table(0), *sc.lc.GAPS[0]), d_pairs, out=res_pairs)
                    said[name] = eng.get_option("last_search_pairs_packed_launches")
                finally:
                    eng.set_option("search_pairs_lanes", 32)
            else:
                assert name == "prefilter16"
                out[name] = db40.prefilter_ungapped_device(d_forty, forty["qoffs"], sc.packed_table(0), sc.ITER_PREFILTER_MIN, cap, want_scores=True, out=pre)
                said[name] = eng.get_option("last_prefilter_packed_launches")

        t.cuda.synchronize()
        t0 = time.perf_counter()
        for name, stream in sc.ITERATING:
            if stream:
                with t.cuda.stream(second):
                    call(name)
            else:
                call(name)
        t1 = time.perf_counter()
        t.cuda.synchronize()
        print(f"\n[iterating] {len(sc.ITERATING)} calls enqueued in {1e3 * (t1 - t0):.1f} ms, drained in {1e3 * (time.perf_counter() - t1):.1f} ms")
        host = lambda x: x.cpu().numpy()  # noqa: E731
        # the routes
        assert said["pairs16"] > 0 and said["prefilter16"] > 0 and all(said[f"update{k}"] == 1 for k in range(5)), said
        # steps 1 and 2
        assert np.array_equal(host(hits0).reshape(nq0, top0, 3), c0.hits) and np.array_equal(host(nhits0), c0.nhits)
        assert np.array_equal(host(aln0).reshape(nq0, top0, 7), c0.aln)
        ops = host(ops0).reshape(nq0 * top0, cap0)
        live = np.arange(cap0)[None, :] < c0.aln.reshape(-1, 7)[:, 6:7]
        assert np.array_equal(ops[live], c0.ops[live]) and (ops[~live] == POISON).all()
        # the five updates against the rule
        wrong = []
        for k, c in enumerate(worlds):
            got, want = host(d_new[k]).reshape(c.prior.shape), sc.update_expected(c)
            front = int(c.qoffs[0])
            if not (got[:front].view(np.uint8) == POISON).all():
                wrong.append(f"update{k}: the unused front columns were written")
            if not np.array_equal(got[front:], want[front:]):
                bad = np.argwhere(got[front:] != want[front:])
                wrong.append(f"update{k}: {len(bad)} entries differ, first (column, letter) {bad[0].tolist()}: {got[front:][tuple(bad[0])]} vs {want[front:][tuple(bad[0])]}")
        assert not wrong, "\n  ".join(wrong)
        # the search on the fifth matrix
        full = sc.iterating_search_again(checker, c4, sc.update_expected(c4))
        want_hits, want_n = pssm_cases.rank_order(full, sc.ITER_TOP_AGAIN, sc.ITER_MIN_SCORE)
        assert np.array_equal(host(hits4).reshape(want_hits.shape), want_hits) and np.array_equal(host(nhits4), want_n)
        # the packed steps
        step = sc.Step("iter_pairs", "search_pairs", 0, db="db200", q="seven", sub=sc.packed_table(0), gaps=sc.lc.GAPS[0])
        table = expect.full_under(step, step.sub, step.gaps)
        want = np.zeros((len(pairs), 3), np.int64)
        want[:140] = table[pairs[:140, 0], pairs[:140, 1]]
        assert np.array_equal(host(res_pairs).reshape(-1, 3), want) and want[:, 1].max() > 0
        u, pr = sc.iterating_prefilter()
        got_pairs, n, scores = host(pre[0]), int(host(pre[1])[0]), host(pre[2])
        assert n == len(pr) and np.array_equal(scores, u.astype(np.int32))
        p = got_pairs[:n]
        assert np.array_equal(p[np.lexsort((p[:, 1], p[:, 0]))], pr) and (got_pairs[n:] == -1).all()
        assert_guards(arena)
    finally:
        for db in dbs:
            db.close()
        eng.close()


def test_weighted_session_weights_and_updates_in_turn(swamd):
    """session_cases.WEIGHTED on one fresh context: search_pssm_top and align_pssm_hits, then for worlds of 4, 24 and 256 letters the
    weights on stream 0 and the update that reads them on stream 1, then a search on the last matrix.  The table the two calls share
    takes the weights layout and the update layout in turn and grows before update0, update1 and update2, the accumulators before
    weights1 and weights2 (tests/test_session_host.py).  Every input is uploaded first; nothing is synchronised, copied or read between
    the calls; every output lies in one guarded arena; expected: the host legs chained (held to the numpy rules in
    tests/test_session_host.py)."""
    import torch as t

    import pssm_hits_cases as phc
    worlds = sc.weighted(swamd)["worlds"]
    steps, (want_hits, want_n), _ = sc.weighted_expected(swamd)
    eng = swamd.Engine(0)
    second = t.cuda.Stream()
    dbs = []
    try:
        i8 = lambda a: t.from_numpy(np.ascontiguousarray(a).reshape(-1).copy()).to(DEV)  # noqa: E731
        w_db = [eng.prepare_db(to_dev(t, c.packed), c.offs) for c in worlds]
        dbs += w_db
        d_prior = [i8(c.prior) for c in worlds]
        c0, c2 = worlds[0], worlds[2]
        nq0, top0, cap0 = len(c0.qoffs) - 1, sc.WEIGHT_TOPS[0], c0.cap
        nq2 = len(c2.qoffs) - 1
        nent = [(len(c.qoffs) - 1) * c.hits.shape[1] for c in worlds]
        sizes = ([nq0 * top0 * 24, nq0 * 8, nq0 * top0 * 56, nq0 * top0 * cap0, nq2 * sc.WEIGHTED_TOP_AGAIN * 24, nq2 * 8] + [c.prior.size for c in worlds]
                 + [4 * n for n in nent])
        arena = Arena(t, DEV, arena_bytes(*sizes))
        i64 = lambda n, name: arena.view(arena.carve(n * 8, align=8, name=name), t.int64, (n,))  # noqa: E731
        hits0, nhits0, aln0 = i64(nq0 * top0 * 3, "hits"), i64(nq0, "nhits"), i64(nq0 * top0 * 7, "aln")
        ops0 = arena.view(arena.carve(nq0 * top0 * cap0, name="ops"), t.uint8, (nq0 * top0 * cap0,))
        hits2, nhits2 = i64(nq2 * sc.WEIGHTED_TOP_AGAIN * 3, "hits again"), i64(nq2, "nhits again")
        d_new = [arena.view(arena.carve(c.prior.size, name=f"matrix {k}"), t.int8, (c.prior.size,)) for k, c in enumerate(worlds)]
        d_w = [arena.view(arena.carve(4 * n, align=4, name=f"weights {k}"), t.int32, (n,)) for k, n in enumerate(nent)]
        tables = [None] + [(t.from_numpy(c.hits.copy()).to(DEV), t.from_numpy(c.aln.copy()).to(DEV), t.from_numpy(c.ops.copy()).to(DEV)) for c in worlds[1:]]
        with t.cuda.stream(second):
            t.zeros(1, dtype=t.int64, device=DEV)
        said = {}

        def call(name):
            if name == "pssm_top":
                w_db[0].search_pssm_top_device(d_prior[0], c0.qoffs, phc.scoring(c0), top0, sc.ITER_MIN_SCORE, out=(hits0, nhits0))
            elif name == "align":
                w_db[0].align_pssm_hits_device(d_prior[0], c0.qoffs, phc.scoring(c0), hits0, nhits0, ops_cap=cap0, out=(aln0, ops0), top=top0)
            elif name == "pssm_top_again":
                w_db[2].search_pssm_top_device(d_new[2], c2.qoffs, phc.scoring(c2), sc.WEIGHTED_TOP_AGAIN, sc.ITER_MIN_SCORE, out=(hits2, nhits2))
            else:
                k = int(name[-1])
                c = worlds[k]
                h, n, a, o = (hits0, nhits0, aln0, ops0) if k == 0 else (tables[k][0], None, tables[k][1], tables[k][2])
                if name.startswith("weights"):
                    w_db[k].pssm_hit_weights_device(c.qoffs, phc.scoring(c), (c.per_hit, c.inc), h, n, a, o, c.cap, out=d_w[k], top=c.hits.shape[1])
                    said[name] = (eng.get_option("last_pssm_weights_launches"), eng.get_option("last_pssm_weights_tiles"))
                else:
                    assert name.startswith("update")
                    w_db[k].pssm_from_hits_device(d_prior[k], c.qoffs, phc.scoring(c), (c.sub, c.pw, c.inc), h, n, a, o, c.cap, weights=d_w[k], out=d_new[k],
                                                  top=c.hits.shape[1])
                    said[name] = eng.get_option("last_pssm_hits_launches")

        t.cuda.synchronize()
        t0 = time.perf_counter()
        for name, stream in sc.WEIGHTED:
            if stream:
                with t.cuda.stream(second):
                    call(name)
            else:
                call(name)
        t1 = time.perf_counter()
        t.cuda.synchronize()
        print(f"\n[weighted] {len(sc.WEIGHTED)} calls enqueued in {1e3 * (t1 - t0):.1f} ms, drained in {1e3 * (time.perf_counter() - t1):.1f} ms")
        host = lambda x: x.cpu().numpy()  # noqa: E731
        # the routes: two launches per weights call, one per update; the 513 columns of the last world at 256 letters take 9 tiles
        assert all(said[f"weights{k}"][0] == 2 and said[f"update{k}"] == 1 for k in range(3)), said
        assert said["weights2"][1] == 9 and said["weights0"][1] >= 1
        # steps 1 and 2
        assert np.array_equal(host(hits0).reshape(nq0, top0, 3), c0.hits) and np.array_equal(host(nhits0), c0.nhits)
        assert np.array_equal(host(aln0).reshape(nq0, top0, 7), c0.aln)
        ops = host(ops0).reshape(nq0 * top0, cap0)
        live = np.arange(cap0)[None, :] < c0.aln.reshape(-1, 7)[:, 6:7]
        assert np.array_equal(ops[live], c0.ops[live]) and (ops[~live] == POISON).all()
        # the weights and the updates against the host legs chained
        wrong = []
        for k, (c, (w, m)) in enumerate(zip(worlds, steps)):
            got_w = host(d_w[k]).reshape(w.shape)
            if not np.array_equal(got_w, w):
                bad = np.argwhere(got_w != w)
                wrong.append(f"weights{k}: {len(bad)} weights differ, first (query, entry) {bad[0].tolist()}: {got_w[tuple(bad[0])]} vs {w[tuple(bad[0])]}")
            got = host(d_new[k]).reshape(c.prior.shape)
            front = int(c.qoffs[0])
            if not (got[:front].view(np.uint8) == POISON).all():
                wrong.append(f"update{k}: the unused front columns were written")
            if not np.array_equal(got[front:], m[front:]):
                bad = np.argwhere(got[front:] != m[front:])
                wrong.append(f"update{k}: {len(bad)} entries differ, first (column, letter) {bad[0].tolist()}: {got[front:][tuple(bad[0])]} vs {m[front:][tuple(bad[0])]}")
        assert not wrong, "\n  ".join(wrong)
        # the search on the last matrix
        assert np.array_equal(host(hits2).reshape(want_hits.shape), want_hits) and np.array_equal(host(nhits2), want_n)
        assert_guards(arena)
    finally:
        for db in dbs:
            db.close()
        eng.close()


def test_two_contexts_interleaved_on_one_device(runs, expect):
    a, b = sc.two_contexts()
    ra, rb = runs(a), runs(b)
    run_sessions([ra, rb], [x for sa, sb in zip(a, b) for x in ((ra, sa), (rb, sb))], "two contexts")
    ra.check(expect)
    rb.check(expect)
