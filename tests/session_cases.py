"""Shared by test_session_host.py and test_session_gpu.py: SESSIONS -- ordered lists of calls of every search and alignment family that
one context runs back to back, with nothing but the library's own ordering between them -- as plain data, and the expectation of every
step from the suite's independent references (tests/affine_oracle.cpp through affine_cases.Checker, pssm_cases.Typed, ungapped_cases,
pairs_top_cases, align_cases.replay, oracle/liboracle.so).  Nothing here runs GPU code; everything is computed once per process and
read-only afterwards.

A step names its call, its database, its query set (or its matrices), a scoring of its own, the stream (0 or 1) and the options to set
just before it.  Every table call brings a table no other step of its pass uses and the second pass brings a second set, so a step
that scored with what an earlier call left in a shared buffer gives a different table: test_session_host.py asserts that on the
references alone.

ITERATING, at the end of this file, is a fourth session of steps of other kinds -- sw_db_pssm_from_hits five times in a row, and the
packed routes of the pair list and the pre-filter -- as data of its own; the three sessions above keep their step lists."""
import functools

import numpy as np

import affine_range_cases as arc
import lanes_cases as lc
import pairs_top_cases as ptc
import pssm_cases
from affine_cases import GAPS, PROTEIN, random_submat
from ungapped_cases import passing, ungapped_score, ungapped_table

FRONT, QFRONT = 3, 4                               # offsets[0] of every database, qoffsets[0] of every query set
OTHER, SMAX = -3, 9                                # of every PSSM scoring: entries are drawn from -8 .. 12, so the clamp is at work
PSSM_QLENS = [1, 63, 256, 257, 513, 1025, 1300]    # seven matrices: all three column classes, a second strip at 16 columns per lane
DNA = np.frombuffer(b"ACGT", np.uint8)
PASSES = 2

TABLE_CALLS = ("search_affine", "search_affine_top", "prefilter", "search_pairs", "align_affine_hits", "search_affine_one", "align_affine_one",
               "top_prefiltered")
PSSM_CALLS = ("search_pssm", "search_pssm_top", "align_pssm_hits")
MULTI_SEARCH_CALLS = ("search_affine", "search_pssm", "search_affine_top", "search_pssm_top")   # they report "last_search_multi_packed_launches"
SELECTING_CALLS = ("search_affine_top", "search_pssm_top", "top_pairs", "top_prefiltered")


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def databases():
    """{"db3", "db40", "db200"} over PROTEIN, each {"targets", "packed", "offs"} with empty targets in between and offsets[0] = FRONT."""
    rng = np.random.default_rng(5101)
    l40 = [0, 300, 90, 0, 90] + [int(x) for x in rng.integers(0, 121, 35)]
    l40[20] = l40[39] = 0
    l200 = [int(x) for x in rng.integers(0, 301, 200)]
    for k in (0, 5, 99, 100, 199):
        l200[k] = 0
    l200[77] = 1100
    out = {}
    for name, lens in (("db3", [5, 0, 5]), ("db40", l40), ("db200", l200)):
        targets = [rng.choice(PROTEIN, n).astype(np.uint8) for n in lens]
        packed, offs = arc.packed_of(targets, FRONT, np.resize(PROTEIN, FRONT))
        _frozen(packed, offs, *targets)
        out[name] = {"targets": targets, "packed": packed, "offs": offs}
    assert [len(d["targets"]) for d in out.values()] == [3, 40, 200] and max(l40) == 300 and 0 in l40[5:]
    return out


@functools.lru_cache(maxsize=None)
def query_sets():
    """{"two": 63 and 300 letters, "seven": lanes_cases.QLENS, "forty": 1 .. 200 letters}, each {"queries", "qpacked", "qoffs"}.
    Protein letters with the byte 0 at about every sixteenth place and at least once in every query of more than one letter: a
    profile reads row x of the 256 x 256 table for a query letter x, and row 0 is the 256 bytes in which a PSSM call leaves
    its code table -- only a query that holds the byte 0 can tell whether a table call brought its own row 0."""
    rng = np.random.default_rng(5102)
    forty = [1, 200] + [int(x) for x in rng.integers(1, 201, 38)]
    out = {}
    for name, lens in (("two", [63, 300]), ("seven", lc.QLENS), ("forty", forty)):
        queries = [rng.choice(PROTEIN, n).astype(np.uint8) for n in lens]
        for q in queries:
            if len(q) > 1:
                q[rng.random(len(q)) < 1 / 16] = 0
                q[rng.integers(len(q))] = 0
        qpacked, qoffs = arc.packed_of(queries, QFRONT, np.resize(PROTEIN, QFRONT))
        _frozen(qpacked, qoffs, *queries)
        out[name] = {"queries": queries, "qpacked": qpacked, "qoffs": qoffs}
    return out


@functools.lru_cache(maxsize=None)
def table(p, k):
    """Table k of pass p: affine_cases.random_submat, no two alike."""
    s = random_submat(np.random.default_rng(5200 + 100 * p + k))
    _frozen(s)
    return s


@functools.lru_cache(maxsize=None)
def packed_table(p):
    """The table of the packed steps: lanes_cases.table24() in the first pass, its transpose (it is asymmetric) in the second."""
    s = lc.table24() if p == 0 else np.ascontiguousarray(lc.table24().T)
    _frozen(s)
    return s


@functools.lru_cache(maxsize=None)
def typed(p, k):
    """pssm_cases.Typed k of pass p: PSSM_QLENS columns over the 24 protein letters in an order of its own, so that no two PSSM steps
    share a code table."""
    rng = np.random.default_rng(5300 + 100 * p + k)
    return pssm_cases.Typed(rng, rng.permutation(PROTEIN), OTHER, SMAX, PSSM_QLENS, front=QFRONT)


def code_row(ty):
    """The 256-byte code table a PSSM call of `ty` uploads into the place of the table's row 0, read as that row: code[x] is the place
    of target byte x among the letters, 255 (-1 as a score) for a byte that is not among them (include/swhip.h names the letters'
    order as the order of a column's entries; smith-waterman_amd/csrc/sw_pssm.hip reads the codes)."""
    code = np.full(256, 255, np.uint8)
    code[ty.letters] = np.arange(len(ty.letters), dtype=np.uint8)
    return code.view(np.int8)


@functools.lru_cache(maxsize=None)
def linear_table(match, mismatch):
    """The 256 x 256 table of a linear search's match and mismatch scores (with gap_open = 0 the affine recurrence is the linear one)."""
    s = np.where(np.eye(256, dtype=bool), match, mismatch).astype(np.int8)
    _frozen(s)
    return s


# the workspaces of a context a call stages through, beside the scoring table's two copies (smith-waterman_amd/csrc/sw_api_search.hip)
WORKSPACES = {
    "search_affine": ("query table", "profiles"), "search_pssm": ("query table", "profiles"),
    "search_affine_top": ("query table", "profiles", "selection"), "search_pssm_top": ("query table", "profiles", "selection"),
    "prefilter": ("query table", "profiles", "prefilter control"), "search_pairs": ("query table", "profiles", "pair items"),
    "top_pairs": ("pair selection",), "align_affine_hits": ("query table", "profiles", "directions", "hit items"),
    "align_pssm_hits": ("query table", "profiles", "directions", "hit items"), "search_linear": ("schedule", "profiles"),
    "search_affine_one": ("schedule", "profiles"), "align_affine_one": ("schedule", "profiles", "directions"),
    "top_prefiltered": ("query table", "profiles", "prefilter control", "pair items", "pair selection", "pair list"), "fill": ("fill",),
}


@functools.lru_cache(maxsize=None)
def fill_pair():
    """(a of 300 letters, b of 200) for the one fill."""
    rng = np.random.default_rng(5103)
    a, b = rng.choice(DNA, 300).astype(np.uint8), rng.choice(DNA, 200).astype(np.uint8)
    _frozen(a, b)
    return a, b


class Step:
    """One call of a session.  key: (name, pass) -- what the expectation is cached under, so that the sessions share it."""

    def __init__(self, name, call, p, db=None, q=None, one=None, sub=None, ty=None, gaps=(0, 0), linear=None, stream=0, lanes=32, checkpoint=0,
                 top=0, min_score=0, cap=0, source=None, hits=None, nhits=None, packed=False):
        self.name, self.call, self.p, self.key = name, call, p, (name, p)
        self.db, self.q, self.one = db, q, one              # one: the index of the one query of a one-query call inside its set
        self.sub, self.ty, self.gaps, self.linear = sub, ty, gaps, linear
        self.stream, self.lanes, self.checkpoint = stream, lanes, checkpoint
        self.top, self.min_score, self.cap, self.source = top, min_score, cap, source
        self.hits, self.nhits, self.packed = hits, nhits, packed

    def on(self, stream):
        s = Step.__new__(Step)
        s.__dict__.update(self.__dict__)
        s.stream = stream
        return s

    @property
    def kind(self):
        return "table" if self.call in TABLE_CALLS else "pssm" if self.call in PSSM_CALLS else None

    @property
    def queries(self):
        """The step's queries as the checker takes them: letters, or one type byte per column."""
        if self.ty is not None:
            return [self.ty.query(k) for k in range(len(PSSM_QLENS))]
        qs = query_sets()[self.q]["queries"]
        return qs if self.one is None else [qs[self.one]]

    @property
    def checker_table(self):
        """The 256 x 256 table the checker scores the step's queries with (None: the step uploads no scoring)."""
        if self.linear is not None:
            return linear_table(*self.linear[:2])
        return self.ty.table if self.ty is not None else self.sub

    @property
    def checker_gaps(self):
        return (0, self.linear[2]) if self.linear is not None else self.gaps

    def measures(self):
        """(queries, longest query, targets, hit or pair entries, cells of the largest direction matrix) of the call: what its
        workspaces follow."""
        if self.call == "fill":
            return (0, 0, 0, 0, 0)
        nq = len(self.queries)
        entries = {"search_affine_top": nq * self.top, "search_pssm_top": nq * self.top, "prefilter": self.cap, "search_pairs": self.cap,
                   "top_pairs": self.cap, "align_affine_hits": nq * self.top, "align_pssm_hits": nq * self.top, "top_prefiltered": self.cap,
                   "align_affine_one": 0 if self.hits is None else len(self.hits)}.get(self.call, 0)
        qmax, tmax = max(len(x) for x in self.queries), int(np.diff(databases()[self.db]["offs"]).max())
        return (nq, qmax, len(databases()[self.db]["targets"]), entries, qmax * tmax if self.call.startswith("align") else 0)


PREFILTER_MIN = 150        # of both filtering steps: test_session_host.py asserts that a strict, non-empty subset of the pairs passes


@functools.lru_cache(maxsize=None)
def growing(p):
    """The growing session of pass p.  Every step raises one of measures() over every step before it or is the first to use one of
    WORKSPACES, but for REUSING: the one-query calls behind the first, which run on workspaces larger calls have grown, and the small
    first call again at the end."""
    rng = np.random.default_rng(5400 + p)
    nt40, nt200 = 40, 200
    hand = rng.integers(0, nt200, (len(PSSM_QLENS), 3)).astype(np.int64)               # the hand-built table of the checkpointed PSSM alignment
    hand[0, 0], hand[2, 1], hand[3, 2], hand[6, 0] = 77, nt200 + 2, -1, 77             # the longest target twice, two entries outside
    hand = np.stack([hand, rng.integers(0, 99, hand.shape), rng.integers(0, 99, hand.shape)], axis=-1).astype(np.int64)
    hand_n = np.array([3, 3, 2, 3, 0, 5, 1], np.int64)                                  # whole rows, a short one, none, above top (clamped)
    hits60 = np.concatenate([[0, 1, 3, 1], rng.integers(0, nt40, 56)]).astype(np.int64)  # empty targets and duplicates among them
    hits30 = np.concatenate([[77, 0, 77], rng.integers(0, nt200, 27)]).astype(np.int64)
    _frozen(hand, hand_n, hits60, hits30)
    cap = 40 * nt40
    return (
        Step("small", "search_affine", p, db="db3", q="two", sub=table(p, 0), gaps=GAPS[0]),
        Step("pssm40", "search_pssm", p, db="db40", ty=typed(p, 0), gaps=GAPS[1]),
        Step("table_after_pssm", "search_affine", p, db="db40", q="seven", sub=table(p, 1), gaps=GAPS[2]),
        Step("top_packed", "search_affine_top", p, db="db200", q="seven", sub=packed_table(p), gaps=lc.GAPS[0], lanes=16, packed=True, top=5, min_score=1),
        Step("pssm_top", "search_pssm_top", p, db="db200", ty=typed(p, 1), gaps=GAPS[3], top=12, min_score=30),
        Step("prefilter", "prefilter", p, db="db40", q="forty", sub=table(p, 2), min_score=PREFILTER_MIN, cap=cap),
        Step("pairs", "search_pairs", p, db="db40", q="forty", sub=table(p, 3), gaps=GAPS[0], cap=cap, source="prefilter"),
        Step("top_pairs", "top_pairs", p, db="db40", q="forty", top=4, min_score=1, cap=cap, source="pairs"),
        Step("align_hits", "align_affine_hits", p, db="db40", q="forty", sub=table(p, 4), gaps=GAPS[1], top=4, source="top_pairs", stream=1),
        Step("align_pssm_ckpt", "align_pssm_hits", p, db="db200", ty=typed(p, 2), gaps=GAPS[0], top=3, hits=hand, nhits=hand_n, checkpoint=1),
        Step("linear_one", "search_linear", p, db="db200", q="seven", one=6, linear=((5, -3, -4), (3, -3, -2))[p]),
        Step("affine_one", "search_affine_one", p, db="db200", q="seven", one=5, sub=table(p, 5), gaps=GAPS[3]),
        Step("align_one", "align_affine_one", p, db="db40", q="two", one=1, sub=table(p, 6), gaps=GAPS[1], hits=hits60),
        Step("align_one_ckpt", "align_affine_one", p, db="db200", q="seven", one=4, sub=table(p, 7), gaps=GAPS[0], hits=hits30, checkpoint=1),
        Step("top_prefiltered", "top_prefiltered", p, db="db40", q="forty", sub=table(p, 8), gaps=GAPS[2], min_score=1, top=6, cap=cap),
        Step("fill", "fill", p),
        Step("small_again", "search_affine", p, db="db3", q="two", sub=table(p, 9), gaps=GAPS[4]),
    )


REUSING = ("affine_one", "align_one", "align_one_ckpt", "small_again")
CHAIN = ("prefilter", "pairs", "top_pairs", "align_hits")     # producer and consumers: they keep their order in every session


def _cells(step):
    if step.call == "fill":
        return 300 * 200
    return sum(len(x) for x in step.queries) * int(np.diff(databases()[step.db]["offs"]).sum())


@functools.lru_cache(maxsize=None)
def shrinking(p):
    """The same steps, the largest (query letters x database letters) first, the chain of the pair list as one unit; the steps
    alternate between the two streams."""
    steps = growing(p)
    units = [[s] for s in steps if s.name not in CHAIN] + [[s for s in steps if s.name in CHAIN]]
    units.sort(key=lambda u: -max(_cells(s) for s in u))
    flat = [s for u in units for s in u]
    assert flat[0].name == "top_packed"                         # the largest search comes first
    return tuple(s.on(i % 2) for i, s in enumerate(flat))


@functools.lru_cache(maxsize=None)
def two_contexts():
    """(steps of context A, all on stream 0; steps of context B, all on stream 1): the growing session of the first set of tables
    beside the shrinking one of the second; the test interleaves them one by one."""
    return tuple(s.on(0) for s in growing(0)), tuple(s.on(1) for s in shrinking(1))


# ---- expectations ----

class Expect:
    """The expectation of every step from the independent references, cached by the step's key.  checker: affine_cases.Checker;
    oracle: oracle_lib.Oracle; swamd: the package, for the host legs of the alignments (checked by align_cases.replay and against the
    checker's scores in test_session_host.py)."""

    def __init__(self, checker, oracle, swamd):
        self.checker, self.oracle, self.swamd = checker, oracle, swamd
        self._full, self._u, self._of = {}, {}, {}

    def full_under(self, step, tab, gaps):
        """(nqueries, ntargets, 3): the step's queries against its database under the checker's table `tab` and `gaps`."""
        d = databases()[step.db]
        return np.stack([self.checker.search(q, d["packed"], d["offs"], tab, *gaps) for q in step.queries])

    def full(self, step):
        if step.key not in self._full:
            t = self.full_under(step, step.checker_table, step.checker_gaps)
            _frozen(t)
            self._full[step.key] = t
        return self._full[step.key]

    def ungapped(self, step):
        """The (nqueries, ntargets) table of U of a filtering step and the sorted pairs that pass."""
        if step.key not in self._u:
            d, qs = databases()[step.db], query_sets()[step.q]
            u = ungapped_table(qs["qpacked"], qs["qoffs"], d["packed"], d["offs"], step.sub)
            thr = PREFILTER_MIN if step.call == "top_prefiltered" else step.min_score
            pr = passing(u, d["offs"], thr)
            _frozen(u, pr)
            self._u[step.key] = (u, pr)
        return self._u[step.key]

    def of(self, step, names=None):
        """The step's expectation, a dict by call; a step with a `source` finds it among the steps of its own pass."""
        if step.key in self._of:
            return self._of[step.key]
        by_name = names or {s.name: s for s in growing(step.p)}
        d = databases()[step.db] if step.db else None
        nt = len(d["targets"]) if d else 0
        c = step.call
        if c in ("search_affine", "search_pssm"):
            e = {"results": self.full(step)}
        elif c in ("search_linear", "search_affine_one"):
            e = {"results": self.full(step)[0]}
        elif c in ("search_affine_top", "search_pssm_top"):
            hits, nhits = pssm_cases.rank_order(self.full(step), step.top, step.min_score)
            e = {"hits": hits, "nhits": nhits}
        elif c == "prefilter":
            u, pr = self.ungapped(step)
            e = {"pairs": pr, "npairs": len(pr), "scores": u.astype(np.int32)}
        elif c == "search_pairs":
            e = {"full": self.full(step), "pairs": self.of(by_name[step.source], by_name)["pairs"]}
            e["results"] = e["full"][e["pairs"][:, 0], e["pairs"][:, 1]]                  # in the order of the sorted list
        elif c == "top_pairs":
            src = self.of(by_name[step.source], by_name)
            hits, nhits = ptc.numpy_top_pairs(src["pairs"], src["results"], len(step.queries), nt, step.top, step.min_score)
            e = {"hits": hits, "nhits": nhits}
        elif c == "top_prefiltered":
            _, pr = self.ungapped(step)
            hits, nhits = ptc.numpy_top_pairs(pr, self.full(step)[pr[:, 0], pr[:, 1]], len(step.queries), nt, step.top, step.min_score)
            e = {"hits": hits, "nhits": nhits, "npairs": len(pr)}
        elif c == "align_affine_hits":
            src = self.of(by_name[step.source], by_name)
            qs = query_sets()[step.q]
            aln, ops = self.swamd.align_affine_hits_host((qs["qpacked"], qs["qoffs"]), (d["packed"], d["offs"]), (step.sub, *step.gaps), src["hits"], src["nhits"])
            e = {"aln": aln, "ops": ops, "table": src["hits"], "counts": src["nhits"]}
        elif c == "align_pssm_hits":
            ty = step.ty
            aln, ops = self.swamd.align_pssm_hits_host((ty.matrix, ty.qoffs), (d["packed"], d["offs"]), ty.scoring(*step.gaps), step.hits, step.nhits)
            e = {"aln": aln, "ops": ops, "table": step.hits, "counts": step.nhits}
        elif c == "align_affine_one":
            aln, ops = self.swamd.align_affine_host(step.queries[0], (d["packed"], d["offs"]), step.sub, *step.gaps, step.hits)
            e = {"aln": aln, "ops": ops}
        elif c == "fill":
            a, b = fill_pair()
            H, P, mp = self.oracle.fill(a, b)
            e = {"H": H, "P": P, "max_pos": mp, "max_score": int(H.flat[mp])}
        else:
            raise ValueError(c)
        for v in e.values():
            if isinstance(v, np.ndarray):
                _frozen(v)
        self._of[step.key] = e
        return e


def by_name(steps):
    return {s.name: s for s in steps}


def differs_per_query(own, other, offs, only=None):
    """Every query with a non-empty target (`only`: of those queries) has an entry in which the two (nqueries, ntargets, 3) tables differ."""
    nonempty = np.diff(offs) > 0
    rows = ((own != other).any(axis=2) & nonempty[None, :]).any(axis=1)
    return bool(rows.all() if only is None else rows[np.asarray(only)].all())


def ungapped_differs(step, prev_table, u, only=None):
    """For every query (`only`: of those) some non-empty target whose U under `prev_table` is not the step's own (the whole table is not
    recomputed)."""
    d, qs = databases()[step.db], query_sets()[step.q]
    for a, q in enumerate(qs["queries"]):
        if only is not None and a not in only:
            continue
        if not any(len(t) and ungapped_score(q, t, prev_table) != u[a, b] for b, t in enumerate(d["targets"])):
            return False
    return True


# ---- the fourth session: updates back to back ----
#
# sw_db_pssm_from_hits stages S, the code table and the offsets through two pinned copies used in turn and one device table that grows,
# so update N + 2 rewrites the copy of update N.  ITERATING is the order of the calls of one fresh context; the five updates stand in a
# row on alternating streams, their worlds hold 4, 24, 256, 4 and 24 letters (the device table grows before the second and before the
# third), and every one has an S, an order of the letters, offsets, a number of queries, a top and a prior weight of its own.

UPDATE_NLETTERS = [4, 24, 256, 4, 24]
UPDATE_QLENS = [[30, 90, 50, 60, 33, 47], [63, 64, 65, 129, 257], [1, 300, 513, 64], [257, 65, 600], [200, 256]]
UPDATE_TOPS = [5, 7, 9, 12, 20]
UPDATE_PW = [2, 1, 3, 0, 5]
ITERATING = (("pssm_top", 0), ("pairs16", 1), ("align", 0), ("prefilter16", 1), ("update0", 0), ("update1", 1), ("update2", 0), ("update3", 1),
             ("update4", 0), ("pssm_top_again", 1))                          # (step, stream)
ITER_MIN_SCORE, ITER_TOP_AGAIN = 1, 3

_iterating = {}


def iterating(swamd):
    """The data of the session: {"worlds": the five cases of tests/pssm_hits_cases.py (worlds[0] holds the host legs' iteration 0 over a
    four-letter database with planted homologues -- test_session_host.py checks those tables against the checker --, the others
    synthetic tables), "pairs": the pair list of the packed pair step over db200 / "seven" / lanes_cases.table24(), "prefilter_min"}."""
    if not _iterating:
        import pssm_hits_cases as phc
        worlds = []
        for k, (nl, qlens, top) in enumerate(zip(UPDATE_NLETTERS, UPDATE_QLENS, UPDATE_TOPS)):
            rng = np.random.default_rng(5600 + k)
            if k == 0:
                alpha = PROTEIN[:4]
                sub = np.full((256, 256), -4, np.int8)
                sub[np.ix_(alpha, alpha)] = rng.integers(-4, 0, (4, 4))
                sub[alpha, alpha] = rng.integers(5, 10, 4)
                sub = np.minimum(sub, sub.T)
                c = phc.real(swamd, rng, top, qlens=qlens, nrandom=30, nletters=4, alpha=alpha, sub=sub)
                order = np.arange(4)                               # (the prior's columns follow the letters: the order stays)
            else:
                c = phc.synthetic(rng, nl, top, qlens=qlens)
                order = rng.permutation(nl)
            c.letters = c.letters[order]
            c.pw, c.inc = UPDATE_PW[k], 0
            worlds.append(c)
        rng = np.random.default_rng(5650)
        pairs = np.stack([rng.integers(0, len(lc.QLENS), 150), rng.integers(0, 200, 150)], axis=1).astype(np.int64)
        pairs[140:] = -1
        pairs[100:110] = pairs[:10]
        _frozen(pairs)
        _iterating.update(worlds=worlds, pairs=pairs)
    return _iterating


def code_of(letters):
    """The place of every byte among the letters, -1 for a byte that is not among them."""
    code = np.full(256, -1, np.int64)
    code[letters] = np.arange(len(letters))
    return code


def update_expected(c, sub=None, code=None, qoffs=None):
    """The matrix the rule gives for update world c (tests/pssm_hits_cases.reference), or what it would give had the call taken another
    call's S, code table or offsets."""
    import types

    import pssm_hits_cases as phc
    v = types.SimpleNamespace(**vars(c))
    if sub is not None:
        v.sub = sub
    if qoffs is not None:
        v.qoffs = np.ascontiguousarray(qoffs[:len(c.qoffs)], np.int64)
    return phc.reference(v, c.pw, c.inc, code=code)[0]


def typed_of_matrix(m, letters, other, smax):
    """A query of at most 256 columns as the checker takes it: every column a type of its own.  (type string, (256, 256) table)."""
    assert len(m) <= 256
    tab = np.full((256, 256), other, np.int8)
    tab[:len(m), letters] = np.minimum(m, smax)
    return np.arange(len(m), dtype=np.uint8), tab


def iterating_search_again(checker, c, m):
    """The checker's (nqueries, ntargets, 3) table of matrix m over the queries of world c (each of at most 256 columns)."""
    import pssm_hits_cases as phc
    _, other, smax, go, ge = phc.scoring(c)
    out = []
    for q in range(len(c.qoffs) - 1):
        names, tab = typed_of_matrix(m[c.qoffs[q]:c.qoffs[q + 1]], c.letters, other, smax)
        out.append(checker.search(names, c.packed, c.offs, tab, go, ge))
    return np.stack(out)


ITER_PREFILTER_MIN = 40


@functools.lru_cache(maxsize=None)
def iterating_prefilter():
    """(U (40, 40), the sorted pairs that pass) of the packed pre-filter step: "forty" against db40 under lanes_cases.table24()."""
    d, qs = databases()["db40"], query_sets()["forty"]
    u = ungapped_table(qs["qpacked"], qs["qoffs"], d["packed"], d["offs"], packed_table(0))
    pr = passing(u, d["offs"], ITER_PREFILTER_MIN)
    _frozen(u, pr)
    return u, pr


def sequence_table(sub, letters, other, smax):
    """The checker's table of a PSSM that sw_pssm_from_queries made of sequence queries under `sub`."""
    tab = np.full((256, 256), other, np.int8)
    tab[:, letters] = np.minimum(sub[:, letters], smax)
    return tab


# ---- the fifth session: weights and updates in turn ----
#
# sw_db_pssm_hit_weights stages its code table and offsets through the device table and the two pinned copies of sw_db_pssm_from_hits,
# in the same turns, but lays the table out differently: its code table stands at byte 0, where the update keeps S.  It owns a second
# workspace, one 64-bit accumulator per entry, which grows with nqueries x top.  WEIGHTED is the order of the calls of one fresh
# context: weightsK on stream 0, updateK -- which takes weightsK's device output as d_weights -- on stream 1, nothing synchronised.  The
# worlds hold 4, 24 and 256 letters and 6, 7 and 8 queries, so the table's need alternates between the two layouts and grows before
# update0 (weights0 allocated it), update1 and update2; the accumulators grow before weights1 and weights2 (asserted in
# test_session_host.py from the sizes the driver computes).

WEIGHT_NLETTERS = [4, 24, 256]
WEIGHT_QLENS = [[30, 90, 50, 60, 33, 47], [40, 63, 33, 64, 30, 65, 257], [1, 63, 64, 65, 129, 100, 30, 513]]   # (the first queries of a world fit the world before)
WEIGHT_TOPS = [5, 7, 9]
WEIGHT_PER_HIT = [16, 7, 100]
WEIGHT_PW = [32, 1, 3]
WEIGHT_INC = [1, 0, 20]
WEIGHTED = (("pssm_top", 0), ("align", 1), ("weights0", 0), ("update0", 1), ("weights1", 0), ("update1", 1), ("weights2", 0), ("update2", 1),
            ("pssm_top_again", 0))                                           # (step, stream)
WEIGHTED_TOP_AGAIN = 3

_weighted = {}


def weighted(swamd):
    """The worlds of the session (cases of tests/pssm_hits_cases.py): worlds[0] holds the host legs' iteration 0 over a four-letter
    database with planted homologues, the others synthetic tables; each with per_hit, pw and inc of its own and the letters in an order
    of its own."""
    if not _weighted:
        import pssm_hits_cases as phc
        worlds = []
        for k, (nl, qlens, top) in enumerate(zip(WEIGHT_NLETTERS, WEIGHT_QLENS, WEIGHT_TOPS)):
            rng = np.random.default_rng(5700 + k)
            if k == 0:
                alpha = PROTEIN[:4]
                sub = np.full((256, 256), -4, np.int8)
                sub[np.ix_(alpha, alpha)] = rng.integers(-4, 0, (4, 4))
                sub[alpha, alpha] = rng.integers(5, 10, 4)
                sub = np.minimum(sub, sub.T)
                c = phc.real(swamd, rng, top, qlens=qlens, nrandom=30, nletters=4, alpha=alpha, sub=sub)
                order = np.arange(4)                               # (the prior's columns follow the letters: the order stays)
            else:
                c = phc.synthetic(rng, nl, top, qlens=qlens)
                order = rng.permutation(nl)
            c.letters = c.letters[order]
            c.per_hit, c.pw, c.inc = WEIGHT_PER_HIT[k], WEIGHT_PW[k], WEIGHT_INC[k]
            worlds.append(c)
        _weighted.update(worlds=worlds)
    return _weighted


def weighted_expected(swamd):
    """The host legs chained: per world (weights, new matrix in the layout of the prior), then the hit table of the search on the last
    matrix.  Computed once."""
    if "expected" not in _weighted:
        import pssm_hits_cases as phc
        import pssm_weights_cases as pwc
        steps = []
        for c in weighted(swamd)["worlds"]:
            w = pwc.host_leg(swamd, c, c.per_hit, c.inc)
            out, _ = phc.host_leg(swamd, c, c.pw, c.inc, w)
            m = c.prior.copy()
            m[int(c.qoffs[0]):] = out
            _frozen(w, m)
            steps.append((w, m))
        c = weighted(swamd)["worlds"][-1]
        full = swamd.search_pssm_multi_host((steps[-1][1], c.qoffs), (c.packed, c.offs), phc.scoring(c))
        _weighted["expected"] = (steps, pssm_cases.rank_order(full, WEIGHTED_TOP_AGAIN, ITER_MIN_SCORE), full)
    return _weighted["expected"]


def table_needs(c):
    """(bytes of the weights call's table, bytes of the update's, accumulators of the weights call) as the driver sizes them
    (smith-waterman_amd/csrc/sw_api_search.hip): 256 + offsets; S padded to 256 bytes + 256 + offsets; nqueries x top."""
    n, nq = len(c.letters), len(c.qoffs) - 1
    off = 8 * (nq + 1)
    return 256 + off, ((n * n + 255) & ~255) + 256 + off, nq * c.hits.shape[1]


def weights_under(c, code=None, qoffs=None, acc=None):
    """The weights the rule gives for world c (tests/pssm_weights_cases.py), or what it would give had the call taken another call's code
    table or offsets, or had it added to another call's accumulators (acc: that call's (T, m), taken entry by entry in table order)
    where it should have started from zero."""
    import types

    import pssm_weights_cases as pwc
    v = types.SimpleNamespace(**vars(c))
    if qoffs is not None:
        v.qoffs = np.ascontiguousarray(qoffs[:len(c.qoffs)], np.int64)
    T, m, _ = pwc.accumulators(v, c.inc, code)
    if acc is not None:
        for mine, theirs in zip((T, m), acc):
            flat, old = mine.reshape(-1), theirs.reshape(-1)
            n = min(len(flat), len(old))
            flat[:n] = flat[:n] + old[:n]
    try:
        return pwc.weights_of(T, m, c.per_hit)[0]
    except AssertionError:
        return None                                                # (outside the rule's ranges: no table a correct call could give)
