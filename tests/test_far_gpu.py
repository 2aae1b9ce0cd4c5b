"""GPU: every database-search call with its buffers and offsets beyond 4 GiB (tests/far_cases.py has the range, the small world and
its decoy).  Only placement changes: the sequences are tiny, a test's time is allocation and memset.  Every comparison is exact,
every output is poisoned first, and every routing claim is asserted from the "last_*" options.  Expected values come from the
checker (tests/affine_oracle.cpp), the rule's walk (tests/align_cases.py) and the numpy reference of the ungapped score alone; the same
call at near placement is an extra bytewise comparison.  A kernel that drops the high half of an offset reads or writes the decoy 2^32
bytes below and shows as wrong values, not as a fault.

The PSSM update and the hit weights (sw_db_pssm_from_hits, sw_db_pssm_hit_weights) are two families of their own: far databases, far
PSSM columns (prior and matrix), ops rows beyond byte 2^32 and a count matrix of 5.4 GB; their expected values are the numpy rules of
tests/pssm_hits_cases.py and tests/pssm_weights_cases.py over the small world (tests/far_cases.py: hits_case, count_case).

Every test frees its tensors and empties torch's cache before the next one starts; none holds more than about 12 GiB."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import far_cases as fc
from affine_cases import checker  # noqa: F401

pytestmark = pytest.mark.gpu

POISON64, POISON32, POISON8 = -0x5A5A5A5A5A5A5A5B, -0x5A5A5A5B, 0xA5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS_CAP = fc.OPS_CAP
NHITS_CUT = fc.NHITS_CUT                          # the counts of the alignment calls: unused entries in the table, one empty row


@pytest.fixture(autouse=True)
def room(engine):
    t = engine.torch
    t.cuda.empty_cache()
    free, total = t.cuda.mem_get_info()
    if free < 16 * 2**30:
        pytest.skip(f"{free} of {total} bytes of device memory are free, 16 GiB are needed")
    rows = engine.get_option("align_checkpoint_rows")
    engine.set_option("align_checkpoint_rows", 64)
    yield
    engine.set_option("align_checkpoint_rows", rows)
    engine.synchronize()
    t.cuda.empty_cache()


def dev_of(engine):
    return f"cuda:{engine.device}"


def on_device(engine, desc, dtype=None):
    """A description of tests/far_cases.py on torch.empty: only the pieces are written."""
    t = engine.torch
    buf = t.empty(desc["size"], dtype=t.uint8, device=dev_of(engine))
    for at, b in desc["pieces"]:
        buf[at:at + len(b)] = t.from_numpy(np.array(b)).to(dev_of(engine))
    return buf.view(dtype) if dtype is not None else buf


def upload(engine, a):
    return engine.torch.from_numpy(np.ascontiguousarray(a).copy()).to(dev_of(engine))


def poison(engine, shape, dtype=None):
    t = engine.torch
    dtype = dtype or t.int64
    return t.full(shape if isinstance(shape, tuple) else (shape,), {t.int64: POISON64, t.int32: POISON32, t.uint8: POISON8}[dtype], dtype=dtype,
                  device=dev_of(engine))


def host(x):
    return x.cpu().numpy()


class option:
    """An option set for a block and restored after it."""

    def __init__(self, engine, name, value):
        self.engine, self.name, self.value = engine, name, value

    def __enter__(self):
        self.before = self.engine.get_option(self.name)
        self.engine.set_option(self.name, self.value)
        assert self.engine.get_option(self.name) == self.value

    def __exit__(self, *exc):
        self.engine.set_option(self.name, self.before)


def ops_rows(ops, cap=OPS_CAP):
    """The (entries, cap) uint8 array a call leaves behind poison: the ops of every used entry, left-justified."""
    flat = [o for row in ops for o in row] if ops and isinstance(ops[0], list) else list(ops)
    out = np.full((len(flat), cap), POISON8, np.uint8)
    for h, o in enumerate(flat):
        out[h, :len(o)] = np.frombuffer(o, np.uint8)
    return out


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype}{got.shape} vs {want.dtype}{want.shape}"
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} words differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]}, expected {want[tuple(bad[0])]}"


class Placed:
    """The small world on the device at one placement of tests/far_cases.py, and the handle of its database."""

    def __init__(self, engine, kind, nletters=24, first_column=3):
        p = fc.placement(kind)
        self.kind, self.engine, self.order, self.offs, self.qoffs = kind, engine, p["order"], p["offs"], p["qoffs"]
        self.d_q, self.d_db = on_device(engine, p["q"]), on_device(engine, p["db"])
        self.nletters = nletters
        desc, self.moffs = fc.pssm_layout(nletters, first_column)
        self.d_m = on_device(engine, desc, engine.torch.int8)
        self.db = engine.prepare_db(self.d_db, self.offs)
        assert self.db.info() == {"ntargets": fc.NT, "nonempty": 7, "longest": 301, "letters": sum(fc.TLENS)}

    def close(self):
        self.db.close()
        self.d_q = self.d_db = self.d_m = None


# ---- the families: what the device gives, and what the references give, under the same keys ----

def run_single(engine, P):
    """sw_search_device, sw_search_affine_device, sw_align_affine_device: one query at a time, at an address of its own."""
    out, t24 = {}, fc.table24()
    hits = np.array(list(range(fc.NT)) + [7, 7, 1], np.int64)
    for k, n in enumerate(fc.QLENS):
        dq = P.d_q[int(P.qoffs[k]):int(P.qoffs[k + 1])]
        out[f"search q{k}"] = host(engine.search_device(dq, n, P.d_db, P.offs, fc.LINEAR, out=poison(engine, (fc.NT, 3))))
        for g in fc.GAPS:
            out[f"search_affine q{k} {g}"] = host(engine.search_affine_device(dq, n, P.d_db, P.offs, t24, *g, out=poison(engine, (fc.NT, 3))))
            for c in (0, 1):
                aln, ops = engine.align_affine_device(dq, n, P.d_db, P.offs, t24, *g, hits, ops_cap=OPS_CAP,
                                                      out=(poison(engine, (len(hits), 7)), poison(engine, (len(hits), OPS_CAP), engine.torch.uint8)), checkpoint=c)
                aln, ops = host(aln), host(ops)
                assert engine.get_option("last_align_affine_checkpointed") == c and engine.get_option("last_align_affine_band_rows") == (64 if c else 0)
                ops[aln[:, 6] == 0] = POISON8                                           # an empty alignment has no ops: its row is not compared
                out[f"align_affine q{k} {g} checkpoint {c}: aln"], out[f"align_affine q{k} {g} checkpoint {c}: ops"] = aln, ops
    return out


def want_single(exp, order):
    out = {}
    hits = list(range(fc.NT)) + [7, 7, 1]
    for k in range(fc.NQ):
        out[f"search q{k}"] = exp["LIN"][k, order]
        for g in fc.GAPS:
            out[f"search_affine q{k} {g}"] = exp["R"][g][k, order]
            rows = [exp["ALN"][g].get((k, order[h]), ((0,) * 7, b"")) for h in hits]
            for c in (0, 1):
                out[f"align_affine q{k} {g} checkpoint {c}: aln"] = np.array([r for r, _ in rows], np.int64)
                out[f"align_affine q{k} {g} checkpoint {c}: ops"] = ops_rows([o for _, o in rows])
    return out


def run_multi(engine, P, pssm=False):
    """sw_db_search_affine and sw_db_search_affine_top under search_lanes 32 and 16 (with pssm: their PSSM twins)."""
    out = {}
    for g in fc.GAPS:
        scoring = fc.pssm_scoring(P.nletters, g) if pssm else (fc.table24(), *g)
        search, top = (P.db.search_pssm_device, P.db.search_pssm_top_device) if pssm else (P.db.search_affine_device, P.db.search_affine_top_device)
        source, soffs = (P.d_m, P.moffs) if pssm else (P.d_q, P.qoffs)
        for lanes in (32, 16):
            with option(engine, "search_lanes", lanes):
                out[f"search {g} lanes {lanes}"] = host(search(source, soffs, scoring, out=poison(engine, fc.NQ * fc.NT * 3)))
                launches, pk = engine.get_option("last_search_multi_launches"), engine.get_option("last_search_multi_packed_launches")
                assert launches > 0 and pk == (launches if lanes == 16 else 0), (lanes, launches, pk)   # every query of the world is eligible
                hits, nhits = top(source, soffs, scoring, fc.TOP, fc.MIN_SCORE, out=(poison(engine, fc.NQ * fc.TOP * 3), poison(engine, fc.NQ)))
                out[f"top {g} lanes {lanes}: hits"], out[f"top {g} lanes {lanes}: nhits"] = host(hits), host(nhits)
                assert engine.get_option("last_search_top_chunks") == 1
                assert engine.get_option("last_search_multi_packed_launches") == (engine.get_option("last_search_multi_launches") if lanes == 16 else 0)
    return out


def want_multi(exp, order):
    out = {}
    for g in fc.GAPS:
        for lanes in (32, 16):
            out[f"search {g} lanes {lanes}"] = exp["R"][g][:, order]
            out[f"top {g} lanes {lanes}: hits"], out[f"top {g} lanes {lanes}: nhits"] = fc.hit_table(exp, g, order)
    return out


def run_pairs(engine, P):
    """sw_db_search_affine_pairs under search_pairs_lanes 32 and 16, and sw_top_hits_pairs_device over its list."""
    out = {}
    pr = fc.pair_list()
    d_pairs = upload(engine, pr)
    for g in fc.GAPS:
        for lanes in (32, 16):
            with option(engine, "search_pairs_lanes", lanes):
                res = P.db.search_affine_pairs_device(P.d_q, P.qoffs, (fc.table24(), *g), d_pairs, out=poison(engine, len(pr) * 3))
                out[f"pairs {g} lanes {lanes}"] = host(res)
                pk = engine.get_option("last_search_pairs_packed_launches")
                assert (pk > 0) == (lanes == 16) and engine.get_option("last_search_pairs_chunks") == 1, (lanes, pk)
            hits, nhits = engine.top_hits_pairs_device(d_pairs, res, len(pr), fc.NQ, fc.NT, fc.TOP, fc.MIN_SCORE,
                                                       out=(poison(engine, fc.NQ * fc.TOP * 3), poison(engine, fc.NQ)))
            out[f"top of pairs {g} lanes {lanes}: hits"], out[f"top of pairs {g} lanes {lanes}: nhits"] = host(hits), host(nhits)
    return out


def want_pairs(exp, order):
    out = {}
    pr = fc.pair_list()
    for g in fc.GAPS:
        res = fc.pair_results(exp, g, pr, order)
        for lanes in (32, 16):
            out[f"pairs {g} lanes {lanes}"] = res
            # the selection's rule (score, target, list position) over a list with duplicates, in numpy from the reference's results
            out[f"top of pairs {g} lanes {lanes}: hits"], out[f"top of pairs {g} lanes {lanes}: nhits"] = fc.rank_pairs(pr, res, fc.NQ, fc.NT, fc.TOP, fc.MIN_SCORE)
    return out


def run_prefilter(engine, P):
    """sw_db_prefilter_ungapped under prefilter_lanes 0 and 32, and sw_db_search_affine_top_prefiltered under search_pairs_lanes 32 and 16."""
    out, t = {}, engine.torch
    cap = fc.NQ * fc.NT
    for lanes in (0, 32):
        with option(engine, "prefilter_lanes", lanes):
            pairs, npairs, scores = P.db.prefilter_ungapped_device(P.d_q, P.qoffs, fc.table24(), fc.PREFILTER_MIN, cap, want_scores=True,
                                                                   out=(poison(engine, (cap, 2)), poison(engine, 1), poison(engine, (fc.NQ, fc.NT), t.int32)))
            pairs, n = host(pairs), int(npairs.item())
            pk, launches = engine.get_option("last_prefilter_packed_launches"), engine.get_option("last_prefilter_launches")
            assert launches > 0 and pk == (launches if lanes == 0 else 0), (lanes, launches, pk)
            assert 0 < n < cap and (pairs[n:] == -1).all()
            head = pairs[:n]
            out[f"prefilter lanes {lanes}: pairs"] = head[np.lexsort((head[:, 1], head[:, 0]))]
            out[f"prefilter lanes {lanes}: scores"] = host(scores)
    for g in fc.GAPS:
        for lanes in (32, 16):
            with option(engine, "search_pairs_lanes", lanes):
                hits, nhits, npairs = P.db.search_affine_top_prefiltered_device(P.d_q, P.qoffs, (fc.table24(), *g), fc.PREFILTER_MIN, cap, fc.TOP, fc.MIN_SCORE,
                                                                                out=(poison(engine, fc.NQ * fc.TOP * 3), poison(engine, fc.NQ)))
                out[f"top prefiltered {g} lanes {lanes}: hits"], out[f"top prefiltered {g} lanes {lanes}: nhits"] = host(hits), host(nhits)
                out[f"top prefiltered {g} lanes {lanes}: npairs"] = host(npairs)
                assert (engine.get_option("last_search_pairs_packed_launches") > 0) == (lanes == 16)
    return out


def want_prefilter(exp, order, offs):
    out = {}
    u = exp["U"][:, order]
    passing = np.argwhere((u >= fc.PREFILTER_MIN) & (np.diff(offs) > 0)[None, :]).astype(np.int64)
    for lanes in (0, 32):
        out[f"prefilter lanes {lanes}: pairs"], out[f"prefilter lanes {lanes}: scores"] = passing, u.astype(np.int32)
    for g in fc.GAPS:
        for lanes in (32, 16):
            out[f"top prefiltered {g} lanes {lanes}: hits"], out[f"top prefiltered {g} lanes {lanes}: nhits"] = fc.prefiltered_table(exp, g, order)
            out[f"top prefiltered {g} lanes {lanes}: npairs"] = np.array([len(passing)], np.int64)
    return out


def run_align_hits(engine, P, exp, pssm=False):
    """sw_db_align_affine_hits (with pssm: sw_db_align_pssm_hits) over the reference's hit table, whole matrices and checkpointed."""
    out, t = {}, engine.torch
    for g in fc.GAPS:
        hits, nhits = fc.hit_table(exp, g, P.order)
        d_hits, d_nhits = upload(engine, hits), upload(engine, np.minimum(nhits, NHITS_CUT))
        for c in (0, 1):
            bufs = (poison(engine, (fc.NQ * fc.TOP, 7)), poison(engine, (fc.NQ * fc.TOP, OPS_CAP), t.uint8))
            if pssm:
                aln, ops = P.db.align_pssm_hits_device(P.d_m, P.moffs, fc.pssm_scoring(P.nletters, g), d_hits, d_nhits, ops_cap=OPS_CAP, out=bufs, checkpoint=c)
            else:
                aln, ops = P.db.align_affine_hits_device(P.d_q, P.qoffs, (fc.table24(), *g), d_hits, d_nhits, ops_cap=OPS_CAP, out=bufs, checkpoint=c)
            out[f"align hits {g} checkpoint {c}: aln"], out[f"align hits {g} checkpoint {c}: ops"] = host(aln), host(ops).reshape(-1, OPS_CAP)
            assert engine.get_option("last_align_hits_checkpointed") == c and engine.get_option("last_align_hits_band_rows") == (64 if c else 0)
            assert engine.get_option("last_align_hits_launches") > 0
    return out


def want_align_hits(exp, order):
    out = {}
    for g in fc.GAPS:
        hits, nhits = fc.hit_table(exp, g, order)
        aln, ops = fc.alignments(exp, g, hits, np.minimum(nhits, NHITS_CUT), order)
        for c in (0, 1):
            out[f"align hits {g} checkpoint {c}: aln"], out[f"align hits {g} checkpoint {c}: ops"] = aln, ops_rows(ops)
    return out


HITS_GUARD = 4096


def poisoned_window(engine, size, lo, hi, far):
    """A uint8 device buffer of `size` bytes, not initialised but for poison on [lo - guard, hi + guard) and, with far, on the same
    range 2^32 bytes below: (buffer, the poisoned (first, last) ranges)."""
    t = engine.torch
    buf = t.empty(size, dtype=t.uint8, device=dev_of(engine))
    spans = [(max(0, lo - HITS_GUARD), min(size, hi + HITS_GUARD))]
    if far:
        assert lo - fc.WRAP - HITS_GUARD >= 0 and hi - fc.WRAP + HITS_GUARD < lo - HITS_GUARD
        spans.append((lo - fc.WRAP - HITS_GUARD, hi - fc.WRAP + HITS_GUARD))
    for a, b in spans:
        buf[a:b] = POISON8
    return buf, spans


def still_poison(buf, spans, lo, hi, what):
    """Every poisoned byte outside the live window [lo, hi) is still poison."""
    for a, b in spans:
        if a <= lo and hi <= b:
            assert bool((buf[a:lo] == POISON8).all()) and bool((buf[hi:b] == POISON8).all()), f"{what}: written outside the queries' columns"
        else:
            assert bool((buf[a:b] == POISON8).all()), f"{what}: the bytes 2^32 below the output were written"


def run_pssm_hits(engine, P, exp, family):
    """sw_db_pssm_hit_weights, or sw_db_pssm_from_hits with and without d_weights, with d_counts, and once with d_pssm_out == d_prior,
    over the reference's hit table and the rule's alignments and ops; every call twice.  The prior is the placement's PSSM; the new
    matrix goes to a buffer of its own at the same columns, with poison around the queries' columns and (far columns) 2^32 bytes
    below them; the in-place call runs last, on the prior itself, whose live window is then put back."""
    out, t, nl = {}, engine.torch, P.nletters
    lo, hi = int(P.moffs[0]) * nl, int(P.moffs[-1]) * nl
    far = lo >= fc.WRAP
    ncnt = (hi - lo)
    for g in fc.GAPS:
        c = fc.hits_case(exp, g, P.order, nl)
        sc = fc.pssm_scoring(nl, g)
        tabs = (upload(engine, c.hits), upload(engine, c.nhits), upload(engine, c.aln), upload(engine, c.ops))
        n = fc.NQ * fc.TOP
        twice = []
        for _ in range(2):
            wbuf = poison(engine, n + 2 * HITS_GUARD, t.int32)
            d_w = P.db.pssm_hit_weights_device(P.moffs, sc, (fc.PER_HIT, fc.INCLUDE_MIN), *tabs, fc.OPS_CAP, out=wbuf[HITS_GUARD:HITS_GUARD + n], top=fc.TOP)
            assert engine.get_option("last_pssm_weights_launches") == 2 and engine.get_option("last_pssm_weights_tiles") >= 1
            engine.synchronize()
            assert bool((wbuf[:HITS_GUARD] == POISON32).all()) and bool((wbuf[HITS_GUARD + n:] == POISON32).all()), "the weights were written outside their buffer"
            twice.append(host(d_w).reshape(fc.NQ, fc.TOP))
        assert twice[0].tobytes() == twice[1].tobytes()
        if family == "pssm_hit_weights":
            out[f"weights {g}"] = twice[0]
            continue
        for how, pw, weights in (("plain", fc.PRIOR_WEIGHT, None), ("weighted", fc.PRIOR_WEIGHT_WEIGHTED, d_w)):
            twice = []
            for _ in range(2):
                mbuf, spans = poisoned_window(engine, P.d_m.numel(), lo, hi, far)
                cbuf = poison(engine, ncnt + 2 * HITS_GUARD, t.int32)
                P.db.pssm_from_hits_device(P.d_m, P.moffs, sc, (fc.table24(), pw, fc.INCLUDE_MIN), *tabs, fc.OPS_CAP, weights=weights, out=mbuf.view(t.int8),
                                           top=fc.TOP, counts=cbuf[HITS_GUARD:HITS_GUARD + ncnt])
                assert engine.get_option("last_pssm_hits_launches") == 1
                engine.synchronize()
                still_poison(mbuf, spans, lo, hi, f"{how} {g}")
                assert bool((cbuf[:HITS_GUARD] == POISON32).all()) and bool((cbuf[HITS_GUARD + ncnt:] == POISON32).all()), "the counts were written outside their buffer"
                twice.append((host(mbuf[lo:hi].view(t.int8)).reshape(-1, nl), host(cbuf[HITS_GUARD:HITS_GUARD + ncnt]).reshape(-1, nl)))
                del mbuf, cbuf
            assert twice[0][0].tobytes() == twice[1][0].tobytes() and twice[0][1].tobytes() == twice[1][1].tobytes()
            out[f"update {g} {how}: matrix"], out[f"update {g} {how}: counts"] = twice[0]
        # in place, on the prior itself: the decoy 2^32 bytes below it stays what it was
        keep = P.d_m[lo:hi].clone()
        below = P.d_m[lo - fc.WRAP:hi - fc.WRAP].clone() if far else None
        P.db.pssm_from_hits_device(P.d_m, P.moffs, sc, (fc.table24(), fc.PRIOR_WEIGHT_WEIGHTED, fc.INCLUDE_MIN), *tabs, fc.OPS_CAP, weights=d_w, out=P.d_m, top=fc.TOP)
        engine.synchronize()
        out[f"update {g} in place: matrix"] = host(P.d_m[lo:hi]).reshape(-1, nl)
        if far:
            assert t.equal(P.d_m[lo - fc.WRAP:hi - fc.WRAP], below), "the decoy PSSM below the prior changed"
        P.d_m[lo:hi] = keep
    return out


def want_pssm_hits(exp, order, nletters, family):
    out = {}
    for g in fc.GAPS:
        c = fc.hits_case(exp, g, order, nletters)
        w, m, _ = fc.hits_want(c, True)
        if family == "pssm_hit_weights":
            out[f"weights {g}"] = w
            continue
        _, plain, counts = fc.hits_want(c, False)
        _, _, wcounts = fc.hits_want(c, True)
        out[f"update {g} plain: matrix"], out[f"update {g} plain: counts"] = plain, counts
        out[f"update {g} weighted: matrix"], out[f"update {g} weighted: counts"] = m, wcounts
        out[f"update {g} in place: matrix"] = m
    return out


def run_family(engine, exp, P, family):
    """(what the device gave, what the references give) of one family at one placement."""
    if family in ("pssm_from_hits", "pssm_hit_weights"):
        return run_pssm_hits(engine, P, exp, family), want_pssm_hits(exp, P.order, P.nletters, family)
    if family == "single":
        return run_single(engine, P), want_single(exp, P.order)
    if family in ("multi", "pssm"):
        return run_multi(engine, P, family == "pssm"), want_multi(exp, P.order)
    if family == "pairs":
        return run_pairs(engine, P), want_pairs(exp, P.order)
    if family == "prefilter":
        return run_prefilter(engine, P), want_prefilter(exp, P.order, P.offs)
    assert family in ("align_hits", "align_pssm_hits")
    return run_align_hits(engine, P, exp, family == "align_pssm_hits"), want_align_hits(exp, P.order)


_NEAR = {}


def near(engine, exp, family, nletters=24):
    """The family's outputs at near placement, once per process."""
    if (family, nletters) not in _NEAR:
        P = Placed(engine, "near", nletters)
        try:
            _NEAR[(family, nletters)] = run_family(engine, exp, P, family)[0]
        finally:
            P.close()
    return _NEAR[(family, nletters)]


def check_family(engine, exp, P, family):
    got, want = run_family(engine, exp, P, family)
    assert set(got) == set(want) and got
    for key in want:
        same(got[key], want[key], f"{P.kind}: {key}")
    if P.order == fc.NATURAL_ORDER:                                                    # the same target order: the same bytes as at near placement
        for key, v in near(engine, exp, family, P.nletters).items():
            assert got[key].tobytes() == v.tobytes(), f"{P.kind} against near placement: {key}"


# ---- A. far inputs ----

FAR_INPUTS = [(kind, family) for kind in ("db_far", "db_straddle") for family in ("single", "multi", "pairs", "prefilter", "align_hits", "pssm", "align_pssm_hits", "pssm_from_hits", "pssm_hit_weights")] + \
             [(kind, family) for kind in ("q_far", "both_far") for family in ("multi", "pairs", "prefilter", "align_hits")]


@pytest.mark.parametrize("kind,family", FAR_INPUTS, ids=[f"{k}-{f}" for k, f in FAR_INPUTS])
def test_far_inputs(engine, checker, kind, family):  # noqa: F811
    exp = fc.expected(checker)
    P = Placed(engine, kind)
    assert P.d_db.numel() > 2**32 or kind == "q_far"
    assert P.d_q.numel() > 2**32 or kind.startswith("db_")
    try:
        check_family(engine, exp, P, family)
    finally:
        P.close()


@pytest.mark.parametrize("kind", ["near", "db_far"])
@pytest.mark.parametrize("nletters", [256, 24])
@pytest.mark.parametrize("family", ["pssm", "align_pssm_hits", "pssm_from_hits", "pssm_hit_weights"])
def test_far_pssm_columns(engine, checker, family, nletters, kind):  # noqa: F811
    """The crossing comes from the product: the column index stays below 2^32, times nletters it does not."""
    exp = fc.expected(checker)
    P = Placed(engine, kind, nletters, fc.PSSM_FAR[nletters])
    assert P.moffs[0] < 2**32 <= P.moffs[0] * nletters and P.d_m.numel() > 2**32
    try:
        check_family(engine, exp, P, family)
    finally:
        P.close()


# ---- E. the Python layer ----

def header_prototypes():
    """{function: [(type, name)]} of every prototype of include/swhip.h."""
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "swhip.h")).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(sw_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        params = []
        for p in m.group(2).split(","):
            p = " ".join(p.split())
            if p and p != "void":
                ty, name = re.match(r"(.*?)(\w+)$", p).groups()
                params.append((ty.strip(), name))
        out[m.group(1)] = params
    return out


def test_every_length_offset_count_cap_and_stride_crosses_ctypes_as_64_bits(swamd):
    """The header says which parameters these are: every int64_t (and size_t) passed by value, and every pointer to int64_t."""
    protos = header_prototypes()
    assert set(swamd.ABI) <= set(protos), sorted(set(swamd.ABI) - set(protos))
    wide = 0
    for name, (_, argtypes) in swamd.ABI.items():
        params = protos[name]
        assert len(params) == len(argtypes), f"{name}: {len(argtypes)} argtypes for {len(params)} parameters"
        for (ty, pname), at in zip(params, argtypes):
            if ty in ("int64_t", "size_t"):
                assert ctypes.sizeof(at) == 8 and at in (ctypes.c_int64, ctypes.c_size_t, ctypes.c_uint64), f"{name}({pname}): {ty} passed as {at}"
                wide += 1
            elif "*" in ty:
                assert ctypes.sizeof(at) == ctypes.sizeof(ctypes.c_void_p), f"{name}({pname}): {ty} passed as {at}"
                if at not in (ctypes.c_void_p, ctypes.c_char_p) and re.match(r"(const )?int64_t ?\*", ty):
                    assert at._type_ is ctypes.c_int64, f"{name}({pname})"
    named = {p for params in protos.values() for ty, p in params if ty == "int64_t"}
    assert {"ntargets", "nqueries", "npairs", "ops_cap", "pairs_cap", "a_stride", "b_stride", "top", "qlen", "nhits"} <= named and wide > 100


def test_public_methods_take_far_offsets(engine, checker):  # noqa: F811
    """One far call per family through Database and Engine as a caller uses them -- no `out`, no raw ctypes."""
    exp = fc.expected(checker)
    g = fc.GAPS[0]
    P = Placed(engine, "both_far", 24, fc.PSSM_FAR[24])
    t24, scoring, psc = fc.table24(), (fc.table24(), *g), fc.pssm_scoring(24, g)
    try:
        dq = P.d_q[int(P.qoffs[3]):int(P.qoffs[4])]
        same(host(engine.search_device(dq, 513, P.d_db, P.offs, fc.LINEAR)), exp["LIN"][3], "Engine.search_device")
        same(host(engine.search_affine_device(dq, 513, P.d_db, P.offs, t24, *g)), exp["R"][g][3], "Engine.search_affine_device")
        aln, _ = engine.align_affine_device(dq, 513, P.d_db, P.offs, t24, *g, [8, 7], ops_cap=OPS_CAP)
        same(host(aln), np.array([exp["ALN"][g][(3, 8)][0], exp["ALN"][g][(3, 7)][0]], np.int64), "Engine.align_affine_device")
        same(host(P.db.search_affine_device(P.d_q, P.qoffs, scoring)), exp["R"][g], "Database.search_affine_device")
        hits, nhits = P.db.search_affine_top_device(P.d_q, P.qoffs, scoring, fc.TOP, fc.MIN_SCORE)
        wh, wn = fc.hit_table(exp, g)
        same(host(hits), wh, "Database.search_affine_top_device")
        same(host(nhits), wn, "Database.search_affine_top_device: nhits")
        same(host(engine.top_hits_device(P.db.search_affine_device(P.d_q, P.qoffs, scoring), fc.NQ, fc.NT, fc.TOP, fc.MIN_SCORE)[0]), wh, "Engine.top_hits_device")
        pr = fc.pair_list()
        d_pairs = upload(engine, pr)
        res = P.db.search_affine_pairs_device(P.d_q, P.qoffs, scoring, d_pairs)
        same(host(res), fc.pair_results(exp, g, pr), "Database.search_affine_pairs_device")
        ph, _ = engine.top_hits_pairs_device(d_pairs, res, len(pr), fc.NQ, fc.NT, fc.TOP, fc.MIN_SCORE)
        same(host(ph), fc.rank_pairs(pr, fc.pair_results(exp, g, pr), fc.NQ, fc.NT, fc.TOP, fc.MIN_SCORE)[0], "Engine.top_hits_pairs_device")
        _, _, scores = P.db.prefilter_ungapped_device(P.d_q, P.qoffs, t24, fc.PREFILTER_MIN, fc.NQ * fc.NT, want_scores=True)
        same(host(scores), exp["U"].astype(np.int32), "Database.prefilter_ungapped_device")
        fh, _, _ = P.db.search_affine_top_prefiltered_device(P.d_q, P.qoffs, scoring, fc.PREFILTER_MIN, fc.NQ * fc.NT, fc.TOP, fc.MIN_SCORE)
        same(host(fh), fc.prefiltered_table(exp, g)[0], "Database.search_affine_top_prefiltered_device")
        want, _ = fc.alignments(exp, g, wh, wn)
        aln, _ = P.db.align_affine_hits_device(P.d_q, P.qoffs, scoring, hits, nhits, ops_cap=OPS_CAP)
        same(host(aln), want, "Database.align_affine_hits_device")
        same(host(P.db.search_pssm_device(P.d_m, P.moffs, psc)), exp["R"][g], "Database.search_pssm_device")
        same(host(P.db.search_pssm_top_device(P.d_m, P.moffs, psc, fc.TOP, fc.MIN_SCORE)[0]), wh, "Database.search_pssm_top_device")
        aln, ops = P.db.align_pssm_hits_device(P.d_m, P.moffs, psc, hits, nhits, ops_cap=OPS_CAP, checkpoint=1)
        same(host(aln), want, "Database.align_pssm_hits_device")
        c = fc.hits_case(exp, g, nhits_cut=[fc.TOP] * fc.NQ)
        ww, wm, _ = fc.hits_want(c, True)
        w = P.db.pssm_hit_weights_device(P.moffs, psc, (fc.PER_HIT, fc.INCLUDE_MIN), hits, nhits, aln, ops, OPS_CAP, top=fc.TOP)
        same(host(w).reshape(fc.NQ, fc.TOP), ww, "Database.pssm_hit_weights_device")
        m = P.db.pssm_from_hits_device(P.d_m, P.moffs, psc, (t24, fc.PRIOR_WEIGHT_WEIGHTED, fc.INCLUDE_MIN), hits, nhits, aln, ops, OPS_CAP, weights=w, out=P.d_m, top=fc.TOP)
        same(host(m[int(P.moffs[0]) * 24:int(P.moffs[-1]) * 24]).reshape(-1, 24), wm, "Database.pssm_from_hits_device")     # (in place: the last use of the PSSM)
    finally:
        P.close()


# ---- B. far outputs ----

STEP = 2**26


def count_unequal(x, value, step=STEP):
    """How many elements of a flat device tensor differ from `value`, counted on the device slice by slice."""
    return sum(int((x[s:s + step] != value).sum()) for s in range(0, x.numel(), step))


class BigDb:
    """The nine targets of the world among 2^24 - 9 empty ones (the bytes of the near placement), and queries repeated from the world."""

    def __init__(self, engine, which):
        p = fc.placement("near")
        self.d_db, self.offs = on_device(engine, p["db"]), fc.big_offsets(int(p["offs"][0]))
        desc, self.qoffs, self.which = fc.repeated_queries(which)
        self.d_q = on_device(engine, desc)
        self.moffs = self.qoffs - self.qoffs[0]
        self.d_m = upload(engine, fc.pssm_of([fc.world()["queries"][k] for k in which], 24).reshape(-1))
        self.db = engine.prepare_db(self.d_db, self.offs)
        assert self.db.info() == {"ntargets": fc.BIG_NT, "nonempty": 7, "longest": 301, "letters": sum(fc.TLENS)}

    def close(self):
        self.db.close()
        self.d_db = self.d_q = self.d_m = None


@pytest.mark.parametrize("how", ["lanes32", "lanes16", "pssm16"])
def test_result_table_beyond_4gib(engine, checker, how):  # noqa: F811
    """12 x 2^24 results: 4.5 GiB, the rows of queries 10 and 11 reach beyond byte 2^32, and the last six targets are live."""
    g, guard = fc.GAPS[0], 1024
    want = fc.expected(checker)["R"][g][[k % fc.NQ for k in range(fc.BIG_NQ)]]
    B = BigDb(engine, [k % fc.NQ for k in range(fc.BIG_NQ)])
    try:
        n = fc.BIG_NQ * fc.BIG_NT * 3
        buf = poison(engine, n + 2 * guard)
        table = buf[guard:guard + n]
        with option(engine, "search_lanes", 32 if how == "lanes32" else 16):
            if how == "pssm16":
                B.db.search_pssm_device(B.d_m, B.moffs, fc.pssm_scoring(24, g), out=table)
            else:
                B.db.search_affine_device(B.d_q, B.qoffs, (fc.table24(), *g), out=table)
            engine.synchronize()
            launches, pk = engine.get_option("last_search_multi_launches"), engine.get_option("last_search_multi_packed_launches")
            assert launches > 0 and pk == (0 if how == "lanes32" else launches), (how, launches, pk)
        assert bool((buf[:guard] == POISON64).all()) and bool((buf[guard + n:] == POISON64).all()), "written outside the table"
        assert count_unequal(table, 0) == np.count_nonzero(want)                       # every other entry is {0, 0, 0} over the poison
        same(host(table.view(fc.BIG_NQ, fc.BIG_NT, 3)[:, fc.BIG_LIVE]), want, f"{how}: the live entries")
        for top, min_score in ((1, 1), (5, 0), (16, 0)):
            hits, nhits = engine.top_hits_device(table, fc.BIG_NQ, fc.BIG_NT, top, min_score, out=(poison(engine, fc.BIG_NQ * top * 3), poison(engine, fc.BIG_NQ)))
            wh, wn = fc.sparse_rank(want, top, min_score)
            same(host(hits), wh, f"{how}: sw_top_hits_device top {top} min_score {min_score}")
            same(host(nhits), wn, f"{how}: sw_top_hits_device top {top} min_score {min_score}: nhits")
            assert engine.get_option("last_search_top_kernel") == 1                    # 2^24 targets: radix select
        del buf, table
    finally:
        B.close()


def test_prefilter_score_table_beyond_4gib(engine, checker):  # noqa: F811
    """72 queries of 1 and 63 letters x 2^24 targets x 4 bytes: 4.5 GiB of scores."""
    t = engine.torch
    which = [k % 2 for k in range(fc.FILTER_NQ)]
    u = fc.expected(checker)["U"][which]
    B = BigDb(engine, which)
    try:
        cap = 4096
        pairs, npairs, scores = B.db.prefilter_ungapped_device(B.d_q, B.qoffs, fc.table24(), fc.PREFILTER_MIN, cap, want_scores=True,
                                                               out=(poison(engine, (cap, 2)), poison(engine, 1), poison(engine, (fc.FILTER_NQ, fc.BIG_NT), t.int32)))
        engine.synchronize()
        assert engine.get_option("last_prefilter_packed_launches") == engine.get_option("last_prefilter_launches") > 0
        assert count_unequal(scores.view(-1), 0) == np.count_nonzero(u)
        same(host(scores[:, fc.BIG_LIVE]), u.astype(np.int32), "the live scores")
        want = np.array([(q, fc.BIG_LIVE[k]) for q in range(fc.FILTER_NQ) for k in range(fc.NT) if fc.TLENS[k] and u[q, k] >= fc.PREFILTER_MIN], np.int64)
        pairs, n = host(pairs), int(npairs.item())
        assert n == len(want) > 0 and (pairs[n:] == -1).all()
        same(pairs[:n][np.lexsort((pairs[:n, 1], pairs[:n, 0]))], want, "the pair list")
        del scores
    finally:
        B.close()


def test_pair_list_and_results_beyond_4gib(engine, checker):  # noqa: F811
    """2^28 entries: 4 GiB of pairs and 6 GiB of results.  Every entry is invalid -- query -1, target = ntargets or an empty target, in
    turn -- but 41 live ones at the head, where the results cross byte 2^32, and at the tail, where the list ends at byte 2^32."""
    t, g, n = engine.torch, fc.GAPS[0], fc.BIG_NPAIRS
    exp = fc.expected(checker)
    live = fc.big_live_pairs()
    want = fc.pair_results(exp, g, live)
    assert (want[:, 1] > 0).all()
    assert sum(1 for p in fc.BIG_LIVE_PAIRS if p >= n - 2**22) % 2 == 1                # an odd number in the last chunk: an odd (query, bucket) cell
    P = Placed(engine, "near")
    try:
        pairs = t.empty((n, 2), dtype=t.int64, device=dev_of(engine))
        for s in range(0, n, 2**25):
            i = t.arange(s, s + 2**25, device=dev_of(engine))
            kind = i % 3
            pairs[s:s + 2**25, 0] = t.where(kind == 0, -1, i % fc.NQ)
            pairs[s:s + 2**25, 1] = t.where(kind == 1, fc.NT, t.where(kind == 2, (i % 2) * 5, i % fc.NT))       # targets 0 and 5 are empty
            del i, kind
        at = upload(engine, np.array(fc.BIG_LIVE_PAIRS, np.int64))
        pairs[at] = upload(engine, live)
        res = poison(engine, n * 3)
        assert engine.get_option("search_pairs_chunk") == 2**22
        for lanes in (32, 16):
            res.fill_(POISON64)
            with option(engine, "search_pairs_lanes", lanes):
                out = P.db.search_affine_pairs_device(P.d_q, P.qoffs, (fc.table24(), *g), pairs, out=res)
                engine.synchronize()
                assert engine.get_option("last_search_pairs_chunks") == n // 2**22 == 64
                assert (engine.get_option("last_search_pairs_packed_launches") > 0) == (lanes == 16)
            assert count_unequal(res, 0) == np.count_nonzero(want), f"lanes {lanes}"
            same(host(out[at]), want, f"lanes {lanes}: the live entries")
        hits, nhits = engine.top_hits_pairs_device(pairs, out, n, fc.NQ, fc.NT, 8, 1, out=(poison(engine, fc.NQ * 8 * 3), poison(engine, fc.NQ)))
        wh, wn = fc.rank_pairs(live, want, fc.NQ, fc.NT, 8, 1)             # the list position orders equal pairs: the live entries in list order
        same(host(hits), wh, "sw_top_hits_pairs_device")
        same(host(nhits), wn, "sw_top_hits_pairs_device: nhits")
        del pairs, res, out
    finally:
        P.close()


@pytest.mark.parametrize("checkpoint", [0, 1])
@pytest.mark.parametrize("pssm", [False, True], ids=["table", "pssm"])
def test_ops_rows_beyond_4gib(engine, checker, pssm, checkpoint):  # noqa: F811
    """ops_cap = 2^20 and top = 1024: 5 GiB of ops rows, the row of query 4 starts at byte 2^32."""
    t, g, cap, top = engine.torch, fc.GAPS[0], 2**20, 1024
    exp = fc.expected(checker)
    nhits = np.array([2, 0, 1, 3, 2], np.int64)
    assert 4 * top * cap == 2**32
    ranked, _ = fc.hit_table(exp, g)
    hits = np.zeros((fc.NQ, top, 3), np.int64)
    hits[:, :, 0] = 7                                                                  # beyond a row's count: a valid target that must not be aligned
    hits[:, :fc.TOP] = ranked
    want, wops = fc.alignments(exp, g, hits, nhits)
    P = Placed(engine, "near")
    try:
        aln, ops = poison(engine, (fc.NQ * top, 7)), poison(engine, (fc.NQ * top, cap), t.uint8)
        call = P.db.align_pssm_hits_device if pssm else P.db.align_affine_hits_device
        source, soffs, scoring = (P.d_m, P.moffs, fc.pssm_scoring(24, g)) if pssm else (P.d_q, P.qoffs, (fc.table24(), *g))
        got, _ = call(source, soffs, scoring, upload(engine, hits), upload(engine, nhits), ops_cap=cap, out=(aln, ops), checkpoint=checkpoint)
        engine.synchronize()
        assert engine.get_option("last_align_hits_checkpointed") == checkpoint and engine.get_option("last_align_hits_launches") > 0
        same(host(got), want, "aln")
        used = [q * top + r for q in range(fc.NQ) for r in range(int(nhits[q]))]
        assert max(used) * cap >= 2**32
        heads = host(ops[used, :OPS_CAP])
        same(heads, ops_rows([wops[q][r] for q in range(fc.NQ) for r in range(int(nhits[q]))]), "the used ops rows")
        assert all(len(wops[q][r]) > 0 for q in range(fc.NQ) for r in range(int(nhits[q])))
        if pssm:
            # the tables the alignment left on the device, rows of 2^20 ops and all, go on to the weights and the update: entry 4 x top
            # starts at byte 2^32 of the ops.  Expected: the numpy rules on the same entries in a table of TOP columns and OPS_CAP ops.
            c = fc.hits_case(exp, g, nhits_cut=nhits, hits=(ranked, np.full(fc.NQ, fc.TOP, np.int64)))
            ww, wm, wc_ = fc.hits_want(c, True)
            d_hits, d_nhits = upload(engine, hits), upload(engine, nhits)
            lo, hi = int(P.moffs[0]) * 24, int(P.moffs[-1]) * 24
            for _ in range(2):
                wbuf = poison(engine, fc.NQ * top + 2 * HITS_GUARD, t.int32)
                d_w = P.db.pssm_hit_weights_device(P.moffs, scoring, (fc.PER_HIT, fc.INCLUDE_MIN), d_hits, d_nhits, got, ops, cap,
                                                   out=wbuf[HITS_GUARD:HITS_GUARD + fc.NQ * top], top=top)
                assert engine.get_option("last_pssm_weights_launches") == 2
                mbuf, spans = poisoned_window(engine, P.d_m.numel(), lo, hi, False)
                cbuf = poison(engine, hi - lo + 2 * HITS_GUARD, t.int32)
                P.db.pssm_from_hits_device(P.d_m, P.moffs, scoring, (fc.table24(), fc.PRIOR_WEIGHT_WEIGHTED, fc.INCLUDE_MIN), d_hits, d_nhits, got, ops, cap,
                                           weights=d_w, out=mbuf.view(t.int8), top=top, counts=cbuf[HITS_GUARD:HITS_GUARD + hi - lo])
                assert engine.get_option("last_pssm_hits_launches") == 1
                engine.synchronize()
                assert bool((wbuf[:HITS_GUARD] == POISON32).all()) and bool((wbuf[HITS_GUARD + fc.NQ * top:] == POISON32).all())
                assert bool((cbuf[:HITS_GUARD] == POISON32).all()) and bool((cbuf[HITS_GUARD + hi - lo:] == POISON32).all())
                still_poison(mbuf, spans, lo, hi, "the update behind far ops rows")
                w = host(d_w).reshape(fc.NQ, top)
                same(w[:, :fc.TOP], ww, "weights from far ops rows")
                assert not w[:, fc.TOP:].any()
                same(host(mbuf[lo:hi].view(t.int8)).reshape(-1, 24), wm, "update from far ops rows: matrix")
                same(host(cbuf[HITS_GUARD:HITS_GUARD + hi - lo]).reshape(-1, 24), wc_, "update from far ops rows: counts")
            assert ww[4].any() and wc_[int(c.qoffs[4]):].any()                           # the entries beyond byte 2^32 weigh and count
            same(host(ops[used, :OPS_CAP]), heads, "the used ops rows after the weights and the update: only read")
        ops[used, :OPS_CAP] = POISON8                                                   # what was compared; everything else must still be poison
        assert count_unequal(ops.view(-1).view(t.int64), POISON64) == 0, "an unused ops row or the tail of a used one was written"
        del aln, ops, got
    finally:
        P.close()


def test_count_matrix_beyond_4gib(engine):
    """sw_db_pssm_from_hits with d_counts over five queries of 2^20 - 1 columns and 256 letters: 5.4 GB of int32 counts (and 1.3 GB each of
    prior and matrix; about 8 GiB in all).  Used entries in the first and the last query only; the last query's counts lie beyond byte
    2^32 and the count 2^32 bytes below each is an expected zero (tests/far_cases.py: count_case), so a count stored through 32 bits
    shows twice: missing above, present below.  The live windows are compared with the numpy rule; everything else is counted on the
    device: no other count is nonzero, no other entry of the matrix differs from min(prior, smax).  Twice, the same buffers poisoned
    again.  A far weights table, hit table or accumulator is NOT built: nqueries x top would have to pass 2^30, and the sw_hit and
    sw_alignment tables alone would then take more than 80 GiB."""
    t, cc = engine.torch, fc.count_case()
    wm, wcnt = fc.count_want()
    nl, L, nq, top = fc.COUNT_NL, fc.COUNT_QLEN, fc.COUNT_NQ, fc.COUNT_TOP
    total = nq * L * nl
    assert total * 4 > 2**32 and total + total + total * 4 < 9 * 2**30
    P = Placed(engine, "near")
    try:
        prior = t.full((total,), fc.COUNT_PRIOR, dtype=t.int8, device=dev_of(engine))
        mbuf = t.empty(total + 2 * HITS_GUARD, dtype=t.uint8, device=dev_of(engine))
        cbuf = t.empty(total + 2 * HITS_GUARD, dtype=t.int32, device=dev_of(engine))
        tabs = (upload(engine, cc["hits"]), upload(engine, cc["nhits"]), upload(engine, cc["aln"]), upload(engine, cc["ops"]))
        d_w = upload(engine, cc["weights"])
        sc = fc.pssm_scoring(nl, fc.GAPS[0])
        for run in range(2):
            mbuf.fill_(POISON8)
            cbuf.fill_(POISON32)
            m, counts = mbuf[HITS_GUARD:HITS_GUARD + total].view(t.int8), cbuf[HITS_GUARD:HITS_GUARD + total]
            P.db.pssm_from_hits_device(prior, cc["qoffs"], sc, (fc.table24(), fc.COUNT_PW, fc.COUNT_INC), *tabs, cc["cap"], weights=d_w, out=m, top=top, counts=counts)
            assert engine.get_option("last_pssm_hits_launches") == 1
            engine.synchronize()
            assert bool((mbuf[:HITS_GUARD] == POISON8).all()) and bool((mbuf[HITS_GUARD + total:] == POISON8).all()), "the matrix was written outside its buffer"
            assert bool((cbuf[:HITS_GUARD] == POISON32).all()) and bool((cbuf[HITS_GUARD + total:] == POISON32).all()), "the counts were written outside their buffer"
            at = 0
            for q, c0, n, r in cc["windows"]:
                lo, hi = (q * L + c0) * nl, (q * L + c0 + n) * nl
                assert (q == nq - 1) == (lo * 4 > 2**32)
                same(host(counts[lo:hi]).reshape(n, nl), wcnt[at:at + n], f"run {run}: counts of query {q}, entry {r}")
                same(host(m[lo:hi]).reshape(n, nl), wm[at:at + n], f"run {run}: matrix of query {q}, entry {r}")
                at += n
            assert count_unequal(counts, 0) == np.count_nonzero(wcnt), "a count outside the live windows is not zero"
            assert count_unequal(m, min(fc.COUNT_PRIOR, fc.SMAX)) == int((wm != min(fc.COUNT_PRIOR, fc.SMAX)).sum()), "an entry outside the live windows changed"
        assert bool((prior == fc.COUNT_PRIOR).all()), "the prior changed"
        del prior, mbuf, cbuf
    finally:
        P.close()


# ---- D. batch strides ----

def test_batch_strides_beyond_4gib(engine, oracle):
    """sw_batch_device_ex with a_stride = b_stride = 2^30 + 64: pair 4 starts at byte 2^32 + 256 of either buffer."""
    t, c, b = engine.torch, fc.batch_case(), fc.BATCH
    cols, rows, n, stride = b["cols"], b["rows"], b["npairs"], b["stride"]
    truth = [oracle.fill(c["A"][k], c["B"][k], fc.LINEAR) for k in range(n)]
    for a_, b_ in ((c["a_wrapped"], c["b_decoy"]), (c["a_wrapped"], c["B"][4]), (c["A"][4], c["b_decoy"])):   # what a wrapped address would give
        h, _, mp = oracle.fill(a_, b_, fc.LINEAR)
        assert (mp, int(h.flat[mp])) != (truth[4][2], int(truth[4][0].flat[truth[4][2]]))
    d_a, d_b = (t.empty((n, stride), dtype=t.uint8, device=dev_of(engine)) for _ in range(2))
    assert d_a[4].data_ptr() - d_a.data_ptr() == 2**32 + b["wrap"]
    d_a[:, :cols], d_b[:, :rows] = upload(engine, c["A"]), upload(engine, c["B"])
    d_a[0, cols:cols + b["wrap"]] = upload(engine, c["a_decoy"][:b["wrap"]])
    d_b[0, b["wrap"]:b["wrap"] + rows] = upload(engine, c["b_decoy"])
    res, _, _ = engine.batch_device(d_a, d_b, cols, rows, fc.LINEAR, out=(poison(engine, (n, 3)), None, None))
    assert engine.get_option("last_batch_kernel") != 0
    res = host(res)
    P8 = t.full((n, rows + 1, cols + 1), 0x5A, dtype=t.int8, device=dev_of(engine))
    res2, _, P, paths = engine.batch_device(d_a, d_b, cols, rows, fc.LINEAR, traceback=True, want_paths=True, out=(poison(engine, (n, 3)), None, P8),
                                            paths=poison(engine, (n, cols + rows + 2)))
    assert engine.get_option("last_batch_kernel") == 2                                # an int8 P alone, more than 512 columns: two pairs per wave
    res2, P, paths = host(res2), host(P), host(paths)
    for k in range(n):
        h, p, mp = truth[k]
        opath = oracle.backtrack(p, mp)
        assert tuple(res[k, :2]) == tuple(res2[k, :2]) == (mp, int(h.flat[mp])), f"pair {k}: {res[k]}, {res2[k]} vs {(mp, int(h.flat[mp]))}"
        assert res2[k, 2] == len(opath) and np.array_equal(paths[k, :len(opath)], opath), f"pair {k}: path"
        assert np.array_equal(P[k].astype(np.int32), p), f"pair {k}: P"
    del d_a, d_b


# ---- C. far internal workspaces ----

def test_profile_workspace_beyond_4gib(engine, checker):  # noqa: F811
    """8100 queries of 2049 letters under search_profile_mib = 6144: one group whose profiles take 6 394 982 400 bytes, so most
    queries' prof_off lies beyond 2^32.  Compared with the reference and with the same calls under the default budget."""
    t = engine.torch
    c, exp = fc.profile_case(), fc.profile_expected(checker)
    nq, which, scoring = fc.PROFILE_NQ, fc.profile_case()["which"], (fc.table24(), *fc.GAPS[0])
    want, u = exp["R"][which], exp["U"][which]
    d_q, d_db = upload(engine, c["qpacked"]), upload(engine, c["packed"])
    db = engine.prepare_db(d_db, c["offs"])
    all_pairs = np.stack([np.repeat(np.arange(nq), 2), np.tile(np.arange(2), nq)], axis=1).astype(np.int64)
    d_pairs = upload(engine, all_pairs)
    default = engine.get_option("search_profile_mib")
    assert default == 256
    try:
        got = {}
        for mib in (fc.PROFILE_MIB, default):
            with option(engine, "search_profile_mib", mib):
                for lanes in (32, 16):
                    with option(engine, "search_lanes", lanes):
                        got[(mib, "search", lanes)] = host(db.search_affine_device(d_q, c["qoffs"], scoring, out=poison(engine, nq * 2 * 3)))
                        groups, pk = engine.get_option("last_search_multi_groups"), engine.get_option("last_search_multi_packed_launches")
                        assert (groups == 1) if mib == fc.PROFILE_MIB else (groups > 20), (mib, groups)
                        assert pk == (engine.get_option("last_search_multi_launches") if lanes == 16 else 0)
                    same(got[(mib, "search", lanes)], want, f"search_profile_mib {mib} lanes {lanes}: sw_db_search_affine")
                pairs, npairs, scores = db.prefilter_ungapped_device(d_q, c["qoffs"], fc.table24(), 1, nq * 2, want_scores=True,
                                                                     out=(poison(engine, (nq * 2, 2)), poison(engine, 1), poison(engine, (nq, 2), t.int32)))
                same(host(scores), u.astype(np.int32), f"search_profile_mib {mib}: sw_db_prefilter_ungapped")
                assert (engine.get_option("last_prefilter_groups") == 1) == (mib == fc.PROFILE_MIB)
                pr = host(pairs)
                assert int(npairs.item()) == nq * 2 and np.array_equal(pr[np.lexsort((pr[:, 1], pr[:, 0]))], all_pairs)   # every U is positive
                res = host(db.search_affine_pairs_device(d_q, c["qoffs"], scoring, d_pairs, out=poison(engine, nq * 2 * 3)))
                assert (engine.get_option("last_search_pairs_groups") == 1) == (mib == fc.PROFILE_MIB)
                same(res.reshape(nq, 2, 3), want, f"search_profile_mib {mib}: sw_db_search_affine_pairs")
        assert got[(fc.PROFILE_MIB, "search", 16)].tobytes() == got[(default, "search", 16)].tobytes() == got[(default, "search", 32)].tobytes()
    finally:
        db.close()


def test_selection_chunk_beyond_4gib(engine, checker):  # noqa: F811
    """sw_db_search_affine_top over 2^24 targets and 12 queries: one chunk of 4.5 GiB under search_results_mib = 6144, six chunks of two
    rows under the default of 1024."""
    g = fc.GAPS[0]
    which = [k % fc.NQ for k in range(fc.BIG_NQ)]
    want = fc.expected(checker)["R"][g][which]
    B = BigDb(engine, which)
    default = engine.get_option("search_results_mib")
    assert default == 1024
    try:
        for top, min_score in ((5, 1), (16, 0)):
            wh, wn = fc.sparse_rank(want, top, min_score)
            got = {}
            for mib, lanes, chunks in ((6144, 32, 1), (6144, 16, 1), (default, 32, 6)):
                with option(engine, "search_results_mib", mib), option(engine, "search_lanes", lanes):
                    hits, nhits = B.db.search_affine_top_device(B.d_q, B.qoffs, (fc.table24(), *g), top, min_score,
                                                                out=(poison(engine, fc.BIG_NQ * top * 3), poison(engine, fc.BIG_NQ)))
                    got[(mib, lanes)] = (host(hits), host(nhits))
                    assert engine.get_option("last_search_top_chunks") == chunks, (mib, engine.get_option("last_search_top_chunks"))
                    assert (engine.get_option("last_search_multi_packed_launches") > 0) == (lanes == 16)
                same(got[(mib, lanes)][0], wh, f"search_results_mib {mib} lanes {lanes} top {top}: hits")
                same(got[(mib, lanes)][1], wn, f"search_results_mib {mib} lanes {lanes} top {top}: nhits")
            assert got[(6144, 32)][0].tobytes() == got[(default, 32)][0].tobytes() == got[(6144, 16)][0].tobytes()
    finally:
        B.close()


@pytest.fixture(scope="module")
def slot_plan(tmp_path_factory):
    """The hit-table alignment's plan as the library's own planner (csrc/sw_plan.cpp) gives it, through tests/align_ckpt_plan_driver.cpp,
    which drives the whole-matrix planner (mode 0) and the checkpointed one (mode 1)."""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the planner")
    exe = str(tmp_path_factory.mktemp("plan") / "align_ckpt_plan")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "align_ckpt_plan_driver.cpp"),
                    os.path.join(ROOT, "smith-waterman_amd", "csrc", "sw_plan.cpp")], check=True)

    def run(mode, forced, mib, per_cu):
        s = fc.SLOTS
        line = f"what=hits qlens={s['qlen']} longest={max(s['tlens'])} top={s['top']} num_cus=256 per_cu={per_cu},{per_cu},{per_cu} budget_bytes={mib * 2**20} mode={mode} forced={forced}"
        return json.loads(subprocess.run([exe], input=line + "\n", capture_output=True, text=True, check=True).stdout)
    return run


def plans_that_match(slot_plan, mode, forced, mib, slots, tiers):
    """The plans, over the occupancies a kernel can have, whose launches and slots are what the device reported: the test does not
    know the occupancy the library measured, the planner's answer for it is read back this way."""
    out = []
    for per_cu in range(1, 9):
        p = slot_plan(mode, forced, mib, per_cu)
        if p["fits"] and p["ckpt"] == mode and len(p["launch"]) == tiers and sum(x["slots"] for x in p["launch"]) == slots:
            out.append(p)
    return out


@pytest.mark.parametrize("checkpoint,rows", [(0, 0), (1, fc.SLOTS["checkpoint_rows"])], ids=["whole", "checkpointed_1024"])
def test_alignment_slots_beyond_4gib(engine, checker, slot_plan, checkpoint, rows):  # noqa: F811
    """2048 hits of about 1100 letters against one query of 2049 under align_workspace_mib = 8192: whole direction matrices, and slots of
    one band of 1024 rows and a checkpoint row.  The library's planner, asked here for the occupancy that reproduces the launches and
    slots the device reports, must say that the direction workspace passes 2^32 bytes (6 926 893 056 and 6 492 782 592 with the
    16-column kernel at two or more workgroups per CU), so the slots of the upper part lie beyond the line.  That a wave with such a
    slot took an item is SUPPOSED, not asserted: the waves of a launch draw their items from one counter, and with as many slots as
    entries every resident wave is expected to get one.  The same call under the default budget gets fewer slots and must write the
    same bytes; both are compared with the rule's walk over the checker's matrices."""
    t, s, g = engine.torch, fc.SLOTS, fc.GAPS[0]
    c, exp = fc.slots_case(), fc.slots_expected(checker)
    top, cap = s["top"], s["qlen"] + max(s["tlens"])
    p, offs = fc.packed(c["targets"], 3)
    d_q, d_db = upload(engine, c["query"]), upload(engine, np.concatenate([np.zeros(3, np.uint8), p]))
    hits = np.zeros((1, top, 3), np.int64)
    hits[0, :, 0] = np.arange(top) % 3
    d_hits = upload(engine, hits)
    default = engine.get_option("align_workspace_mib")
    assert default == 1024
    db = engine.prepare_db(d_db, offs)
    try:
        got = {}
        for mib in (s["workspace_mib"], default):
            with option(engine, "align_workspace_mib", mib), option(engine, "align_checkpoint_rows", rows):
                aln, ops = db.align_affine_hits_device(d_q, np.array([0, s["qlen"]], np.int64), (fc.table24(), *g), d_hits, None, ops_cap=cap,
                                                       out=(poison(engine, (top, 7)), poison(engine, (top, cap), t.uint8)), checkpoint=checkpoint)
                engine.synchronize()
                assert engine.get_option("last_align_hits_checkpointed") == checkpoint and engine.get_option("last_align_hits_band_rows") == rows
                slots, tiers = engine.get_option("last_align_hits_slots"), engine.get_option("last_align_hits_tiers")
            plans = plans_that_match(slot_plan, checkpoint, rows, mib, slots, tiers)
            print(f"align_workspace_mib {mib}: {slots} slots in {tiers} launches; dir_need {sorted({x['dir_need'] for x in plans})}")
            assert plans, f"align_workspace_mib {mib}: no occupancy gives {slots} slots in {tiers} launches"
            got[mib] = (host(aln).reshape(top, 7), host(ops).reshape(top, cap), slots, plans)
            same(got[mib][0], np.array([exp[k % 3][0] for k in range(top)], np.int64), f"align_workspace_mib {mib}: aln")
            same(got[mib][1], ops_rows([exp[k % 3][1] for k in range(top)], cap), f"align_workspace_mib {mib}: ops")
        far, near_ = got[s["workspace_mib"]], got[default]
        assert all(x["dir_need"] > 2**32 for x in far[3]), [x["dir_need"] for x in far[3]]
        assert all(max(l["slots"] * l["slot_bytes"] for l in x["launch"]) > 2**32 for x in far[3])    # one launch's slots x slot bytes, not a sum
        assert all(x["dir_need"] <= default * 2**20 for x in near_[3]) and near_[2] < far[2], (near_[2], far[2])
        assert far[0].tobytes() == near_[0].tobytes() and far[1].tobytes() == near_[1].tobytes()
    finally:
        db.close()
