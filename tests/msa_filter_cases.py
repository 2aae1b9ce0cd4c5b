"""Column rows for the tests of the alignment filter (sw_msa_filter_device / sw_msa_filter_host): a restatement of the rule of
include/swhip.h in numpy, seeded families of rows that the filter thins to between a tenth and nine tenths, and the greedy chain laid
across row blocks.  No GPU, no library call but in reference()'s callers."""
from dataclasses import dataclass

import numpy as np

DASH = 0x2D
GUARD, POISON = 64, 0xA5


@dataclass
class Case:
    cols: np.ndarray        # uint8, query q's (top, qlen) rows at (qoffs[q] - qoffs[0]) * top
    qpacked: np.ndarray     # uint8, query q's letters at qoffs[q] (the bytes below qoffs[0] are never read)
    qoffs: np.ndarray       # int64
    top: int
    hits: np.ndarray        # (nq, top, 3) int64

    @property
    def nq(self):
        return len(self.qoffs) - 1

    def rows(self, q):
        g0, qlen = int(self.qoffs[q]), int(self.qoffs[q + 1] - self.qoffs[q])
        base = (g0 - int(self.qoffs[0])) * self.top
        return self.cols[base:base + self.top * qlen].reshape(self.top, qlen)


def reference(c: Case, max_ident_pct: int, min_cover_pct: int, with_query: bool = True):
    """The rule, restated: (keep (nq, top) int32, nkept (nq,) int64, hits with target = -1 where dropped)."""
    keep = np.zeros((c.nq, c.top), np.int32)
    for q in range(c.nq):
        rows = c.rows(q)
        qlen = rows.shape[1]
        letter = rows != DASH
        n = letter.sum(axis=1)
        query = c.qpacked[int(c.qoffs[q]):int(c.qoffs[q + 1])]
        kept = []
        for r in range(c.top):
            ok = n[r] >= 1 and 100 * n[r] >= min_cover_pct * qlen
            if ok and with_query:
                ok = 100 * int((letter[r] & (rows[r] == query)).sum()) < max_ident_pct * n[r]
            if ok and kept:
                same = (letter[r][None, :] & (rows[kept] == rows[r][None, :])).sum(axis=1)
                ok = bool((100 * same < max_ident_pct * n[r]).all())
            if ok:
                kept.append(r)
        keep[q, kept] = 1
    hits = c.hits.copy()
    hits[..., 0][keep == 0] = -1
    return keep, keep.sum(axis=1).astype(np.int64), hits


def _hits(rng, nq, top):
    h = rng.integers(0, 1 << 20, (nq, top, 3)).astype(np.int64)
    h[..., 0] = rng.integers(0, 5000, (nq, top))
    return h


def families(seed: int, top: int, qlens, q0: int = 0) -> Case:
    """Per query a few family centres -- the first is the query itself, so self-hits occur -- and `top` rows that are a centre with
    0 / 3 / 30 / 60 percent of its bytes redrawn, some cut to a part of the columns, a few without a letter.  Bytes from all 256 values
    (0x00, 0x2D and 0xFF among them); queries of fewer than 8 columns draw from six, or every row would be unique."""
    rng = np.random.default_rng(seed)
    qoffs = (q0 + np.concatenate([[0], np.cumsum(qlens)])).astype(np.int64)
    qpacked = rng.integers(0, 256, int(qoffs[-1])).astype(np.uint8)
    out = []
    for q, qlen in enumerate(qlens):
        alphabet = np.arange(256, dtype=np.uint8) if qlen >= 8 else np.array([0x00, DASH, 0xFF, 65, 66, 200], np.uint8)
        nfam = 2 + top // 8
        centres = alphabet[rng.integers(0, len(alphabet), (nfam, qlen))]
        if qlen < 8:
            qpacked[int(qoffs[q]):int(qoffs[q + 1])] = centres[0]
        else:
            centres[0] = qpacked[int(qoffs[q]):int(qoffs[q + 1])]
        rows = centres[rng.integers(0, nfam, top)].copy()
        p = rng.choice([0.0, 0.03, 0.3, 0.6], top)
        redraw = rng.random((top, qlen)) < p[:, None]
        rows[redraw] = alphabet[rng.integers(0, len(alphabet), int(redraw.sum()))]
        for r in np.flatnonzero(rng.random(top) < 0.4):                       # a part of the columns only
            a = int(rng.integers(0, qlen))
            b = int(rng.integers(a, qlen + 1))
            rows[r, :a] = DASH
            rows[r, b:] = DASH
        rows[rng.random(top) < 0.05] = DASH
        out.append(rows.reshape(-1))
    return Case(np.concatenate(out), qpacked, qoffs, top, _hits(rng, len(qlens), top))


def chain_rows(qlen: int = 100):
    """A; B, 90 percent of A; C, 90 percent of B and 80 percent of A: at max_ident_pct 90, B falls to A and C stays."""
    a = np.full(qlen, ord("A"), np.uint8)
    b = a.copy(); b[:qlen // 10] = ord("B")
    c = b.copy(); c[qlen // 10:2 * (qlen // 10)] = ord("C")
    return a, b, c


def chain_case(places, top: int, qlen: int = 100) -> Case:
    """One query whose rows are all '-' but the chain A, B, C at the three `places`; the query is unlike all of them."""
    rows = np.full((top, qlen), DASH, np.uint8)
    for r, row in zip(places, chain_rows(qlen)):
        rows[r] = row
    rng = np.random.default_rng(top)
    return Case(rows.reshape(-1), np.full(qlen, ord("Q"), np.uint8), np.array([0, qlen], np.int64), top, _hits(rng, 1, top))
