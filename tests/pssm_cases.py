"""Shared by the PSSM tests (test_pssm_host.py, test_pssm_gpu.py, test_pssm_cli_gpu.py): position-specific matrices the independent
checker (tests/affine_oracle.cpp) can express.  The checker scores a cell through a 256 x 256 table indexed by the query's byte, so a
PSSM with at most 256 distinct columns goes to it as the "query" whose byte j names the TYPE of column j and the table
sub[type][x] = s(type, x); longer queries draw their columns from 256 random types.  The table is built here, in numpy, from the rule
in include/swhip.h -- min(entry, smax) for a listed byte, `other` for every other byte -- and shares no code with the library."""
import numpy as np

from affine_cases import PROTEIN, database

# query lengths in one call: all three classes of columns per lane (<= 256, <= 512, longer), both sides of each class edge and of each
# padding edge, and 1300: a second strip at 16 columns per lane
QLENS = [1, 63, 64, 65, 255, 256, 257, 300, 512, 513, 1025, 1300]
NLETTERS = [1, 4, 24, 255, 256]
QFRONT = 3                         # qoffsets[0]: unused columns in front of the first query


def letters_of(rng, n):
    """n distinct target bytes: protein letters first (the databases are drawn from those), then random other bytes.  The last protein
    letter joins only as the 256th byte: below 256 letters a protein database always holds a byte that scores `other`, and n = 255
    leaves out exactly that one."""
    if n < len(PROTEIN):
        return PROTEIN[:n].copy()
    rest = np.setdiff1d(np.arange(256, dtype=np.uint8), PROTEIN)
    return np.concatenate([PROTEIN[:-1], rng.permutation(rest)[:n - len(PROTEIN) + 1], PROTEIN[-1:]])[:n].astype(np.uint8)


class Typed:
    """256 random column types over `letters`, queries that name types, and both views of them: the column-major matrix the library
    takes and the (type string, table) pair the checker takes."""

    def __init__(self, rng, letters, other, smax, qlens, lo=-8, hi=12, front=QFRONT):
        self.letters, self.other, self.smax = np.asarray(letters, np.uint8), int(other), int(smax)
        n = len(self.letters)
        self.types = rng.integers(lo, hi + 1, (256, n)).astype(np.int8)
        self.types[:, 0] = rng.integers(max(lo, 4), hi + 1, 256).astype(np.int8)         # something to align with in every column
        self.qoffs = np.zeros(len(qlens) + 1, np.int64)
        self.qoffs[0] = front
        self.qoffs[1:] = front + np.cumsum(qlens)
        self.names = rng.integers(0, 256, int(self.qoffs[-1])).astype(np.uint8)          # the type of every column, the unused ones too
        self.table = np.full((256, 256), self.other, np.int8)                            # the checker's view
        self.table[:, self.letters] = np.minimum(self.types, self.smax)

    @property
    def matrix(self):
        """(qoffsets[nqueries], nletters) int8: row g is column g, the `front` unused columns included."""
        return self.types[self.names]

    def query(self, q):
        """The checker's "query" of query q: one type byte per column."""
        return self.names[self.qoffs[q]:self.qoffs[q + 1]]

    def scoring(self, go, ge):
        return (self.letters, self.other, self.smax, go, ge)

    def expected(self, checker, packed, offs, go, ge):
        """(nqueries, ntargets, 3) from the checker, query by query."""
        return np.stack([checker.search(self.query(q), packed, offs, self.table, go, ge) for q in range(len(self.qoffs) - 1)])


def small_database(rng, alpha, budget=2.5e6):
    """affine_cases.database -- empty, 1-letter and lane-edge targets, an odd offsets[0] -- with a budget that keeps a call of QLENS
    (5111 columns) to a few hundred million cells."""
    return database(rng, max(QLENS), alpha, budget=budget)


def rank_order(res, top, min_score):
    """(hits (nq, top, 3), nhits (nq,)) in the rank order of include/swhip.h, computed in numpy from a full (nq, ntargets, 3) table."""
    nq, nt, _ = res.shape
    hits = np.zeros((nq, top, 3), np.int64)
    hits[:, :, 0] = -1
    nhits = np.zeros(nq, np.int64)
    for q in range(nq):
        order = np.lexsort((np.arange(nt), -res[q, :, 1]))
        order = order[res[q, order, 1] >= min_score][:top]
        nhits[q] = len(order)
        hits[q, :len(order), 0] = order
        hits[q, :len(order), 1] = res[q, order, 0]
        hits[q, :len(order), 2] = res[q, order, 1]
    return hits, nhits


def write_ascii_pssm(path, letters, matrix, consensus, tail=True):
    """A file in the layout PSI-BLAST writes: a title, the alphabet printed twice, one line per column (position, residue, the scores,
    the percentages, two floats), a blank line and the statistics."""
    hdr = "   ".join(chr(x) for x in letters)
    lines = ["", "Last position-specific scoring matrix computed, weighted observed percentages rounded down, information per position",
             "            " + hdr + "   " + hdr]
    for g, row in enumerate(matrix):
        lines.append(f"{g + 1:5d} {chr(consensus[g])}   " + " ".join(f"{int(v):3d}" for v in row) + "   " + " ".join("  0" for _ in row) + "  0.55 0.12")
    if tail:
        lines += ["", "                      K         Lambda", "Standard Ungapped    0.1350     0.3166"]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
