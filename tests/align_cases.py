"""Shared by the alignment tests (test_align_affine_host.py, test_align_affine_gpu.py): the walk of the canonical alignment
(include/swhip.h) over the checker's whole H, E, F, written from the rule alone, and the rule-independent replay of a set of ops over the
letters.  Nothing here shares code with the library; both are O(path length)."""
import numpy as np

from affine_cases import PROTEIN


def walk(H, E, F, query, target, submat, go, ge, max_pos):
    """(ops in alignment order as bytes, (t_begin, q_begin), H-state cells as linear indices in walk order) from max_pos."""
    M = len(query) + 1
    i, j = divmod(int(max_pos), M)
    ops, cells, state = [], [], "H"
    while True:
        if state == "H":
            if H[i, j] == 0:
                break
            cells.append(i * M + j)
            if H[i, j] == H[i - 1, j - 1] + int(submat[query[j - 1], target[i - 1]]):
                ops.append("M")
                i, j = i - 1, j - 1
            elif H[i, j] == E[i, j]:
                state = "E"
            else:
                assert H[i, j] == F[i, j]
                state = "F"
        elif state == "E":
            ops.append("D")
            if E[i, j] == H[i - 1, j] + go + ge:
                state = "H"
            i -= 1
        else:
            ops.append("I")
            if F[i, j] == H[i, j - 1] + go + ge:
                state = "H"
            j -= 1
    return "".join(reversed(ops)).encode(), (i, j), cells


def expected(checker, query, target, submat, go, ge):
    """The sw_alignment row and the ops the rule gives for one pair, from the checker's matrices."""
    s, p, H, E, F = checker.matrices(query, target, submat, go, ge)
    if s == 0:
        return (0, 0, 0, 0, 0, 0, 0), b"", []
    ops, (i0, j0), cells = walk(H, E, F, query, target, submat, go, ge, p)
    i1, j1 = divmod(p, len(query) + 1)
    return (p, s, j0, i0, j1, i1, len(ops)), ops, cells


def replay(query, target, submat, go, ge, aln_row, ops):
    """Rule-independent: the ops, replayed over the letters from (t_begin, q_begin), end at (t_end, q_end) = divmod(max_pos, qlen + 1),
    re-score to exactly max_score (table entries, go + k ge per gap run) and begin and end with M."""
    max_pos, max_score, qb, tb, qe, te, nops = (int(x) for x in aln_row)
    assert nops == len(ops)
    if max_score == 0:
        assert (max_pos, qb, tb, qe, te, nops) == (0, 0, 0, 0, 0, 0)
        return
    assert ops[:1] == b"M" and ops[-1:] == b"M", ops
    assert set(ops) <= set(b"MID")
    i, j, score, prev = tb, qb, 0, None
    for op in ops:
        if op == ord("M"):
            score += int(submat[query[j], target[i]])
            i, j = i + 1, j + 1
        else:
            score += ge + (go if op != prev else 0)
            if op == ord("D"):
                i += 1
            else:
                j += 1
        prev = op
    assert (i, j) == (te, qe) == divmod(max_pos, len(query) + 1)
    assert score == max_score, (score, max_score)


def h_cells(aln_row, ops, qlen, go_is_zero=True):
    """The linear indices of the cells the walk visits in state H, in walk order (end to begin), implied by the ops.  A gap run is left
    for state H where it opens: with gap_open = 0 every gap step opens (a tie opens), so every op stands for one H cell."""
    assert go_is_zero
    M = qlen + 1
    i, j = int(aln_row[5]), int(aln_row[4])
    cells = []
    for op in reversed(bytes(ops)):
        cells.append(i * M + j)
        if op == ord("M"):
            i, j = i - 1, j - 1
        elif op == ord("D"):
            i -= 1
        else:
            j -= 1
    return cells


def pack(targets):
    offs = np.zeros(len(targets) + 1, np.int64)
    offs[1:] = np.cumsum([len(t) for t in targets])
    packed = np.concatenate([np.asarray(t, np.uint8) for t in targets]) if offs[-1] else np.zeros(0, np.uint8)
    return packed.astype(np.uint8), offs


def _crisp_submat(swamd, rng):
    """Matches 5..9, mismatches -4..-1 over the protein letters (tests/test_search_affine_gpu.py)."""
    n = len(PROTEIN)
    sc = rng.integers(-4, 0, (n, n)).astype(np.int8)
    sc[np.arange(n), np.arange(n)] = rng.integers(5, 10, n).astype(np.int8)
    return swamd.submat_from_letters(PROTEIN, sc, -4)


def indel_cases(swamd, rng, query, B, span=200):
    """The indel targets of test_indels_open_gaps_across_strip_boundaries around column B: (target, expected ops, expected score)."""
    sub = _crisp_submat(swamd, rng)
    go, ge = -8, -1
    diag = lambda seq: int(sum(int(sub[x, x]) for x in seq))  # noqa: E731
    cases = []
    for d in (1, 5, 15):       # a run of 2d query letters missing from the target: I x 2d after span - d pairs
        t = np.concatenate([query[B - span:B - d], query[B + d:B + span]])
        cases.append((t, b"M" * (span - d) + b"I" * (2 * d) + b"M" * (span - d), diag(t) + go + 2 * d * ge))
    for n in (1, 15, 30):      # a run of n foreign letters inserted into the target: D x n after span pairs
        t = np.concatenate([query[B - span:B], rng.choice(PROTEIN[20:], n).astype(np.uint8), query[B:B + span]])
        cases.append((t, b"M" * span + b"D" * n + b"M" * span, diag(t[:span]) + diag(t[span + n:]) + go + n * ge))
    return sub, go, ge, cases
