"""The search statistics restated in numpy from the rules of include/swhip.h -- the half-octave length class, the score bin, the
histogram, the fit, the E-value and the thresholds -- and the hand-made tables the host and GPU tests share.  Nothing here calls the
library."""
import math

import numpy as np

CLASSES, BINS, CELLS = 40, 256, 40 * 256
GUARD = 64
P32, P64 = 0x55555555, 0x5555555555555555
GAMMA = 0.57721566490153286061
SHIFTS = (0, 3, 16)
SCORES = (0, 1, 254, 255, 256, (1 << 24) - 1, -1, -(1 << 40))


def length_class(L):
    """class(1) = 0; for L >= 2 with e = floor(log2 L): 2 e + ((L >> (e - 1)) & 1)."""
    if L < 2:
        return 0
    e = L.bit_length() - 1
    return 2 * e + ((L >> (e - 1)) & 1)


def score_bin(v, shift):
    return min(max(int(v), 0) >> shift, 255)


def edge_lengths():
    """Both sides of every class edge below 2^20: 1 .. 8, then 3 x 2^(k-1) - 1, 3 x 2^(k-1), 2^(k+1) - 1, 2^(k+1) for k = 3 .. 19."""
    ls = [1, 2, 3, 4, 5, 6, 7, 8]
    for k in range(3, 20):
        ls += [3 * (1 << (k - 1)) - 1, 3 * (1 << (k - 1)), (1 << (k + 1)) - 1, 1 << (k + 1)]
    return [x for x in ls if x < (1 << 20)]


def offsets_of(lengths, first=0):
    offs = np.zeros(len(lengths) + 1, np.int64)
    offs[0] = first
    offs[1:] = first + np.cumsum(np.asarray(lengths, np.int64))
    return offs


def table(scores):
    """(nq, ntargets) scores -> the (nq, ntargets, 3) result table; max_pos and path_len carry bytes the histogram must not read."""
    scores = np.asarray(scores, np.int64)
    res = np.empty(scores.shape + (3,), np.int64)
    res[..., 0] = 0x1111111111111111
    res[..., 1] = scores
    res[..., 2] = -7
    return res


def hist_ref(res, offs, shift):
    nq, nt = res.shape[:2]
    h = np.zeros((nq, CLASSES, BINS), np.uint32)
    lens = np.diff(offs)
    for k in range(nt):
        L = int(lens[k])
        if L < 1:
            continue
        c = length_class(L)
        for q in range(nq):
            h[q, c, score_bin(res[q, k, 1], shift)] += 1
    return h


def edge_case(shift, nq=3, seed=0):
    """Every edge length (and empty targets between them) against the edge scores, rotated per query so that every (length, score)
    pair occurs."""
    rng = np.random.default_rng(seed)
    lens = []
    for L in edge_lengths():
        lens += [L, 0] if L % 3 == 0 else [L]
    # offsets only: the lengths sum to ~10^7, nothing is allocated for them
    offs = offsets_of(lens, first=5)
    nt = len(lens)
    sc = np.empty((nq, nt), np.int64)
    for q in range(nq):
        for k in range(nt):
            sc[q, k] = SCORES[(k + q) % len(SCORES)] if (k + q) % 11 else int(rng.integers(0, 256 << shift))
    return table(sc), offs


def fit_ref(hist, shift):
    """One query's (40, 256) histogram -> dict(a, b, sigma, n_db, n_fit, n_censored, valid) and the list of the four rounds' (a, b, sigma)."""
    h = np.asarray(hist, np.float64)
    x = np.repeat(np.arange(CLASSES, dtype=np.float64)[:, None], BINS - 1, axis=1)
    y = np.repeat((np.arange(BINS - 1, dtype=np.float64) * 2.0 ** shift + (2.0 ** shift - 1) / 2)[None, :], CLASSES, axis=0)
    full = h[:, :BINS - 1]
    rounds = []
    a = b = sigma = W = 0.0
    for rnd in range(4):
        w = full.copy()
        if rnd and sigma > 0:
            z = (y - a - b * x) / sigma
            w[(z > 5) | (z < -4)] = 0
        W = w.sum()
        if W > 0:
            mx, my = (w * x).sum() / W, (w * y).sum() / W
            den = (w * (x - mx) ** 2).sum()
            b = (w * (x - mx) * (y - my)).sum() / den if den > 0 else 0.0
            a = my - b * mx
            sigma = math.sqrt((w * (y - a - b * x) ** 2).sum() / (W - 2)) if W > 2 else 0.0
        else:
            a = b = sigma = 0.0
        rounds.append((a, b, sigma))
    return dict(a=a, b=b, sigma=sigma, n_db=int(np.asarray(hist, np.int64).sum()), n_fit=int(W), n_censored=int(np.asarray(hist, np.int64)[:, 255].sum()),
                valid=int(W >= 30 and sigma > 0)), rounds


def evalue_ref(f, L, score):
    if not f["valid"]:
        return math.nan
    z = (score - f["a"] - f["b"] * length_class(L)) / f["sigma"]
    return f["n_db"] * -math.expm1(-math.exp(-math.pi / math.sqrt(6) * z - GAMMA))


def thresholds_ref(f, evalue):
    if not f["valid"] or evalue >= f["n_db"]:
        return np.zeros(CLASSES, np.int64)
    z0 = -(math.sqrt(6) / math.pi) * (math.log(-math.log1p(-evalue / f["n_db"])) + GAMMA)
    return np.array([math.ceil(f["a"] + f["b"] * c + f["sigma"] * z0) for c in range(CLASSES)], np.int64)


def null_hist(seed, n=4000, planted=0, planted_score=200):
    """A histogram as a null database gives it: n targets of log-normal length (median 150, sigma 0.6, 20..800), scores Gumbel around
    a line of slope 1.1 per half octave with sigma 3.8 (beta = sigma sqrt 6 / pi), plus `planted` targets of planted_score."""
    rng = np.random.default_rng(seed)
    lens = np.clip(np.exp(rng.normal(math.log(150), 0.6, n)).astype(np.int64), 20, 800)
    cls = np.array([length_class(int(L)) for L in lens])
    beta = 3.8 * math.sqrt(6) / math.pi
    sc = np.maximum(0, np.rint(20 + 1.1 * cls + rng.gumbel(-GAMMA * beta, beta, n))).astype(np.int64)
    h = np.zeros((CLASSES, BINS), np.uint32)
    np.add.at(h, (cls, np.minimum(sc, 255)), 1)
    if planted:
        pc = cls[:planted]
        np.add.at(h, (pc, np.full(planted, min(planted_score, 255))), 1)
    return h


def hits_case(seed, nq, top, ntargets=300):
    """A hit table around its thresholds: targets of every kind (in range, -1, >= ntargets, empty), scores at threshold - 1, threshold
    and threshold + 1, counts below, at and above top and negative.  Returns (offsets, thresholds, hits, nhits)."""
    rng = np.random.default_rng(seed)
    lens = rng.choice(np.array(edge_lengths()[:40] + [0, 0, 0], np.int64), ntargets)
    lens[:3] = (0, 1, 37)
    offs = offsets_of(lens, first=3)
    thr = rng.integers(5, 60, (nq, CLASSES)).astype(np.int64)
    hits = np.zeros((nq, top, 3), np.int64)
    tg = rng.integers(0, ntargets, (nq, top))
    kind = rng.integers(0, 12, (nq, top))
    tg = np.where(kind == 0, -1, np.where(kind == 1, ntargets, np.where(kind == 2, ntargets + (1 << 40), np.where(kind == 3, -(1 << 33), tg))))
    hits[..., 0] = tg
    hits[..., 1] = rng.integers(0, 1 << 40, (nq, top))
    for q in range(nq):
        for r in range(top):
            t = int(tg[q, r])
            L = int(lens[t]) if 0 <= t < ntargets else 1
            hits[q, r, 2] = thr[q, length_class(max(L, 1))] + int(rng.integers(-1, 2))
    nhits = rng.integers(0, top + 1, nq).astype(np.int64)
    nhits[0] = top
    if nq > 1:
        nhits[1] = top + 5
    if nq > 2:
        nhits[2] = -3
    if nq > 3:
        nhits[3] = 0
    return offs, thr, hits, nhits


def threshold_ref(offs, thr, hits, nhits):
    nq, top = hits.shape[:2]
    nt = len(offs) - 1
    keep = np.zeros((nq, top), np.int32)
    for q in range(nq):
        n = top if nhits is None else min(max(int(nhits[q]), 0), top)
        for r in range(n):
            t = int(hits[q, r, 0])
            if 0 <= t < nt:
                L = int(offs[t + 1] - offs[t])
                if L >= 1 and hits[q, r, 2] >= thr[q, length_class(L)]:
                    keep[q, r] = 1
    out = hits.copy()
    out[..., 0] = np.where(keep == 1, hits[..., 0], -1)
    return keep, keep.sum(axis=1).astype(np.int64), out
