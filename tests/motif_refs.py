"""TEST INFRASTRUCTURE: the brute-force restatement of the motif arithmetic, independent of
muon_amd/_atac/motifs.py: log-odds, the threshold by the dynamic programme, the same tail by enumerating all 4^L
words (matrices of up to 8 columns), and the scan as a numpy sliding window, j-ascending in f64: ``scan`` sequence by
sequence with the hits appended one at a time (small fixtures), ``scan_stream`` over a whole code stream at once (the
streams of tests/test_gpu_motif_edges.py, up to a few hundred thousand positions)."""
import itertools
import math

import numpy as np

LETTER = {"A": 0, "C": 1, "G": 2, "T": 3, "a": 0, "c": 1, "g": 2, "t": 3}


def read_counts(path):
    rows = []
    with open(path) as f:
        for line in f:
            if line.strip() and not line.startswith(">"):
                rows.append([float(x) for x in line.split()])
    assert len(rows) == 4
    return np.array(rows, dtype=np.float64)


def log_odds(counts, bg=(0.25, 0.25, 0.25, 0.25), ps=1e-4):
    c = np.asarray(counts, dtype=np.float64)
    M = np.empty_like(c)
    for j in range(c.shape[1]):
        tot = c[:, j].sum()
        for b in range(4):
            M[b, j] = math.log((c[b, j] + ps * bg[b]) / (tot + ps)) - math.log(bg[b])
    return M


def rounded(M, precision=1000.0):
    """round half away from zero, as Python integers in an int64 array"""
    S = np.empty(M.shape, dtype=np.int64)
    for idx, v in np.ndenumerate(M):
        x = precision * float(v)
        S[idx] = int(math.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)
    return S


def dp_tails(M, bg=(0.25, 0.25, 0.25, 0.25), precision=1000.0):
    """(tail[i] = P(total >= lowest + i) summed from the largest total downwards, lowest, highest)"""
    S = rounded(M, precision)
    lowest = int(S.min(axis=0).sum())
    highest = int(S.max(axis=0).sum())
    dist = np.zeros(highest - lowest + 1)
    dist[0] = 1.0
    reach = 1  # entries of dist in use
    for j in range(S.shape[1]):
        lo, hi = int(S[:, j].min()), int(S[:, j].max())
        new = np.zeros_like(dist)
        for b in range(4):  # A, C, G, T
            o = int(S[b, j]) - lo
            new[o:o + reach] += bg[b] * dist[:reach]
        reach += hi - lo
        dist = new
    assert reach == dist.size
    tail = np.cumsum(dist[::-1])[::-1]
    return tail, lowest, highest


def dp_total(M, pvalue, bg=(0.25, 0.25, 0.25, 0.25), precision=1000.0):
    """T: the smallest integer total with P(total >= T) <= pvalue; highest + 1 when there is none"""
    tail, lowest, highest = dp_tails(M, bg, precision)
    T = highest + 1
    while T - 1 >= lowest and tail[T - 1 - lowest] <= pvalue:
        T -= 1
    return T


def threshold(M, pvalue, bg=(0.25, 0.25, 0.25, 0.25), precision=1000.0):
    return dp_total(M, pvalue, bg, precision) / precision


def scan_threshold(M, pvalue, bg=(0.25, 0.25, 0.25, 0.25), precision=1000.0):
    """what a scan compares with: the threshold, or +inf where T is the largest total + 1 (the motif cannot hit)"""
    T = dp_total(M, pvalue, bg, precision)
    return T / precision if T <= int(rounded(M, precision).max(axis=0).sum()) else math.inf


def enumerated_tail(M, T, bg=(0.25, 0.25, 0.25, 0.25), precision=1000.0):
    """P(total >= T) over all 4^L words of the integer matrix (L <= 8)"""
    S = rounded(M, precision)
    L = S.shape[1]
    assert L <= 8
    p = 0.0
    for word in itertools.product(range(4), repeat=L):
        if sum(int(S[b, j]) for j, b in enumerate(word)) >= T:
            p += math.prod(bg[b] for b in word)
    return p


def enumerated_tails(M, totals, bg=(0.25, 0.25, 0.25, 0.25), precision=1000.0):
    """``enumerated_tail`` for several T at once (the words' totals and probabilities as arrays, summed per T)"""
    S = rounded(M, precision)
    L = S.shape[1]
    assert L <= 8
    tot = np.zeros(1, dtype=np.int64)
    pr = np.ones(1)
    for j in range(L):
        tot = (tot[:, None] + S[None, :, j]).reshape(-1)
        pr = (pr[:, None] * np.asarray(bg)[None, :]).reshape(-1)
    return [float(pr[tot >= T].sum()) for T in totals]


def encode(seq):
    return np.array([LETTER.get(ch, 4) for ch in seq], dtype=np.int64)


def scan(sequences, matrices, thresholds):
    """(rows [(sequence index, motif index, position, score)] in the reference's loop order, the smallest
    |score - threshold| over every admissible window)"""
    rows, margin = [], np.inf
    for si, seq in enumerate(sequences):
        codes = encode(seq)
        for mi, M in enumerate(matrices):
            L = M.shape[1]
            n = codes.size - L + 1
            if n <= 0:
                continue
            M5 = np.vstack([M, np.zeros((1, L))])
            score = np.zeros(n)
            ok = np.ones(n, dtype=bool)
            for j in range(L):
                w = codes[j:j + n]
                score = score + M5[w, j]
                ok &= w < 4
            if ok.any():
                margin = min(margin, float(np.min(np.abs(score[ok] - thresholds[mi]))))
            for pos in np.nonzero(ok & (score >= thresholds[mi]))[0]:
                rows.append((si, mi, int(pos), float(score[pos])))
    return rows, margin


def stream_room(codes, offsets):
    """int64 per stream position: the distance to the next code >= 4 or to the end of its sequence, whichever comes
    first (0 at an invalid code), uncapped.  A plain loop over the runs of valid codes of every sequence."""
    codes = np.asarray(codes)
    offsets = np.asarray(offsets, dtype=np.int64)
    room = np.zeros(codes.size, dtype=np.int64)
    for s in range(offsets.size - 1):
        a, b = int(offsets[s]), int(offsets[s + 1])
        stops = np.append(a + np.flatnonzero(codes[a:b] >= 4), b)  # where a run ends: an invalid code or the end
        first = a
        for stop in stops.tolist():
            room[first:stop] = np.arange(stop - first, 0, -1)
            first = stop + 1
    return room


def stream_scores(codes, room, M):
    """(score f64 [total - L + 1], admissible bool) of one motif at every stream position that leaves it L codes: the
    j-ascending sliding-window sum (an invalid code adds 0), admissible iff the room holds the motif"""
    L = M.shape[1]
    n = codes.size - L + 1
    if n <= 0:
        return np.zeros(0), np.zeros(0, dtype=bool)
    M5 = np.vstack([np.asarray(M, dtype=np.float64), np.zeros((1, L))])
    score = np.zeros(n)
    for j in range(L):
        score = score + M5[:, j].take(codes[j:j + n])
    return score, room[:n] >= L


def scan_stream(codes, offsets, matrices, thresholds):
    """The scan of a whole code stream (0..3 = A C G T, anything else invalid; ``offsets`` int64 [n + 1]) at once:
    for every motif the j-ascending f64 sliding-window sum over the stream, a window admissible iff the room at its
    first position holds the motif.  Returns the hits as arrays ``(sequence int64, motif int64, position int64, score
    f64)`` in the reference's loop order: sequence, motif, position."""
    codes = np.minimum(np.asarray(codes), 4).astype(np.intp)
    offsets = np.asarray(offsets, dtype=np.int64)
    room = stream_room(codes, offsets)
    gpos, mot, sc = [], [], []
    for mi, M in enumerate(matrices):
        score, ok = stream_scores(codes, room, M)
        hit = np.flatnonzero(ok & (score >= thresholds[mi]))
        gpos.append(hit)
        mot.append(np.full(hit.size, mi, dtype=np.int64))
        sc.append(score[hit])
    if not gpos:
        e = np.zeros(0, dtype=np.int64)
        return e, e.copy(), e.copy(), np.zeros(0)
    gpos, mot, sc = np.concatenate(gpos), np.concatenate(mot), np.concatenate(sc)
    seq = np.searchsorted(offsets, gpos, side="right") - 1  # (empty sequences own no position)
    order = np.lexsort((gpos, mot, seq))
    return seq[order], mot[order], (gpos - offsets[seq])[order], sc[order]
