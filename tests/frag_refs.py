"""TEST INFRASTRUCTURE: the fragment passes of csrc/fragments.hip stated in plain numpy, independent of
muon_amd/_atac/fragments.py: brute force over the (window x fragment) matrix instead of candidate ranges, chunks and
slots.  A fragment table is five integer columns in file order (``chrom`` the contig's code, grouped; ``start``
ascending inside a contig); a window is (contig code, lo, hi); ``cell_of`` maps a barcode code to a row.

A pair (window, fragment) PASSES when the fragment lies on the window's contig, ``end > max(lo, 0)``, ``start < hi``,
its barcode is a valid code and ``0 <= cell_of[barcode] < n_obs``.  All arithmetic is integer."""
import numpy as np

BLOCK = 2048  # windows per slice of the (window x fragment) matrix


def _i64(*arrays):
    return [np.asarray(a).astype(np.int64) for a in arrays]


def cells(barcode, cell_of, n_obs):
    """int64 per fragment: its row, -1 where the barcode is no code of ``cell_of`` or the entry is no row"""
    barcode, cell_of = _i64(barcode, cell_of)
    known = (barcode >= 0) & (barcode < cell_of.size)
    cell = np.full(barcode.size, -1, dtype=np.int64)
    cell[known] = cell_of[barcode[known]]
    cell[(cell < 0) | (cell >= int(n_obs))] = -1
    return cell


def range_lengths(chrom, start, wchrom, wlo, whi, max_len):
    """int64 per window: the candidates, fragments of its contig with ``start > max(lo, 0) - max_len`` and
    ``start < hi`` (0 on a contig the table lacks)"""
    chrom, start, wchrom, wlo, whi = _i64(chrom, start, wchrom, wlo, whi)
    out = np.zeros(wchrom.size, dtype=np.int64)
    for a in range(0, wchrom.size, BLOCK):
        s = slice(a, a + BLOCK)
        lo = np.maximum(wlo[s], 0)[:, None]
        m = (chrom[None, :] == wchrom[s][:, None]) & (start[None, :] > lo - int(max_len)) & (start[None, :] < whi[s][:, None])
        out[s] = m.sum(axis=1)
    return out


def pairs(chrom, start, end, barcode, cell_of, n_obs, wchrom, wlo, whi):
    """(window, fragment, cell) of the passing pairs in window order, then file order"""
    chrom, start, end, wchrom, wlo, whi = _i64(chrom, start, end, wchrom, wlo, whi)
    cell = cells(barcode, cell_of, n_obs)
    ws, ps = [], []
    for a in range(0, wchrom.size, BLOCK):
        s = slice(a, a + BLOCK)
        lo = np.maximum(wlo[s], 0)[:, None]
        m = ((chrom[None, :] == wchrom[s][:, None]) & (end[None, :] > lo) & (start[None, :] < whi[s][:, None])
             & (cell[None, :] >= 0))
        w, p = np.nonzero(m)  # row-major: window, then fragment
        ws.append(w + a)
        ps.append(p)
    w = np.concatenate(ws) if ws else np.zeros(0, dtype=np.int64)
    p = np.concatenate(ps) if ps else np.zeros(0, dtype=np.int64)
    return w, p, cell[p]


def overlap(chrom, start, end, barcode, score, cell_of, n_obs, wchrom, wlo, whi, n_features):
    """(keys int64, values int32): key = cell * n_features + window, value = the fragment's score (``score`` None: 1)"""
    w, p, cell = pairs(chrom, start, end, barcode, cell_of, n_obs, wchrom, wlo, whi)
    vals = np.ones(p.size, dtype=np.int32) if score is None else np.asarray(score).astype(np.int32)[p]
    return cell * int(n_features) + w, vals


def pileup_diff(chrom, start, end, barcode, score, cell_of, n_obs, wchrom, wlo, whi, width):
    """int32 [n_obs, width + 1]: every passing pair adds its score at the fragment's first column of the window
    (columns count from ``lo``, negative or not) and takes it away behind its last one; slices are clipped to
    [0, width] and empty ones add nothing"""
    w, p, cell = pairs(chrom, start, end, barcode, cell_of, n_obs, wchrom, wlo, whi)
    start, end, wlo = _i64(start, end, wlo)
    c0 = np.maximum(start[p] - wlo[w], 0)
    c1 = np.minimum(end[p] - wlo[w], int(width))
    ok = c0 < c1
    s = np.asarray(score).astype(np.int64)[p][ok]
    diff = np.zeros((int(n_obs), int(width) + 1), dtype=np.int64)
    np.add.at(diff, (cell[ok], c0[ok]), s)
    np.add.at(diff, (cell[ok], c1[ok]), -s)
    assert np.abs(diff).max(initial=0) < 2 ** 31
    return diff.astype(np.int32)


def pileup_scan(diff, flank, centre):
    """(pileup int64 [n, W], sums int64 [n, 2]) of a difference array [n, W + 1]: the row prefix sums of its first W
    columns; the sum over the ``flank`` first and ``flank`` last columns, and over the columns
    ``centre <= j < W - centre``"""
    W = diff.shape[1] - 1
    pile = np.cumsum(np.asarray(diff)[:, :W].astype(np.int64), axis=1)
    fl = pile[:, :flank].sum(axis=1) + pile[:, W - flank:].sum(axis=1)
    ce = pile[:, centre:W - centre].sum(axis=1)
    return pile, np.stack([fl, ce], axis=1)


def length_classes(start, end, barcode, cell_of, n_obs, n_take, free_bound, mono_bound):
    """int32 [n_obs, 2]: among the first ``n_take`` fragments, per cell, those shorter than ``free_bound`` and the
    others shorter than ``mono_bound``"""
    start, end = _i64(start[:n_take], end[:n_take])
    cell = cells(barcode[:n_take], cell_of, n_obs)
    length = end - start
    cls = np.where(length < free_bound, 0, np.where(length < mono_bound, 1, 2))
    ok = (cell >= 0) & (cls < 2)
    return np.bincount(cell[ok] * 2 + cls[ok], minlength=2 * int(n_obs)).reshape(int(n_obs), 2).astype(np.int32)
