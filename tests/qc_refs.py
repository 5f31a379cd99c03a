"""TEST INFRASTRUCTURE: the NumPy statements of the per-row sums behind ``pp.qc_metrics(qc_vars=, percent_top=)``
(csrc/qc.hip) and the engineered matrices the host and the GPU tests share.  Row loops, f64."""
import numpy as np
import scipy.sparse as sp

D = 520
LENGTHS = [0, 1, 2, 49, 50, 51, 63, 64, 65, 99, 100, 101, 199, 200, 201, 255, 256, 257, 499, 500, 501, 520]
NS = (50, 100, 200, 500)


def top_sums(stored_values_of_row, ns):
    v = np.sort(stored_values_of_row.astype(np.float64))[::-1]
    c = np.concatenate([[0.0], np.cumsum(v)])
    return [c[min(n, len(v))] for n in ns]


def row_top_sums(m, ns):
    """f64 [n_rows, len(ns)] of CSR ``m``: ``top_sums`` row by row over the STORED entries"""
    return np.asarray([top_sums(m.data[m.indptr[i]:m.indptr[i + 1]], ns) for i in range(m.shape[0])],
                      dtype=np.float64).reshape(m.shape[0], len(ns))


def row_masked_sums(m, masks):
    """f64 [n_rows, len(masks)]: per row the sum of the stored values whose column lies in the boolean mask"""
    out = np.zeros((m.shape[0], len(masks)))
    for i in range(m.shape[0]):
        cols = m.indices[m.indptr[i]:m.indptr[i + 1]]
        vals = m.data[m.indptr[i]:m.indptr[i + 1]].astype(np.float64)
        for q, mask in enumerate(masks):
            out[i, q] = vals[mask[cols]].sum()
    return out


def top_sums_bound(m, ns):
    """what two f64 sums of the same k terms may differ by, whatever their orders: k * 2**-52 * sum(abs(terms)), per row
    and per n with the row's own k = min(n, stored entries) and its own k largest terms"""
    out = np.zeros((m.shape[0], len(ns)))
    for i in range(m.shape[0]):
        v = np.sort(m.data[m.indptr[i]:m.indptr[i + 1]].astype(np.float64))[::-1]
        for j, n in enumerate(ns):
            k = min(n, len(v))
            out[i, j] = k * 2.0 ** -52 * np.abs(v[:k]).sum()
    return out


def masked_sums_bound(m, masks):
    out = np.zeros((m.shape[0], len(masks)))
    for i in range(m.shape[0]):
        cols = m.indices[m.indptr[i]:m.indptr[i + 1]]
        vals = np.abs(m.data[m.indptr[i]:m.indptr[i + 1]].astype(np.float64))
        for q, mask in enumerate(masks):
            out[i, q] = mask[cols].sum() * 2.0 ** -52 * vals[mask[cols]].sum()
    return out


def _rows_to_csr(rows, d, dtype):
    indptr = np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])]).astype(np.int64)
    indices = np.concatenate([c for c, _ in rows]).astype(np.int32) if rows else np.zeros(0, np.int32)
    data = np.concatenate([v for _, v in rows]).astype(dtype) if rows else np.zeros(0, dtype)
    m = sp.csr_matrix((data, indices, indptr), shape=(len(rows), d))
    m.has_sorted_indices = False
    return m


def engineered(dtype, d=D, seed=0):
    """Rows of the lengths LENGTHS (around 64 lanes and around every n of NS; the first and the last row empty), every
    third one stored in DESCENDING column order; integer values 1..5 with ~15 % explicitly stored zeros, so the n-th
    value always sits inside a run of ties; one all-equal row of 300 entries; one row with a single 2^20 among ones;
    a closing empty row.  Every sum is an integer below 2^53: exact in f64 in any order."""
    rng = np.random.default_rng(seed)
    rows = []
    for i, k in enumerate(LENGTHS + [0]):
        cols = np.sort(rng.choice(d, k, replace=False))
        if i % 3 == 1:
            cols = cols[::-1]
        vals = rng.integers(1, 6, k).astype(np.float64)
        vals[rng.random(k) < 0.15] = 0
        rows.append((cols, vals))
    rows.insert(5, (np.sort(rng.choice(d, 300, replace=False)), np.full(300, 3.0)))
    big = np.ones(260)
    big[137] = 2.0 ** 20
    rows.insert(9, (np.sort(rng.choice(d, 260, replace=False)), big))
    m = _rows_to_csr(rows, d, dtype)
    assert m[0].nnz == 0 and m[m.shape[0] - 1].nnz == 0 and (m.data == 0).sum() > 50
    return m


def with_long_row(dtype, long=20000, d=20008, seed=1):
    """short rows around one row of ``long`` stored entries (the select has no row-length limit: this row is walked in
    313 steps of 64 per pass) and two neighbours of long - 1 and long + 1"""
    rng = np.random.default_rng(seed)
    rows = []
    for k in (3, 0, long - 1, 7, long, long + 1, 1):
        vals = rng.integers(1, 6, k).astype(np.float64)
        vals[rng.random(k) < 0.15] = 0
        rows.append((np.sort(rng.choice(d, k, replace=False)), vals))
    return _rows_to_csr(rows, d, dtype)


def many_short_rows(dtype, n, d=40, seed=2):
    """n rows of 0 - 3 stored entries"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 4, n)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    indices = rng.integers(0, d, int(indptr[-1])).astype(np.int32)  # (a duplicate column inside a row is just two entries)
    data = rng.integers(0, 6, int(indptr[-1])).astype(dtype)
    m = sp.csr_matrix((data, indices, indptr), shape=(n, d))
    m.has_sorted_indices = False
    return m


def masks_for(d, M, seed=3):
    """M boolean column masks: mask 0 empty, mask 1 full (where M allows), the others random; with M = 32 the last one
    is bit 31 of the flag word"""
    rng = np.random.default_rng(seed)
    masks = rng.random((M, d)) < 0.3
    if M >= 3:
        masks[0] = False
        masks[1] = True
    return masks
