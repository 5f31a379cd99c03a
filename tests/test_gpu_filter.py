"""csrc/filter.hip on the GPU: the QC sweep and the submatrix kernels against numpy / scipy on matrices built to hit the
wave loop's edges, and filter_* / qc_metrics end to end on the resident copy (reference muon/_core/preproc.py:675-881)."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import muon_amd as mu
from muon_amd import _ffi
from muon_amd._hostmatrix import resident
from oracle import lsi_oracle
from tests.synth import planted_topics_csr

pytestmark = pytest.mark.gpu
ANGLE = 1e-4  # the bar of tests/test_gpu_lsi.py

N, D = 300, 520
LENGTHS = [0, 1, 63, 64, 65, 128, 129, 400, 0, 2, 256, 257, 191, 192, 193, 520]


def _engineered(dtype, n=N, d=D, descending=True, seed=0):
    """row lengths around the 64-lane chunk and the 256-entry step, an empty first and last row, rows stored in DESCENDING
    column order, explicitly stored zeros and one NaN; integer values (every sum exact in f64)"""
    rng = np.random.default_rng(seed)
    indptr, indices, data = [0], [], []
    for i in range(n):
        if i in (0, n - 1):
            k = 0
        elif i <= len(LENGTHS):
            k = min(LENGTHS[i - 1], d)
        else:
            k = int(rng.integers(0, min(d, 90)))
        cols = np.sort(rng.choice(d, k, replace=False))
        if descending:
            cols = cols[::-1]
        vals = rng.integers(1, 6, k).astype(dtype)
        vals[rng.random(k) < 0.15] = 0  # explicit zeros
        indices.append(cols.astype(np.int32))
        data.append(vals)
        indptr.append(indptr[-1] + k)
    data = np.concatenate(data)
    data[int(indptr[8]) + 5] = np.nan  # inside the 400-entry row
    m = sp.csr_matrix((data, np.concatenate(indices), np.asarray(indptr, dtype=np.int64)), shape=(n, d))
    m.has_sorted_indices = not descending
    return m


@pytest.fixture(scope="module", params=[np.float32, np.float64], ids=["f32", "f64"])
def case(request, hip):
    m = _engineered(request.param)
    assert (m.data == 0).sum() > 10 and np.isnan(m.data).sum() == 1
    assert set(LENGTHS) <= set(np.diff(m.indptr).tolist())
    return m, hip.upload_csr(m.indptr, m.indices, m.data, m.shape, slab_ptr=False)


def _table(cmask):
    t = (np.cumsum(cmask, dtype=np.int64) - 1).astype(np.int32)
    t[~cmask] = -1
    return t


def _sub(hip, X, rmask, cmask):
    rows = hip.to_device(np.nonzero(rmask)[0].astype(np.int64), np.int64)
    return hip.csr_submatrix(X, rows, hip.to_device(_table(cmask), np.int32), int(cmask.sum()))


def _same_arrays(hip, Y, want):
    assert Y.shape == want.shape
    assert Y.indptr.dtype == torch.int64 and Y.indices.dtype == torch.int32
    assert np.array_equal(hip.to_host(Y.indptr), want.indptr)
    assert np.array_equal(hip.to_host(Y.indices), want.indices)
    assert hip.to_host(Y.values).tobytes() == np.ascontiguousarray(want.data).tobytes()  # bit for bit, the NaN included


def _selections(n, d):
    rng = np.random.default_rng(5)
    full_r, full_c = np.ones(n, bool), np.ones(d, bool)
    return {
        "everything": (full_r, full_c),
        "no rows": (np.zeros(n, bool), full_c),
        "no columns": (full_r, np.zeros(d, bool)),
        "first row": (np.arange(n) == 0, full_c),
        "last row": (np.arange(n) == n - 1, full_c),
        "last column": (full_r, np.arange(d) == d - 1),
        "random": (rng.random(n) < 0.6, rng.random(d) < 0.5),
    }


@pytest.mark.parametrize("name", list(_selections(N, D)))
def test_submatrix_is_scipy_slicing_bit_for_bit(hip, case, name):
    m, X = case
    rmask, cmask = _selections(N, D)[name]
    if name == "random":  # the draw must not drop the one NaN: its row and its column are kept whatever the masks say
        at = int(np.nonzero(np.isnan(m.data))[0][0])
        rmask[np.searchsorted(m.indptr, at, side="right") - 1] = True
        cmask[m.indices[at]] = True
        assert 0.5 < rmask.mean() < 0.7 and 0.4 < cmask.mean() < 0.6 and not rmask.all()
    want = m[rmask][:, cmask]
    Y = _sub(hip, X, rmask, cmask)
    _same_arrays(hip, Y, want)
    assert Y.plans is None and Y.xstream is None  # none of the source's derived tables
    Y2 = _sub(hip, X, rmask, cmask)  # two launches agree
    assert torch.equal(Y.indptr, Y2.indptr) and torch.equal(Y.indices, Y2.indices)
    assert torch.equal(Y.values.view(torch.uint8), Y2.values.view(torch.uint8))
    if name == "random":
        assert (want.data == 0).any() and np.isnan(want.data).any()  # the explicit zeros and the NaN are still there


def _qc_checks(hip, m, X):
    got = [hip.to_host(t) for t in hip.csr_qc(X)]
    again = [hip.to_host(t) for t in hip.csr_qc(X)]
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()
    row_nnz, rowsum, col_nnz, colsum = got
    assert row_nnz.dtype == np.int64 and col_nnz.dtype == np.int64 and rowsum.dtype == np.float64
    a = m.toarray()
    nz = a != 0  # NaN != 0: counted; stored zeros: not
    assert np.array_equal(row_nnz, nz.sum(axis=1)) and np.array_equal(col_nnz, nz.sum(axis=0))
    assert (m.getnnz(axis=1) != row_nnz).any()
    rs, cs = (hip.to_host(t) for t in hip.row_col_sums(X))
    assert rowsum.tobytes() == rs.tobytes() and colsum.tobytes() == cs.tobytes()
    return got


def test_qc_counts_and_sums(hip, case):
    m, X = case  # (520 columns are one slab: the sweep does not need the rows sorted)
    row_nnz, rowsum, col_nnz, colsum = _qc_checks(hip, m, X)
    assert np.isnan(rowsum).sum() == 1 and np.isnan(colsum).sum() == 1
    ok = ~np.isnan(rowsum)
    assert np.array_equal(rowsum[ok], np.nan_to_num(m.toarray()).sum(axis=1)[ok])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_narrow_matrix(hip, dtype):
    m = _engineered(dtype, n=70, d=5, seed=2)
    X = hip.upload_csr(m.indptr, m.indices, m.data, m.shape, slab_ptr=False)
    _qc_checks(hip, m, X)
    for rmask, cmask in _selections(70, 5).values():
        _same_arrays(hip, _sub(hip, X, rmask, cmask), m[rmask][:, cmask])


@pytest.mark.parametrize("with_table", [False, True])
def test_qc_across_two_slabs(hip, with_table):
    """9000 columns: two 8192-column slabs, sorted rows; 3000 empty rows in a run, which fall to ONE workgroup - more
    than the 1024 rows its waves take per strip -, and a row that runs through both slabs"""
    a = _engineered(np.float32, n=1500, d=9000, descending=False, seed=3)
    b = _engineered(np.float32, n=200, d=9000, descending=False, seed=4)
    wide = np.sort(np.random.default_rng(0).choice(9000, 8500, replace=False)).astype(np.int32)
    m = sp.vstack([a, sp.csr_matrix((3000, 9000), dtype=np.float32),
                   sp.csr_matrix((np.ones(8500, np.float32), wide, [0, 8500]), shape=(1, 9000)), b]).tocsr()
    m.sort_indices()
    assert m.dtype == np.float32 and (m.data == 0).any() and np.isnan(m.data).sum() == 2
    X = hip.upload_csr(m.indptr, m.indices, m.data, m.shape, slab_ptr=False)
    if with_table:  # the slab pointers alone, as mu_csr_slab_ptr makes them where a device CSR is made
        from muon_amd._backend import CsrPlans, _n_slab_ptr

        table = hip.empty((_n_slab_ptr(*m.shape),), torch.int64)
        _ffi.check(hip.lib.mu_csr_slab_ptr(m.shape[0], m.shape[1], X.indptr.data_ptr(), X.indices.data_ptr(),
                                           table.data_ptr(), hip._stream()))
        X.plans = CsrPlans(CsrPlans.key_of(X), slab_ptr=table)
    assert (hip._slab_ptr_of(X) is not None) == with_table
    _qc_checks(hip, m, X)
    rmask, cmask = np.arange(m.shape[0]) % 3 != 1, np.arange(9000) % 5 != 0
    _same_arrays(hip, _sub(hip, X, rmask, cmask), m[rmask][:, cmask])


def test_arguments_are_validated_before_any_hip_call():
    lib = _ffi.lib()
    assert lib.mu_csr_qc(0, 4, 4, None, None, None, None, None, None, None, None, 0, None, None) == -1
    assert b"mu_csr_qc" in lib.mu_last_error()
    assert lib.mu_csr_qc(7, 4, 4, None, None, None, None, None, None, None, None, 0, None, None) == -1
    assert lib.mu_csr_qc(0, -1, 4, None, None, None, None, None, None, None, None, 0, None, None) == -1
    assert lib.mu_csr_submatrix_count(4, 4, 2, None, None, None, None, None, None) == -1
    assert b"mu_csr_submatrix_count" in lib.mu_last_error()
    assert lib.mu_csr_submatrix_count(4, 4, 5, None, None, None, None, None, None) == -1  # more kept rows than rows
    assert lib.mu_csr_submatrix_fill(0, 4, 4, 2, None, None, None, None, None, None, None, None, None) == -1
    assert lib.mu_csr_submatrix_fill(3, 4, 4, 0, None, None, None, None, None, None, None, None, None) == -1
    assert b"dtype" in lib.mu_last_error()
    assert lib.mu_csr_submatrix_fill(0, 4, 1 << 31, 0, None, None, None, None, None, None, None, None, None) == -1


def test_filtered_pipeline_stays_resident():
    """qc_metrics -> filter_var -> filter_obs -> tfidf -> lsi with ONE upload, against the same calls on a fresh object
    built from the host-filtered matrix (same kernels, same input: tfidf bit-identical, lsi inside the oracle bar)"""
    from muon_amd._backend import get_backend

    be = get_backend()
    X = planted_topics_csr(2000, 3000, n_topics=10, density=0.01, seed=3, dtype=np.float32)
    ad = mu.AnnData(X.copy())
    uploads = []
    orig = be.upload_csr
    be.upload_csr = lambda *a, **k: (uploads.append(1), orig(*a, **k))[1]
    try:
        mu.pp.qc_metrics(ad)
        cols = np.asarray((X != 0).sum(axis=0)).reshape(-1)
        rows = np.asarray((X != 0).sum(axis=1)).reshape(-1)
        assert np.array_equal(ad.var["n_cells_by_counts"].values, cols)
        assert np.array_equal(ad.obs["n_genes_by_counts"].values, rows)
        assert np.array_equal(ad.obs["total_counts"].values, np.asarray(X.sum(axis=1, dtype=np.float64)).reshape(-1))
        mu.pp.filter_var(ad, "n_cells_by_counts", lambda x: x >= 3)
        mu.pp.filter_obs(ad, "n_genes_by_counts", lambda x: x >= 45)
        host = X[:, cols >= 3][rows >= 45]
        assert ad.shape == host.shape and 0 < host.shape[0] < 2000 and 0 < host.shape[1] < 3000
        assert np.array_equal(ad.X.indptr, host.indptr) and np.array_equal(ad.X.indices, host.indices)
        R = resident(ad.X, be)
        assert R is not None and np.array_equal(be.to_host(R.indices), host.indices)
        mu.atac.pp.tfidf(ad)
        mu.atac.tl.lsi(ad, n_comps=10)
        assert len(uploads) == 1
    finally:
        be.upload_csr = orig
    ref = mu.AnnData(host.copy())
    mu.atac.pp.tfidf(ref)
    mu.atac.tl.lsi(ref, n_comps=10)
    assert np.array_equal(ad.X.indices, ref.X.indices) and ad.X.data.tobytes() == ref.X.data.tobytes()
    assert lsi_oracle.max_subspace_angle(ad.varm["LSI"], ref.varm["LSI"]) < ANGLE
    np.testing.assert_allclose(ad.uns["lsi"]["stdev"], ref.uns["lsi"]["stdev"], rtol=1e-5)
