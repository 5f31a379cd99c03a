"""csrc/qc.hip on the GPU: the masked row sums and the top-n row sums (a radix select per row) against the NumPy
statements of tests/qc_refs.py on rows built around the wave's 64 lanes and around every n, and
qc_metrics(qc_vars=, percent_top=) -> filter_obs -> intersect_obs end to end on the resident copies."""
import ctypes

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

import muon_amd as mu
from muon_amd import _ffi
from muon_amd._hostmatrix import resident
from tests import qc_refs
from tests.cpu_backend import CpuTestBackend
from tests.synth import planted_topics_csr

pytestmark = pytest.mark.gpu

# A launch of the masked sums has at most 256 CUs x 16 workgroups x 4 waves = 16 384 waves, one of the top sums
# 256 x 8 x 4 = 8192 (wave_grid in csrc/qc.hip): with N_STRIDE rows every wave of either walks its row loop at least twice
N_STRIDE = 2 * 16384 + 5


def _upload(hip, m):
    return hip.upload_csr(m.indptr, m.indices, m.data, m.shape, slab_ptr=False)


def _flags(hip, masks):
    w = np.zeros(masks.shape[1], dtype=np.uint32)
    for b, mask in enumerate(masks):
        w |= mask.astype(np.uint32) << np.uint32(b)
    return hip.to_device(w.view(np.int32), np.int32)


@pytest.fixture(scope="module", params=[np.float32, np.float64], ids=["f32", "f64"])
def case(request, hip):
    m = qc_refs.engineered(request.param)
    assert set(qc_refs.LENGTHS) <= set(np.diff(m.indptr).tolist())
    return m, _upload(hip, m)


@pytest.mark.parametrize("ns", [qc_refs.NS, (520,), (1,), (1, 2, 3, 64, 65, 300, 519, 520)], ids=str)
def test_top_sums_bit_equal_and_repeatable(hip, case, ns):
    m, X = case
    got = hip.row_top_sums(X, ns)
    assert got.dtype == torch.float64 and tuple(got.shape) == (m.shape[0], len(ns))
    assert hip.to_host(got).tobytes() == qc_refs.row_top_sums(m, ns).tobytes()
    assert hip.to_host(hip.row_top_sums(X, ns)).tobytes() == hip.to_host(got).tobytes()


@pytest.mark.parametrize("M", [1, 3, 32])
def test_masked_sums_bit_equal_and_repeatable(hip, case, M):
    m, X = case
    masks = qc_refs.masks_for(m.shape[1], M)
    assert M < 3 or (not masks[0].any() and masks[1].all())
    assert M < 32 or masks[31].any()  # bit 31 of the flag word
    flags = _flags(hip, masks)
    got = hip.row_masked_sums(X, flags, M)
    assert got.dtype == torch.float64 and tuple(got.shape) == (m.shape[0], M)
    assert hip.to_host(got).tobytes() == qc_refs.row_masked_sums(m, masks).tobytes()
    assert hip.to_host(hip.row_masked_sums(X, flags, M)).tobytes() == hip.to_host(got).tobytes()


def test_thirty_three_qc_variables_are_two_launches(hip):
    m = qc_refs.engineered(np.float32)
    m.sort_indices()
    masks = qc_refs.masks_for(m.shape[1], 33, seed=9)
    var = pd.DataFrame({f"q{i}": masks[i] for i in range(33)}, index=[f"g{j}" for j in range(m.shape[1])])
    ad = mu.AnnData(m.copy(), var=var)
    calls = []
    orig = hip.row_masked_sums
    hip.row_masked_sums = lambda X, flags, M: (calls.append(M), orig(X, flags, M))[1]
    try:
        obs, _ = mu.pp.qc_metrics(ad, qc_vars=[f"q{i}" for i in range(33)], inplace=False, log1p=False, backend=hip)
    finally:
        del hip.row_masked_sums
    assert calls == [32, 1]
    want = qc_refs.row_masked_sums(m, masks)
    for i in (0, 1, 31, 32):
        assert obs[f"total_counts_q{i}"].values.tobytes() == want[:, i].tobytes(), i
    assert want[:, 32].any() and list(obs.columns)[-1] == "pct_counts_q32"


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_values_that_are_no_integers_within_the_derived_bound(hip, dtype):
    m = qc_refs.engineered(dtype)
    m.data = np.log1p(m.data)
    X = _upload(hip, m)
    got = hip.to_host(hip.row_top_sums(X, qc_refs.NS))
    err, bound = np.abs(got - qc_refs.row_top_sums(m, qc_refs.NS)), qc_refs.top_sums_bound(m, qc_refs.NS)
    print("top sums: largest error / bound", float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()
    masks = qc_refs.masks_for(m.shape[1], 3)
    got = hip.to_host(hip.row_masked_sums(X, _flags(hip, masks), 3))
    err, bound = np.abs(got - qc_refs.row_masked_sums(m, masks)), qc_refs.masked_sums_bound(m, masks)
    print("masked sums: largest error / bound", float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_row_of_twenty_thousand_entries_through_the_public_call(hip, dtype):
    """the select has no row-length limit: rows of 19 999, 20 000 and 20 001 entries among short ones"""
    m = qc_refs.with_long_row(dtype)
    m.sort_indices()
    rng = np.random.default_rng(0)
    ad = mu.AnnData(m.copy(), var=pd.DataFrame({"mt": rng.random(m.shape[1]) < 0.2},
                                               index=[f"g{j}" for j in range(m.shape[1])]))
    ns = (1, 50, 500, 19999, 20000, 20001, 20008)
    obs, _ = mu.pp.qc_metrics(ad, qc_vars="mt", percent_top=ns, inplace=False, backend=hip)
    total = np.asarray(m.sum(axis=1, dtype=np.float64)).reshape(-1)
    top = qc_refs.row_top_sums(m, ns)
    with np.errstate(invalid="ignore"):
        for j, n in enumerate(ns):
            assert obs[f"pct_counts_in_top_{n}_genes"].values.tobytes() == (100.0 * top[:, j] / total).tobytes(), n
    assert obs["total_counts_mt"].values.tobytes() == qc_refs.row_masked_sums(m, [ad.var["mt"].values])[:, 0].tobytes()


def test_more_rows_than_a_launch_has_waves(hip):
    m = qc_refs.many_short_rows(np.float32, N_STRIDE)
    assert m.shape[0] == 32773 and np.diff(m.indptr).max() == 3 and (np.diff(m.indptr) == 0).any()
    X = _upload(hip, m)
    ns = (1, 2, 3, 4)
    assert hip.to_host(hip.row_top_sums(X, ns)).tobytes() == qc_refs.row_top_sums(m, ns).tobytes()
    masks = qc_refs.masks_for(m.shape[1], 3)
    got = hip.to_host(hip.row_masked_sums(X, _flags(hip, masks), 3))
    assert got.tobytes() == qc_refs.row_masked_sums(m, masks).tobytes()


def test_a_row_that_stores_a_nan_terminates_and_the_others_are_right(hip):
    m = qc_refs.engineered(np.float32)
    at = int(m.indptr[12]) + 3
    row = int(np.searchsorted(m.indptr, at, side="right") - 1)
    m.data[at] = np.nan
    got = hip.to_host(hip.row_top_sums(_upload(hip, m), qc_refs.NS))
    ok = np.arange(m.shape[0]) != row
    assert got[ok].tobytes() == qc_refs.row_top_sums(m, qc_refs.NS)[ok].tobytes()


def test_end_to_end_stays_resident():
    """qc_metrics(qc_vars, percent_top) -> filter_obs on pct_counts_mt -> intersect_obs -> tfidf with one upload per
    modality; the frames are those of the tensor formulations (integers: exact)"""
    from muon_amd._backend import get_backend

    be = get_backend()
    rng = np.random.default_rng(1)
    X = planted_topics_csr(1500, 2000, n_topics=8, density=0.03, seed=5, dtype=np.float32)
    Y = planted_topics_csr(1400, 900, n_topics=8, density=0.02, seed=6, dtype=np.float32)
    var = pd.DataFrame({"mt": rng.random(2000) < 0.18}, index=[f"g{j}" for j in range(2000)])
    names = np.asarray([f"c{i}" for i in range(1500)])
    rna = mu.AnnData(X.copy(), obs=pd.DataFrame(index=names), var=var.copy())
    own = rng.permutation(names)[:1400]
    atac = mu.AnnData(Y.copy(), obs=pd.DataFrame(index=own))
    uploads = []
    orig = be.upload_csr
    be.upload_csr = lambda *a, **k: (uploads.append(1), orig(*a, **k))[1]
    try:
        mu.pp.qc_metrics(rna, qc_vars=["mt"], percent_top=(50, 100))
        twin = mu.AnnData(X.copy(), obs=pd.DataFrame(index=names), var=var.copy())
        cpu_obs, cpu_var = mu.pp.qc_metrics(twin, qc_vars=["mt"], percent_top=(50, 100), inplace=False,
                                            backend=CpuTestBackend())
        for c in cpu_obs.columns:
            assert rna.obs[c].values.tobytes() == cpu_obs[c].values.tobytes(), c
        for c in cpu_var.columns:
            assert rna.var[c].values.tobytes() == cpu_var[c].values.tobytes(), c
        assert list(rna.obs.columns) == list(cpu_obs.columns)
        mu.pp.qc_metrics(atac)
        assert len(uploads) == 2
        keep = rna.obs["pct_counts_mt"].values < 20
        assert 0.2 < keep.mean() < 0.9
        mu.pp.filter_obs(rna, "pct_counts_mt", lambda x: x < 20)
        mdata = mu.MuData({"rna": rna, "atac": atac})
        mu.pp.intersect_obs(mdata)
        common = set(names[keep]) & set(own)
        assert set(mdata.obs_names) == common and 0 < len(common) < min(int(keep.sum()), 1400)
        for ad, host, order in ((rna, X, names), (atac, Y, own)):
            sel = np.isin(order, list(common))
            assert list(ad.obs_names) == list(order[sel])
            want = host[sel]
            assert np.array_equal(ad.X.indptr, want.indptr) and np.array_equal(ad.X.indices, want.indices)
            R = resident(ad.X, be)
            assert R is not None and R.shape == want.shape
            assert np.array_equal(be.to_host(R.indptr), want.indptr) and np.array_equal(be.to_host(R.indices), want.indices)
            assert be.to_host(R.values).tobytes() == want.data.tobytes()
        mu.atac.pp.tfidf(atac)
        mu.pp.qc_metrics(rna, qc_vars=["mt"], percent_top=(50,))
        assert len(uploads) == 2
    finally:
        be.upload_csr = orig


def test_arguments_are_validated_before_any_hip_call():
    lib = _ffi.lib()
    ns = (ctypes.c_int64 * 9)(50, 100, 200, 500, 501, 502, 503, 504, 505)
    top = lambda dtype, n, d, nnz, ip, v, L, h, out: lib.mu_csr_row_top_sums(dtype, n, d, nnz, ip, v, L, h, out, None)  # noqa: E731
    one = ctypes.c_int64(0)
    p = ctypes.addressof(one)  # (an address that is never followed: every call below is refused first)
    assert top(0, 4, 520, 8, None, p, 4, ns, p) == -1 and b"mu_csr_row_top_sums" in lib.mu_last_error()
    assert top(0, 4, 520, 8, p, None, 4, ns, p) == -1 and top(0, 4, 520, 8, p, p, 4, ns, None) == -1
    assert top(0, 4, 520, 8, p, p, 4, None, p) == -1 and b"null" in lib.mu_last_error()
    assert top(0, -1, 520, 8, p, p, 4, ns, p) == -1 and top(0, 4, -1, 8, p, p, 4, ns, p) == -1
    assert top(0, 4, 520, -8, p, p, 4, ns, p) == -1 and b"negative" in lib.mu_last_error()
    assert top(7, 4, 520, 8, p, p, 4, ns, p) == -1 and b"dtype" in lib.mu_last_error()
    assert top(0, 4, 520, 8, p, p, 0, ns, p) == -1 and top(0, 4, 520, 8, p, p, 9, ns, p) == -1
    assert b"mu_csr_row_top_sums" in lib.mu_last_error()
    assert top(0, 4, 520, 8, p, p, 2, (ctypes.c_int64 * 2)(100, 100), p) == -1 and b"ascending" in lib.mu_last_error()
    assert top(0, 4, 520, 8, p, p, 2, (ctypes.c_int64 * 2)(100, 50), p) == -1
    assert top(0, 4, 520, 8, p, p, 2, (ctypes.c_int64 * 2)(50, 521), p) == -1 and b"n_cols" in lib.mu_last_error()
    assert top(0, 4, 520, 8, p, p, 1, (ctypes.c_int64 * 1)(0), p) == -1
    assert top(0, 0, 520, 0, None, None, 4, ns, None) == 0  # (no rows: nothing to do, nothing to point at)
    msk = lambda dtype, n, d, nnz, ip, ix, v, f, M, out: lib.mu_csr_row_masked_sums(dtype, n, d, nnz, ip, ix, v, f, M, out, None)  # noqa: E731
    assert msk(0, 4, 520, 8, None, p, p, p, 3, p) == -1 and b"mu_csr_row_masked_sums" in lib.mu_last_error()
    assert msk(0, 4, 520, 8, p, None, p, p, 3, p) == -1 and msk(0, 4, 520, 8, p, p, None, p, 3, p) == -1
    assert msk(0, 4, 520, 8, p, p, p, None, 3, p) == -1 and msk(0, 4, 520, 8, p, p, p, p, 3, None) == -1
    assert msk(0, -4, 520, 8, p, p, p, p, 3, p) == -1 and msk(0, 4, -520, 8, p, p, p, p, 3, p) == -1
    assert msk(3, 4, 520, 8, p, p, p, p, 3, p) == -1 and b"dtype" in lib.mu_last_error()
    assert msk(0, 4, 520, 8, p, p, p, p, 0, p) == -1 and msk(0, 4, 520, 8, p, p, p, p, 33, p) == -1
    assert msk(0, 4, 1 << 31, 8, p, p, p, p, 3, p) == -1 and b"int32" in lib.mu_last_error()
    assert msk(1, 0, 520, 0, None, None, None, None, 32, None) == 0
