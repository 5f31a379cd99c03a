"""muon_amd.rna.pp.scale without a GPU: the CPU operator set of the tests (the tensor formulations behind
``has(be, "scale_values")`` / ``"scale_dense_rows"``, and the same branch with stand-in operators) and the pure-host
route, against the NumPy statement of tests/scale_refs.py.

Fed the call's own ``var["mean"]`` / ``var["std"]``, every route computes the statement's IEEE operations in f64 and
rounds once: the comparisons are bit for bit.  The moments themselves are compared with numpy's two-pass f64 moments
within 1e-9 relative (sums of at most 400 terms in f64; a gene without variance is excluded from the relative check of
the variance).
"""
import logging

import numpy as np
import pytest
import scipy.sparse as sp

import muon_amd as mu
from muon_amd import AnnData, MuData, rna
from muon_amd._hostmatrix import resident
from muon_amd._rna import preproc as rp
from tests import scale_refs as sr
from tests.scale_support import CountingCpuBackend, KernelCpuBackend

N, D = 400, 37


def _matrix(dtype, seed=0, with_nan=False):
    rng = np.random.default_rng(seed)
    A = rng.gamma(2.0, 1.0, (N, D)) * (rng.random((N, D)) < 0.15)
    return sr.append_crafted(sp.csr_matrix(A.astype(dtype)), seed=seed, with_nan=with_nan)


def _dense_and_stored(M):
    A = M.astype(np.float64).toarray()
    st = np.zeros(A.shape, dtype=bool)
    st[np.repeat(np.arange(M.shape[0]), np.diff(M.indptr)), M.indices] = True
    return A, st


def _check_dense(ad_X, M, var, max_value):
    A, st = _dense_and_stored(M)
    C, _S, _z = sr.scale_ref(A, var["mean"].values, var["std"].values, max_value)
    assert type(ad_X) is np.ndarray and ad_X.flags.c_contiguous and ad_X.dtype == M.dtype
    assert sr.bits_equal(ad_X, C.astype(M.dtype))
    return A, st


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("max_value", [None, 10, 1.5])
@pytest.mark.parametrize("backend", ["tensor", "operators", "host"])
def test_scale_equals_the_statement(dtype, max_value, backend):
    M = _matrix(dtype)
    be = {"tensor": CountingCpuBackend, "operators": KernelCpuBackend, "host": lambda: None}[backend]()
    ad = AnnData(M.copy())
    assert rna.pp.scale(ad, max_value=max_value, backend=be) is None
    A, st = _check_dense(ad.X, M, ad.var, max_value)
    mean, std = sr.moments_ref(A)
    np.testing.assert_allclose(ad.var["mean"].values, mean, rtol=1e-9, atol=0)
    np.testing.assert_allclose(ad.var["std"].values, std, rtol=1e-9, atol=0)
    assert ad.var["std"].values[D] == 1.0 and ad.var["std"].values[D + 1] == 1.0  # the all-zero and the constant gene
    if max_value is not None:
        below, above, zclip = sr.clip_counts(A, st, mean, std, max_value)
        assert below > 0 and above > 0 and zclip > 0
        assert ad.X.min() == -max_value and ad.X.max() == max_value
    if backend == "operators":
        assert be.calls["scale_dense_rows"] >= 1 and be.calls["scale_values"] == 1


def test_nan_stays_nan_and_stored_zero_equals_implicit_zero():
    M = _matrix(np.float32, with_nan=True)
    ad = AnnData(M.copy())
    rna.pp.scale(ad, max_value=10, backend=CountingCpuBackend())
    j = M.shape[1] - 1
    assert np.isnan(ad.X[:, j]).all()  # the gene's moments are NaN: so is the gene, as in scanpy
    g = D + 5  # the gene with explicitly stored zeros
    col = M[:, g].toarray().reshape(-1)
    assert len(set(ad.X[col == 0, g].tolist())) == 1
    assert np.isfinite(ad.X[:, :j]).all()


def test_chunks_and_the_log_line(monkeypatch, caplog):
    M = _matrix(np.float32)
    monkeypatch.setattr(rp, "_DENSE_CHUNK_BYTES", 7 * M.shape[1] * 4 + 3)  # 7 rows a chunk, the last one short
    be = KernelCpuBackend()
    ad = AnnData(M.copy())
    with caplog.at_level(logging.INFO, logger="muon_amd"):
        rna.pp.scale(ad, max_value=3, backend=be)
    assert any("densifies" in r.message for r in caplog.records)
    assert be.calls["scale_dense_rows"] == -(-N // 7)
    _check_dense(ad.X, M, ad.var, 3)
    ref = AnnData(M.copy())
    rna.pp.scale(ref, max_value=3)  # the host route, chunked as well
    assert sr.bits_equal(ref.X, ad.X)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("backend", ["tensor", "operators", "host"])
def test_zero_center_false_stays_sparse_and_clips_from_above_only(dtype, backend):
    M = _matrix(dtype)
    be = {"tensor": CountingCpuBackend, "operators": KernelCpuBackend, "host": lambda: None}[backend]()
    ad = AnnData(M.copy())
    rna.pp.scale(ad, zero_center=False, max_value=1.5, backend=be)
    got = ad.X
    assert sp.issparse(got) and got.dtype == dtype
    assert np.array_equal(got.indptr, M.indptr) and np.array_equal(got.indices, M.indices)
    std = ad.var["std"].values
    t = M.data.astype(np.float64) / std[M.indices]
    assert (t > 1.5).any() and (t < -1.5).any()  # both occur; only the upper side is clipped
    assert sr.bits_equal(got.data, np.minimum(t, 1.5).astype(dtype))
    assert got.data.max() == 1.5 and got.data.min() < -1.5
    C, _S, _z = sr.scale_ref(M.astype(np.float64).toarray(), ad.var["mean"].values, std, 1.5, zero_center=False)
    assert sr.bits_equal(got.toarray(), C.astype(dtype))
    if be is not None:
        Xd = resident(got, be)
        assert Xd is not None and np.array_equal(be.to_host(Xd.values), got.data) and be.calls["upload_csr"] == 1
    assert rp.scaled_form(got) is None


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("max_value", [None, 10, 1.5])
def test_identity_S_plus_z_is_C(dtype, max_value):
    M = _matrix(dtype)
    be = KernelCpuBackend()
    ad = AnnData(M.copy())
    rna.pp.scale(ad, max_value=max_value, backend=be)
    S, z, be2 = rp.scaled_form(ad.X)
    assert be2 is be and np.array_equal(be.to_host(S.indices), M.indices) and np.array_equal(be.to_host(S.indptr), M.indptr)
    A, _st = _dense_and_stored(M)
    Cr, Sr, zr = sr.scale_ref(A, ad.var["mean"].values, ad.var["std"].values, max_value)
    assert sr.bits_equal(z, zr)
    assert sr.bits_equal(be.to_host(S.values), Sr[np.repeat(np.arange(N), np.diff(M.indptr)), M.indices].astype(dtype))
    Sd = sp.csr_matrix((be.to_host(S.values).astype(np.float64), M.indices, M.indptr), shape=M.shape).toarray()
    # S and C are each rounded once from f64 values whose difference is z: one rounding of the storage type apart
    eps = np.finfo(dtype).eps
    assert np.all(np.abs(Sd + z - ad.X.astype(np.float64)) <= eps * np.maximum(np.abs(Cr), np.abs(Cr - zr)))


def test_arguments(monkeypatch):
    M = _matrix(np.float32)
    ad = AnnData(M.copy())
    ad.layers["lognorm"] = M.copy()
    out = rna.pp.scale(ad, max_value=10, copy=True, layer="lognorm")
    assert out is not ad and sp.issparse(ad.layers["lognorm"]) and "mean" not in ad.var.columns
    assert type(out.layers["lognorm"]) is np.ndarray and sp.issparse(out.X)
    assert list(out.var.columns[-2:]) == ["mean", "std"]
    _check_dense(out.layers["lognorm"], M, out.var, 10)

    for kw in (dict(obsm="X_pca"), dict(mask_obs=np.ones(N, dtype=bool))):
        with pytest.raises(NotImplementedError):
            rna.pp.scale(AnnData(M.copy()), **kw)

    class TwoRanks:
        world_size = 2

    with pytest.raises(NotImplementedError):
        rna.pp.scale(AnnData(M.copy()), comm=TwoRanks())
    with pytest.raises(TypeError):
        rna.pp.scale(M)

    mdata = MuData({"rna": AnnData(M.copy())})
    rna.pp.scale(mdata, max_value=10, backend=CountingCpuBackend())
    _check_dense(mdata.mod["rna"].X, M, mdata.mod["rna"].var, 10)
    with pytest.raises(TypeError):
        rna.pp.scale(MuData({"atac": AnnData(M.copy())}))


@pytest.mark.parametrize("sparse", [True, False])
def test_integer_input_becomes_float32(sparse):
    rng = np.random.default_rng(3)
    A = rng.poisson(0.4, (N, D)).astype(np.int64)
    ad = AnnData(sp.csr_matrix(A) if sparse else A.copy())
    rna.pp.scale(ad, max_value=4, backend=CountingCpuBackend() if sparse else None)
    assert ad.X.dtype == np.float32
    C, _S, _z = sr.scale_ref(A, ad.var["mean"].values, ad.var["std"].values, 4)
    assert sr.bits_equal(ad.X, C.astype(np.float32))


def test_dense_input_takes_the_host_route():
    M = _matrix(np.float64)
    be = CountingCpuBackend()
    ad = AnnData(M.toarray())
    rna.pp.scale(ad, max_value=10, backend=be)
    assert be.calls["upload_csr"] == 0 and rp.scaled_form(ad.X) is None
    _check_dense(ad.X, M, ad.var, 10)


# ---- the next step starts without an upload ------------------------------------------------------------------------------
def _prepared(be, max_value=10.0):
    ad = AnnData(sr.e2e_matrix("b16_clip10").copy())
    rna.pp.scale(ad, max_value=max_value, backend=be)
    assert be.calls["upload_csr"] == 1
    return ad


def test_pca_uses_the_remembered_form():
    be = KernelCpuBackend()
    ad = _prepared(be)
    diag = {}
    mu.tl.pca(ad, n_comps=11, oversample=5, diagnostics=diag)  # (no backend=: the form's own serves)
    assert be.calls["upload_csr"] == 1 and diag["block"] == 16 and diag["converged"]  # diagnostics: a device route
    a_pcs, a_x, v, r = sr.deviations("b16_clip10", ad)
    print(f"PARITY cpu b16_clip10: ({a_pcs:.2e}, {a_x:.2e}, {v:.2e}, {r:.2e})")
    assert a_pcs < 1e-4 and a_x < 1e-4 and v < 1e-5 and r < 1e-5  # (the ceiling; the device's figures: test_gpu_scale)

    # a mask cuts S's columns; zero_center=False and another backend go where dense matrices go
    mask = np.random.default_rng(2).random(ad.shape[1]) < 0.6
    diag = {}
    mu.tl.pca(ad, n_comps=11, oversample=5, mask_var=mask, diagnostics=diag)
    assert diag["converged"] and not ad.varm["PCs"][~mask].any() and be.calls["upload_csr"] == 1
    C = ad.X[:, mask].astype(np.float64)
    C -= C.mean(axis=0)
    from oracle.lsi_oracle import max_subspace_angle

    _u, _s, vt = np.linalg.svd(C, full_matrices=False)
    assert max_subspace_angle(ad.varm["PCs"][mask], vt[:11].T) < 1e-4
    for kw in (dict(zero_center=False), dict(backend=CountingCpuBackend())):
        diag = {}
        mu.tl.pca(ad, n_comps=11, diagnostics=diag, **kw)
        assert diag == {}


def test_the_form_is_dropped_after_an_edit_in_place():
    be = KernelCpuBackend()
    ad = _prepared(be)
    assert rp.scaled_form(ad.X, be) is not None
    ad.X[17, 3] += 1.0
    assert rp.scaled_form(ad.X, be) is None and id(ad.X) not in rp._FORMS
    ad.X[17, 3] -= 1.0  # dropped is dropped: the old bytes do not bring it back
    diag = {}
    mu.tl.pca(ad, n_comps=11, diagnostics=diag)
    assert diag == {}


def test_the_form_dies_with_its_array():
    be = KernelCpuBackend()
    ad = _prepared(be)
    key = id(ad.X)
    assert key in rp._FORMS
    copy = ad.X.copy()
    assert rp.scaled_form(copy) is None  # another array with the same bytes has no form
    ad.X = copy
    assert key not in rp._FORMS
