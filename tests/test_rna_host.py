"""muon_amd.rna.pp and muon_amd.tl.pca without a GPU: the CPU operator set of the tests (tensor formulations behind
``has(be, ...)``) and the pure-host route (no device copy, no ``backend=``).

What is pinned, and against what:
  * ``tl.pca``: every case of tests/golden/rna_golden.npz (scikit-learn 1.7.2 on the densified matrix), by the largest
    principal angle of ``PCs`` and of ``X_pca`` (inside the top k singular values lie 0.07 % apart: never single
    vectors) and the relative deviation of ``variance`` / ``variance_ratio``.  The bounds are ten times the worst case
    measured on the CPU operator set (CPU_MEASURED), and no angle bound exceeds lsi's 1e-4, no rtol 1e-5.  The device's
    own figures are in tests/test_gpu_rna.py.
  * ``normalize_total`` / ``log1p``: the f64 statements of tests/rna_fixture.py, within 2 ulp of f32 for f32 input and
    4 * 2^-53 relative for f64; pattern and index arrays identical.
  * ``highly_variable_genes``: an independent restatement in plain numpy loops over explicit bin edges, and one
    hand-computed case.  Parity with scanpy itself is not pinned.
"""
import warnings

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

import muon_amd as mu
from muon_amd import AnnData, MuData, rna
from muon_amd._hostmatrix import resident
from tests import rna_fixture as fx
from tests.cpu_backend import CpuTestBackend

BE = CpuTestBackend()

# (angle of PCs, angle of X_pca, variance, variance_ratio) measured on the CPU operator set, per case
CPU_MEASURED = {
    "b16": (5.64e-06, 1.64e-06, 2.43e-08, 2.27e-08), "b16_scale": (3.11e-07, 2.45e-07, 2.05e-08, 2.05e-08),
    "b32": (6.46e-07, 3.56e-07, 2.03e-08, 1.98e-08), "b32_scale": (3.33e-06, 1.46e-06, 2.03e-08, 2.03e-08),
    "b64": (1.92e-06, 1.17e-06, 2.35e-08, 2.67e-08), "wide": (1.27e-06, 3.53e-07, 3.88e-08, 3.90e-08),
    "masked": (4.38e-07, 2.36e-07, 1.30e-08, 1.50e-08), "uncentred": (9.43e-06, 2.89e-06, 1.43e-07, 1.41e-07),
}
ANGLE = min(10 * max(max(v[:2]) for v in CPU_MEASURED.values()), 1e-4)   # 9.4e-5
VAR_RTOL = min(10 * max(max(v[2:]) for v in CPU_MEASURED.values()), 1e-5)  # 1.4e-6
# the host route is scipy's ARPACK in f64 on the f32-rounded input: what is left is the rounding of the input.
# (angle of PCs, angle of X_pca, variance, variance_ratio) measured per case; the bounds are ten times the worst
HOST_MEASURED = {
    "b16": (3.13e-08, 3.17e-08, 6.91e-09, 5.24e-09), "b16_scale": (3.01e-08, 3.37e-08, 2.83e-09, 2.83e-09),
    "wide": (2.81e-08, 3.15e-08, 2.09e-09, 1.82e-09), "masked": (3.08e-08, 3.38e-08, 5.76e-09, 4.66e-09),
    "uncentred": (3.22e-08, 3.29e-08, 1.41e-08, 1.24e-08),
}
HOST_ANGLE = 10 * max(max(v[:2]) for v in HOST_MEASURED.values())
HOST_RTOL = 10 * max(max(v[2:]) for v in HOST_MEASURED.values())
U53 = 2.0 ** -53


def _ulps32(got, ref64):
    ref32 = ref64.astype(np.float32)
    return np.max(np.abs(got.astype(np.float64) - ref64) / np.spacing(np.abs(ref32)).astype(np.float64)) if got.size else 0.0


def _same_pattern(a, b):
    return np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)


# ---- tl.pca ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fx.CASES))
def test_pca_golden_cpu_set(name):
    ad, diag = fx.run_case(mu, name, BE)
    c = fx.CASES[name]
    assert diag["block"] == c["block"] and diag["converged"]
    a_pcs, a_x, v, r = fx.deviations(name, ad)
    print(f"{name}: PCs {a_pcs:.2e} rad, X_pca {a_x:.2e} rad, variance {v:.2e}, ratio {r:.2e}")
    assert a_pcs < ANGLE and a_x < ANGLE and v < VAR_RTOL and r < VAR_RTOL
    assert ad.obsm["X_pca"].shape == (c["n"], c["k"]) and ad.obsm["X_pca"].dtype == np.float32
    assert ad.varm["PCs"].shape == (c["d"], c["k"])
    p = ad.uns["pca"]["params"]
    assert p["zero_center"] == c["zero_center"] and p["scale"] == c["scale"]
    assert p["use_highly_variable"] == c["masked"]


@pytest.mark.parametrize("name", list(HOST_MEASURED))
def test_pca_golden_host_route(name):
    ad, diag = fx.run_case(mu, name, None)
    assert diag == {} and resident(ad.X, BE) is None
    a_pcs, a_x, v, r = fx.deviations(name, ad)
    assert a_pcs < HOST_ANGLE and a_x < HOST_ANGLE and v < HOST_RTOL and r < HOST_RTOL


def test_pca_repeats_byte_equal_and_f64_input():
    a, _ = fx.run_case(mu, "wide", BE)
    b, _ = fx.run_case(mu, "wide", BE)
    assert a.obsm["X_pca"].tobytes() == b.obsm["X_pca"].tobytes() and a.varm["PCs"].tobytes() == b.varm["PCs"].tobytes()
    # an f64 matrix goes through the f32 process
    c = fx.CASES["wide"]
    ad = AnnData(fx.lognorm("wide").copy())
    mu.tl.pca(ad, n_comps=c["k"], oversample=c["oversample"], dtype="float64", backend=BE)
    assert ad.obsm["X_pca"].dtype == np.float64
    dev = fx.deviations("wide", ad)
    assert max(dev[:2]) < ANGLE and max(dev[2:]) < VAR_RTOL


def test_pca_arguments_and_slots():
    X = fx.lognorm("wide").astype(np.float32)
    n, d = X.shape
    ad = AnnData(X)
    with pytest.raises(TypeError):
        mu.tl.pca(MuData({"rna": ad}), backend=BE)
    with pytest.raises(NotImplementedError):
        mu.tl.pca(ad, svd_solver="randomized", backend=BE)
    with pytest.raises(ValueError, match="0 < k < min"):
        mu.tl.pca(ad, n_comps=min(n, d), backend=BE)
    with pytest.raises(ValueError, match="0 < k < min"):
        mu.tl.pca(ad, n_comps=min(n, d))
    with pytest.raises(ValueError):
        mu.tl.pca(ad, use_highly_variable=True, backend=BE)
    with pytest.raises(ValueError):
        mu.tl.pca(ad, use_highly_variable=False, mask_var=np.ones(d, bool), backend=BE)

    class _Two:
        world_size = 2

    with pytest.raises(NotImplementedError, match="runs on one rank"):
        mu.tl.pca(ad, comm=_Two(), backend=BE)
    assert not ad.obsm and not ad.varm and "pca" not in ad.uns

    # key_added, copy, layer, mask_var by name and as an array, use_highly_variable=False, svd_solver spellings
    mask = np.random.default_rng(5).random(d) < 0.6
    mask[:8] = True
    ad.var["keep"] = mask
    ad.var["highly_variable"] = ~mask
    ad.layers["L"] = X.copy()
    out = mu.tl.pca(ad, n_comps=7, mask_var="keep", key_added="mine", copy=True, layer="L", svd_solver="arpack",
                    oversample=9, backend=BE)
    assert out is not ad and not ad.obsm and set(out.obsm) == {"mine"} and set(out.varm) == {"mine"}
    assert out.uns["mine"]["params"]["mask_var"] == "keep" and out.uns["mine"]["params"]["layer"] == "L"
    assert not out.varm["mine"][~mask].any() and out.varm["mine"][mask].any()
    assert mu.tl.pca(ad, n_comps=7, mask_var=mask, svd_solver="auto", oversample=9, backend=BE) is None
    assert np.array_equal(ad.varm["PCs"], out.varm["mine"]) and np.array_equal(ad.obsm["X_pca"], out.obsm["mine"])
    assert ad.uns["pca"]["params"]["use_highly_variable"] is False
    mu.tl.pca(ad, n_comps=7, use_highly_variable=False, oversample=9, backend=BE)
    assert ad.varm["PCs"].all(axis=1).sum() > mask.sum()  # every gene takes part
    # the default number of components
    small = AnnData(X[:40, :30].copy())
    mu.tl.pca(small, backend=BE)
    assert small.obsm["X_pca"].shape == (40, 29)
    dense = AnnData(X[:60, :50].toarray())
    mu.tl.pca(dense, n_comps=5)  # a dense matrix: the host route
    assert dense.obsm["X_pca"].shape == (60, 5)


# ---- normalize_total / log1p -------------------------------------------------------------------------------------------
def _messy_counts(dtype):
    """300 x 200 counts with a zero-total cell that stores zeros, a cell without entries and an all-zero gene."""
    X = fx.counts(900, 700, 21)[:300, :200].tolil(copy=True)
    X[:, 17] = 0
    X[5, :] = 0
    X[9, :] = 0
    X = sp.csr_matrix(X, dtype=dtype)
    X.eliminate_zeros()
    row9 = sp.csr_matrix((np.zeros(3, dtype), np.array([2, 40, 41]), np.array([0, 3])), shape=(1, 200))
    X = sp.vstack([X[:9], row9, X[10:]], format="csr")
    X.indices, X.indptr = X.indices.astype(np.int32), X.indptr.astype(np.int64)
    assert X[9].nnz == 3 and X[5].nnz == 0 and X[:, 17].nnz == 0
    return X


def _uncanonical(kind, dtype=np.float32):
    C = _messy_counts(dtype)
    return fx.uncanonical(C, kind), C


@pytest.mark.parametrize("backend", [BE, None], ids=["cpu_set", "host"])
@pytest.mark.parametrize("kind", ["unsorted", "duplicates"])
def test_uncanonical_csr_is_canonicalised_first(backend, kind):
    """Unsorted column indices and duplicate entries: every step computes what it computes on the canonical matrix - the
    values belong to the index arrays they come back with - and the caller's matrix is not changed."""
    M, C = _uncanonical(kind)
    keep = (M.data.copy(), M.indices.copy(), M.indptr.copy())
    ad, ref = AnnData(M), AnnData(C.copy())
    out = rna.pp.normalize_total(ad, target_sum=100.0, inplace=False, backend=backend)
    assert all(np.array_equal(a, b) for a, b in zip(keep, (M.data, M.indices, M.indptr)))
    dense = fx.normalize_f64(C, 100.0)[0].toarray()
    assert _same_pattern(out["X"], C) and np.max(np.abs(out["X"].toarray() - dense)) <= 1e-5
    for a in (ad, ref):
        rna.pp.normalize_total(a, target_sum=100.0, backend=backend)
        rna.pp.log1p(a, backend=backend)
        rna.pp.highly_variable_genes(a, n_top_genes=30, backend=backend)
        mu.tl.pca(a, n_comps=5, use_highly_variable=False, oversample=9, backend=backend)
    assert _same_pattern(ad.X, C) and ad.X.has_sorted_indices and np.array_equal(ad.X.data, ref.X.data)
    assert _ulps32(ad.X.data, fx.log1p_f64(fx.normalize_f64(C, 100.0)[0].astype(np.float32)).data) <= 2
    for col in ("means", "dispersions", "dispersions_norm", "highly_variable"):
        assert np.array_equal(ad.var[col].values, ref.var[col].values, equal_nan=col != "highly_variable")
    assert np.array_equal(ad.obsm["X_pca"], ref.obsm["X_pca"])
    # log1p and highly_variable_genes straight on such a matrix (they are not linear in the stored parts)
    L = fx.log1p_f64(fx.normalize_f64(C, 100.0)[0]).astype(np.float32)
    order = np.concatenate([np.arange(L.indptr[i], L.indptr[i + 1])[::-1] for i in range(L.shape[0])])
    Lu = sp.csr_matrix((L.data[order], L.indices[order], L.indptr.copy()), shape=L.shape)
    a, b = AnnData(Lu), AnnData(L.copy())
    for x in (a, b):
        rna.pp.highly_variable_genes(x, backend=backend)
    assert np.array_equal(a.var["dispersions_norm"].values, b.var["dispersions_norm"].values, equal_nan=True)
    M2, C2 = _uncanonical(kind)
    a2 = AnnData(M2)
    rna.pp.log1p(a2, backend=backend)
    assert _same_pattern(a2.X, C2) and _ulps32(a2.X.data, fx.log1p_f64(C2).data) <= 2


@pytest.mark.parametrize("backend", [BE, None], ids=["cpu_set", "host"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("target", [None, 1e4])
def test_normalize_total_and_log1p_against_the_statement(backend, dtype, target):
    X = _messy_counts(dtype)
    ad = AnnData(X.copy())
    assert rna.pp.normalize_total(ad, target_sum=target, key_added="n_counts", backend=backend) is None
    ref, tot = fx.normalize_f64(X, target)
    assert ad.X.dtype == dtype and _same_pattern(ad.X, X)
    assert np.array_equal(ad.obs["n_counts"].values, tot)
    assert np.array_equal(ad.X[9].data, np.zeros(3, dtype))  # the zero-total cell is left as it is
    if dtype == np.float32:
        assert _ulps32(ad.X.data, ref.data) <= 2
    else:
        assert np.all(np.abs(ad.X.data - ref.data) <= 4 * U53 * np.abs(ref.data))
    assert (resident(ad.X, BE) is not None) == (backend is not None)
    for base in (None, 2):
        a2 = ad.copy()
        start = a2.X.copy()
        assert rna.pp.log1p(a2, base=base, backend=backend) is None
        refl = fx.log1p_f64(start, base)
        assert a2.uns["log1p"] == {"base": base} and a2.X.dtype == dtype and _same_pattern(a2.X, X)
        if dtype == np.float32:
            assert _ulps32(a2.X.data, refl.data) <= 2
        else:
            assert np.all(np.abs(a2.X.data - refl.data) <= 4 * U53 * np.abs(refl.data))


def test_normalize_total_options():
    X = _messy_counts(np.float32)
    ad = AnnData(X.copy(), layers={"raw": X.copy()})
    out = rna.pp.normalize_total(ad, inplace=False, backend=BE)
    ref, tot = fx.normalize_f64(X)
    assert set(out) == {"X", "norm_factor"} and np.array_equal(out["norm_factor"], tot)
    assert _ulps32(out["X"].data, ref.data) <= 2
    assert np.array_equal(ad.X.data, X.data) and "log1p" not in ad.uns and not len(ad.obs.columns)
    cp = rna.pp.normalize_total(ad, copy=True, backend=BE)
    assert cp is not ad and np.array_equal(ad.X.data, X.data) and np.array_equal(cp.X.data, out["X"].data)
    rna.pp.normalize_total(ad, layer="raw", target_sum=100.0, backend=BE)
    assert np.array_equal(ad.X.data, X.data)
    assert _ulps32(ad.layers["raw"].data, fx.normalize_f64(X, 100.0)[0].data) <= 2
    lg = rna.pp.log1p(ad, layer="raw", copy=True, backend=BE)
    assert lg is not ad and "log1p" not in ad.uns and lg.uns["log1p"] == {"base": None}
    with pytest.raises(NotImplementedError):
        rna.pp.normalize_total(ad, exclude_highly_expressed=True, backend=BE)
    with pytest.raises(TypeError, match="'rna' modality"):
        rna.pp.normalize_total(MuData({"atac": ad}), backend=BE)
    with pytest.raises(TypeError, match="'rna' modality"):
        rna.pp.log1p(3.0)
    with pytest.raises(TypeError, match="'rna' modality"):
        rna.pp.highly_variable_genes(MuData({"prot": ad}))

    class _Two:
        world_size = 2

    for fn in (rna.pp.normalize_total, rna.pp.log1p, rna.pp.highly_variable_genes):
        with pytest.raises(NotImplementedError, match="runs on one rank"):
            fn(ad, comm=_Two(), backend=BE)


@pytest.mark.parametrize("backend", [BE, None], ids=["cpu_set", "host"])
def test_integer_and_dense_input_and_mudata(backend):
    Xi = sp.csr_matrix(_messy_counts(np.float64).astype(np.int64))
    ad = AnnData(Xi.copy())
    md = MuData({"rna": ad, "other": AnnData(np.ones((Xi.shape[0], 2)))})
    rna.pp.normalize_total(md, backend=backend)
    assert md.mod["rna"].X.dtype == np.float32  # integers become float32
    ref, _ = fx.normalize_f64(Xi)
    assert _ulps32(md.mod["rna"].X.data, ref.data) <= 2
    rna.pp.log1p(md, backend=backend)
    refl = fx.log1p_f64(fx.normalize_f64(Xi)[0].astype(np.float32))
    assert _ulps32(md.mod["rna"].X.data, refl.data) <= 2
    rna.pp.highly_variable_genes(md, n_top_genes=30, backend=backend)
    assert int(md.mod["rna"].var["highly_variable"].sum()) >= 30
    # a dense matrix runs on the host, whatever the backend
    dn = AnnData(Xi.toarray())
    rna.pp.normalize_total(dn, backend=backend)
    rna.pp.log1p(dn, backend=backend)
    assert dn.X.dtype == np.float32 and _ulps32(dn.X[dn.X != 0], refl.data[refl.data != 0]) <= 2
    rna.pp.highly_variable_genes(dn, n_top_genes=30, backend=backend)
    assert np.array_equal(dn.var["highly_variable"].values, md.mod["rna"].var["highly_variable"].values)


# ---- highly_variable_genes ----------------------------------------------------------------------------------------------
def _hvg_restated(L, base, n_bins):
    """Flavor "seurat" in plain loops: L the dense log-normalised matrix (f64)."""
    n, d = L.shape
    E = np.expm1(L * (np.log(base) if base is not None else 1.0))
    means, disps = np.empty(d), np.empty(d)
    for j in range(d):
        col = E[:, j]
        m = col.sum() / n
        v = ((col - m) ** 2).sum() / (n - 1)
        if m == 0:
            m = 1e-12
        q = v / m
        disps[j] = np.log(q) if q != 0 else np.nan
        means[j] = np.log1p(m)
    lo, hi = means.min(), means.max()
    edges = [lo + (hi - lo) * i / n_bins for i in range(n_bins + 1)]
    edges[0] -= (hi - lo) * 0.001  # pandas.cut: the lowest edge moves out by 0.1 % of the range; intervals (a, b]
    norm = np.full(d, np.nan)
    for b in range(n_bins):
        last = b == n_bins - 1
        inside = [j for j in range(d) if edges[b] < means[j] and (means[j] <= edges[b + 1] or (last and means[j] <= hi))]
        vals = [disps[j] for j in inside if not np.isnan(disps[j])]
        if len(vals) >= 2:
            bm = sum(vals) / len(vals)
            bs = (sum((x - bm) ** 2 for x in vals) / (len(vals) - 1)) ** 0.5
        elif len(vals) == 1:
            bm, bs = 0.0, vals[0]  # a bin with one gene: std = that bin's mean, mean = 0
        else:
            continue
        for j in inside:
            with np.errstate(divide="ignore", invalid="ignore"):
                norm[j] = np.float64(disps[j] - bm) / np.float64(bs)
    return means, disps, norm


@pytest.mark.parametrize("backend", [BE, None], ids=["cpu_set", "host"])
@pytest.mark.parametrize("base", [None, 2])
def test_hvg_against_the_restatement(backend, base):
    X = _messy_counts(np.float32)
    L = fx.log1p_f64(fx.normalize_f64(X)[0], base)
    ad = AnnData(sp.csr_matrix(L.astype(np.float32)), uns={"log1p": {"base": base}})
    L32 = ad.X.toarray().astype(np.float64)
    means, disps, norm = _hvg_restated(L32, base, 20)
    assert rna.pp.highly_variable_genes(ad, backend=backend) is None
    assert ad.uns["hvg"] == {"flavor": "seurat"}
    np.testing.assert_allclose(ad.var["means"].values, means, rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(ad.var["dispersions"].values, disps, rtol=0, atol=1e-11, equal_nan=True)
    np.testing.assert_allclose(ad.var["dispersions_norm"].values, norm, rtol=0, atol=1e-9, equal_nan=True)
    assert np.isnan(ad.var["dispersions_norm"].values[17]) and not ad.var["highly_variable"].values[17]
    with np.errstate(invalid="ignore"):
        sel = (means > 0.0125) & (means < 3) & (norm > 0.5) & (norm < np.inf)
    assert np.array_equal(ad.var["highly_variable"].values, sel) and 0 < sel.sum() < sel.size
    # n_top_genes: >= the cutoff value; inplace=False returns the frame and touches nothing
    before = ad.var.copy()
    df = rna.pp.highly_variable_genes(ad, n_top_genes=25, inplace=False, backend=backend)
    assert isinstance(df, pd.DataFrame) and ad.var.equals(before)
    cut = np.sort(norm[~np.isnan(norm)])[::-1][24]
    assert np.array_equal(df["highly_variable"].values, np.nan_to_num(norm, nan=-np.inf) >= cut)
    assert df["highly_variable"].sum() >= 25
    with pytest.warns(UserWarning, match="n_top_genes"):
        df = rna.pp.highly_variable_genes(ad, n_top_genes=10 ** 6, inplace=False, backend=backend)
    assert np.array_equal(df["highly_variable"].values, ~np.isnan(norm))
    for kw in ({"flavor": "seurat_v3"}, {"flavor": "cell_ranger"}, {"batch_key": "batch"}):
        with pytest.raises(NotImplementedError):
            rna.pp.highly_variable_genes(ad, backend=backend, **kw)


@pytest.mark.parametrize("backend", [BE, None], ids=["cpu_set", "host"])
def test_hvg_hand_computed(backend):
    """6 genes, 4 cells, 3 bins.  e = expm1(x):
      g0 0 0 0 0     mean 0 -> 1e-12, disp 0 -> NaN                           bin 0
      g1 0 0 0 2     mean 1/2, var 1,    disp 2,    log 2                     bin 0
      g2 0 0 1 1     mean 1/2, var 1/3,  disp 2/3,  log 2/3                   bin 0   (means log 1.5 = 0.405)
      g3 1 1 1 5     mean 2,   var 4,    disp 2,    log 2                     bin 1   (means log 3 = 1.099)
      g4 0 0 4 4     mean 2,   var 16/3, disp 8/3,  log 8/3                   bin 1
      g5 2 2 10 10   mean 6,   var 64/3, disp 32/9, log 32/9                  bin 2   (means log 7 = 1.946), alone
    Bin edges of pandas.cut over [1e-12, log 7]: 0.6486, 1.2973.  Two genes in a bin: (x - mean) / std = +- 1 / sqrt 2.
    The single gene: std = its dispersion, mean = 0 -> 1."""
    E = np.array([[0, 0, 0, 1, 0, 2], [0, 0, 0, 1, 0, 2], [0, 0, 1, 1, 4, 10], [0, 2, 1, 5, 4, 10]], dtype=np.float64)
    ad = AnnData(sp.csr_matrix(np.log1p(E)))
    rna.pp.highly_variable_genes(ad, n_bins=3, backend=backend)
    r = 1 / np.sqrt(2)
    np.testing.assert_allclose(ad.var["means"].values, np.log1p([1e-12, 0.5, 0.5, 2, 2, 6]), rtol=1e-12)
    np.testing.assert_allclose(ad.var["dispersions"].values, np.log([np.nan, 2, 2 / 3, 2, 8 / 3, 32 / 9]), rtol=1e-12,
                               atol=1e-14, equal_nan=True)
    np.testing.assert_allclose(ad.var["dispersions_norm"].values, [np.nan, r, -r, -r, r, 1.0], rtol=1e-12,
                               equal_nan=True)
    assert list(ad.var["highly_variable"].values) == [False, True, False, False, True, True]
    rna.pp.highly_variable_genes(ad, n_bins=3, n_top_genes=1, backend=backend)
    assert list(ad.var["highly_variable"].values) == [False, False, False, False, False, True]
    rna.pp.highly_variable_genes(ad, n_bins=3, n_top_genes=3, backend=backend)
    assert list(ad.var["highly_variable"].values) == [False, True, False, False, True, True]


@pytest.mark.parametrize("backend", [BE, None], ids=["cpu_set", "host"])
def test_hvg_subset_follows_on_the_device(backend):
    X = _messy_counts(np.float32)
    ad = AnnData(X.copy(), layers={"counts": X.copy()})
    ad.varm["w"] = np.arange(X.shape[1] * 2.0).reshape(-1, 2)
    rna.pp.normalize_total(ad, backend=backend)
    rna.pp.log1p(ad, backend=backend)
    full = ad.X.copy()
    rna.pp.highly_variable_genes(ad, n_top_genes=40, subset=True, backend=backend)
    keep = ad.var["highly_variable"].values
    assert keep.all() and 40 <= ad.shape[1] < X.shape[1] and ad.varm["w"].shape[0] == ad.shape[1]
    assert ad.layers["counts"].shape == ad.shape
    ref = AnnData(full.copy())
    rna.pp.highly_variable_genes(ref, n_top_genes=40, backend=backend)
    sel = ref.var["highly_variable"].values
    assert np.array_equal(ad.X.toarray(), full[:, sel].toarray())
    Xd = resident(ad.X, BE)
    assert (Xd is not None) == (backend is not None)
    if Xd is not None:
        assert Xd.shape == ad.shape and np.array_equal(BE.to_host(Xd.values), ad.X.data)
        assert np.array_equal(BE.to_host(Xd.indices), ad.X.indices)


# ---- the resident pipeline ----------------------------------------------------------------------------------------------
def test_pipeline_uploads_once():
    be = CpuTestBackend()
    uploads = []
    orig = be.upload_csr
    be.upload_csr = lambda *a, **k: (uploads.append(1), orig(*a, **k))[1]
    ad = AnnData(fx.case_counts("wide").copy())
    rna.pp.normalize_total(ad, backend=be)
    assert len(uploads) == 1
    rna.pp.log1p(ad, backend=be)
    rna.pp.highly_variable_genes(ad, n_top_genes=600, backend=be)
    mu.tl.pca(ad, n_comps=7, oversample=9, backend=be)
    assert len(uploads) == 1  # every later step started from the copy the step before left
    assert ad.uns["pca"]["params"]["use_highly_variable"] and ad.obsm["X_pca"].shape == (700, 7)
    # ... and without backend= the copy's own backend serves
    ad2 = AnnData(fx.case_counts("wide").copy())
    rna.pp.normalize_total(ad2, backend=be)
    rna.pp.log1p(ad2)
    rna.pp.highly_variable_genes(ad2, n_top_genes=600)
    mu.tl.pca(ad2, n_comps=7, oversample=9)
    assert len(uploads) == 2 and np.array_equal(ad2.obsm["X_pca"], ad.obsm["X_pca"])
    # the same steps on the host alone agree to the precision of the f32 process
    ad3 = AnnData(fx.case_counts("wide").copy())
    rna.pp.normalize_total(ad3)
    rna.pp.log1p(ad3)
    rna.pp.highly_variable_genes(ad3, n_top_genes=600)
    mu.tl.pca(ad3, n_comps=7)
    assert len(uploads) == 2 and np.array_equal(ad3.var["highly_variable"].values, ad.var["highly_variable"].values)
    from oracle.lsi_oracle import max_subspace_angle

    assert max_subspace_angle(ad3.varm["PCs"], ad.varm["PCs"]) < ANGLE
    np.testing.assert_allclose(ad3.uns["pca"]["variance"], ad.uns["pca"]["variance"], rtol=VAR_RTOL)


# ---- lsi is what it was --------------------------------------------------------------------------------------------------
def test_lsi_reaches_the_operators_it_reached(monkeypatch):
    """``atac.tl.lsi`` without an operand: byte-equal to a run in which the basis' image is again the plain product it
    was before the operand existed, and none of the new operators is reached."""
    from muon_amd._atac import tools

    class Traced(CpuTestBackend):
        def __init__(self):
            self.calls = []

        def __getattribute__(self, name):
            if name in ("spmm", "gram", "gram_cross", "apply", "transpose", "project_out_block", "randn"):
                object.__getattribute__(self, "calls").append(name)
            return object.__getattribute__(self, name)

    def run():
        be = Traced()
        ad = AnnData(fx.lognorm("wide").astype(np.float32))
        warnings.simplefilter("ignore")
        mu.atac.tl.lsi(ad, n_comps=7, backend=be)
        return ad, be.calls

    new, calls_new = run()
    monkeypatch.setattr(tools._KrylovBasis, "_image", lambda self, X, Q: self.backend.spmm(X, Q))
    old, calls_old = run()
    assert calls_new == calls_old
    for slot, key in (("obsm", "X_lsi"), ("varm", "LSI")):
        assert getattr(new, slot)[key].tobytes() == getattr(old, slot)[key].tobytes()
    assert new.uns["lsi"]["stdev"].tobytes() == old.uns["lsi"]["stdev"].tobytes()
    for op in ("shift_cols", "scale_rows", "gene_moments", "value_sweep"):
        assert getattr(CpuTestBackend, op) is None  # the CPU set has none of them: a call would have raised


def test_the_library_declares_the_new_entry_points():
    from muon_amd import _ffi
    from muon_amd._operators import DECLARED

    for name in ("mu_gene_moments", "mu_gene_moments_max_blocks", "mu_rna_value_sweep", "mu_shift_cols_f32",
                 "mu_scale_rows_f32"):
        assert name in _ffi.SIGNATURES
    assert {"gene_moments", "gene_moments_max_blocks", "value_sweep", "shift_cols", "scale_rows"} <= DECLARED
    assert _ffi.lib().mu_version() >= 811
