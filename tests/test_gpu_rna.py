"""muon_amd.rna.pp and muon_amd.tl.pca on the device: the kernels of csrc/rna.hip at their edges and every case of
tests/golden/rna_golden.npz (scikit-learn 1.7.2 on the densified matrix) end to end.

  * gene moments: a derived bound against a ``np.longdouble`` restatement, valid for any order of the additions:
    |sum - ref| <= (len + 64) 2^-53 sum|terms|, and 4 * 2^-53 sum|terms| more for libm's expm1 in the e sums.
  * ``shift_cols`` / ``scale_rows``: bit-equal to numpy's f32 subtraction / product; padding columns come back untouched.
  * the value sweep: within 2 ulp of f32 (f32 values) and 4 * 2^-53 relative (f64) of the f64 statement.
  * every kernel and a whole ``pca`` call, run twice, are byte-equal.
  * PCA: subspaces of ``PCs`` and ``X_pca`` and the explained variances against the golden, never against the host
    route.  The bounds are ten times the worst case measured on an MI355X (PARITY_MEASURED below); the
    sanity ceiling is a condition, not a measurement: no angle bound above lsi's 1e-4, no variance rtol above 1e-5.
"""
import numpy as np
import pytest
import torch

import muon_amd as mu
from muon_amd import AnnData, rna
from muon_amd._hostmatrix import resident
from muon_amd._backend import DeviceCSR
from tests import rna_fixture as fx

pytestmark = pytest.mark.gpu

# (angle of PCs, angle of X_pca, variance, variance_ratio) measured on an MI355X, per case
PARITY_MEASURED = {
    "b16": (7.36e-06, 2.17e-06, 2.02e-08, 1.85e-08), "b16_scale": (2.79e-07, 2.27e-07, 2.53e-08, 2.53e-08),
    "b32": (4.59e-07, 3.21e-07, 2.85e-08, 2.90e-08), "b32_scale": (3.01e-06, 1.38e-06, 2.74e-08, 2.74e-08),
    "b64": (2.13e-06, 1.27e-06, 2.71e-08, 1.93e-08), "wide": (9.32e-07, 2.80e-07, 3.81e-08, 3.78e-08),
    "masked": (3.34e-07, 2.27e-07, 2.41e-08, 2.62e-08), "uncentred": (8.18e-06, 2.42e-06, 1.12e-07, 1.10e-07),
}
ANGLE = min(10 * max(max(v[:2]) for v in PARITY_MEASURED.values()), 1e-4)   # 8.2e-5
VAR_RTOL = min(10 * max(max(v[2:]) for v in PARITY_MEASURED.values()), 1e-5)  # 1.1e-6
assert ANGLE <= 1e-4 and VAR_RTOL <= 1e-5
U53 = 2.0 ** -53
LENS = (0, 1, 63, 64, 65, 129, 1000)


def _gene_rows(n_cells, dtype, seed):
    """X^T as a CSR: three rounds of genes with 0, 1, 63, 64, 65, 129 and 1000 entries (those that fit n_cells), values
    of both signs and explicitly stored zeros."""
    rng = np.random.default_rng(seed)
    lens = [l for l in LENS if l <= n_cells] * 3
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = np.concatenate([np.sort(rng.choice(n_cells, l, replace=False)) for l in lens] + [np.zeros(0)]).astype(np.int32)
    val = (rng.standard_normal(int(indptr[-1])) * 3).astype(dtype)
    val[rng.random(val.size) < 0.1] = 0
    return indptr, idx, val, lens


@pytest.mark.parametrize("n_cells", [1, 70, 1100])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("max_blocks", [0, 2])
def test_gene_moments(hip, n_cells, dtype, max_blocks):
    indptr, idx, val, lens = _gene_rows(n_cells, dtype, n_cells)
    d, c = len(lens), 0.37
    assert d > 8 or n_cells == 1  # two workgroups of four waves walk more than one round of genes
    Xt = hip.upload_csr(indptr, idx, val, (d, n_cells), slab_ptr=False)
    assert hip.gene_moments_max_blocks() >= 2
    for with_e in (True, False):
        sums, cnt = hip.gene_moments(Xt, c=c, with_e=with_e, max_blocks=max_blocks)
        again = hip.gene_moments(Xt, c=c, with_e=with_e, max_blocks=max_blocks)
        assert torch.equal(sums, again[0]) and torch.equal(cnt, again[1])
        sums, cnt = hip.to_host(sums), hip.to_host(cnt)
        for j in range(d):
            x = val[indptr[j]:indptr[j + 1]].astype(np.longdouble)
            e = np.expm1(x * np.longdouble(c))
            slack = (lens[j] + 64) * U53
            for row, terms, extra in ((0, x, 0.0), (1, x * x, 0.0), (2, e, 4 * U53), (3, e * e, 4 * U53)):
                if row >= 2 and not with_e:
                    assert sums[row, j] == 0
                    continue
                assert abs(np.longdouble(sums[row, j]) - terms.sum()) <= (slack + extra) * np.abs(terms).sum(), (j, row)
            assert cnt[j] == np.count_nonzero(x)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("B", [16, 32, 64])
def test_shift_cols_and_scale_rows_bit_equal(hip, n, B):
    rng = np.random.default_rng(n * 100 + B)
    w = B - 3
    Y = rng.standard_normal((n, B)).astype(np.float32)
    Y[:, w:] = 0
    m = np.zeros(B)
    m[:w] = rng.standard_normal(w) * 1e-3 + 0.7
    ref = Y - m.astype(np.float32)
    Yd = hip.to_device(Y)
    out = hip.shift_cols(Yd, hip.to_device(m, np.float64))
    assert out.data_ptr() == Yd.data_ptr()
    got = hip.to_host(Yd)
    assert got.tobytes() == ref.tobytes() and not got[:, w:].any()
    Y2 = hip.to_device(Y)
    hip.shift_cols(Y2, hip.to_device(m, np.float64))
    assert torch.equal(Y2, Yd)

    s = (rng.random(n) + 0.5).astype(np.float32)
    ref = s[:, None] * Y
    Qd = hip.to_device(Y)
    got = hip.scale_rows(hip.to_device(s), Qd)
    assert hip.to_host(got).tobytes() == ref.tobytes() and hip.to_host(Qd).tobytes() == Y.tobytes()
    assert not hip.to_host(got)[:, w:].any()
    hip.scale_rows(hip.to_device(s), Qd, out=Qd)  # in place
    assert torch.equal(Qd, got)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_value_sweep(hip, dtype):
    rng = np.random.default_rng(7)
    lens = [0, 1, 64, 65, 257, 0, 3] * 40  # more rows than one round of the grid's waves on a small grid
    n, d = len(lens), 300
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = np.concatenate([np.sort(rng.choice(d, l, replace=False)) for l in lens]).astype(np.int32)
    val = rng.gamma(2.0, 3.0, int(indptr[-1])).astype(dtype)
    val[rng.random(val.size) < 0.05] = 0
    div = rng.random(n) * 4 + 0.25
    X = hip.upload_csr(indptr, idx, val, (n, d), slab_ptr=False)
    rows = np.repeat(np.arange(n), lens)
    v64 = val.astype(np.float64)
    cases = [(dict(div=div), v64 / div[rows]), (dict(log=True), np.log1p(v64)),
             (dict(log=True, log_div=float(np.log(2))), np.log1p(v64) / np.log(2)),
             (dict(div=div, log=True, log_div=float(np.log(10))), np.log1p(v64 / div[rows]) / np.log(10))]
    for kw, ref in cases:
        if "div" in kw:
            kw = dict(kw, div=hip.to_device(div, np.float64))
        got = hip.value_sweep(X, **kw)
        assert torch.equal(got, hip.value_sweep(X, **kw))
        g = hip.to_host(got)
        assert g.dtype == dtype and hip.to_host(X.values).tobytes() == val.tobytes()
        if dtype == np.float32:
            ref32 = ref.astype(np.float32)
            assert np.max(np.abs(g.astype(np.float64) - ref) / np.spacing(np.abs(ref32))) <= 2
        else:
            assert np.all(np.abs(g - ref) <= 4 * U53 * np.abs(ref))
        assert not g[val == 0].any()
        # in place
        Xc = DeviceCSR(X.indptr, X.indices, X.values.clone(), X.shape)
        hip.value_sweep(Xc, out=Xc.values, **kw)
        assert torch.equal(Xc.values, got)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_normalize_log1p_on_the_device(hip, dtype):
    X = fx.case_counts("wide").astype(dtype)
    ad = AnnData(X.copy())
    rna.pp.normalize_total(ad, backend=hip)
    ref, _tot = fx.normalize_f64(X)
    start = ad.X.copy()
    rna.pp.log1p(ad, backend=hip)
    refl = fx.log1p_f64(start)
    for got, r in ((start, ref), (ad.X, refl)):
        assert np.array_equal(got.indptr, X.indptr) and np.array_equal(got.indices, X.indices) and got.dtype == dtype
        if dtype == np.float32:
            assert np.max(np.abs(got.data.astype(np.float64) - r.data) / np.spacing(np.abs(r.data.astype(np.float32)))) <= 2
        else:
            assert np.all(np.abs(got.data - r.data) <= 4 * U53 * np.abs(r.data))
    Xd = resident(ad.X, hip)
    assert Xd is not None and np.array_equal(hip.to_host(Xd.values), ad.X.data)


@pytest.mark.parametrize("kind", ["unsorted", "duplicates"])
def test_uncanonical_csr_is_canonicalised_first(hip, kind):
    """Unsorted column indices / duplicate entries: the steps compute what they compute on the canonical matrix, the
    values come back with the index arrays they belong to, and the caller's matrix is not changed."""
    C = fx.case_counts("wide")[:300].copy()
    C.indices, C.indptr = C.indices.astype(np.int32), C.indptr.astype(np.int64)
    M = fx.uncanonical(C, kind)
    keep = (M.data.copy(), M.indices.copy(), M.indptr.copy())
    ad, ref = AnnData(M), AnnData(C.copy())
    for a in (ad, ref):
        rna.pp.normalize_total(a, target_sum=100.0, backend=hip)
        rna.pp.log1p(a, backend=hip)
        rna.pp.highly_variable_genes(a, n_top_genes=200, backend=hip)
    assert all(np.array_equal(x, y) for x, y in zip(keep, (M.data, M.indices, M.indptr)))
    assert np.array_equal(ad.X.indptr, C.indptr) and np.array_equal(ad.X.indices, C.indices)
    assert np.array_equal(ad.X.data, ref.X.data)
    r = fx.log1p_f64(fx.normalize_f64(C, 100.0)[0].astype(np.float32)).data
    assert np.max(np.abs(ad.X.data.astype(np.float64) - r) / np.spacing(np.abs(r.astype(np.float32)))) <= 2
    assert np.array_equal(ad.var["dispersions_norm"].values, ref.var["dispersions_norm"].values, equal_nan=True)
    Xd = resident(ad.X, hip)
    assert Xd is not None and np.array_equal(hip.to_host(Xd.indices), C.indices)


@pytest.mark.parametrize("name", list(fx.CASES))
def test_pca_golden(hip, name):
    ad, diag = fx.run_case(mu, name, hip)
    assert diag["block"] == fx.CASES[name]["block"] and diag["converged"]
    a_pcs, a_x, v, r = fx.deviations(name, ad)
    print(f"PARITY {name}: ({a_pcs:.2e}, {a_x:.2e}, {v:.2e}, {r:.2e}) iterations {diag['iterations']} spmm {diag['spmm']}")
    assert a_pcs < ANGLE and a_x < ANGLE and v < VAR_RTOL and r < VAR_RTOL


def test_pca_repeats_byte_equal(hip):
    for name in ("b16_scale", "b64"):
        a, _ = fx.run_case(mu, name, hip)
        b, _ = fx.run_case(mu, name, hip)
        for slot, key in (("obsm", "X_pca"), ("varm", "PCs")):
            assert getattr(a, slot)[key].tobytes() == getattr(b, slot)[key].tobytes()
        assert a.uns["pca"]["variance"].tobytes() == b.uns["pca"]["variance"].tobytes()


def test_resident_pipeline_uploads_once(hip):
    uploads = []
    orig = hip.upload_csr
    hip.upload_csr = lambda *a, **k: (uploads.append(1), orig(*a, **k))[1]
    try:
        ad = AnnData(fx.case_counts("b16").copy())
        rna.pp.normalize_total(ad, backend=hip)
        assert len(uploads) == 1
        rna.pp.log1p(ad, backend=hip)
        rna.pp.highly_variable_genes(ad, n_top_genes=500, backend=hip)
        mu.tl.pca(ad, n_comps=11, backend=hip)
        assert len(uploads) == 1
    finally:
        hip.upload_csr = orig
    # the host route on the matrix the device steps left: the same genes (the per-gene sums differ by their rounding)
    import scipy.sparse as sp

    ref = AnnData(sp.csr_matrix((ad.X.data.copy(), ad.X.indices.copy(), ad.X.indptr.copy()), shape=ad.X.shape))
    assert resident(ref.X, hip) is None
    rna.pp.highly_variable_genes(ref, n_top_genes=500)
    assert np.array_equal(ad.var["highly_variable"].values, ref.var["highly_variable"].values)
    np.testing.assert_allclose(ad.var["dispersions_norm"].values, ref.var["dispersions_norm"].values, rtol=0, atol=1e-9,
                               equal_nan=True)
    assert 500 <= int(ad.var["highly_variable"].sum()) < 900 and ad.obsm["X_pca"].shape == (1500, 11)
    assert not ad.varm["PCs"][~ad.var["highly_variable"].values].any()
