"""Size-independent properties at BASELINE.json's per-GPU size (125 000 cells x 200 000 peaks,
7.8e8 stored entries - far beyond what the CPU oracle finishes in seconds): round trips, adjoint
identities, checksums of checksums and eigen-residuals, all evaluated on the device."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, D = 125_000, 200_000


@pytest.fixture(scope="module")
def shard(hip):
    from muon_amd._atac.preproc import tfidf_device

    X = hip.synth_counts(0, N, D, 50, 0.03, 0)
    T = tfidf_device(hip, X, N, 3, 1e4)
    return X, T


@pytest.fixture(scope="module")
def shard10(hip):
    """The same size and model with 10 planted topics: n_comps = 10 at a spectral gap (with 50 topics the 10th value
    sits inside the planted cluster, where the 1e-4 angle, and with it the residual bars below, is not well posed)."""
    from muon_amd._atac.preproc import tfidf_device

    X = hip.synth_counts(0, N, D, 10, 0.03, 0)
    return X, tfidf_device(hip, X, N, 3, 1e4)


def _rows_of(X):
    counts = (X.indptr[1:] - X.indptr[:-1])
    return torch.repeat_interleave(torch.arange(X.shape[0], device=X.indptr.device), counts)


def test_tfidf_inverts_back_to_the_counts(hip, shard):
    """out = log1p(c / rowsum * 1e4) * log1p(n / colsum)  =>  c = expm1(out / idf) * rowsum / 1e4."""
    X, T = shard
    assert T.indices.data_ptr() == X.indices.data_ptr() or torch.equal(T.indices, X.indices)
    rows = _rows_of(X)
    cols = X.indices.long()
    c = X.values.double()
    rowsum = torch.zeros(N, dtype=torch.float64, device=c.device).index_add_(0, rows, c)
    colsum = torch.zeros(D, dtype=torch.float64, device=c.device).index_add_(0, cols, c)
    idf = torch.log1p(N / colsum)
    back = torch.expm1(T.values.double() / idf[cols]) * rowsum[rows] / 1e4
    assert torch.isfinite(T.values).all() and (T.values > 0).all()
    rel = ((back - c).abs() / c).max().item()
    assert rel < 2e-5, rel  # two f32 roundings of the forward pass, amplified by expm1


def test_stream_spmm_adjoint_and_checksums_full_size(hip, shard):
    _, T = shard
    Tp = hip.stream(T)
    Ttp = hip.transpose_stream(T)
    q = hip.randn(D, 64, 3)
    y = hip.randn(N, 64, 4)
    Yq = hip.spmm(Tp, q)
    Zy = hip.spmm(Ttp, y)
    lhs = (Yq.double() * y.double()).sum(dim=0)
    rhs = (q.double() * Zy.double()).sum(dim=0)
    assert torch.allclose(lhs, rhs, rtol=2e-5, atol=1e-4 * float(lhs.abs().max()))
    # X 1 = row sums, X^T 1 = column sums (checksum of checksums against index_add in f64)
    ones_d = torch.ones((D, 64), dtype=torch.float32, device=q.device)
    ones_n = torch.ones((N, 64), dtype=torch.float32, device=q.device)
    rows, cols, v = _rows_of(T), T.indices.long(), T.values.double()
    rs = torch.zeros(N, dtype=torch.float64, device=v.device).index_add_(0, rows, v)
    cs = torch.zeros(D, dtype=torch.float64, device=v.device).index_add_(0, cols, v)
    r1 = hip.spmm(Tp, ones_d)[:, 0].double()
    c1 = hip.spmm(Ttp, ones_n)[:, 7].double()
    assert ((r1 - rs).abs() / rs).max().item() < 2e-5
    nz = cs > 0
    assert ((c1[nz] - cs[nz]).abs() / cs[nz]).max().item() < 2e-5
    assert (c1[~nz] == 0).all()
    # bit-reproducible
    assert torch.equal(hip.spmm(Tp, q), Yq) and torch.equal(hip.spmm(Ttp, y), Zy)


def _eigen_residuals(hip, shard, k):
    """lsi_device with default settings on the shard (7.8e8 stored entries: above the 5e8 at which the warm start is on
    by default, on the ranged slice products); V orthonormal, singular values descending, X^T X v_i = s_i^2 v_i for
    the leading components to the accuracy a 1e-4 subspace angle implies; U has zero mean / unit variance."""
    from muon_amd._atac.tools import lsi_device

    _, T = shard
    U, stdev, V, info = lsi_device(hip, T, n_comps=k, return_info=True)
    assert info["warm_start"] is not None and info["warm_start"]["slice"] == "ranges", info["warm_start"]
    s = stdev * np.sqrt(N - 1)
    assert np.all(np.diff(s) <= 0) and info["converged"] and info["iterations"] <= 8, (info["iterations"], info["bounds"])
    Vd = V.double()
    G = Vd.T @ Vd
    assert (G - torch.eye(k, dtype=torch.float64, device=G.device)).abs().max().item() < 1e-5
    Vb = torch.zeros((D, 64), dtype=torch.float32, device=V.device)
    Vb[:, :k] = V
    W = hip.spmm(hip.transpose_stream(T), hip.spmm(hip.stream(T), Vb))[:, :k].double()
    s2 = torch.as_tensor(s**2, device=W.device)
    res = (W - Vd * s2).norm(dim=0) / s2
    # the trailing components sit next to the bulk: their residual is bounded by the angle target
    # times the spectral spread; the planted ones are far better
    assert res.max().item() < 2e-3, res.max().item()
    assert res[:min(40, k)].max().item() < 2e-4, res[:min(40, k)].max().item()
    Ud = U.double()
    assert Ud.mean(dim=0).abs().max().item() < 1e-3 and (Ud.std(dim=0, unbiased=False) - 1).abs().max().item() < 1e-3
    return info


def test_lsi_eigen_residuals_full_size(hip, shard):
    """n_comps = 50: block width 64."""
    _eigen_residuals(hip, shard, 50)


def test_lsi_eigen_residuals_full_size_narrow_block(hip, shard10):
    """n_comps = 10: block width 32 (pick_block(10 + 14)), what a user asking for fewer components at this shard size
    gets - the warm start's ranged slice products on a block narrower than their kernel."""
    info = _eigen_residuals(hip, shard10, 10)
    assert info["block"] == 32


def test_c4_sparse_view_products_with_the_narrow_block_kernel(hip):
    """BASELINE configs[3]'s sparse view (100 000 x 100 000 at 3 %) through csrc/spmm_narrow.hip, B = 16:
    the adjoint identity <X q, y> == <q, X^T y> across the two operands, the B = 64 kernel's NB = 1 instance
    as a second implementation, bit-reproducibility."""
    import torch

    from muon_amd._atac.preproc import tfidf_device

    n = d = 100_000
    X = tfidf_device(hip, hip.synth_counts(0, n, d, 50, 0.03, 0), n, 3, 1e4)
    P, Pt = hip.stream(X), hip.transpose_stream(X)
    q, y = hip.randn(d, 16, 5), hip.randn(n, 16, 6)
    Xq, Xty = hip.spmm(P, q), hip.spmm(Pt, y)
    lhs = (Xq.double() * y.double()).sum(dim=0)
    rhs = (q.double() * Xty.double()).sum(dim=0)
    assert torch.allclose(lhs, rhs, rtol=1e-5, atol=1e-5 * float(lhs.abs().max()))
    assert torch.equal(Xq, hip.spmm(P, q))
    try:
        hip.tune("spmm_narrow_off", 1)
        ref = hip.spmm(P, q)
    finally:
        hip.tune("spmm_narrow_off", 0)
    scale = float(ref.abs().max())
    assert float((Xq - ref).abs().max()) < 2e-5 * scale  # (two summation orders in f32)


def test_exhaustive_search_at_100k_cells(hip):
    """The filter-kernel search at the size of the WNN bench record: every sampled query's neighbours equal a
    dense evaluation of its row, distances ascending, nobody is its own neighbour."""
    import torch

    from muon_amd._core import preproc as pp

    n, p, k = 100_000, 50, 20
    rng = np.random.default_rng(2)
    lab = rng.integers(0, 30, n)
    X = hip.to_device(rng.standard_normal((30, p))[lab] * 2 + rng.standard_normal((n, p)))
    idx, dst = pp.device_knn(X, k, "euclidean", backend=hip)
    assert idx.shape == (n, k) and bool((idx != torch.arange(n, device=idx.device)[:, None]).all())
    assert bool((dst[:, 1:] >= dst[:, :-1]).all())
    rows = torch.as_tensor(rng.choice(n, 256, replace=False), device=X.device)
    D = torch.cdist(X[rows], X)
    D[torch.arange(rows.numel(), device=X.device), rows] = float("inf")
    want = torch.topk(D, k, dim=1, largest=False)
    assert torch.allclose(dst[rows], want.values, rtol=1e-10, atol=1e-10)
    assert torch.equal(torch.sort(idx[rows], dim=1).values, torch.sort(want.indices, dim=1).values)
