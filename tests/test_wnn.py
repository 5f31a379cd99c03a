"""muon.pp.neighbors (weighted nearest neighbours) and muon.pp.l2norm - host logic and the
tensor formulation on the CPU test operator set against oracle/wnn_oracle.py (exhaustive search, numpy
loops; the reference itself needs numba / umap / pynndescent / scanpy and has no test for this function)."""
import numpy as np
import pytest
import scipy.sparse as sp

import muon_amd as mu
from muon_amd import AnnData, MuData
from muon_amd._core import preproc as pp
from oracle import wnn_oracle
from tests.cpu_backend import CpuTestBackend

BE = CpuTestBackend()


def two_modalities(n=140, seed=0):
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, 4, n)
    c1 = rng.standard_normal((4, 8)) * 3
    c2 = rng.standard_normal((4, 6)) * 3
    c2[1] = c2[0]  # modality 2 cannot tell clusters 0 and 1 apart: modality 1 should win there
    x1 = c1[lab] + rng.standard_normal((n, 8))
    x2 = c2[lab] + rng.standard_normal((n, 6))
    return lab, x1, x2


def test_l2norm_dense_sparse_and_mudata():
    _, x1, x2 = two_modalities()
    a = AnnData(x1.copy())
    pp.l2norm(a, rep="X")
    np.testing.assert_allclose(np.linalg.norm(a.X, axis=1), 1.0, rtol=1e-12)
    s = sp.random(50, 30, density=0.2, format="csr", random_state=1) + sp.eye(50, 30, format="csr")
    b = AnnData(s.tocsr().astype(np.float64))
    pp.l2norm(b, rep="X")
    np.testing.assert_allclose(np.sqrt(np.asarray(b.X.multiply(b.X).sum(axis=1))).ravel(), 1.0, rtol=1e-12)
    # csc and coo are normalised in place too (reference preproc.py:194-195; r03 normalised a copy)
    for fmt in ("csc", "coo"):
        c = AnnData(s.asformat(fmt).astype(np.float64))
        pp.l2norm(c, rep="X")
        assert c.X.format == fmt
        np.testing.assert_allclose(np.sqrt(np.asarray(c.X.multiply(c.X).sum(axis=1))).ravel(), 1.0, rtol=1e-12)
        np.testing.assert_allclose(c.X.toarray(), b.X.toarray(), rtol=1e-12)
    md = MuData({"a": AnnData(x1.copy()), "b": AnnData(x2.copy())})
    out = pp.l2norm(md, rep="X", copy=True)
    assert out is not md and np.allclose(np.linalg.norm(out.mod["b"].X, axis=1), 1.0)
    assert not np.allclose(np.linalg.norm(md.mod["b"].X, axis=1), 1.0)
    with pytest.raises(RuntimeError):
        pp.l2norm(AnnData(x1.copy()), rep=["X", "X"])


def test_pair_distances_follow_scipy():
    """r04 (VERDICT r03 missing #5): every `metric` of the reference's signature (preproc.py:270-294) that scipy
    evaluates pair by pair - what the reference's final step calls through cdist (:596-606)."""
    import torch
    from scipy.spatial.distance import cdist

    rng = np.random.default_rng(5)
    real_a, real_b = rng.standard_normal((40, 9)), rng.standard_normal((40, 9))
    pos_a, pos_b = rng.random((40, 9)) + 0.01, rng.random((40, 9)) + 0.01
    pos_a[:, 2] = 0.0  # (zeros: canberra's 0/0 terms and the xlogy(0, .) terms of jensenshannon)
    pos_b[::2, 2] = 0.0
    bin_a, bin_b = (rng.random((40, 9)) < 0.5).astype(float), (rng.random((40, 9)) < 0.4).astype(float)
    bin_a[0], bin_b[0] = 0.0, 0.0  # (two empty rows: jaccard 0, yule 0)
    cnt_a, cnt_b = rng.integers(0, 3, (40, 9)).astype(float), rng.integers(0, 3, (40, 9)).astype(float)
    import scipy.spatial.distance as ssd
    for metric in pp._PAIR_METRICS:
        if metric in ("jensenshannon", "braycurtis", "canberra"):
            A, B = pos_a, pos_b
        elif metric in ("dice", "kulsinski", "rogerstanimoto", "russellrao", "sokalmichener", "sokalsneath", "yule"):
            A, B = bin_a, bin_b
        elif metric in ("hamming", "matching", "jaccard"):
            A, B = cnt_a, cnt_b
        else:
            A, B = real_a, real_b
        got = pp._pair_dist(torch.from_numpy(A), torch.from_numpy(B), metric).numpy()
        if metric == "kulsinski":  # (dropped from scipy 1.11+: its published definition)
            a, b = A != 0, B != 0
            ntt, dis = (a & b).sum(1), (a != b).sum(1)
            want = (dis - ntt + A.shape[1]) / (dis + A.shape[1])
        elif metric == "manhattan":
            want = np.diag(cdist(A, B, metric="cityblock"))
        elif metric in ("dice", "rogerstanimoto", "russellrao", "sokalmichener", "sokalsneath", "yule"):
            want = np.diag(cdist(A.astype(bool), B.astype(bool), metric=metric))
        else:
            want = np.diag(cdist(A, B, metric=metric))
        with np.errstate(invalid="ignore"):
            ok = np.isfinite(want)
        np.testing.assert_allclose(got[ok], want[ok], rtol=1e-12, atol=1e-14, err_msg=metric)
        assert np.array_equal(np.isnan(got), np.isnan(want)), metric
    for metric in ("mahalanobis", "seuclidean", "wminkowski"):  # (the first two: per cell, `_cell_dist`)
        with pytest.raises(NotImplementedError):
            pp._pair_dist(torch.from_numpy(real_a), torch.from_numpy(real_b), metric)


@pytest.mark.parametrize("metric", ["euclidean", "cosine", "cityblock", "correlation", "chebyshev", "canberra", "minkowski"])
def test_knn_matches_exhaustive_search(metric):
    _, x1, _ = two_modalities()
    a = AnnData(x1.copy())
    pp.knn(a, n_neighbors=12, use_rep="X", metric=metric, backend=BE)
    D, C, uns = wnn_oracle.knn_graph(x1, 12, metric)
    got = a.obsp["distances"]
    assert got.shape == D.shape and np.all(np.diff(got.indptr) == 11)
    assert (abs(got - D) > 1e-10).nnz == 0
    assert (abs(a.obsp["connectivities"] - C) > 1e-6).nnz == 0
    assert a.uns["neighbors"]["params"]["n_neighbors"] == 12 and a.uns["neighbors"]["distances_key"] == "distances"


def _run_both(n=140, seed=0, **kw):
    lab, x1, x2 = two_modalities(n, seed)
    md = MuData({"rna": AnnData(x1.copy()), "atac": AnnData(x2.copy())})
    for m in md.mod.values():
        pp.knn(m, n_neighbors=15, use_rep="X", backend=BE)
    pp.neighbors(md, backend=BE, **kw)
    graphs = {k: v.obsp["distances"] for k, v in md.mod.items()}
    okw = {k: v for k, v in kw.items() if k in ("n_neighbors", "n_bandwidth_neighbors", "n_multineighbors", "metric", "eps")}
    ref = wnn_oracle.neighbors({"rna": x1, "atac": x2}, graphs, **okw)
    return lab, md, ref


@pytest.mark.parametrize("kw", [dict(n_multineighbors=40), dict(n_multineighbors=30, n_neighbors=10, n_bandwidth_neighbors=12),
                                dict(n_multineighbors=40, metric="cityblock"),
                                dict(n_multineighbors=40, metric="correlation"),
                                dict(n_multineighbors=40, metric="braycurtis"),
                                dict(n_multineighbors=40, metric="seuclidean"),
                                dict(n_multineighbors=40, metric="mahalanobis")])
def test_wnn_matches_oracle(kw):
    lab, md, (D, C, W, sig, k) = _run_both(**kw)
    got = md.obsp["distances"]
    assert got.shape == D.shape and np.all(np.diff(got.indptr) == k + 1)
    assert np.array_equal(got.indices, D.indices)
    np.testing.assert_allclose(got.data, D.data, rtol=1e-6, atol=1e-9)
    assert (abs(md.obsp["connectivities"] - C) > 1e-5).nnz == 0
    np.testing.assert_allclose(md.obs["rna:mod_weight"].values, W[:, 0], rtol=1e-5)
    np.testing.assert_allclose(md.obs["atac:mod_weight"].values + md.obs["rna:mod_weight"].values, 1.0, rtol=1e-12)
    p = md.uns["neighbors"]["params"]
    assert p["n_neighbors"] == k and p["method"] == "umap" and p["use_rep"] == {"rna": "X", "atac": "X"}
    # where modality 2 cannot separate the clusters, modality 1 carries the weight
    w1 = md.obs["rna:mod_weight"].values
    assert w1[lab <= 1].mean() > w1[lab >= 2].mean()


def test_wnn_modalities_in_a_different_order_and_with_missing_cells():
    """r04 (VERDICT r03 missing #2): the modalities of a MuData object need not list the observations in the same
    order, and a modality may lack cells (reference preproc.py:381-384, :451, :546-575).  r03 raised."""
    import pandas as pd

    n = 130
    lab, x1, x2 = two_modalities(n, 3)
    names = np.array([f"c{i}" for i in range(n)])
    # (a) same cells, the second modality shuffled: identical graph and weights
    base = MuData({"rna": AnnData(x1.copy(), obs=pd.DataFrame(index=names)), "atac": AnnData(x2.copy(), obs=pd.DataFrame(index=names))})
    perm = np.random.default_rng(0).permutation(n)
    shuf = MuData({"rna": AnnData(x1.copy(), obs=pd.DataFrame(index=names)),
                   "atac": AnnData(x2[perm].copy(), obs=pd.DataFrame(index=names[perm]))})
    for md in (base, shuf):
        for m in md.mod.values():
            pp.knn(m, n_neighbors=12, use_rep="X", backend=BE)
        pp.neighbors(md, n_multineighbors=35, add_weights_to_modalities=True, backend=BE)
    assert list(shuf.obs.index) == list(names)
    assert np.array_equal(shuf.obsp["distances"].indices, base.obsp["distances"].indices)
    np.testing.assert_allclose(shuf.obsp["distances"].data, base.obsp["distances"].data, rtol=1e-9)
    np.testing.assert_allclose(shuf.mod["atac"].obs["mod_weight"].values, base.mod["atac"].obs["mod_weight"].values[perm], rtol=1e-9)
    # (b) the second modality lacks every seventh cell: against the oracle with presence masks
    have = np.arange(n) % 7 != 3
    part = MuData({"rna": AnnData(x1.copy(), obs=pd.DataFrame(index=names)),
                   "atac": AnnData(x2[have].copy(), obs=pd.DataFrame(index=names[have]))})
    for m in part.mod.values():
        pp.knn(m, n_neighbors=12, use_rep="X", backend=BE)
    pp.neighbors(part, n_multineighbors=35, backend=BE)
    loc = np.nonzero(have)[0]
    g2 = part.mod["atac"].obsp["distances"].tocoo()
    G2 = sp.csr_matrix((g2.data, (loc[g2.row], loc[g2.col])), shape=(n, n))
    x2g = np.zeros_like(x2)
    x2g[have] = x2[have]
    D, C, W, sig, k = wnn_oracle.neighbors({"rna": x1, "atac": x2g}, {"rna": part.mod["rna"].obsp["distances"], "atac": G2},
                                           n_multineighbors=35, present={"atac": have})
    got = part.obsp["distances"]
    assert np.array_equal(got.indices, D.indices)
    np.testing.assert_allclose(got.data, D.data, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(part.obs["rna:mod_weight"].values, W[:, 0], rtol=1e-5)
    assert np.all(part.obs["atac:mod_weight"].values[~have] == 0) and np.all(part.obs["rna:mod_weight"].values[~have] == 1)
    assert (abs(part.obsp["connectivities"] - C) > 1e-5).nnz == 0


def test_wnn_undefined_bandwidths_are_reported():
    """a cell that shares no neighbour with any other cell has no kernel bandwidth (the reference averages
    an empty selection: NaN, silently carried into the weights and the graph)."""
    rng = np.random.default_rng(2)
    x1 = rng.standard_normal((60, 4))
    x2 = rng.standard_normal((60, 3))
    md = MuData({"a": AnnData(x1.copy()), "b": AnnData(x2.copy())})
    for m in md.mod.values():
        pp.knn(m, n_neighbors=4, use_rep="X", backend=BE)
    # cut one cell off: its neighbour list points at cells that never list it or its neighbours
    g = md.mod["a"].obsp["distances"].tolil()
    far = np.arange(50, 53)
    g[0, :] = 0
    g[0, far] = 1.0
    for j in range(1, 60):
        for c in list(far) + [0]:
            g[j, c] = 0
    md.mod["a"].obsp["distances"] = g.tocsr()
    md.mod["a"].obsp["distances"].eliminate_zeros()
    if (np.diff(md.mod["a"].obsp["distances"].indptr) == 0).any():
        pytest.skip("the construction emptied a row")
    with pytest.raises(ValueError, match="kernel bandwidth is undefined"):
        pp.neighbors(md, n_multineighbors=20, backend=BE)


def test_wnn_slots_errors_and_copy():
    _, x1, x2 = two_modalities(90, 1)
    md = MuData({"a": AnnData(x1.copy()), "b": AnnData(x2.copy())})
    with pytest.raises(ValueError, match="Run `sc.pp.neighbors`"):
        pp.neighbors(md, backend=BE)
    for m in md.mod.values():
        pp.knn(m, n_neighbors=10, use_rep="X", backend=BE)
    out = pp.neighbors(md, key_added="wnn", n_multineighbors=25, add_weights_to_modalities=True, copy=True, backend=BE)
    assert "wnn" not in md.uns and "wnn_distances" in out.obsp and "wnn_connectivities" in out.obsp
    assert out.uns["wnn"]["distances_key"] == "wnn_distances"
    assert "mod_weight" in out.mod["a"].obs.columns and "a:mod_weight" not in out.obs.columns
    with pytest.raises(TypeError):
        pp.neighbors(AnnData(x1), backend=BE)
    assert mu.pp.neighbors is pp.neighbors


class _FilterEmulation(CpuTestBackend):
    """CpuTestBackend + a torch emulation of the HIP filter kernel (csrc/knn.hip): exercises the panel walk,
    the merges and the overflow redo of ``_candidates_filtered`` without a GPU."""

    def knn_filter(self, Xq, Xc, sqq, sqc, thr, self_pos, c_lo, c_hi, buf_pos, buf_d, cnt):
        import torch

        cap = buf_pos.shape[1]
        D = sqq[:, None] + sqc[None, c_lo:c_hi] - 2.0 * (Xq @ Xc[c_lo:c_hi].T)
        ok = D < thr[:, None]
        pos = torch.arange(c_lo, c_hi)[None, :].expand_as(D)
        ok &= pos != self_pos[:, None].long()
        cnt[:] = ok.sum(dim=1).to(cnt.dtype)
        for i in torch.nonzero(cnt > 0)[:, 0].tolist():
            j = torch.nonzero(ok[i])[:, 0][:cap]
            buf_pos[i, : j.numel()] = (j + c_lo).to(buf_pos.dtype)
            buf_d[i, : j.numel()] = D[i, j]


@pytest.mark.parametrize("metric,k", [("euclidean", 12), ("cosine", 40)])
def test_filtered_candidate_search_equals_the_tiled_search(metric, k):
    import torch

    rng = np.random.default_rng(5)
    lab = rng.integers(0, 12, 9000)
    X = rng.standard_normal((12, 7))[lab] * 2 + rng.standard_normal((9000, 7))
    X[100:140] = X[100]  # duplicated rows: exact ties
    Xd = torch.as_tensor(X)
    i0, d0 = pp.device_knn(Xd, k, metric)
    i1, d1 = pp.device_knn(Xd, k, metric, backend=_FilterEmulation())
    np.testing.assert_allclose(d1.numpy(), d0.numpy(), rtol=0, atol=1e-12)
    # the same neighbours, except WHICH of the 40 identical rows are listed where they tie
    a, b = i0.numpy(), i1.numpy()
    dup = lambda v: (v >= 100) & (v < 140)  # noqa: E731
    assert np.all((a == b) | (dup(a) & dup(b)))


def test_filtered_candidate_search_redoes_rows_whose_buffer_overflowed():
    import torch

    rng = np.random.default_rng(6)
    X = torch.as_tensor(rng.standard_normal((8500, 5)))
    sq = (X * X).sum(dim=1)
    kc = 20
    got, _ = pp._candidates_filtered(_FilterEmulation(), X, sq, kc, 1 << 26, cap=3)  # ~kc candidates per panel >> 3
    D = sq[:, None] + sq[None, :] - 2.0 * (X @ X.T)
    D.fill_diagonal_(float("inf"))
    want = torch.topk(D, kc, dim=1, largest=False).indices
    assert torch.equal(torch.sort(got, dim=1).values, torch.sort(want, dim=1).values)


def test_symmetrise_matches_the_scipy_formula():
    """P + P^T - P o P^T (umap's fuzzy union) built from keys and two scatter-adds equals the sparse-matrix expression"""
    import scipy.sparse as sp
    import torch

    from muon_amd._core.preproc import _symmetrise

    rng = np.random.default_rng(4)
    n, k = 300, 12
    idx = np.stack([rng.choice(n, size=k, replace=False) for _ in range(n)])
    idx[:, 0] = np.arange(n)  # the cell itself, strength 0 (dropped)
    val = rng.random((n, k))
    val[:, 0] = 0.0
    val[rng.random((n, k)) < 0.1] = 0.0  # some exact zeros
    got = _symmetrise(torch.from_numpy(idx), torch.from_numpy(val), n)
    P = sp.csr_matrix((val.reshape(-1), (np.repeat(np.arange(n), k), idx.reshape(-1))), shape=(n, n))
    P.eliminate_zeros()
    want = (P + P.T - P.multiply(P.T)).tocsr()
    want.eliminate_zeros()
    want.sort_indices()
    assert got.has_sorted_indices and (got.indptr == want.indptr).all() and (got.indices == want.indices).all()
    np.testing.assert_allclose(got.data, want.data, rtol=0, atol=1e-15)
    assert abs(got - got.T).max() < 1e-15


# ---- reference-executed fixtures (tests/golden/make_wnn_golden.py: the reference's own neighbors() / l2norm run in the
#      build container with stubs for numba / pynndescent / umap / scanpy only) -------------------------------------
def _golden_case(golden_dir, tag):
    import os

    g = np.load(os.path.join(golden_dir, "wnn_golden.npz"))
    x1, x2 = g[f"{tag}_x1"], g[f"{tag}_x2"]
    n = x1.shape[0]
    graphs = {m: sp.csr_matrix((g[f"{tag}_{m}_g_data"], g[f"{tag}_{m}_g_indices"], g[f"{tag}_{m}_g_indptr"]), shape=(n, n))
              for m in ("rna", "atac")}
    nb, nm, nn = (int(v) for v in g[f"{tag}_kw"])
    kw = dict(n_bandwidth_neighbors=nb, n_multineighbors=nm)
    if nn >= 0:
        kw["n_neighbors"] = nn
    ref = sp.csr_matrix((g[f"{tag}_dist_data"], g[f"{tag}_dist_indices"], g[f"{tag}_dist_indptr"]), shape=(n, n))
    want = dict(dist=ref, w_rna=g[f"{tag}_rna_weight"], w_atac=g[f"{tag}_atac_weight"], n_neighbors=int(g[f"{tag}_n_neighbors"][0]),
                k=[int(v) for v in g[f"{tag}_k"]])
    return x1, x2, graphs, kw, want


def _same_graph(got, want, tol):
    n = want.shape[0]
    k1 = int(np.diff(want.indptr)[0])
    got = got.tocsr()
    assert np.all(np.diff(got.indptr) == k1) and np.all(np.diff(want.indptr) == k1)
    gd = np.sort(np.asarray(got.data).reshape(n, k1), axis=1)
    wd = np.sort(np.asarray(want.data).reshape(n, k1), axis=1)
    assert np.max(np.abs(gd - wd)) < tol
    for i in range(n):  # (neighbour SETS: the reference's argsort inside a row is not stable)
        assert set(got.indices[got.indptr[i]:got.indptr[i + 1]]) == set(want.indices[want.indptr[i]:want.indptr[i + 1]])


@pytest.mark.parametrize("tag", ["a", "b"])
def test_oracle_is_pinned_to_the_reference_executing(golden_dir, tag):
    """oracle/wnn_oracle.neighbors against the output of /root/reference/muon/_core/preproc.py:264-640 itself: modality
    weights to 1e-15, the multimodal graph's distances to 1e-15, identical neighbour sets in every row"""
    x1, x2, graphs, kw, want = _golden_case(golden_dir, tag)
    D, _C, W, _sig, nn = wnn_oracle.neighbors({"rna": x1, "atac": x2}, graphs, **kw)
    assert nn == want["n_neighbors"]
    np.testing.assert_allclose(W[:, 0], want["w_rna"], rtol=0, atol=1e-14)
    np.testing.assert_allclose(W[:, 1], want["w_atac"], rtol=0, atol=1e-14)
    _same_graph(D, want["dist"], 1e-14)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_neighbors_against_the_reference_executing(golden_dir, tag):
    """muon_amd.pp.neighbors (tensor formulation on the CPU operator set) on the fixture's inputs"""
    x1, x2, graphs, kw, want = _golden_case(golden_dir, tag)
    md = MuData({"rna": AnnData(x1.copy()), "atac": AnnData(x2.copy())})
    for m, k in zip(("rna", "atac"), want["k"]):
        md.mod[m].obsp["distances"] = graphs[m]
        md.mod[m].uns["neighbors"] = {"connectivities_key": "connectivities", "distances_key": "distances",
                                      "params": {"n_neighbors": k, "method": "umap", "metric": "euclidean"}}
    pp.neighbors(md, backend=BE, **kw)
    assert md.uns["neighbors"]["params"]["n_neighbors"] == want["n_neighbors"]
    # (the neighbourhood means run through the f32 SpMM: 1e-7 in the weights, like against the oracle above)
    np.testing.assert_allclose(np.asarray(md.obs["rna:mod_weight"]), want["w_rna"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(np.asarray(md.obs["atac:mod_weight"]), want["w_atac"], rtol=0, atol=1e-6)
    _same_graph(md.obsp["distances"], want["dist"], 1e-6)


def test_l2norm_against_the_reference_executing(golden_dir):
    import os

    g = np.load(os.path.join(golden_dir, "wnn_golden.npz"))
    a = AnnData(g["l2_dense_in"].copy())
    pp.l2norm(a)
    np.testing.assert_allclose(a.X, g["l2_dense_out"], rtol=1e-14)
    s = sp.csr_matrix((g["l2_csr_in_data"], g["l2_csr_in_indices"], g["l2_csr_in_indptr"]), shape=(20, 30))
    b = AnnData(s.copy())
    pp.l2norm(b)
    np.testing.assert_allclose(b.X.tocsr().data, g["l2_csr_out_data"], rtol=1e-14)


# ---- the references of tests/test_gpu_knn_edges.py against the tensor paths (tests/knn_edge_refs.py) ---------------
#      the same checks with the CPU operator set and the filter's emulation in the kernels' place: what the GPU tests
#      compare the kernels with is itself compared with an independent formulation here
@pytest.mark.parametrize("square", [False, True], ids=["distinct", "square"])
@pytest.mark.parametrize("p_pad", [4, 156])
def test_filter_reference_agrees_with_the_emulation(p_pad, square):
    from tests import knn_edge_refs as ref

    ref.check_filter(_FilterEmulation(), p_pad, square, n_qs=(1, 65) + ((ref.FILTER_N_CAND,) if square else ()))


@pytest.mark.parametrize("n,p,kc", [(2500, 3, 5), (2500, 64, 40), (4500, 3, 40), (4500, 64, 5)])
def test_candidate_search_reference_agrees_with_the_emulation(n, p, kc):
    from tests import knn_edge_refs as ref

    ref.check_candidates_separated(_FilterEmulation(), n, p, kc)


def test_candidate_search_reference_agrees_with_the_emulation_on_tied_rows():
    from tests import knn_edge_refs as ref

    ref.check_candidates_tied(_FilterEmulation())


@pytest.mark.parametrize("p", [3, 64])
def test_candidate_search_reference_agrees_with_the_emulation_at_kc_300(p):
    from tests import knn_edge_refs as ref

    ref.check_candidates_separated(_FilterEmulation(), 4500, p, 300, cap=3 * 300 + 64)


@pytest.mark.parametrize("n_bw", [1, 20, 64])
@pytest.mark.parametrize("p", [1, 63, 64, 65, 256])
@pytest.mark.parametrize("n", [3, 5, 67, 300])
def test_bandwidth_reference_agrees_with_the_tensor_formulation(n, p, n_bw):
    import torch

    from tests import knn_edge_refs as ref

    X, G = ref.irregular_graph(n, p)
    want = ref.check_bandwidth(BE, X, G, n_bw, direct=False)
    assert bool(torch.isnan(want).any()) and bool(torch.isfinite(want).any())


@pytest.mark.parametrize("n_bw", [1, 10, 20])
def test_bandwidth_reference_agrees_with_the_tensor_formulation_on_tied_keys(n_bw):
    from tests import knn_edge_refs as ref

    X, G = ref.tied_graph()
    ref.check_bandwidth(BE, X, G, n_bw, min_gap=None, direct=False)


@pytest.mark.parametrize("listers", [63, 64, 65, 4095, 4096, 4097])
def test_bandwidth_reference_agrees_with_the_tensor_formulation_on_hubs(listers):
    from tests import knn_edge_refs as ref

    X, G = ref.hub_graph(listers)
    ref.check_bandwidth(BE, X, G, 20, cells=None if listers < 100 else ref.hub_sample(G, listers), direct=False)


def test_bandwidth_reference_gaps_on_the_buffer_boundary_graphs():
    """(the two 8k graphs run on the GPU only: here the condition on their input)"""
    from tests import knn_edge_refs as ref

    for listers in (8193, 8194):
        X, G = ref.hub_graph(listers, private=False)
        want, gap = ref.bandwidth_reference(X, G.indptr, G.indices, 20, ref.hub_sample(G, listers))
        assert gap > 1e-9 and np.isnan(want[0]) and np.isfinite(want[1:]).all()


@pytest.mark.parametrize("k", [2, 3, 21])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_umap_oracle_agrees_with_the_tensor_bisection(n, k):
    from tests import knn_edge_refs as ref

    ref.check_umap(BE, n, k, backend=None)
