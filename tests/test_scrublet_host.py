"""muon_amd.pp.scrublet without a GPU: the NumPy restatement (tests/scrublet_refs.py) against scipy, the tensor
formulation of the pair merge against the restatement byte for byte, the score formulas, the threshold routine, the
write-back, and the search stage through CpuTestBackend against brute force on the same embedding."""
import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

import muon_amd as mu
from muon_amd._core import scrublet as S
from muon_amd._hostmatrix import resident
from tests import scrublet_refs as R
from tests.cpu_backend import CpuTestBackend


@pytest.fixture(scope="module")
def be():
    return CpuTestBackend()


@pytest.fixture(scope="module")
def planted():
    return R.planted_doublets()


@pytest.fixture(scope="module")
def planted_ref(planted):
    out = R.scrublet(planted[0])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def planted_cpu(planted, be):
    ad = mu.AnnData(planted[0].copy())
    mu.pp.scrublet(ad, backend=be)
    return ad


def _upload(be, m):
    return be.upload_csr(m.indptr, m.indices, m.data, m.shape, slab_ptr=False)


# ---- simulation ---------------------------------------------------------------------------------------------------------
def test_restated_simulation_is_scipys_sum_on_positive_counts():
    rng = np.random.default_rng(0)
    E = sp.random(200, 300, density=0.1, format="csr", random_state=rng, dtype=np.float64)
    E.data = rng.integers(1, 50, size=E.nnz).astype(np.float32)  # strictly positive: scipy's sum prunes nothing
    E = E.astype(np.float32)
    E.sort_indices()
    parents = R.np.random.RandomState(3).randint(0, 200, size=(400, 2))
    parents[:5, 1] = parents[:5, 0]  # a cell paired with itself
    got = R.simulate_csr(E, parents)
    want = (E[parents[:, 0]] + E[parents[:, 1]]).tocsr()
    want.sort_indices()
    assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
    assert got.data.tobytes() == want.data.astype(np.float32).tobytes()


@pytest.mark.parametrize("index_dtype", ["int32", "int64"])
def test_tensor_pair_merge_is_the_restatement_byte_for_byte(be, index_dtype):
    E, parents = R.pair_case(index_dtype)
    want = R.simulate(E, parents)
    X = mu._backend.DeviceCSR(torch.from_numpy(E.indptr.copy()), torch.from_numpy(E.indices.copy()),
                              torch.from_numpy(E.data.copy()), E.shape)
    got = S.pair_rows_tensor(X, torch.from_numpy(parents.copy()))
    assert got.indices.dtype == X.indices.dtype and got.shape == (len(parents), E.shape[1])
    assert np.array_equal(got.indptr.numpy(), want[0]) and np.array_equal(got.indices.numpy(), want[1])
    assert got.values.numpy().tobytes() == want[2].tobytes()
    # the union keeps every stored column, zeros included, and a row paired with itself is the row doubled
    lens = np.diff(E.indptr)
    assert (np.diff(want[0]) <= lens[parents[:, 0]] + lens[parents[:, 1]]).all()
    same = np.flatnonzero(parents[:, 0] == parents[:, 1])
    assert same.size and all(np.diff(want[0])[s] == lens[parents[s, 0]] for s in same)
    assert (want[2] == 0).any()


def test_tensor_pair_merge_takes_rows_that_are_not_canonical(be):
    """duplicates and unsorted columns: concatenate, sort, segmented sum = scipy's sum of the canonicalised rows"""
    indptr = np.array([0, 4, 7], dtype=np.int64)
    indices = np.array([5, 1, 5, 9, 9, 0, 1], dtype=np.int32)
    data = np.array([1, 2, 4, 8, 16, 32, 64], dtype=np.float32)
    X = mu._backend.DeviceCSR(torch.from_numpy(indptr), torch.from_numpy(indices), torch.from_numpy(data), (2, 12))
    got = S.simulate_device(be, X, np.array([[0, 1], [1, 1]]), canonical=False)
    m = sp.csr_matrix((data, indices, indptr), shape=(2, 12))
    m.sum_duplicates()
    want = sp.vstack([m[0] + m[1], m[1] + m[1]]).tocsr()
    want.sort_indices()
    assert np.array_equal(got.indptr.numpy(), want.indptr) and np.array_equal(got.indices.numpy(), want.indices)
    assert np.array_equal(got.values.numpy(), want.data)


# ---- scores and threshold --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k_adj,r,rho,se_rho", [(60, 2.0, 0.05, 0.02), (474, 2.0, 0.06, 0.03), (7, 0.5, 0.2, 0.01)])
def test_score_formulas(k_adj, r, rho, se_rho):
    nsn = np.arange(0, k_adj + 1)
    Ld, se = S.doublet_scores(nsn, k_adj, r, rho, se_rho)
    want_Ld, want_se = R.scores(nsn, k_adj, r, rho, se_rho)
    np.testing.assert_allclose(Ld, want_Ld, rtol=1e-12, atol=0)
    np.testing.assert_allclose(se, want_se, rtol=1e-12, atol=0)
    assert (np.diff(Ld) > 0).all() and (Ld > 0).all() and (se > 0).all()


def _bimodal(seed=0):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.normal(0.08, 0.02, 3000), rng.normal(0.5, 0.08, 6000)]).clip(0.001, 0.999)


def test_threshold_of_a_bimodal_sample_is_the_restated_bin_centre():
    s = _bimodal()
    t = S.bimodal_threshold(s)
    assert t is not None and t == R.threshold(s) and 0.12 < t < 0.4
    edges = np.histogram(s, bins=256)[1]
    centres = 0.5 * (edges[:-1] + edges[1:])
    assert np.abs(centres - t).min() == 0.0
    rates = S.call_doublets(s[:100], s, None)
    assert rates["threshold"] == t and rates["detectable_doublet_fraction"] == (s > t).mean()
    assert rates["overall_doublet_rate"] == rates["detected_doublet_rate"] / rates["detectable_doublet_fraction"]


def test_local_maxima_on_plateaus_and_edges():
    h = np.array([3, 3, 1, 2, 2, 2, 1, 0, 0, 5], dtype=np.float64)
    assert S._local_maxima(h).tolist() == R._maxima(h) == [0, 3, 9]
    assert S._local_maxima(np.ones(5)).tolist() == R._maxima(np.ones(5)) == [0]


def test_unimodal_scores_warn_and_write_no_call(planted, be):
    # a histogram that rises to one bin and falls again: one maximum from the start (a sampled bell curve would not do:
    # the last bump of its tail survives the smoothing as a second maximum, and the statement then sets a threshold)
    centres = (np.arange(256) + 0.5) / 256
    s = np.repeat(centres, 1 + np.minimum(np.arange(256), 255 - np.arange(256)))
    assert S.bimodal_threshold(s) is None and R.threshold(s) is None
    assert S.bimodal_threshold(np.full(50, 0.3)) is None and R.threshold(np.full(50, 0.3)) is None
    with pytest.warns(UserWarning, match="not bimodal"):
        assert S.call_doublets(s[:10], s, None) == {}
    # through the public call: with k_adj = every other row all simulated rows have n_sim - 1 simulated neighbours, so
    # their scores are one value
    ad = mu.AnnData(planted[0][:300].copy())
    ad.obs["predicted_doublet"] = False  # (a stale column from an earlier call goes)
    with pytest.warns(UserWarning, match="not bimodal"):
        mu.pp.scrublet(ad, n_prin_comps=5, n_neighbors=300, backend=be)
    u = ad.uns["scrublet"]
    assert "predicted_doublet" not in ad.obs.columns and "threshold" not in u and "overall_doublet_rate" not in u
    assert np.unique(u["doublet_scores_sim"]).size == 1 and u["doublet_scores_sim"].shape == (600,)
    assert np.unique(ad.obs["doublet_score"].values).size == 1
    assert set(u) == {"doublet_scores_sim", "doublet_parents", "doublet_errors_obs", "doublet_errors_sim", "parameters"}


# ---- the search stage on the same embedding -----------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_search_stage_reproduces_the_brute_force_counts(be, metric):
    rng = np.random.default_rng(5)
    Zo = rng.standard_normal((700, 12)) + 2.0 * rng.integers(0, 2, (700, 1))
    Zs = rng.standard_normal((1400, 12)) + 1.0
    k_adj = R.adjusted_k(700, 1400)
    assert k_adj == 39
    want, gap = R.sim_neighbours(Zo, Zs, k_adj, metric)
    assert (gap >= 1e-9).all()  # the fixture leaves no query out
    res = S.scrublet_scores_device(be, torch.from_numpy(Zo), torch.from_numpy(Zs), k_adj, knn_dist_metric=metric,
                                   chunk_elems=1 << 18)  # (several query tiles)
    assert res["route"] == "tiled" and res["k_adj"] == k_adj
    assert np.array_equal(res["n_sim_neigh"], want)
    Ld, se = R.scores(want, k_adj, 2.0)
    np.testing.assert_allclose(res["scores"], Ld, rtol=1e-12, atol=0)
    np.testing.assert_allclose(res["errors"], se, rtol=1e-12, atol=0)


def test_ties_are_broken_by_row_index(be):
    """duplicated rows on both sides of the observed / simulated border: (distance, index) decides"""
    Zo = np.array([[0.0, 0], [1, 0], [1, 0], [5, 5]])
    Zs = np.array([[1.0, 0], [1, 0], [9, 9], [9, 9]])
    want, _gap = R.sim_neighbours(Zo, Zs, 2)
    res = S.scrublet_scores_device(be, torch.from_numpy(Zo), torch.from_numpy(Zs), 2)
    assert np.array_equal(res["n_sim_neigh"], want) and want[0] == 0 and want[1] == 1


# ---- the public call ---------------------------------------------------------------------------------------------------------------
def test_cpu_route_on_the_planted_data(planted, planted_ref, planted_cpu):
    X, is_dbl = planted
    ad, ref = planted_cpu, planted_ref
    u = ad.uns["scrublet"]
    assert "threshold" in ref and "threshold" in u
    assert np.array_equal(u["doublet_parents"], ref["doublet_parents"]) and u["doublet_parents"].dtype == np.int64
    assert u["doublet_parents"].shape == (2 * X.shape[0], 2)
    score = ad.obs["doublet_score"].values
    assert score[is_dbl].mean() > score[~is_dbl].mean()
    assert ref["doublet_score"][is_dbl].mean() > ref["doublet_score"][~is_dbl].mean()
    called = ad.obs["predicted_doublet"].values
    assert called.dtype == bool and (called & is_dbl).sum() > 0.6 * is_dbl.sum() and (called & ~is_dbl).mean() < 0.02
    assert u["detected_doublet_rate"] == called.mean()
    assert u["detectable_doublet_fraction"] == (u["doublet_scores_sim"] > u["threshold"]).mean()
    assert u["overall_doublet_rate"] == u["detected_doublet_rate"] / u["detectable_doublet_fraction"]


def test_write_back_keys_and_an_untouched_matrix(planted, planted_cpu, be):
    X, _ = planted
    ad = planted_cpu
    u = ad.uns["scrublet"]
    assert set(u) == {"doublet_scores_sim", "doublet_parents", "doublet_errors_obs", "doublet_errors_sim", "parameters",
                      "threshold", "detected_doublet_rate", "detectable_doublet_fraction", "overall_doublet_rate"}
    assert u["parameters"]["sim_doublet_ratio"] == 2.0 and u["parameters"]["n_prin_comps"] == 30
    assert u["doublet_scores_sim"].shape == u["doublet_errors_sim"].shape == (2 * X.shape[0],)
    assert u["doublet_errors_obs"].shape == (X.shape[0],) and (u["doublet_errors_obs"] > 0).all()
    assert ad.X.data.tobytes() == X.data.tobytes() and np.array_equal(ad.X.indices, X.indices)
    assert resident(ad.X, be) is not None  # the copy stays with the user's matrix
    fixed = mu.AnnData(X.copy())
    mu.pp.scrublet(fixed, threshold=0.2, backend=be)
    assert fixed.uns["scrublet"]["threshold"] == 0.2
    assert np.array_equal(fixed.obs["predicted_doublet"].values, fixed.obs["doublet_score"].values > 0.2)
    assert np.array_equal(fixed.obs["doublet_score"].values, ad.obs["doublet_score"].values)


def test_copy_mudata_and_simulate(planted, planted_cpu, be):
    X, _ = planted
    ad = mu.AnnData(X.copy())
    out = mu.pp.scrublet(ad, copy=True, backend=be)
    assert out is not ad and "doublet_score" not in ad.obs.columns and "scrublet" not in ad.uns
    assert np.array_equal(out.obs["doublet_score"].values, planted_cpu.obs["doublet_score"].values)
    md = mu.MuData({"rna": mu.AnnData(X.copy()), "other": mu.AnnData(X[:, :50].copy())})
    assert mu.pp.scrublet(md, backend=be) is None
    assert np.array_equal(md.mod["rna"].obs["doublet_score"].values, planted_cpu.obs["doublet_score"].values)
    assert "doublet_score" not in md.mod["other"].obs.columns
    with pytest.raises(TypeError):
        mu.pp.scrublet(mu.MuData({"other": mu.AnnData(X.copy())}), backend=be)
    sim = mu.pp.scrublet_simulate_doublets(ad, sim_doublet_ratio=0.5, random_seed=4, backend=be)
    parents = np.random.RandomState(4).randint(0, X.shape[0], size=(X.shape[0] // 2, 2))
    assert sim.shape == (X.shape[0] // 2, X.shape[1]) and np.array_equal(sim.obsm["doublet_parents"], parents)
    want = R.simulate(X, parents)
    assert np.array_equal(sim.X.indptr, want[0]) and np.array_equal(sim.X.indices, want[1])
    assert sim.X.data.tobytes() == want[2].tobytes() and resident(sim.X, be) is not None
    assert sim.uns["scrublet"]["parameters"]["sim_doublet_ratio"] == 0.5
    # simulated rows handed back in: all variables, the ratio from the simulated object
    sub = mu.AnnData(X[:, :400].copy())
    sim = mu.pp.scrublet_simulate_doublets(sub, sim_doublet_ratio=1.0, backend=be)
    mu.pp.scrublet(sub, sim, n_prin_comps=10, threshold=0.25, backend=be)
    assert sub.uns["scrublet"]["parameters"]["sim_doublet_ratio"] == 1.0
    assert sub.uns["scrublet"]["doublet_scores_sim"].shape == (X.shape[0],)
    with pytest.raises(ValueError, match="batch_key"):
        mu.pp.scrublet(sub, sim, batch_key="b", backend=be)


def test_batch_key_runs_the_procedure_per_level(planted, be):
    X, _ = planted
    n = X.shape[0]
    batch = np.where(np.arange(n) % 3 == 0, "b", "a")
    ad = mu.AnnData(X.copy(), obs=pd.DataFrame({"batch": batch}, index=[f"c{i}" for i in range(n)]))
    mu.pp.scrublet(ad, batch_key="batch", n_prin_comps=10, threshold=0.2, backend=be)
    u = ad.uns["scrublet"]
    assert u["batched_by"] == "batch" and list(u["batches"]) == ["a", "b"]
    assert u["doublet_scores_sim"].shape == (2 * (batch == "a").sum() + 2 * (batch == "b").sum(),)
    for level in ("a", "b"):
        mask = batch == level
        alone = mu.AnnData(X[mask].copy())
        mu.pp.scrublet(alone, n_prin_comps=10, threshold=0.2, backend=be)
        assert np.array_equal(ad.obs["doublet_score"].values[mask], alone.obs["doublet_score"].values)
        assert np.array_equal(ad.obs["predicted_doublet"].values[mask], alone.obs["predicted_doublet"].values)
        assert np.array_equal(u["batches"][level]["doublet_parents"], alone.uns["scrublet"]["doublet_parents"])
        assert u["batches"][level]["threshold"] == 0.2
    with pytest.raises(ValueError, match="batch_key"):
        mu.pp.scrublet(ad, batch_key="nope", backend=be)


def test_what_is_not_offered_raises(planted, be):
    ad = mu.AnnData(planted[0].copy())
    with pytest.raises(NotImplementedError, match="1.0"):
        mu.pp.scrublet(ad, synthetic_doublet_umi_subsampling=0.5, backend=be)
    with pytest.raises(NotImplementedError, match="1.0"):
        mu.pp.scrublet_simulate_doublets(ad, synthetic_doublet_umi_subsampling=0.5, backend=be)
    with pytest.raises(NotImplementedError, match="euclidean.*cosine"):
        mu.pp.scrublet(ad, knn_dist_metric="manhattan", backend=be)
    with pytest.raises(NotImplementedError, match="euclidean.*cosine"):
        S.scrublet_scores_device(be, torch.zeros((4, 2), dtype=torch.float64), torch.zeros((4, 2), dtype=torch.float64), 2,
                                 knn_dist_metric="jaccard")


# ---- the library's argument checks (no HIP call is made) -------------------------------------------------------------------------------
def test_arguments_are_validated_before_any_hip_call():
    import ctypes

    from muon_amd import _ffi

    lib = _ffi.lib()
    assert lib.mu_version() >= 817 and lib.mu_knn_merge_wide_max() == 8192
    one = ctypes.c_int64(0)
    p = ctypes.addressof(one)  # (an address that is never followed: every call below is refused first)
    wide = lambda n, kc, cap, *ptrs: lib.mu_knn_merge_wide_f64(n, kc, cap, *ptrs, None)  # noqa: E731
    assert wide(4, 8192, 1, p, p, p, p, p, p, p, p) == -1 and b"8192" in lib.mu_last_error()  # 8193 pairs
    assert wide(4, 0, 8, p, p, p, p, p, p, p, p) == -1 and wide(4, 8, 0, p, p, p, p, p, p, p, p) == -1
    assert wide(-1, 8, 8, p, p, p, p, p, p, p, p) == -1
    assert wide(4, 8, 8, None, p, p, p, p, p, p, p) == -1 and b"null" in lib.mu_last_error()
    assert wide(4, 8, 8, p, p, p, p, p, p, p, None) == -1
    q = ctypes.addressof(ctypes.c_int64(0))
    assert wide(4, 8, 8, p, q, p, p, p, p, p, p) == -1 and b"in place" in lib.mu_last_error()
    assert wide(0, 8, 8, None, None, None, None, None, None, None, None) == 0
    cnt = lambda ib, n, k, ip, ix, par, out: lib.mu_csr_pair_rows_count(ib, n, k, ip, ix, par, out, None)  # noqa: E731
    assert cnt(2, 4, 4, p, p, p, p) == -1 and b"index_bytes" in lib.mu_last_error()
    assert cnt(4, -4, 4, p, p, p, p) == -1 and cnt(4, 4, -4, p, p, p, p) == -1
    assert cnt(4, 4, 4, None, p, p, p) == -1 and cnt(4, 4, 4, p, p, None, p) == -1 and cnt(4, 4, 4, p, p, p, None) == -1
    assert cnt(8, 4, 0, None, None, None, None) == 0
    fill = lambda ib, n, k, *ptrs: lib.mu_csr_pair_rows_fill(ib, n, k, *ptrs, None)  # noqa: E731
    assert fill(3, 4, 4, p, p, p, p, p, p, p) == -1 and fill(4, 4, 4, None, p, p, p, p, p, p) == -1
    assert fill(4, 4, 4, p, p, p, None, p, p, p) == -1 and fill(4, 4, 4, p, p, p, p, None, p, p) == -1
    assert fill(4, 4, 0, None, None, None, None, None, None, None) == 0
