"""pp.qc_metrics(qc_vars=, percent_top=), pp.intersect_obs and pp.sample_obs: host logic and the tensor formulations of
the two per-row sums on the CPU test operator set, against the NumPy statements of tests/qc_refs.py (reference
muon/_core/preproc.py:646-669, :887-931; scanpy's calculate_qc_metrics columns).  The HIP kernels are exercised by
tests/test_gpu_qc.py."""
import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

import muon_amd as mu
from muon_amd._core.preproc import masked_sums_tensor, qc_row_sums_device, top_sums_tensor
from muon_amd._hostmatrix import resident
from muon_amd._operators import has
from tests import qc_refs
from tests.cpu_backend import CpuTestBackend

BE = CpuTestBackend()
OBS_PARENT = ["n_genes_by_counts", "log1p_n_genes_by_counts", "total_counts", "log1p_total_counts"]
VAR_PARENT = ["n_cells_by_counts", "mean_counts", "log1p_mean_counts", "pct_dropout_by_counts", "total_counts",
              "log1p_total_counts"]


def _upload(m):
    return BE.upload_csr(m.indptr, m.indices, m.data, m.shape)


def _flags(masks):
    w = np.zeros(masks.shape[1], dtype=np.uint32)
    for b, mask in enumerate(masks):
        w |= mask.astype(np.uint32) << np.uint32(b)
    return BE.to_device(w.view(np.int32), np.int32)


@pytest.fixture(scope="module", params=[np.float32, np.float64], ids=["f32", "f64"])
def case(request):
    m = qc_refs.engineered(request.param)
    return m, _upload(m)


def test_the_cpu_operator_set_takes_the_tensor_formulations():
    assert not has(BE, "row_masked_sums") and not has(BE, "row_top_sums")


@pytest.mark.parametrize("ns", [qc_refs.NS, (520,), (1,), (1, 2, 3, 64, 65, 300, 519, 520)])
def test_top_sums_tensor_is_the_numpy_statement(case, ns):
    m, X = case
    want = qc_refs.row_top_sums(m, ns)
    got = top_sums_tensor(X, ns).numpy()
    assert got.dtype == np.float64 and got.tobytes() == want.tobytes()
    blocks = top_sums_tensor(X, ns, max_cells=7 * max(ns)).numpy()  # row blocks of 7 rows: the same numbers
    assert blocks.tobytes() == want.tobytes()


@pytest.mark.parametrize("M", [1, 3, 32])
def test_masked_sums_tensor_is_the_numpy_statement(case, M):
    m, X = case
    masks = qc_refs.masks_for(m.shape[1], M)
    assert M < 32 or masks[31].any()  # (bit 31 of the flag word: the sign bit of the int32 torch carries)
    got = masked_sums_tensor(X, _flags(masks), M).numpy()
    assert got.dtype == np.float64 and got.tobytes() == qc_refs.row_masked_sums(m, masks).tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_tensor_formulations_on_values_that_are_no_integers(dtype):
    m = qc_refs.engineered(dtype)
    m.data = np.log1p(m.data)
    X = _upload(m)
    got = top_sums_tensor(X, qc_refs.NS).numpy()
    assert (np.abs(got - qc_refs.row_top_sums(m, qc_refs.NS)) <= qc_refs.top_sums_bound(m, qc_refs.NS)).all()
    masks = qc_refs.masks_for(m.shape[1], 3)
    got = masked_sums_tensor(X, _flags(masks), 3).numpy()
    assert (np.abs(got - qc_refs.row_masked_sums(m, masks)) <= qc_refs.masked_sums_bound(m, masks)).all()


def test_more_masks_and_more_ns_than_one_launch_takes(case):
    m, X = case
    masks = qc_refs.masks_for(m.shape[1], 33, seed=9)
    ns = list(range(1, 520, 47))
    assert len(ns) > 8
    masked, top = qc_row_sums_device(BE, X, masks, ns)
    assert masked.tobytes() == qc_refs.row_masked_sums(m, masks).tobytes()
    assert top.tobytes() == qc_refs.row_top_sums(m, ns).tobytes()


def _adata(dtype=np.float32, dense=False):
    m = qc_refs.engineered(dtype)
    m.sort_indices()
    rng = np.random.default_rng(11)
    var = pd.DataFrame({"mt": rng.random(m.shape[1]) < 0.1, "ribo": rng.random(m.shape[1]) < 0.3,
                        "score": rng.random(m.shape[1])}, index=[f"g{j}" for j in range(m.shape[1])])
    return mu.AnnData(m.toarray() if dense else m.copy(), var=var), m


def _want_obs(ad, m, ns, qs, log1p):
    total = np.asarray(m.sum(axis=1, dtype=np.float64)).reshape(-1)
    cols = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        for j, n in enumerate(ns):
            cols[f"pct_counts_in_top_{n}_genes"] = 100.0 * qc_refs.row_top_sums(m, ns)[:, j] / total
        for q in qs:
            s = qc_refs.row_masked_sums(m, [ad.var[q].values])[:, 0]
            cols[f"total_counts_{q}"] = s
            if log1p:
                cols[f"log1p_total_counts_{q}"] = np.log1p(s)
            cols[f"pct_counts_{q}"] = 100.0 * s / total
    return cols


@pytest.mark.parametrize("log1p", [True, False])
def test_qc_metrics_columns_and_their_order(log1p):
    ad, m = _adata()
    obs, var = mu.pp.qc_metrics(ad, qc_vars=["mt", "ribo"], percent_top=(200, 50), log1p=log1p, inplace=False, backend=BE)
    want = ["n_genes_by_counts", "log1p_n_genes_by_counts", "total_counts", "log1p_total_counts",
            "pct_counts_in_top_50_genes", "pct_counts_in_top_200_genes",
            "total_counts_mt", "log1p_total_counts_mt", "pct_counts_mt",
            "total_counts_ribo", "log1p_total_counts_ribo", "pct_counts_ribo"]
    if not log1p:
        want = [c for c in want if not c.startswith("log1p")]
    assert list(obs.columns) == want
    assert list(var.columns) == [c for c in VAR_PARENT if log1p or not c.startswith("log1p")]
    assert list(obs.index) == list(ad.obs_names) and "total_counts_mt" not in ad.obs.columns  # (inplace=False)
    for c, v in _want_obs(ad, m, (50, 200), ["mt", "ribo"], log1p).items():
        assert obs[c].values.tobytes() == v.tobytes(), c
    empty = np.asarray(m.sum(axis=1)).reshape(-1) == 0
    assert empty[0] and empty[-1]
    for c in obs.columns:
        assert np.isnan(obs[c].values[empty]).all() == c.startswith("pct_"), c
        assert not np.isnan(obs[c].values[~empty]).any(), c
    # in place, a single name as a string, and one n
    assert mu.pp.qc_metrics(ad, qc_vars="mt", percent_top=[520], log1p=log1p, backend=BE) is None
    assert ad.obs["pct_counts_mt"].values.tobytes() == obs["pct_counts_mt"].values.tobytes()
    assert np.array_equal(ad.obs["pct_counts_in_top_520_genes"].values[~empty], np.full(int((~empty).sum()), 100.0))
    assert "n_cells_by_counts" in ad.var.columns


def test_a_call_without_the_new_keywords_returns_the_frames_it_returned_before():
    ad, m = _adata()
    obs, var = mu.pp.qc_metrics(ad, inplace=False, backend=BE)
    assert list(obs.columns) == OBS_PARENT and list(var.columns) == VAR_PARENT
    a = m.toarray().astype(np.float64)
    assert np.array_equal(obs["n_genes_by_counts"].values, (a != 0).sum(axis=1))
    assert np.array_equal(obs["total_counts"].values, a.sum(axis=1))
    assert np.array_equal(var["n_cells_by_counts"].values, (a != 0).sum(axis=0))
    assert np.array_equal(var["total_counts"].values, a.sum(axis=0))
    again, _ = mu.pp.qc_metrics(ad, qc_vars=(), percent_top=None, inplace=False, backend=BE)
    assert again.equals(obs)
    obs2, var2 = mu.pp.qc_metrics(ad, log1p=False, inplace=False, backend=BE)
    assert list(obs2.columns) == ["n_genes_by_counts", "total_counts"]
    assert list(var2.columns) == ["n_cells_by_counts", "mean_counts", "pct_dropout_by_counts", "total_counts"]


def test_qc_metrics_errors():
    ad, m = _adata()
    for bad in ((0,), (50, 521), (-3, 50)):
        with pytest.raises(IndexError, match="Positions outside range of features."):
            mu.pp.qc_metrics(ad, percent_top=bad, backend=BE)
    mu.pp.qc_metrics(ad, percent_top=(1, 520), backend=BE)  # (both ends of the range are positions)
    with pytest.raises(ValueError, match="score"):
        mu.pp.qc_metrics(ad, qc_vars=["mt", "score"], backend=BE)
    with pytest.raises(ValueError, match="nothing_here"):
        mu.pp.qc_metrics(ad, qc_vars="nothing_here", backend=BE)
    assert "total_counts_mt" not in ad.obs.columns  # (refused before anything was written)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_dense_x_gives_the_frames_of_its_csr(dtype):
    sparse, _ = _adata(dtype)
    dense, _ = _adata(dtype, dense=True)
    kw = dict(qc_vars=["mt", "ribo"], percent_top=(50, 100, 200, 500), inplace=False, backend=BE)
    (so, sv), (do, dv) = mu.pp.qc_metrics(sparse, **kw), mu.pp.qc_metrics(dense, **kw)
    assert list(so.columns) == list(do.columns) and list(sv.columns) == list(dv.columns)
    for c in so.columns:
        assert so[c].values.tobytes() == do[c].values.tobytes(), c
    for c in sv.columns:
        assert sv[c].values.tobytes() == dv[c].values.tobytes(), c


# ---- intersect_obs --------------------------------------------------------------------------------------------------
def _three_modalities():
    rng = np.random.default_rng(4)
    names = np.asarray([f"c{i}" for i in range(30)])
    keep = {"rna": np.arange(30) % 5 != 0, "atac": np.arange(30) % 7 != 1, "prot": np.ones(30, bool)}
    mods, mats = {}, {}
    for k, (name, mask) in enumerate(keep.items()):
        own = rng.permutation(names[mask])
        m = sp.random(len(own), 12 + k, density=0.4, format="csr", random_state=rng, dtype=np.float64)
        m.data = (1 + rng.poisson(1.0, m.nnz)).astype(np.float32)
        m = m.astype(np.float32)
        m.sort_indices()
        mods[name] = mu.AnnData(m.copy(), obs=pd.DataFrame({"depth": np.asarray(m.sum(axis=1)).reshape(-1)}, index=own))
        mats[name] = (own, m)
    common = set(names[keep["rna"] & keep["atac"]])
    return mu.MuData(mods), mats, common


def test_intersect_obs_keeps_every_modality_in_its_own_order():
    mdata, mats, common = _three_modalities()
    assert len(mdata.obs_names) == 30 and 0 < len(common) < 24
    for ad in mdata.mod.values():
        mu.pp.qc_metrics(ad, backend=BE)  # (leaves a device copy with every matrix)
        assert resident(ad.X, BE) is not None
    assert mu.pp.intersect_obs(mdata, backend=BE) is None
    for name, ad in mdata.mod.items():
        own, m = mats[name]
        sel = np.isin(own, list(common))
        assert list(ad.obs_names) == list(own[sel]) and ad.shape == (len(common), m.shape[1])
        assert (ad.X != m[sel]).nnz == 0
        assert np.array_equal(ad.obs["depth"].values, np.asarray(m[sel].sum(axis=1)).reshape(-1))
        R = resident(ad.X, BE)  # the device copy went along: the host slice, entry for entry
        assert R is not None and R.shape == ad.shape
        assert np.array_equal(BE.to_host(R.indptr), ad.X.indptr) and np.array_equal(BE.to_host(R.indices), ad.X.indices)
        assert BE.to_host(R.values).tobytes() == ad.X.data.tobytes()
    assert set(mdata.obs_names) == common and len(mdata.obs_names) == len(common)
    assert list(mdata.obs_names) == list(mdata.mod["rna"].obs_names)  # (the union in the first modality's order)
    # idempotent, and a modality that holds exactly the common cells is not touched: same matrix, same device copy
    before = {k: (ad.X, resident(ad.X, BE), list(ad.obs_names)) for k, ad in mdata.mod.items()}
    mu.pp.intersect_obs(mdata, backend=BE)
    for k, ad in mdata.mod.items():
        assert ad.X is before[k][0] and resident(ad.X, BE) is before[k][1] and list(ad.obs_names) == before[k][2]
    assert set(mdata.obs_names) == common


def test_intersect_obs_leaves_the_modality_that_is_the_intersection_alone():
    mdata, mats, common = _three_modalities()
    small = mdata.mod["rna"][np.isin(mdata.mod["rna"].obs_names, list(common))]
    small._init_as_actual()
    mdata.mod["rna"] = small
    mdata.update()
    mu.pp.qc_metrics(small, backend=BE)
    X0, R0 = small.X, resident(small.X, BE)
    assert R0 is not None
    mu.pp.intersect_obs(mdata)  # without a backend: the copies' own serves
    assert mdata.mod["rna"].X is X0 and resident(X0, BE) is R0
    assert mdata.mod["atac"].n_obs == mdata.mod["prot"].n_obs == len(common)
    assert set(mdata.mod["prot"].obs_names) == common


def test_intersect_obs_refuses_a_view_like_filter_obs():
    mdata, _, _ = _three_modalities()
    mdata.mod["prot"] = mdata.mod["prot"][:20]
    with pytest.raises(ValueError, match="view"):
        mu.pp.intersect_obs(mdata)


# ---- sample_obs -----------------------------------------------------------------------------------------------------
def _grouped():
    ad, _ = _adata()
    n = ad.n_obs
    ad.obs["grp"] = pd.Categorical(np.asarray(["b", "a", "c"])[np.arange(n) % 3], categories=["b", "a", "c"])
    ad.obs["text"] = [f"t{i % 2}" for i in range(n)]
    return ad


def _reference_lines(data, frac=0.1, groupby=None, min_n=None):
    """the reference's statements (muon/_core/preproc.py:912-931), restated: which np.random calls, in which order"""
    if groupby is None:
        new_n = np.ceil(data.n_obs * frac).astype(int)
        if min_n is not None and new_n < min_n:
            new_n = min_n
        return np.random.choice(range(data.n_obs), size=new_n, replace=False)
    obs_names = []
    for cat in data.obs[groupby].cat.categories:
        view = data[data.obs[groupby] == cat]
        new_n = np.ceil(view.n_obs * frac).astype(int)
        if min_n is not None and new_n < min_n:
            new_n = min_n
        obs_names.append(np.random.choice(view.obs_names.values, size=new_n, replace=False))
    return np.concatenate(obs_names)


@pytest.mark.parametrize("kw", [dict(), dict(frac=0.37), dict(frac=0.01, min_n=5), dict(frac=0.3, groupby="grp"),
                                dict(frac=0.05, groupby="grp", min_n=4)], ids=str)
def test_sample_obs_draws_the_cells_the_reference_draws(kw):
    ad = _grouped()
    np.random.seed(123)
    want = _reference_lines(ad, **kw)
    np.random.seed(123)
    got = mu.pp.sample_obs(ad, **kw)
    names = list(ad.obs_names[want]) if "groupby" not in kw else list(want)
    assert list(got.obs_names) == names and got.is_view and got.n_obs == len(want) > 0
    assert (got.X != ad[names].X).nnz == 0
    if kw.get("min_n") and "groupby" not in kw:
        assert got.n_obs == kw["min_n"]
    if kw.get("min_n") and "groupby" in kw:
        assert got.obs["grp"].value_counts().tolist() == [kw["min_n"]] * 3


def test_sample_obs_on_mudata_and_its_errors():
    mdata, _, _ = _three_modalities()
    np.random.seed(5)
    want = mdata.obs_names.values[_reference_lines(mdata, frac=0.5)]
    np.random.seed(5)
    got = mu.pp.sample_obs(mdata, frac=0.5)
    assert set(got.obs_names) == set(want) and got.n_obs == 15
    ad = _grouped()
    with pytest.raises(ValueError, match="nowhere is not in .obs"):
        mu.pp.sample_obs(ad, groupby="nowhere")
    with pytest.raises(TypeError, match=r"\.obs\['text'\] is not categorical"):
        mu.pp.sample_obs(ad, groupby="text")


def test_the_package_exports_the_new_entry_points():
    assert callable(mu.pp.intersect_obs) and callable(mu.pp.sample_obs)
    assert "intersect_obs" in mu.__doc__ and "sample_obs" in mu.__doc__
    assert torch.float64 == top_sums_tensor(_upload(qc_refs.engineered(np.float32)), (1,)).dtype
