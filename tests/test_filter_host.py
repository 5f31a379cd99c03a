"""muon_amd.pp.filter_obs / filter_var / qc_metrics: host logic on the CPU test operator set (reference
muon/_core/preproc.py:675-881; scanpy's calculate_qc_metrics columns).  The HIP kernels are exercised by
tests/test_gpu_filter.py."""
import os
import socket
import sys
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch
import torch.multiprocessing as mp

import muon_amd as mu
from muon_amd._hostmatrix import DEVICE_ATTR, attach_device, resident
from muon_amd._core import io as mio
from muon_amd._core.preproc import _submatrix_tensor, submatrix_device
from muon_amd._operators import has
from tests.cpu_backend import CpuTestBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BE = CpuTestBackend()


class _NoBackend:
    """Any use of this operator set is an error: what a host-only object must never reach."""

    def __getattr__(self, name):
        raise AssertionError(f"backend.{name} was touched")


def _counts(n=40, d=30, seed=0, dtype=np.float32):
    rng = np.random.default_rng(seed)
    m = sp.random(n, d, density=0.25, format="csr", random_state=rng, dtype=np.float64)
    m.data = (1 + rng.poisson(1.0, m.nnz)).astype(dtype)
    m.sort_indices()
    return m


def _adata(n=40, d=30, seed=0, dense=False):
    m = _counts(n, d, seed)
    rng = np.random.default_rng(seed + 100)
    obs = pd.DataFrame({"depth": np.asarray(m.sum(axis=1)).reshape(-1), "good": rng.random(n) < 0.6},
                       index=[f"c{i}" for i in range(n)])
    var = pd.DataFrame({"cells": np.asarray((m != 0).sum(axis=0)).reshape(-1), "hv": rng.random(d) < 0.5},
                       index=[f"p{j}" for j in range(d)])
    ad = mu.AnnData(m.toarray() if dense else m.copy(), obs=obs, var=var,
                    layers={"counts": m.copy(), "dense": m.toarray()},
                    obsm={"X_a": rng.standard_normal((n, 3))}, varm={"L": rng.standard_normal((d, 2))})
    ad.obsp["g"] = sp.random(n, n, density=0.1, format="csr", random_state=rng)
    ad.raw = SimpleNamespace(X=sp.hstack([m, m]).tocsr())
    return ad, m


def _check_subset(ad, ad0, m, rmask, cmask):
    """every slot of ``ad`` is the (rmask, cmask) subset of the untouched twin ``ad0``"""
    want = m[rmask][:, cmask]
    assert ad.shape == want.shape == (int(rmask.sum()), int(cmask.sum()))
    assert ad.n_obs == want.shape[0] and ad.n_vars == want.shape[1]
    assert (ad.X != want).nnz == 0 and ad.X.shape == want.shape
    assert list(ad.obs_names) == list(ad0.obs_names[rmask]) and list(ad.var_names) == list(ad0.var_names[cmask])
    assert ad.obs.equals(ad0.obs[rmask]) and ad.var.equals(ad0.var[cmask])
    assert (ad.layers["counts"] != want).nnz == 0
    assert np.array_equal(ad.layers["dense"], m.toarray()[rmask][:, cmask])
    assert np.array_equal(ad.obsm["X_a"], ad0.obsm["X_a"][rmask]) and np.array_equal(ad.varm["L"], ad0.varm["L"][cmask])
    assert (ad.obsp["g"] != ad0.obsp["g"][rmask][:, rmask]).nnz == 0
    assert (ad.raw.X != ad0.raw.X[rmask]).nnz == 0 and ad.raw.X.shape[1] == ad0.raw.X.shape[1]  # raw: observations only


def _full(n):
    return np.ones(n, dtype=bool)


def test_filter_obs_forms_on_anndata():
    ad0, m = _adata()
    n, d = m.shape
    # a column of .obs with a function
    ad, _ = _adata()
    assert mu.pp.filter_obs(ad, "depth", lambda x: x >= 12) is None
    _check_subset(ad, ad0, m, ad0.obs["depth"].values >= 12, _full(d))
    # a boolean column without a function
    ad, _ = _adata()
    mu.pp.filter_obs(ad, "good")
    _check_subset(ad, ad0, m, ad0.obs["good"].values, _full(d))
    # a name of the other axis: that column of X
    ad, _ = _adata()
    mu.pp.filter_obs(ad, "p3", lambda x: x > 0)
    _check_subset(ad, ad0, m, m[:, 3].toarray().reshape(-1) > 0, _full(d))
    # a sequence of names (the object's own order is kept, unknown names are ignored)
    ad, _ = _adata()
    mu.pp.filter_obs(ad, ["c7", "c2", "c30", "nobody"])
    assert list(ad.obs_names) == ["c2", "c7", "c30"]
    _check_subset(ad, ad0, m, np.isin(np.arange(n), [2, 7, 30]), _full(d))
    # a boolean array
    mask = np.arange(n) % 3 != 0
    ad, _ = _adata()
    mu.pp.filter_obs(ad, mask)
    _check_subset(ad, ad0, m, mask, _full(d))
    ad, _ = _adata()
    mu.pp.filter_obs(ad, list(mask))
    _check_subset(ad, ad0, m, mask, _full(d))


def test_filter_var_forms_on_anndata():
    ad0, m = _adata()
    n, d = m.shape
    ad, _ = _adata()
    assert mu.pp.filter_var(ad, "cells", lambda x: x >= 10) is None
    _check_subset(ad, ad0, m, _full(n), ad0.var["cells"].values >= 10)
    ad, _ = _adata()
    mu.pp.filter_var(ad, "hv")
    _check_subset(ad, ad0, m, _full(n), ad0.var["hv"].values)
    ad, _ = _adata()
    mu.pp.filter_var(ad, "c5", lambda x: x == 0)  # a row of X
    _check_subset(ad, ad0, m, _full(n), m[5].toarray().reshape(-1) == 0)
    ad, _ = _adata()
    mu.pp.filter_var(ad, pd.Index(["p9", "p1"]))
    assert list(ad.var_names) == ["p1", "p9"]
    mask = np.arange(d) % 2 == 1
    ad, _ = _adata()
    mu.pp.filter_var(ad, mask)
    _check_subset(ad, ad0, m, _full(n), mask)
    # both axes, one after the other; then everything dropped on one axis
    mu.pp.filter_obs(ad, "good")
    _check_subset(ad, ad0, m, ad0.obs["good"].values, mask)
    mu.pp.filter_var(ad, np.zeros(ad.n_vars, dtype=bool))
    assert ad.shape == (int(ad0.obs["good"].sum()), 0) and ad.X.shape == ad.shape and ad.X.nnz == 0


def test_filter_dense_x():
    ad, m = _adata(dense=True)
    keep = ad.obs["depth"].values >= 12
    mu.pp.filter_obs(ad, "depth", lambda x: x >= 12)
    assert np.array_equal(ad.X, m.toarray()[keep]) and ad.shape == (int(keep.sum()), m.shape[1])
    cols = ad.X[2] > 0
    mu.pp.filter_var(ad, ad.obs_names[2], lambda x: x > 0)
    assert np.array_equal(ad.X, m.toarray()[keep][:, cols])


@pytest.mark.parametrize("fn,attr,other", [(mu.pp.filter_obs, "obs", "var"), (mu.pp.filter_var, "var", "obs")])
def test_filter_errors(fn, attr, other):
    ad, _ = _adata()
    numeric, name = ("depth", "c1") if attr == "obs" else ("cells", "p1")
    view = ad[np.arange(10)] if attr == "obs" else ad[:, np.arange(10)]
    with pytest.raises(ValueError, match="The provided adata is a view. In-place filtering does not operate on views."):
        fn(view, numeric, lambda x: x > 0)
    with pytest.raises(ValueError, match=f"Function has to be provided since {numeric} is not boolean"):
        fn(ad, numeric)
    with pytest.raises(ValueError, match=f"When providing {attr}_names directly, func has to be None."):
        fn(ad, [name], lambda x: x)
    with pytest.raises(ValueError, match=f"Column name from .{attr} or one of the {other}_names was expected but got nope."):
        fn(ad, "nope", lambda x: x)
    assert ad.shape == (40, 30)  # nothing was changed on the way to an error


def _mdata():
    a, ma = _adata(seed=1)
    b, mb = _adata(n=40, d=12, seed=2)
    # the second modality holds a subset of the cells, in an order of its own
    order = np.random.default_rng(3).permutation(40)[:25]
    b = b[order]
    b._init_as_actual()
    b.var.index = pd.Index([f"g{j}" for j in range(12)])
    md = mu.MuData({"atac": a, "rna": b})
    md.obs["batch"] = (np.arange(md.n_obs) % 4).astype(np.int64)
    md.obs["ok"] = np.arange(md.n_obs) % 5 != 0
    md.obsm["X_joint"] = np.arange(md.n_obs * 2, dtype=np.float64).reshape(-1, 2)
    return md, ma, mb[order]


def test_filter_obs_on_mudata():
    md, ma, mb = _mdata()
    rna_names = list(md["rna"].obs_names)
    # a column of the MuData's own .obs with a function
    keep = md.obs["batch"].values != 2
    kept = set(md.obs_names[keep])
    joint = md.obsm["X_joint"][keep]
    assert mu.pp.filter_obs(md, "batch", lambda x: x != 2) is None
    assert set(md.obs_names) == kept and md.n_obs == len(kept)
    assert np.array_equal(md.obsm["X_joint"], joint)
    assert list(md["atac"].obs_names) == [f"c{i}" for i in range(40) if f"c{i}" in kept]
    assert list(md["rna"].obs_names) == [c for c in rna_names if c in kept]  # its own order
    sel = np.array([c in kept for c in rna_names])
    assert (md["rna"].X != mb[sel]).nnz == 0 and md["rna"].shape == (int(sel.sum()), 12)
    assert (md["atac"].X != ma[np.array([f"c{i}" in kept for i in range(40)])]).nnz == 0
    assert md["rna"].obsm["X_a"].shape[0] == md["rna"].n_obs and md["rna"].layers["counts"].shape == md["rna"].shape
    # a boolean column without a function, then names, then a boolean array
    ok = md.obs["ok"].values.astype(bool)
    kept = set(md.obs_names[ok])
    mu.pp.filter_obs(md, "ok")
    assert set(md.obs_names) == kept
    names = [c for c in md.obs_names if c in set(rna_names)][:4] + ["c39" if "c39" in kept else md.obs_names[0]]
    mu.pp.filter_obs(md, names)
    assert set(md.obs_names) == set(names) and set(md["rna"].obs_names) == set(names) & set(rna_names)
    assert set(md["atac"].obs_names) == set(names)
    mask = np.arange(md.n_obs) != 1
    want = set(md.obs_names[mask])
    mu.pp.filter_obs(md, mask)
    assert set(md.obs_names) == want and md.shape[0] == len(want)


def test_filter_var_on_mudata_and_errors():
    md, ma, mb = _mdata()
    mu.pp.filter_var(md, ["p3", "g5", "p1", "g0", "p29"])
    assert list(md["atac"].var_names) == ["p1", "p3", "p29"] and list(md["rna"].var_names) == ["g0", "g5"]
    assert list(md.var_names) == ["p1", "p3", "p29", "g0", "g5"] and md.n_vars == 5
    assert (md["atac"].X != ma[:, [1, 3, 29]]).nnz == 0 and (md["rna"].X != mb[:, [0, 5]]).nnz == 0
    assert md["atac"].varm["L"].shape == (3, 2) and md["atac"].shape == (40, 3)
    mu.pp.filter_var(md, "hv")  # a boolean column shared by the modalities
    assert md["atac"].var["hv"].all() and md["rna"].var["hv"].all() and md.n_vars == md["atac"].n_vars + md["rna"].n_vars
    with pytest.raises(ValueError, match="Function has to be provided since cells is not boolean"):
        mu.pp.filter_var(md, "cells")
    with pytest.raises(ValueError, match="When providing var_names directly, func has to be None."):
        mu.pp.filter_var(md, ["p1"], lambda x: x)
    with pytest.raises(ValueError, match="Column name from .obs or one of the var_names was expected but got nope."):
        mu.pp.filter_obs(md, "nope", lambda x: x)


def _awkward_csr(dtype=np.float32):
    """rows stored in DESCENDING column order, explicitly stored zeros, an empty first and last row"""
    rng = np.random.default_rng(7)
    n, d = 23, 37
    indptr, indices, data = [0], [], []
    for i in range(n):
        k = 0 if i in (0, n - 1, 9) else int(rng.integers(1, d))
        cols = np.sort(rng.choice(d, k, replace=False))[::-1]
        vals = rng.integers(1, 9, k).astype(dtype)
        vals[rng.random(k) < 0.2] = 0  # explicit zeros
        indices += list(cols)
        data += list(vals)
        indptr.append(len(indices))
    m = sp.csr_matrix((np.asarray(data, dtype=dtype), np.asarray(indices, dtype=np.int32), np.asarray(indptr, dtype=np.int64)),
                      shape=(n, d))
    assert (m.data == 0).any() and not m.has_sorted_indices
    return m


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_fallback_arrays_equal_scipy_slicing(dtype):
    m = _awkward_csr(dtype)
    n, d = m.shape
    rng = np.random.default_rng(1)
    X = BE.upload_csr(m.indptr, m.indices, m.data, m.shape)
    cases = [(rng.random(n) < 0.6, rng.random(d) < 0.5), (_full(n), _full(d)), (np.zeros(n, bool), _full(d)),
             (_full(n), np.zeros(d, bool)), (np.arange(n) == 0, _full(d)), (np.arange(n) == n - 2, np.arange(d) == d - 1)]
    for rmask, cmask in cases:
        for want in (m[rmask][:, cmask], m[:, cmask][rmask]):  # scipy: stored order and explicit zeros, either way round
            Y = submatrix_device(BE, X, rmask, cmask)
            assert Y.shape == want.shape
            assert np.array_equal(Y.indptr.numpy(), want.indptr) and Y.indptr.dtype == torch.int64
            assert np.array_equal(Y.indices.numpy(), want.indices) and Y.indices.dtype == torch.int32
            assert Y.values.numpy().tobytes() == want.data.tobytes()
    Y = submatrix_device(BE, X, cases[0][0], None)
    assert np.array_equal(Y.indices.numpy(), m[cases[0][0]].indices) and (Y.values == 0).any()


def _tenx(n_cells=230, n_feat=90, seed=0):
    rng = np.random.default_rng(seed)
    m = sp.random(n_cells, n_feat, density=0.1, format="csr", random_state=rng, dtype=np.float64)
    m.data = (1 + rng.poisson(0.5, m.nnz)).astype(np.float32)
    m.sort_indices()
    matrix = {"data": m.data, "indices": m.indices.astype(np.int64), "indptr": m.indptr.astype(np.int64),
              "shape": np.array([n_feat, n_cells])}
    return m, matrix


def test_residency_survives_qc_and_both_filters():
    from muon_amd import atac as ac
    from oracle import tfidf_oracle

    m, matrix = _tenx(seed=3)
    be = CpuTestBackend()
    ad = mio.read_10x_arrays(matrix, backend=be, atac_only=False, barcodes=[f"c{i}" for i in range(m.shape[0])],
                             feature_names=[f"f{j}" for j in range(m.shape[1])])
    ad.layers["counts"] = ad.X  # the same matrix object: its copy is found again
    uploads = []
    orig = be.upload_csr
    be.upload_csr = lambda *a, **k: (uploads.append(1), orig(*a, **k))[1]
    try:
        mu.pp.qc_metrics(ad, backend=be)
        mu.pp.filter_var(ad, "n_cells_by_counts", lambda x: x >= 20)
        mu.pp.filter_obs(ad, "n_genes_by_counts", lambda x: x >= 7)
        X = resident(ad.X, be)
        assert X is not None and X.shape == ad.shape and resident(ad.layers["counts"], be) is not None
        assert np.array_equal(X.indices.numpy(), ad.X.indices) and np.array_equal(X.indptr.numpy(), ad.X.indptr)
        assert np.array_equal(X.values.numpy(), ad.X.data)
        ac.pp.tfidf(ad, backend=be)
    finally:
        be.upload_csr = orig
    assert not uploads
    cols = np.asarray((m != 0).sum(axis=0)).reshape(-1) >= 20
    rows = np.asarray((m != 0).sum(axis=1)).reshape(-1) >= 7
    assert 0 < rows.sum() < m.shape[0] and 0 < cols.sum() < m.shape[1]
    ref = tfidf_oracle.canonical(tfidf_oracle.tfidf(m[rows][:, cols].astype(np.float32)))
    assert ad.shape == ref.shape and np.array_equal(ad.X.indices, ref.indices)
    assert np.allclose(ad.X.data, ref.data, rtol=1e-5)
    # without a backend argument the copy's own backend is found (and no other is constructed)
    ad2 = mio.read_10x_arrays(matrix, backend=be, atac_only=False)
    mu.pp.filter_obs(ad2, rows)
    assert resident(ad2.X, be) is not None and resident(ad2.X, be).shape == (int(rows.sum()), m.shape[1])


def test_host_only_objects_make_no_backend_call():
    ad, m = _adata()
    mu.pp.filter_var(ad, "cells", lambda x: x >= 10, backend=_NoBackend())
    mu.pp.filter_obs(ad, "good", backend=_NoBackend())
    assert not hasattr(ad.X, DEVICE_ATTR) and ad.shape == (int(ad.obs["good"].sum()), int((ad.var["cells"] >= 10).sum()))
    ad, m = _adata()
    mu.pp.filter_obs(ad, "good")  # no backend at all: none is constructed (there is no GPU to construct one on)
    assert not hasattr(ad.X, DEVICE_ATTR)
    # a copy that no longer describes the host matrix is not used (and not subset)
    ad, m = _adata()
    attach_device(ad.X, BE.upload_csr(m.indptr, m.indices, m.data, m.shape), BE)
    ad.X.data[0] += 1
    mu.pp.filter_obs(ad, "good", backend=BE)
    assert not hasattr(ad.X, DEVICE_ATTR)


def _np_qc(m):
    a = m.toarray().astype(np.float64)
    nz = (a != 0)
    return nz.sum(axis=1), nz.sum(axis=0)


@pytest.mark.parametrize("dense", [False, True])
def test_qc_metrics_against_numpy(dense):
    ad, m = _adata(seed=5, dense=dense)
    m = m.copy()
    m.data[::7] = 0  # explicitly stored zeros: not counted
    if not dense:
        ad.X = m.copy()
    else:
        ad.X = m.toarray()
    n, d = m.shape
    obs, var = mu.pp.qc_metrics(ad, inplace=False, backend=BE)
    assert "n_genes_by_counts" not in ad.obs.columns
    rn, cn = _np_qc(m)
    assert np.array_equal(obs["n_genes_by_counts"].values, rn) and np.array_equal(var["n_cells_by_counts"].values, cn)
    assert (m.getnnz(axis=1) != rn).any()  # (the deliberate difference from getnnz)
    Xd = BE.upload_csr(m.indptr, m.indices, m.data, m.shape)
    rs, cs = (t.numpy() for t in BE.row_col_sums(Xd))
    assert np.array_equal(obs["total_counts"].values, rs) and np.array_equal(var["total_counts"].values, cs)
    assert obs["total_counts"].dtype == np.float64
    assert np.array_equal(var["mean_counts"].values, cs / n)
    assert np.array_equal(var["pct_dropout_by_counts"].values, (1.0 - cn / n) * 100.0)
    for frame, c in ((obs, "n_genes_by_counts"), (obs, "total_counts"), (var, "mean_counts"), (var, "total_counts")):
        assert np.array_equal(frame["log1p_" + c].values, np.log1p(frame[c].values))
    assert list(obs.columns) == ["n_genes_by_counts", "log1p_n_genes_by_counts", "total_counts", "log1p_total_counts"]
    assert list(var.columns) == ["n_cells_by_counts", "mean_counts", "log1p_mean_counts", "pct_dropout_by_counts",
                                 "total_counts", "log1p_total_counts"]
    # in place, without the log1p companions, from a layer
    ad.layers["c2"] = ad.X
    assert mu.pp.qc_metrics(ad, layer="c2", log1p=False, backend=BE) is None
    assert list(ad.obs.columns[-2:]) == ["n_genes_by_counts", "total_counts"]
    assert list(ad.var.columns[-4:]) == ["n_cells_by_counts", "mean_counts", "pct_dropout_by_counts", "total_counts"]
    assert np.array_equal(ad.var["n_cells_by_counts"].values, cn)
    if not dense:  # the upload was the pipeline's only one: the copy stays with the matrix
        assert resident(ad.X, BE) is not None
    with pytest.raises(TypeError):
        mu.pp.qc_metrics(np.zeros((2, 2)), backend=BE)


def test_qc_counts_nan_as_nonzero():
    m = _counts(12, 9, seed=2)
    m.data[3] = np.nan
    ad = mu.AnnData(m)
    obs, var = mu.pp.qc_metrics(ad, inplace=False, backend=BE)
    rn, cn = _np_qc(m)
    assert np.array_equal(obs["n_genes_by_counts"].values, rn) and np.array_equal(var["n_cells_by_counts"].values, cn)
    assert np.isnan(obs["total_counts"].values).sum() == 1


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _qc_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import muon_amd as mu
        from muon_amd._comm import TorchDistComm
        from tests.cpu_backend import CpuTestBackend
        from tests.test_filter_host import _counts

        m = _counts(61, 45, seed=11)
        lo, hi = (0, 27) if rank == 0 else (27, 61)  # uneven shards
        ad = mu.AnnData(m[lo:hi].copy())
        obs, var = mu.pp.qc_metrics(ad, inplace=False, comm=TorchDistComm(), backend=CpuTestBackend())
        if rank == 0:
            q.put({"var": {c: var[c].values for c in var.columns}, "n_obs_rows": len(obs),
                   "obs_counts": obs["n_genes_by_counts"].values})
    finally:
        dist.barrier()
        dist.destroy_process_group()


def test_qc_metrics_two_row_shards_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_qc_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = q.get(timeout=240)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    m = _counts(61, 45, seed=11)
    obs, var = mu.pp.qc_metrics(mu.AnnData(m.copy()), inplace=False, backend=BE)
    assert got["n_obs_rows"] == 27 and np.array_equal(got["obs_counts"], obs["n_genes_by_counts"].values[:27])
    assert set(got["var"]) == set(var.columns)
    for c in var.columns:  # counts: sums of integers, exact in f64 in any grouping
        assert np.array_equal(got["var"][c], var[c].values), c


def test_tensor_fallback_is_what_the_backend_would_be_asked_for():
    """the operator set of the CPU tests has no csr_submatrix / csr_qc: the tensor forms serve (`_operators.has`)"""
    assert not has(BE, "csr_submatrix") and not has(BE, "csr_qc")
    m = _counts(10, 8, seed=4)
    X = BE.upload_csr(m.indptr, m.indices, m.data, m.shape)
    Y = _submatrix_tensor(X, torch.tensor([1, 4, 9]), torch.tensor([0, -1, 1, -1, 2, 3, -1, 4], dtype=torch.int32), 5)
    want = m[[1, 4, 9]][:, [0, 2, 4, 5, 7]]
    assert np.array_equal(Y.indptr.numpy(), want.indptr) and np.array_equal(Y.indices.numpy(), want.indices)
    assert np.array_equal(Y.values.numpy(), want.data)
