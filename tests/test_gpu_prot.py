"""muon_amd.prot on the device: the moments and per-cell fit kernels of csrc/prot.hip against the reference's own dsb
executing (tests/golden/prot_golden.npz) and against the tensor formulation of muon_amd/_prot/preproc.py on shapes the
fixture does not reach; clr through the row_col_sums kernel; dsb -> knn -> neighbors end to end.

Identities (iteration counts, model choice, sparse pattern, bit-equal repeats) are conditions.  Value bounds are ten
times the deviation measured on an MI355X (DESIGN.md 9.4 records both figures), to leave room for other libm builds."""
import os
import warnings

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

from muon_amd import AnnData, MuData, prot
from muon_amd import pp as mpp
from muon_amd._prot import preproc as P

pytestmark = pytest.mark.gpu

N_EMPTY = 600
# measured on an MI355X: max |dsb - fixture| 9.663e-13 over the f64 cases (the matrix reaches 135: 7e-15 relative) and
# 2.289e-05 for the float32 case (the reference runs its EM and regression in float32 there)
F64_BOUND = 9.7e-12
F32_BOUND = 2.3e-4
# the moments kernel against numpy on the densified 100 000 x 200 matrix: 1.32e-12 (mean) and 1.37e-12 (std), relative.
# That figure is numpy's: `mean(axis=0)` of a row-major matrix adds the 100 000 rows one after the other (pairwise
# summation only runs along the contiguous axis), nearly all of them the same log(pseudocount), so its rounding errors
# line up.  Against the exactly rounded sum (math.fsum) the kernel's mean is held to 1e-15: log(pc) and the final sum
# round once each, the sparse part S1 / n is 0.4 % of the mean.
MOMENTS_BOUND = 1.4e-11
MOMENTS_EXACT_BOUND = 1e-15
# kernel against the tensor formulation - the same statements, another summation order: a sum of d <= 1024 terms moves
# by at most d * 2^-53 = 1.1e-13 relative, the EM map is a contraction near its fixed point; measured 6.5e-16 on the
# BICs and background means, 2.8e-15 on the final matrix at d = 1024
KERNEL_VS_TENSOR = 1e-12


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "prot_golden.npz"))


def _names(n, prefix, start=0):
    return pd.Index([f"{prefix}{i}" for i in range(start, start + n)], dtype=object)


def _inputs(gold, kind="int_csr"):
    counts = gold["prot_counts"].astype(np.int64)
    obs_all, var = _names(counts.shape[0], "d"), _names(counts.shape[1], "prot")
    if kind == "f32_dense":
        cells, raw = counts[N_EMPTY:].astype(np.float32), counts.astype(np.float32)
    else:
        cells, raw = sp.csr_matrix(counts[N_EMPTY:]), sp.csr_matrix(counts)
    return (AnnData(cells, obs=pd.DataFrame(index=obs_all[N_EMPTY:]), var=pd.DataFrame(index=var)),
            AnnData(raw, obs=pd.DataFrame(index=obs_all), var=pd.DataFrame(index=var)))


class _Spy:
    """Forwards to a backend and counts the calls of the prot kernels."""

    def __init__(self, be):
        self._be, self.calls = be, {"prot_dsb_fit": 0, "prot_log_moments": 0}

    def __getattr__(self, name):
        got = getattr(self._be, name)
        if name in self.calls:
            def counted(*a, **k):
                self.calls[name] += 1
                return got(*a, **k)

            return counted
        return got


CASES = {
    "int_csr": {},
    "f32_dense": {},
    "meansub": dict(scale_factor="mean_subtract"),
    "isotype": dict(isotype_controls=["prot5", "prot17", "prot31"]),
    "clip": dict(quantile_clipping=True),
    "nodenoise": dict(denoise_counts=False),
}


@pytest.mark.parametrize("tag", list(CASES))
def test_dsb_kernels_match_the_reference_executing(gold, hip, tag):
    cells, raw = _inputs(gold, tag)
    spy = _Spy(hip)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert prot.pp.dsb(cells, raw, random_state=int(gold["seed"][0]), backend=spy, **CASES[tag]) is None
    assert spy.calls["prot_log_moments"] == 1 and spy.calls["prot_dsb_fit"] == (0 if tag == "nodenoise" else 1)
    ref = gold[f"dsb_{tag}"]
    assert cells.X.dtype == ref.dtype
    dev = float(np.abs(cells.X.astype(np.float64) - ref).max())
    bound = F32_BOUND if ref.dtype == np.float32 else F64_BOUND
    print(f"MEASURE dsb {tag}: max |dsb - fixture| = {dev:.4g} (bound {bound:.3g}, max |fixture| {np.abs(ref).max():.4g})")
    assert dev <= bound


@pytest.mark.parametrize("tag", ["int_csr", "f32_dense", "meansub"])
def test_kernel_iteration_counts_and_model_choice_are_the_references(gold, hip, tag):
    cells, raw = _inputs(gold, tag)
    diag = {}
    P._dsb_arrays(cells.X, raw.X[:N_EMPTY], random_state=int(gold["seed"][0]), backend=hip, diagnostics=diag,
                  **CASES[tag])
    n_iter, bic, bg = gold[f"dsb_{tag}_n_iter"], gold[f"dsb_{tag}_bic"], gold[f"dsb_{tag}_bg"]
    assert np.array_equal(diag["n_iter"], n_iter)
    assert np.array_equal(diag["bic"][:, 0] < diag["bic"][:, 1], bic[:, 0] < bic[:, 1])
    dev_bic = float(np.max(np.abs(diag["bic"] - bic) / np.abs(bic)))
    dev_bg = float(np.max(np.abs(diag["bgmeans"] - bg)))
    print(f"MEASURE fits {tag}: BIC rel {dev_bic:.4g}, background mean abs {dev_bg:.4g}")
    tol = 32 * 2.0 ** -23 if tag == "f32_dense" else 1e-12
    assert dev_bic <= tol and dev_bg <= tol * max(1.0, float(np.abs(bg).max()))


def test_add_layer_and_unfiltered_mudata_on_the_gpu(gold, hip):
    cells, raw = _inputs(gold)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        prot.pp.dsb(cells, raw, add_layer=True, random_state=int(gold["seed"][0]), backend=hip)
    assert sp.issparse(cells.X) and np.abs(cells.layers["dsb"] - gold["dsb_int_csr"]).max() <= F64_BOUND
    counts = gold["prot_counts"].astype(np.int64)
    obs_all = _names(counts.shape[0], "d")
    md = MuData({"prot": AnnData(sp.csr_matrix(counts), obs=pd.DataFrame(index=obs_all)),
                 "rna": AnnData(sp.csr_matrix(gold["rna_rowsum"].astype(np.int64)[:, None]),
                                obs=pd.DataFrame(index=obs_all))})
    e0, e1, c0, c1 = gold["raw_none_ranges"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = prot.pp.dsb(md, empty_counts_range=(e0, e1), cell_counts_range=(c0, c1),
                          random_state=int(gold["seed"][0]), backend=hip)
    assert list(got.mod["prot"].obs_names) == list(obs_all[N_EMPTY:])
    assert np.abs(got.mod["prot"].X - gold["dsb_int_csr"]).max() <= F64_BOUND


def _synthetic(n, d, seed, n_empty=300):
    rng = np.random.default_rng(seed)
    ambient = rng.gamma(2.0, 1.5, d)
    empty = rng.poisson(ambient * rng.gamma(4.0, 0.25, (n_empty, 1))).astype(np.float64)
    cells = rng.poisson(ambient * rng.gamma(6.0, 1.0, (n, 1)))
    cells = cells + (rng.random((n, d)) < 0.3) * rng.poisson(300.0, (n, d))
    return cells.astype(np.float64), empty


def _compare_fit(hip, X, pc, mean, std, resp, what):
    z_k, bg_k, bic_k, it_k = hip.prot_dsb_fit(X, pc, mean, std, resp)
    z_t, bg_t, bic_t, it_t = P._fit_torch(X, pc, mean, std, resp)
    assert torch.equal(it_k, it_t), what
    assert torch.equal(bic_k[:, 0] < bic_k[:, 1], bic_t[:, 0] < bic_t[:, 1]), what
    scale = max(1.0, float(z_t.abs().max()))
    dz = float((z_k - z_t).abs().max()) / scale
    dbg = float((bg_k - bg_t).abs().max()) / scale
    dbic = float(((bic_k - bic_t).abs() / bic_t.abs().clamp_min(1.0)).max())
    print(f"MEASURE kernel vs tensor {what}: scaled {dz:.3g}, background mean {dbg:.3g}, BIC {dbic:.3g}, "
          f"n_iter max {int(it_k.max())}")
    assert dz <= KERNEL_VS_TENSOR and dbg <= KERNEL_VS_TENSOR and dbic <= KERNEL_VS_TENSOR, what
    return z_k, bg_k, bic_k, it_k


# (both sides of every edge of the proteins-per-lane ladder: 64 | 65, 128 | 129, 256 | 257, 512 | 513)
@pytest.mark.parametrize("d", [1, 2, 63, 64, 65, 128, 129, 256, 257, 300, 512, 513, 1024])
def test_fit_kernel_equals_the_tensor_formulation(hip, d):
    assert hip.prot_max_proteins() == 1024
    n = 97 if d < 1024 else 33
    cells, empty = _synthetic(n, d, seed=d)
    Xc, Xe = hip.to_device(cells, np.float64), hip.to_device(empty, np.float64)
    mean, std = hip.prot_log_moments(Xe, 10.0)
    shared = hip.to_device(np.random.RandomState(d).uniform(size=(d, 2)), np.float64)
    _compare_fit(hip, Xc, 10.0, mean, std, shared, f"d={d} dense shared")
    per_cell = hip.to_device(np.random.RandomState(d + 1).uniform(size=(n, 2, d, 2)), np.float64)
    m = sp.csr_matrix(cells)
    Xs = hip.upload_csr(m.indptr, m.indices, m.data, m.shape, slab_ptr=False)
    a = _compare_fit(hip, Xs, 10.0, mean, None, per_cell, f"d={d} csr per-cell mean_subtract")
    b = hip.prot_dsb_fit(Xc, 10.0, mean, None, per_cell)
    assert all(torch.equal(x, y) for x, y in zip(a, b))  # a CSR row scattered over zeros IS the dense row


def test_panel_past_the_limit_routes_to_the_tensor_formulation(hip):
    d = hip.prot_max_proteins() + 1
    cells, empty = _synthetic(21, d, seed=9)
    spy, diag, diag_t = _Spy(hip), {}, {}
    z = P._dsb_arrays(cells, empty, random_state=5, backend=spy, diagnostics=diag)
    assert spy.calls == {"prot_dsb_fit": 0, "prot_log_moments": 0}
    z_t = P._dsb_arrays(cells, empty, random_state=5, backend=hip, force_tensor=True, diagnostics=diag_t)
    assert torch.equal(z, z_t) and np.array_equal(diag["n_iter"], diag_t["n_iter"])
    # one protein fewer: the kernels run, and agree with the formulation the wide panel took
    spy, diag_k, diag_t = _Spy(hip), {}, {}
    zk = P._dsb_arrays(cells[:, :-1], empty[:, :-1], random_state=5, backend=spy, diagnostics=diag_k)
    assert spy.calls == {"prot_dsb_fit": 1, "prot_log_moments": 1}
    zt = P._dsb_arrays(cells[:, :-1], empty[:, :-1], random_state=5, backend=hip, force_tensor=True, diagnostics=diag_t)
    assert np.array_equal(diag_k["n_iter"], diag_t["n_iter"])
    assert np.array_equal(diag_k["bic"][:, 0] < diag_k["bic"][:, 1], diag_t["bic"][:, 0] < diag_t["bic"][:, 1])
    dev = float((zk - zt).abs().max()) / float(zt.abs().max())
    print(f"MEASURE dsb kernels vs tensor at d=1024: {dev:.3g}")
    assert dev <= KERNEL_VS_TENSOR


def test_all_zero_cell_and_empty_csr_row(hip):
    cells, empty = _synthetic(40, 50, seed=3)
    cells[7] = 0.0
    cells[39] = 0.0
    m = sp.csr_matrix(cells)
    assert m.indptr[8] == m.indptr[7]
    Xs = hip.upload_csr(m.indptr, m.indices, m.data, m.shape, slab_ptr=False)
    Xe = hip.to_device(empty, np.float64)
    mean, std = hip.prot_log_moments(Xe, 10.0)
    resp = hip.to_device(np.random.RandomState(0).uniform(size=(50, 2)), np.float64)
    z, bg, bic, it = _compare_fit(hip, Xs, 10.0, mean, std, resp, "zero cell / empty row")
    want = (np.log(10.0) - hip.to_host(mean)) / hip.to_host(std)
    assert np.abs(hip.to_host(z[7]) - want).max() < 1e-14 and torch.equal(z[7], z[39])
    assert torch.isfinite(bg).all() and torch.isfinite(bic).all() and bg[7] == bg[39] and int(it.max()) < 100
    dense = hip.prot_dsb_fit(hip.to_device(cells, np.float64), 10.0, mean, std, resp)
    assert all(torch.equal(x, y) for x, y in zip((z, bg, bic, it), dense))


def test_moments_kernel_on_100000_sparse_droplets(hip):
    n, d = 100_000, 200
    m = sp.random(n, d, density=0.01, format="csr", random_state=1, dtype=np.float64)
    m.data = np.ceil(m.data * 30)
    Xe = hip.upload_csr(m.indptr, m.indices, m.data, m.shape, slab_ptr=False)
    mean, std = (hip.to_host(t) for t in hip.prot_log_moments(Xe, 10.0))
    le = np.log(m.toarray() + 10.0)
    rm, rs = le.mean(axis=0, dtype=np.float64), le.std(axis=0, ddof=1, dtype=np.float64)
    dm, ds = float(np.max(np.abs(mean - rm) / np.abs(rm))), float(np.max(np.abs(std - rs) / rs))
    print(f"MEASURE moments csr 100000 x 200 at 1%: mean rel {dm:.3g}, std rel {ds:.3g}")
    assert dm <= MOMENTS_BOUND and ds <= MOMENTS_BOUND
    import math

    dense = m.toarray()
    exact = np.array([math.fsum(np.log(dense[:, j] + 10.0)) / n for j in range(0, d, 8)])
    de = float(np.max(np.abs(mean[::8] - exact) / exact))
    print(f"MEASURE moments csr mean against the exactly rounded sum: {de:.3g}")
    assert de <= MOMENTS_EXACT_BOUND
    # the dense variant on a slice, float32 too (numpy takes that logarithm in float32)
    sub = m[:5000].toarray()
    for dt in (np.float64, np.float32):
        mean, std = (hip.to_host(t) for t in hip.prot_log_moments(hip.to_device(sub.astype(dt), dt), 10.0))
        le = np.log(sub.astype(dt) + 10)
        assert le.dtype == dt
        rm, rs = le.mean(axis=0, dtype=np.float64), le.std(axis=0, ddof=1, dtype=np.float64)
        # float32: numpy's logf and the kernel's rounded f64 logarithm may differ by one float32 ulp of a value near 3
        # (2.4e-7) in any entry: that much on the mean (about 2.3), and as a perturbation of rms 2.4e-7 on a standard
        # deviation of about 0.1
        tol_m, tol_s = (MOMENTS_BOUND, MOMENTS_BOUND) if dt == np.float64 else (2.0 ** -22, 1e-5)
        dm, ds = float(np.max(np.abs(mean - rm) / np.abs(rm))), float(np.max(np.abs(std - rs) / rs))
        print(f"MEASURE moments dense {np.dtype(dt).name}: mean rel {dm:.3g}, std rel {ds:.3g}")
        assert dm <= tol_m and ds <= tol_s


def test_two_runs_agree_bit_for_bit(gold, hip):
    runs = []
    for _ in range(2):
        cells, raw = _inputs(gold)
        diag = {}
        z = P._dsb_arrays(cells.X, raw.X[:N_EMPTY], random_state=3, backend=hip, diagnostics=diag)
        runs.append((hip.to_host(z), diag))
    (z0, d0), (z1, d1) = runs
    assert np.array_equal(z0, z1)
    for k in ("mean", "std", "bgmeans", "bic", "n_iter", "scaled"):
        assert np.array_equal(d0[k], d1[k]), k
    m = sp.random(30_000, 64, density=0.02, format="csr", random_state=2, dtype=np.float64)
    Xe = hip.upload_csr(m.indptr, m.indices, m.data, m.shape, slab_ptr=False)
    a, b = hip.prot_log_moments(Xe, 1.0), hip.prot_log_moments(Xe, 1.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("fmt", ["csr", "csc"])
@pytest.mark.parametrize("axis", [0, 1])
def test_clr_on_the_gpu(gold, hip, fmt, axis):
    x = gold["clr_x"]
    m = sp.csr_matrix(x) if fmt == "csr" else sp.csc_matrix(x)
    ad = AnnData(m.copy())
    prot.pp.clr(ad, axis=axis, backend=hip)
    assert ad.X.format == fmt and np.array_equal(ad.X.indices, m.indices) and np.array_equal(ad.X.indptr, m.indptr)
    dev = float(np.abs(ad.X.toarray() - gold[f"clr_sparse_seurat_{axis}"]).max())
    print(f"MEASURE clr seurat {fmt} axis {axis}: {dev:.3g}")
    assert dev <= 1e-13
    for flavor in ("seurat", "stoeckius", "standard"):
        src = gold["clr_xp"] if flavor == "standard" else x
        ad = AnnData(src.copy())
        prot.pp.clr(ad, axis=axis, flavor=flavor, backend=hip)
        ref = gold[f"clr_dense_{flavor}_{axis}"]
        np.testing.assert_array_equal(np.isfinite(ad.X), np.isfinite(ref))
        ok = np.isfinite(ref)
        assert np.abs(ad.X[ok] - ref[ok]).max() <= 1e-13


def test_dsb_feeds_knn_and_weighted_neighbours(hip):
    """The CITE-seq workflow: dsb on the protein counts, knn per modality, then mu.pp.neighbors."""
    rng = np.random.default_rng(0)
    n, d, k = 600, 48, 4
    lab = rng.integers(0, k, n)
    rna = AnnData(rng.standard_normal((k, 15))[lab] * 2 + rng.standard_normal((n, 15)))
    marker = rng.random((k, d)) < 0.3
    counts = rng.poisson(6.0, (n, d)) + marker[lab] * rng.poisson(250.0, (n, d))
    empty = rng.poisson(2.0, (2000, d))
    names = _names(n, "cell")
    rna.obs_names = names
    adt = AnnData(sp.csr_matrix(counts), obs=pd.DataFrame(index=names))
    raw = AnnData(sp.csr_matrix(np.vstack([empty, counts])),
                  obs=pd.DataFrame(index=_names(2000, "empty").append(names)))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        prot.pp.dsb(adt, raw, random_state=0, backend=hip)
    assert isinstance(adt.X, np.ndarray) and adt.X.shape == (n, d) and np.isfinite(adt.X).all()
    md = MuData({"rna": rna, "prot": adt})
    mpp.knn(md.mod["rna"], n_neighbors=15, use_rep="X", backend=hip)
    mpp.knn(md.mod["prot"], n_neighbors=15, use_rep="X", backend=hip)
    mpp.neighbors(md, n_multineighbors=60, backend=hip)
    g = md.obsp["distances"]
    assert g.shape == (n, n) and md.obsp["connectivities"].shape == (n, n)
    assert "neighbors" in md.uns and "rna:mod_weight" in md.obs and "prot:mod_weight" in md.obs
    agree = np.mean(lab[g.indices] == np.repeat(lab, np.diff(g.indptr)))
    assert agree > 0.9, agree
