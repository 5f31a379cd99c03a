"""muon_amd.prot.pp.dsb / clr without a GPU: the whole of both functions through tests/cpu_backend.CpuTestBackend, which
has none of the prot kernels - so the tensor formulation of muon_amd/_prot/preproc.py runs - against
tests/golden/prot_golden.npz (the reference's own dsb / clr executing, tests/golden/make_prot_golden.py).

Identities (iteration counts of both mixtures, the model chosen, the sparse pattern) are conditions for every cell.
Value bounds: f64 cases 1e-10 absolute - the reference's matrix reaches 135, a numpy restatement of scikit-learn's EM
agreed with GaussianMixture to 1e-14 relative, and a deviation beyond 1e-10 would be an arithmetic difference, not
rounding.  The float32 case: the reference runs the EM and the regression IN float32 there, this package in f64 on the
float32-rounded matrix; 32 float32 roundings of the largest entry (32 * 2^-23 * max|ref|, about 5e-4) bound that."""
import warnings

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

from muon_amd import AnnData, MuData, prot
from muon_amd._prot import preproc as P
from tests.cpu_backend import CpuTestBackend

N_EMPTY = 600
F64_BOUND = 1e-10


@pytest.fixture(scope="module")
def gold(golden_dir):
    import os

    return np.load(os.path.join(golden_dir, "prot_golden.npz"))


@pytest.fixture(scope="module")
def be():
    return CpuTestBackend()


def _names(n, prefix, start=0):
    return pd.Index([f"{prefix}{i}" for i in range(start, start + n)], dtype=object)


def _adata(x, obs_names, var_names):
    return AnnData(x, obs=pd.DataFrame(index=obs_names), var=pd.DataFrame(index=var_names))


def _inputs(gold, kind="int_csr"):
    prot_counts = gold["prot_counts"].astype(np.int64)
    n_all, d = prot_counts.shape
    obs_all, var = _names(n_all, "d"), _names(d, "prot")
    if kind == "f32_dense":
        cells, raw = prot_counts[N_EMPTY:].astype(np.float32), prot_counts.astype(np.float32)
    elif kind == "f64_dense":
        cells, raw = prot_counts[N_EMPTY:].astype(np.float64), prot_counts.astype(np.float64)
    else:
        cells, raw = sp.csr_matrix(prot_counts[N_EMPTY:]), sp.csr_matrix(prot_counts)
    return _adata(cells, obs_all[N_EMPTY:], var), _adata(raw, obs_all, var)


def _bound(gold, tag):
    ref = gold[f"dsb_{tag}"]
    return 32 * 2.0 ** -23 * float(np.abs(ref).max()) if ref.dtype == np.float32 else F64_BOUND


CASES = {
    "int_csr": {},
    "f32_dense": {},
    "meansub": dict(scale_factor="mean_subtract"),
    "isotype": dict(isotype_controls=["prot5", "prot17", "prot31"]),
    "clip": dict(quantile_clipping=True),
    "nodenoise": dict(denoise_counts=False),
}


@pytest.mark.parametrize("tag", list(CASES))
def test_dsb_matches_the_reference_executing(gold, be, tag):
    cells, raw = _inputs(gold, tag)
    before = cells.X
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ret = prot.pp.dsb(cells, raw, random_state=int(gold["seed"][0]), backend=be, **CASES[tag])
    assert ret is None and cells.X is not before and "dsb" not in cells.layers
    ref = gold[f"dsb_{tag}"]
    assert isinstance(cells.X, np.ndarray) and cells.X.dtype == ref.dtype and cells.X.shape == ref.shape
    dev = float(np.abs(cells.X.astype(np.float64) - ref).max())
    print(f"{tag}: max |dsb - reference| = {dev:.3g} (bound {_bound(gold, tag):.3g})")
    assert dev <= _bound(gold, tag)


@pytest.mark.parametrize("tag", ["int_csr", "f32_dense", "meansub"])
def test_iteration_counts_and_model_choice_are_the_references_for_every_cell(gold, be, tag):
    cells, raw = _inputs(gold, tag)
    diag = {}
    P._dsb_arrays(cells.X, raw.X[:N_EMPTY], random_state=int(gold["seed"][0]), backend=be, diagnostics=diag,
                  **CASES[tag])
    n_iter, bic, bg = gold[f"dsb_{tag}_n_iter"], gold[f"dsb_{tag}_bic"], gold[f"dsb_{tag}_bg"]
    assert n_iter.max() < 100
    assert np.array_equal(diag["n_iter"], n_iter)
    assert np.array_equal(diag["bic"][:, 0] < diag["bic"][:, 1], bic[:, 0] < bic[:, 1])
    f32 = tag == "f32_dense"
    tol = 32 * 2.0 ** -23 if f32 else 1e-12  # (relative; the fixture's float32 case ran its EM in float32)
    dev_bic = float(np.max(np.abs(diag["bic"] - bic) / np.abs(bic)))
    dev_bg = float(np.max(np.abs(diag["bgmeans"] - bg)))
    print(f"{tag}: BIC rel {dev_bic:.3g}, background mean abs {dev_bg:.3g}")
    assert dev_bic <= tol and dev_bg <= tol * max(1.0, float(np.abs(bg).max()))


def test_add_layer_writes_the_layer_and_leaves_x(gold, be):
    cells, raw = _inputs(gold)
    before = cells.X
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert prot.pp.dsb(cells, raw, add_layer=True, random_state=int(gold["seed"][0]), backend=be) is None
    assert cells.X is before
    assert np.abs(cells.layers["dsb"] - gold["dsb_int_csr"]).max() <= F64_BOUND


def test_mudata_arguments_use_their_prot_modality(gold, be):
    cells, raw = _inputs(gold)
    md, md_raw = MuData({"prot": cells}), MuData({"prot": raw})
    with pytest.warns(UserWarning, match="empty_counts_range values are not provided"):
        assert prot.pp.dsb(md, md_raw, random_state=int(gold["seed"][0]), backend=be) is None
    assert np.abs(md.mod["prot"].X - gold["dsb_int_csr"]).max() <= F64_BOUND


def _unfiltered(gold):
    prot_counts = gold["prot_counts"].astype(np.int64)
    n_all, d = prot_counts.shape
    obs_all = _names(n_all, "d")
    # an RNA matrix with the fixture's row sums (one column is enough: only the sums drive the selection)
    rna = sp.csr_matrix(gold["rna_rowsum"].astype(np.int64)[:, None])
    return MuData({"prot": _adata(sp.csr_matrix(prot_counts), obs_all, _names(d, "prot")),
                   "rna": _adata(rna, obs_all, _names(1, "g"))})


def test_unfiltered_mudata_with_count_ranges_returns_the_filtered_object(gold, be):
    md = _unfiltered(gold)
    e0, e1, c0, c1 = gold["raw_none_ranges"]
    with pytest.warns(DeprecationWarning, match="empty_counts_range will be deprecated"):
        got = prot.pp.dsb(md, empty_counts_range=(e0, e1), cell_counts_range=(c0, c1),
                          random_state=int(gold["seed"][0]), backend=be)
    assert isinstance(got, MuData) and set(got.mod) == {"prot", "rna"}
    n_all = md.mod["prot"].n_obs
    assert list(got.mod["prot"].obs_names) == list(_names(n_all - N_EMPTY, "d", N_EMPTY))
    assert got.mod["rna"].n_obs == n_all - N_EMPTY
    assert np.abs(got.mod["prot"].X - gold["dsb_int_csr"]).max() <= F64_BOUND
    assert sp.issparse(md.mod["prot"].X) and md.mod["prot"].n_obs == n_all  # the unfiltered object is left alone


def test_raw_mudata_with_rna_and_empty_range_selects_by_counts(gold, be):
    cells, _ = _inputs(gold)
    md_raw = _unfiltered(gold)
    with pytest.warns(DeprecationWarning):
        prot.pp.dsb(cells, md_raw, empty_counts_range=(0.5, 2.5), random_state=int(gold["seed"][0]), backend=be)
    assert np.abs(cells.X - gold["dsb_int_csr"]).max() <= F64_BOUND
    # a range that reaches into the cells: those droplets are dropped with a warning, the result is the same
    cells, _ = _inputs(gold)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        prot.pp.dsb(cells, md_raw, empty_counts_range=(0.5, 9.0), cell_counts_range=(3.0, 5.0),
                    random_state=int(gold["seed"][0]), backend=be)
    msgs = [str(w.message) for w in rec]
    assert any("Dropping 130 empty droplets as they are already defined as cells" in m for m in msgs)
    assert any("cell_counts_range values are ignored" in m for m in msgs)
    assert np.abs(cells.X - gold["dsb_int_csr"]).max() <= F64_BOUND
    # data_raw without an RNA modality: the range is ignored with a warning
    cells, raw = _inputs(gold)
    with pytest.warns(UserWarning, match="data_raw must be a MuData object with 'rna' modality"):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", DeprecationWarning)
            prot.pp.dsb(cells, raw, empty_counts_range=(0.5, 2.5), random_state=int(gold["seed"][0]), backend=be)
    assert np.abs(cells.X - gold["dsb_int_csr"]).max() <= F64_BOUND


def test_every_error_of_the_reference(gold, be):
    cells, raw = _inputs(gold)
    md = _unfiltered(gold)
    with pytest.raises(ValueError, match="no count ranges provided"):
        prot.pp.dsb(md, backend=be)
    with pytest.raises(ValueError, match="no count ranges provided"):
        prot.pp.dsb(md, empty_counts_range=(1, 2), backend=be)
    with pytest.raises(ValueError, match="overlapping count ranges"):
        prot.pp.dsb(md, empty_counts_range=(1, 4), cell_counts_range=(3, 5), backend=be)
    with pytest.raises(TypeError, match="data is not MuData"):
        prot.pp.dsb(cells, empty_counts_range=(1, 2), cell_counts_range=(3, 5), backend=be)
    with pytest.raises(TypeError, match="data is not MuData"):
        prot.pp.dsb(MuData({"prot": cells}), empty_counts_range=(1, 2), cell_counts_range=(3, 5), backend=be)
    short = MuData({"prot": md.mod["prot"], "rna": md.mod["rna"][np.arange(10)]})
    with pytest.raises(ValueError, match="different numbers of cells"):
        prot.pp.dsb(short, empty_counts_range=(1, 2), cell_counts_range=(3, 5), backend=be)
    with pytest.raises(TypeError, match="data_raw must be an AnnData or a MuData object with 'prot' modality"):
        prot.pp.dsb(cells, MuData({"rna": md.mod["rna"]}), backend=be)
    with pytest.raises(TypeError, match="data_raw must be an AnnData"):
        prot.pp.dsb(cells, np.zeros((3, 3)), backend=be)
    with pytest.raises(TypeError, match="data must be an AnnData or a MuData object with 'prot' modality"):
        prot.pp.dsb(MuData({"rna": md.mod["rna"]}), raw, backend=be)
    with pytest.raises(ValueError, match="pseudocount cannot be negative"):
        prot.pp.dsb(cells, raw, pseudocount=-1, backend=be)
    with pytest.raises(ValueError, match="quantile_clip must have exactly 2 values"):
        prot.pp.dsb(cells, raw, quantile_clipping=True, quantile_clip=(0.1, 0.5, 0.9), backend=be)
    with pytest.raises(ValueError, match="quantile_clip must be between 0 and 1"):
        prot.pp.dsb(cells, raw, quantile_clipping=True, quantile_clip=(-0.1, 0.9), backend=be)
    with pytest.raises(ValueError, match="different numbers of proteins"):
        prot.pp.dsb(cells, raw[:, np.arange(10)], backend=be)
    with pytest.raises(ValueError, match="cannot be used to seed"):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            prot.pp.dsb(cells, raw, random_state=np.random.default_rng(0), backend=be)
    assert sp.issparse(cells.X)  # nothing was written by the failed calls


def test_missing_isotype_controls_warn(gold, be):
    cells, raw = _inputs(gold)
    with pytest.warns(UserWarning, match="Some isotype controls are not present in the data."):
        prot.pp.dsb(cells, raw, isotype_controls=["prot5", "nope"], random_state=1, backend=be)


def test_dense_and_csr_input_give_the_same_result(gold, be):
    res = {}
    for kind in ("int_csr", "f64_dense"):
        cells, raw = _inputs(gold, kind)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            prot.pp.dsb(cells, raw, random_state=3, isotype_controls=["prot1", "prot2"], backend=be)
        res[kind] = cells.X
    assert res["int_csr"].dtype == np.float64 and np.array_equal(res["int_csr"], res["f64_dense"])


def test_pseudocount_zero_reproduces_numpys_non_finite_results(be):
    rng = np.random.default_rng(0)
    cells = rng.poisson(20.0, (12, 6)).astype(np.float64) + 1
    empty = rng.poisson(3.0, (50, 6)).astype(np.float64) + 1
    empty[4, 2] = 0.0  # log(0): that protein's mean is -inf and its std nan
    z = P._dsb_arrays(cells, empty, pseudocount=0, denoise_counts=False, backend=be).numpy()
    with np.errstate(all="ignore"):
        le = np.log(empty)
        ref = (np.log(cells) - le.mean(axis=0)) / le.std(axis=0, ddof=1)
    assert np.array_equal(np.isnan(z), np.isnan(ref)) and np.isnan(z[:, 2]).all()
    ok = ~np.isnan(ref)
    assert np.abs(z[ok] - ref[ok]).max() < 1e-12


def test_random_state_instance_advances_like_the_per_cell_loop(be):
    """A RandomState instance is consumed tied-then-full, cell after cell (scikit-learn draws n_proteins x 2 uniforms
    per fit): against a direct GaussianMixture loop on a second random case."""
    pytest.importorskip("sklearn")
    from sklearn.mixture import GaussianMixture

    rng = np.random.default_rng(5)
    d = 24
    empty = rng.poisson(3.0, (200, d)).astype(np.float64)
    cells = rng.poisson(8.0, (40, d)) + (rng.random((40, d)) < 0.3) * rng.poisson(300.0, (40, d))
    cells = cells.astype(np.float64)
    diag = {}
    P._dsb_arrays(cells, empty, random_state=np.random.RandomState(11), backend=be, diagnostics=diag)
    le = np.log(empty + 10)
    scaled = (np.log(cells + 10) - le.mean(axis=0)) / le.std(axis=0, ddof=1)
    rs = np.random.RandomState(11)
    tied = GaussianMixture(n_components=2, covariance_type="tied", init_params="random", random_state=rs)
    full = GaussianMixture(n_components=2, covariance_type="full", init_params="random", random_state=rs)
    for c in range(cells.shape[0]):
        x = scaled[c, :, np.newaxis]
        tied.fit(x)
        full.fit(x)
        bt, bf = tied.bic(x), full.bic(x)
        assert (tied.n_iter_, full.n_iter_) == tuple(diag["n_iter"][c]), c
        assert (bt < bf) == (diag["bic"][c, 0] < diag["bic"][c, 1]), c
        want = np.min(tied.means_) if bt < bf else np.min(full.means_)
        assert abs(diag["bgmeans"][c] - want) < 1e-12, c
    # and chunking the cells does not change the order of consumption
    one = P._dsb_arrays(cells, empty, random_state=np.random.RandomState(11), backend=be).numpy()
    chunks = list(P._resp_chunks(np.random.RandomState(11), 40, d))
    assert len(chunks) == 1 and chunks[0][2].shape == (40, 2, d, 2)
    assert np.array_equal(one, P._dsb_arrays(cells, empty, random_state=np.random.RandomState(11), backend=be).numpy())


def test_seeding_rules(be):
    rng = np.random.default_rng(2)
    empty = rng.poisson(3.0, (80, 10)).astype(np.float64)
    cells = (rng.poisson(8.0, (20, 10)) + (rng.random((20, 10)) < 0.3) * 200).astype(np.float64)
    a = P._dsb_arrays(cells, empty, random_state=4, backend=be).numpy()
    assert np.array_equal(a, P._dsb_arrays(cells, empty, random_state=np.int64(4), backend=be).numpy())
    assert np.isfinite(P._dsb_arrays(cells, empty, random_state=None, backend=be).numpy()).all()
    (lo, hi, u), = P._resp_chunks(4, 20, 10)
    assert (lo, hi) == (0, 20) and np.array_equal(u, np.random.RandomState(4).uniform(size=(10, 2)))


def test_mudata_subsetting_by_names_and_full_slice():
    a = AnnData(np.arange(12.0).reshape(4, 3), obs=pd.DataFrame(index=_names(4, "c")))
    b = AnnData(np.arange(8.0).reshape(4, 2), obs=pd.DataFrame(index=_names(4, "c")))
    md = MuData({"rna": a, "prot": b})
    sub = md[np.array(["c1", "c3"], dtype=object), :]
    assert list(sub.obs_names) == ["c1", "c3"] and np.array_equal(sub.mod["prot"].X, b.X[[1, 3]])
    assert np.array_equal(md[np.array(["c1", "c3"], dtype=object)].mod["rna"].X, sub.mod["rna"].X)
    with pytest.raises(NotImplementedError):
        md[np.array(["c1"], dtype=object), np.array(["var0"], dtype=object)]


# ---- clr ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", ["seurat", "stoeckius", "standard"])
@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("fmt", ["csr", "csc"])
def test_clr_sparse_input(gold, be, flavor, axis, fmt):
    x = gold["clr_x"]
    m = sp.csr_matrix(x) if fmt == "csr" else sp.csc_matrix(x)
    ad = AnnData(m.copy())
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # a CSR / CSC matrix is not converted: nothing to warn about
        assert prot.pp.clr(ad, axis=axis, flavor=flavor, backend=be) is None
    ref = gold[f"clr_sparse_{flavor}_{axis}"]
    if flavor == "seurat":
        got = ad.X
        assert sp.issparse(got) and got.format == fmt and type(got) is type(m)
        assert np.array_equal(got.indices, m.indices) and np.array_equal(got.indptr, m.indptr)  # pattern untouched
        assert np.abs(got.toarray() - ref).max() <= 1e-13
    else:
        assert isinstance(ad.X, np.ndarray)
        np.testing.assert_array_equal(np.isfinite(ad.X), np.isfinite(ref))
        np.testing.assert_array_equal(np.isnan(ad.X), np.isnan(ref))
        ok = np.isfinite(ref)
        assert not ok.any() or np.abs(ad.X[ok] - ref[ok]).max() <= 1e-13


@pytest.mark.parametrize("flavor", ["seurat", "stoeckius", "standard"])
@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("inplace", [True, False])
def test_clr_dense_input(gold, be, flavor, axis, inplace):
    x = gold["clr_x"] if flavor != "standard" else gold["clr_xp"]
    ad = AnnData(x.copy())
    with np.errstate(all="ignore"):
        ret = prot.pp.clr(ad, inplace=inplace, axis=axis, flavor=flavor, backend=be)
    ref = gold[f"clr_dense_{flavor}_{axis}"]
    if inplace:
        assert ret is None
        got = ad.X
    else:
        assert ret is not ad and np.array_equal(ad.X, x)  # the caller's object is untouched
        got = ret.X
    assert isinstance(got, np.ndarray) and got.dtype == np.float64
    np.testing.assert_array_equal(np.isposinf(got), np.isposinf(ref))
    np.testing.assert_array_equal(np.isneginf(got), np.isneginf(ref))
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    if flavor == "standard":
        assert not np.isfinite(ref).all()  # the zero of the input shows
    ok = np.isfinite(ref)
    assert np.abs(got[ok] - ref[ok]).max() <= 1e-13


def test_clr_keeps_float32_and_converts_other_sparse_formats(gold, be):
    x = gold["clr_x"]
    ad = AnnData(sp.csr_matrix(x.astype(np.float32)))
    prot.pp.clr(ad, backend=be)
    assert ad.X.dtype == np.float32 and np.abs(ad.X.toarray() - gold["clr_sparse_seurat_0"]).max() < 1e-6
    ad = AnnData(sp.coo_matrix(x))
    with pytest.warns(UserWarning, match="Converting to CSC"):
        prot.pp.clr(ad, axis=0, backend=be)
    assert ad.X.format == "csc" and np.abs(ad.X.toarray() - gold["clr_sparse_seurat_0"]).max() <= 1e-13
    ad = AnnData(sp.coo_matrix(x))
    with pytest.warns(UserWarning, match="Converting to CSR"):
        prot.pp.clr(ad, axis=1, backend=be)
    assert ad.X.format == "csr" and np.abs(ad.X.toarray() - gold["clr_sparse_seurat_1"]).max() <= 1e-13


def test_clr_errors(gold, be):
    ad = AnnData(gold["clr_x"].copy())
    with pytest.raises(ValueError, match="Invalid value for `axis` provided"):
        prot.pp.clr(ad, axis=2, backend=be)
    with pytest.raises(ValueError, match="Unknown flavor `nope`."):
        prot.pp.clr(ad, flavor="nope", backend=be)
    assert np.array_equal(ad.X, gold["clr_x"])
