"""muon_amd.pp.harmony_integrate on the CPU operator set (tests/cpu_backend.py has no harmony kernels: the tensor
formulation runs) against the NumPy restatement of the package's statement (tests/harmony_refs.py), and the host logic
around it: keys and levels, per-key and per-cluster arguments, dtypes, write-back, ``return_info`` and every error.
Parity with harmonypy is not pinned (it is not installed here); the restatement is the reference.

End to end, per case: ``kmeans_rounds`` and ``n_iter`` equal the f64 restatement's; the corrected embedding lies within
100 times the restatement's own f64-versus-longdouble deviation (computed here, printed as MEASURE); the same-batch
share among the 15 nearest neighbours falls from 1.00 to under the case's cap (chance: 0.50 / 0.34 / 0.50).

The argument checks of the C-ABI entries of csrc/harmony.hip run here too: they come before any HIP call."""
import ctypes

import numpy as np
import pandas as pd
import pytest

from tests import harmony_refs as hr
from tests.cpu_backend import CpuTestBackend
from muon_amd import AnnData, MuData, pp
from muon_amd._core import harmony as H


@pytest.fixture(scope="module")
def be():
    return CpuTestBackend()


def _adata(Z, **obs):
    return AnnData(np.zeros((Z.shape[0], 1)), obs=pd.DataFrame({k: np.asarray(v) for k, v in obs.items()}),
                   obsm={"X_pca": Z})


@pytest.mark.parametrize("name", sorted(hr.CASES))
def test_end_to_end_against_the_restatement(be, name):
    Z, codes, _, _ = hr.case(name)
    res = H._harmonize(be, Z, [codes], [hr.CASES[name][3]], nclust=hr.CASES[name][4])
    assert res["route"] == "tensor"
    hr.check_case(name, res, "cpu")


def test_public_function_writes_back_and_reports(be):
    Z, codes, ref, own = hr.case("n300")
    ad = _adata(Z.copy(), batch=np.array(["b", "a"])[codes])  # levels in category order: "a" < "b" swaps the codes
    info = pp.harmony_integrate(ad, "batch", nclust=10, return_info=True, backend=be)
    assert sorted(info) == ["converged", "kmeans_rounds", "n_iter", "nclust", "objective_harmony"]
    assert info["kmeans_rounds"] == ref["kmeans_rounds"] and info["n_iter"] == ref["n_iter"] and info["nclust"] == 10
    assert len(info["objective_harmony"]) == info["n_iter"] + 1 and info["converged"] is True
    out = ad.obsm["X_pca_harmony"]
    assert out.dtype == np.float64 and out.shape == Z.shape and np.array_equal(ad.obsm["X_pca"], Z)
    # theta and lamb are the same for both levels, so naming the levels the other way round changes nothing but the
    # order of the K x B sums
    assert hr.deviation(out, ref["Z_corr"]) <= 100 * own
    ad2 = _adata(Z.copy(), batch=codes)
    assert pp.harmony_integrate(ad2, "batch", nclust=10, basis="X_pca", adjusted_basis="X_h", backend=be) is None
    assert hr.deviation(ad2.obsm["X_h"], ref["Z_corr"]) <= 100 * own and "X_pca_harmony" not in ad2.obsm


def test_mudata_and_knn_on_the_result(be):
    Z, codes, ref, own = hr.case("n300")
    md = MuData({"rna": AnnData(np.zeros((300, 2))), "atac": AnnData(np.zeros((300, 3)))})
    md.obs["lane"] = codes
    md.obsm["X_mofa"] = Z.copy()
    assert pp.harmony_integrate(md, "lane", basis="X_mofa", adjusted_basis="X_mofa_harmony", nclust=10, backend=be) is None
    assert hr.deviation(md.obsm["X_mofa_harmony"], ref["Z_corr"]) <= 100 * own
    ad = _adata(Z.copy(), batch=codes)
    pp.harmony_integrate(ad, "batch", nclust=10, backend=be)
    pp.knn(ad, n_neighbors=15, use_rep="X_pca_harmony", backend=be)
    assert ad.obsp["distances"].shape == (300, 300) and ad.obsp["connectivities"].nnz > 0


def _two_keys():
    Z, _, batch = hr.planted(600, 8, 3, 2)
    donor = np.random.default_rng(5).integers(3, size=600)
    Z = Z + np.random.default_rng(6).normal(size=(3, 8))[donor]
    return Z, batch, donor


def test_two_keys_equal_the_dense_phi_restatement(be):
    """several keys: Phi has one 1 per key and row, the regression's matrix is no arrow matrix any more"""
    Z, batch, donor = _two_keys()
    kw = dict(sigma=0.1, nclust=12, max_iter_harmony=3)
    ref = hr.harmony_ref(Z, hr.one_hot([batch, donor], [2, 3]), theta=2.0, lamb=1.0, **kw)
    ext = hr.harmony_ref(Z, hr.one_hot([batch, donor], [2, 3]), theta=2.0, lamb=1.0, dtype=np.longdouble, **kw)
    ad = _adata(Z.copy(), batch=batch, donor=donor)
    info = pp.harmony_integrate(ad, ["batch", "donor"], return_info=True, backend=be, **kw)
    dev, own = hr.deviation(ad.obsm["X_pca_harmony"], ref["Z_corr"]), hr.deviation(ext["Z_corr"], ref["Z_corr"])
    print(f"MEASURE harmony cpu two keys: rounds {info['kmeans_rounds']} deviation {dev:.3g} (restatement {own:.3g})")
    assert info["kmeans_rounds"] == ref["kmeans_rounds"] == ext["kmeans_rounds"] and info["n_iter"] == ref["n_iter"]
    assert dev <= 100 * own


def test_per_key_theta_lamb_tau_and_a_sigma_vector(be):
    """theta=[..], lamb=[..]: one value per key, repeated over its levels; tau scales theta by the level's size; sigma
    one value per cluster"""
    Z, batch, donor = _two_keys()
    sig = np.linspace(0.08, 0.15, 12)
    kw = dict(sigma=sig, nclust=12, tau=5, max_iter_harmony=2)
    ref = hr.harmony_ref(Z, hr.one_hot([batch, donor], [2, 3]), theta=np.repeat([1.5, 3.0], [2, 3]),
                         lamb=np.repeat([0.5, 2.0], [2, 3]), **kw)
    res = H._harmonize(be, Z, [batch, donor], [2, 3], theta=[1.5, 3.0], lamb=[0.5, 2.0], **kw)
    assert res["kmeans_rounds"] == ref["kmeans_rounds"] and hr.deviation(res["Z_corr"], ref["Z_corr"]) < 1e-10
    for bad in (dict(theta=[1.0]), dict(lamb=[1.0, 2.0, 3.0])):
        with pytest.raises(ValueError, match=next(iter(bad))):
            H._harmonize(be, Z, [batch, donor], [2, 3], nclust=12, **bad)
    with pytest.raises(ValueError, match="sigma"):
        H._harmonize(be, Z, [batch, donor], [2, 3], nclust=12, sigma=[0.1, 0.2])


def test_theta_zero_leaves_a_plain_soft_kmeans(be):
    """theta = 0: F = 1, so R is the row-normalised S of the last round's centres"""
    Z, codes, _, _ = hr.case("n300")
    res = H._harmonize(be, Z, [codes], [2], theta=0.0, nclust=10, max_iter_harmony=1)
    Zc = Z / np.sqrt((Z * Z).sum(1, keepdims=True))
    T = -(2 * (1 - Zc @ res["Y"].T)) / 0.1
    S = np.exp(T - T.max(1, keepdims=True))
    assert np.abs(res["R"] - S / S.sum(1, keepdims=True)).max() <= 26 * 2.0 ** -52  # (K + 16) 2^-52, K = 10


def test_float32_basis_is_widened_exactly_and_rounded_once(be):
    Z, codes, _, _ = hr.case("n300")
    Z32 = Z.astype(np.float32)
    a64, a32 = _adata(Z32.astype(np.float64), batch=codes), _adata(Z32.copy(), batch=codes)
    pp.harmony_integrate(a64, "batch", nclust=10, backend=be)
    pp.harmony_integrate(a32, "batch", nclust=10, backend=be)
    out = a32.obsm["X_pca_harmony"]
    assert out.dtype == np.float32 and a32.obsm["X_pca"].dtype == np.float32
    want = a64.obsm["X_pca_harmony"]
    assert np.abs(out - want).max() <= 2.0 ** -23 * np.abs(want).max()


def test_errors_name_the_argument(be):
    Z, codes, _, _ = hr.case("n300")
    ad = _adata(Z.copy(), batch=codes)
    with pytest.raises(KeyError, match="donor"):
        pp.harmony_integrate(ad, ["batch", "donor"], backend=be)
    with pytest.raises(KeyError, match="X_lsi"):
        pp.harmony_integrate(ad, "batch", basis="X_lsi", backend=be)
    small = _adata(Z[:29].copy(), batch=codes[:29])
    with pytest.raises(ValueError, match="nclust"):
        pp.harmony_integrate(small, "batch", backend=be)
    pp.harmony_integrate(small, "batch", nclust=3, max_iter_harmony=1, backend=be)  # (with nclust it runs)
    for bad in (0, -1, 301):
        with pytest.raises(ValueError, match="nclust"):
            pp.harmony_integrate(ad, "batch", nclust=bad, backend=be)
    for bad in (0, -0.1, 1.5):
        with pytest.raises(ValueError, match="block_size"):
            pp.harmony_integrate(ad, "batch", nclust=10, block_size=bad, backend=be)
    for value in (0.0, np.nan, np.inf):
        Zb = Z.copy()
        Zb[7] = value
        with pytest.raises(ValueError, match="basis"):
            pp.harmony_integrate(_adata(Zb, batch=codes), "batch", nclust=10, backend=be)
    assert "X_pca_harmony" not in ad.obsm


# ---- the C-ABI's argument checks (before any HIP call: they need no device) --------------------------------------------
def test_c_abi_refuses_bad_arguments_by_name():
    from muon_amd import _ffi

    lib = _ffi.lib()
    assert (lib.mu_harmony_max_clusters(), lib.mu_harmony_max_dims(), lib.mu_harmony_max_levels()) == (128, 64, 64)
    assert lib.mu_version() >= 816
    p = ctypes.c_void_p(4096)  # (never dereferenced: every call below is refused first)
    seg = (ctypes.c_int64 * 3)(0, 5, 10)

    def gram(n=10, m=10, K=4, d=3, R=p, ldr=16, Z=p, ldz=3, idx=None, n_seg=2, seg=seg, out=p, work=p, wb=1 << 30):
        return lib.mu_harmony_gram_f64(n, m, K, d, R, ldr, Z, ldz, idx, n_seg, seg, out, work, wb, None)

    def assign(n=10, K=4, d=3, B=2, nb=10, Zc=p, ldz=3, Y=p, sigma=p, F=p, codes=p, idx=None, R=p, ldr=16):
        return lib.mu_harmony_assign_f64(n, K, d, B, nb, Zc, ldz, Y, sigma, F, codes, idx, R, ldr, None)

    def objective(n=10, K=4, d=3, B=2, Zc=p, ldz=3, Y=p, R=p, ldr=16, sigma=p, G=p, codes=p, out=p, work=p, wb=1 << 20):
        return lib.mu_harmony_objective_f64(n, K, d, B, Zc, ldz, Y, R, ldr, sigma, G, codes, out, work, wb, None)

    def correct(n=10, K=4, d=3, B=2, Z=p, ldz=3, R=p, ldr=16, W=p, seg=seg, Zcorr=p, Zc=p, ldo=3):
        return lib.mu_harmony_correct_f64(n, K, d, B, Z, ldz, R, ldr, W, seg, Zcorr, Zc, ldo, None)

    desc = (ctypes.c_int64 * 3)(0, 7, 5)
    short = (ctypes.c_int64 * 3)(0, 5, 9)
    past = (ctypes.c_int64 * 3)(0, 5, 11)
    for name, call, bad in (
            ("mu_harmony_gram_f64", gram, [dict(R=None), dict(Z=None), dict(out=None), dict(seg=None), dict(work=None),
                                           dict(n=-1), dict(m=-1), dict(K=0), dict(K=129), dict(d=0), dict(d=65),
                                           dict(n_seg=0), dict(n_seg=65), dict(seg=desc), dict(seg=past), dict(ldr=3),
                                           dict(ldz=2), dict(m=11), dict(wb=8)]),
            ("mu_harmony_objective_f64", objective, [dict(Zc=None), dict(Y=None), dict(R=None), dict(sigma=None),
                                                     dict(G=None), dict(codes=None), dict(out=None), dict(work=None),
                                                     dict(n=-1), dict(K=0), dict(K=129), dict(d=65), dict(B=0),
                                                     dict(B=65), dict(ldr=3), dict(ldz=2), dict(wb=8)]),
            ("mu_harmony_correct_f64", correct, [dict(Z=None), dict(R=None), dict(W=None), dict(seg=None),
                                                 dict(Zcorr=None), dict(Zc=None), dict(n=-1), dict(K=129), dict(d=65),
                                                 dict(B=0), dict(B=65), dict(seg=desc), dict(seg=short), dict(seg=past),
                                                 dict(ldr=3), dict(ldz=2), dict(ldo=2)]),
            ("mu_harmony_assign_f64", assign, [dict(Zc=None), dict(Y=None), dict(sigma=None), dict(F=None),
                                               dict(codes=None), dict(R=None), dict(n=-1), dict(nb=-1), dict(K=0),
                                               dict(K=129), dict(d=65), dict(B=0), dict(B=65), dict(ldr=15), dict(ldz=2),
                                               dict(nb=11)])):
        for kw in bad:
            assert call(**kw) == -1, (name, kw)
            assert name.encode() in lib.mu_last_error(), (name, kw, lib.mu_last_error())
    assert lib.mu_harmony_gram_worksize(10, 2, 4, 3) == 2 * 1 * 16 * 16 * 8
    assert lib.mu_harmony_gram_worksize(10 ** 6, 4, 100, 50) == 4 * 128 * 112 * 64 * 8
    assert lib.mu_harmony_objective_worksize(10 ** 6) == 512 * 3 * 8 and lib.mu_harmony_objective_worksize(65) == 2 * 3 * 8
    assert lib.mu_harmony_gram_worksize(10, 65, 4, 3) == 0 and lib.mu_harmony_gram_worksize(10, 1, 129, 3) == 0


def test_65_levels_of_one_key(be):
    """one level more than the kernels take: the tensor route, whatever the backend"""
    Z, codes, ref, own = hr.levels65()
    res = H._harmonize(be, Z, [codes], [65], nclust=8, max_iter_harmony=2)
    assert res["route"] == "tensor" and res["kmeans_rounds"] == ref["kmeans_rounds"]
    assert hr.deviation(res["Z_corr"], ref["Z_corr"]) <= 100 * own
