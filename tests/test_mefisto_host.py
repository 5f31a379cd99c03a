"""muon.tl.mofa with smooth_covariate (MEFISTO, muon_amd/_core/mefisto.py) on the CPU operator set: the GP algebra of
the engine against the dense NumPy restatement (tests/mefisto_refs.py), the option routing against the record made by
executing the reference's own ``mofa()`` (tests/golden/make_mefisto_golden.py), write-back and error cases.

Tolerances: 1e-10 relative for single updates (fixtures hold s <= 0.99: the restatement inverts Sigma, whose condition
number is at most N / (1 - s)); 1e-12 for the plain-MOFA equivalence; 1e-9 for whole fits (the project's bar for the
general engine)."""
import functools
import json
import os

import numpy as np
import pandas as pd
import pytest
import torch

import muon_amd as mu
from muon_amd import AnnData, MuData
from muon_amd._core import tools
from muon_amd._core.mefisto import SmoothMofaEngine
from muon_amd._core.mofa_general import GeneralMofaEngine
from tests import mefisto_refs as R
from tests.cpu_backend import CpuTestBackend

BE = CpuTestBackend()
FIT = dict(n_factors=3, n_iterations=30, start_opt=5, opt_freq=5, n_grid=6)


def planted(N=60):
    """One sinusoidal and one white factor (unit variance each) on a time grid; views of 30 and 20 features."""
    rng = np.random.default_rng(2)
    t = np.linspace(0.0, 1.0, N)
    z = np.column_stack([np.sqrt(2.0) * np.sin(2 * np.pi * t), rng.standard_normal(N)])
    w1, w2 = rng.standard_normal((30, 2)), rng.standard_normal((20, 2))
    return [z @ w1.T + 0.5 * rng.standard_normal((N, 30)), z @ w2.T + 0.5 * rng.standard_normal((N, 20))], t, z


@functools.lru_cache(maxsize=None)
def full_ref():
    views, t, _ = planted()
    return R.run_smooth(views, t, **FIT)


@functools.lru_cache(maxsize=None)
def full_fit():
    views, t, _ = planted()
    eng = SmoothMofaEngine(BE, views, ["gaussian"] * 2, np.zeros(60, dtype=int), 3, t, start_opt=5, n_grid=6, opt_freq=5,
                           seed=1)
    eng.run(30, "slow")
    return eng.results(sort_factors=False)


# ---- single updates from random statistics ---------------------------------------------------------------------------
UNIT_S = (0.99, 0.5, 0.0, 0.9)      # scale per factor of the unit fixtures
UNIT_L = (3, 1, 0, 4)               # ... and its index into a grid of 6


def unit_fixture(row_constant: bool, N=40, K=4):
    rng = np.random.default_rng(9)
    t = np.sort(rng.random(N)) * 3.0
    w = rng.standard_normal((12, K))
    om = rng.random((1, 12)) + 0.5 if row_constant else rng.random((N, 12)) + 0.5
    om = np.broadcast_to(om, (N, 12))
    S = np.einsum("nd,dk,dj->nkj", om, w, w)
    a = rng.standard_normal((N, K)) * 3.0
    m0 = rng.standard_normal((N, K))
    return t, a, S, m0


def unit_engine(t, m0, eigen):
    N, K = m0.shape
    rng = np.random.default_rng(0)
    eng = SmoothMofaEngine(BE, [rng.standard_normal((N, 5))], ["gaussian"], np.zeros(N, dtype=int), K, t, n_grid=6, seed=1)
    eng.li, eng.s = list(UNIT_L), list(UNIT_S)
    eng._m64.copy_(torch.from_numpy(m0))
    eng.eigen_route = eigen
    return eng


def test_unit_fixtures_hold_scales_up_to_0_99():
    """from the restatement alone: the scales the unit tests use and the conditioning they imply"""
    assert max(UNIT_S) <= 0.99 and min(UNIT_S) >= 0.0
    t = unit_fixture(True)[0]
    ells = R.grid(t, 6)
    assert ells[0] == 0.0 and np.all(np.diff(ells) > 0) and len(ells) == 6
    d = np.sqrt(R.sq_dists(t))
    np.testing.assert_allclose([ells[1], ells[-1]], [d[d > 0].min(), d.max()], rtol=1e-15)
    for l, s in zip(UNIT_L, UNIT_S):
        ev = np.linalg.eigvalsh(R.sigma(R.sq_dists(t), ells[l], s))
        assert ev.min() >= (1.0 - s) * (1 - 1e-9) - 1e-12 and ev.max() / max(ev.min(), 1e-300) <= len(t) / (1.0 - s) * 1.01


@pytest.mark.parametrize("row_constant,eigen", [(True, True), (True, False), (False, False)])
def test_z_update_against_the_restatement(row_constant, eigen):
    t, a, S, m0 = unit_fixture(row_constant)
    eng = unit_engine(t, m0, eigen)
    np.testing.assert_allclose(eng.grid, R.grid(t, 6), rtol=1e-14)
    eng._gp_sweep(torch.from_numpy(a), torch.from_numpy(S))
    d2 = R.sq_dists(t)
    Sigs = [R.sigma(d2, eng.grid[l], s) for l, s in zip(UNIT_L, UNIT_S)]
    m, dC, Cs = R.z_update(a, S, m0, Sigs)
    np.testing.assert_allclose(eng.EZ.numpy(), m, rtol=1e-10, atol=1e-10 * np.abs(m).max())
    np.testing.assert_allclose(eng.EZ2.numpy(), m * m + dC, rtol=1e-10, atol=1e-10)
    eng._gp_now = True
    got = float(eng._factor_terms(torch.zeros((), dtype=torch.float64)))
    want = sum(R.z_term(Sigs[k], Cs[k], m[:, k]) for k in range(m.shape[1]))
    assert abs(got - want) <= 1e-10 * abs(want)


def test_eigen_route_equals_general_route_at_a_constant_diagonal():
    t, a, S, m0 = unit_fixture(True)
    out = []
    for eigen in (True, False):
        eng = unit_engine(t, m0, eigen)
        eng._gp_sweep(torch.from_numpy(a), torch.from_numpy(S))
        out.append((eng.EZ.numpy().copy(), eng.EZ2.numpy().copy(), eng._quad.numpy().copy(), eng._ldS.numpy().copy(),
                    eng._ldC.numpy().copy(), torch.stack([eng._grid_q(k) for k in range(4)]).numpy()))
    for x, y in zip(*out):
        np.testing.assert_allclose(x, y, rtol=1e-10, atol=1e-10 * np.abs(y).max())


@pytest.mark.parametrize("row_constant,eigen", [(True, True), (False, False)])
def test_hyperparameter_objective_through_q_equals_trace_and_logdet(row_constant, eigen):
    t, a, S, m0 = unit_fixture(row_constant)
    eng = unit_engine(t, m0, eigen)
    eng._gp_sweep(torch.from_numpy(a), torch.from_numpy(S))
    d2 = R.sq_dists(t)
    Sigs = [R.sigma(d2, eng.grid[l], s) for l, s in zip(UNIT_L, UNIT_S)]
    m, _, Cs = R.z_update(a, S, m0, Sigs)
    e = eng._e.numpy()
    for k in range(4):
        q = eng._grid_q(k).numpy()
        E = Cs[k] + np.outer(m[:, k], m[:, k])
        for l, ell in enumerate(eng.grid):
            for s in (0.0, 0.3, 0.99):
                lam = s * e[l] + (1.0 - s)
                got = -0.5 * np.sum(np.log(lam) + q[l] / lam)
                want = R.hyper_F(R.sigma(d2, ell, s), E)
                assert abs(got - want) <= 1e-10 * abs(want), (k, l, s)


def test_best_scale_is_on_the_2_pow_minus_20_lattice_and_no_worse_than_zero():
    from muon_amd._core.mefisto import S_MAX, best_scale

    rng = np.random.default_rng(3)
    e = np.sort(rng.random(30)) * 5
    for q in (e * 0.9 + 0.05, np.ones(30), rng.random(30)):
        s, F = best_scale(e, q)
        assert 0.0 <= s <= S_MAX and s * 2 ** 20 == round(s * 2 ** 20)
        assert F >= -0.5 * q.sum() - 1e-12


# ---- whole fits ------------------------------------------------------------------------------------------------------
def test_before_start_opt_the_fit_is_plain_mofa_with_alpha_z_one():
    views, t, _ = planted()
    g = np.zeros(60, dtype=int)
    eng = SmoothMofaEngine(BE, views, ["gaussian"] * 2, g, 3, t, start_opt=1000, n_grid=3, seed=1)
    plain = GeneralMofaEngine(BE, views, ["gaussian"] * 2, g, 3, ard_factors=False, seed=1)
    for e in (eng, plain):
        e.run(12, "slow")
        assert torch.all(e.alpha_z == 1.0)  # (the hook: without an ARD node on the factors alpha_z stays at 1)
    np.testing.assert_allclose(eng.elbo, plain.elbo, rtol=1e-12)
    np.testing.assert_allclose(eng.EZ.numpy(), plain.EZ.numpy(), rtol=1e-12, atol=1e-12)
    assert eng.s == [0.0] * 3


def test_full_fit_against_the_restatement():
    ref, res = full_ref(), full_fit()
    assert len(res["elbo"]) == len(ref["elbo"]) == 30
    np.testing.assert_allclose(res["elbo"], ref["elbo"], rtol=1e-9)
    np.testing.assert_allclose(res["Z"], ref["Z"], rtol=1e-9, atol=1e-9)
    np.testing.assert_array_equal(res["smooth"]["scale"], ref["scale"])
    np.testing.assert_allclose(res["smooth"]["lengthscale"], ref["lengthscale"], rtol=1e-14)
    assert ref["scale"].max() > 0  # (the GP prior was in use)


def test_elbo_never_falls_hyperparameter_steps_included():
    for trace in (full_fit()["elbo"], full_ref()["elbo"]):
        assert np.all(np.diff(trace) >= -1e-9 * abs(trace[0]))


def test_the_sinusoidal_factor_learns_the_larger_scale():
    _, _, z = planted()
    res = full_fit()
    corr = np.abs(np.corrcoef(np.column_stack([z, res["Z"]]).T)[:2, 2:])
    k_sin, k_white = int(np.argmax(corr[0])), int(np.argmax(corr[1]))
    assert k_sin != k_white
    assert res["smooth"]["scale"][k_sin] > res["smooth"]["scale"][k_white]


# ---- the wrapper -----------------------------------------------------------------------------------------------------
def _mdata(groups=False):
    views, t, _ = planted()
    names = [f"cell{i:02d}" for i in range(60)]
    obs = pd.DataFrame(index=names)
    md = MuData({"a": AnnData(views[0], obs=obs.copy()), "b": AnnData(views[1], obs=obs.copy())})
    md.obs["time"] = t
    md.obs["label"] = ["x"] * 60
    md.obs["bad"] = [np.nan] + [1.0] * 59
    if groups:
        md.obs["grp"] = np.where(np.arange(60) % 3 == 0, "g1", "g0")
    return md, views, t


def _match_columns(got, want):
    """the permutation p with got[:, i] = want[:, p[i]]"""
    p = [int(np.argmin([np.abs(got[:, i] - want[:, j]).max() for j in range(want.shape[1])])) for i in range(got.shape[1])]
    assert sorted(p) == list(range(want.shape[1]))
    return p


def test_wrapper_write_back_prediction_and_model_file(tmp_path):
    md, views, t = _mdata()
    new = [0.1, 0.45, 1.2]
    mu.tl.mofa(md, n_factors=3, n_iterations=30, convergence_mode="slow", smooth_covariate="time", quiet=True, backend=BE,
               smooth_kwargs=dict(start_opt=5, opt_freq=5, n_grid=6, new_values=new), outfile=str(tmp_path / "m.hdf5"))
    ref = full_ref()
    X = md.obsm["X_mofa"]
    assert X.shape == (60, 3) and md.varm["LFs"].shape == (50, 3)
    p = _match_columns(X, ref["Z"])
    np.testing.assert_allclose(X, ref["Z"][:, p], rtol=1e-9, atol=1e-9)
    sm = md.uns["mofa"]["smooth"]
    assert set(sm) == {"covariates_names", "lengthscale", "scale", "grid", "new_values", "Z_predicted"}
    assert sm["covariates_names"] == ["time"]
    np.testing.assert_array_equal(sm["scale"], ref["scale"][p])
    np.testing.assert_allclose(sm["lengthscale"], ref["lengthscale"][p], rtol=1e-14)
    np.testing.assert_allclose(sm["grid"], ref["grid"], rtol=1e-14)
    assert sm["new_values"].shape == (3, 1) and sm["Z_predicted"].shape == (3, 3)
    want = np.column_stack([R.predict(t, np.asarray(new), ref["lengthscale"][k], ref["scale"][k], ref["Z"][:, k]) for k in p])
    np.testing.assert_allclose(sm["Z_predicted"], want, rtol=1e-9, atol=1e-9)
    assert np.abs(want).max() > 0.1
    np.testing.assert_allclose(md.uns["mofa"]["elbo"], ref["elbo"], rtol=1e-9)
    z = np.load(md.uns["mofa"]["model_file"])
    np.testing.assert_array_equal(z["training_stats/length_scales"], sm["lengthscale"])
    np.testing.assert_array_equal(z["training_stats/scales"], sm["scale"])
    np.testing.assert_array_equal(z["covariates/group1"], t[:, None])
    np.testing.assert_allclose(z["expectations/Z/group1"], X.T)


def test_wrapper_two_groups_one_covariance_matches_the_restatement():
    md, views, t = _mdata(groups=True)
    with pytest.raises(NotImplementedError, match="model_groups"):
        mu.tl.mofa(md, groups_label="grp", n_factors=3, smooth_covariate="time", quiet=True, backend=BE)
    mu.tl.mofa(md, groups_label="grp", n_factors=3, n_iterations=12, convergence_mode="slow", smooth_covariate="time",
               quiet=True, backend=BE, smooth_kwargs=dict(start_opt=5, opt_freq=5, n_grid=6, model_groups=False))
    codes = (np.arange(60) % 3 == 0).astype(int)  # ("g1" appears first: group 0 of the model)
    codes = 1 - codes
    ref = R.run_smooth(views, t, groups=codes, n_factors=3, n_iterations=12, start_opt=5, opt_freq=5, n_grid=6)
    X = md.obsm["X_mofa"]
    p = _match_columns(X, ref["Z"])
    np.testing.assert_allclose(X, ref["Z"][:, p], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(md.uns["mofa"]["elbo"], ref["elbo"], rtol=1e-9)
    np.testing.assert_array_equal(md.uns["mofa"]["smooth"]["scale"], ref["scale"][p])
    assert "new_values" not in md.uns["mofa"]["smooth"]


def test_scale_cov_z_scores_the_covariates_and_the_new_values():
    md, views, t = _mdata()
    md.obs["depth"] = np.random.default_rng(4).random(60) * 7 + 3
    kw = dict(n_factors=2, n_iterations=8, convergence_mode="slow", quiet=True, backend=BE)
    mu.tl.mofa(md, smooth_covariate=["time", "depth"], **kw,
               smooth_kwargs=dict(scale_cov=True, start_opt=3, opt_freq=2, n_grid=4, covariates_names=["t", "d"],
                                  new_values=[[0.5, 5.0], [0.7, 6.0]]))
    sm = md.uns["mofa"]["smooth"]
    cov = np.column_stack([t, md.obs["depth"].values])
    zc = (cov - cov.mean(axis=0)) / cov.std(axis=0)
    ref = R.run_smooth(views, zc, n_factors=2, n_iterations=8, start_opt=3, opt_freq=2, n_grid=4)
    p = _match_columns(md.obsm["X_mofa"], ref["Z"])
    np.testing.assert_allclose(md.obsm["X_mofa"], ref["Z"][:, p], rtol=1e-9, atol=1e-9)
    assert sm["covariates_names"] == ["t", "d"] and sm["new_values"].shape == (2, 2)
    new = (np.array([[0.5, 5.0], [0.7, 6.0]]) - cov.mean(axis=0)) / cov.std(axis=0)
    want = np.column_stack([R.predict(zc, new, ref["lengthscale"][k], ref["scale"][k], ref["Z"][:, k]) for k in p])
    np.testing.assert_allclose(sm["Z_predicted"], want, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("kw,err,word", [
    (dict(smooth_warping=True), NotImplementedError, "smooth_warping"),
    (dict(smooth_kwargs={"sparseGP": True}), NotImplementedError, "sparseGP"),
    (dict(smooth_kwargs={"frac_inducing": 0.2}), NotImplementedError, "frac_inducing"),
    (dict(spikeslab_factors=True), ValueError, "spikeslab_factors"),
    (dict(smooth_covariate="nope"), KeyError, "nope"),
    (dict(smooth_covariate="label"), ValueError, "numeric"),
    (dict(smooth_covariate="bad"), ValueError, "NaN"),
    (dict(smooth_covariate=["time", "nope"]), KeyError, "nope"),
])
def test_error_cases(kw, err, word):
    md, _, _ = _mdata()
    kw = {"smooth_covariate": "time", **kw}
    with pytest.raises(err, match=word):
        mu.tl.mofa(md, n_factors=2, n_iterations=3, quiet=True, backend=BE, **kw)
    assert "X_mofa" not in md.obsm


def test_more_than_one_rank_is_refused():
    class TwoRanks:
        world_size, rank = 2, 0

    with pytest.raises(NotImplementedError, match="runs on one rank"):
        tools._check_smooth_options(tools._smooth_options("time", False, None) | {"model_groups": False}, 1, False, TwoRanks())


def test_memory_need_is_stated_when_it_does_not_fit():
    class Small(CpuTestBackend):
        def free_memory(self):
            return 1000

    views, t, _ = planted()
    with pytest.raises(ValueError, match=str(6 * 60 * 60 * 8)):
        SmoothMofaEngine(Small(), views, ["gaussian"] * 2, np.zeros(60, dtype=int), 3, t, n_grid=6)


def test_smooth_options_without_a_covariate_are_ignored_like_the_reference(caplog):
    md, views, _ = _mdata()
    kw = dict(n_factors=3, n_iterations=6, convergence_mode="slow", quiet=True, backend=BE)
    mu.tl.mofa(md, smooth_warping=True, smooth_kwargs={"sparseGP": True, "n_grid": 3}, **kw)
    md2, _, _ = _mdata()
    mu.tl.mofa(md2, **kw)
    np.testing.assert_array_equal(md.obsm["X_mofa"], md2.obsm["X_mofa"])
    assert "smooth" not in md.uns["mofa"]
    with pytest.raises(NotImplementedError, match="svi_mode"):
        mu.tl.mofa(md, svi_mode=True, smooth_covariate="time", **kw)


def test_ard_factors_is_ignored_with_one_log_line(caplog):
    import logging

    md, _, _ = _mdata()
    with caplog.at_level(logging.INFO, logger="muon_amd"):
        mu.tl.mofa(md, n_factors=2, n_iterations=3, smooth_covariate="time", quiet=True, backend=BE,
                   smooth_kwargs=dict(start_opt=1, opt_freq=1, n_grid=3))
    assert sum("ard_factors is ignored" in r.getMessage() for r in caplog.records) == 1


# ---- the option routing against the reference, executed (tests/golden/make_mefisto_golden.py) -------------------------
@pytest.mark.parametrize("tag", ["defaults", "list_scaled", "new_values_1d"])
def test_merged_options_equal_what_the_reference_hands_to_mofapy2(golden_dir, tag):
    with np.load(os.path.join(golden_dir, "mefisto_options_golden.npz")) as f:
        rec = json.loads(str(f["record"]))[tag]
    kw = rec["keywords"]
    opts = tools._smooth_options(kw["smooth_covariate"], kw.get("smooth_warping", False), kw.get("smooth_kwargs"))
    assert rec["set_covariates"]["args"] == [kw["smooth_covariate"]]
    assert opts["covariates_names"] == rec["set_covariates"]["kwargs"]["covariates_names"]
    want = rec["set_smooth_options"]
    assert len(want) == 12
    for k, v in want.items():
        assert opts[k] == v, k
    assert set(opts) == set(want) | {"covariates_names", "new_values"}
    nv = tools._smooth_new_values(opts)
    if rec["predict_factor"] is None:
        assert nv is None
    else:
        np.testing.assert_array_equal(nv, np.asarray(rec["predict_factor"]["new_covariates"], dtype=np.float64))
    # the options the fit reads are the recorded ones (the defaults of the reference, not ours)
    assert (opts["start_opt"], opts["opt_freq"], opts["model_groups"]) == (want["start_opt"], want["opt_freq"], want["model_groups"])
