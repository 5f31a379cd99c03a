"""MEFISTO on the GPU: the two kernels of csrc/gp.hip against the tensor route at the lane / unroll / panel edges, a whole
fit through the public wrapper against the NumPy restatement (tests/mefisto_refs.py), and which route calls the kernels.

Kernel bound: two differently ordered sums of the same N terms (each term up to two products) differ by at most
(2 N + 4) 2^-53 sum |term_i| - the forward-error bound of recursive summation, applied to both sides; nothing measured.
Fit tolerance: 1e-9 on the ELBO trace and <Z>, the bar of the general engine."""
import numpy as np
import pytest
import torch

import muon_amd as mu
from muon_amd._core.mefisto import SmoothMofaEngine
from tests import mefisto_refs as R
from tests.test_mefisto_host import FIT, _match_columns, _mdata, full_ref, planted

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1025])
def test_kernels_against_the_tensor_route(hip, n):
    g = torch.Generator().manual_seed(n)
    V = torch.randn((n, n), dtype=torch.float64, generator=g).to(hip.device)
    r, gg, u = (torch.randn((n,), dtype=torch.float64, generator=g).to(hip.device) for _ in range(3))
    gg = gg.abs()
    got_u = hip.gp_project(V, r)
    got_m, got_dc = hip.gp_posterior(V, gg, u)
    torch.cuda.synchronize()
    bound = (2 * n + 4) * U
    for name, got, want, mag in (("project", got_u, V.T @ r, V.abs().T @ r.abs()),
                                 ("posterior mean", got_m, V @ (gg * u), V.abs() @ (gg * u).abs()),
                                 ("posterior variance", got_dc, (V * V) @ gg, (V * V) @ gg)):
        diff = (got - want).abs()
        print(name, n, "max |diff| / bound", float((diff / (bound * mag).clamp(min=1e-300)).max()))
        assert torch.all(diff <= bound * mag), name
    again_u = hip.gp_project(V, r)
    again_m, again_dc = hip.gp_posterior(V, gg, u)
    assert torch.equal(again_u, got_u) and torch.equal(again_m, got_m) and torch.equal(again_dc, got_dc)


def test_kernels_take_a_slice_of_a_stack(hip):
    """the engine hands the kernels V_l = stack[l]: a contiguous n x n slice at an offset"""
    n = 130
    g = torch.Generator().manual_seed(5)
    stack = torch.randn((3, n, n), dtype=torch.float64, generator=g).to(hip.device)
    r = torch.randn((n,), dtype=torch.float64, generator=g).to(hip.device)
    assert torch.equal(hip.gp_project(stack[1], r), hip.gp_project(stack[1].clone(), r))
    wide = torch.randn((n, n + 7), dtype=torch.float64, generator=g).to(hip.device)
    a, b = hip.gp_posterior(wide[:, :n], r.abs(), r)  # (a row stride larger than n)
    c, d = hip.gp_posterior(wide[:, :n].contiguous(), r.abs(), r)
    assert torch.equal(a, c) and torch.equal(b, d)


class _Spy:
    """Forwards to a backend and counts the calls of the two kernels."""

    def __init__(self, be):
        self._be, self.calls = be, {"gp_project": 0, "gp_posterior": 0}

    def __getattr__(self, name):
        got = getattr(self._be, name)
        if name in self.calls:
            def counted(*a, **k):
                self.calls[name] += 1
                return got(*a, **k)

            return counted
        return got


def test_full_fit_through_the_wrapper_against_the_restatement(hip):
    md, views, t = _mdata()
    spy = _Spy(hip)
    mu.tl.mofa(md, n_factors=3, n_iterations=30, convergence_mode="slow", smooth_covariate="time", quiet=True, backend=spy,
               smooth_kwargs=dict(start_opt=5, opt_freq=5, n_grid=6, new_values=[0.1, 0.45, 1.2]))
    ref = full_ref()
    X = md.obsm["X_mofa"]
    p = _match_columns(X, ref["Z"])
    elbo = np.asarray(md.uns["mofa"]["elbo"])
    print("ELBO: max relative difference", np.abs(elbo / np.asarray(ref["elbo"]) - 1).max(),
          " <Z>: max difference", np.abs(X - ref["Z"][:, p]).max())
    np.testing.assert_allclose(elbo, ref["elbo"], rtol=1e-9)
    np.testing.assert_allclose(X, ref["Z"][:, p], rtol=1e-9, atol=1e-9)
    sm = md.uns["mofa"]["smooth"]
    np.testing.assert_array_equal(sm["scale"], ref["scale"][p])
    want = np.column_stack([R.predict(t, np.asarray([0.1, 0.45, 1.2]), ref["lengthscale"][k], ref["scale"][k], ref["Z"][:, k])
                            for k in p])
    np.testing.assert_allclose(sm["Z_predicted"], want, rtol=1e-9, atol=1e-9)
    # the eigen route ran on the kernels: a pair of calls per factor and iteration under the GP prior (one with a
    # hyperparameter step, or after one that left some s_k > 0)
    trace = ref["hyper_trace"]
    gp = sum(1 for it in range(30) if (it >= 5 and (it - 5) % 5 == 0) or (it > 0 and max(trace[it - 1][1]) > 0))
    assert gp >= 20 and spy.calls == {"gp_project": 3 * gp, "gp_posterior": 3 * gp}


def test_masked_fit_takes_the_general_route_without_the_kernels(hip):
    views, t, _ = planted()
    views = [views[0].copy(), views[1]]
    views[0][3, 4] = np.nan
    views[0][20:24, 7] = np.nan
    spy = _Spy(hip)
    eng = SmoothMofaEngine(spy, views, ["gaussian"] * 2, np.zeros(60, dtype=int), 3, t, start_opt=5, n_grid=6, opt_freq=5,
                           seed=1)
    assert not eng.eigen_route
    eng.run(12, "slow")
    ref = R.run_smooth(views, t, **{**FIT, "n_iterations": 12})
    res = eng.results(sort_factors=False)
    np.testing.assert_allclose(res["elbo"], ref["elbo"], rtol=1e-9)
    np.testing.assert_allclose(res["Z"], ref["Z"], rtol=1e-9, atol=1e-9)
    assert spy.calls == {"gp_project": 0, "gp_posterior": 0}


def test_operator_set_without_the_kernels_takes_the_tensor_route(hip):
    class NoKernels(_Spy):
        def __getattr__(self, name):
            if name in ("gp_project", "gp_posterior"):
                raise AttributeError(name)
            return super().__getattr__(name)

    views, t, _ = planted()
    out = []
    for be in (hip, NoKernels(hip)):
        eng = SmoothMofaEngine(be, views, ["gaussian"] * 2, np.zeros(60, dtype=int), 3, t, start_opt=2, n_grid=4, opt_freq=3,
                               seed=1)
        assert eng.eigen_route and eng._kernels == (be is hip)
        eng.run(8, "slow")
        out.append(eng.results(sort_factors=False))
    np.testing.assert_allclose(out[0]["elbo"], out[1]["elbo"], rtol=1e-9)
    np.testing.assert_allclose(out[0]["Z"], out[1]["Z"], rtol=1e-9, atol=1e-9)
