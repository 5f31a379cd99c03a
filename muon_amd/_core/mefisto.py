"""MEFISTO: MOFA+ whose factors are smooth over a covariate (time, space) - ``smooth_covariate`` of muon.tl.mofa.

The reference reaches it through ``ent.set_covariates`` / ``ent.set_smooth_options`` / ``ent.predict_factor``
(/root/reference/muon/_core/tools.py:529-597); the arithmetic is mofapy2's, which cannot be inspected here.  Like the rest
of MOFA the model is STATED here, restated in plain NumPy (tests/mefisto_refs.py) and **parity with
mofapy2 is unpinned**.  Weights, noise and their nodes are GeneralMofaEngine's; only the factors' prior differs.

Prior.    z_k ~ N(0, Sigma_k),  Sigma_k = s_k K(l_k) + (1 - s_k) I  over ALL samples of the fit (one covariance spans the
          groups),  K(l)_nn' = exp(-|c_n - c_n'|^2 / 2 l^2),  K(0) = I,  s_k in [0, 1 - 1e-6].  No ARD node on the
          factors (``ard_factors`` is ignored).
Grid.     (ours; mofapy2's is unpinned)  l = 0 and ``n_grid - 1`` values spaced geometrically from the smallest non-zero
          to the largest pairwise covariate distance.  K(l) = V_l diag(e_l) V_l^T is factorised once per grid value
          (torch.linalg.eigh in f64, e clamped at 0): n_grid N^2 8 bytes on the device.
Schedule. Until iteration ``start_opt`` every s_k = 0, Sigma = I: plain MOFA with alpha_z = 1, run by the parent's
          sweep.  From ``start_opt`` on, every ``opt_freq`` iterations, the hyperparameters are re-optimised after the
          Z update of that iteration.
Z update. q(z_k) = N(m_k, C_k).  With a [N, K] and S [N, K, K] as GeneralMofaEngine._update_z forms them, for k in order:
            r_k = a[:, k] - sum_{j != k} S[:, k, j] o m_j   (the updated m_j for j < k),    D_k = diag(S[:, k, k]),
            C_k = (Sigma_k^-1 + D_k)^-1,   m_k = C_k r_k,   <z_nk> = m_nk,   <z_nk^2> = m_nk^2 + (C_k)_nn.
          Eigen route (D_k = c_k I: one group and no view with a sample-dependent precision):
            lambda = s e + 1 - s,  g = lambda / (1 + c lambda),  u = V^T r,  m = V (g o u),  diag C = (V o V) g
            - the operators ``gp_project`` / ``gp_posterior`` (csrc/gp.hip: two passes over V) where the set has them,
            three tensor passes otherwise.
          General route (masks, non-gaussian views, several groups): B = I + D^1/2 Sigma D^1/2 = L L^T,
            C = Sigma - Sigma D^1/2 B^-1 D^1/2 Sigma  (tensor operations).
ELBO.     The factors' term is -KL(q || p) = -1/2 sum_k [tr(Sigma_k^-1 C_k) + m_k^T Sigma_k^-1 m_k - N + ln|Sigma_k|
          - ln|C_k|]: on the eigen route four length-N sums per factor.
Hyper.    For every grid value l:  q_i(l) = diag(V_l^T (C_k + m_k m_k^T) V_l)  (one GEMM and a column-wise product-sum),
          F(l, s) = -1/2 sum_i [ln lambda_i + q_i / lambda_i] is maximised over s on the host
          (scipy.optimize.minimize_scalar, bounded) and the maximiser is rounded to a multiple of 2^-20, so that two
          operator sets whose F differ in the last bits choose the same s.  The best (l, s) replaces the current pair only
          if its F is larger: the bound cannot fall.  l = 0 goes with s = 0.
Predict.  Z*[:, k] = s_k K(l_k)(c*, c) Sigma_k^-1 m_k.
Precision. The GP algebra is f64 whatever the fit's type: with ``use_float32`` only <z> and <z^2> are cast.
"""
from __future__ import annotations

import math
from typing import List

import numpy as np
import torch
from scipy.optimize import minimize_scalar

from .._operators import has
from .mofa_general import GeneralMofaEngine

S_MAX = 1.0 - 1e-6
S_STEP = 2.0 ** -20


def lengthscale_grid(dmin: float, dmax: float, n_grid: int) -> np.ndarray:
    """0 and ``n_grid - 1`` values spaced geometrically from ``dmin`` to ``dmax``."""
    if n_grid < 2:
        raise ValueError(f"n_grid must be at least 2 (the white kernel and one lengthscale), not {n_grid}")
    return np.concatenate([[0.0], np.geomspace(dmin, dmax, n_grid - 1)])


def best_scale(e: np.ndarray, q: np.ndarray):
    """(s, F) maximising F(s) = -1/2 sum_i [ln lambda_i + q_i / lambda_i], lambda = s e + 1 - s, over the multiples of
    2^-20 in [0, 1 - 1e-6] next to the bounded scalar minimiser's answer (and s = 0)."""
    def f(s):
        lam = s * e + (1.0 - s)
        return 0.5 * float(np.sum(np.log(lam) + q / lam))

    opt = minimize_scalar(f, bounds=(0.0, S_MAX), method="bounded", options={"xatol": 1e-8})
    s = min(math.floor(float(opt.x) / S_STEP + 0.5) * S_STEP, math.floor(S_MAX / S_STEP) * S_STEP)
    f0, fs = f(0.0), f(s)
    return (0.0, -f0) if f0 <= fs else (s, -fs)


class SmoothMofaEngine(GeneralMofaEngine):
    def __init__(self, backend, views: List, likelihoods: List[str], groups, n_factors: int, covariates, *,
                 start_opt: int = 20, n_grid: int = 20, opt_freq: int = 10, **kw):
        kw["ard_factors"] = False  # (no alpha_z node under a GP prior: it stays 1 and the parent never updates it)
        if kw.get("spikeslab_factors"):
            raise ValueError("spikeslab_factors=True cannot be combined with smooth_covariate")
        super().__init__(backend, views, likelihoods, groups, n_factors, **kw)
        if self.comm.world_size > 1:
            raise NotImplementedError("smooth_covariate runs on one rank")
        self._graph_ok = False  # (the hyperparameter step asks the host: an iteration is not a fixed launch sequence)
        f64 = torch.float64
        N, K = self.N, self.K
        cov = np.asarray(covariates, dtype=np.float64)
        cov = cov.reshape(N, -1)[self.perm]
        self.start_opt, self.opt_freq, self.n_grid = int(start_opt), max(1, int(opt_freq)), int(n_grid)
        need = self.n_grid * N * N * 8
        if has(backend, "free_memory") and need > backend.free_memory():
            raise ValueError(f"smooth_covariate keeps n_grid x N x N f64 eigenvectors on the device: {self.n_grid} x {N}^2 "
                             f"x 8 = {need} bytes, more than the {backend.free_memory()} bytes that are free "
                             "(a smaller n_grid needs less)")
        self.cov = backend.to_device(np.ascontiguousarray(cov)).to(f64)
        d2 = ((self.cov[:, None, :] - self.cov[None, :, :]) ** 2).sum(dim=2)
        pos = d2[d2 > 0]
        if pos.numel() == 0:
            raise ValueError("smooth_covariate: every sample has the same covariate value")
        self.grid = lengthscale_grid(math.sqrt(float(pos.min())), math.sqrt(float(d2.max())), self.n_grid)
        self._V = torch.empty((self.n_grid, N, N), dtype=f64, device=self.dev)
        self._e = torch.empty((self.n_grid, N), dtype=f64, device=self.dev)
        for l, ell in enumerate(self.grid):
            if ell == 0.0:
                self._V[l] = torch.eye(N, dtype=f64, device=self.dev)
                self._e[l] = 1.0
            else:
                e, V = torch.linalg.eigh(torch.exp(d2 * (-0.5 / (ell * ell))))
                self._V[l], self._e[l] = V, e.clamp(min=0.0)
        del d2
        # D_k = c_k I: one group and every view's precision the same for all samples
        self.eigen_route = bool(self.G == 1 and all(self._row_constant(v) for v in self.views))
        self._kernels = has(backend, "gp_project", "gp_posterior")
        self.li = [0] * K          # index into the grid per factor
        self.s = [0.0] * K         # scale per factor
        self._m64 = self.EZ.to(f64).clone()
        self._d = torch.zeros((N, K), dtype=f64, device=self.dev)   # diag D_k of the last GP sweep
        # per factor, for the ELBO: tr(Sigma^-1 C) + m^T Sigma^-1 m, ln|Sigma|, ln|C|
        self._quad = torch.zeros((K,), dtype=f64, device=self.dev)
        self._ldS = torch.zeros((K,), dtype=f64, device=self.dev)
        self._ldC = torch.zeros((K,), dtype=f64, device=self.dev)
        self._gp_now = False       # this iteration's Z update ran (runs) under the GP prior
        self._chunks_z = []

    @staticmethod
    def _row_constant(V) -> bool:
        if V.stats:
            return V.mask is None
        if V.fused:
            return True
        return bool(V.lik == "gaussian" and V.kind == "sparse" and bool((V.rowmask == 1).all()))

    # -- schedule ---------------------------------------------------------------------------------------------------
    def _hyper_due(self) -> bool:
        it = len(self.elbo)
        return it >= self.start_opt and (it - self.start_opt) % self.opt_freq == 0

    def _update_z(self):
        self._gp_now = any(s > 0.0 for s in self.s) or self._hyper_due()
        self._chunks_z = []
        super()._update_z()

    def _sweep_z(self, g, lo, hi, S, a, az):
        if not self._gp_now:  # Sigma = I: the parent's sweep with alpha_z = 1
            return super()._sweep_z(g, lo, hi, S, a, az)
        self._chunks_z.append((lo, S.to(torch.float64), a.to(torch.float64)))

    def _finish_z(self):
        if not self._gp_now:
            self._m64.copy_(self.EZ)
            return
        parts = sorted(self._chunks_z, key=lambda t: t[0])
        self._chunks_z = []
        S = torch.cat([p[1] for p in parts]) if len(parts) > 1 else parts[0][1]
        a = torch.cat([p[2] for p in parts]) if len(parts) > 1 else parts[0][2]
        self._gp_sweep(a, S)
        if self._hyper_due():
            self._optimise_hyperparameters()

    # -- the factors under the GP prior -----------------------------------------------------------------------------
    def _sigma(self, k):
        l, s = self.li[k], self.s[k]
        eye = torch.eye(self.N, dtype=torch.float64, device=self.dev)
        if s == 0.0 or self.grid[l] == 0.0:
            return eye
        V = self._V[l]
        return s * ((V * self._e[l][None, :]) @ V.T) + (1.0 - s) * eye

    def _dense_cov(self, k, d):
        """(C_k, ln|B|) on the general route: B = I + D^1/2 Sigma D^1/2 = L L^T, C = Sigma - Sigma D^1/2 B^-1 D^1/2 Sigma."""
        Sig = self._sigma(k)
        sd = torch.sqrt(d.clamp(min=0.0))
        B = sd[:, None] * Sig * sd[None, :]
        B.diagonal().add_(1.0)
        L = torch.linalg.cholesky(B)
        X = torch.cholesky_solve(sd[:, None] * Sig, L)  # B^-1 D^1/2 Sigma
        C = Sig - (Sig * sd[None, :]) @ X
        return C, X, sd, 2.0 * torch.log(L.diagonal()).sum()

    def _gp_sweep(self, a, S):
        m, N = self._m64, self.N
        dC = torch.empty_like(m)
        for k in range(self.K):
            d = S[:, k, k]
            r = a[:, k] - (S[:, k, :] * m).sum(dim=1) + d * m[:, k]
            l, s = self.li[k], self.s[k]
            e = self._e[l]
            lam = s * e + (1.0 - s)
            if self.eigen_route:
                c = d[0]
                V = self._V[l]
                g = lam / (1.0 + c * lam)
                if self._kernels:
                    u = self.be.gp_project(V, r.contiguous())
                    mk, dk = self.be.gp_posterior(V, g, u)
                else:
                    u = V.T @ r
                    mk, dk = V @ (g * u), (V * V) @ g
                self._quad[k] = (1.0 / (1.0 + c * lam)).sum() + ((g * u) ** 2 / lam).sum()
                self._ldS[k] = torch.log(lam).sum()
                self._ldC[k] = torch.log(g).sum()
            else:
                C, X, sd, ldB = self._dense_cov(k, d)
                mk, dk = C @ r, C.diagonal().clone()
                # tr(Sigma^-1 C) = tr(B^-1) = N - tr(B^-1 D^1/2 Sigma D^1/2);  Sigma^-1 m = r - D m
                self._quad[k] = (N - (X.diagonal() * sd).sum()) + (mk * (r - d * mk)).sum()
                self._ldS[k] = torch.log(lam).sum()
                self._ldC[k] = self._ldS[k] - ldB
            m[:, k] = mk
            dC[:, k] = dk
            self._d[:, k] = d
        self.EZ.copy_(m)
        self.EZ2.copy_(m * m + dC)

    def _grid_q(self, k):
        """q_i(l) = diag(V_l^T (C_k + m_k m_k^T) V_l) for every grid value l [n_grid, N], from the state the last GP sweep
        left: a GEMM and a column-wise product-sum per grid value."""
        N = self.N
        lc, sc = self.li[k], self.s[k]
        d, mk = self._d[:, k], self._m64[:, k]
        if self.eigen_route:
            lam = sc * self._e[lc] + (1.0 - sc)
            g = lam / (1.0 + d[0] * lam)
            Vc = self._V[lc]
        else:
            C = self._dense_cov(k, d)[0]
        q = torch.empty((self.n_grid, N), dtype=torch.float64, device=self.dev)
        for l in range(self.n_grid):
            V = self._V[l]
            um = V.T @ mk
            if not self.eigen_route:
                q[l] = (V * (C @ V)).sum(dim=0) + um * um
            elif l == lc:
                q[l] = g + um * um
            else:
                A = Vc.T @ V  # C = Vc diag(g) Vc^T: diag(V^T C V)_i = sum_j A_ji^2 g_j
                q[l] = (A * A * g[:, None]).sum(dim=0) + um * um
        return q

    def _optimise_hyperparameters(self):
        for k in range(self.K):
            lc, sc = self.li[k], self.s[k]
            q = self._grid_q(k)
            qh, eh = q.cpu().numpy(), self._e.cpu().numpy()
            lam = sc * eh[lc] + (1.0 - sc)
            best = (lc, sc, -0.5 * float(np.sum(np.log(lam) + qh[lc] / lam)))
            for l in range(self.n_grid):
                s, F = (0.0, -0.5 * float(qh[l].sum())) if self.grid[l] == 0.0 else best_scale(eh[l], qh[l])
                if F > best[2]:
                    best = (l, s, F)
            l, s, _ = best
            if s == 0.0:
                l = 0  # (Sigma = I is the grid's white kernel)
            self.li[k], self.s[k] = l, s
            lam = s * eh[l] + (1.0 - s)
            self._quad[k] = float(np.sum(qh[l] / lam))
            self._ldS[k] = float(np.sum(np.log(lam)))

    def _factor_terms(self, elbo):
        if not self._gp_now:  # Sigma = I, alpha_z = 1 (ard_factors is off): the parent's terms
            return super()._factor_terms(elbo)
        return elbo + (-0.5 * (self._quad - float(self.N) + self._ldS - self._ldC)).sum()

    # -- results ------------------------------------------------------------------------------------------------------
    def predict(self, new_values) -> np.ndarray:
        """Z* [P, K] at the covariate values ``new_values`` [P, C] (in the covariates' own units as the engine was given
        them): s_k K(l_k)(c*, c) Sigma_k^-1 m_k; zero for a factor with s_k = 0.  Factor order of the engine."""
        f64 = torch.float64
        c = self.be.to_device(np.ascontiguousarray(np.asarray(new_values, dtype=np.float64).reshape(-1, self.cov.shape[1]))).to(f64)
        out = torch.zeros((c.shape[0], self.K), dtype=f64, device=self.dev)
        d2 = ((c[:, None, :] - self.cov[None, :, :]) ** 2).sum(dim=2)
        for k in range(self.K):
            l, s = self.li[k], self.s[k]
            if s == 0.0 or self.grid[l] == 0.0:
                continue
            V, lam = self._V[l], s * self._e[l] + (1.0 - s)
            w = V @ ((V.T @ self._m64[:, k]) / lam)  # Sigma^-1 m
            out[:, k] = s * (torch.exp(d2 * (-0.5 / self.grid[l] ** 2)) @ w)
        return self.be.to_host(out).astype(np.float64)

    def results(self, sort_factors=True):
        res = super().results(sort_factors=sort_factors)
        order = res["order"]
        res["smooth"] = {"lengthscale": np.asarray([self.grid[l] for l in self.li], dtype=np.float64)[order],
                         "scale": np.asarray(self.s, dtype=np.float64)[order],
                         "grid": np.asarray(self.grid, dtype=np.float64)}
        return res
