"""Plain NumPy restatement of MEFISTO as muon_amd/_core/mefisto.py states it (TEST INFRASTRUCTURE; parity with mofapy2
unpinned, like oracle/mofa_oracle.py whose weight / noise updates this file repeats for gaussian views).

Everything is dense float64: covariances are built entry by entry, inverted with ``np.linalg.inv`` and their
determinants taken with ``np.linalg.slogdet`` - no eigen decomposition, no Woodbury form, no shared code with the package.

    prior      z_k ~ N(0, Sigma_k),  Sigma_k = s_k K(l_k) + (1 - s_k) I,  K(l)_nn' = exp(-|c_n - c_n'|^2 / 2 l^2),  K(0) = I
    grid       0 and n_grid - 1 values spaced geometrically between the smallest non-zero and the largest distance
    Z update   r_k = a[:, k] - sum_{j != k} S[:, k, j] o m_j,  C_k = (Sigma_k^-1 + diag S[:, k, k])^-1,  m_k = C_k r_k
    Z term     -1/2 [tr(Sigma^-1 C) + m^T Sigma^-1 m - N + ln|Sigma| - ln|C|]
    hyper      F(l, s) = -1/2 [ln|Sigma(l, s)| + tr(Sigma(l, s)^-1 (C + m m^T))]: per grid value the bounded scalar
               minimiser over s in [0, 1 - 1e-6], its answer rounded to a multiple of 2^-20 (s = 0 if that is no worse);
               the best pair replaces the current one only if its F is larger; l = 0 goes with s = 0
    predict    Z*[:, k] = s_k K(l_k)(c*, c) Sigma_k^-1 m_k
"""
import math

import numpy as np
from scipy.optimize import minimize_scalar
from scipy.special import digamma

from oracle.mofa_oracle import A0, B0, TH_A0, TH_B0, TOL, _beta_kl, _gamma_kl, init_state, prepare_views

S_MAX = 1.0 - 1e-6
S_STEP = 2.0 ** -20


def sq_dists(c, c2=None):
    c = np.asarray(c, dtype=np.float64).reshape(len(c), -1)
    c2 = c if c2 is None else np.asarray(c2, dtype=np.float64).reshape(len(c2), -1)
    return ((c[:, None, :] - c2[None, :, :]) ** 2).sum(axis=2)


def kernel(d2, ell):
    if ell == 0.0:
        assert d2.shape[0] == d2.shape[1]
        return np.eye(d2.shape[0])
    return np.exp(-d2 / (2.0 * ell * ell))


def grid(cov, n_grid):
    d = np.sqrt(sq_dists(cov))
    return np.concatenate([[0.0], np.geomspace(d[d > 0].min(), d.max(), n_grid - 1)])


def sigma(d2, ell, s):
    N = d2.shape[0]
    return s * kernel(d2, ell) + (1.0 - s) * np.eye(N)


def z_update(a, S, m, Sigmas):
    """One sweep over the factors: (m [N, K] updated copy, diag C [N, K], [C_k])."""
    m = np.array(m, dtype=np.float64, copy=True)
    N, K = m.shape
    dC, Cs = np.zeros((N, K)), []
    for k in range(K):
        r = a[:, k].copy()
        for j in range(K):
            if j != k:
                r -= S[:, k, j] * m[:, j]
        C = np.linalg.inv(np.linalg.inv(Sigmas[k]) + np.diag(S[:, k, k]))
        m[:, k] = C @ r
        dC[:, k] = np.diag(C)
        Cs.append(C)
    return m, dC, Cs


def z_term(Sig, C, m):
    Si = np.linalg.inv(Sig)
    return -0.5 * (np.trace(Si @ C) + m @ Si @ m - len(m) + np.linalg.slogdet(Sig)[1] - np.linalg.slogdet(C)[1])


def hyper_F(Sig, E):
    return -0.5 * (np.linalg.slogdet(Sig)[1] + np.trace(np.linalg.inv(Sig) @ E))


def optimise(d2, ells, C, m, ell_now, s_now):
    """The (l, s) of one factor after a hyperparameter step."""
    E = C + np.outer(m, m)
    best = (ell_now, s_now, hyper_F(sigma(d2, ell_now, s_now), E))
    for ell in ells:
        if ell == 0.0:
            s, F = 0.0, hyper_F(np.eye(len(m)), E)
        else:
            Kl = kernel(d2, ell)
            f = lambda s: -hyper_F(s * Kl + (1.0 - s) * np.eye(len(m)), E)  # noqa: E731
            opt = minimize_scalar(f, bounds=(0.0, S_MAX), method="bounded", options={"xatol": 1e-8})
            s = min(math.floor(float(opt.x) / S_STEP + 0.5) * S_STEP, math.floor(S_MAX / S_STEP) * S_STEP)
            f0, fs = f(0.0), f(s)
            s, F = (0.0, -f0) if f0 <= fs else (s, -fs)
        if F > best[2]:
            best = (ell, s, F)
    ell, s, _ = best
    return (0.0, 0.0) if s == 0.0 else (ell, s)


def predict(cov, new, ell, s, m):
    if s == 0.0 or ell == 0.0:
        return np.zeros(len(new))
    d2 = sq_dists(cov)
    return s * kernel(sq_dists(new, cov), ell) @ np.linalg.inv(sigma(d2, ell, s)) @ m


def run_smooth(views, cov, groups=None, n_factors=3, n_iterations=30, convergence_mode="slow", start_opt=5, opt_freq=5,
               n_grid=6, seed=1, ard_weights=True, spikeslab_weights=True, center_groups=True, scale_views=False,
               scale_groups=False, min_iterations=2):
    """Gaussian views (NaN = missing entry) with a GP prior on the factors; schedule, initialisation and the weight /
    noise updates of oracle.mofa_oracle.run_general.  One covariance spans all samples, whatever the groups."""
    M, N = len(views), views[0].shape[0]
    groups = np.zeros(N, dtype=np.int64) if groups is None else np.asarray(groups, dtype=np.int64)
    G, K = int(groups.max()) + 1, int(n_factors)
    Ys, masks = [], []
    for Y in views:
        (Y,), _ = prepare_views([np.array(Y, dtype=np.float64, copy=True)], groups, center_groups, scale_views, scale_groups)
        masks.append((~np.isnan(Y)).astype(np.float64))
        Ys.append(np.nan_to_num(Y))
    Ds = [Y.shape[1] for Y in Ys]
    st = init_state(N, Ds, G, K, seed)
    EZ, EZ2 = st["EZ"], st["EZ2"]
    gidx = [np.nonzero(groups == g)[0] for g in range(G)]
    gamma = [np.ones((D, K)) for D in Ds]
    EWh2 = [np.ones((D, K)) for D in Ds]
    sig2w = [np.ones((D, K)) for D in Ds]
    d2 = sq_dists(cov)
    ells = grid(cov, n_grid)
    ell, s = [0.0] * K, [0.0] * K
    elbos, hyper_trace = [], []

    for it in range(n_iterations):
        # ---- W (run_general) ------------------------------------------------------------------------------------
        for m in range(M):
            Om = st["tau"][m][groups] * masks[m]
            R = Om * Ys[m]
            EW, EW2 = st["EW"][m], st["EW2"][m]
            aw = st["alpha_w"][m] if ard_weights else np.ones(K)
            b = R.T @ EZ
            for k in range(K):
                t = b[:, k].copy()
                for j in range(K):
                    if j != k:
                        t -= EW[:, j] * (Om.T @ (EZ[:, k] * EZ[:, j]))
                prec = Om.T @ EZ2[:, k] + aw[k]
                s2 = 1.0 / prec
                mu = t * s2
                if spikeslab_weights:
                    lam = (st["lth"][m][k] - st["l1mth"][m][k] + 0.5 * np.log(aw[k]) - 0.5 * np.log(prec) + 0.5 * t * t * s2)
                    gam = 1.0 / (1.0 + np.exp(-lam))
                else:
                    gam = np.ones(Ds[m])
                EW[:, k] = gam * mu
                EW2[:, k] = gam * (mu * mu + s2)
                gamma[m][:, k] = gam
                EWh2[m][:, k] = gam * (mu * mu + s2) + (1.0 - gam) / aw[k]
                sig2w[m][:, k] = s2
        # ---- Z under the GP prior ---------------------------------------------------------------------------------
        a, S = np.zeros((N, K)), np.zeros((N, K, K))
        for m in range(M):
            Om = st["tau"][m][groups] * masks[m]
            EW, EW2 = st["EW"][m], st["EW2"][m]
            a += (Om * Ys[m]) @ EW
            for k in range(K):
                for j in range(K):
                    S[:, k, j] += Om @ (EW2[:, k] if j == k else EW[:, k] * EW[:, j])
        Sigs = [sigma(d2, ell[k], s[k]) for k in range(K)]
        mnew, dC, Cs = z_update(a, S, EZ, Sigs)
        EZ[:], EZ2[:] = mnew, mnew * mnew + dC
        if it >= start_opt and (it - start_opt) % opt_freq == 0:
            for k in range(K):
                ell[k], s[k] = optimise(d2, ells, Cs[k], EZ[:, k], ell[k], s[k])
            Sigs = [sigma(d2, ell[k], s[k]) for k in range(K)]
        hyper_trace.append((list(ell), list(s)))
        # ---- tau and the data terms (run_general) -------------------------------------------------------------------
        elbo = 0.0
        for m in range(M):
            EW, EW2 = st["EW"][m], st["EW2"][m]
            zeta = EZ @ EW.T
            var = EZ2 @ EW2.T - (EZ ** 2) @ (EW ** 2).T
            res = masks[m] * ((Ys[m] - zeta) ** 2 + var)
            for g in range(G):
                i = gidx[g]
                Sg, Ngd = res[i].sum(axis=0), masks[m][i].sum(axis=0)
                pa, pb = A0 + 0.5 * Ngd, B0 + 0.5 * Sg
                st["tau"][m][g], st["ltau"][m][g] = pa / pb, digamma(pa) - np.log(pb)
                elbo += np.sum(0.5 * Ngd * (st["ltau"][m][g] - np.log(2 * np.pi)) - 0.5 * st["tau"][m][g] * Sg)
                elbo += np.sum(_gamma_kl(A0, B0, pa, pb, st["tau"][m][g], st["ltau"][m][g]))
            if ard_weights:
                pa, pb = A0 + 0.5 * Ds[m], B0 + 0.5 * EWh2[m].sum(axis=0)
                st["alpha_w"][m], st["lalpha_w"][m] = pa / pb, digamma(pa) - np.log(pb)
            if spikeslab_weights:
                sg = gamma[m].sum(axis=0)
                pa, pb = TH_A0 + sg, TH_B0 + Ds[m] - sg
                st["lth"][m], st["l1mth"][m] = digamma(pa) - digamma(pa + pb), digamma(pb) - digamma(pa + pb)
        for m in range(M):
            aw = st["alpha_w"][m] if ard_weights else np.ones(K)
            law = st["lalpha_w"][m] if ard_weights else np.zeros(K)
            gam = gamma[m]
            elbo += np.sum(0.5 * law - 0.5 * aw * EWh2[m])
            elbo += np.sum(gam * 0.5 * np.log(sig2w[m]) + (1 - gam) * 0.5 * np.log(1.0 / aw) + 0.5)
            if spikeslab_weights:
                elbo += np.sum(gam * st["lth"][m] + (1 - gam) * st["l1mth"][m])
                with np.errstate(divide="ignore", invalid="ignore"):
                    ent = -(gam * np.log(gam) + (1 - gam) * np.log1p(-gam))
                elbo += np.sum(np.nan_to_num(ent))
                sg = gam.sum(axis=0)
                pa, pb = TH_A0 + sg, TH_B0 + Ds[m] - sg
                elbo += np.sum(_beta_kl(TH_A0, TH_B0, pa, pb, st["lth"][m], st["l1mth"][m]))
            if ard_weights:
                pa, pb = A0 + 0.5 * Ds[m], B0 + 0.5 * EWh2[m].sum(axis=0)
                elbo += np.sum(_gamma_kl(A0, B0, pa, pb, aw, law))
        for k in range(K):
            elbo += z_term(Sigs[k], Cs[k], EZ[:, k])
        elbos.append(float(elbo))
        if it >= min_iterations and len(elbos) >= 2:
            if 100.0 * abs((elbos[-1] - elbos[-2]) / elbos[0]) < TOL[convergence_mode]:
                break
    return {"Z": EZ, "W": st["EW"], "elbo": elbos, "lengthscale": np.asarray(ell), "scale": np.asarray(s),
            "grid": ells, "hyper_trace": hyper_trace}
