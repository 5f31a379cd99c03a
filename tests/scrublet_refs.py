"""TEST INFRASTRUCTURE: the NumPy / SciPy restatement of muon_amd.pp.scrublet's statement (the docstring of
muon_amd/_core/scrublet.py), independent of the package's tensors and kernels: row-by-row unions, a
dense centred matrix and ``np.linalg.svd``, brute-force distances, plain loops over histogram bins.  Also the engineered
parent rows of the pair-merge tests and the planted data set with true doublets that the tests share."""
from functools import lru_cache

import numpy as np
import pandas as pd
import scipy.sparse as sp
from scipy.ndimage import uniform_filter1d

from tests.synth import planted_topics_csr


# ---- step 2: simulation -------------------------------------------------------------------------------------------------
def simulate(E, parents):
    """(indptr int64, indices, data f32) of E_sim: row s = the union of the patterns of E[parents[s, 0]] and
    E[parents[s, 1]] (canonical rows), columns ascending, nothing pruned, the f32 sum where both store the column."""
    ip, ix, dv = E.indptr, E.indices, E.data.astype(np.float32)
    cols_out, vals_out, lens = [], [], []
    for a, b in np.asarray(parents):
        ca, va = ix[ip[a]:ip[a + 1]], dv[ip[a]:ip[a + 1]]
        cb, vb = ix[ip[b]:ip[b + 1]], dv[ip[b]:ip[b + 1]]
        cols = np.union1d(ca, cb)
        out = np.zeros(cols.size, dtype=np.float32)
        from_a = np.zeros(cols.size, dtype=bool)
        ia, ib = np.searchsorted(cols, ca), np.searchsorted(cols, cb)
        out[ia] = va
        from_a[ia] = True
        both = from_a[ib]
        out[ib[both]] = out[ib[both]] + vb[both]
        out[ib[~both]] = vb[~both]
        cols_out.append(cols.astype(ix.dtype))
        vals_out.append(out)
        lens.append(cols.size)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cat = lambda parts, dt: np.concatenate(parts) if parts else np.zeros(0, dtype=dt)  # noqa: E731
    return indptr, cat(cols_out, ix.dtype), cat(vals_out, np.float32)


def simulate_csr(E, parents):
    indptr, indices, data = simulate(E, parents)
    return sp.csr_matrix((data, indices, indptr), shape=(len(parents), E.shape[1]))


# ---- the engineered parent rows of the pair-merge tests ---------------------------------------------------------------------
PAIR_LENGTHS = (0, 1, 63, 64, 65, 129, 520)
PAIR_CONDITIONS = ("disjoint", "identical", "nested", "interleaved", "late_matches", "stored_zeros")


def _row_pair(rng, la, lb, condition, d):
    """Two ascending column lists of lengths la and lb (as far as the condition allows) in [0, d)."""
    if condition == "identical":
        a = np.sort(rng.choice(d, size=la, replace=False))
        return a, a.copy()
    if condition == "nested":  # the shorter row's columns are all among the longer row's
        big = np.sort(rng.choice(d, size=max(la, lb), replace=False))
        small = np.sort(rng.choice(big, size=min(la, lb), replace=False)) if min(la, lb) else big[:0]
        return (big, small) if la >= lb else (small, big)
    if condition == "interleaved":  # a on even columns, b on odd ones, strictly alternating while both last
        return 2 * np.arange(la), 2 * np.arange(lb) + 1
    if condition == "late_matches":  # the rows share columns only in a's last 64-entry step
        a = np.sort(rng.choice(d // 2, size=la, replace=False))
        tail = a[(max(la - 1, 0) // 64) * 64:]
        n_shared = min(lb, tail.size)
        shared = tail[tail.size - n_shared:]
        rest = d // 2 + np.sort(rng.choice(d // 2, size=lb - n_shared, replace=False))
        return a, np.sort(np.concatenate([shared, rest]))
    cols = rng.choice(d, size=la + lb, replace=False)  # disjoint, stored_zeros
    return np.sort(cols[:la]), np.sort(cols[la:])


@lru_cache(maxsize=None)
def pair_case(index_dtype="int32", d=4096, seed=3):
    """(E canonical CSR f32, parents int64 [n_sim, 2]): every pairing of PAIR_LENGTHS under every condition, both
    orders of the pair among them, and a row paired with itself."""
    rng = np.random.default_rng(seed)
    rows, parents = [], []
    for condition in PAIR_CONDITIONS:
        for la in PAIR_LENGTHS:
            for lb in PAIR_LENGTHS:
                a, b = _row_pair(rng, la, lb, condition, d)
                va = rng.integers(1, 9, size=a.size).astype(np.float32)
                vb = rng.integers(1, 9, size=b.size).astype(np.float32)
                if condition == "stored_zeros":
                    va[::3], vb[1::2] = 0.0, 0.0
                rows += [(a, va), (b, vb)]
                parents.append((len(rows) - 2, len(rows) - 1))
                if condition in ("nested", "late_matches"):
                    parents.append((len(rows) - 1, len(rows) - 2))
    parents += [(i, i) for i in range(0, len(rows), 7)]
    indptr = np.concatenate([[0], np.cumsum([r[0].size for r in rows])]).astype(np.int64)
    E = sp.csr_matrix((np.concatenate([r[1] for r in rows]),
                       np.concatenate([r[0] for r in rows]).astype(index_dtype), indptr), shape=(len(rows), d))
    parents = np.asarray(parents, dtype=np.int64)
    for arr in (E.data, E.indices, E.indptr, parents):
        arr.setflags(write=False)
    return E, parents


# ---- steps 1, 3, 4: gene selection, normalisation, embedding ------------------------------------------------------------------
def _scaled_f32(M, target):
    """the rows of M scaled to ``target`` (f64 arithmetic, one rounding to f32); target None: the median of the totals > 0"""
    M = sp.csr_matrix(M, dtype=np.float32)
    M.sort_indices()
    totals = np.asarray(M.astype(np.float64).sum(axis=1)).reshape(-1)
    pos = totals > 0
    if target is None:
        target = float(np.median(totals[pos])) if pos.any() else 1.0
    div = np.ones_like(totals)
    div[pos] = totals[pos] / target
    out = M.copy()
    out.data = (M.data.astype(np.float64) / np.repeat(div, np.diff(M.indptr))).astype(np.float32)
    return out


def select_genes(counts):
    """boolean gene mask: normalize_total (median target), log1p, highly_variable_genes (flavor "seurat", defaults)"""
    Y = _scaled_f32(counts, None)
    Y.data = np.log1p(Y.data.astype(np.float64)).astype(np.float32)
    n = Y.shape[0]
    e = np.expm1(Y.toarray().astype(np.float64))
    mean = e.sum(axis=0) / n
    var = ((e * e).sum(axis=0) / n - mean ** 2) * (n / (n - 1))
    mean[mean == 0] = 1e-12
    disp = var / mean
    disp[disp == 0] = np.nan
    with np.errstate(invalid="ignore", divide="ignore"):
        disp = np.log(disp)
    mean = np.log1p(mean)
    bins = pd.cut(pd.Series(mean), bins=20)
    norm = np.full(mean.size, np.nan)
    for b in bins.cat.categories:
        sel = np.asarray(bins == b)
        ok = disp[sel][~np.isnan(disp[sel])]
        if ok.size >= 2:
            m, s = ok.mean(), ok.std(ddof=1)
        else:  # a bin with fewer than two dispersions: std = its mean, mean = 0
            m, s = 0.0, (ok.mean() if ok.size else np.nan)
        with np.errstate(invalid="ignore", divide="ignore"):
            norm[sel] = (disp[sel] - m) / s
    with np.errstate(invalid="ignore"):
        return (mean > 0.0125) & (mean < 3) & (norm > 0.5) & (norm < np.inf)


def embed(E, E_sim, n_prin_comps=30, mean_center=True, normalize_variance=True, log_transform=False, solver="svd",
          solver_seed=0):
    """(Z_obs, Z_sim) in f64: rows to a total of 1e6, optional log1p, the observed rows' means and population standard
    deviations, V from ``np.linalg.svd`` of the dense centred and scaled observed matrix (``solver="pca_host"``: from
    the package's ARPACK route, the measure of what a different eigensolver changes), Z = A V for both."""
    A, S = _scaled_f32(E, 1e6), _scaled_f32(E_sim, 1e6)
    if log_transform:
        A.data = np.log1p(A.data.astype(np.float64)).astype(np.float32)
        S.data = np.log1p(S.data.astype(np.float64)).astype(np.float32)
    A_sparse = A
    A, S = A.toarray().astype(np.float64), S.toarray().astype(np.float64)
    mu = A.mean(axis=0)
    sigma = A.std(axis=0)
    sigma[sigma == 0] = 1.0
    if not normalize_variance:
        sigma = np.ones_like(sigma)
    if not mean_center:
        mu = np.zeros_like(mu)
    A, S = (A - mu) / sigma, (S - mu) / sigma
    if solver == "svd":
        V = np.linalg.svd(A, full_matrices=False)[2][:n_prin_comps].T
    else:
        from muon_amd._core.pca import pca_host

        V = pca_host(A_sparse, n_prin_comps, zero_center=mean_center, scale=normalize_variance, seed=solver_seed)[1]
    return A @ V, S @ V


# ---- steps 5, 6: search and scores ---------------------------------------------------------------------------------------------
def adjusted_k(n_obs, n_sim, n_neighbors=None):
    k = n_neighbors or int(round(0.5 * np.sqrt(n_obs)))
    return int(round(k * (1 + n_sim / n_obs)))


def sim_neighbours(Z_obs, Z_sim, k_adj, metric="euclidean"):
    """(n_sim_neigh int64 [n], gap f64 [n]): brute force over the f64 GEMM-form squared distances, ties by row index;
    gap = the relative difference between the k_adj-th and the (k_adj + 1)-th squared distance of the row."""
    Z = np.concatenate([Z_obs, Z_sim]).astype(np.float64)
    if metric == "cosine":
        Z = Z / np.sqrt((Z * Z).sum(axis=1, keepdims=True))
    n_obs = Z_obs.shape[0]
    sq = (Z * Z).sum(axis=1)
    D = sq[:, None] + sq[None, :] - 2.0 * (Z @ Z.T)
    np.fill_diagonal(D, np.inf)
    order = np.argsort(D, axis=1, kind="stable")  # (equal distances stay in index order)
    nsn = (order[:, :k_adj] >= n_obs).sum(axis=1).astype(np.int64)
    dk = np.take_along_axis(D, order[:, k_adj - 1:k_adj + 1], axis=1)
    gap = (dk[:, 1] - dk[:, 0]) / np.maximum(np.abs(dk[:, 1]), 1e-300)
    return nsn, gap


def sim_neighbours_by_partition(Z_obs, Z_sim, k_adj):
    """``sim_neighbours`` (euclidean) for inputs too large to sort whole rows: the k_adj-th and (k_adj + 1)-th smallest
    squared distances by ``np.partition``, the count = the simulated rows at or below the k_adj-th.  The count is the
    sorted one wherever gap > 0 (no tie at the k_adj-th place); the callers leave the other rows out."""
    Z = np.concatenate([Z_obs, Z_sim]).astype(np.float64)
    n_obs = Z_obs.shape[0]
    sq = (Z * Z).sum(axis=1)
    D = sq[:, None] + sq[None, :] - 2.0 * (Z @ Z.T)
    np.fill_diagonal(D, np.inf)
    dk = np.partition(D, [k_adj - 1, k_adj], axis=1)[:, k_adj - 1:k_adj + 1]
    nsn = (D[:, n_obs:] <= dk[:, :1]).sum(axis=1).astype(np.int64)
    return nsn, (dk[:, 1] - dk[:, 0]) / np.maximum(np.abs(dk[:, 1]), 1e-300)


def merge_reference(cur_d, cur_p, buf_d, buf_pos, cnt):
    """(out_d, out_p, thr) of the merge after a filter pass: per query the kc smallest (distance, position) pairs of
    list ++ buffer[:min(cnt, cap)] by a stable two-key sort."""
    n, kc = cur_d.shape
    cap = buf_d.shape[1]
    out_d, out_p = np.empty_like(cur_d), np.empty_like(cur_p)
    for q in range(n):
        c = min(max(int(cnt[q]), 0), cap)
        d = np.concatenate([cur_d[q], buf_d[q, :c]])
        p = np.concatenate([cur_p[q], buf_pos[q, :c].astype(np.int64)])
        o = np.argsort(p, kind="stable")
        o = o[np.argsort(d[o], kind="stable")][:kc]
        out_d[q], out_p[q] = d[o], p[o]
    return out_d, out_p, out_d[:, -1].copy()


def scores(n_sim_neigh, k_adj, r, rho=0.05, se_rho=0.02):
    """(Ld, se_Ld), one row at a time in Python floats (f64)"""
    Ld, se = np.empty(len(n_sim_neigh)), np.empty(len(n_sim_neigh))
    for i, m in enumerate(n_sim_neigh):
        q = (int(m) + 1) / (k_adj + 2)
        denom = 1 - rho - q * (1 - rho - rho / r)
        Ld[i] = q * rho / r / denom
        se_q = (q * (1 - q) / (k_adj + 3)) ** 0.5
        se[i] = q * rho / r / denom ** 2 * ((se_q / q * (1 - rho)) ** 2 + (se_rho / rho * (1 - q)) ** 2) ** 0.5
    return Ld, se


# ---- steps 7, 8: threshold and rates ---------------------------------------------------------------------------------------------
def _maxima(h):
    """the first bins of the plateaus that are higher than what lies on both sides (a missing side counts as lower)"""
    out, i, n = [], 0, len(h)
    while i < n:
        j = i
        while j + 1 < n and h[j + 1] == h[i]:
            j += 1
        left_lower = i == 0 or h[i - 1] < h[i]
        right_lower = j == n - 1 or h[j + 1] < h[i]
        if left_lower and right_lower:
            out.append(i)
        i = j + 1
    return out


def threshold(scores_sim):
    """the centre of the lowest bin between the two maxima of the smoothed 256-bin histogram, or None"""
    hist, edges = np.histogram(np.asarray(scores_sim, dtype=np.float64), bins=256)
    h = hist.astype(np.float64)
    rounds = 0
    while len(_maxima(h)) >= 3 and rounds < 10000:
        h = uniform_filter1d(h, size=3)
        rounds += 1
    peaks = _maxima(h)
    if len(peaks) != 2:
        return None
    best = peaks[0]
    for i in range(peaks[0], peaks[1] + 1):
        if h[i] < h[best]:
            best = i
    return (edges[best] + edges[best + 1]) / 2


def scrublet(counts, *, sim_doublet_ratio=2.0, expected_doublet_rate=0.05, stdev_doublet_rate=0.02,
             knn_dist_metric="euclidean", normalize_variance=True, log_transform=False, mean_center=True,
             n_prin_comps=30, n_neighbors=None, random_state=0, solver="svd", solver_seed=0, thr=None):
    """The whole statement for one matrix of raw counts (scipy CSR): a dict with the keys the package writes."""
    counts = sp.csr_matrix(counts)
    counts.sort_indices()
    n_obs = counts.shape[0]
    genes = select_genes(counts)
    E = counts[:, genes].astype(np.float32)
    E.sort_indices()
    n_sim = int(n_obs * sim_doublet_ratio)
    parents = np.random.RandomState(random_state).randint(0, n_obs, size=(n_sim, 2))
    E_sim = simulate_csr(E, parents)
    Z_obs, Z_sim = embed(E, E_sim, n_prin_comps, mean_center, normalize_variance, log_transform, solver, solver_seed)
    k_adj = adjusted_k(n_obs, n_sim, n_neighbors)
    nsn, gap = sim_neighbours(Z_obs, Z_sim, k_adj, knn_dist_metric)
    Ld, se = scores(nsn, k_adj, n_sim / n_obs, expected_doublet_rate, stdev_doublet_rate)
    out = {"genes": genes, "doublet_parents": parents, "n_sim_neigh": nsn, "gap": gap, "k_adj": k_adj,
           "doublet_score": Ld[:n_obs], "doublet_scores_sim": Ld[n_obs:], "doublet_errors_obs": se[:n_obs],
           "doublet_errors_sim": se[n_obs:], "Z_obs": Z_obs, "Z_sim": Z_sim}
    t = threshold(out["doublet_scores_sim"]) if thr is None else thr
    if t is not None:
        called, sim = out["doublet_score"] > t, out["doublet_scores_sim"] > t
        out.update(threshold=t, predicted_doublet=called, detected_doublet_rate=called.mean(),
                   detectable_doublet_fraction=sim.mean(),
                   overall_doublet_rate=called.mean() / sim.mean() if sim.mean() > 0 else 0.0)
    return out


# ---- the planted data set ---------------------------------------------------------------------------------------------------------
def _planted_labels(n, d, n_topics, seed):
    """the topic of every cell of planted_topics_csr(n, d, n_topics, seed=seed): the generator's own draws, replayed"""
    rng = np.random.default_rng(seed)
    rng.gamma(2.0, 1.0, size=d)
    for _ in range(n_topics):
        sel = rng.choice(d, size=max(1, int(0.05 * d)), replace=False)
        rng.gamma(2.0, 1.0, size=sel.size)
    return rng.integers(0, n_topics, size=n)


@lru_cache(maxsize=None)
def planted_doublets(n=1500, d=2000, frac=0.10, density=0.05, seed=11):
    """(counts CSR f32 [n + n_dbl, d], is_doublet bool): three well separated clusters from tests/synth.py's generator and
    ``frac`` true heterotypic doublets, each the sum of two cells of different clusters, appended and then shuffled."""
    X = planted_topics_csr(n, d, n_topics=3, density=density, seed=seed, dtype=np.float32)
    labels = _planted_labels(n, d, 3, seed)
    # (the replay is right: the cells of a label are nearest to that label's mean profile)
    P = sp.diags(1.0 / np.asarray(X.sum(axis=1)).reshape(-1)) @ X
    cent = np.stack([np.asarray(P[labels == t].mean(axis=0)).reshape(-1) for t in range(3)])
    assert ((P @ cent.T).argmax(axis=1) == labels).mean() > 0.99
    rng = np.random.default_rng(seed + 1)
    n_dbl = int(frac * n)
    a = rng.integers(0, n, size=n_dbl)
    b = np.array([rng.choice(np.flatnonzero(labels != labels[i])) for i in a])
    both = sp.vstack([X, X[a] + X[b]], format="csr")
    order = rng.permutation(n + n_dbl)
    out = both[order].astype(np.float32)
    out.sort_indices()
    out.indices, out.indptr = out.indices.astype(np.int32), out.indptr.astype(np.int64)
    return out, (order >= n)
