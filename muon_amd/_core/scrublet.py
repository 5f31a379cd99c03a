"""``muon_amd.pp.scrublet`` / ``muon_amd.pp.scrublet_simulate_doublets``: doublet detection on the device CSR
(scanpy's ``pp.scrublet`` and ``pp.scrublet_simulate_doublets``, in its core since 1.10; its place in a workflow is
between ``pp.filter_obs`` and ``rna.pp.normalize_total``, on raw counts).

Neither scrublet nor scanpy is installed where this package is tested: parity with their numbers and labels is NOT
pinned.  The arithmetic is this module's own statement, written out below and restated in NumPy / SciPy in
tests/scrublet_refs.py.

The statement, for one matrix of raw counts with n_obs rows (``batch_key``: once per level, on that level's rows):

  1. Gene selection.  On a copy of the observed counts: ``rna.pp.normalize_total`` (median target), ``rna.pp.log1p`` and
     ``rna.pp.highly_variable_genes`` with their defaults.  E = the RAW counts of the flagged genes (a column mask of
     the device CSR); the user's matrix is not modified.
  2. Simulation.  n_sim = int(n_obs * sim_doublet_ratio); parents = np.random.RandomState(random_seed).randint(0, n_obs,
     size=(n_sim, 2)) on the host; E_sim[s] = E[parents[s, 0]] + E[parents[s, 1]]: every column stored in either parent
     stays a stored entry (nothing is pruned), columns ascend, the value is the f32 sum (``csr_pair_rows``,
     csrc/scrublet.hip; ``pair_rows_tensor`` below for operator sets without the kernel).
  3. Normalisation.  The rows of E and of E_sim are scaled to a total of 1e6 (``normalize_total``'s sweep; a row with
     total 0 is left as it is), then ``log1p`` when ``log_transform``.  mu_j and sigma_j are the mean and the POPULATION
     standard deviation (ddof = 0; 0 -> 1) of gene j over the OBSERVED rows only, from the per-gene sums of x and x^2
     (``gene_moments``).  With ``mean_center`` both matrices are centred by mu, with ``normalize_variance`` both are
     divided by sigma (D = diag(sigma)) - implicitly: neither dense matrix ever exists.
  4. Embedding.  V [d, n_prin_comps] = the leading right singular vectors of the observed matrix under that centring and
     scaling (``pca_device``: ``zero_center=mean_center``, ``scale=normalize_variance``; its scale differs from D by
     the constant sqrt(n / (n - 1)), which does not change V).  Both sets of scores are ONE projection each, in f64:
     Z = E_norm (D^-1 V) - mu^T D^-1 V (the row shift only with ``mean_center``, D = I without ``normalize_variance``) -
     one SpMM plus a row shift, for the observed and for the simulated rows alike, so both lie in the same coordinates
     to the last bit of the same operations.
  5. Search.  The rows are [Z_obs; Z_sim] in f64 (``knn_dist_metric="cosine"``: every row divided by its norm first).
     k = n_neighbors or int(round(0.5 * sqrt(n_obs))), r = n_sim / n_obs, k_adj = int(round(k * (1 + r))).  Every row
     takes its k_adj nearest OTHER rows by the f64 GEMM-form squared distance |x|^2 + |y|^2 - 2 x.y, ties by row index;
     n_sim_neigh = the number of them whose index is >= n_obs.  No exact re-evaluation of the candidates' distances
     (``indices_only``: it would gather 3 n_obs * k_adj * p values).  With the filter kernel and enough rows the search
     is ``_candidates_filtered`` over blocks of queries that keep its per-query buffers under ``_BUFFER_BUDGET``; k_adj +
     8 candidates per row come back, ordered by (distance, candidate position) inside the merges, and the final k_adj
     are chosen among them by (distance, row index): a tie changes the count only where more than 8 rows tie at the
     k_adj-th place.  Otherwise: tiles of queries against all rows.
  6. Scores.  rho = expected_doublet_rate, se_rho = stdev_doublet_rate, all f64:
         q     = (n_sim_neigh + 1) / (k_adj + 2)
         Ld    = q * rho / r / (1 - rho - q * (1 - rho - rho / r))
         se_q  = sqrt(q * (1 - q) / (k_adj + 3))
         se_Ld = q * rho / r / (1 - rho - q * (1 - rho - rho / r))**2
                 * sqrt((se_q / q * (1 - rho))**2 + (se_rho / rho * (1 - q))**2)
     Ld over the first n_obs rows is ``doublet_score``, over the rest ``doublet_scores_sim``; se_Ld goes to
     ``doublet_errors_obs`` / ``doublet_errors_sim``.
  7. Threshold (``threshold=None``; on the host).  A 256-bin histogram of the simulated scores is smoothed with
     ``scipy.ndimage.uniform_filter1d(size=3)`` until fewer than three local maxima remain (at most 10 000 rounds; a
     local maximum is a run of equal bins higher than the runs on both sides, a missing side counting as lower, at the
     run's first bin).  With exactly two maxima the threshold is the centre of the lowest bin between them (the first
     such bin).  Otherwise: a ``UserWarning``, no threshold and no ``predicted_doublet``.
  8. Rates.  predicted_doublet = score > threshold; detected_doublet_rate and detectable_doublet_fraction are the means
     of that test over the observed and the simulated rows, overall_doublet_rate their ratio (0 / 0 := 0).
"""
from __future__ import annotations

from typing import Optional
from warnings import warn

import numpy as np
import pandas as pd
import torch
from scipy.ndimage import uniform_filter1d
from scipy.sparse import issparse

from .._backend import DeviceCSR
from .._containers import AnnData, modality
from .._hostmatrix import device_copy, host_view
from .._operators import has

METRICS = ("euclidean", "cosine")
_BUFFER_BUDGET = 1 << 30  # bytes of per-query candidate buffers and lists a block of queries of the search may hold


# ---- 2. simulation ----------------------------------------------------------------------------------------------------
def draw_parents(n_obs: int, sim_doublet_ratio: float, random_seed: int) -> np.ndarray:
    n_sim = int(n_obs * sim_doublet_ratio)
    return np.random.RandomState(random_seed).randint(0, n_obs, size=(n_sim, 2)).astype(np.int64)


def pair_rows_tensor(X: DeviceCSR, parents: torch.Tensor) -> DeviceCSR:
    """``csr_pair_rows`` as tensor operations: the entries of both parents concatenated, sorted by (row, column), and a
    segmented sum - the first entry of a (row, column) as it is, the others added to it (one f32 addition for canonical
    rows: the kernel's bytes).  Also takes rows that are not canonical."""
    n, d = X.shape
    dev = X.indptr.device
    k = int(parents.shape[0])
    rows = parents.reshape(-1)
    lo = X.indptr[rows]
    ln = X.indptr[rows + 1] - lo
    seg = torch.repeat_interleave(torch.arange(2 * k, device=dev), ln)
    first = torch.cumsum(ln, 0) - ln
    pos = lo[seg] + (torch.arange(int(seg.numel()), device=dev) - first[seg])
    key = torch.div(seg, 2, rounding_mode="floor") * d + X.indices[pos].long()
    key, order = torch.sort(key, stable=True)
    v = X.values[pos][order]
    head = torch.ones(key.numel(), dtype=torch.bool, device=dev)
    head[1:] = key[1:] != key[:-1]
    group = torch.cumsum(head.long(), 0) - 1
    out = v[head].clone()
    out.index_add_(0, group[~head], v[~head])
    ukey = key[head]
    srow = torch.div(ukey, d, rounding_mode="floor")
    indptr = torch.zeros(k + 1, dtype=torch.int64, device=dev)
    torch.cumsum(torch.bincount(srow, minlength=k), 0, out=indptr[1:])
    return DeviceCSR(indptr, (ukey - srow * d).to(X.indices.dtype).contiguous(), out.contiguous(), (k, int(d)))


def simulate_device(be, E: DeviceCSR, parents: np.ndarray, canonical: bool = True) -> DeviceCSR:
    """E_sim of step 2 for device CSR ``E`` (f32 values).  ``canonical`` False (rows that may hold duplicates or
    unsorted columns) and operator sets without ``csr_pair_rows`` take the tensor formulation."""
    if E.values.dtype != torch.float32:
        E = E.with_values(E.values.to(torch.float32))
    p = be.to_device(np.ascontiguousarray(parents, dtype=np.int64), np.int64)
    if canonical and has(be, "csr_pair_rows"):
        S = be.csr_pair_rows(E, p)
    else:
        S = pair_rows_tensor(E, p)
    return be.with_slab_ptr(S) if has(be, "with_slab_ptr") else S


# ---- 3 / 4. normalisation and embedding ---------------------------------------------------------------------------------
def _normalise(be, E: DeviceCSR, target: float, log: bool) -> DeviceCSR:
    from .._rna.preproc import _sweep

    totals = be.to_host(be.row_col_sums(E)[0])
    div = np.ones_like(totals)
    pos = totals > 0
    div[pos] = totals[pos] / target
    E = E.with_values(_sweep(be, E, div=be.to_device(div, np.float64)))
    return E.with_values(_sweep(be, E, log=True)) if log else E


def _project(be, E: DeviceCSR, M: torch.Tensor) -> torch.Tensor:
    """E @ M in f64 (M [d, k] f64): SpMMs over blocks of at most 64 columns, padded to the widths the SpMM takes."""
    n, d = E.shape
    k = int(M.shape[1])
    E64 = E.with_values(E.values.to(torch.float64))
    out = torch.empty((n, k), dtype=torch.float64, device=M.device)
    for c0 in range(0, k, 64):
        w = min(64, k - c0)
        B = 16 if w <= 16 else 32 if w <= 32 else 64
        Q = torch.zeros((d, B), dtype=torch.float64, device=M.device)
        Q[:, :w] = M[:, c0:c0 + w]
        out[:, c0:c0 + w] = be.spmm(E64, Q)[:, :w]
    return out


def embed_device(be, E: DeviceCSR, E_sim: DeviceCSR, *, n_prin_comps=30, mean_center=True, normalize_variance=True,
                 log_transform=False, seed=1):
    """``(Z_obs, Z_sim)`` of steps 3 and 4, f64 tensors on the device."""
    from .._rna.preproc import gene_moments_device
    from .pca import pca_device

    n = E.shape[0]
    En = _normalise(be, E, 1e6, log_transform)
    Sn = _normalise(be, E_sim, 1e6, log_transform)
    sums, _nnz = gene_moments_device(be, En, with_e=False)
    mu = sums[0] / n
    sigma = np.sqrt(np.maximum(sums[1] / n - mu ** 2, 0.0))
    sigma[sigma == 0] = 1.0
    _Xp, V, _var, _ratio = pca_device(be, En, int(n_prin_comps), zero_center=bool(mean_center),
                                      scale=bool(normalize_variance), seed=seed)
    M = V.to(torch.float64)
    if normalize_variance:
        M = M / be.to_device(sigma, np.float64)[:, None]
    M = M.contiguous()
    Z_obs, Z_sim = _project(be, En, M), _project(be, Sn, M)
    if mean_center:
        shift = be.to_device(mu, np.float64) @ M
        Z_obs, Z_sim = Z_obs - shift, Z_sim - shift
    return Z_obs, Z_sim


# ---- 5 / 6. search and scores ---------------------------------------------------------------------------------------------
def adjusted_k(n_obs: int, n_sim: int, n_neighbors: Optional[int] = None) -> int:
    k = int(n_neighbors) if n_neighbors else int(round(0.5 * np.sqrt(n_obs)))
    return int(round(k * (1.0 + n_sim / float(n_obs))))


def doublet_scores(n_sim_neigh, k_adj: int, r: float, rho: float, se_rho: float):
    """``(Ld, se_Ld)`` of step 6 for the int array ``n_sim_neigh``."""
    q = (np.asarray(n_sim_neigh, dtype=np.float64) + 1.0) / (k_adj + 2.0)
    den = 1.0 - rho - q * (1.0 - rho - rho / r)
    Ld = q * rho / r / den
    se_q = np.sqrt(q * (1.0 - q) / (k_adj + 3.0))
    se_Ld = q * rho / r / den ** 2 * np.sqrt((se_q / q * (1.0 - rho)) ** 2 + (se_rho / rho * (1.0 - q)) ** 2)
    return Ld, se_Ld


def _count_sim(D, cols, k_adj: int, n_obs: int):
    """Per row of ``D`` [m, c]: how many of its k_adj smallest entries by (value, column number) have a column number
    >= n_obs.  ``cols`` [m, c]: the column numbers, ascending along every row (None: 0 .. c - 1)."""
    kth = torch.kthvalue(D, k_adj, dim=1).values[:, None]
    less = D < kth
    tie = D == kth
    need = k_adj - less.sum(dim=1, keepdim=True)
    take = less | (tie & (torch.cumsum(tie.to(torch.int32), dim=1) <= need))
    sim = (torch.arange(D.shape[1], device=D.device)[None, :] if cols is None else cols) >= n_obs
    return (take & sim).sum(dim=1)


def scrublet_scores_device(be, Z_obs: torch.Tensor, Z_sim: torch.Tensor, k_adj: int, *, expected_doublet_rate=0.05,
                           stdev_doublet_rate=0.02, knn_dist_metric="euclidean", chunk_elems: int = 1 << 28,
                           buffer_budget: Optional[int] = None) -> dict:
    """Steps 5 and 6 for the embeddings ``Z_obs`` [n_obs, p] and ``Z_sim`` [n_sim, p] (f64 tensors on the backend's
    device): ``{"n_sim_neigh" int64 [n_obs + n_sim], "scores", "errors" f64 [n_obs + n_sim], "k_adj", "route"}`` as
    host arrays.  ``buffer_budget``: bytes of per-query buffers a block of queries may hold (default
    ``_BUFFER_BUDGET``)."""
    from . import preproc as pp

    if knn_dist_metric not in METRICS:
        raise NotImplementedError(f"scrublet: knn_dist_metric {knn_dist_metric!r} is not implemented (offered: {METRICS})")
    n_obs, n_sim = int(Z_obs.shape[0]), int(Z_sim.shape[0])
    Z = torch.cat([Z_obs, Z_sim]).to(torch.float64)
    n, p = Z.shape
    k_adj = max(1, min(int(k_adj), n - 1))
    if knn_dist_metric == "cosine":
        Z = Z / torch.sqrt((Z * Z).sum(dim=1, keepdim=True))
    Z = Z.contiguous()
    sq = (Z * Z).sum(dim=1)
    kc = min(k_adj + 8, n - 1)
    counts = torch.empty((n,), dtype=torch.int64, device=Z.device)
    filtered = (has(be, "knn_filter") and n >= 8192 and 4 * kc <= n // 2 and -(-p // 4) * 4 <= pp._KNN_FILTER_MAX_P)
    if filtered:
        cap = 3 * kc + 64
        per_query = cap * 12 + 2 * kc * 16  # the buffer's pairs, and the list before and after a merge
        block = max(64, int(buffer_budget or _BUFFER_BUDGET) // per_query)
        for lo in range(0, n, block):
            hi = min(n, lo + block)
            idx, d = pp._candidates_filtered(be, Z, sq, kc, chunk_elems, queries=None if (lo, hi) == (0, n) else (lo, hi))
            o = torch.argsort(idx, dim=1)
            counts[lo:hi] = _count_sim(torch.gather(d, 1, o), torch.gather(idx, 1, o), k_adj, n_obs)
    else:
        rows = max(1, min(n, chunk_elems // n))
        ar = torch.arange(n, device=Z.device)
        for lo in range(0, n, rows):
            hi = min(n, lo + rows)
            D = sq[lo:hi, None] + sq[None, :] - 2.0 * (Z[lo:hi] @ Z.T)
            D[ar[lo:hi] - lo, ar[lo:hi]] = float("inf")  # not the row itself
            counts[lo:hi] = _count_sim(D, None, k_adj, n_obs)
    nsn = be.to_host(counts)
    Ld, se = doublet_scores(nsn, k_adj, n_sim / float(n_obs), float(expected_doublet_rate), float(stdev_doublet_rate))
    return {"n_sim_neigh": nsn, "scores": Ld, "errors": se, "k_adj": k_adj, "route": "filtered" if filtered else "tiled"}


# ---- 7 / 8. threshold and rates -------------------------------------------------------------------------------------------
def _local_maxima(h: np.ndarray) -> np.ndarray:
    """First bins of the runs of equal values that are higher than the runs on both sides (a missing side: lower)."""
    start = np.flatnonzero(np.r_[True, h[1:] != h[:-1]])
    v = h[start]
    left = np.r_[-np.inf, v[:-1]]
    right = np.r_[v[1:], -np.inf]
    return start[(v > left) & (v > right)]


def bimodal_threshold(scores_sim, n_bins: int = 256, max_rounds: int = 10000) -> Optional[float]:
    """The threshold of step 7 for the simulated scores, or None when the smoothed histogram is not bimodal."""
    scores_sim = np.asarray(scores_sim, dtype=np.float64)
    if scores_sim.size == 0:
        return None
    hist, edges = np.histogram(scores_sim, bins=n_bins)
    h = hist.astype(np.float64)
    peaks = _local_maxima(h)
    rounds = 0
    while peaks.size >= 3 and rounds < max_rounds:
        h = uniform_filter1d(h, size=3)
        peaks = _local_maxima(h)
        rounds += 1
    if peaks.size != 2:
        return None
    i = int(peaks[0]) + int(np.argmin(h[peaks[0]:peaks[1] + 1]))
    return float(0.5 * (edges[i] + edges[i + 1]))


def call_doublets(scores_obs, scores_sim, threshold: Optional[float] = None) -> dict:
    """Steps 7 and 8: ``{"threshold", "predicted_doublet", "detected_doublet_rate", "detectable_doublet_fraction",
    "overall_doublet_rate"}``, or ``{}`` (after a ``UserWarning``) when no threshold is given and none is found."""
    if threshold is None:
        threshold = bimodal_threshold(scores_sim)
        if threshold is None:
            warn("scrublet: the histogram of the simulated doublet scores is not bimodal: no threshold was set and "
                 "`predicted_doublet` is not written; pass `threshold=`.", UserWarning, stacklevel=3)
            return {}
    threshold = float(threshold)
    called = np.asarray(scores_obs) > threshold
    detected = float(called.mean()) if called.size else 0.0
    sim = np.asarray(scores_sim) > threshold
    detectable = float(sim.mean()) if sim.size else 0.0
    return {"threshold": threshold, "predicted_doublet": called, "detected_doublet_rate": detected,
            "detectable_doublet_fraction": detectable,
            "overall_doublet_rate": detected / detectable if detectable > 0 else 0.0}


# ---- the whole procedure for one matrix -------------------------------------------------------------------------------------
def select_genes_device(be, X: DeviceCSR) -> np.ndarray:
    """The boolean gene mask of step 1 for the raw counts ``X`` (f32 or f64 device CSR); ``X`` is not modified."""
    from .._rna.preproc import _sweep, gene_moments_device, seurat_dispersions

    n = X.shape[0]
    totals = be.to_host(be.row_col_sums(X)[0])
    pos = totals > 0
    target = float(np.median(totals[pos])) if pos.any() else 1.0
    div = np.ones_like(totals)
    div[pos] = totals[pos] / target
    Y = X.with_values(_sweep(be, X, div=be.to_device(div, np.float64)))
    Y = Y.with_values(_sweep(be, Y, log=True))
    sums, _nnz = gene_moments_device(be, Y, c=1.0, with_e=True)
    means, _disp, norm = seurat_dispersions(sums[2], sums[3], n)
    with np.errstate(invalid="ignore"):
        return (means > 0.0125) & (means < 3) & (norm > 0.5) & (norm < np.inf)


def scrublet_device(be, E: DeviceCSR, E_sim: DeviceCSR, *, expected_doublet_rate=0.05, stdev_doublet_rate=0.02,
                    knn_dist_metric="euclidean", normalize_variance=True, log_transform=False, mean_center=True,
                    n_prin_comps=30, n_neighbors=None, threshold=None, random_state=0) -> dict:
    """Steps 3 to 8 for the observed and the simulated counts on the selected genes; the result of one batch."""
    n_obs, n_sim = int(E.shape[0]), int(E_sim.shape[0])
    if n_obs < 2 or n_sim < 1:
        raise ValueError(f"scrublet: {n_obs} observed and {n_sim} simulated rows are too few")
    Z_obs, Z_sim = embed_device(be, E, E_sim, n_prin_comps=n_prin_comps, mean_center=mean_center,
                                normalize_variance=normalize_variance, log_transform=log_transform,
                                seed=int(random_state or 0) + 1)
    k_adj = adjusted_k(n_obs, n_sim, n_neighbors)
    res = scrublet_scores_device(be, Z_obs, Z_sim, k_adj, expected_doublet_rate=expected_doublet_rate,
                                 stdev_doublet_rate=stdev_doublet_rate, knn_dist_metric=knn_dist_metric)
    out = {"doublet_score": res["scores"][:n_obs], "doublet_scores_sim": res["scores"][n_obs:],
           "doublet_errors_obs": res["errors"][:n_obs], "doublet_errors_sim": res["errors"][n_obs:]}
    out.update(call_doublets(out["doublet_score"], out["doublet_scores_sim"], threshold))
    return out


def _raw_counts(adata, layer, backend):
    """(host CSR, device CSR, backend) of the raw counts: the resident copy where there is one, else one upload."""
    from .._rna.preproc import _float_csr

    counts = adata.X if layer is None else adata.layers[layer]
    if not issparse(counts):
        raise TypeError("scrublet: expected a sparse matrix of raw counts")
    return device_copy(_float_csr(counts), backend)


def _check_offered(synthetic_doublet_umi_subsampling, knn_dist_metric="euclidean"):
    if synthetic_doublet_umi_subsampling != 1.0:
        raise NotImplementedError("scrublet: synthetic_doublet_umi_subsampling != 1.0 is not implemented (offered: 1.0, "
                                  "the plain sum of the two parents)")
    if knn_dist_metric not in METRICS:
        raise NotImplementedError(f"scrublet: knn_dist_metric {knn_dist_metric!r} is not implemented (offered: {METRICS})")


def scrublet_simulate_doublets(data, *, layer: Optional[str] = None, sim_doublet_ratio: float = 2.0,
                               synthetic_doublet_umi_subsampling: float = 1.0, random_seed: int = 0, backend=None):
    """
    Simulate doublets by adding the raw counts of random pairs of observed cells (scanpy's signature).

    Returns an AnnData of the ``int(n_obs * sim_doublet_ratio)`` simulated rows over ALL variables of ``data`` (an
    AnnData, or a MuData with an ``'rna'`` modality): ``X`` is a CSR that carries its device copy, ``obsm[
    "doublet_parents"]`` the pairs (int64 [n_sim, 2]) and ``uns["scrublet"]["parameters"]`` the arguments.  Step 2 of
    the module docstring; ``synthetic_doublet_umi_subsampling != 1.0`` raises ``NotImplementedError``.
    """
    _check_offered(synthetic_doublet_umi_subsampling)
    adata = modality(data, "rna")
    _m, X, be = _raw_counts(adata, layer, backend)
    parents = draw_parents(X.shape[0], sim_doublet_ratio, random_seed)
    S = simulate_device(be, X, parents)
    sim = AnnData(host_view(S, be, canonical=True), var=adata.var.copy(), obsm={"doublet_parents": parents},
                  uns={"scrublet": {"parameters": {"sim_doublet_ratio": float(sim_doublet_ratio),
                                                   "synthetic_doublet_umi_subsampling": 1.0,
                                                   "random_seed": random_seed}}})
    return sim


def scrublet(data, adata_sim=None, *, batch_key: Optional[str] = None, sim_doublet_ratio: float = 2.0,
             expected_doublet_rate: float = 0.05, stdev_doublet_rate: float = 0.02,
             synthetic_doublet_umi_subsampling: float = 1.0, knn_dist_metric: str = "euclidean",
             normalize_variance: bool = True, log_transform: bool = False, mean_center: bool = True,
             n_prin_comps: int = 30, n_neighbors: Optional[int] = None, threshold: Optional[float] = None,
             copy: bool = False, random_state: int = 0, backend=None):
    """
    Predict doublets from raw counts (scanpy's ``pp.scrublet`` signature; the statement is the module docstring).

    ``data``: an AnnData of raw counts (sparse), or a MuData with an ``'rna'`` modality.  Writes ``obs["doublet_score"]``,
    ``obs["predicted_doublet"]`` when a threshold exists, and ``uns["scrublet"]`` = ``{"doublet_scores_sim",
    "doublet_parents", "doublet_errors_obs", "doublet_errors_sim", "parameters"}`` plus ``"threshold"``,
    ``"detected_doublet_rate"``, ``"detectable_doublet_fraction"`` and ``"overall_doublet_rate"`` when a threshold
    exists.  ``batch_key``: the whole procedure per level of that ``obs`` column; ``uns["scrublet"]["batches"]`` holds one
    such dict per level (``doublet_parents`` in the level's own row numbers), ``"batched_by"`` the key, and the top level
    the concatenated simulated scores.  ``adata_sim``: simulated rows from ``scrublet_simulate_doublets`` over the same
    variables; the gene selection is then skipped and all variables are used (not with ``batch_key``).
    ``copy=True`` writes to a copy and returns it.

    The matrix is used through its device copy (uploaded once where it has none) and is not modified: a following
    ``pp.filter_obs(data, "predicted_doublet", lambda x: ~x)`` subsets that copy on the device.
    ``synthetic_doublet_umi_subsampling != 1.0`` and metrics other than "euclidean" and "cosine" raise
    ``NotImplementedError``.  Parity with scanpy's or scrublet's numbers is not pinned.
    """
    from .preproc import submatrix_device

    _check_offered(synthetic_doublet_umi_subsampling, knn_dist_metric)
    adata = modality(data, "rna")
    if adata_sim is not None and batch_key is not None:
        raise ValueError("scrublet: adata_sim cannot be combined with batch_key")
    if batch_key is not None and batch_key not in adata.obs.columns:
        raise ValueError(f"scrublet: `batch_key` {batch_key!r} is no column of .obs")
    _m, X, be = _raw_counts(adata, None, backend)
    n = int(X.shape[0])
    kw = dict(expected_doublet_rate=expected_doublet_rate, stdev_doublet_rate=stdev_doublet_rate,
              knn_dist_metric=knn_dist_metric, normalize_variance=normalize_variance, log_transform=log_transform,
              mean_center=mean_center, n_prin_comps=n_prin_comps, n_neighbors=n_neighbors, threshold=threshold,
              random_state=random_state)

    def one(Xb):
        if adata_sim is not None:
            if int(adata_sim.shape[1]) != int(Xb.shape[1]):
                raise ValueError("scrublet: adata_sim must have the variables of the observed data")
            _ms, S, _be = _raw_counts(adata_sim, None, be)
            res = scrublet_device(be, Xb, S, **kw)
            res["doublet_parents"] = np.asarray(adata_sim.obsm["doublet_parents"], dtype=np.int64)
            return res
        genes = select_genes_device(be, Xb)
        if int(genes.sum()) < 2:
            raise ValueError("scrublet: fewer than two genes pass highly_variable_genes' defaults")
        E = submatrix_device(be, Xb, None, genes)
        parents = draw_parents(int(Xb.shape[0]), sim_doublet_ratio, random_state)
        res = scrublet_device(be, E, simulate_device(be, E, parents), **kw)
        res["doublet_parents"] = parents
        return res

    ratio = sim_doublet_ratio
    if adata_sim is not None:
        ratio = ((adata_sim.uns.get("scrublet") or {}).get("parameters") or {}).get("sim_doublet_ratio", ratio)
    params = {"sim_doublet_ratio": float(ratio), "expected_doublet_rate": expected_doublet_rate,
              "stdev_doublet_rate": stdev_doublet_rate, "synthetic_doublet_umi_subsampling": 1.0,
              "knn_dist_metric": knn_dist_metric, "normalize_variance": normalize_variance,
              "log_transform": log_transform, "mean_center": mean_center, "n_prin_comps": n_prin_comps,
              "n_neighbors": n_neighbors, "random_state": random_state}
    rate_keys = ("threshold", "detected_doublet_rate", "detectable_doublet_fraction", "overall_doublet_rate")
    uns_keys = ("doublet_scores_sim", "doublet_parents", "doublet_errors_obs", "doublet_errors_sim")

    if batch_key is None:
        res = one(X)
        score, called = res["doublet_score"], res.get("predicted_doublet")
        uns = {k: res[k] for k in uns_keys + rate_keys if k in res}
    else:
        levels = pd.Series(np.asarray(adata.obs[batch_key])).astype("category")
        score = np.full(n, np.nan)
        called = np.zeros(n, dtype=bool)
        batches, all_called = {}, True
        for level in levels.cat.categories:
            mask = np.asarray(levels == level)
            res = one(submatrix_device(be, X, mask, None))
            score[mask] = res["doublet_score"]
            if "predicted_doublet" in res:
                called[mask] = res["predicted_doublet"]
            else:
                all_called = False
            batches[level] = {k: res[k] for k in uns_keys + rate_keys if k in res}
        if not all_called:
            called = None
        uns = {"batches": batches, "batched_by": batch_key,
               "doublet_scores_sim": np.concatenate([b["doublet_scores_sim"] for b in batches.values()])}
    uns["parameters"] = params

    target = adata.copy() if copy else adata
    target.obs["doublet_score"] = score
    if called is not None:
        target.obs["predicted_doublet"] = called
    elif "predicted_doublet" in target.obs.columns:
        del target.obs["predicted_doublet"]
    target.uns["scrublet"] = uns
    return target if copy else None
