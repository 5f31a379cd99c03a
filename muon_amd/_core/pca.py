"""``muon_amd.tl.pca``: scanpy's ``pca`` on the device CSR, without the dense centred copy.

With mu = 1^T X / n and an optional per-gene scale D (the standard deviations), the centred operator is
A = (X - 1 mu^T) D^-1.  A Q = X (D^-1 Q) - 1 (mu^T D^-1 Q), and the second term is the column mean of Y = X (D^-1 Q);
because the columns of the centred image Y_c sum to zero, A^T Y_c = D^-1 X^T Y_c exactly.  So PCA is the block Lanczos
process of ``atac.tl.lsi`` (``_atac.tools._lsi_device``) with every image block centred column-wise before anything
else reads it (``shift_cols``, csrc/rna.hip) and, with ``scale=True``, two row scalings of d x B blocks per expansion
(``scale_rows``): the matrix stays the CSR it is, and the Krylov phase and its stopping rule work on A.  The per-gene
means and variances come from one sweep over the CSR of X^T (``gene_moments``).  DESIGN.md 9.14.

An f64 ``X`` goes through the f32 process (lsi's f64 continuation is not threaded through the centring).  Without a
device copy and without ``backend=`` the same operator is handed to scipy's ARPACK on the host in f64, like
``pp.filter_obs`` never starts using the GPU on its own.

Pinned against scikit-learn 1.7.2's ``PCA(svd_solver="full")`` on the densified centred (and scaled) matrix and
``TruncatedSVD(algorithm="arpack")`` for ``zero_center=False`` (tests/golden/make_rna_golden.py): subspaces of ``PCs``
and ``X_pca`` and the explained variances.  Parity with scanpy itself is NOT pinned.
"""
from __future__ import annotations

import logging
from typing import Optional

import numpy as np
import torch
from scipy.sparse import issparse

from .._containers import is_anndata
from .._hostmatrix import device_copy

logger = logging.getLogger("muon_amd")


def _mask(adata, mask_var, use_highly_variable):
    """scanpy's rule: ``mask_var`` (a boolean array or the name of a ``var`` column), else ``var["highly_variable"]``
    when it is there and not switched off.  Returns (mask or None, the name recorded in ``uns``)."""
    if use_highly_variable is not None and mask_var is not None:
        raise ValueError("These arguments are incompatible: use_highly_variable and mask_var")
    if use_highly_variable is True and "highly_variable" not in adata.var.columns:
        raise ValueError("Did not find `adata.var['highly_variable']`. Either your data already only consists of highly-"
                         "variable genes or consider running `highly_variable_genes` first.")
    if mask_var is None:
        if use_highly_variable is False or "highly_variable" not in adata.var.columns:
            return None, None
        mask_var = "highly_variable"
    name = mask_var if isinstance(mask_var, str) else None
    if isinstance(mask_var, str):
        if mask_var not in adata.var.columns:
            raise ValueError(f"Did not find `adata.var[{mask_var!r}]`")
        mask_var = adata.var[mask_var].values
    mask = np.asarray(mask_var)
    if mask.dtype != bool or mask.shape != (adata.shape[1],):
        raise ValueError("mask_var must be a boolean array with one entry per variable, or the name of such a column")
    return mask, name


def _moments(sx, sxx, n, zero_center):
    """Per-gene mean and variance (ddof = 1 about the mean; ``zero_center=False``: ddof = 0, scikit-learn's
    TruncatedSVD measures its ratio against that) from the sums of x and x^2."""
    mean = sx / n
    var = np.maximum(sxx / n - mean ** 2, 0.0)
    return mean, (var * (n / (n - 1.0)) if zero_center else var)


def pca_device(backend, X, k, *, zero_center=True, scale=False, seed=1, oversample=None, return_info=False):
    """``(X_pca [n, k] f64 tensor, PCs [d, k] f32 tensor, variance [k], variance_ratio [k][, info])`` of device CSR ``X``
    (one rank).  See the module docstring."""
    from .._atac.tools import DEFAULT_OVERSAMPLE, CentredOperand, lsi_device
    from .._rna.preproc import gene_moments_device

    n, d = X.shape
    if X.values.dtype != torch.float32:
        X = X.with_values(X.values.to(torch.float32))
    sums, _nnz = gene_moments_device(backend, X, with_e=False)
    _mean, var = _moments(sums[0], sums[1], n, True)
    std = np.sqrt(var)
    std[std == 0] = 1.0
    dinv = backend.to_device(1.0 / std, np.float32) if scale else None
    operand = CentredOperand(n, mean=zero_center, dinv=dinv) if (zero_center or scale) else None
    U, stdev, V, info = lsi_device(backend, X, n_comps=k, scale_embeddings=False, seed=seed, return_info=True,
                                   oversample=DEFAULT_OVERSAMPLE if oversample is None else int(oversample),
                                   operand=operand)
    s = stdev * np.sqrt(n - 1.0)
    Xp = U.to(torch.float64) * backend.to_device(s, np.float64)
    _m0, var_used = _moments(sums[0], sums[1], n, zero_center)
    total = float(np.sum(var_used / std ** 2 if scale else var_used))
    if zero_center:
        variance = s ** 2 / (n - 1.0)
    else:  # the variance of the transformed columns, like TruncatedSVD
        variance = backend.to_host(Xp.var(dim=0, unbiased=False))
    ratio = variance / total if total > 0 else np.zeros_like(variance)
    return (Xp, V, variance, ratio, info) if return_info else (Xp, V, variance, ratio)


def pca_host(X, k, *, zero_center=True, scale=False, seed=0):
    """The same operator through scipy's ARPACK in f64 on the host (numpy arrays back)."""
    from scipy.sparse.linalg import LinearOperator, svds

    n, d = X.shape
    if k < 1 or k >= min(n, d):
        raise ValueError(f"`k` must be an integer satisfying `0 < k < min(A.shape)`; got k={k}")
    Xs = X.astype(np.float64) if issparse(X) else np.asarray(X, dtype=np.float64)
    sx = np.asarray(Xs.sum(axis=0)).reshape(-1)
    sxx = np.asarray(Xs.multiply(Xs).sum(axis=0)).reshape(-1) if issparse(X) else (Xs * Xs).sum(axis=0)
    mean, var = _moments(sx, sxx, n, True)
    std = np.sqrt(var)
    std[std == 0] = 1.0
    dinv = 1.0 / std if scale else np.ones(d)
    mu = mean if zero_center else np.zeros(d)

    def mm(Q):
        Qs = dinv[:, None] * Q
        return Xs @ Qs - (mu @ Qs)[None, :]

    def rmm(Y):
        return dinv[:, None] * (Xs.T @ Y - np.outer(mu, Y.sum(axis=0)))

    A = LinearOperator((n, d), matvec=lambda q: mm(q.reshape(-1, 1)).reshape(-1),
                       rmatvec=lambda y: rmm(y.reshape(-1, 1)).reshape(-1), matmat=mm, rmatmat=rmm, dtype=np.float64)
    v0 = np.random.default_rng(seed).standard_normal(min(n, d))
    u, s, vt = svds(A, k=k, v0=v0, tol=1e-12)
    order = np.argsort(-s)
    u, s, vt = u[:, order], s[order], vt[order]
    Xp = u * s
    _m0, var_used = _moments(sx, sxx, n, zero_center)
    total = float(np.sum(var_used * dinv ** 2))
    variance = s ** 2 / (n - 1.0) if zero_center else Xp.var(axis=0)
    return Xp, vt.T, variance, (variance / total if total > 0 else np.zeros_like(variance))


def pca(adata, n_comps: Optional[int] = None, *, zero_center: bool = True, scale: bool = False,
        svd_solver: Optional[str] = None, random_state: int = 0, mask_var=None,
        use_highly_variable: Optional[bool] = None, layer: Optional[str] = None, dtype="float32", copy: bool = False,
        key_added: Optional[str] = None, oversample: Optional[int] = None, diagnostics: Optional[dict] = None,
        comm=None, backend=None):
    """
    Principal component analysis of ``adata.X`` (or ``layer``), scanpy's signature and slots.

    n_comps
            Default ``min(50, min(n_obs, n_vars) - 1)``; ``n_comps >= min(n_obs, n_vars)`` raises lsi's ``ValueError``.
    zero_center
            ``False``: the uncentred truncated SVD; the variances are those of the transformed columns, as in
            scikit-learn's ``TruncatedSVD``.
    scale
            Divide every gene by its standard deviation (ddof = 1; 0 -> 1) after centring: ``sc.pp.scale`` WITHOUT
            ``max_value``, and the scaled matrix is never formed.  With ``max_value`` use ``rna.pp.scale`` first: the
            clipped scaled matrix is a sparse matrix plus one row, and the dense ``X`` it writes from a device CSR is
            decomposed here through that sparse form, without an upload.
    svd_solver
            ``None``, ``"arpack"`` or ``"auto"``: all run the block Lanczos process; others raise
            ``NotImplementedError``.
    mask_var, use_highly_variable
            scanpy's rule: ``var["highly_variable"]`` restricts the genes when it is there and not switched off.  The
            columns are cut out on the device.
    oversample, diagnostics
            Not scanpy's: the block of the Lanczos process holds ``n_comps + oversample`` columns (default 14, as in
            ``atac.tl.lsi``; widths 16, 32 or 64), and ``diagnostics=dict()`` receives the process' own account
            (``block``, ``iterations``, ``spmm``, ``angle_bound``, ``converged``, ...) on a device route.
    Writes ``obsm["X_pca"]`` (n x k, U S), ``varm["PCs"]`` (d x k, zero rows outside the mask) and ``uns["pca"] =
    {"params", "variance" (sigma^2 / (n - 1)), "variance_ratio" (against the sum of the used genes' variances)}``; with
    ``key_added`` all three go under that key.  ``copy=True`` works on a copy and returns it.

    An AnnData only.  One rank.  An f64 matrix goes through the f32 process.  See the module docstring for the
    algorithm and for where it runs.
    """
    if not is_anndata(adata):
        raise TypeError("Expected AnnData object")
    if svd_solver not in (None, "arpack", "auto"):
        raise NotImplementedError(f"pca: svd_solver {svd_solver!r} is not implemented (None, 'arpack', 'auto')")
    if comm is not None and getattr(comm, "world_size", 1) > 1:
        raise NotImplementedError("tl.pca runs on one rank")
    if copy:
        adata = adata.copy()
    mask, mask_name = _mask(adata, mask_var, use_highly_variable)
    counts = adata.X if layer is None else adata.layers[layer]
    n, d_full = counts.shape
    d = d_full if mask is None else int(mask.sum())
    k = min(50, min(n, d) - 1) if n_comps is None else int(n_comps)
    seed = int(random_state) + 1 if random_state is not None else 1

    X = be = None
    if issparse(counts):
        from .._rna.preproc import _float_csr

        counts, X, be = device_copy(_float_csr(counts), backend, host_route=True)
    elif zero_center:
        # a dense matrix that rna.pp.scale wrote from a device CSR is S + 1 z^T with S still on the device: centring
        # removes the rank-one term, so its PCA is the centred process on S
        from .._rna.preproc import scaled_form

        form = scaled_form(counts, backend)
        if form is not None:
            X, _z, be = form
    if X is not None:
        if mask is not None:
            from .preproc import submatrix_device

            X = submatrix_device(be, X, None, mask)
        Xp, V, variance, ratio, info = pca_device(be, X, k, zero_center=zero_center, scale=scale, seed=seed,
                                                  oversample=oversample, return_info=True)
        if diagnostics is not None:
            diagnostics.update({key: val for key, val in info.items() if key != "basis"})
        if not info["converged"]:
            logger.warning("pca: top-%d subspace not resolved to 1e-4 rad (relative gap %.1e, guaranteed angle %.1e "
                           "after %d products)", k, info["gap_rel"], info["angle_bound"], info["spmm"])
        Xp, V = be.to_host(Xp.contiguous()), be.to_host(V.contiguous())
    else:
        sub = counts if mask is None else (counts.tocsr()[:, mask] if issparse(counts) else np.asarray(counts)[:, mask])
        Xp, V, variance, ratio = pca_host(sub, k, zero_center=zero_center, scale=scale, seed=seed)

    dt = np.dtype(dtype)
    pcs = np.zeros((d_full, k), dtype=dt)
    pcs[(slice(None) if mask is None else mask)] = V.astype(dt)
    key_obsm, key_varm, key_uns = ("X_pca", "PCs", "pca") if key_added is None else (key_added,) * 3
    adata.obsm[key_obsm] = Xp.astype(dt)
    adata.varm[key_varm] = pcs
    params = {"zero_center": zero_center, "use_highly_variable": mask_name == "highly_variable", "mask_var": mask_name,
              "scale": scale}
    if layer is not None:
        params["layer"] = layer
    adata.uns[key_uns] = {"params": params, "variance": np.asarray(variance, dtype=np.float64),
                          "variance_ratio": np.asarray(ratio, dtype=np.float64)}
    return adata if copy else None
