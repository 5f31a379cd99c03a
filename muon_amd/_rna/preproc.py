"""``muon_amd.rna.pp``: scanpy's ``normalize_total``, ``log1p``, ``highly_variable_genes`` and ``scale`` on the device
CSR.

The reference opens every RNA modality with these steps (/root/reference/docs/source/omics/*.rst) and hands them to
scanpy; signatures and slots here follow scanpy's.  Parity with scanpy itself is NOT pinned (it is not installed where
this package is tested): every function is stated below and pinned by an independent restatement in the tests, and
``highly_variable_genes`` additionally by a hand-computed case.

Where each step runs:

  * a matrix that carries a device copy (``_hostmatrix.attach_device``), or any sparse matrix when ``backend=`` is
    given: on that backend.  The matrix is uploaded at most once; the result keeps the device copy attached, so
    ``normalize_total -> log1p -> highly_variable_genes -> tl.pca`` cross PCIe for results only.  The value sweep and the
    per-gene moments are kernels of csrc/rna.hip (``value_sweep``, ``gene_moments``); an operator set without them (the
    CPU set of the tests) takes the tensor formulation of the same statements.
  * a matrix without a device copy and no ``backend=``: numpy / scipy on the host, like ``pp.filter_obs`` - these
    functions never start using the GPU on their own.  Dense matrices always take this route.

Statements (f64 arithmetic, one rounding to the storage type; integer matrices become float32):

  normalize_total   x <- x / (total_i / target); target_sum=None: the median of the totals > 0; a cell with total 0
                    keeps its values (divisor 1).
  log1p             x <- log1p(x) (/ ln(base)); ``uns["log1p"] = {"base": base}``.
  highly_variable_genes (flavor "seurat")   e = expm1(x ln(base)) (base from ``uns["log1p"]``), mean_j = sum_i e_ij / n,
                    var_j with ddof = 1 (zeros count); mean == 0 -> 1e-12; disp = var / mean, 0 -> NaN; dispersions =
                    log(disp), means = log1p(mean); bins = pandas.cut(means, n_bins); per bin mean and std (ddof = 1) of
                    the non-NaN dispersions, a bin with fewer than two of them gets std = its mean and mean = 0;
                    dispersions_norm = (dispersions - bin mean) / bin std.  The device computes the per-gene sums, the
                    binning runs on d-vectors on the host.
  scale             stated above ``scale`` at the end of this module: clipped z-scores as a sparse matrix plus one row
                    (csrc/scale.hip: ``scale_values``, ``scale_dense_rows``).
"""
from __future__ import annotations

import logging
import weakref
from typing import Optional
from warnings import warn

import numpy as np
import pandas as pd
import torch
from scipy.sparse import csr_matrix, issparse

from .._containers import modality
from .._hostmatrix import _hash_arrays, device_copy, host_view
from .._operators import has

logger = logging.getLogger("muon_amd")

def _one_rank(comm, what):
    if comm is not None and getattr(comm, "world_size", 1) > 1:
        raise NotImplementedError(f"{what} runs on one rank")


def _float_csr(m):
    """A sparse matrix as float CSR (integers -> float32; a float CSR comes back as it is).  ``device_copy`` then gives
    the CANONICAL host matrix every result is built on: scipy's products and slices hand out unsorted rows, a stored
    value is only a matrix entry once duplicates are summed, and ``log1p`` / ``expm1`` are not linear."""
    if m.format != "csr":
        m = m.tocsr()
    if m.dtype not in (np.float32, np.float64):
        m = m.astype(np.float32)
    return m


def _row_of(X):
    n = X.shape[0]
    return torch.repeat_interleave(torch.arange(n, device=X.indptr.device), X.indptr[1:] - X.indptr[:-1])


def _sweep(be, X, div=None, log=False, log_div=0.0):
    """New values of device CSR ``X``: x / div[row], then log1p, then / log_div (see the module docstring)."""
    if has(be, "value_sweep"):
        return be.value_sweep(X, div=div, log=log, log_div=log_div)
    v = X.values.to(torch.float64)
    if div is not None:
        v = v / div[_row_of(X)]
    if log:
        v = torch.log1p(v)
        if log_div:
            v = v / log_div
    return v.to(X.values.dtype)


def _sweep_host(m, div=None, log=False, log_div=0.0):
    v = m.data.astype(np.float64)
    if div is not None:
        v = v / np.repeat(div, np.diff(m.indptr))
    if log:
        v = np.log1p(v)
        if log_div:
            v = v / log_div
    return v.astype(m.dtype)


def _with_values(m, X, be, values):
    """The host CSR with ``m``'s pattern and the new values; with a device CSR ``X`` the values are a device tensor and
    the new matrix keeps the device copy."""
    if X is None:
        return csr_matrix((values, m.indices.copy(), m.indptr.copy()), shape=m.shape)
    return host_view(X.with_values(values), be, indices=m.indices.copy(), indptr=m.indptr.copy())


def _get(adata, layer):
    return adata.X if layer is None else adata.layers[layer]


def _put(adata, layer, m):
    if layer is None:
        adata.X = m
    else:
        adata.layers[layer] = m


def normalize_total(data, target_sum: Optional[float] = None, *, exclude_highly_expressed: bool = False,
                    layer: Optional[str] = None, inplace: bool = True, copy: bool = False,
                    key_added: Optional[str] = None, comm=None, backend=None):
    """
    Normalize counts per cell: every cell's values are divided by ``total / target_sum`` (scanpy's signature).

    ``target_sum=None``: the median of the totals over the cells with a total > 0.  A cell with total 0 is left as it
    is.  An integer matrix becomes float32.  ``key_added``: the totals go to ``.obs``.  ``inplace=False`` returns
    ``{"X": ..., "norm_factor": ...}`` and touches nothing; ``copy=True`` works on a copy and returns it.
    ``exclude_highly_expressed=True`` is not implemented.  See the module docstring for where it runs.
    """
    if exclude_highly_expressed:
        raise NotImplementedError("normalize_total: exclude_highly_expressed=True is not implemented")
    _one_rank(comm, "rna.pp.normalize_total")
    adata = modality(data, "rna")
    if copy:
        if not inplace:
            raise ValueError("`copy=True` cannot be used with `inplace=False`.")
        adata = adata.copy()
    counts = _get(adata, layer)
    X = be = None
    if issparse(counts):
        m, X, be = device_copy(_float_csr(counts), backend, host_route=True)
        totals = be.to_host(be.row_col_sums(X)[0]) if X is not None else \
            np.asarray(m.astype(np.float64).sum(axis=1)).reshape(-1)
    else:
        m = np.asarray(counts)
        if m.dtype not in (np.float32, np.float64):
            m = m.astype(np.float32)
        totals = m.sum(axis=1, dtype=np.float64)
    totals = np.asarray(totals, dtype=np.float64)
    pos = totals > 0
    target = float(target_sum) if target_sum is not None else (float(np.median(totals[pos])) if pos.any() else 1.0)
    div = np.ones_like(totals)
    div[pos] = totals[pos] / target
    if X is not None:
        new = _with_values(m, X, be, _sweep(be, X, div=be.to_device(div, np.float64)))
    elif issparse(counts):
        new = _with_values(m, None, None, _sweep_host(m, div=div))
    else:
        new = (m.astype(np.float64) / div[:, None]).astype(m.dtype)
    if not inplace:
        return {"X": new, "norm_factor": totals}
    _put(adata, layer, new)
    if key_added is not None:
        adata.obs[key_added] = totals
    return adata if copy else None


def log1p(data, *, base: Optional[float] = None, layer: Optional[str] = None, copy: bool = False, comm=None,
          backend=None):
    """
    Logarithmize the data matrix: ``log1p`` of the stored values, divided by ``ln(base)`` if ``base`` is given;
    ``uns["log1p"] = {"base": base}`` (scanpy's signature).  An integer matrix becomes float32.
    """
    _one_rank(comm, "rna.pp.log1p")
    adata = modality(data, "rna")
    if copy:
        adata = adata.copy()
    counts = _get(adata, layer)
    log_div = float(np.log(base)) if base is not None else 0.0
    if issparse(counts):
        m, X, be = device_copy(_float_csr(counts), backend, host_route=True)
        vals = _sweep(be, X, log=True, log_div=log_div) if X is not None else _sweep_host(m, log=True, log_div=log_div)
        new = _with_values(m, X, be, vals)
    else:
        m = np.asarray(counts)
        if m.dtype not in (np.float32, np.float64):
            m = m.astype(np.float32)
        v = np.log1p(m.astype(np.float64))
        new = (v / log_div if log_div else v).astype(m.dtype)
    _put(adata, layer, new)
    adata.uns["log1p"] = {"base": base}
    return adata if copy else None


# ---- highly variable genes --------------------------------------------------------------------------------------------
def gene_moments_device(be, X, c: float = 1.0, with_e: bool = True):
    """``(sums f64 [4, d], nnz int64 [d])`` of the columns of device CSR ``X`` as host arrays: sum x, sum x^2, sum e,
    sum e^2 with e = expm1(x c) (zero without ``with_e``) and the count of stored non-zero values.  The kernel walks
    the CSR of X^T, a wave per gene (csrc/rna.hip); without it the same sums are tensor operations."""
    d = X.shape[1]
    if has(be, "gene_moments", "gene_moments_max_blocks"):
        sums, cnt = be.gene_moments(be.transpose(X), c=c, with_e=with_e)
    else:
        v = X.values.to(torch.float64)
        col = X.indices.long()
        sums = torch.zeros((4, d), dtype=torch.float64, device=v.device)
        sums[0].index_add_(0, col, v)
        sums[1].index_add_(0, col, v * v)
        if with_e:
            e = torch.expm1(v * c)
            sums[2].index_add_(0, col, e)
            sums[3].index_add_(0, col, e * e)
        cnt = torch.bincount(col[X.values != 0], minlength=d)
    return be.to_host(sums), be.to_host(cnt)


def _e_sums_host(m, c):
    """sum e, sum e^2 per column of a host matrix, e = expm1(x c)."""
    if issparse(m):
        e = m.astype(np.float64).tocsc()
        e.data = np.expm1(e.data * c)
        s1 = np.asarray(e.sum(axis=0)).reshape(-1)
        e.data = e.data * e.data
        return s1, np.asarray(e.sum(axis=0)).reshape(-1)
    e = np.expm1(np.asarray(m, dtype=np.float64) * c)
    return e.sum(axis=0), (e * e).sum(axis=0)


def seurat_dispersions(s1, s2, n, n_bins=20):
    """``(means, dispersions, dispersions_norm)`` of flavor "seurat" from the per-gene sums of e and e^2 over ``n``
    cells (the module docstring states every step)."""
    mean = np.asarray(s1, dtype=np.float64) / n
    var = (np.asarray(s2, dtype=np.float64) / n - mean ** 2) * (n / (n - 1))
    mean[mean == 0] = 1e-12
    disp = var / mean
    disp[disp == 0] = np.nan
    with np.errstate(invalid="ignore", divide="ignore"):
        disp = np.log(disp)
    mean = np.log1p(mean)
    df = pd.DataFrame({"means": mean, "dispersions": disp})
    df["mean_bin"] = pd.cut(df["means"], bins=n_bins)
    grouped = df.groupby("mean_bin", observed=False)["dispersions"]
    bin_mean, bin_std = grouped.mean(), grouped.std(ddof=1)
    single = bin_std.isnull()
    bin_std[single] = bin_mean[single]
    bin_mean[single] = 0
    with np.errstate(invalid="ignore", divide="ignore"):
        norm = (df["dispersions"].values - bin_mean[df["mean_bin"].values].values) / bin_std[df["mean_bin"].values].values
    return mean, disp, np.asarray(norm, dtype=np.float64)


def highly_variable_genes(data, *, n_top_genes: Optional[int] = None, min_mean: float = 0.0125, max_mean: float = 3,
                          min_disp: float = 0.5, max_disp: float = np.inf, n_bins: int = 20, flavor: str = "seurat",
                          subset: bool = False, inplace: bool = True, layer: Optional[str] = None, batch_key=None,
                          comm=None, backend=None):
    """
    Annotate highly variable genes, flavor "seurat", on log-normalised data (scanpy's signature; other flavors and
    ``batch_key`` raise ``NotImplementedError``).

    Writes ``var["highly_variable" | "means" | "dispersions" | "dispersions_norm"]`` and ``uns["hvg"] = {"flavor":
    "seurat"}``; ``inplace=False`` returns the DataFrame instead.  With ``n_top_genes`` the genes whose normalised
    dispersion is ``>=`` the n-th largest non-NaN one are selected (all of them, with a warning, when fewer exist);
    without it ``min_mean < means < max_mean`` and ``min_disp < dispersions_norm < max_disp``; NaN is never selected.
    ``subset=True`` subsets through ``pp.filter_var``, so a device copy follows.  See the module docstring for the
    statement and for where it runs.
    """
    if flavor != "seurat":
        raise NotImplementedError(f"highly_variable_genes: flavor {flavor!r} is not implemented (only 'seurat')")
    if batch_key is not None:
        raise NotImplementedError("highly_variable_genes: batch_key is not implemented")
    _one_rank(comm, "rna.pp.highly_variable_genes")
    adata = modality(data, "rna")
    counts = _get(adata, layer)
    n = int(counts.shape[0])
    base = (adata.uns.get("log1p") or {}).get("base")
    c = float(np.log(base)) if base is not None else 1.0
    X = None
    if issparse(counts):
        m, X, be = device_copy(_float_csr(counts), backend, host_route=True)
    if X is not None:
        sums, _nnz = gene_moments_device(be, X, c=c, with_e=True)
        s1, s2 = sums[2], sums[3]
    else:
        s1, s2 = _e_sums_host(m if issparse(counts) else counts, c)
    means, disps, norm = seurat_dispersions(s1, s2, n, n_bins)

    if n_top_genes is not None:
        ok = norm[~np.isnan(norm)]
        ok[::-1].sort()
        if n_top_genes > ok.size:
            warn("`n_top_genes` > number of normalized dispersions, returning all genes with normalized dispersions.")
            n_top_genes = ok.size
        hv = (np.nan_to_num(norm, nan=-np.inf) >= ok[n_top_genes - 1]) if n_top_genes > 0 else np.zeros(norm.size, bool)
    else:
        with np.errstate(invalid="ignore"):
            hv = (means > min_mean) & (means < max_mean) & (norm > min_disp) & (norm < max_disp)
    df = pd.DataFrame({"means": means, "dispersions": disps, "dispersions_norm": norm, "highly_variable": hv},
                      index=adata.var_names)
    if not inplace:
        return df[df["highly_variable"].values] if subset else df
    adata.uns["hvg"] = {"flavor": "seurat"}
    for col in ("highly_variable", "means", "dispersions", "dispersions_norm"):
        adata.var[col] = df[col].values
    if subset:
        from .._core.preproc import filter_var

        filter_var(adata, np.asarray(hv, dtype=bool), backend=backend)
    return None


# ---- scale ------------------------------------------------------------------------------------------------------------
# Statement (f64 arithmetic, one rounding to the storage type).  Per gene j: mean_j and var_j (ddof = 1) from the sums of
# x and x^2 over all n cells (``_core.pca._moments``), std_j = sqrt(var_j) with 0 -> 1.  The clip range is [-max_value,
# max_value] with ``zero_center``, (-inf, max_value] without (scanpy >= 1.10), the infinities without ``max_value``:
#     C_ij = clip((x_ij - mean_j) / std_j, lo, hi)              (zero_center=False: mean_j = 0 in this formula)
# Every implicit zero of gene j therefore maps to z_j = clip((0 - mean_j) / std_j, lo, hi), and C = S + 1 z^T with
# S_ij = C_ij - z_j on the stored entries of X and nothing anywhere else.
_DENSE_CHUNK_BYTES = 512 << 20  # the dense result leaves the device in row chunks of at most this size


def _clip_np(t, lo, hi):
    """np.clip's result by comparisons (NaN fails both and stays)."""
    t = np.where(t < lo, lo, t)
    return np.where(t > hi, hi, t)


def _clip_t(t, lo, hi):
    t = torch.where(t < lo, torch.full_like(t, lo), t)
    return torch.where(t > hi, torch.full_like(t, hi), t)


def scale_tables(sx, sxx, n, zero_center=True, max_value=None):
    """``(mean, std, centre, z, lo, hi)`` of the statement above from the per-gene sums of x and x^2: ``mean`` and
    ``std`` are what ``var`` receives, ``centre`` is what is subtracted (``mean``, or zeros without ``zero_center``)."""
    from .._core.pca import _moments

    mean, var = _moments(np.asarray(sx, dtype=np.float64), np.asarray(sxx, dtype=np.float64), n, True)
    std = np.sqrt(var)
    std[std == 0] = 1.0
    hi = np.inf if max_value is None else float(max_value)
    lo = -hi if zero_center else -np.inf
    centre = mean if zero_center else np.zeros_like(mean)
    z = _clip_np((0.0 - centre) / std, lo, hi)
    return mean, std, centre, z, lo, hi


def scale_values_tensor(X, mean, std, z, lo, hi):
    """``scale_values`` (include/muon_amd.h) as tensor operations, for operator sets without the kernel."""
    c = X.indices.long()
    t = _clip_t((X.values.to(torch.float64) - mean[c]) / std[c], lo, hi)
    return (t - z[c]).to(X.values.dtype)


def scale_dense_rows_tensor(X, mean, std, z, lo, hi, row_lo, row_hi):
    """``scale_dense_rows`` (include/muon_amd.h) as tensor operations, for operator sets without the kernel."""
    T, d = X.values.dtype, X.shape[1]
    out = z.to(T).repeat(row_hi - row_lo, 1)
    a, b = int(X.indptr[row_lo]), int(X.indptr[row_hi])
    ln = X.indptr[row_lo + 1:row_hi + 1] - X.indptr[row_lo:row_hi]
    row = torch.repeat_interleave(torch.arange(row_hi - row_lo, device=ln.device), ln)
    c = X.indices[a:b].long()
    out[row, c] = _clip_t((X.values[a:b].to(torch.float64) - mean[c]) / std[c], lo, hi).to(T)
    return out.reshape(row_hi - row_lo, d)


# The device form of a dense result.  A plain ndarray takes no attributes, so the forms live in a registry keyed by the
# array's id, each with a weak reference whose callback drops the entry (and with it the device arrays) when the array
# dies: an id is only ever looked up while its array is alive.  Validity is ``resident()``'s rule: the same backend and
# a fingerprint over every byte of the array.
_FORMS = {}


def _dense_fingerprint(a):
    return (a.shape, a.dtype.str, a.flags.c_contiguous) + _hash_arrays([a])


def remember_scaled_form(a, S, z, backend):
    """Remember ``(S, z)`` - ``a == S + 1 z^T`` rounded once - as the device form of the dense ndarray ``a``."""
    key = id(a)
    _FORMS[key] = (weakref.ref(a, lambda _r, key=key: _FORMS.pop(key, None)), S, z, backend, _dense_fingerprint(a))


def scaled_form(a, backend=None):
    """``(S, z, backend)`` remembered for the dense ndarray ``a`` if it still describes ``a``, else None.  Without a
    ``backend`` the form's own serves.  A form whose array was edited in place is dropped."""
    ent = _FORMS.get(id(a)) if type(a) is np.ndarray else None
    if ent is None or ent[0]() is not a or (backend is not None and ent[3] is not backend):
        return None
    if ent[4] != _dense_fingerprint(a):
        _FORMS.pop(id(a), None)
        return None
    return ent[1], ent[2], ent[3]


def _scale_dense_host(m, centre, std, lo, hi):
    """The dense statement on the host, for a dense or a sparse matrix, in row chunks of f64."""
    n, d = m.shape
    out = np.empty((n, d), dtype=m.dtype)
    rows = max(1, _DENSE_CHUNK_BYTES // max(1, 8 * d))
    for r0 in range(0, n, rows):
        blk = m[r0:r0 + rows]
        blk = blk.toarray() if issparse(blk) else np.asarray(blk)
        out[r0:r0 + rows] = _clip_np((blk.astype(np.float64) - centre) / std, lo, hi).astype(m.dtype)
    return out


def scale(data, zero_center: bool = True, max_value: Optional[float] = None, copy: bool = False, *,
          layer: Optional[str] = None, obsm: Optional[str] = None, mask_obs=None, comm=None, backend=None):
    """
    Scale every gene to unit variance and, with ``zero_center``, zero mean (scanpy's signature).

    Mean and standard deviation (ddof = 1; 0 -> 1) are per gene over all cells and go to ``var["mean"]`` and
    ``var["std"]``.  ``max_value`` clips the result: to ``[-max_value, max_value]`` with ``zero_center``, from above
    only without it (scanpy >= 1.10's rule).  An integer matrix becomes float32 (scanpy makes it the default float
    type).  ``obsm`` and ``mask_obs`` raise ``NotImplementedError``.  ``copy=True`` works on a copy and returns it.

    ``zero_center=True`` on a sparse matrix gives a C-ordered dense ndarray of the storage type, as scanpy does.  On a
    device route the dense matrix is written by one fused pass in row chunks that are copied to the host one by one -
    it never exists on the device - and the sparse form ``S`` with ``result == S + 1 z^T`` stays on the device, so that
    a following ``tl.pca`` starts without an upload.  ``zero_center=False`` keeps a sparse matrix sparse (and its
    device copy).  See the module docstring for where it runs; a dense matrix takes the host route.
    """
    if obsm is not None:
        raise NotImplementedError("scale: obsm= is not implemented")
    if mask_obs is not None:
        raise NotImplementedError("scale: mask_obs= is not implemented")
    _one_rank(comm, "rna.pp.scale")
    adata = modality(data, "rna")
    if copy:
        adata = adata.copy()
    counts = _get(adata, layer)
    n = int(counts.shape[0])
    X = be = None
    if issparse(counts):
        m, X, be = device_copy(_float_csr(counts), backend, host_route=True)
    else:
        m = np.asarray(counts)
        if m.dtype not in (np.float32, np.float64):
            m = m.astype(np.float32)
    if X is not None:
        sums, _nnz = gene_moments_device(be, X, with_e=False)
        sx, sxx = sums[0], sums[1]
    elif issparse(m):
        m64 = m.astype(np.float64)
        sx, sxx = np.asarray(m64.sum(axis=0)).reshape(-1), np.asarray(m64.multiply(m64).sum(axis=0)).reshape(-1)
    else:
        m64 = m.astype(np.float64)
        sx, sxx = m64.sum(axis=0), (m64 * m64).sum(axis=0)
    mean, std, centre, z, lo, hi = scale_tables(sx, sxx, n, zero_center, max_value)

    if issparse(m) and zero_center:
        logger.info("scale: zero-centering a sparse matrix densifies it")
    if X is not None:
        tabs = [be.to_device(t, np.float64) for t in (centre, std, z)]
        values = be.scale_values if has(be, "scale_values") else scale_values_tensor
        if zero_center:
            d = int(X.shape[1])
            new = np.empty((n, d), dtype=m.dtype)
            rows = max(1, _DENSE_CHUNK_BYTES // max(1, d * new.dtype.itemsize))
            buf = be.empty((min(rows, n), d), X.values.dtype) if n else None
            for r0 in range(0, n, rows):
                r1 = min(n, r0 + rows)
                if has(be, "scale_dense_rows"):
                    blk = be.scale_dense_rows(X, *tabs, lo, hi, r0, r1, out=buf[:r1 - r0])
                else:
                    blk = scale_dense_rows_tensor(X, *tabs, lo, hi, r0, r1)
                be.to_host(blk.reshape(-1), out=new[r0:r1].reshape(-1))
            remember_scaled_form(new, X.with_values(values(X, *tabs, lo, hi)), z, be)
        else:
            new = _with_values(m, X, be, values(X, *tabs, lo, hi))
    elif issparse(m) and not zero_center:
        v = _clip_np(m.data.astype(np.float64) / std[m.indices], lo, hi)
        new = _with_values(m, None, None, v.astype(m.dtype))
    else:
        new = _scale_dense_host(m, centre, std, lo, hi)
    _put(adata, layer, new)
    adata.var["mean"] = mean
    adata.var["std"] = std
    return adata if copy else None
