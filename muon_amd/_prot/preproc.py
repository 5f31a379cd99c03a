"""muon.prot.pp.dsb / muon.prot.pp.clr on MI355X.

Host side mirrors /root/reference/muon/_prot/preproc.py:17-224 (``dsb``) and :227-299 (``clr``): same signatures and
defaults, same argument checks, errors, warnings and write-back.  The reference densifies both matrices and fits two
scikit-learn ``GaussianMixture`` models per cell in a Python loop (:189-198); here

  * the mean and ``ddof=1`` standard deviation of ``log(x + pseudocount)`` over the empty droplets come from the CSR as
    it is (``HipBackend.prot_log_moments``, csrc/prot.hip);
  * every cell is one wave: row -> scaled values in registers -> scikit-learn's EM for the ``tied`` and the ``full``
    model in f64 -> background mean, both BICs, both iteration counts (``HipBackend.prot_dsb_fit``);
  * the rank-1 regression and the clip are element-wise tensor operations on the device.

``_gmm_fit_torch`` is the same EM as batched tensor operations over all cells at once, with per-cell convergence masks.
It runs when the backend lacks the kernels (the CPU operator set of the tests) and for panels wider than
``prot_max_proteins()``, and it is what the kernel is compared with on shapes no fixture reaches.

Random responsibilities follow scikit-learn (``init_params="random"``): with an integer ``random_state`` every fit
re-seeds, so one ``(n_proteins, 2)`` matrix of uniform draws serves every cell and both models; a ``RandomState``
instance advances through tied then full, cell after cell, and is consumed in that order (in chunks of cells);
``None`` takes a fresh seed.
"""
from __future__ import annotations

import numbers
from typing import Iterable, Optional, Tuple
from warnings import warn

import numpy as np
import pandas as pd
import torch
from scipy.sparse import issparse

from .._backend import DeviceCSR, backend_or_default
from .._containers import is_anndata, is_mudata
from .._operators import has

_REG_COVAR = 1e-6
_TOL = 1e-3
_MAX_ITER = 100
_NK_EPS = 10 * np.finfo(np.float64).eps
_LOG_2PI = float(np.log(2 * np.pi))
_LN2 = float(np.log(2.0))


# ---- host matrix -> device ------------------------------------------------------------------------------------------
def _value_dtype(dt) -> np.dtype:
    """float32 stays (numpy keeps it through ``log(x + pseudocount)``), everything else is computed from f64 values."""
    return np.dtype(np.float32) if np.dtype(dt) == np.float32 else np.dtype(np.float64)


def _to_device(be, X):
    """``X`` (scipy sparse, ndarray, DeviceCSR or tensor) as a DeviceCSR or a dense [n, d] tensor of f32 / f64."""
    if isinstance(X, (DeviceCSR, torch.Tensor)):
        return X
    if issparse(X):
        m = X.tocsr()
        if not (m.has_canonical_format and m.has_sorted_indices):
            m = m.copy()
            m.sum_duplicates()
        kw = {"slab_ptr": False} if has(be, "with_slab_ptr") else {}  # (no sweep of tfidf / lsi follows)
        return be.upload_csr(m.indptr, m.indices, m.data, m.shape, values_dtype=_value_dtype(m.dtype), **kw)
    a = np.asarray(X)
    return be.to_device(a, _value_dtype(a.dtype))


def _rows(X, lo: int, hi: int):
    """Rows [lo, hi) of a device matrix; a CSR keeps its entry arrays (row pointers stay absolute)."""
    if isinstance(X, DeviceCSR):
        return DeviceCSR(X.indptr[lo:hi + 1], X.indices, X.values, (hi - lo, X.shape[1]))
    return X[lo:hi]


def _dense(X) -> torch.Tensor:
    if not isinstance(X, DeviceCSR):
        return X
    n, d = X.shape
    out = torch.zeros((n, d), dtype=X.values.dtype, device=X.values.device)
    e0, e1 = int(X.indptr[0].item()), int(X.indptr[-1].item())
    rows = torch.repeat_interleave(torch.arange(n, device=out.device), X.indptr[1:] - X.indptr[:-1])
    out[rows, X.indices[e0:e1].long()] = X.values[e0:e1]
    return out


def _log_pc(Xd: torch.Tensor, pc: float) -> torch.Tensor:
    """``np.log(X + pseudocount)`` as f64; a float32 matrix is added and logged in float32, as numpy does."""
    if Xd.dtype == torch.float32:
        return torch.log(Xd + torch.tensor(pc, dtype=torch.float32, device=Xd.device)).double()
    return torch.log(Xd.double() + pc)


def _is_f32(X) -> bool:
    return (X.values.dtype if isinstance(X, DeviceCSR) else X.dtype) == torch.float32


# ---- the tensor formulation -------------------------------------------------------------------------------------------
def _log_moments_torch(X, pc: float):
    y = _log_pc(_dense(X), pc)
    if y.shape[0] < 2:
        return y.mean(dim=0), torch.full((y.shape[1],), float("nan"), dtype=torch.float64, device=y.device)
    return y.mean(dim=0), y.std(dim=0, unbiased=True)


def _scale_torch(X, pc: float, mean, std):
    z = _log_pc(_dense(X), pc) - mean
    if std is not None:
        z = z / std
    if _is_f32(X):
        z = z.float().double()
    return z


def _m_step(x, x2, r0, r1, full: bool):
    """sklearn.mixture._gaussian_mixture._estimate_gaussian_parameters for one feature; rows = cells."""
    nk0, nk1 = r0.sum(dim=1) + _NK_EPS, r1.sum(dim=1) + _NK_EPS
    m0, m1 = (r0 * x).sum(dim=1) / nk0, (r1 * x).sum(dim=1) / nk1
    if full:
        d0, d1 = x - m0[:, None], x - m1[:, None]
        c0 = ((r0 * d0) * d0).sum(dim=1) / nk0 + _REG_COVAR
        c1 = ((r1 * d1) * d1).sum(dim=1) / nk1 + _REG_COVAR
    else:
        c0 = c1 = (x2 - ((nk0 * m0) * m0 + (nk1 * m1) * m1)) / (nk0 + nk1) + _REG_COVAR
    return nk0, nk1, m0, m1, 1.0 / torch.sqrt(c0), 1.0 / torch.sqrt(c1)


def _e_step(x, w0, w1, m0, m1, p0, p1):
    """_estimate_log_prob_resp: log p(x) per value and the responsibilities (scipy's logsumexp over two entries)."""
    y0 = x * p0[:, None] - (m0 * p0)[:, None]
    y1 = x * p1[:, None] - (m1 * p1)[:, None]
    a0 = (-0.5 * (_LOG_2PI + y0 * y0) + torch.log(p0)[:, None]) + torch.log(w0)[:, None]
    a1 = (-0.5 * (_LOG_2PI + y1 * y1) + torch.log(p1)[:, None]) + torch.log(w1)[:, None]
    mx, mn = torch.maximum(a0, a1), torch.minimum(a0, a1)
    lpn = torch.where(a0 == a1, _LN2 + a0, torch.log1p(torch.exp(mn - mx)) + mx)
    return lpn, torch.exp(a0 - lpn), torch.exp(a1 - lpn)


def _gmm_fit_torch(x: torch.Tensor, u: torch.Tensor, full: bool):
    """scikit-learn's ``GaussianMixture(2, covariance_type=tied|full, init_params="random").fit`` of every row of ``x``
    [n, d] at once.  ``u``: uniform draws [d, 2] or [n, d, 2].  Returns (min of the means [n], BIC [n], n_iter_ [n])."""
    n, d = x.shape
    su = u[..., 0] + u[..., 1]
    r0 = (u[..., 0] / su).expand(n, d).contiguous()
    r1 = (u[..., 1] / su).expand(n, d).contiguous()
    x2 = (x * x).sum(dim=1)
    nk0, nk1, m0, m1, p0, p1 = _m_step(x, x2, r0, r1, full)
    par = torch.stack([nk0 / d, nk1 / d, m0, m1, p0, p1], dim=1)  # (_initialize: weights / n_samples)
    del r0, r1
    lower = torch.full((n,), -float("inf"), dtype=torch.float64, device=x.device)
    n_iter = torch.zeros((n,), dtype=torch.int32, device=x.device)
    active = torch.arange(n, device=x.device)
    for it in range(1, _MAX_ITER + 1):
        if active.numel() == 0:
            break
        xa, x2a = x[active], x2[active]
        lpn, q0, q1 = _e_step(xa, *par[active].unbind(dim=1))
        nk0, nk1, m0, m1, p0, p1 = _m_step(xa, x2a, q0, q1, full)
        ws = nk0 + nk1
        par[active] = torch.stack([nk0 / ws, nk1 / ws, m0, m1, p0, p1], dim=1)
        new = lpn.sum(dim=1) / d
        change = new - lower[active]
        lower[active] = new
        n_iter[active] = it
        active = active[~(change.abs() < _TOL)]
    lpn, _, _ = _e_step(x, *par.unbind(dim=1))
    score = lpn.sum(dim=1) / d
    bic = -2.0 * score * d + (5.0 if full else 4.0) * float(np.log(d))
    lo = torch.minimum(par[:, 2], par[:, 3])
    lo = torch.where(torch.isnan(par[:, 2]) | torch.isnan(par[:, 3]), torch.full_like(lo, float("nan")), lo)
    return lo, bic, n_iter


def _fit_torch(X, pc: float, mean, std, resp):
    """What ``HipBackend.prot_dsb_fit`` computes, as tensor operations."""
    z = _scale_torch(X, pc, mean, std)
    shared = resp.dim() == 2
    lo_t, bic_t, it_t = _gmm_fit_torch(z, resp if shared else resp[:, 0], False)
    lo_f, bic_f, it_f = _gmm_fit_torch(z, resp if shared else resp[:, 1], True)
    bg = torch.where(bic_t < bic_f, lo_t, lo_f)
    if _is_f32(X):
        bg = bg.float().double()
    return z, bg, torch.stack([bic_t, bic_f], dim=1), torch.stack([it_t, it_f], dim=1)


# ---- random responsibilities ------------------------------------------------------------------------------------------
def _resp_chunks(random_state, n: int, d: int):
    """Yield (lo, hi, uniform draws) over the cells: one shared [d, 2] matrix for a seed, [hi - lo, 2, d, 2] blocks in
    scikit-learn's order of consumption (cell after cell, tied then full) for a RandomState instance."""
    if random_state is None:
        random_state = int(np.random.SeedSequence().generate_state(1)[0])
    if isinstance(random_state, numbers.Integral):
        yield 0, n, np.random.RandomState(int(random_state)).uniform(size=(d, 2))
        return
    if not isinstance(random_state, np.random.RandomState):
        raise ValueError(f"{random_state!r} cannot be used to seed a numpy.random.RandomState instance")
    step = max(1, (64 << 20) // (32 * d))
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        yield lo, hi, random_state.uniform(size=(hi - lo, 2, d, 2))


# ---- the arithmetic of dsb ------------------------------------------------------------------------------------------
def _quantiles(flat_sorted: torch.Tensor, q: np.ndarray) -> np.ndarray:
    """np.quantile(..., method="linear") of a sorted vector (numpy's lerp, including its branch for t >= 0.5)."""
    N = flat_sorted.numel()
    out = []
    for qi in np.asarray(q, dtype=np.float64):
        pos = qi * (N - 1)
        lo = int(np.floor(pos))
        hi = min(lo + 1, N - 1)
        t = pos - lo
        a, b = float(flat_sorted[lo].item()), float(flat_sorted[hi].item())
        out.append(b - (b - a) * (1 - t) if t >= 0.5 else a + (b - a) * t)
    return np.asarray(out)


def _dsb_arrays(cells_X, empty_X, *, pseudocount=10, denoise_counts=True, ctrl_idx=None, scale_factor="standardize",
                quantile_clipping=False, quantile_clip=(0.001, 0.9995), random_state=None, backend=None,
                force_tensor=False, diagnostics: Optional[dict] = None):
    """Lines :161-218 of the reference on the device: the normalised matrix as a [n_cells, n_proteins] f64 tensor.
    ``force_tensor``: the tensor formulation even where the kernels apply (what tests compare the kernels with).
    ``diagnostics``: a dict that receives mean / std of the empty droplets and, with denoising, the background means,
    BICs and iteration counts (host arrays)."""
    be = backend_or_default(backend)
    pc = float(pseudocount)
    Xc, Xe = _to_device(be, cells_X), _to_device(be, empty_X)
    n, d = (int(s) for s in Xc.shape)
    limit = be.prot_max_proteins() if has(be, "prot_max_proteins") else 0
    kernels = not force_tensor and d <= limit
    if kernels and has(be, "prot_log_moments") and pc > 0 and Xe.shape[0] >= 1:
        mean, std = be.prot_log_moments(Xe, pc)
    else:  # (also pseudocount == 0: log(0) makes the closed form for the zeros invalid; numpy's non-finite results)
        mean, std = _log_moments_torch(Xe, pc)
    std_used = std if scale_factor == "standardize" else None
    if diagnostics is not None:
        diagnostics["mean"], diagnostics["std"] = be.to_host(mean), be.to_host(std)
    if not denoise_counts:
        z = _scale_torch(Xc, pc, mean, std_used)
    else:
        if d < 2:
            # scikit-learn's validate_data(ensure_min_samples=2): a cell's proteins are the samples of its mixture
            raise ValueError(f"Found array with {d} sample(s) (shape=({d}, 1)) while a minimum of 2 is required by "
                             "GaussianMixture.")
        use_fit = kernels and has(be, "prot_dsb_fit")
        parts = []
        for lo, hi, u in _resp_chunks(random_state, n, d):
            resp = be.to_device(u, np.float64)
            Xs = _rows(Xc, lo, hi) if (lo, hi) != (0, n) else Xc
            parts.append(be.prot_dsb_fit(Xs, pc, mean, std_used, resp) if use_fit else
                         _fit_torch(Xs, pc, mean, std_used, resp))
        z, bg, bic, n_iter = (torch.cat([p[i] for p in parts]) if len(parts) > 1 else parts[0][i] for i in range(4))
        if diagnostics is not None:
            diagnostics.update(bgmeans=be.to_host(bg), bic=be.to_host(bic), n_iter=be.to_host(n_iter),
                               scaled=be.to_host(z))
        if ctrl_idx is not None:
            # first principal component of [isotype controls, background mean]: sign and whitening scale cancel in
            # covar * slope below, so the leading eigenvector of the (c + 1) x (c + 1) scatter matrix is enough
            idx = torch.as_tensor(np.asarray(ctrl_idx, dtype=np.int64), device=z.device)
            M = torch.cat([z[:, idx], bg[:, None]], dim=1)
            Mc = M - M.mean(dim=0)
            _w, V = np.linalg.eigh(be.to_host(Mc.T @ Mc))
            covar = Mc @ torch.as_tensor(np.ascontiguousarray(V[:, -1]), device=z.device)
        else:
            covar = bg
        # LinearRegression(fit_intercept=True, copy_X=False) of every protein on the covariate, then
        # `predict(covar) - intercept_` (:211-214).  copy_X=False lets fit() centre the covariate IN PLACE, and the
        # reference predicts from that same array: what it subtracts is (covar - mean(covar)) * slope (the principal
        # component of the isotype branch has mean zero anyway)
        cc = covar - covar.mean()
        slope = (cc @ (z - z.mean(dim=0))) / (cc @ cc)
        z = z - cc[:, None] * slope[None, :]
    if _is_f32(Xc):
        z = z.float().double()  # (the reference's matrix is float32 from :177 on)
    if quantile_clipping:
        qs = _quantiles(torch.sort(z.reshape(-1)).values, np.asarray(quantile_clip))
        z = torch.clamp(z, min=float(qs.min()), max=float(qs.max()))
    return z


def _out_dtype(X) -> np.dtype:
    dt = np.dtype(X.dtype) if not isinstance(X, (DeviceCSR, torch.Tensor)) else None
    if dt is None:
        return np.dtype(np.float32) if _is_f32(X) else np.dtype(np.float64)
    return dt if dt.kind == "f" else np.dtype(np.float64)


def _row_sums(X, be) -> np.ndarray:
    if isinstance(X, DeviceCSR):
        return be.to_host(be.row_col_sums(X)[0])
    return np.asarray(X.sum(axis=1)).squeeze()


def dsb(
    data,
    data_raw=None,
    pseudocount: numbers.Integral = 10,
    denoise_counts: bool = True,
    isotype_controls: Optional[Iterable[str]] = None,
    empty_counts_range: Optional[Tuple[numbers.Real, numbers.Real]] = None,
    cell_counts_range: Optional[Tuple[numbers.Real, numbers.Real]] = None,
    scale_factor: str = "standardize",
    quantile_clipping: bool = False,
    quantile_clip: Tuple[float, float] = (0.001, 0.9995),
    add_layer: bool = False,
    random_state=None,
    *,
    backend=None,
):
    """
    Normalize protein expression with DSB (Denoised and Scaled by Background)

    Normalized data will be written to ``data`` (if it is an AnnData object) or ``data.mod['prot']``
    (if it is a MuData object) as an X matrix or as a new layer named ``dsb``.  Arguments, checks, warnings and
    return value are the reference's (/root/reference/muon/_prot/preproc.py:17-224); see the module docstring for
    where the arithmetic runs.  Float input keeps its dtype, integer counts give float64; the arithmetic is f64.

    Returns ``None`` if ``data_raw`` is not ``None`` (the normalized data are written to ``data``), otherwise a
    ``MuData`` object containing the filtered data (non-empty droplets).
    """
    be = None
    toreturn = None
    if data_raw is None:
        if empty_counts_range is None or cell_counts_range is None:
            raise ValueError(
                "data_raw is None, assuming data is the unfiltered object, but no count ranges provided"
            )
        if max(*empty_counts_range) > min(*cell_counts_range):
            raise ValueError("overlapping count ranges")
        if not is_mudata(data) or "prot" not in data.mod or "rna" not in data.mod:
            raise TypeError(
                "No data_raw given, assuming data is the unfiltered object, but data is not MuData"
                " or does not contain 'prot' and 'rna' modalities"
            )
        if data.mod["rna"].n_obs != data.mod["prot"].n_obs:
            raise ValueError("different numbers of cells in 'rna' and 'prot' modalities.")

        be = backend_or_default(backend)
        log10umi = np.log10(_row_sums(data.mod["rna"].X, be) + 1)
        empty_idx = np.where(
            (log10umi >= min(*empty_counts_range)) & (log10umi < max(*empty_counts_range))
        )[0]
        cell_idx = np.where(
            (log10umi >= min(*cell_counts_range)) & (log10umi < max(*cell_counts_range))
        )[0]
        cellidx = data.mod["prot"].obs_names[cell_idx]
        empty = data.mod["prot"][empty_idx, :]

        data = data[cellidx, :].copy()
        cells = data.mod["prot"]

        toreturn = data

    elif is_anndata(data_raw):
        empty = data_raw
    elif is_mudata(data_raw) and "prot" in data_raw.mod:
        empty = data_raw["prot"]
    else:
        raise TypeError("data_raw must be an AnnData or a MuData object with 'prot' modality")

    if is_anndata(data):
        cells = data
    elif is_mudata(data) and "prot" in data.mod:
        cells = data["prot"]
    else:
        raise TypeError("data must be an AnnData or a MuData object with 'prot' modality")

    if pseudocount < 0:
        raise ValueError("pseudocount cannot be negative")

    if quantile_clipping:
        if len(quantile_clip) != 2:
            raise ValueError("quantile_clip must have exactly 2 values")
        quantile_clip = np.asarray(quantile_clip)
        if np.any((quantile_clip < 0) | (quantile_clip > 1)):
            raise ValueError("quantile_clip must be between 0 and 1")

    if cells.shape[1] != empty.shape[1]:  # this should only be possible if data_raw != None
        raise ValueError("data and data_raw have different numbers of proteins")

    if empty_counts_range is None:  # data_raw != None
        warn(
            "empty_counts_range values are not provided, treating all the non-cells as empty droplets"
        )
        empty = empty[~empty.obs_names.isin(cells.obs_names)]
    else:
        warn(
            "empty_counts_range will be deprecated in the future versions",
            DeprecationWarning,
            stacklevel=2,
        )
        if data_raw is not None:
            if not is_mudata(data_raw) or "rna" not in data_raw.mod:
                warn(
                    "data_raw must be a MuData object with 'rna' modality, ignoring empty_counts_range and treating all the non-cells as empty droplets"
                )
                empty = empty[~empty.obs_names.isin(cells.obs_names)]
            else:
                # data_raw is a MuData with 'rna' modality and empty_counts_range values are provided
                be = backend_or_default(backend)
                log10umi = np.log10(_row_sums(data_raw.mod["rna"].X, be) + 1)
                names = data_raw.mod["rna"].obs_names
                empty_droplets = names[
                    (log10umi >= min(*empty_counts_range)) & (log10umi < max(*empty_counts_range))
                ].values

                empty_len_orig = len(empty_droplets)
                empty_droplets = empty_droplets[~pd.Index(empty_droplets).isin(cells.obs_names)]
                empty_len = len(empty_droplets)
                if empty_len != empty_len_orig:
                    warn(
                        f"Dropping {empty_len_orig - empty_len} empty droplets as they are already defined as cells"
                    )
                empty = empty[empty_droplets].copy()

    if data_raw is not None and cell_counts_range is not None:
        warn("cell_counts_range values are ignored since cells are provided in data")

    ctrl_idx = None
    if denoise_counts and isotype_controls is not None:
        ctrl_idx = np.where(cells.var_names.isin(set(isotype_controls)))[0]
        if len(ctrl_idx) < len(isotype_controls):
            warn("Some isotype controls are not present in the data.")

    be = backend_or_default(backend) if be is None else be
    z = _dsb_arrays(cells.X, empty.X, pseudocount=pseudocount, denoise_counts=denoise_counts, ctrl_idx=ctrl_idx,
                    scale_factor=scale_factor, quantile_clipping=quantile_clipping, quantile_clip=quantile_clip,
                    random_state=random_state, backend=be)
    cells_scaled = be.to_host(z).astype(_out_dtype(cells.X), copy=False)

    if add_layer:
        cells.layers["dsb"] = cells_scaled
    else:
        cells.X = cells_scaled
    return toreturn


# ---- clr --------------------------------------------------------------------------------------------------------------
def clr(adata, inplace: bool = True, axis: int = 0, flavor: str = "seurat", *, backend=None):
    """
    Apply the centered log ratio (CLR) transformation
    to normalize counts in adata.X.

    Args:
        data: AnnData object with protein expression counts.
        inplace: Whether to update adata.X inplace.
        axis: Axis across which CLR is performed.
        flavor: How to perform the CLR transformation.

            - seurat: Uses log1p transformations throughout. This results in non-negative values and preserves
                sparse matrices.
            - stoeckius: Adds a pseudocount of 1 before any transformation and uses the standard log transform; can
                yield negative values, the result is always a dense matrix.
            - standard: The standard CLR transform without any pseudocounts. Dense result; infinite values where the
                input contains zeros.

    Signature, checks and write-back follow /root/reference/muon/_prot/preproc.py:227-299.  Differences of layout, not
    of values: for sparse ``seurat`` input the reference converts to CSC (``axis=0``) or CSR (``axis=1``) and warns;
    here a CSR or CSC matrix stays in the format it came in, with its pattern untouched - ``log1p`` of the stored
    values, their row and column sums from the ``row_col_sums`` kernel, then ``v <- log1p(v / exp(sum / n))`` on the
    device - and holds the same matrix as the reference's result (no conversion, hence no warning; other sparse formats
    are converted as the reference does).  Float input keeps its dtype (the arithmetic is f64); integer input, which
    the reference's in-place statements refuse, gives float64.
    """
    if axis not in [0, 1]:
        raise ValueError("Invalid value for `axis` provided. Admissible options are `0` and `1`.")

    if not inplace:
        adata = adata.copy()

    x = adata.X

    if flavor not in ("seurat", "stoeckius", "standard"):
        raise ValueError(f"Unknown flavor `{flavor}`.")
    be = backend_or_default(backend)
    odt = _out_dtype(x)
    n_along = x.shape[axis]
    if flavor == "seurat" and issparse(x):
        if x.format not in ("csr", "csc"):
            if axis == 0:
                warn(
                    "adata.X is sparse but not in CSC format. CSC format required for `axis=0`. Converting to CSC."
                )
                x = x.tocsc()
            else:
                warn(
                    "adata.X is sparse but not in CSR format. CSR format required for `axis=1`. Converting to CSR."
                )
                x = x.tocsr()
        # the three arrays of a CSC matrix are the CSR of its transpose: `major` = the compressed axis
        major = 0 if x.format == "csr" else 1
        shape = (x.shape[major], x.shape[1 - major])
        kw = {"slab_ptr": False} if has(be, "with_slab_ptr") else {}
        X = be.upload_csr(x.indptr, x.indices, x.data, shape, values_dtype=np.float64, **kw)
        lv = torch.log1p(X.values)
        major_sum, minor_sum = be.row_col_sums(DeviceCSR(X.indptr, X.indices, lv, X.shape))
        if axis == major:  # one mean per column of the compressed layout
            g = torch.exp(minor_sum / n_along)[X.indices.long()]
        else:
            g = torch.repeat_interleave(torch.exp(major_sum / n_along), X.indptr[1:] - X.indptr[:-1])
        vals = be.to_host(torch.log1p(X.values / g)).astype(odt, copy=False)
        x = type(x)((vals, x.indices.copy(), x.indptr.copy()), shape=x.shape)
    else:
        if issparse(x):
            x = x.toarray()
        X = be.to_device(np.asarray(x), np.float64)
        if flavor == "seurat":
            out = torch.log1p(X / torch.exp(torch.log1p(X).mean(dim=axis, keepdim=True)))
        else:
            if flavor == "stoeckius":
                X = X + 1
            # scipy.stats.gmean = exp(mean(log(x)))
            out = torch.log(X / torch.exp(torch.log(X).mean(dim=axis, keepdim=True)))
        x = be.to_host(out).astype(odt, copy=False)

    adata.X = x

    return None if inplace else adata
