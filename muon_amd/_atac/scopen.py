"""muon.atac.pp.scopen on MI355X: bounded NMF imputation of the peak matrix, which never leaves CSR.

The reference (/root/reference/muon/_atac/preproc.py:155-236) densifies ``adata.X.T``, binarises it, scales cell c by
``s_c = 1 / (1 - rho_c)`` (lines 199-214) and hands the dense d x n matrix to ``scopen.MF.non_negative_factorization``,
which is derived from scikit-learn's coordinate-descent NMF.  The matrix is ``X[p, c] = s_c [A[c, p] > 0]``: the
binary pattern of the peak matrix ``A`` (n cells x d peaks) with one scale per cell.  Here it stays the device CSR
``A_b`` (the pattern, values 1.0 / 0.0 in f64) and the vector ``s``:

  * solver: ``1/2 |X - W H|^2 + 1/2 l2 (|W|^2 + |H|^2)`` by alternating cyclic coordinate descent, statement for
    statement ``sklearn/decomposition/_nmf.py::_fit_coordinate_descent`` and ``_cdnmf_fast.pyx::_update_cdnmf_fast``
    (no shuffling, l1 = 0): W is d x k, H is k x n (stored as H^T, n x k); an iteration is a W sweep, then an H sweep;
    ``violation`` is the sum of |projected gradient| over both; the loop stops when ``violation / violation_init <= tol``
    or ``violation_init == 0``.  ``l2 = alpha`` on the factors ``regularization`` names - the UNSCALED convention of
    scikit-learn <= 0.24, which scOpen copied;
  * products: with S = diag(s), the W sweep needs ``B = A_b^T (S H^T)`` and ``G = H H^T + l2 I``, the H sweep
    ``B = S (A_b W)`` and ``G = W^T W + l2 I``.  Both products are ``backend.spmm`` on operands made once per call
    (``A_b`` and its ``backend.transpose``, f64 CSR against f64 blocks of the padded width 16 / 32 / 64, padding columns
    zero); the factors live on the device in that padded row-major layout for the whole fit;
  * sweep: ``backend.nmf_cd_sweep`` (csrc/nmf.hip) - one kernel per half-iteration that applies ``s`` to the right-hand
    side, updates the factor in place and leaves what the next half-iteration needs: the Gram matrix of the updated
    factor and, after the H sweep, ``S H^T``.  One half-iteration is one ``spmm``, one ``nmf_cd_sweep`` and k adds on a
    diagonal; the only host traffic per iteration is the violation scalar, which the loop tests;
  * ``_sweep_torch`` is the sweep as tensor operations (k sequential steps of five launches).  It runs where the
    backend has no ``nmf_cd_sweep`` (the CPU operator set of the tests) and for more than ``nmf_max_components()``
    components.

Parity is pinned against scikit-learn's own ``_update_coordinate_descent`` with ``l2_reg_W = l2_reg_H = alpha`` run
under the reference's wrapper (tests/golden/make_scopen_golden.py).  The ``scopen`` package itself is not available
where this was written: parity with ITS ``MF`` module, defaults included, is NOT pinned.

Deviations from the reference:
  * a cell without an open peak (``log10(0)``) and cells that all have the same number of open peaks (0 / 0) give the
    reference a NaN ``rho``, on which its solver fails; both raise ``ValueError`` here;
  * the reference's ``print`` lines are ``logging.getLogger("muon_amd").info`` lines;
  * ``init="nndsvd"`` applies scikit-learn's NNDSVD statements to the top-k singular triplets of the package's own
    truncated SVD (block Lanczos continued in f64), not to a seeded randomised SVD: NNDSVD does not depend on the joint
    sign of a triplet, so the start is deterministic.
"""
from __future__ import annotations

import logging
import numbers
import time
from typing import Optional

import numpy as np
import torch

from .._backend import backend_or_default
from .._containers import modality
from .._hostmatrix import canonical_csr, resident
from .._operators import has

logger = logging.getLogger("muon_amd")

_REGULARIZATION = ("both", "components", "transformation", None)
_IMPUTE_BYTES = 1 << 30  # device temporaries of the imputed matrix's row chunks


def pad_width(k: int) -> int:
    """Columns of the factor blocks: 16 / 32 / 64 (what the SpMM takes), beyond that whole blocks of 64."""
    return 16 if k <= 16 else 32 if k <= 32 else -(-k // 64) * 64


def scales(n_open: np.ndarray, min_rho: float, max_rho: float):
    """``(rho, s)`` of lines 203-214 from the number of open peaks per cell, in f64."""
    n_open = np.asarray(n_open, dtype=np.float64)
    if n_open.size == 0 or n_open.min() <= 0:
        raise ValueError("scopen: a cell has no open peak (log10(0) in the reference's rho); filter empty cells first")
    lg = np.log10(n_open)
    hi, lo = np.max(lg), np.min(lg)
    if hi == lo:
        raise ValueError("scopen: every cell has the same number of open peaks (0 / 0 in the reference's rho)")
    rho = min_rho + (max_rho - min_rho) * (hi - lg) / (hi - lo)
    return rho, 1 / (1 - rho)


# ---- the tensor formulation ---------------------------------------------------------------------------------------------
def _sweep_torch(W, B, G, *, bscale=None, l1: float = 0.0, oscale=None, out=None):
    """What ``HipBackend.nmf_cd_sweep`` computes, as tensor operations: ``W`` updated in place, ``(gram, viol)``."""
    k = int(G.shape[0])
    Wk = W[:, :k]
    b = B[:, :k] * bscale[:, None] if bscale is not None else B[:, :k]
    if l1 != 0.0:
        b = b - l1
    hess = G.diagonal().tolist()
    viol = torch.zeros((1,), dtype=W.dtype, device=W.device)
    for t in range(k):
        wt = Wk[:, t]
        grad = Wk @ G[t] - b[:, t]
        viol += torch.where(wt == 0, torch.clamp(grad, max=0.0), grad).abs().sum()
        if hess[t] != 0.0:
            Wk[:, t] = torch.clamp(wt - grad / hess[t], min=0.0)
    if out is not None:
        out.zero_()
        out[:, :k] = Wk * oscale[:, None] if oscale is not None else Wk
    return Wk.T @ Wk, viol


def _spmm(be, X, Q):
    """``X Q`` for a padded block: one product up to 64 columns, block after block of 64 beyond."""
    if Q.shape[1] <= 64:
        return be.spmm(X, Q)
    return torch.cat([be.spmm(X, Q[:, c:c + 64].contiguous()) for c in range(0, Q.shape[1], 64)], dim=1)


# ---- initialisation -----------------------------------------------------------------------------------------------------
def _nndsvd(U, S, V, eps: float = 1e-6):
    """scikit-learn's ``_initialize_nmf(init="nndsvd")`` after its SVD: U [rows, k], S [k], V [cols, k] (the right
    vectors as columns) -> (W [rows, k], H^T [cols, k]), tensor statements over all components at once."""
    def parts(x):
        return torch.clamp(x, min=0.0), torch.clamp(-x, min=0.0)

    x_p, x_n = parts(U)
    y_p, y_n = parts(V)
    x_p_nrm, y_p_nrm = torch.linalg.norm(x_p, dim=0), torch.linalg.norm(y_p, dim=0)
    x_n_nrm, y_n_nrm = torch.linalg.norm(x_n, dim=0), torch.linalg.norm(y_n, dim=0)
    m_p, m_n = x_p_nrm * y_p_nrm, x_n_nrm * y_n_nrm
    pos = m_p > m_n
    u = torch.where(pos, x_p / x_p_nrm, x_n / x_n_nrm)
    v = torch.where(pos, y_p / y_p_nrm, y_n / y_n_nrm)
    lbd = torch.sqrt(S * torch.where(pos, m_p, m_n))
    W, Ht = lbd * u, lbd * v
    W[:, 0] = torch.sqrt(S[0]) * U[:, 0].abs()
    Ht[:, 0] = torch.sqrt(S[0]) * V[:, 0].abs()
    W[W < eps] = 0
    Ht[Ht < eps] = 0
    return W, Ht


def _init_nndsvd(be, Ab, s, k: int, diagnostics):
    """NNDSVD of ``X = (S A_b)^T`` from the package's truncated SVD of ``S A_b`` (n x d): its left vectors belong to the
    cells (H), its right vectors to the peaks (W)."""
    from .tools import _lsi_device

    n, d = Ab.shape
    if not 1 <= k < min(n, d):
        raise ValueError(f"init='nndsvd' needs n_components < min(n_obs, n_vars) = {min(n, d)}, got {k}")
    rows = torch.repeat_interleave(torch.arange(n, device=s.device), Ab.indptr[1:] - Ab.indptr[:-1])
    SA = Ab.with_values(Ab.values * s[rows])
    U, _stdev, V, info = _lsi_device(be, SA, n_comps=k, scale_embeddings=False, n_obs=n, return_info=True,
                                     refine_f64=True)
    if not info["converged"]:  # (not an error here: a starting point)
        logger.info("scopen: the SVD behind init='nndsvd' had not settled (angle bound %.1e); used as it is",
                    info["angle_bound"])
    if diagnostics is not None:
        diagnostics["svd"] = {"converged": bool(info["converged"]), "angle_bound": float(info["angle_bound"]),
                              "svalues": np.asarray(info["svalues"], dtype=np.float64)}
    S = be.to_device(np.ascontiguousarray(info["svalues"], dtype=np.float64), np.float64)
    return _nndsvd(V.to(torch.float64), S, U.to(torch.float64))


def _init_random(be, n: int, d: int, k: int, mean: float, random_state):
    """scikit-learn's ``init="random"`` statements for X of d samples x n features, drawn on the host."""
    from .._core.ica import _check_random_state

    avg = np.sqrt(mean / k)
    rng = _check_random_state(random_state)
    H = avg * rng.standard_normal(size=(k, n))
    W = avg * rng.standard_normal(size=(d, k))
    np.abs(H, out=H)
    np.abs(W, out=W)
    return be.to_device(W, np.float64), be.to_device(np.ascontiguousarray(H.T), np.float64)


def _init_given(be, init, n: int, d: int, k: int):
    try:
        W0, H0 = init
    except (TypeError, ValueError):
        raise ValueError("init must be 'nndsvd', 'random' or a pair (W0, H0)") from None
    W0, H0 = np.asarray(W0, dtype=np.float64), np.asarray(H0, dtype=np.float64)
    if W0.shape != (d, k):
        raise ValueError(f"init: W0 has shape {W0.shape}, expected {(d, k)}")
    if H0.shape != (k, n):
        raise ValueError(f"init: H0 has shape {H0.shape}, expected {(k, n)}")
    if not (np.isfinite(W0).all() and np.isfinite(H0).all()) or W0.min() < 0 or H0.min() < 0:
        raise ValueError("init: W0 and H0 must be finite and non-negative")
    return be.to_device(W0, np.float64), be.to_device(np.ascontiguousarray(H0.T), np.float64)


# ---- the fit ------------------------------------------------------------------------------------------------------------
def _padded(be, M, kp: int):
    out = be.zeros((int(M.shape[0]), kp), torch.float64)
    out[:, :M.shape[1]] = M
    return out


def _fit(be, Ab, At, s, W, Ht, k: int, *, l2_w: float, l2_h: float, tol: float, max_iter: int, verbose: bool,
         force_tensor: bool = False):
    """``_fit_coordinate_descent`` on padded device factors ``W`` [d, kp] and ``Ht`` [n, kp] (updated in place).
    Returns (n_iter, the violation ratio after every iteration, the route)."""
    kernel = (not force_tensor and has(be, "nmf_cd_sweep", "nmf_max_components") and k <= be.nmf_max_components())
    sweep = be.nmf_cd_sweep if kernel else _sweep_torch
    eye_w = torch.eye(k, dtype=torch.float64, device=W.device) * l2_w
    eye_h = torch.eye(k, dtype=torch.float64, device=W.device) * l2_h
    SHt = Ht * s[:, None]
    gram_h = Ht[:, :k].T @ Ht[:, :k]
    ratios, violation_init, n_iter = [], 0.0, 0
    for n_iter in range(1, max_iter + 1):
        gram_w, v_w = sweep(W, _spmm(be, At, SHt), gram_h + eye_w if l2_w != 0 else gram_h)
        gram_h, v_h = sweep(Ht, _spmm(be, Ab, W), gram_w + eye_h if l2_h != 0 else gram_w, bscale=s, oscale=s, out=SHt)
        violation = float(be.to_host(v_w + v_h)[0])  # the one copy the loop's test needs
        if n_iter == 1:
            violation_init = violation
        if violation_init == 0:
            break
        ratios.append(violation / violation_init)
        if verbose:
            logger.info("scopen: iteration %d, violation: %.6e", n_iter, ratios[-1])
        if ratios[-1] <= tol:
            break
    return n_iter, np.asarray(ratios, dtype=np.float64), "kernel" if kernel else "tensor"


def scopen_device(be, X, k: int, *, max_iter: int = 500, min_rho: float = 0.0, max_rho: float = 0.5, alpha: float = 1.0,
                  tol: float = 1e-4, init="nndsvd", regularization="both", random_state=0, verbose: bool = False,
                  force_tensor: bool = False, diagnostics: Optional[dict] = None):
    """The fit on a device CSR ``X`` (n cells x d peaks, canonical; its values are not modified): returns the padded
    device factors ``W`` [d, kp], ``H^T`` [n, kp] and ``dict(n_iter, ratios, rho, route)``.  ``force_tensor``: the tensor
    formulation of the sweep even where the kernel applies (what the probe compares the kernel with)."""
    n, d = X.shape
    Ab = X.with_values((X.values > 0).to(torch.float64))  # (a new tensor: the resident copy keeps its values)
    n_open, _ = be.row_col_sums(Ab)
    nnz = int(be.to_host(Ab.values.sum().reshape(1))[0])
    rho, s_host = scales(np.rint(be.to_host(n_open)), min_rho, max_rho)
    logger.info("scopen: Number of peaks: %d, Number of cells: %d", d, n)
    logger.info("scopen: Number of non-zeros before imputation: %d", nnz)
    s = be.to_device(s_host, np.float64)
    At = be.transpose(Ab)

    if isinstance(init, str) and init == "nndsvd":
        W0, Ht0 = _init_nndsvd(be, Ab, s, k, diagnostics)
    elif isinstance(init, str):
        W0, Ht0 = _init_random(be, n, d, k, float(np.dot(s_host, be.to_host(n_open))) / (float(n) * float(d)),
                               random_state)
    else:
        W0, Ht0 = _init_given(be, init, n, d, k)
    kp = pad_width(k)
    W, Ht = _padded(be, W0, kp), _padded(be, Ht0, kp)
    del W0, Ht0

    n_iter, ratios, route = _fit(be, Ab, At, s, W, Ht, k, tol=tol, max_iter=max_iter, verbose=verbose,
                                 l2_w=alpha if regularization in ("both", "transformation") else 0.0,
                                 l2_h=alpha if regularization in ("both", "components") else 0.0,
                                 force_tensor=force_tensor)
    info = dict(n_iter=int(n_iter), ratios=ratios, rho=rho, route=route)
    if diagnostics is not None:
        diagnostics.update(info)
    return W, Ht, info


def _impute(be, W, Ht, k: int) -> np.ndarray:
    """``clip(W H, 0, 1)^T`` as a dense f64 [n, d] host array, in row chunks whose device temporary stays under 1 GiB."""
    n, d = int(Ht.shape[0]), int(W.shape[0])
    out = np.empty((n, d), dtype=np.float64)
    Wk = W[:, :k].T.contiguous()
    step = max(1, min(n, _IMPUTE_BYTES // (8 * max(d, 1))))
    for r0 in range(0, n, step):
        chunk = torch.matmul(Ht[r0:r0 + step, :k], Wk)
        out[r0:r0 + step] = be.to_host(chunk.clamp_(0.0, 1.0))
    return out


def scopen(data, n_components: int = 30, max_iter: int = 500, min_rho: float = 0.0, max_rho: float = 0.5, alpha=1,
           verbose: bool = False, *, tol: float = 1e-4, init="nndsvd", regularization="both", random_state=0,
           impute: bool = True, backend=None, diagnostics: Optional[dict] = None):
    """
    Run scOpen (Li et al., 2019, https://doi.org/10.1101/865931) on the count matrix

    ``data``: AnnData with peak counts or MuData with an 'atac' modality.  Argument order, defaults and write-back
    follow /root/reference/muon/_atac/preproc.py:155-236: ``obsm["X_scopen"]`` = H^T (n x k), ``varm["scopen"]`` = W
    (d x k) and, with ``impute=True``, ``adata.X = clip(W H, 0, 1)^T`` as a dense f64 n x d array - the reference's
    contract, and 8 n d bytes of host memory (160 GB at 100 000 x 200 000): ``impute=False`` leaves ``X`` alone.
    Returns None.

    "Open" is ``> 0`` on the matrix as ``toarray()`` gives it: duplicates are summed first; stored zeros, negative
    values and NaN are not open.  A device copy left by ``binarize`` / ``filter_obs`` / ``count_fragments_features`` is
    used as it is (its values are not modified).

    Keyword-only: ``tol`` (the stopping ratio), ``init`` ("nndsvd", "random" with ``random_state``, or a pair
    ``(W0 [d, k], H0 [k, n])``), ``regularization`` ("both", "components" = H, "transformation" = W, None: which
    factors get ``l2 = alpha``), ``diagnostics=dict()`` receives ``n_iter``, ``ratios``, ``rho`` and ``route``.

    Deviations: a cell without an open peak, or cells that all have the same number of open peaks, raise ``ValueError``
    (the reference computes a NaN ``rho`` and fails in its solver); the solver is scikit-learn's coordinate descent with
    the unscaled ``alpha`` of scikit-learn <= 0.24 - parity with the ``scopen`` package itself is not pinned.  See the
    module docstring.
    """
    adata = modality(data, "atac")

    k = n_components
    if isinstance(k, bool) or not isinstance(k, numbers.Integral) or k < 1:
        raise ValueError(f"n_components must be a positive integer, got {n_components!r}")
    k = int(k)
    if isinstance(max_iter, bool) or not isinstance(max_iter, numbers.Integral) or max_iter < 1:
        raise ValueError(f"max_iter must be a positive integer, got {max_iter!r}")
    if not 0 <= min_rho < 1 or not 0 <= max_rho < 1:
        raise ValueError(f"min_rho and max_rho must lie in [0, 1), got {min_rho!r} and {max_rho!r}")
    if not alpha >= 0:
        raise ValueError(f"alpha must be non-negative, got {alpha!r}")
    if not tol >= 0:
        raise ValueError(f"tol must be non-negative, got {tol!r}")
    if regularization not in _REGULARIZATION:
        raise ValueError(f"regularization must be one of {_REGULARIZATION}, got {regularization!r}")
    if isinstance(init, str) and init not in ("nndsvd", "random"):
        raise ValueError(f"init must be 'nndsvd', 'random' or a pair (W0, H0), got {init!r}")

    be = backend_or_default(backend)  # raises without a GPU: there is no CPU path in the package
    import torch.distributed as dist

    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise NotImplementedError("scopen runs on one rank")

    start = time.time()
    X = resident(adata.X, be)
    if X is None:
        host = canonical_csr(adata.X)
        X = be.upload_csr(host.indptr, host.indices, host.data, host.shape)
    W, Ht, info = scopen_device(be, X, k, max_iter=int(max_iter), min_rho=float(min_rho), max_rho=float(max_rho),
                                alpha=float(alpha), tol=float(tol), init=init, regularization=regularization,
                                random_state=random_state, verbose=bool(verbose), diagnostics=diagnostics)
    n_iter, route = info["n_iter"], info["route"]

    adata.obsm["X_scopen"] = be.to_host(Ht[:, :k].contiguous())
    adata.varm["scopen"] = be.to_host(W[:, :k].contiguous())
    if impute:
        adata.X = _impute(be, W, Ht, k)
    secs = time.time() - start
    m, sec = divmod(secs, 60)
    h, m = divmod(m, 60)
    logger.info("scopen: %d iterations (%s sweep), total time: %dh %dm %ds", n_iter, route, h, m, sec)
    return None
