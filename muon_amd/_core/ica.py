"""muon.tl.ica on MI355X: FastICA of an embedding that stays on the device.

The reference (/root/reference/muon/_core/tools.py:1365-1386) runs scikit-learn's ``FastICA`` on ``data.obsm[basis]``
and writes ``obsm["X_ica"]``.  Here the same statements (scikit-learn 1.7, ``sklearn/decomposition/_fastica.py``) are
split between the device, which touches everything n x k, and the host, which touches everything k x k:

  * whitening: column means and the centred Gram matrix ``Xc^T Xc`` (f x f, f64) on the device; ``eigh``, the descending
    sort, ``u *= sign(u[0])`` and ``K = (u / d).T[:k]`` on the host; ``Z = Xc K^T sqrt(n)`` a new row-major f64 tensor
    [n, kp] on the device, kp = k rounded up to 16, padding columns zero (scikit-learn's ``X1.T``);
  * one iteration of the parallel algorithm: ``(A, gp) = backend.ica_sweep(Z, W, fun, alpha)`` with ``A = g(Z W^T)^T Z``
    and ``gp = column sums of g'(Z W^T)`` - one fused kernel that reads Z once (csrc/ica.hip) - then, on the host in
    numpy f64, ``_sym_decorrelation`` of ``A / n - (gp / n)[:, None] W`` statement for statement and the convergence
    measure ``lim``.  One small device-to-host copy per iteration is inherent: the loop tests ``lim``;
  * finish: ``S = Z W^T / sqrt(n)``, the division by ``std(S, axis=0)`` for ``whiten="unit-variance"``, the optional
    ``scale``.

``_sweep_torch`` is the sweep as tensor operations (three passes over n x k, an n x k temporary).  It runs where the
backend has no ``ica_sweep`` (the CPU operator set of the tests) and for more than ``ica_max_components()`` components;
``algorithm="deflation"`` is a tensor formulation of ``_ica_def`` (no kernel).

Precision policy: all arithmetic is f64 whatever the dtype of the basis.  A float32 basis is widened exactly and
``X_ica`` comes back as float32, rounded once at the end.  scikit-learn runs everything in float32 for such a basis;
its result then differs from its own float64 run (by 1.8e-5 on the ``k6`` data of the fixture, max |S| 7.9) - the
package returns the float64 answer.

Whitening always goes through the f64 Gram matrix, for ``whiten_solver="svd"`` too: on a basis of full column rank the
two agree with scikit-learn's SVD to rounding; on a rank-deficient basis (eigenvalues below ``10 eps``, clamped to
``eps`` with scikit-learn's warning for either solver) they differ from it, as scikit-learn's own ``"eigh"`` does.
"""
from __future__ import annotations

import numbers
from typing import Optional
from warnings import warn

import numpy as np
import torch
from scipy import linalg

from .._backend import backend_or_default
from .._operators import has

_FUNS = ("logcosh", "exp", "cube")


class ConvergenceWarning(UserWarning):
    """FastICA reached ``max_iter`` (scikit-learn's warning of the same name; defined here because scikit-learn need
    not be installed where the package runs)."""


def _check_random_state(seed):
    """sklearn.utils.check_random_state."""
    if seed is None or seed is np.random:
        return np.random.mtrand._rand
    if isinstance(seed, numbers.Integral):
        return np.random.RandomState(int(seed))
    if isinstance(seed, np.random.RandomState):
        return seed
    raise ValueError(f"{seed!r} cannot be used to seed a numpy.random.RandomState instance")


def _validate(n_components, algorithm, whiten, fun, fun_args, max_iter, tol, whiten_solver):
    """FastICA._parameter_constraints of scikit-learn 1.7, with its messages."""
    def bad(name, what, got):
        return ValueError(f"The {name!r} parameter of FastICA must be {what}. Got {got!r} instead.")

    if n_components is not None and (isinstance(n_components, bool) or not isinstance(n_components, numbers.Integral)
                                     or n_components < 1):
        raise bad("n_components", "an int in the range [1, inf) or None", n_components)
    if algorithm not in ("parallel", "deflation"):
        raise bad("algorithm", "a str among {'deflation', 'parallel'}", algorithm)
    if not (whiten is False or (isinstance(whiten, str) and whiten in ("arbitrary-variance", "unit-variance"))):
        raise bad("whiten", "a str among {'arbitrary-variance', 'unit-variance'} or a bool among {False}", whiten)
    if callable(fun):
        raise NotImplementedError("muon_amd.tl.ica: a callable `fun` cannot run on the device; the built-in "
                                  "contrast functions are 'logcosh', 'exp' and 'cube'")
    if fun not in _FUNS:
        raise bad("fun", "a str among {'cube', 'exp', 'logcosh'} or a callable", fun)
    if fun_args is not None and not isinstance(fun_args, dict):
        raise bad("fun_args", "an instance of 'dict' or None", fun_args)
    if isinstance(max_iter, bool) or not isinstance(max_iter, numbers.Integral) or max_iter < 1:
        raise bad("max_iter", "an int in the range [1, inf)", max_iter)
    if isinstance(tol, bool) or not isinstance(tol, numbers.Real) or not tol >= 0:
        raise bad("tol", "a float in the range [0.0, inf)", tol)
    if whiten_solver not in ("eigh", "svd"):
        raise bad("whiten_solver", "a str among {'eigh', 'svd'}", whiten_solver)


# ---- the k x k statements, on the host ----------------------------------------------------------------------------------
def _sym_decorrelation(W: np.ndarray) -> np.ndarray:
    """W <- (W W^T)^-1/2 W, as scikit-learn states it."""
    s, u = linalg.eigh(np.dot(W, W.T))
    s = np.clip(s, a_min=np.finfo(W.dtype).tiny, a_max=None)
    return np.linalg.multi_dot([u * (1.0 / np.sqrt(s)), u.T, W])


# ---- the tensor formulation ---------------------------------------------------------------------------------------------
def _g_torch(y: torch.Tensor, fun: str, alpha: float):
    if fun == "logcosh":
        t = torch.tanh(alpha * y)
        return t, alpha * (1.0 - t * t)
    if fun == "exp":
        e = torch.exp(-(y * y) / 2)
        return y * e, (1.0 - y * y) * e
    return y * y * y, 3.0 * (y * y)


def _sweep_torch(Z: torch.Tensor, W: torch.Tensor, fun: str, alpha: float = 1.0):
    """What ``HipBackend.ica_sweep`` computes, as tensor operations."""
    k = W.shape[0]
    Zk = Z[:, :k]
    g, gp = _g_torch(Zk @ W.T, fun, alpha)
    return g.T @ Zk, gp.sum(dim=0)


def _deflation_torch(be, Z, w_init: np.ndarray, fun: str, alpha: float, tol: float, max_iter: int):
    """scikit-learn's ``_ica_def`` with the n-long statements on the device; returns (W, max n_iter, last lim)."""
    k = w_init.shape[0]
    Zk = Z[:, :k]
    W = torch.zeros((k, k), dtype=torch.float64, device=Z.device)
    n_iter, lim = [], float("nan")
    for j in range(k):
        w = be.to_device(np.ascontiguousarray(w_init[j]), np.float64)
        w = w / torch.sqrt((w ** 2).sum())
        for i in range(max_iter):
            g, gp = _g_torch(Zk @ w, fun, alpha)
            w1 = (Zk * g[:, None]).mean(dim=0) - gp.mean() * w
            w1 = w1 - (w1 @ W[:j].T) @ W[:j]
            w1 = w1 / torch.sqrt((w1 ** 2).sum())
            lim = abs(abs(float((w1 * w).sum().item())) - 1)
            w = w1
            if lim < tol:
                break
        n_iter.append(i + 1)
        W[j] = w
    return be.to_host(W), max(n_iter), lim


# ---- FastICA.fit_transform ----------------------------------------------------------------------------------------------
def _fastica_arrays(X, n_components=None, *, random_state=None, algorithm="parallel", whiten="unit-variance",
                    fun="logcosh", fun_args=None, max_iter=200, tol=1e-4, w_init=None, whiten_solver="svd",
                    backend=None, force_tensor=False, diagnostics: Optional[dict] = None) -> torch.Tensor:
    """``FastICA(...).fit_transform(X)`` as an [n, k] f64 tensor on the backend's device.  ``force_tensor``: the tensor
    formulation of the sweep even where the kernel applies (what tests and the probe compare the kernel with).
    ``diagnostics``: a dict that receives ``n_iter``, ``components_``, ``mean_``, ``whitening_``, the last ``lim`` and
    the whole ``lim_history`` (host values)."""
    _validate(n_components, algorithm, whiten, fun, fun_args, max_iter, tol, whiten_solver)
    be = backend_or_default(backend)
    fun_args = {} if fun_args is None else fun_args
    rs = _check_random_state(random_state)
    alpha = fun_args.get("alpha", 1.0)
    if not 1 <= alpha <= 2:
        raise ValueError("alpha must be in [1,2]")

    if isinstance(X, torch.Tensor):
        Xd = X.to(torch.float64)
        if Xd.dim() != 2:
            raise ValueError(f"Expected 2D array, got {Xd.dim()}D array instead")
        if not bool(torch.isfinite(Xd).all()):
            raise ValueError("Input X contains NaN or infinity.")
    else:
        Xh = np.asarray(X)
        if Xh.ndim != 2:
            raise ValueError(f"Expected 2D array, got {Xh.ndim}D array instead")
        if Xh.dtype not in (np.float32, np.float64):
            Xh = Xh.astype(np.float64)
        if np.isnan(Xh).any():
            raise ValueError("Input X contains NaN.")
        if not np.isfinite(Xh).all():
            raise ValueError(f"Input X contains infinity or a value too large for dtype({Xh.dtype.name!r}).")
        Xd = be.to_device(Xh, Xh.dtype).to(torch.float64)  # (a float32 basis travels as float32, widened exactly)
    n, f = (int(s) for s in Xd.shape)
    if n < 2:
        raise ValueError(f"Found array with {n} sample(s) (shape=({n}, {f})) while a minimum of 2 is required by FastICA.")

    k = n_components
    if not whiten and k is not None:
        k = None
        warn("Ignoring n_components with whiten=False.")
    if k is None:
        k = min(n, f)
    if k > min(n, f):
        k = min(n, f)
        warn("n_components is too large: it will be set to %s" % k)
    if not whiten and k != f:
        raise ValueError(f"whiten=False needs at least as many samples as features, got {n} samples and {f} features")
    kp = (k + 15) // 16 * 16

    K = mean = None
    Z = torch.zeros((n, kp), dtype=torch.float64, device=Xd.device)
    if whiten:
        mean = Xd.mean(dim=0)
        Xc = Xd - mean
        d, u = linalg.eigh(be.to_host(Xc.T @ Xc))
        sort_indices = np.argsort(d)[::-1]
        eps = np.finfo(d.dtype).eps * 10
        degenerate_idx = d < eps
        if np.any(degenerate_idx):
            warn("There are some small singular values, using whiten_solver = 'svd' might lead to more accurate results."
                 if whiten_solver == "eigh" else
                 "There are some small singular values: the basis is rank deficient and the whitening, which goes "
                 "through the Gram matrix, differs from scikit-learn's SVD there.")
        d[degenerate_idx] = eps  # For numerical issues
        np.sqrt(d, out=d)
        d, u = d[sort_indices], u[:, sort_indices]
        u *= np.sign(u[0])
        K = np.ascontiguousarray((u / d).T[:k])
        Z[:, :k] = (Xc @ be.to_device(K, np.float64).T) * float(np.sqrt(n))
        del Xc
    else:
        Z[:, :k] = Xd
    del Xd

    if w_init is None:
        w_init = np.asarray(rs.normal(size=(k, k)), dtype=np.float64)
    else:
        w_init = np.asarray(w_init)
        if w_init.shape != (k, k):
            raise ValueError("w_init has invalid shape -- should be %(shape)s" % {"shape": (k, k)})
        w_init = w_init.astype(np.float64)

    lims = []
    if algorithm == "parallel":
        kernel = (not force_tensor and has(be, "ica_sweep", "ica_max_components")
                  and k <= be.ica_max_components())
        W = _sym_decorrelation(w_init)
        p_ = float(n)
        for ii in range(max_iter):
            Wd = be.to_device(np.ascontiguousarray(W), np.float64)
            A, gp = be.ica_sweep(Z, Wd, fun, alpha) if kernel else _sweep_torch(Z, Wd, fun, alpha)
            host = be.to_host(torch.cat([A.reshape(-1), gp]))  # the one copy the loop's test needs
            A, g_wtx = host[:k * k].reshape(k, k), host[k * k:] / p_
            W1 = _sym_decorrelation(A / p_ - g_wtx[:, np.newaxis] * W)
            lim = max(abs(abs(np.einsum("ij,ij->i", W1, W)) - 1))
            lims.append(float(lim))
            W = W1
            if lim < tol:
                break
        else:
            warn("FastICA did not converge. Consider increasing tolerance or the maximum number of iterations.",
                 ConvergenceWarning)
        n_iter = ii + 1
    else:
        W, n_iter, lim = _deflation_torch(be, Z, w_init, fun, alpha, tol, max_iter)
        lims.append(float(lim))

    S = Z[:, :k] @ be.to_device(np.ascontiguousarray(W), np.float64).T
    if whiten:
        S = S / float(np.sqrt(n))
        if whiten == "unit-variance":
            S_std = S.std(dim=0, unbiased=False, keepdim=True)
            S = S / S_std
            W = W / be.to_host(S_std).T
    if diagnostics is not None:
        diagnostics.update(n_iter=int(n_iter), lim=lims[-1], lim_history=np.asarray(lims),
                           components_=np.dot(W, K) if whiten else W, unmixing_=W,
                           mean_=be.to_host(mean) if whiten else None, whitening_=K)
    return S


def ica(data, basis="X_pca", n_components=None, *, random_state=None, scale=False, copy=False, backend=None, **kwargs):
    """Run Independent component analysis

    ``data``: AnnData or MuData; FastICA of ``data.obsm[basis]`` goes to ``data.obsm["X_ica"]`` (``copy=True``: to a
    copy, which is returned; ``data`` stays untouched).  ``scale=True`` divides the columns by ``std(axis=0)``.
    Argument order, defaults and write-back follow /root/reference/muon/_core/tools.py:1365-1386; ``**kwargs`` are
    ``FastICA``'s constructor arguments with scikit-learn 1.7's defaults and checks: ``algorithm``, ``whiten``, ``fun``
    ('logcosh', 'exp', 'cube'; a callable raises ``NotImplementedError``), ``fun_args``, ``max_iter``, ``tol``,
    ``w_init``, ``whiten_solver``.  An integer ``random_state`` draws the same ``w_init`` as scikit-learn.  A run that
    reaches ``max_iter`` warns with ``muon_amd.tl.ConvergenceWarning`` and still returns its result.
    ``diagnostics=dict()`` receives ``n_iter``, ``components_``, ``mean_``, ``whitening_`` and the last ``lim``.

    Precision: all arithmetic is f64 whatever the dtype of the basis; a float32 basis is widened exactly and ``X_ica``
    comes back as float32, rounded once (scikit-learn computes in float32 there; its result differs from its own float64
    run, by 1.8e-5 on the fixture's ``k6`` data).  Whitening goes through the f64 Gram matrix for both values of ``whiten_solver``: on a
    rank-deficient basis this differs from scikit-learn's SVD (and warns).  See the module docstring for where each
    statement runs.
    """
    be = backend_or_default(backend)
    X = data.obsm[basis]
    if isinstance(X, torch.Tensor):
        dt = np.dtype(np.float32) if X.dtype == torch.float32 else np.dtype(np.float64)
    else:
        dt = np.dtype(getattr(X, "dtype", np.float64))
    odt = dt if dt in (np.float32, np.float64) else np.dtype(np.float64)
    S = _fastica_arrays(X, n_components, random_state=random_state, backend=be, **kwargs)
    if scale:
        S = S / S.std(dim=0, unbiased=False)
    x_ica = be.to_host(S).astype(odt, copy=False)

    data = data.copy() if copy else data
    data.obsm["X_ica"] = x_ica
    return data if copy else None
