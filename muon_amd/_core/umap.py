"""muon.tl.umap on MI355X: the UMAP layout of the multimodal neighbourhood graph.

The reference (/root/reference/muon/_core/tools.py:1209-1362) builds an AnnData around ``mdata.obsp`` and hands it to
scanpy's ``tl.umap``, which hands the connectivities to umap-learn's ``simplicial_set_embedding``.  scanpy and umap-learn
are third-party and absent here.  The wrapper's behaviour (the neighbours key, the graph's slot, the keyword arguments
handed on, the write-back, ``copy``, the error text) is the reference's and is pinned by a record of its own ``umap``
executing (tests/golden/umap_golden.npz).  The optimiser below is this module's own and is stated here in full
(tests/umap_refs.py restates it per vertex and per entry).  Parity with umap-learn's coordinates is NOT pinned: its
layout loop is hogwild SGD, seeded but not repeatable across thread counts even upstream.

Deviation: the reference concatenates the modalities' representations into a data matrix (:1310-1334).  scanpy uses
that matrix only to place the components of a disconnected graph under the spectral initialisation, and the
reference's imputation line ``rep[~idx, nfeatures : crep.shape[1]] = imputed`` slices wrongly for every modality after
the first.  The initialisation below needs no data matrix, so none is built.

Parameters.  ``n_epochs`` = ``maxiter``, or 500 for n <= 10 000 and 200 above (umap-learn's rule).  ``a`` / ``b``: given,
or umap-learn's ``find_ab_params``: ``scipy.optimize.curve_fit`` of 1 / (1 + a x^(2b)) to the 300 points x =
linspace(0, 3 spread), y = 1 where x < min_dist, else exp(-(x - min_dist) / spread).

Edges.  The stored entries (v, u, w) of the connectivities as a CSR sorted by (row, column), duplicates summed.  With
w_max the largest value, entries with w <= 0 or w < w_max / n_epochs are dropped; an entry's period is eps = w_max / w
>= 1 epochs, kept as the integer E = rint(eps 2^16) (int64).  The entry index j below is the entry's position among the
kept ones.  The schedule is a pure function of (entry, epoch e = 1 .. n_epochs), in integers, S = 2^16:

    c(e) = floor(e S / E)                      activations through epoch e
    active at e  iff  c(e) > c(e - 1)          (equivalently (e S) mod E < S, since E >= S)
    m(e) = floor(e S rate / E)                 negatives due through epoch e, rate = negative_sample_rate
    an activation at e draws m(e) - m(p) negatives, p = ceil((c(e) - 1) E / S) the previous activation epoch
    (p = 0 and m(0) = 0 at the first activation)

One epoch is a Jacobi step, all f64: every force is evaluated on the snapshot Y_t, then Y_{t+1} = Y_t + alpha_e F with
alpha_e = alpha (1 - (e - 1) / n_epochs); two buffers, ping-pong.  With d2 = |y_v - y_x|^2 added in coordinate order,
d2^b ONE ``pow(d2, b)`` and d2^(b-1) that value divided by d2, clip(.) to [-4, 4] per coordinate:

  * attraction: an active entry (v, u) adds to F_v only  clip(-2ab d2^(b-1) / (1 + a d2^b) (y_v - y_u)), nothing when
    d2 == 0 (umap-learn's ``move_other=False``; on the symmetric graphs pp.neighbors writes, the mirrored entry moves u
    in the same epoch);
  * repulsion: each of the entry's negatives s = 0, 1, ... adds  clip(2 gamma b / ((0.001 + d2)(1 + a d2^b)) (y_v -
    y_k)), nothing when k == v or d2 == 0;
  * the negative's index: h = splitmix64(splitmix64(splitmix64(seed + e) ^ j) + s) in arithmetic modulo 2^64
    (``splitmix64``: csrc/common.hpp), k = ((h >> 32) n) >> 32; seed = random_state modulo 2^64;
  * the order of F_v's sum: sixteen lanes; lane g adds the row's entries g, g + 16, ... in order, for an entry its
    attraction and then its negatives in order; then the lanes' sums are added by the xor butterfly over the offsets
    8, 4, 2, 1 (lane g takes g ^ off's).  A vertex without an active entry keeps its coordinates (F = 0).

Initialisation, then for every kind a rescaling per coordinate to [0, 10] (10 (y - min) / (max - min); a constant
coordinate becomes 0), as umap-learn does.  ``rng = np.random.default_rng(random_state)``:

  * "random": ``rng.uniform(-10, 10, (n, n_components))``;
  * an array [n, n_components], or the name of an ``.obsm`` key holding one;
  * "spectral": with m = n_components + 1 + SPECTRAL_OVERSAMPLE columns (n <= m: the random one instead), A the kept
    entries' weights, D its row sums (1 / sqrt(D) := 0 for an empty row), M = D^(-1/2) A D^(-1/2): Q = qr(
    rng.standard_normal((n, m))), then SPECTRAL_STEPS times Q = qr((Q + M Q) / 2) (orthogonal iteration: the sparse
    product is a gather and the fixed-order segmented sum, the QR numpy's on the host), then one Rayleigh-Ritz step:
    H = Q^T (Q + M Q) / 2, symmetrised, ``numpy.linalg.eigh``, Ritz vectors by decreasing value; the leading one is
    dropped, the next n_components are kept, each signed so that its entry of largest magnitude (the first of them) is
    positive; scaled to max |coordinate| = 10 (an all-zero result is left), plus ``rng.normal(0, 1e-4, (n,
    n_components))``.  A disconnected graph needs nothing extra: its components span the eigenvalue-1 space.

Two formulations of an epoch:

  * the kernel (csrc/umap.hip ``k_umap_epoch`` through ``HipBackend.umap_epoch``): sixteen lanes per vertex, one launch
    per epoch on the backend's stream, no host synchronisation between epochs;
  * the tensor formulation (``_epoch_tensor``): active mask, forces over the entries and their negatives, one segmented
    sum per row (``cluster_segsum`` on a device, ``index_add_`` on the CPU operator set - never a device's
    ``index_add_``, which adds with atomics).  It runs where the backend has no ``umap_*`` methods (the CPU operator set
    of the tests), for ``n_components`` above ``umap_max_components()`` (or 1), and for n >= 2^31.  It adds a row's terms
    in another order than the kernel (its attractions, then its negatives, each in entry order): the two agree to
    rounding.

Repeats are byte-equal within a formulation.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch
from scipy.sparse import csr_matrix

from .._backend import backend_or_default
from .._containers import is_anndata, is_mudata
from .._operators import has
from .cluster import _ptr_of_counts, _segsum

_KERNEL_METHODS = ("umap_epoch", "umap_max_components")
SHIFT = 16  # the schedule's fixed point: E = rint(period 2^16)
SPECTRAL_STEPS = 40  # the other eigenvalues of (I + M) / 2 on a clique are below 1/2: 2^-40 of them is left
SPECTRAL_OVERSAMPLE = 4
_M64 = (1 << 64) - 1


# ---- parameters ---------------------------------------------------------------------------------------------------------------
def find_ab(spread: float, min_dist: float):
    """umap-learn's ``find_ab_params`` (module docstring)."""
    from scipy.optimize import curve_fit

    def curve(x, a, b):
        return 1.0 / (1.0 + a * x ** (2 * b))

    xv = np.linspace(0, spread * 3, 300)
    yv = np.zeros(xv.shape)
    yv[xv < min_dist] = 1.0
    yv[xv >= min_dist] = np.exp(-(xv[xv >= min_dist] - min_dist) / spread)
    params, _ = curve_fit(curve, xv, yv)
    return float(params[0]), float(params[1])


def default_epochs(n: int) -> int:
    return 500 if n <= 10000 else 200


# ---- the graph ----------------------------------------------------------------------------------------------------------------
class _Graph:
    """The kept entries as a CSR sorted by (row, column): rows / cols64 / cols (int32) / w / E per entry, indptr."""

    def __init__(self, be, n: int, rows, cols, w, E):
        self.n = int(n)
        self.rows = be.to_device(np.ascontiguousarray(rows, dtype=np.int64), np.int64)
        self.cols64 = be.to_device(np.ascontiguousarray(cols, dtype=np.int64), np.int64)
        self.cols = self.cols64.to(torch.int32)
        self.w = be.to_device(np.ascontiguousarray(w, dtype=np.float64), np.float64)
        self.E = be.to_device(np.ascontiguousarray(E, dtype=np.int64), np.int64)
        self.indptr = be.to_device(np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=self.n))]), np.int64)


def edges(connectivities, n_epochs: int):
    """``(rows, cols, w, E)`` of the kept entries (module docstring, "Edges"), host arrays."""
    A = csr_matrix(connectivities)
    if A.shape[0] != A.shape[1]:
        raise ValueError("the graph must be square")
    A = A.astype(np.float64)
    A.sum_duplicates()
    A.sort_indices()
    coo = A.tocoo()
    r, c, w = coo.row.astype(np.int64), coo.col.astype(np.int64), coo.data
    if w.size == 0 or not (w.max() > 0):
        z = np.zeros(0, dtype=np.int64)
        return z, z, np.zeros(0), z
    w_max = float(w.max())
    keep = (w > 0) & (w >= w_max / n_epochs)
    r, c, w = r[keep], c[keep], w[keep]
    E = np.rint((w_max / w) * float(1 << SHIFT)).astype(np.int64)
    return r, c, w, E


# ---- the tensor formulation -----------------------------------------------------------------------------------------------------
def _i64(x: int) -> int:
    """The value modulo 2^64 as the int64 of the same bits."""
    x &= _M64
    return x - (1 << 64) if x >= (1 << 63) else x


def _lsr(x: torch.Tensor, k: int) -> torch.Tensor:
    return (x >> k) & ((1 << (64 - k)) - 1)  # (int64's >> carries the sign in: masked off)


def _splitmix64(x: torch.Tensor) -> torch.Tensor:
    """csrc/common.hpp's ``splitmix64`` on the bits of an int64 tensor (the products and sums wrap)."""
    x = x + _i64(0x9E3779B97F4A7C15)
    x = (x ^ _lsr(x, 30)) * _i64(0xBF58476D1CE4E5B9)
    x = (x ^ _lsr(x, 27)) * _i64(0x94D049BB133111EB)
    return x ^ _lsr(x, 31)


def _splitmix64_int(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def _force(diff, b, coef_of):
    """clip(coef_of(d2, d2^b) diff) per row, 0 where d2 == 0."""
    d2 = diff[:, 0] * diff[:, 0]
    for d in range(1, int(diff.shape[1])):
        d2 = d2 + diff[:, d] * diff[:, d]
    pw = torch.pow(d2, b)
    coef = torch.where(d2 > 0, coef_of(d2, pw), torch.zeros_like(d2))
    return torch.clamp(coef[:, None] * diff, -4.0, 4.0)


def _epoch_tensor(be, g: _Graph, Y, e: int, n_epochs: int, rate: int, a, b, gamma, alpha_e, seed: int):
    """Y_{t+1} of the module docstring from Y = Y_t [n, dim] f64."""
    S = 1 << SHIFT
    n, dim = g.n, int(Y.shape[1])
    t = torch.full_like(g.E, e * S)
    c = torch.div(t, g.E, rounding_mode="floor")
    idx = torch.nonzero(t - c * g.E < S).reshape(-1)
    Ea, ca = g.E[idx], c[idx]
    p = torch.div((ca - 1) * Ea + (S - 1), S, rounding_mode="floor")
    nneg = torch.div(t[idx] * rate, Ea, rounding_mode="floor") - torch.div(p * (S * rate), Ea, rounding_mode="floor")
    rows_a = g.rows[idx]
    if int(rows_a.numel()) == 0:
        return Y.clone()
    fa = _force(Y[rows_a] - Y[g.cols64[idx]], b, lambda d2, pw: (-2.0 * a * b * (pw / d2)) / (1.0 + a * pw))
    ent = torch.repeat_interleave(idx, nneg)
    first = torch.cumsum(nneg, dim=0) - nneg
    s = torch.arange(int(ent.numel()), dtype=torch.int64, device=Y.device) - torch.repeat_interleave(first, nneg)
    h = _splitmix64(_splitmix64(_i64(_splitmix64_int((seed + e) & _M64)) ^ ent) + s)
    k = (_lsr(h, 32) * n) >> 32
    rows_r = g.rows[ent]
    fr = _force(Y[rows_r] - Y[k], b, lambda d2, pw: (2.0 * gamma * b) / ((0.001 + d2) * (1.0 + a * pw)))
    fr = torch.where((k != rows_r)[:, None], fr, torch.zeros_like(fr))
    # a row's terms side by side: its attractions, then its negatives, each in entry order (both lists are sorted by row)
    na, nr = torch.bincount(rows_a, minlength=n), torch.bincount(rows_r, minlength=n)
    ptr = _ptr_of_counts(na + nr)
    pos_a = ptr[rows_a] + torch.arange(int(rows_a.numel()), device=Y.device) - (torch.cumsum(na, dim=0) - na)[rows_a]
    pos_r = (ptr[rows_r] + na[rows_r] + torch.arange(int(rows_r.numel()), device=Y.device)
             - (torch.cumsum(nr, dim=0) - nr)[rows_r])
    terms = torch.empty((int(rows_a.numel() + rows_r.numel()), dim), dtype=torch.float64, device=Y.device)
    terms[pos_a] = fa
    terms[pos_r] = fr
    F = _segsum(be, terms, ptr)
    return Y + alpha_e * F


# ---- initialisation -------------------------------------------------------------------------------------------------------------
def rescale(Y: np.ndarray) -> np.ndarray:
    """Per coordinate to [0, 10]; a constant coordinate becomes 0."""
    Y = np.asarray(Y, dtype=np.float64)
    if Y.shape[0] == 0:
        return Y.copy()
    lo, hi = Y.min(axis=0), Y.max(axis=0)
    span = np.where(hi > lo, hi - lo, 1.0)
    return 10.0 * (Y - lo) / span


def spectral_init(be, g: _Graph, dim: int, rng, noise: bool = True) -> np.ndarray:
    """The "spectral" initialisation of the module docstring, before the rescaling (host f64 [n, dim])."""
    n = g.n
    m = dim + 1 + SPECTRAL_OVERSAMPLE
    if n <= m:
        return rng.uniform(-10, 10, (n, dim))
    deg = _segsum(be, g.w.reshape(-1, 1), g.indptr)[:, 0]
    dinv = torch.where(deg > 0, 1.0 / torch.sqrt(deg), torch.zeros_like(deg))
    mw = (dinv[g.rows] * g.w * dinv[g.cols64]).reshape(-1, 1)
    has_entries = int(g.w.numel()) > 0

    def op(Qh: np.ndarray) -> np.ndarray:
        Q = be.to_device(np.ascontiguousarray(Qh), np.float64)
        MQ = _segsum(be, (mw * Q[g.cols64]).contiguous(), g.indptr) if has_entries else torch.zeros_like(Q)
        return be.to_host((Q + MQ) / 2)

    Q = np.linalg.qr(rng.standard_normal((n, m)))[0]
    for _ in range(SPECTRAL_STEPS):
        Q = np.linalg.qr(op(Q))[0]
    H = Q.T @ op(Q)
    vals, vecs = np.linalg.eigh((H + H.T) / 2)
    V = Q @ vecs[:, ::-1][:, 1:dim + 1]
    for d in range(dim):
        if V[np.argmax(np.abs(V[:, d])), d] < 0:
            V[:, d] = -V[:, d]
    top = np.abs(V).max()
    if top > 0:
        V = V * (10.0 / top)
    if noise:
        V = V + rng.normal(0.0, 1e-4, (n, dim))
    return V


def initial_positions(be, g: _Graph, init_pos, dim: int, random_state, obsm=None) -> np.ndarray:
    """The rescaled initial coordinates (host f64 [n, dim])."""
    n = g.n
    rng = np.random.default_rng(random_state)
    if isinstance(init_pos, str):
        if init_pos == "paga":
            raise NotImplementedError("muon_amd.tl.umap: init_pos='paga' is not implemented")
        if init_pos == "random":
            Y = rng.uniform(-10, 10, (n, dim))
        elif init_pos == "spectral":
            Y = spectral_init(be, g, dim, rng)
        elif obsm is not None and init_pos in obsm:
            Y = np.asarray(obsm[init_pos], dtype=np.float64)
        else:
            raise ValueError(f"init_pos: 'spectral', 'random', an array or a key of .obsm, not {init_pos!r}")
    else:
        Y = np.asarray(init_pos, dtype=np.float64)
    if Y.shape != (n, dim):
        raise ValueError(f"init_pos has shape {tuple(Y.shape)}, expected ({n}, {dim})")
    if not np.isfinite(Y).all():
        raise ValueError("init_pos must be finite")
    return rescale(Y)


# ---- the layout -------------------------------------------------------------------------------------------------------------------
def layout(be, g: _Graph, Y0: np.ndarray, n_epochs: int, alpha: float, gamma: float, rate: int, a: float, b: float,
           seed: int, diagnostics: Optional[dict] = None, first_epoch: int = 1, last_epoch: Optional[int] = None):
    """The epochs ``first_epoch .. last_epoch`` (default: all) from Y0; the result as a device f64 tensor [n, dim]."""
    n, dim = g.n, int(Y0.shape[1])
    kernel = (has(be, *_KERNEL_METHODS) and 2 <= dim <= be.umap_max_components() and n < (1 << 31))
    if diagnostics is not None:
        diagnostics["path"] = "kernel" if kernel else "tensor"
        diagnostics["n_epochs"] = n_epochs
        diagnostics["entries"] = int(g.E.numel())
    Y = be.to_device(np.ascontiguousarray(Y0, dtype=np.float64), np.float64)
    if n == 0 or dim == 0:
        return Y
    other = be.empty((n, dim), torch.float64) if kernel else None
    for e in range(first_epoch, (n_epochs if last_epoch is None else last_epoch) + 1):
        alpha_e = alpha * (1.0 - (e - 1) / n_epochs)
        if kernel:
            be.umap_epoch(g.indptr, g.cols, g.E, e, n_epochs, rate, a, b, gamma, alpha_e, seed, Y, other)
            Y, other = other, Y
        else:
            Y = _epoch_tensor(be, g, Y, e, n_epochs, rate, a, b, gamma, alpha_e, seed)
    return Y


# ---- the interface ----------------------------------------------------------------------------------------------------------------
def umap(mdata, min_dist: float = 0.5, spread: float = 1.0, n_components: int = 2, maxiter: Optional[int] = None,
         alpha: float = 1.0, gamma: float = 1.0, negative_sample_rate: int = 5, init_pos="spectral", random_state=42,
         a: Optional[float] = None, b: Optional[float] = None, copy: bool = False, method: str = "umap",
         neighbors_key: Optional[str] = None, *, backend=None, diagnostics: Optional[dict] = None):
    """Embed the multimodal neighbourhood graph with the layout of the module docstring (reference :1209-1362).

    ``mdata``: a MuData after ``pp.neighbors`` - or an AnnData, which the reference forwards to scanpy; here the same
    code runs on its ``.obsp``.  ``neighbors_key=None`` means ``"neighbors"``; the graph is
    ``.obsp[.uns[neighbors_key]["connectivities_key"]]``.  ``maxiter``: the epochs (None: 500 for n <= 10 000, else
    200); ``a`` / ``b``: None fits them to ``min_dist`` / ``spread``; ``init_pos``: "spectral", "random", an array
    [n, n_components] or the name of an ``.obsm`` key (scanpy's "paga" is not implemented); ``random_state``: an integer
    or None; ``method="rapids"`` is not implemented.

    Writes ``.obsm["X_umap"]`` (float32 [n, n_components], the f64 result rounded once) and ``.uns["umap"] = {"params":
    {"a": a, "b": b}}`` plus ``"random_state"`` when it is not 0.  That is scanpy's documented shape; it is NOT pinned
    by a record (scanpy is absent), unlike the write-back of the two slots themselves.  ``copy=True`` returns a copy and
    leaves ``mdata`` untouched, otherwise None is returned.  Coordinates are not umap-learn's.

    ``diagnostics=dict()`` receives ``path`` ("kernel" or "tensor"), ``n_epochs``, ``entries``, ``a`` and ``b``.
    """
    if not (is_anndata(mdata) or is_mudata(mdata)):
        raise TypeError("Expected a MuData or an AnnData object")
    if neighbors_key is None:
        neighbors_key = "neighbors"
    try:
        neighbors = mdata.uns[neighbors_key]
    except KeyError:
        raise ValueError(f'Did not find .uns["{neighbors_key}"]. Run `muon.pp.neighbors` first.')
    if method == "rapids":
        raise NotImplementedError("muon_amd.tl.umap: method='rapids' is not implemented")
    if method != "umap":
        raise ValueError(f"method must be 'umap' or 'rapids', not {method!r}")
    if random_state is not None and (isinstance(random_state, bool) or not isinstance(random_state, (int, np.integer))):
        raise TypeError("muon_amd.tl.umap: random_state must be an integer or None")
    if isinstance(n_components, bool) or not isinstance(n_components, (int, np.integer)) or n_components < 1:
        raise ValueError("n_components must be an integer >= 1")
    if (isinstance(negative_sample_rate, bool) or not isinstance(negative_sample_rate, (int, np.integer))
            or not 0 <= negative_sample_rate <= 1024):
        raise ValueError("negative_sample_rate must be an integer in 0..1024")
    conn_key = neighbors["connectivities_key"]
    if conn_key not in mdata.obsp:
        raise ValueError(f'Did not find .obsp["{conn_key}"]. Run `muon.pp.neighbors` first.')
    conn = mdata.obsp[conn_key]
    n = int(conn.shape[0])
    if n != int(mdata.n_obs):
        raise ValueError("the graph must have one row per observation")
    n_epochs = default_epochs(n) if maxiter is None else int(maxiter)
    if not 1 <= n_epochs <= (1 << 20):
        raise ValueError("maxiter must be in 1..2^20")
    if a is None or b is None:
        a, b = find_ab(spread, min_dist)
    a, b = float(a), float(b)
    if not (a > 0 and b > 0):
        raise ValueError("a and b must be positive")

    be = backend_or_default(backend)
    g = _Graph(be, n, *edges(conn, n_epochs))
    seed = (int(np.random.default_rng().integers(0, 1 << 63)) if random_state is None else int(random_state)) & _M64
    Y0 = initial_positions(be, g, init_pos, int(n_components), random_state, mdata.obsm)
    if diagnostics is not None:
        diagnostics.update(a=a, b=b)
    Y = layout(be, g, Y0, n_epochs, float(alpha), float(gamma), int(negative_sample_rate), a, b, seed, diagnostics)
    X = be.to_host(Y).astype(np.float32)

    out = mdata.copy() if copy else mdata
    out.obsm["X_umap"] = X
    params = {"params": {"a": a, "b": b}}
    if random_state != 0:
        params["params"]["random_state"] = random_state
    out.uns["umap"] = params
    return out if copy else None
