"""muon_amd.pp.harmony_integrate on MI355X: Harmony batch correction of an embedding that stays on the device.

Harmony (Korsunsky et al. 2019) alternates a soft k-means whose assignments are pushed towards an even mix of the batch
levels inside every cluster with a per-cluster ridge regression that takes the batch offsets out of the embedding.
scanpy offers it as ``scanpy.external.pp.harmony_integrate`` (harmonypy).  What follows is THE PACKAGE'S OWN STATEMENT of
the method, written after harmonypy from memory: harmonypy is not installed where the package is developed and PARITY
WITH IT IS NOT PINNED.  Two differences are deliberate: rows are normalised by their plain 2-norm (harmonypy first divides
a cell by its largest coordinate, which only flips the sign of cells with no positive coordinate), and the centres start
from one k-means++ draw on cosine distance followed by at most 25 spherical Lloyd rounds (harmonypy calls scikit-learn's
KMeans with ten restarts).  tests/harmony_refs.py restates the statement in NumPy; the tests hold both routes to it.

Notation: rows are cells, Z is N x d, ``l2rows`` divides every row by its 2-norm, Phi is the one-hot N x B matrix over
the levels of all keys, Pr = Phi.sum(0) / N, K the number of clusters.

  set-up      K = nclust or min(round(N / 30), 100);  th = theta per level, times 1 - exp(-(N_b / (K tau))^2) if tau > 0;
              lam = lamb per level;  Zc = l2rows(Z);  rs = np.random.RandomState(random_state)
  start       seeds: rs.randint(N), then K - 1 times min(searchsorted(cumsum(d2), rs.random_sample() * total, "right"),
              N - 1) with d2 the running minimum of max(2 (1 - Zc zc_j), 0); at most 25 Lloyd rounds: label = first
              arg-max of Zc Y^T, stop when the labels repeat, Y_k = l2rows(sum of the cluster's rows) through the
              one-hot product, an empty cluster keeps its centre
  assignment  D = 2 (1 - Zc Y^T);  S = exp(-D / sigma - rowmax(-D / sigma));  R = S / rowsum(S);
              E = outer(colsum(R), Pr);  O = R^T Phi
  objective   sum(R D) + sum(sigma_k R log R) + sum(sigma_k R_ik G[k, i]),  0 log 0 := 0,
              G = (th log((O + 1) / (E + 1))) Phi^T; both objective lists start with its first value
  iteration   (at most max_iter_harmony)
    cluster   at most max_iter_kmeans rounds: Y = l2rows(R^T Zc), D and S as above; order = rs.permutation(N) cut by
              np.array_split into ceil(1 / block_size) blocks; per block b, simultaneously for its cells:
                  E -= outer(colsum(R[b]), Pr);  O -= R[b]^T Phi[b];  F = ((E + 1) / (O + 1))^th
                  R[b] = rownormalise_L1(S[b] * (Phi[b] F^T));  E, O += the same sums of the new rows
              then the objective; from the fifth round on stop when (old - new) / |old| < epsilon_cluster, old and new
              the sums of the two last windows of 3 objectives (one list over all iterations)
    correct   Zcorr = Z; for every cluster k, Phi_moe = [1 | Phi]:
                  A_k = Phi_moe^T diag(R_:k) Phi_moe + diag(0, lam);  W_k = inv(A_k) Phi_moe^T diag(R_:k) Z;  W_k[0] = 0
                  Zcorr -= R_:k * (Phi W_k[1:])
              Zc = l2rows(Zcorr)
    stop      when (obj_h[-2] - obj_h[-1]) / |obj_h[-2]| < epsilon_harmony

Where each statement runs.  Everything N-long is on the device, everything K x B and the K inverses of order B + 1 are
small: the inverses are host NumPy (as ``tl.ica``'s k x k step), the permutation is the host generator's.  Per k-means
round one scalar comes back (the loop tests it), per iteration K B (B + d) numbers for the regressions.

  * the kernel route - one key with at most ``harmony_limits()`` levels (64), K <= 128, d <= 64, a backend with
    the ``harmony_*`` operators (csrc/harmony.hip): the cells are kept physically sorted by level inside
    the call (permuted on entry, undone on exit), R is row-major [N, Kp], Kp = K rounded up to 16, padding zero.
    ``harmony_gram`` gives R^T Zc (one segment), the Lloyd sums, the per-level moments of the regression (the level
    offsets as segments) and a block's per-(cluster, level) sums (an index list, Z a column of ones);
    ``harmony_assign`` computes distances, weights, the factor F[:, code_i] and the normalisation for a block's cells
    and writes their rows of R once; ``harmony_objective`` takes the three terms from one read of R;
    ``harmony_correct`` writes Zcorr and its normalised rows in one pass.
  * the tensor route - several keys, more levels, a wider basis, more clusters, or a backend without the kernels (the
    CPU operator set of the tests): the same statements as dense tensor operations with Phi [N, B].

Precision: all arithmetic is f64.  A float32 basis is widened exactly and the result is rounded once, as in ``tl.ica``.
"""
from __future__ import annotations

import numbers

import numpy as np
import pandas as pd
import torch

from .._backend import backend_or_default
from .._operators import has

_LLOYD_ROUNDS = 25
_KERNEL_OPS = ("harmony_limits", "harmony_gram", "harmony_assign", "harmony_objective", "harmony_correct")


def _l2rows(X: torch.Tensor) -> torch.Tensor:
    return X / torch.sqrt((X * X).sum(dim=1, keepdim=True))


def _per_level(value, default, n_levels, name):
    """A scalar or one value per key, repeated over that key's levels."""
    if value is None:
        value = default
    if isinstance(value, numbers.Real):
        vals = [float(value)] * len(n_levels)
    else:
        vals = [float(v) for v in np.asarray(value, dtype=np.float64).reshape(-1)]
        if len(vals) != len(n_levels):
            raise ValueError(f"{name}: a scalar or one value per key ({len(n_levels)}), got {len(vals)}")
    return np.repeat(np.asarray(vals, dtype=np.float64), n_levels)


class _Route:
    """What differs between the two routes: the layout of the cells and of R, and who computes the cell-long sums."""

    def __init__(self, be, Z, codes, n_levels, K, kernel):
        self.be, self.K, self.kernel = be, K, kernel
        N, d = Z.shape
        self.N, self.d, self.B = N, d, int(sum(n_levels))
        f64 = torch.float64
        if kernel:
            c = codes[0]
            self.perm = np.argsort(c, kind="stable")
            self.inv = np.empty(N, dtype=np.int64)
            self.inv[self.perm] = np.arange(N, dtype=np.int64)
            self.lvl_ptr = np.concatenate([[0], np.cumsum(np.bincount(c, minlength=self.B))]).astype(np.int64)
            self.codes = be.to_device(np.ascontiguousarray(c[self.perm], dtype=np.int32), np.int32)
            self.Z = be.to_device(np.ascontiguousarray(Z[self.perm]), np.float64)
            self.ones = torch.ones((N, 1), dtype=f64, device=self.Z.device)
            self.Kp = (K + 15) // 16 * 16
            self.Phi = None
        else:
            self.perm = self.inv = None
            self.Z = be.to_device(np.ascontiguousarray(Z), np.float64)
            Phi = np.zeros((N, self.B), dtype=np.float64)
            off = 0
            for c, nl in zip(codes, n_levels):
                Phi[np.arange(N), off + c] = 1.0
                off += nl
            self.Phi = be.to_device(Phi, np.float64)
            self.Kp = K

    # -- products over all cells -------------------------------------------------------------------------------------
    def gram(self, R, X):
        """R[:, :K]^T X, [K, width of X]."""
        if self.kernel:
            return self.be.harmony_gram(R, X, (0, self.N), self.K)[0, :self.K, :X.shape[1]]
        return R.T @ X

    def level_sums(self, R):
        """O = R^T Phi, [K, B]."""
        if self.kernel:
            return self.be.harmony_gram(R, self.ones, self.lvl_ptr, self.K)[:, :self.K, 0].T.contiguous()
        return R.T @ self.Phi

    def moments(self, R):
        """(G [K, B, B] = Phi^T diag(R_:k) Phi, M [K, B, d] = Phi^T diag(R_:k) Z) for every cluster k."""
        if self.kernel:
            M = self.be.harmony_gram(R, self.Z, self.lvl_ptr, self.K)[:, :self.K, :self.d].permute(1, 0, 2)
            return torch.diag_embed(self.level_sums(R)), M
        G, M = [], []
        for b in range(self.B):
            Rb = R * self.Phi[:, b:b + 1]
            G.append(Rb.T @ self.Phi)
            M.append(Rb.T @ self.Z)
        return torch.stack(G, dim=1), torch.stack(M, dim=1)

    def corrected(self, R, W):
        """(Zcorr = Z - sum_k R_:k * (Phi W_k), l2rows(Zcorr)) for W [K, B, d]."""
        if self.kernel:
            return self.be.harmony_correct(self.Z, R, W.permute(1, 0, 2).contiguous(), self.lvl_ptr)
        out = self.Z.clone()
        for b in range(self.B):
            out -= self.Phi[:, b:b + 1] * (R @ W[:, b, :])
        return out, _l2rows(out)

    # -- the soft assignment --------------------------------------------------------------------------------------------
    def first_assignment(self, Zc, Y, sigma):
        """R = S / rowsum(S)."""
        if self.kernel:
            R = torch.empty((self.N, self.Kp), dtype=torch.float64, device=Zc.device)
            F1 = torch.ones((self.K, self.B), dtype=torch.float64, device=Zc.device)
            self.be.harmony_assign(Zc, Y.contiguous(), sigma, F1, self.codes, R)
            return R
        S = self.weights(Zc, Y, sigma)
        return S / S.sum(dim=1, keepdim=True)

    @staticmethod
    def weights(Zc, Y, sigma):
        T = -(2.0 * (1.0 - Zc @ Y.T)) / sigma
        return torch.exp(T - T.max(dim=1, keepdim=True).values)

    def round_blocks(self, R, Zc, Y, sigma, E, O, Pr, th, blocks):
        """One pass over the blocks of a k-means round: R, E and O are updated in place."""
        if self.kernel:
            pos = [np.sort(self.inv[b]) for b in blocks]  # (sorted positions: sorted by level)
            idx_all = self.be.to_device(np.concatenate(pos), np.int64)
            start = 0
            for p in pos:
                idx = idx_all[start:start + p.size]
                start += p.size
                seg = np.searchsorted(p, self.lvl_ptr, side="left")
                O_old = self.be.harmony_gram(R, self.ones, seg, self.K, idx=idx, checked=True)[:, :self.K, 0].T
                E -= torch.outer(O_old.sum(dim=1), Pr)
                O -= O_old
                F = torch.pow((E + 1.0) / (O + 1.0), th).contiguous()
                self.be.harmony_assign(Zc, Y, sigma, F, self.codes, R, idx=idx, checked=True)
                O_new = self.be.harmony_gram(R, self.ones, seg, self.K, idx=idx, checked=True)[:, :self.K, 0].T
                E += torch.outer(O_new.sum(dim=1), Pr)
                O += O_new
            return
        S = self.weights(Zc, Y, sigma)
        for b in blocks:
            ib = self.be.to_device(np.ascontiguousarray(b, dtype=np.int64), np.int64)
            Rb, Pb = R[ib], self.Phi[ib]
            E -= torch.outer(Rb.sum(dim=0), Pr)
            O -= Rb.T @ Pb
            F = torch.pow((E + 1.0) / (O + 1.0), th)
            Rb = S[ib] * (Pb @ F.T)
            Rb = Rb / Rb.sum(dim=1, keepdim=True)
            R[ib] = Rb
            E += torch.outer(Rb.sum(dim=0), Pr)
            O += Rb.T @ Pb

    def objective(self, R, Zc, Y, sigma, E, O, th) -> float:
        G = th * torch.log((O + 1.0) / (E + 1.0))
        if self.kernel:
            total = self.be.harmony_objective(Zc, Y, R, sigma, G.contiguous(), self.codes).sum()
        else:
            D = 2.0 * (1.0 - Zc @ Y.T)
            total = (R * D).sum() + (torch.xlogy(R, R) * sigma).sum() + (R * (self.Phi @ G.T) * sigma).sum()
        return float(total.item())  # the one scalar a round's test needs


def _initial_centres(route: _Route, Zc, K: int, rs) -> torch.Tensor:
    """The k-means++ draw on cosine distance and the spherical Lloyd rounds; the cells in the caller's order."""
    be, N = route.be, route.N
    seeds = [int(rs.randint(N))]
    d2 = None
    for _ in range(1, K):
        dist = torch.clamp(2.0 * (1.0 - Zc @ Zc[seeds[-1]]), min=0.0)
        d2 = dist if d2 is None else torch.minimum(d2, dist)
        c = np.cumsum(be.to_host(d2))  # (the N-long d2 goes to the host for the draw)
        seeds.append(min(int(np.searchsorted(c, rs.random_sample() * c[-1], side="right")), N - 1))
    Y = Zc[be.to_device(np.asarray(seeds, dtype=np.int64), np.int64)].clone()
    labels = None
    for _ in range(_LLOYD_ROUNDS):
        new = torch.argmax(Zc @ Y.T, dim=1)
        if labels is not None and bool(torch.equal(new, labels)):
            break
        labels = new
        onehot = torch.zeros((N, route.Kp), dtype=torch.float64, device=Zc.device)
        onehot[torch.arange(N, device=Zc.device), labels] = 1.0
        sums = route.gram(onehot, Zc)
        count = torch.bincount(labels, minlength=K)
        Y = torch.where((count > 0)[:, None], _l2rows(sums), Y)
    return Y


def _regression(G, M, lam, n_first: int):
    """W [K, B, d]: for every cluster the ridge regression on [1 | Phi] with the intercept's row dropped.  Host NumPy;
    G [K, B, B] and M [K, B, d] as ``_Route.moments`` gives them.  Every cell has one level of the first key, so the
    sums over its ``n_first`` levels are the sums over all cells: the intercept's row and column."""
    K, B, d = M.shape
    W = np.empty((K, B, d), dtype=np.float64)
    ridge = np.diag(np.concatenate([[0.0], lam]))
    for k in range(K):
        o = np.diagonal(G[k])
        A = np.empty((B + 1, B + 1), dtype=np.float64)
        A[1:, 1:] = G[k]
        A[0, 1:] = A[1:, 0] = o
        A[0, 0] = o[:n_first].sum()
        rhs = np.empty((B + 1, d), dtype=np.float64)
        rhs[1:] = M[k]
        rhs[0] = M[k, :n_first].sum(axis=0)
        W[k] = (np.linalg.inv(A + ridge) @ rhs)[1:]
    return W


def _harmonize(be, Z: np.ndarray, codes, n_levels, *, theta=None, lamb=None, sigma=0.1, nclust=None, tau=0,
               block_size=0.05, max_iter_harmony=10, max_iter_kmeans=20, epsilon_cluster=1e-5, epsilon_harmony=1e-4,
               random_state=0, force_tensor=False) -> dict:
    """The statement of the module docstring on arrays: Z [N, d] host f64, ``codes`` one int array of level codes per
    key, ``n_levels`` their numbers of levels.  Returns a dict with ``Z_corr`` and ``R`` (host, the caller's cell order,
    R [N, K]), ``Y`` (the last round's centres), ``route`` ("kernel" or "tensor") and the entries of ``return_info``.
    ``force_tensor``: the tensor formulation even where the kernels apply (what tests and the probe compare with)."""
    Z = np.ascontiguousarray(Z, dtype=np.float64)
    N, d = Z.shape
    n_levels = [int(v) for v in n_levels]
    codes = [np.asarray(c, dtype=np.int64) for c in codes]
    B = sum(n_levels)
    for c, nl in zip(codes, n_levels):
        if c.shape != (N,) or (N and (c.min() < 0 or c.max() >= nl)):  # checked on the host before any launch
            raise ValueError("key: a level code outside [0, number of levels)")
    if not 0 < block_size <= 1:
        raise ValueError(f"block_size must lie in (0, 1], got {block_size!r}")
    if nclust is None:
        if N < 30:
            raise ValueError(f"nclust: fewer than 30 cells ({N}) leave no cluster; give nclust")
        K = int(min(np.round(N / 30.0), 100))
    else:
        K = int(nclust)
        if K < 1 or K > N:
            raise ValueError(f"nclust must lie in [1, number of cells = {N}], got {nclust!r}")
    bad = ~np.isfinite(Z).all(axis=1) | ~(np.abs(Z).max(axis=1, initial=0.0) > 0)
    if bad.any():
        raise ValueError(f"basis: row {int(np.flatnonzero(bad)[0])} is all zero or not finite")
    th_h = _per_level(theta, 2.0, n_levels, "theta")
    lam_h = _per_level(lamb, 1.0, n_levels, "lamb")
    sig_h = np.asarray(sigma, dtype=np.float64).reshape(-1)
    if sig_h.size == 1:
        sig_h = np.repeat(sig_h, K)
    if sig_h.size != K or not (sig_h > 0).all():
        raise ValueError(f"sigma: a positive scalar or one positive value per cluster ({K})")
    counts = np.concatenate([np.bincount(c, minlength=nl) for c, nl in zip(codes, n_levels)]).astype(np.float64)
    if tau > 0:
        th_h = th_h * (1.0 - np.exp(-(counts / (K * tau)) ** 2))
    rs = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)

    kernel = False
    if not force_tensor and len(codes) == 1 and has(be, *_KERNEL_OPS):
        lim = be.harmony_limits()
        kernel = B <= lim["levels"] and K <= lim["clusters"] and d <= lim["dims"]

    # the start: in the caller's cell order on both routes (the draw walks the cells in that order)
    start = _Route(be, Z, codes, n_levels, K, False) if not kernel else None
    Z0 = start.Z if start is not None else be.to_device(Z, np.float64)
    probe = start if start is not None else _StartOnly(be, N, K)
    Y = _initial_centres(probe, _l2rows(Z0), K, rs)
    route = start if start is not None else _Route(be, Z, codes, n_levels, K, True)
    del Z0, probe, start

    th = be.to_device(th_h, np.float64)
    sig = be.to_device(sig_h, np.float64)
    Pr = be.to_device(counts / N, np.float64)
    Zc = _l2rows(route.Z)
    R = route.first_assignment(Zc, Y, sig)
    O = route.level_sums(R)
    E = torch.outer(R[:, :K].sum(dim=0) if not kernel else O.sum(dim=1), Pr)
    obj_k = [route.objective(R, Zc, Y, sig, E, O, th)]
    obj_h = [obj_k[0]]
    n_blocks = int(np.ceil(1.0 / block_size))
    rounds, converged = [], False
    Zcorr = route.Z
    for it in range(int(max_iter_harmony)):
        r = -1
        for r in range(int(max_iter_kmeans)):
            Y = _l2rows(route.gram(R, Zc)).contiguous()
            blocks = np.array_split(rs.permutation(N), n_blocks)
            route.round_blocks(R, Zc, Y, sig, E, O, Pr, th, blocks)
            obj_k.append(route.objective(R, Zc, Y, sig, E, O, th))
            if r > 3:
                old, new = sum(obj_k[-6:-3]), sum(obj_k[-3:])
                if (old - new) / abs(old) < epsilon_cluster:
                    break
        rounds.append(r + 1)
        obj_h.append(obj_k[-1])
        G, M = route.moments(R)
        host = be.to_host(torch.cat([G.reshape(-1), M.reshape(-1)]))  # the numbers the K regressions need
        W = _regression(host[:K * B * B].reshape(K, B, B), host[K * B * B:].reshape(K, B, d), lam_h, n_levels[0])
        Zcorr, Zc = route.corrected(R, be.to_device(W, np.float64))
        if (obj_h[-2] - obj_h[-1]) / abs(obj_h[-2]) < epsilon_harmony:
            converged = True
            break
    n_iter = len(rounds)

    Zh, Rh = be.to_host(Zcorr), be.to_host(R[:, :K].contiguous())
    if route.kernel:
        Zh, Rh = Zh[route.inv], Rh[route.inv]
    return {"Z_corr": Zh, "R": Rh, "Y": be.to_host(Y), "route": "kernel" if route.kernel else "tensor",
            "kmeans_rounds": rounds, "n_iter": n_iter, "converged": converged, "objective_harmony": obj_h,
            "objective_kmeans": obj_k, "nclust": K}


class _StartOnly:
    """The one product the start needs on the kernel route (the cells still in the caller's order)."""

    def __init__(self, be, N, K):
        self.be, self.N, self.K, self.Kp = be, N, K, (K + 15) // 16 * 16

    def gram(self, R, X):
        return self.be.harmony_gram(R, X, (0, self.N), self.K)[0, :self.K, :X.shape[1]]


def harmony_integrate(data, key, *, basis="X_pca", adjusted_basis="X_pca_harmony", theta=None, lamb=None, sigma=0.1,
                      nclust=None, tau=0, block_size=0.05, max_iter_harmony=10, max_iter_kmeans=20,
                      epsilon_cluster=1e-5, epsilon_harmony=1e-4, random_state=0, return_info=False, backend=None):
    """Harmony batch correction of an embedding (scanpy.external.pp.harmony_integrate's place in a workflow).

    ``data``: AnnData or MuData (anything with ``.obs`` and ``.obsm``); ``key``: one ``.obs`` column or a sequence of
    them, the levels in the order of pandas' ``astype("category")``; ``data.obsm[basis]`` [N, d] is corrected into
    ``data.obsm[adjusted_basis]``, in the dtype of the basis.  ``theta`` (default 2) and ``lamb`` (default 1): a scalar or
    one value per key; ``sigma``: a scalar or one value per cluster; ``nclust`` defaults to min(round(N / 30), 100).
    Returns None, or with ``return_info=True`` a dict with ``kmeans_rounds`` (one count per Harmony iteration),
    ``n_iter``, ``converged``, ``objective_harmony`` and ``nclust``.

    The arithmetic is the package's own statement of Harmony (module docstring), all in f64: parity with
    harmonypy is not pinned.  One key with at most 64 levels, at most 128 clusters and a basis of at most 64 columns runs
    the k-means rounds on the kernels of csrc/harmony.hip; everything else takes the tensor formulation in the same
    call.  Raises KeyError for a missing column, ValueError for N < 30 without ``nclust``, ``nclust`` outside [1, N], a
    basis row that is all zero or not finite, and ``block_size`` outside (0, 1].
    """
    be = backend_or_default(backend)
    keys = [key] if isinstance(key, str) else list(key)
    if not keys:
        raise ValueError("key: at least one .obs column")
    codes, n_levels = [], []
    for k in keys:
        if k not in data.obs.columns:
            raise KeyError(f"key: {k!r} is no column of .obs")
        cat = pd.Series(np.asarray(data.obs[k])).astype("category").cat
        if (cat.codes < 0).any():
            raise ValueError(f"key: column {k!r} has missing values")
        codes.append(np.asarray(cat.codes, dtype=np.int64))
        n_levels.append(len(cat.categories))
    if basis not in data.obsm:
        raise KeyError(f"basis: {basis!r} is no entry of .obsm")
    X = data.obsm[basis]
    X = X.detach().cpu().numpy() if isinstance(X, torch.Tensor) else np.asarray(X)
    if X.ndim != 2:
        raise ValueError(f"basis: expected a 2D array, got {X.ndim}D")
    odt = X.dtype if X.dtype in (np.float32, np.float64) else np.dtype(np.float64)
    res = _harmonize(be, X.astype(np.float64), codes, n_levels, theta=theta, lamb=lamb, sigma=sigma, nclust=nclust,
                     tau=tau, block_size=block_size, max_iter_harmony=max_iter_harmony,
                     max_iter_kmeans=max_iter_kmeans, epsilon_cluster=epsilon_cluster,
                     epsilon_harmony=epsilon_harmony, random_state=random_state)
    data.obsm[adjusted_basis] = res["Z_corr"].astype(odt, copy=False)
    if return_info:
        return {n: res[n] for n in ("kmeans_rounds", "n_iter", "converged", "objective_harmony", "nclust")}
    return None
