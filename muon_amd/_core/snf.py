"""muon.tl.snf on MI355X: similarity network fusion (Wang et al. 2014) of the modalities' distance matrices.

The reference (/root/reference/muon/_core/tools.py:716-920) is restated statement for statement, all f64:

  * ``_affinity_matrix``: ``D <- (D + D^T) / 2`` with a zero diagonal; ``means_i`` = mean of the finite values among the
    2nd .. (k+1)-th smallest of row i, plus ``eps``; ``sig = (means_i + means_j) / 3 + D / 3 + eps``;
    ``W = N(0, sigma sig).pdf(D)``, symmetrised;
  * ``_normalize``: ``r_i`` = row sum minus diagonal (1 where that is 0), ``x_ij / (2 r_i)``, diagonal 0.5, symmetrised;
  * ``_dominateset``: per COLUMN the k largest are kept, then ``z / z.sum(axis=1)`` - a 1-d sum that broadcasts over the
    last axis, so ``P[i, j] = z[i, j] / rowsum_z[j]``.  P is built once, before the iterations;
  * the iteration ``next_j = P_j (sum_{i != j} W_i / (M - 1)) P_j^T`` then ``W_j <- _normalize(next_j)`` for all j;
  * ``W = _normalize(sum_j W_j / M)`` and the two graphs: the k smallest non-zero values of every row of ``0.5 - W``
    (distances) and of ``W`` (connectivities - the k SMALLEST affinities: that is what the reference states, and what is
    reproduced), ordered by ascending value.

Two formulations of the same statements:

  * the kernel path (csrc/snf.hip through ``HipBackend.snf_*``): P has k entries per column, so ``P S P^T`` is two
    sparse-times-dense passes ``Y = (P X)^T`` - N^2 k multiply-adds instead of N^3, bound by memory traffic - with X
    formed on read from the other modalities' matrices; affinity, normalisation and the top-k are kernels too; the
    counting / sorting that turns the top-k table into the CSR of P is tensor plumbing.  ``n_neighbors`` above
    ``snf_max_k()`` takes ``torch.topk`` for the dominate set (above ``snf_affinity_max_k()`` the tensor affinity), more
    than ``snf_max_terms() + 1`` modalities pre-sum the terms with a tensor operation;
  * the tensor formulation (``_fuse_torch``): the straightforward dense port, ``new @ S @ new.T``.  It runs where the
    backend has no ``snf_*`` methods (the CPU operator set of the tests) and needs no GPU.

The one place the package goes on where the reference raises: ``.obsp[distances_key]`` that is SPARSE (the only thing
scanpy ever writes; the reference ends in ``ValueError: shape too large to be a matrix``).  The package then computes
all pairwise Euclidean distances of the modality's representation - the ``use_rep`` / ``n_pcs`` of its neighbours
parameters, which the reference reads and never uses - in f64 on the device with the direct difference formula
``sqrt(sum_c (x_ic - x_jc)^2)`` (not the Gram trick), and continues as for a dense input.
"""
from __future__ import annotations

from typing import Dict, Optional, Union

import numpy as np
import torch
from scipy.sparse import csr_matrix, issparse

from .._backend import backend_or_default
from .._operators import has

_SQRT_2PI = float(np.sqrt(2 * np.pi))
_KERNEL_METHODS = ("snf_affinity", "snf_normalize", "snf_topk", "snf_p_scale", "snf_diffuse")


# ---- the tensor formulation: the reference's statements as torch operations ----------------------------------------------
def pairwise_distances(X: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """All pairwise Euclidean distances of the rows of X [n, p] (f64) by the direct formula, the squares added in
    column order: p passes over the n x n result, no n x n x p temporary."""
    n, p = (int(s) for s in X.shape)
    D = torch.zeros((n, n), dtype=torch.float64, device=X.device) if out is None else out.zero_()
    for c in range(p):
        col = X[:, c]
        d = col[:, None] - col[None, :]
        d.mul_(d)
        D.add_(d)
    if D.device.type == "cpu":  # (torch's vectorised host sqrt is not correctly rounded; the device's and numpy's are)
        h = D.numpy()
        np.sqrt(h, out=h)
        return D
    return D.sqrt_()


def _affinity_torch(D: torch.Tensor, k: int, sigma: float, eps: float) -> torch.Tensor:
    D = (D + D.T) / 2
    D.fill_diagonal_(0)
    srt = torch.sort(D, dim=1).values[:, 1:k + 1]
    fin = ~torch.isinf(srt)
    means = torch.where(fin, srt, torch.zeros_like(srt)).sum(dim=1) / fin.sum(dim=1) + eps
    sig = (means[:, None] + means[None, :]) / 3 + D / 3 + eps
    scale = sigma * sig
    y = D / scale
    dens = torch.exp(-(y * y) / 2.0) / _SQRT_2PI / scale  # scipy.stats.norm(0, scale).pdf(D)
    return (dens + dens.T) / 2


def _normalize_torch(x: torch.Tensor) -> torch.Tensor:
    r = x.sum(dim=1) - x.diagonal()
    r = torch.where(r == 0, torch.ones_like(r), r)
    x = x / (2 * r[:, None])
    x.fill_diagonal_(0.5)
    return (x + x.T) / 2


def _dominateset_torch(x: torch.Tensor, k: int) -> torch.Tensor:
    idx = torch.topk(x, k, dim=0).indices
    z = torch.zeros_like(x)
    z.scatter_(0, idx, x.gather(0, idx))
    return z / z.sum(dim=1)  # (1-d: broadcasts over the last axis, as in the reference)


def _fuse_torch(dists, k: int, n_iterations: int, sigma: float, eps: float, diagnostics: dict) -> torch.Tensor:
    wall = [_normalize_torch(_affinity_torch(D, k, sigma, eps)) for D in dists]
    new = [_dominateset_torch(w, k) for w in wall]
    diagnostics["p_row_counts"] = [(p != 0).sum(dim=1).cpu().numpy() for p in new]
    M = len(wall)
    for _ in range(n_iterations):
        nxt = []
        for j in range(M):
            s = torch.zeros_like(wall[j])
            for i in range(M):
                if i != j:
                    s = s + wall[i]
            nxt.append(new[j] @ (s / (M - 1)) @ new[j].T)
        wall = [_normalize_torch(x) for x in nxt]
    w = wall[0]
    for x in wall[1:]:
        w = w + x
    return _normalize_torch(w / M)


# ---- the kernel path -----------------------------------------------------------------------------------------------------
def dominate_csr(be, W: torch.Tensor, k: int, diagnostics: Optional[dict] = None):
    """P of ``_dominateset(W, k)`` for a symmetric W as a CSR ``(indptr int64, cols int32, vals f64)`` sorted by (row,
    column), and ``rowsum_z``.  Column j of z holds the k largest of row j of W (``be.snf_topk``; ``torch.topk`` past the
    kernel's k); entry (i, j) is then divided by the sum of row j of z."""
    n = int(W.shape[0])
    if k <= be.snf_max_k():
        idx, val = be.snf_topk(W, k)
        route = "kernel"
    else:
        val, idx = torch.topk(W[:, :n], k, dim=1)
        route = "tensor"
    if diagnostics is not None:
        diagnostics.setdefault("topk", []).append(route)
    rows = idx.reshape(-1).to(torch.int64)
    cols = torch.arange(n, device=W.device, dtype=torch.int64).repeat_interleave(k)
    order = torch.argsort(rows * n + cols)  # (the keys are distinct: any sort gives this order)
    indptr = torch.zeros((n + 1,), dtype=torch.int64, device=W.device)
    indptr[1:] = torch.cumsum(torch.bincount(rows, minlength=n), dim=0)
    p_cols = cols[order].to(torch.int32).contiguous()
    p_vals = val.reshape(-1)[order].contiguous()
    rowsum = be.snf_p_scale(indptr, p_cols, p_vals)
    return (indptr, p_cols, p_vals), rowsum


def diffuse(be, P, terms, out: torch.Tensor) -> torch.Tensor:
    """``out = (P X)^T`` with X the mean of ``terms``; more terms than the kernel adds are pre-summed."""
    if len(terms) > be.snf_max_terms():
        s = terms[0] + terms[1]
        for t in terms[2:]:
            s += t
        s /= len(terms)
        terms = [s]
    return be.snf_diffuse(P, terms, out)


def _need_bytes(n: int, M: int, k: int) -> int:
    """2 M + 2 dense n x n f64 matrices, and per modality the top-k table, the CSR of P and the sort's keys."""
    return (2 * M + 2) * n * n * 8 + M * (n * k * (12 + 12 + 24) + (n + 1) * 8)


def _fuse_kernel(be, load_distance, M: int, n: int, k: int, n_iterations: int, sigma: float, eps: float,
                 diagnostics: dict) -> torch.Tensor:
    W, P = [], []
    scratch = be.empty((n, n), torch.float64)
    tensor_affinity = k > be.snf_affinity_max_k()
    for m in range(M):
        D = load_distance(m, scratch)
        w = be.empty((n, n), torch.float64)
        if tensor_affinity:
            w.copy_(_affinity_torch(D, k, sigma, eps))
        else:
            be.snf_affinity(D, k, sigma, eps, out=w)
        be.snf_normalize(w, out=w)
        W.append(w)
    diagnostics["affinity"] = "tensor" if tensor_affinity else "kernel"
    counts = []
    for m in range(M):
        p, _ = dominate_csr(be, W[m], k, diagnostics)
        counts.append(be.to_host(p[0][1:] - p[0][:-1]))
        P.append(p)
    diagnostics["p_row_counts"] = counts
    diagnostics["diffuse_terms"] = min(M - 1, be.snf_max_terms())  # how many matrices the kernel adds while it reads
    nxt = [be.empty((n, n), torch.float64) for _ in range(M)]
    half, total = scratch, be.empty((n, n), torch.float64)
    for _ in range(n_iterations):
        for j in range(M):
            diffuse(be, P[j], [W[i] for i in range(M) if i != j], half)  # (P S)^T = S P^T: S is symmetric
            diffuse(be, P[j], [half], nxt[j])                            # (P S P^T)^T
        for j in range(M):
            be.snf_normalize(nxt[j], out=W[j])
    torch.add(W[0], W[1], out=total)
    for w in W[2:]:
        total += w
    total /= M
    return be.snf_normalize(total, out=total)


# ---- the graphs ----------------------------------------------------------------------------------------------------------
def _knn_rows(be, A: torch.Tensor, k: int) -> csr_matrix:
    """``_sparse_csr_fast_knn(csr_matrix(A), k)``: the k smallest non-zero values of every row, ascending."""
    n = int(A.shape[0])
    A = torch.where(A == 0, torch.full_like(A, float("inf")), A)  # the CSR conversion drops the exact zeros
    vals, idx = torch.topk(A, k, dim=1, largest=False, sorted=True)
    del A
    if bool(torch.isinf(vals[:, -1]).any()):
        raise ValueError(f"a row has fewer than n_neighbors = {k} non-zero entries")
    return csr_matrix((be.to_host(vals).reshape(-1), be.to_host(idx.to(torch.int32)).reshape(-1),
                       np.arange(0, n * k + 1, k, dtype=np.int32)), shape=(n, n))


def snf(mdata, n_neighbors: int = 20, neighbor_keys: Optional[Union[str, Dict[str, Optional[str]]]] = None,
        key_added: Optional[str] = None, n_iterations: int = 20, sigma: float = 0.5,
        eps: float = np.finfo(np.float64).eps, copy: bool = False, *, backend=None, diagnostics: Optional[dict] = None):
    """Similarity network fusion (SNF)

    Arguments, slots, parameters and error messages follow /root/reference/muon/_core/tools.py:716-920: the fused graph
    goes to ``.obsp["distances"]`` / ``.obsp["connectivities"]`` and ``.uns["neighbors"]`` (``key_added``: to
    ``.obsp[key_added + "_distances"]``, ...), every modality of ``mdata.mod`` is fused and ``neighbor_keys`` names the
    ``.uns`` slot of each modality's neighbours (a dict: only its modalities appear in the written ``use_rep`` /
    ``n_pcs``).  ``connectivities`` holds the k SMALLEST affinities of every row, as the reference states it.

    ``.obsp[distances_key]`` of a modality: a dense array of all pairwise distances, as the reference needs it, or a
    sparse graph (what scanpy writes; the reference raises) - then all pairwise Euclidean distances of the modality's
    representation are computed in f64 on the device (see the module docstring).

    ``diagnostics=dict()`` receives ``W`` (the fused dense matrix, a host array), ``p_row_counts`` (entries per row of
    each P), ``path`` ("kernel" or "tensor"), on the kernel path ``topk`` / ``affinity`` (which route each took) and
    ``diffuse_terms``, and ``distances`` ("dense" or "computed" per modality).

    Two more places where the reference does not give a result and the package says so or goes on: a single modality
    (the reference divides by M - 1 = 0) raises ``ValueError``; a modality that a ``neighbor_keys`` dict leaves out is
    fused through its ``.uns["neighbors"]`` (the reference ends in a ``KeyError`` there).
    """
    be = backend_or_default(backend)
    from .preproc import _choose_representation

    mdata = mdata.copy() if copy else mdata
    if neighbor_keys is None:
        modalities = list(mdata.mod.keys())
        neighbor_keys = {}
    elif isinstance(neighbor_keys, str):
        modalities = list(mdata.mod.keys())
        neighbor_keys = {m: neighbor_keys for m in modalities}
    else:
        modalities = list(neighbor_keys.keys())

    mod_reps, mod_n_pcs, neighbors_params, reps = {}, {}, {}, {}
    for mod in modalities:
        nkey = neighbor_keys.get(mod, "neighbors")
        try:
            nparams = mdata.mod[mod].uns[nkey]
        except KeyError:
            raise ValueError(
                f'Did not find .uns["{nkey}"] for modality "{mod}". Run `sc.pp.neighbors` on all modalities first.'
            )
        use_rep = nparams["params"].get("use_rep", None)
        n_pcs = nparams["params"].get("n_pcs", None)
        neighbors_params[mod] = nparams
        reps[mod] = _choose_representation(mdata.mod[mod], use_rep, n_pcs)
        mod_reps[mod] = use_rep if use_rep is not None else -1  # otherwise this is not saved to h5mu
        mod_n_pcs[mod] = n_pcs if n_pcs is not None else -1

    sources = []
    for mod in mdata.mod:
        nkey = neighbor_keys.get(mod, "neighbors")
        # the key has to exists in every modality
        if nkey not in mdata.mod[mod].uns:
            raise ValueError(f"The key '{nkey}' is missing from the .uns slot of modality '{mod}'")
        nparams = neighbors_params.get(mod, mdata.mod[mod].uns[nkey])
        dist = mdata.mod[mod].obsp[nparams["distances_key"]]
        if issparse(dist):
            if mod not in reps:
                reps[mod] = _choose_representation(mdata.mod[mod], nparams["params"].get("use_rep", None),
                                                   nparams["params"].get("n_pcs", None))
            X = reps[mod]
            sources.append(("computed", X.toarray() if issparse(X) else X))
        else:
            sources.append(("dense", dist))
    M = len(sources)
    n = int(sources[0][1].shape[0])
    k = int(n_neighbors)
    if k >= n:
        raise ValueError("'n_neighbors' seems to be too high.")
    if M < 2:
        raise ValueError("similarity network fusion needs at least two modalities")
    for kind, a in sources:
        if int(a.shape[0]) != n or (kind == "dense" and tuple(a.shape) != (n, n)):
            raise ValueError("every modality must hold the same observations: the distance matrices differ in shape")

    diag = {} if diagnostics is None else diagnostics
    diag["distances"] = [kind for kind, _ in sources]
    kernel = has(be, *_KERNEL_METHODS)
    diag["path"] = "kernel" if kernel else "tensor"
    if has(be, "free_memory"):
        need, free = _need_bytes(n, M, k), int(be.free_memory())
        if need > free:
            raise MemoryError(f"muon_amd.tl.snf: {M} modalities of {n} observations need {need} bytes on the device "
                              f"({2 * M + 2} dense {n} x {n} float64 matrices and the tables of P), {free} bytes are free")

    def as_device(a):
        if isinstance(a, torch.Tensor):
            return a.to(device=be.device, dtype=torch.float64)
        return be.to_device(np.ascontiguousarray(a, dtype=np.float64), np.float64)

    def load_distance(m, out=None):
        kind, a = sources[m]
        if kind == "computed":
            return pairwise_distances(as_device(a), out=out)
        if out is None:
            return as_device(a)
        out.copy_(as_device(a))
        return out

    if kernel:
        Wf = _fuse_kernel(be, load_distance, M, n, k, int(n_iterations), float(sigma), float(eps), diag)
    else:
        Wf = _fuse_torch([load_distance(m) for m in range(M)], k, int(n_iterations), float(sigma), float(eps), diag)

    neighbordistances = _knn_rows(be, 0.5 - Wf, k)
    # (the k smallest affinities of every row: what the reference states)
    connectivities = _knn_rows(be, Wf, k)
    if diagnostics is not None:
        diagnostics["W"] = be.to_host(Wf)
    del Wf

    if key_added is None:
        key_added = "neighbors"
        conns_key = "connectivities"
        dists_key = "distances"
    else:
        conns_key = key_added + "_connectivities"
        dists_key = key_added + "_distances"
    neighbors_dict = {"connectivities_key": conns_key, "distances_key": dists_key}
    neighbors_dict["params"] = {
        "n_neighbors": n_neighbors,
        "eps": eps,
        "use_rep": mod_reps,
        "n_pcs": mod_n_pcs,
        "method": "snf",
    }
    mdata.obsp[conns_key] = connectivities
    mdata.obsp[dists_key] = neighbordistances
    mdata.uns[key_added] = neighbors_dict
    return mdata if copy else None
