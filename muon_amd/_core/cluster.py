"""muon.tl.leiden / muon.tl.louvain on MI355X: multiplex community detection over the modalities' graphs.

The reference (/root/reference/muon/_core/tools.py:928-1206) builds one igraph per modality, one
RBConfigurationVertexPartition per graph (each with its own resolution, and WITHOUT ``weights=``: every stored non-zero
entry is an edge of weight 1) and hands them with ``layer_weights`` to leidenalg's / louvain's
``optimise_partition_multiplex``.  Those libraries are third-party C++ and absent here; the quality function below is
theirs, the optimiser is this module's own and is stated here in full (tests/cluster_refs.py restates it with
per-vertex dictionaries).  Parity with leidenalg's own labels is NOT pinned: leidenalg visits vertices one at a time in
a random queue and refines at random; this optimiser decides a quarter of the vertices at a time from one snapshot.

The quality function, all f64.  For layer l: A its matrix (ones at the stored non-zeros, or the stored values), with
``directed=False`` A <- A + A^T (igraph's undirected graph from both triangles); m = sum(A), kout = row sums, kin =
column sums, lambda the layer weight, gamma the resolution:

    Q_l = sum_c [ sum_{i,j in c} A_ij - gamma Kout_c Kin_c / m ],      Q = sum_l lambda_l Q_l

(leidenalg's RBConfiguration, unnormalised; a layer with m = 0 contributes nothing).  The layers share their vertices,
so the optimiser works on ONE graph: S = sum_l lambda_l (A_l + A_l^T), coalesced, its diagonal kept aside as self_v, and
a strength table P[v, 2L] = (kout^1, kin^1, kout^2, ...) with coefficients c_l = (gamma_l lambda_l) / m_l.  Then

    Q = sum_c [ (sum_{v in c} self_v + sum_{u != v in c} S_uv) / 2 - sum_l c_l Kout_c^l Kin_c^l ],  K[c] = sum_{u in c} P[u].

The optimiser, per level with nv vertices:

  1. Labels and classes.  At level 0 labels are arange(nv) (a later ``n_iterations`` pass: its predecessor's result),
     at later levels the ones handed down by step 5.  ``cls = rng.permutation(nv) % 4`` with
     ``rng = np.random.default_rng(random_state)`` carried across levels and passes.
  2. Sweep = four sub-rounds r = 0..3.  In a sub-round every vertex v of class r decides from the same snapshot of
     labels, totals K and community sizes.  Candidates: its own community a and the communities of its neighbours in
     S.  ``score(C) = w(v, C) - sum_l c_l (kout_v Kin_C + kin_v Kout_C)`` (the sum over l in order, from 0), w the sum
     of S's weights from v into C, and P[v] taken out of K[a].  Swap guard: when v is alone in a, a candidate C != a
     with one member and C > a is no candidate.  The best is the largest score, ties to the smallest id; v moves if
     that is not a and ``score > score(a)`` strictly.  All moves of the sub-round are applied, then K and the sizes are
     recomputed.
  3. After a sweep in which something moved, Q is computed; if it did not strictly increase the labels from before
     that sweep are restored and the level's sweeps end.  They also end after a sweep without moves, or after 50.
  4. Refinement (leiden; louvain: refined = step 3's labels).  Refined labels start as singletons; sweeps as in step 2
     with the level's classes, but only vertices still alone in their refined community decide, and only neighbours
     with the same step-3 label count.  The own score is 0, so a vertex moves when its best score is > 0.  Same swap
     guard.  A move into a one-member community whose own vertex (there the community id is that vertex's id) also
     proposes a move in this sub-round is cancelled.  Sweeps repeat until none moves.  Members of a refined community
     never leave it, so every refined community is connected.
  5. Aggregate: the refined labels are compacted in id order; coarse S, P and self are segment sums over sorted keys
     (self_C = sum of the members' self + sum of S inside C); the next level's labels are step 3's communities of the
     members, named by their smallest coarse vertex.
  6. Stop when step 3 ends with the labels the level began with.  Membership is the composition through the levels;
     communities are numbered by decreasing size, ties by smallest member (leidenalg's renumbering).

Two formulations of a sub-round:

  * the kernel (csrc/cluster.hip ``k_cluster_move`` through ``HipBackend.cluster_move``): a wave per vertex, neighbours
    64 at a time, grouped by community with ballots and a fixed-order cross-lane sum into a wave-private LDS table;
  * the tensor formulation (``_move_tensor``): sort (vertex, neighbour's label) keys, segment-sum, segmented arg-max
    with the tie rule.  It runs where the backend has no ``cluster_*`` methods (the CPU operator set of the tests), with
    more layers than ``cluster_max_layers()``, and for a level on which the kernel reported that a vertex has more
    distinct neighbouring communities than its table holds (``cluster_max_table()``).  The two add a vertex's
    w(v, C) in different orders: on exactly representable weights they agree bit for bit, on float weights to rounding.

Totals, aggregation and Q's per-community terms are fixed-order segmented sums (``k_cluster_segsum``; ``index_add_`` on
the CPU operator set); sorting is ``torch.sort(stable=True)``.  No float atomics: repeats are bit-equal.
"""
from __future__ import annotations

import time
from collections.abc import Mapping, Sequence
from types import MappingProxyType
from typing import Any, Optional

import numpy as np
import pandas as pd
import torch
from scipy.sparse import csr_matrix

from .._backend import backend_or_default
from .._containers import is_anndata, is_mudata
from .._operators import has

_KERNEL_METHODS = ("cluster_move", "cluster_segsum", "cluster_max_table", "cluster_max_layers")
MAX_SWEEPS = 50
N_CLASSES = 4


class _TableOverflow(Exception):
    pass


# ---- fixed-order building blocks --------------------------------------------------------------------------------------------
def _ptr_of_counts(counts: torch.Tensor) -> torch.Tensor:
    ptr = torch.zeros((int(counts.numel()) + 1,), dtype=torch.int64, device=counts.device)
    ptr[1:] = torch.cumsum(counts, dim=0)
    return ptr


def _segsum(be, vals: torch.Tensor, ptr: torch.Tensor) -> torch.Tensor:
    """``out[s] = sum(vals[ptr[s]:ptr[s + 1]])`` for f64 rows [n, w], in a fixed order."""
    if has(be, "cluster_segsum"):
        return be.cluster_segsum(vals.contiguous(), ptr)
    if vals.device.type != "cpu":  # (a device's index_add_ adds with atomics: no fixed order, no bit-equal repeats)
        raise RuntimeError("muon_amd.tl.leiden / louvain / umap: a device backend must provide cluster_segsum")
    nseg = int(ptr.numel()) - 1
    out = torch.zeros((nseg, int(vals.shape[1])), dtype=torch.float64, device=vals.device)
    ids = torch.repeat_interleave(torch.arange(nseg, device=vals.device), ptr[1:] - ptr[:-1])
    return out.index_add_(0, ids, vals)  # (the host's index_add_ adds in index order)


def _coalesce(be, r: torch.Tensor, c: torch.Tensor, v: torch.Tensor, nv: int):
    """The entries (r, c, v) summed per distinct (r, c), sorted by (r, c); equal keys are added in the order given."""
    key, order = torch.sort(r * nv + c, stable=True)
    uk, counts = torch.unique_consecutive(key, return_counts=True)
    sv = _segsum(be, v[order].reshape(-1, 1), _ptr_of_counts(counts))[:, 0]
    return torch.div(uk, nv, rounding_mode="floor"), uk % nv, sv


class _Graph:
    """One level's graph: S without its diagonal as a CSR sorted by (row, column), self, P and the coefficients."""

    def __init__(self, nv, r, c, v, selfw, P, coef):
        self.nv = int(nv)
        self.rows = r
        self.cols64 = c
        self.cols = c.to(torch.int32)
        self.vals = v
        self.indptr = _ptr_of_counts(torch.bincount(r, minlength=self.nv))
        self.selfw = selfw
        self.P = P.contiguous()
        self.coef = [float(x) for x in coef]
        self.L = len(self.coef)

    @classmethod
    def from_entries(cls, be, nv, r, c, v, selfw, P, coef):
        """Coalesces (r, c, v); what lands on the diagonal is added to ``selfw``."""
        r, c, v = _coalesce(be, r, c, v, nv)
        d = r == c
        selfw = selfw.clone()
        selfw[r[d]] += v[d]  # (distinct rows: no two diagonal entries share one)
        off = ~d
        return cls(nv, r[off], c[off], v[off], selfw, P, coef)


def _build_graph(be, layers, lambdas, gammas, directed: bool) -> _Graph:
    """``layers``: per modality ``(rows, cols, values)`` host arrays of its edges."""
    nv = layers[0][3]
    dev = be.device
    rs, cs, vs, Pcols, coef = [], [], [], [], []
    for (r, c, v, _n), lam, gam in zip(layers, lambdas, gammas):
        r = be.to_device(np.ascontiguousarray(r, dtype=np.int64), np.int64)
        c = be.to_device(np.ascontiguousarray(c, dtype=np.int64), np.int64)
        v = be.to_device(np.ascontiguousarray(v, dtype=np.float64), np.float64)
        if not directed:
            r, c, v = torch.cat([r, c]), torch.cat([c, r]), torch.cat([v, v])
        # strengths: entries sorted by row / by column, added in that order
        for idx in (r, c):
            key, order = torch.sort(idx, stable=True)
            ptr = _ptr_of_counts(torch.bincount(key, minlength=nv))
            Pcols.append(_segsum(be, v[order].reshape(-1, 1), ptr))
        m = float(Pcols[-2].sum()) if nv > 0 else 0.0
        coef.append((gam * lam) / m if m != 0 else 0.0)
        rs += [r, c]
        cs += [c, r]
        vs += [lam * v, lam * v]
    P = torch.cat(Pcols, dim=1) if nv > 0 else torch.zeros((0, 2 * len(layers)), dtype=torch.float64, device=dev)
    selfw = torch.zeros((nv,), dtype=torch.float64, device=dev)
    return _Graph.from_entries(be, nv, torch.cat(rs), torch.cat(cs), torch.cat(vs), selfw, P, coef)


def _totals(be, g: _Graph, labels: torch.Tensor):
    """``K[c] = sum of P over the members of c`` [nv, 2L] and the sizes [nv] (int32)."""
    lab = labels.long()
    order = torch.sort(lab, stable=True).indices
    cnt = torch.bincount(lab, minlength=g.nv)
    return _segsum(be, g.P[order], _ptr_of_counts(cnt)), cnt.to(torch.int32)


def quality(be, g: _Graph, labels: torch.Tensor) -> float:
    """Q of ``labels`` on the level's graph (module docstring)."""
    if g.nv == 0:
        return 0.0
    lab = labels.long()
    same = lab[g.rows] == lab[g.cols64]
    inner = torch.where(same, g.vals, torch.zeros_like(g.vals))
    win = _segsum(be, inner.reshape(-1, 1), g.indptr)[:, 0] + g.selfw
    order = torch.sort(lab, stable=True).indices
    ptr = _ptr_of_counts(torch.bincount(lab, minlength=g.nv))
    T = _segsum(be, torch.cat([win.reshape(-1, 1), g.P], dim=1)[order], ptr)
    pen = torch.zeros((g.nv,), dtype=torch.float64, device=T.device)
    for l in range(g.L):
        pen = pen + g.coef[l] * (T[:, 1 + 2 * l] * T[:, 2 + 2 * l])
    return float(torch.sum(T[:, 0] / 2 - pen))


# ---- one sub-round: the tensor formulation ------------------------------------------------------------------------------------
def _move_tensor(be, g: _Graph, labels, bound, only_single: bool, active, K, size):
    """Proposals [nv] int32 (the own label where a vertex stays or does not decide) and the score of the community each
    proposal names [nv] f64 (0 where the vertex does not decide)."""
    nv = g.nv
    lab = labels.long()
    if only_single:
        active = active & (size[lab] == 1)
    ent = active[g.rows]
    if bound is not None:
        ent = ent & (bound[g.rows] == bound[g.cols64])
    av = torch.nonzero(active).reshape(-1)
    r_all = torch.cat([av, g.rows[ent]])
    c_all = torch.cat([lab[av], lab[g.cols64[ent]]])
    w_all = torch.cat([torch.zeros((int(av.numel()),), dtype=torch.float64, device=lab.device), g.vals[ent]])
    pv, pc, w = _coalesce(be, r_all, c_all, w_all, max(nv, 1))
    a = lab[pv]
    own = pc == a
    Pv = g.P[pv]
    Kc = K[pc]
    Kc = torch.where(own[:, None], Kc - Pv, Kc)
    pen = torch.zeros_like(w)
    for l in range(g.L):
        pen = pen + g.coef[l] * (Pv[:, 2 * l] * Kc[:, 2 * l + 1] + Pv[:, 2 * l + 1] * Kc[:, 2 * l])
    score = w - pen
    guarded = (~own) & (size[a] == 1) & (size[pc] == 1) & (pc > a)
    ranked = torch.where(guarded, torch.full_like(score, float("-inf")), score)
    npair = int(pv.numel())
    best = torch.full((nv,), float("-inf"), dtype=torch.float64, device=lab.device)
    best = best.scatter_reduce(0, pv, ranked, "amax", include_self=True)
    pos = torch.arange(npair, device=lab.device)
    first = torch.full((nv,), npair, dtype=torch.int64, device=lab.device)
    # the pairs are sorted by (vertex, community): the first position holding the maximum is the smallest id
    first = first.scatter_reduce(0, pv, torch.where(ranked == best[pv], pos, torch.full_like(pos, npair)), "amin",
                                 include_self=True)
    own_score = torch.zeros((nv,), dtype=torch.float64, device=lab.device)
    own_score[pv[own]] = score[own]
    prop = labels.clone()
    out = torch.zeros((nv,), dtype=torch.float64, device=lab.device)
    if int(av.numel()):
        bv = first[av]
        bc, bs = pc[bv], score[bv]
        mv = (bc != lab[av]) & (bs > own_score[av])
        prop[av] = torch.where(mv, bc, lab[av]).to(torch.int32)
        out[av] = torch.where(mv, bs, own_score[av])
    return prop, out


# ---- a level -----------------------------------------------------------------------------------------------------------------
class _Level:
    def __init__(self, be, g: _Graph, cls_host: np.ndarray, kernel: bool):
        self.be, self.g, self.kernel = be, g, kernel
        cls = be.to_device(np.ascontiguousarray(cls_host, dtype=np.int64), np.int64)
        self.active = [cls == r for r in range(N_CLASSES)]
        self.count = [int((cls_host == r).sum()) for r in range(N_CLASSES)]
        if kernel:
            self.verts = [torch.nonzero(m).reshape(-1).to(torch.int32) for m in self.active]
            self.flag = be.zeros((1,), torch.int32)

    def sub_round(self, r: int, labels, bound, only_single: bool):
        be, g = self.be, self.g
        K, size = _totals(be, g, labels)
        if self.kernel:
            prop = labels.clone()
            score = be.zeros((g.nv,), torch.float64)
            be.cluster_move(self.verts[r], g.indptr, g.cols, g.vals, labels, bound, size, g.P, K, g.coef, only_single,
                            prop, score, self.flag)
        else:
            prop, _ = _move_tensor(be, g, labels, bound, only_single, self.active[r], K, size)
        if only_single:  # refinement: no move into a one-member community whose own vertex proposes a move
            moved = prop != labels
            tgt = prop.long()
            cancel = moved & (size[tgt] == 1) & moved[tgt]
            prop = torch.where(cancel, labels, prop)
        return prop

    def sweep(self, labels, bound, only_single: bool):
        """One sweep: ``(labels after it, number of moves)``."""
        moves = torch.zeros((), dtype=torch.int64, device=labels.device)
        for r in range(N_CLASSES):
            if self.count[r] == 0:
                continue
            new = self.sub_round(r, labels, bound, only_single)
            moves = moves + (new != labels).sum()
            labels = new
        if self.kernel:
            nm, flag = (int(x) for x in torch.stack([moves, self.flag[0].to(torch.int64)]).tolist())
            if flag:
                raise _TableOverflow()
            return labels, nm
        return labels, int(moves)

    def local_moving(self, labels, rec: dict):
        q = quality(self.be, self.g, labels)
        rec["sweeps"] = 0
        while rec["sweeps"] < MAX_SWEEPS:
            new, nm = self.sweep(labels, None, False)
            rec["sweeps"] += 1
            if nm == 0:
                break
            qn = quality(self.be, self.g, new)
            if not qn > q:
                break  # (the labels from before this sweep stay)
            labels, q = new, qn
        rec["q"] = q
        return labels

    def refine(self, bound, rec: dict):
        ref = torch.arange(self.g.nv, dtype=torch.int32, device=bound.device)
        rec["refine_sweeps"] = 0
        while True:
            ref, nm = self.sweep(ref, bound, True)
            rec["refine_sweeps"] += 1
            if nm == 0:
                return ref


def _aggregate(be, g: _Graph, refined, labels):
    """``(coarse graph, coarse vertex of every vertex, the next level's labels)``."""
    nv = g.nv
    ref = refined.long()
    present = torch.bincount(ref, minlength=nv) > 0
    newid = torch.cumsum(present.to(torch.int64), dim=0) - 1
    cv = newid[ref]
    nc = int(present.sum())
    order = torch.sort(cv, stable=True).indices
    ptr = _ptr_of_counts(torch.bincount(cv, minlength=nc))
    T = _segsum(be, torch.cat([g.selfw.reshape(-1, 1), g.P], dim=1)[order], ptr)
    coarse = _Graph.from_entries(be, nc, cv[g.rows], cv[g.cols64], g.vals, T[:, 0].contiguous(), T[:, 1:], g.coef)
    comm = torch.zeros((nc,), dtype=torch.int64, device=ref.device)
    comm[cv] = labels.long()  # (all members of a refined community carry one label)
    smallest = torch.full((nv,), nc, dtype=torch.int64, device=ref.device)
    smallest = smallest.scatter_reduce(0, comm, torch.arange(nc, device=ref.device), "amin", include_self=True)
    return coarse, cv, smallest[comm].to(torch.int32)


def optimise(be, g0: _Graph, algorithm: str, rng, n_iterations: int = 1, diagnostics: Optional[dict] = None):
    """Membership [nv] (host int64, communities numbered by decreasing size), Q(final) and Q(singletons)."""
    nv0 = g0.nv
    dev = g0.P.device
    can_kernel = has(be, *_KERNEL_METHODS) and 1 <= g0.L <= be.cluster_max_layers()
    levels = []
    member = torch.arange(nv0, dtype=torch.int32, device=dev)
    for _ in range(n_iterations):
        g, labels = g0, member
        vmap = torch.arange(nv0, dtype=torch.int64, device=dev)
        while True:
            cls = rng.permutation(g.nv) % N_CLASSES
            rec = {"nv": g.nv, "nnz": int(g.vals.numel())}
            start = labels
            for kernel in ([True, False] if can_kernel else [False]):
                lv = _Level(be, g, cls, kernel)
                rec["route"] = "kernel" if kernel else "tensor"
                try:
                    t0 = time.perf_counter()
                    labels = lv.local_moving(start, rec)
                    moved = not bool(torch.equal(labels, start))
                    rec["local_seconds"] = time.perf_counter() - t0  # (every sweep ends in a read of its move count)
                    refined = lv.refine(labels, rec) if (moved and algorithm == "leiden") else labels
                    rec["seconds"] = time.perf_counter() - t0
                    break
                except _TableOverflow:
                    rec["overflow"] = True  # (a vertex met more communities than the table's entries)
                    rec["table"] = int(be.cluster_max_table())
            levels.append(rec)
            if not moved:
                break
            g, cv, labels = _aggregate(be, g, refined, labels)
            vmap = cv[vmap]
        member = labels[vmap]
    host = be.to_host(member).astype(np.int64)
    uniq, inv, counts = np.unique(host, return_inverse=True, return_counts=True)
    firsts = np.full(len(uniq), nv0, dtype=np.int64)
    np.minimum.at(firsts, inv, np.arange(nv0))
    rank = np.empty(len(uniq), dtype=np.int64)
    rank[np.lexsort((firsts, -counts))] = np.arange(len(uniq))
    groups = rank[inv.reshape(-1)] if nv0 else host
    final = be.to_device(np.ascontiguousarray(groups, dtype=np.int32), np.int32)
    q_final = quality(be, g0, final)
    q_single = quality(be, g0, torch.arange(nv0, dtype=torch.int32, device=dev))
    if diagnostics is not None:
        diagnostics["levels"] = levels
        diagnostics["path"] = levels[0]["route"] if levels else "tensor"
        diagnostics["q"] = q_final
        diagnostics["q_singletons"] = q_single
    return groups, q_final, q_single


# ---- the interface ----------------------------------------------------------------------------------------------------------------
_REQUIRED = object()


def _per_modality(value, mods, label: str, missing=_REQUIRED):
    """One entry per modality from a scalar (repeated), a sequence (its length must fit: ``AssertionError`` with the
    reference's text) or a mapping (a modality it lacks gets ``missing``, or raises ``KeyError`` when none is given);
    None for a falsy value."""
    if not value:
        return None
    if isinstance(value, Mapping):
        return [value[m] if missing is _REQUIRED else value.get(m, missing) for m in mods]
    if isinstance(value, Sequence) and not isinstance(value, str):
        if len(value) != len(mods):
            raise AssertionError(f"Length of {label} ({len(value)}) does not match the number of modalities ({len(mods)})")
        return list(value)
    return [value] * len(mods)


def _resolve_arguments(mods, resolution, mod_weights):
    """``(the resolution of each modality's layer - None where the call gives none -, the layer weights or None)``: what
    the reference hands to its partitions and to the optimiser (pinned by tests/golden/cluster_golden.npz)."""
    mods = list(mods)
    weights = _per_modality(mod_weights, mods, "layers_weights", missing=1)
    res = _per_modality(resolution, mods, "resolution")
    return ([None] * len(mods) if res is None else res), weights


def _choose_graph(adata, neighbors_key, what: str):
    if neighbors_key is None:
        key = "connectivities"
    else:
        try:
            key = adata.uns[neighbors_key]["connectivities_key"]
        except KeyError:
            raise ValueError(f'Did not find .uns["{neighbors_key}"]["connectivities_key"] for {what}. '
                             "Run `pp.neighbors` first.")
    if key not in adata.obsp:
        raise ValueError(f'Did not find .obsp["{key}"] for {what}. Run `pp.neighbors` first to compute a '
                         "neighborhood graph.")
    return adata.obsp[key]


def _edges(adjacency, use_weights: bool):
    """``(rows, cols, values, n)`` of the stored NON-ZERO entries (``adjacency.nonzero()`` drops the explicit zeros)."""
    A = csr_matrix(adjacency)
    if A.shape[0] != A.shape[1]:
        raise ValueError("the graph must be square")
    A.sum_duplicates()
    coo = A.tocoo()
    keep = coo.data != 0
    r, c = coo.row[keep], coo.col[keep]
    v = coo.data[keep].astype(np.float64) if use_weights else np.ones(int(keep.sum()), dtype=np.float64)
    return r, c, v, int(A.shape[0])


def _categorical(groups: np.ndarray) -> pd.Categorical:
    """The labels as strings, categories in numeric order."""
    ids = [int(g) for g in groups]
    return pd.Categorical([str(g) for g in ids], categories=[str(g) for g in sorted(set(ids))])


def _cluster(data, resolution, mod_weights, random_state, key_added, neighbors_key, directed, partition_type,
             partition_kwargs, algorithm, backend, diagnostics, kwargs):
    if not (is_anndata(data) or is_mudata(data)):
        raise TypeError("Expected a MuData object")
    kwargs = dict(kwargs)
    if "is_membership_fixed" in kwargs:
        raise NotImplementedError("muon_amd.tl.%s: fixed memberships (is_membership_fixed) are not supported" % algorithm)
    n_iterations = kwargs.pop("n_iterations", 1)
    if kwargs:
        raise TypeError(f"{algorithm}() got an unexpected keyword argument '{next(iter(kwargs))}'")
    if isinstance(n_iterations, bool) or not isinstance(n_iterations, (int, np.integer)) or n_iterations < 1:
        raise ValueError("n_iterations must be an integer >= 1")
    if partition_type is not None and partition_type != "RBConfigurationVertexPartition":
        raise NotImplementedError(f"muon_amd.tl.{algorithm}: only RBConfigurationVertexPartition is implemented, "
                                  f"not {partition_type!r}")
    partition_kwargs = dict(partition_kwargs)
    weights_arg = partition_kwargs.pop("weights", None)
    if partition_kwargs:
        raise NotImplementedError(f"muon_amd.tl.{algorithm}: partition_kwargs['{next(iter(partition_kwargs))}'] is not "
                                  "supported (only 'weights')")
    if weights_arg not in (None, "weight"):
        raise NotImplementedError(f"muon_amd.tl.{algorithm}: partition_kwargs['weights'] must be 'weight' (the stored "
                                  "values)")

    if is_anndata(data):
        # scanpy's call: one layer, the stored values are the weights, resolution None means 1
        layers = [_edges(_choose_graph(data, neighbors_key, "the AnnData object"), True)]
        gammas, lambdas = [1.0 if resolution is None else float(resolution)], [1.0]
    else:
        mods = list(data.mod.keys())
        res, layer_weights = _resolve_arguments(mods, resolution, mod_weights)
        layers = []
        for mod in mods:
            ad = data.mod[mod]
            if int(ad.n_obs) != int(data.n_obs):
                raise ValueError(f'modality "{mod}" holds {ad.n_obs} observations, the MuData object {data.n_obs}: '
                                 "multiplex clustering needs every modality to hold all of them")
            layers.append(_edges(_choose_graph(ad, neighbors_key, f'modality "{mod}"'), weights_arg == "weight"))
        gammas = [1.0 if x is None else float(x) for x in res]
        lambdas = [1.0] * len(mods) if layer_weights is None else [float(x) for x in layer_weights]
    if not layers:
        raise ValueError("no modality to cluster")
    n = layers[0][3]
    if any(l[3] != n for l in layers):
        raise ValueError("every modality's graph must have one row per observation")

    be = backend_or_default(backend)
    g0 = _build_graph(be, layers, lambdas, gammas, bool(directed))
    rng = np.random.default_rng(random_state)
    groups, q_final, q_single = optimise(be, g0, algorithm, rng, int(n_iterations), diagnostics)

    data.obs[key_added] = _categorical(groups)
    params = {"resolution": resolution, "random_state": random_state}
    if is_anndata(data):
        params.update(resolution=1 if resolution is None else resolution, n_iterations=int(n_iterations))
        data.uns[key_added] = {"params": params}
    else:
        params["partition_improvement"] = q_final - q_single
        data.uns[algorithm] = {"params": params}
    return None


def leiden(data, resolution=None, mod_weights=None, random_state: int = 0, key_added: str = "leiden",
           neighbors_key: Optional[str] = None, directed: bool = True, partition_type=None,
           partition_kwargs: Mapping[str, Any] = MappingProxyType({}), *, backend=None,
           diagnostics: Optional[dict] = None, **kwargs):
    """Cluster cells with the multiplex Leiden scheme of the module docstring (reference :1057-1130).

    MuData: one layer per modality from ``.obsp["connectivities"]`` (``neighbors_key``: from
    ``.obsp[.uns[neighbors_key]["connectivities_key"]]``).  ``resolution`` / ``mod_weights``: a scalar, a sequence or a
    mapping per modality, resolved as the reference does.  As in the reference every stored non-zero entry is an edge
    of weight 1 unless ``partition_kwargs={"weights": "weight"}``.  ``partition_type``: None or
    ``"RBConfigurationVertexPartition"``.  ``n_iterations`` (default 1) runs the optimiser again from its own result.
    Writes ``.obs[key_added]`` (a categorical of the labels as strings, communities numbered by decreasing size) and
    ``.uns["leiden"]["params"]`` with ``partition_improvement = Q(final) - Q(singletons)``; returns None.

    AnnData: one layer with scanpy's semantics (stored values are the weights, ``resolution=None`` means 1), results in
    ``.obs[key_added]`` and ``.uns[key_added]["params"]``.

    ``diagnostics=dict()`` receives ``levels`` (per level: ``nv``, ``nnz``, ``route``, ``sweeps``, ``refine_sweeps``,
    ``q``, ``local_seconds`` and ``seconds`` of steps 2-4; ``overflow`` and ``table`` where the kernel reported a full table), ``path`` (the route of level 0), ``q`` and ``q_singletons``.  Labels are not leidenalg's.
    """
    return _cluster(data, resolution, mod_weights, random_state, key_added, neighbors_key, directed, partition_type,
                    partition_kwargs, "leiden", backend, diagnostics, kwargs)


def louvain(data, resolution=None, mod_weights=None, random_state: int = 0, key_added: str = "louvain",
            neighbors_key: Optional[str] = None, directed: bool = True, partition_type=None,
            partition_kwargs: Mapping[str, Any] = MappingProxyType({}), *, backend=None,
            diagnostics: Optional[dict] = None, **kwargs):
    """Cluster cells with the multiplex Louvain scheme (reference :1133-1206): ``leiden`` without the refinement step.
    Same arguments and write-back, ``.uns["louvain"]``."""
    return _cluster(data, resolution, mod_weights, random_state, key_added, neighbors_key, directed, partition_type,
                    partition_kwargs, "louvain", backend, diagnostics, kwargs)
