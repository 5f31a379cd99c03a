"""What MOFA's two engines share: the constants of the priors, the weight node's record and the driver base.

``MofaDriver`` owns the group layout of the samples, the collectives (one rule for where a collective's operand
lives), the initial expectations that the engines and the oracle (oracle/mofa_oracle.py init_state) create alike, the
single-graph step protocol and ``run`` / ``results``.  An engine supplies ``_iteration`` (one coordinate-ascent sweep,
device work only, the ELBO as a device scalar), ``variance_explained`` and - where it needs them - the three hooks of
``step``: ``_before_capture``, ``_capture_refused`` and ``_eager_step``.
"""
from __future__ import annotations

import warnings
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from .._comm import default_comm
from .._operators import has

A0 = 1e-14
B0 = 1e-14
TH_A0 = 1.0
TH_B0 = 1.0
TOL = {"fast": 5e-4, "medium": 5e-5, "slow": 5e-6}
# E ln theta = E ln(1 - theta) under the Beta(TH_A0, TH_B0) prior: where the sparsity nodes start
LN_THETA0 = float(torch.digamma(torch.tensor(1.0, dtype=torch.float64)) - torch.digamma(torch.tensor(2.0, dtype=torch.float64)))


def sparse_operands(be, X, width: int, dtype):
    """``(Xs, Xt)``: the operands of X Q and X^T Y for a sparse view X (a device CSR with values of ``dtype``) that a fit
    multiplies hundreds of times by dense blocks of ``dtype``, ``width`` (16 / 32 / 64) columns wide.  Laid out once, by
    the first rung that ``be`` and the shape allow:
      1. width 16: sliced ELL (csrc/spmm_ell.hip) - no per-row protocol is left in the product; X^T through the
         tile-staged transposition; f64: f32 stored values, hi + lo where some value is not exact in f32
      2. f32: row streams in both directions
      3. f64, width <= 32: the same row streams with f32 stored values, hi + lo
      4. the CSR itself and its general transpose"""
    wide = dtype == torch.float64
    if width == 16 and has(be, "ell16_pair", "ell16_fits") and be.ell16_fits(X, wide=wide):
        return be.ell16_pair(X, wide=wide)
    if dtype == torch.float32 and has(be, "can_stream") and be.can_stream(X, 16):
        Xt = be.transpose_stream(X)
        return be.stream(X), Xt
    if wide and has(be, "split_streams") and width <= 32 and min(X.shape) > 0:
        return be.split_streams(X)
    return X, be.transpose(X)


@dataclass(slots=True)
class WeightNode:
    """Expectations of one view's weights (D x K), noise precisions (G x D) and ARD / sparsity nodes (K)."""
    EW: torch.Tensor
    EW2: torch.Tensor
    gamma: torch.Tensor
    EWh2: torch.Tensor
    sig2: torch.Tensor
    tau: torch.Tensor
    ltau: torch.Tensor
    alpha: torch.Tensor
    lalpha: torch.Tensor
    lth: torch.Tensor
    l1mth: torch.Tensor
    a_alpha: Optional[torch.Tensor] = None

    @classmethod
    def initial(cls, D, K, G, dtype, small, dev):
        """``small``: the type of the K-long nodes (the general engine keeps them in f64 where they are tensor formulas)."""
        return cls(EW=torch.zeros((D, K), dtype=dtype, device=dev),
                   EW2=torch.ones((D, K), dtype=dtype, device=dev),
                   gamma=torch.ones((D, K), dtype=dtype, device=dev),
                   EWh2=torch.ones((D, K), dtype=dtype, device=dev),
                   sig2=torch.ones((D, K), dtype=dtype, device=dev),
                   tau=torch.ones((G, D), dtype=dtype, device=dev),
                   ltau=torch.zeros((G, D), dtype=dtype, device=dev),
                   alpha=torch.ones((K,), dtype=small, device=dev),
                   lalpha=torch.zeros((K,), dtype=small, device=dev),
                   lth=torch.full((K,), LN_THETA0, dtype=small, device=dev),
                   l1mth=torch.full((K,), LN_THETA0, dtype=small, device=dev))


class MofaDriver:
    def __init__(self, backend, groups, n_views: int, n_factors: int, comm, graph: bool):
        """``groups``: int [N], this rank's samples.  ``graph``: the engine's switch for capturing an iteration."""
        self.be = backend
        self.comm = default_comm(comm)
        self._hip = backend.name == "hip"
        self.K = int(n_factors)
        self.M = int(n_views)
        groups = np.asarray(groups, dtype=np.int64)
        self.N = len(groups)
        # (the group count is the ranks' maximum: a shard need not hold a sample of the last group)
        gmax = self._allreduce_max(torch.tensor([int(groups.max()) if groups.size else 0], dtype=torch.int64))
        self.G = G = int(gmax.item()) + 1
        # samples sorted by group (stable) so that every group is a contiguous row range
        self.perm = np.argsort(groups, kind="stable")
        gs = groups[self.perm]
        self.gslice = [(int(np.searchsorted(gs, g, "left")), int(np.searchsorted(gs, g, "right"))) for g in range(G)]
        self.Ng = self._allreduce(torch.tensor([b - a for a, b in self.gslice], dtype=torch.float64))
        self.elbo = []
        # an iteration without collectives inside, on a GPU: captured once into a HIP graph and replayed, so the host
        # only launches the graph and reads the ELBO back
        self._graph = None
        self._graph_elbo = None
        self._graph_ok = bool(self._hip and self.comm.world_size == 1 and graph)
        self._eager_steps = 0

    # -- collectives ------------------------------------------------------------------------------
    def _collective(self, op, ts):
        """``op`` over the ranks, in place.  The one rule for where a collective's operand lives: on the backend's device
        (a host tensor travels there and its result back)."""
        if self.comm.world_size > 1:
            moved = [t.to(self.be.device) if self._hip and not t.is_cuda else t for t in ts]
            op(*moved)
            for t, m in zip(ts, moved):
                if m is not t:
                    t.copy_(m)
        return ts[0] if len(ts) == 1 else ts

    def _allreduce(self, *ts):
        return self._collective(self.comm.all_reduce_sum, ts)

    def _allreduce_max(self, t):
        return self._collective(self.comm.all_reduce_max, (t,))

    def _all_ranks(self, flag: bool) -> bool:
        """True iff ``flag`` holds on EVERY rank (a per-shard property that selects a code path with collectives)."""
        if self.comm.world_size == 1:
            return bool(flag)
        bad = self._allreduce(torch.tensor([0.0 if flag else 1.0], dtype=torch.float64))
        return float(bad.item()) == 0.0

    # -- initial state (oracle/mofa_oracle.py init_state) ------------------------------------------
    def _draw_z0(self, seed, row_offset, n_total):
        """The seeded host draw of the factors' initial expectations: this rank's rows of the global draw, in group order."""
        n_total = self.N if n_total is None else int(n_total)
        z0 = np.random.default_rng(seed).standard_normal((n_total, self.K))
        return np.ascontiguousarray(z0[row_offset:row_offset + self.N][self.perm])

    def _init_nodes(self, z0, dtype, small):
        """Factors, one WeightNode per view and the factors' ARD node; ``small``: see WeightNode.initial."""
        self.EZ = self.be.to_device(z0).to(dtype)
        self.EZ2 = self.EZ ** 2 + 1.0
        self.sig2z = torch.ones_like(self.EZ)
        dev = self.EZ.device
        self.W = [WeightNode.initial(V.D, self.K, self.G, dtype, small, dev) for V in self.views]
        self.alpha_z = torch.ones((self.G, self.K), dtype=small, device=dev)
        self.lalpha_z = torch.zeros((self.G, self.K), dtype=small, device=dev)

    # -- driver --------------------------------------------------------------------------------
    def _before_capture(self):
        pass

    def _capture_refused(self):
        pass

    def _eager_step(self) -> torch.Tensor:
        out = self._iteration()
        self._eager_steps += 1
        return out

    def _capture(self):
        self._before_capture()
        torch.cuda.synchronize(self.be.device)
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g):
                out = self._iteration()
        except Exception as e:  # capture refused (e.g. a call that allocates or asks the device a question): stay eager
            warnings.warn(f"MOFA iteration not captured into a HIP graph ({e}); running eagerly")
            self._graph_ok = False
            self._capture_refused()
            return
        self._graph, self._graph_elbo = g, out

    def step(self):
        # (two eager iterations first: they answer the once-per-fit questions and warm the allocator)
        if self._graph is None and self._graph_ok and self._eager_steps >= 2:
            self._capture()
        if self._graph is not None:
            self._graph.replay()
            out = self._graph_elbo
        else:
            out = self._eager_step()
        e = float(out.item())
        self.elbo.append(e)
        return e

    def run(self, n_iterations=1000, convergence_mode="fast", min_iterations=2, callback=None):
        tol = TOL[convergence_mode]
        for it in range(n_iterations):
            self.step()
            if callback is not None:
                callback(it, self)
            if it >= min_iterations and len(self.elbo) >= 2:
                # (rank 0 decides: a rank that leaves alone strands the others in their next collective)
                if self.comm.agree(100.0 * abs((self.elbo[-1] - self.elbo[-2]) / self.elbo[0]) < tol):
                    break
        return len(self.elbo)

    def results(self, sort_factors=True):
        """Factors / weights on the host in the caller's sample order."""
        inv = np.empty_like(self.perm)
        inv[self.perm] = np.arange(self.N)
        Z = self.be.to_host(self.EZ)[inv].astype(np.float64)
        W = [self.be.to_host(w.EW).astype(np.float64) for w in self.W]
        r2 = self.variance_explained()
        order = np.arange(self.K)
        if sort_factors:
            order = np.argsort(-r2.sum(axis=(0, 1)), kind="stable")
        return {"Z": Z[:, order], "W": [w[:, order] for w in W], "r2": r2[:, :, order],
                "elbo": list(self.elbo), "order": order,
                "intercepts": [self.be.to_host(v.intercepts) for v in self.views]}
