#!/usr/bin/env python
"""Times muon_amd.tl.leiden / muon_amd.tl.louvain on one MI355X.

Two modalities, each the directed 15-nearest-neighbour graph (brute force on the device, f32) of a Gaussian mixture of
the same cells seen with different noise; stored values 1.  Per size and algorithm it prints one JSON line: wall time
of the call, per level (vertices, entries of S, route, sweeps, seconds) and per sweep of level 0, once on the kernel
path and once with the tensor formulation of the sub-round on the same device (a backend view without
``cluster_move``); the edge traffic of a level-0 sweep - 16 bytes per entry of S: column, weight and the gathered label
- against the 8 TB/s HBM peak; and networkx's ``louvain_communities`` on the CPU on the first modality at
``--networkx-cells`` cells with the modularity of both.  No hardware counters are collected.

    python scripts/cluster_probe.py --cells 100000 500000 --networkx-cells 20000
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from muon_amd import AnnData, MuData, tl  # noqa: E402
from muon_amd._backend import get_backend  # noqa: E402

HBM_PEAK = 8.0e12
K = 15


class TensorOnly:
    """The backend without ``cluster_move``: every level takes the tensor formulation; the segmented sums stay kernels."""

    def __init__(self, be):
        self._be = be

    def __getattr__(self, name):
        if name == "cluster_move":
            raise AttributeError(name)
        return getattr(self._be, name)


def knn_graph(X: torch.Tensor, k: int, chunk: int = 2048) -> sp.csr_matrix:
    n = int(X.shape[0])
    sq = (X * X).sum(dim=1)
    out = np.empty((n, k), dtype=np.int32)
    for r0 in range(0, n, chunk):
        r1 = min(n, r0 + chunk)
        d = sq[r0:r1, None] - 2.0 * (X[r0:r1] @ X.T) + sq[None, :]
        d[torch.arange(r1 - r0, device=X.device), torch.arange(r0, r1, device=X.device)] = float("inf")
        out[r0:r1] = torch.topk(d, k, dim=1, largest=False).indices.to(torch.int32).cpu().numpy()
    indptr = np.arange(0, n * k + 1, k, dtype=np.int64)
    return sp.csr_matrix((np.ones(n * k), out.reshape(-1), indptr), shape=(n, n))


def modalities(n: int, device, blocks: int = 30, dim: int = 10, seed: int = 0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    centres = torch.randn((blocks, dim), generator=g) * 2.5
    truth = torch.randint(0, blocks, (n,), generator=g)
    graphs = []
    for noise in (1.0, 1.4):
        X = (centres[truth] + noise * torch.randn((n, dim), generator=g)).to(device)
        graphs.append(knn_graph(X, K))
    return graphs


def mudata(graphs) -> MuData:
    mods = {}
    for m, A in enumerate(graphs):
        ad = AnnData(np.zeros((A.shape[0], 1), dtype=np.float32))
        ad.obsp["connectivities"] = A
        mods[f"m{m}"] = ad
    return MuData(mods)


def timed(fn, md, be, **kw):
    diag = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(md, backend=be, diagnostics=diag, **kw)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, diag


def report(n, graphs, be):
    for alg in ("leiden", "louvain"):
        for name, backend in (("kernel", be), ("tensor", TensorOnly(be))):
            fn = getattr(tl, alg)
            timed(fn, mudata(graphs), backend)  # first use: allocator and code objects
            wall, diag = timed(fn, mudata(graphs), backend)
            lv0 = diag["levels"][0]
            per_sweep = lv0["local_seconds"] / lv0["sweeps"]  # (includes the sweep's share of the Q evaluations)
            rec = {
                "cells": n, "algorithm": alg, "sub_round": name, "wall_s": round(wall, 4),
                "q": diag["q"], "levels": [
                    {k: (round(v, 5) if isinstance(v, float) else v) for k, v in l.items()} for l in diag["levels"]],
                "level0_sweep_ms": round(1e3 * per_sweep, 3),
                "level0_edge_bytes_per_sweep": 16 * lv0["nnz"],
                "level0_edge_rate_of_hbm_peak": round(16 * lv0["nnz"] / per_sweep / HBM_PEAK, 5),
            }
            print(json.dumps(rec), flush=True)


def networkx_compare(n, be):
    import networkx as nx

    A = modalities(n, be.device, seed=1)[0]
    G = nx.from_scipy_sparse_array(A, create_using=nx.DiGraph)
    t0 = time.perf_counter()
    parts = nx.community.louvain_communities(G, seed=0)
    t_nx = time.perf_counter() - t0
    ad = AnnData(np.zeros((n, 1), dtype=np.float32))
    ad.obsp["connectivities"] = A
    md = MuData({"m0": ad})
    timed(tl.louvain, md, be)
    wall, diag = timed(tl.louvain, md, be)
    lab = md.obs["louvain"].to_numpy().astype(str).astype(np.int64)
    ours = nx.community.modularity(G, [set(np.nonzero(lab == c)[0].tolist()) for c in np.unique(lab)])
    print(json.dumps({"cells": n, "networkx_louvain_s": round(t_nx, 2), "networkx_modularity": nx.community.modularity(G, parts),
                      "device_louvain_s": round(wall, 4), "device_modularity": ours}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs="+", default=[100000])
    ap.add_argument("--networkx-cells", type=int, default=20000)
    args = ap.parse_args()
    be = get_backend()
    for n in args.cells:
        t0 = time.perf_counter()
        graphs = modalities(n, be.device)
        print(json.dumps({"cells": n, "graph_generation_s": round(time.perf_counter() - t0, 2),
                          "entries_per_modality": int(graphs[0].nnz)}), flush=True)
        report(n, graphs, be)
    if args.networkx_cells:
        networkx_compare(args.networkx_cells, be)


if __name__ == "__main__":
    main()
