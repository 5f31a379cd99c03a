#!/usr/bin/env python
"""Times muon_amd.tl.umap on one MI355X.

The graph is the symmetrised 15-nearest-neighbour graph (brute force on the device, f32) of a Gaussian mixture, with
seeded weights in (0, 1] so that only a part of the entries is active in an epoch.  Per size it prints JSON lines: the
wall time of ``tl.umap`` (random initialisation, ``--epochs`` epochs; the spectral one is timed apart) and the time of a
single epoch - the mean of ``--epochs`` epochs between two device synchronisations - once for the kernel and once for
the tensor formulation on the same device (a backend view without ``umap_epoch``); the entries visited per second
(every kept entry is visited in every epoch: its schedule is evaluated) and the epoch's streamed traffic - 12 bytes per
entry (column and period), the offsets, the read and the write of Y; the gathered rows of Y are left to the caches -
against the 8 TB/s HBM peak.  No hardware counters are collected.

    python scripts/umap_probe.py --cells 100000 1000000 --epochs 50
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
from muon_amd import AnnData, tl  # noqa: E402
from muon_amd._backend import get_backend  # noqa: E402
from muon_amd._core import umap as U  # noqa: E402

HBM_PEAK = 8.0e12
K = 15
AB = (0.58303002, 1.33416699)


class TensorOnly:
    """The backend without ``umap_epoch``: every epoch takes the tensor formulation; the segmented sums stay kernels."""

    def __init__(self, be):
        self._be = be

    def __getattr__(self, name):
        if name == "umap_epoch":
            raise AttributeError(name)
        return getattr(self._be, name)


def knn_graph(n: int, device, blocks: int = 30, dim: int = 10, seed: int = 0, chunk: int = 2048) -> sp.csr_matrix:
    g = torch.Generator(device="cpu").manual_seed(seed)
    centres = torch.randn((blocks, dim), generator=g) * 2.5
    X = (centres[torch.randint(0, blocks, (n,), generator=g)] + torch.randn((n, dim), generator=g)).to(device)
    sq = (X * X).sum(dim=1)
    idx = np.empty((n, K), dtype=np.int32)
    for r0 in range(0, n, chunk):
        r1 = min(n, r0 + chunk)
        d = sq[r0:r1, None] - 2.0 * (X[r0:r1] @ X.T) + sq[None, :]
        d[torch.arange(r1 - r0, device=device), torch.arange(r0, r1, device=device)] = float("inf")
        idx[r0:r1] = torch.topk(d, K, dim=1, largest=False).indices.to(torch.int32).cpu().numpy()
    w = np.random.default_rng(seed).uniform(0.02, 1.0, n * K)
    w[::K] = 1.0
    A = sp.csr_matrix((w, idx.reshape(-1), np.arange(0, n * K + 1, K, dtype=np.int64)), shape=(n, n))
    T = A.T.tocsr()
    A = (A + T - A.multiply(T)).tocsr()
    A.sort_indices()
    return A


def anndata(A) -> AnnData:
    ad = AnnData(np.zeros((A.shape[0], 1), dtype=np.float32))
    ad.obsp["connectivities"] = A
    ad.uns["neighbors"] = {"connectivities_key": "connectivities", "distances_key": "distances", "params": {}}
    return ad


def report(n, A, be, epochs):
    for name, backend in (("kernel", be), ("tensor", TensorOnly(be))):
        for init in ("random", "spectral"):
            if init == "spectral" and name == "tensor":
                continue  # (the initialisation does not depend on the epoch's formulation)
            diag = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tl.umap(anndata(A), maxiter=epochs, init_pos=init, a=AB[0], b=AB[1], backend=backend, diagnostics=diag)
            torch.cuda.synchronize()
            print(json.dumps({"cells": n, "epoch": name, "init_pos": init, "epochs": epochs, "path": diag["path"],
                              "tl_umap_wall_s": round(time.perf_counter() - t0, 4)}), flush=True)
        g = U._Graph(be, n, *U.edges(A, epochs))
        Y0 = U.initial_positions(be, g, "random", 2, 0)
        U.layout(backend, g, Y0, epochs, 1.0, 1.0, 5, AB[0], AB[1], 0, last_epoch=2)  # first use: code objects, allocator
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        U.layout(backend, g, Y0, epochs, 1.0, 1.0, 5, AB[0], AB[1], 0)
        torch.cuda.synchronize()
        per_epoch = (time.perf_counter() - t0) / epochs
        nnz = int(g.E.numel())
        traffic = 12 * nnz + 2 * 16 * n + 8 * n
        print(json.dumps({"cells": n, "epoch": name, "entries": nnz, "ms_per_epoch": round(1e3 * per_epoch, 4),
                          "entries_per_s": round(nnz / per_epoch), "streamed_bytes_per_epoch": traffic,
                          "share_of_hbm_peak": round(traffic / per_epoch / HBM_PEAK, 5)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--epochs", type=int, default=50)
    args = ap.parse_args()
    be = get_backend()
    for n in args.cells:
        t0 = time.perf_counter()
        A = knn_graph(n, be.device)
        print(json.dumps({"cells": n, "graph_generation_s": round(time.perf_counter() - t0, 2), "entries": int(A.nnz)}),
              flush=True)
        report(n, A, be, args.epochs)


if __name__ == "__main__":
    main()
