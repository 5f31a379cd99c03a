"""TEST INFRASTRUCTURE: the CPU stand-in of tests/cpu_backend.py extended for the scale tests.

``CountingCpuBackend`` counts the calls of the operators the route tests ask about.  ``KernelCpuBackend`` additionally
implements ``scale_values`` / ``scale_dense_rows`` - by the NumPy statement of tests/scale_refs.py, entry by entry - so
that the branch host code takes behind ``has(be, "scale_values")`` runs without a GPU too; the plain stand-in leaves
both out and takes the tensor formulations.
"""
import collections

import numpy as np
import torch

from tests.cpu_backend import CpuTestBackend


class CountingCpuBackend(CpuTestBackend):
    def __init__(self):
        self.calls = collections.Counter()

    def upload_csr(self, *a, **k):
        self.calls["upload_csr"] += 1
        return super().upload_csr(*a, **k)


def _clip(t, lo, hi):
    with np.errstate(invalid="ignore"):
        return np.clip(t, lo, hi)


class KernelCpuBackend(CountingCpuBackend):
    def scale_values(self, X, mean, std, z, lo, hi, out=None):
        self.calls["scale_values"] += 1
        c = X.indices.numpy()
        t = _clip((X.values.numpy().astype(np.float64) - mean.numpy()[c]) / std.numpy()[c], lo, hi) - z.numpy()[c]
        res = torch.from_numpy(t.astype(X.values.numpy().dtype))
        if out is not None:
            out.copy_(res)
            return out
        return res

    def scale_dense_rows(self, X, mean, std, z, lo, hi, row_lo, row_hi, out=None):
        self.calls["scale_dense_rows"] += 1
        T = X.values.numpy().dtype
        blk = np.tile(z.numpy().astype(T), (row_hi - row_lo, 1))
        ip, idx, val = X.indptr.numpy(), X.indices.numpy(), X.values.numpy().astype(np.float64)
        for i in range(row_lo, row_hi):
            c = idx[ip[i]:ip[i + 1]]
            blk[i - row_lo, c] = _clip((val[ip[i]:ip[i + 1]] - mean.numpy()[c]) / std.numpy()[c], lo, hi).astype(T)
        res = torch.from_numpy(blk)
        if out is not None:
            out.copy_(res)
            return out
        return res
