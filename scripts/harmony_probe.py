#!/usr/bin/env python
"""Event-times the steps of muon_amd.pp.harmony_integrate on the device, kernels (csrc/harmony.hip) against the tensor
formulation of the same statement on the same device:

  * one ``assign`` block (5 % of the cells): harmony_assign against  S[b] * F[:, codes[b]].T, row-normalised, scattered
    into R, with S = exp(-D / sigma - rowmax) precomputed for the tensor side as its round does (the tensor round's
    cost of S is in the round's figure);
  * one ``gram``: R^T Zc over all cells, harmony_gram against R.T @ Zc;
  * a whole k-means round (Y, the 20 blocks, the objective) on either route;
  * the whole call (planted data, two Harmony iterations of at most five rounds) on either route, wall clock.

Shapes: N cells (default 10^5 and 10^6), K = 100, d = 50, B = 4.  Prints one JSON line per shape; every figure is the
median of ``--reps`` event-timed repetitions after one warm-up, in milliseconds.

Usage: python scripts/harmony_probe.py [--cells 100000 1000000] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from muon_amd._backend import HipBackend  # noqa: E402
from muon_amd._core import harmony as H  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def planted(N, d, C, B, seed=1):
    rng = np.random.default_rng(seed)
    cent = rng.normal(size=(C, d)) * 4
    sh = rng.normal(size=(B, d))
    sh = (sh - sh.mean(0)) * 1.5
    codes = rng.choice(B, size=N)
    return cent[rng.integers(C, size=N)] + sh[codes] + rng.normal(size=(N, d)) * 0.5, codes


def probe(be, N, reps, K=100, d=50, B=4):
    Z, codes = planted(N, d, 8, B)
    rs = np.random.RandomState(0)
    kr = H._Route(be, Z, [codes], [B], K, True)
    tr = H._Route(be, Z, [codes], [B], K, False)
    sig = be.to_device(np.full(K, 0.1), np.float64)
    th = be.to_device(np.full(B, 2.0), np.float64)
    Pr = be.to_device(np.bincount(codes, minlength=B) / N, np.float64)
    state = {}
    for name, r in (("kernel", kr), ("tensor", tr)):
        Zc = H._l2rows(r.Z)
        Y = H._l2rows(Zc[:: max(N // K, 1)][:K]).contiguous()
        R = r.first_assignment(Zc, Y, sig)
        O = r.level_sums(R)
        E = torch.outer(O.sum(dim=1), Pr)
        state[name] = (r, Zc, Y, R, E, O)
    res = {"cells": N, "K": K, "d": d, "B": B, "reps": reps}

    # one gram
    r, Zc, Y, R, E, O = state["kernel"]
    res["gram_kernel_ms"] = timed(lambda: r.gram(R, Zc), reps)
    rt, Zct, Yt, Rt, Et, Ot = state["tensor"]
    res["gram_tensor_ms"] = timed(lambda: rt.gram(Rt, Zct), reps)

    # one assign block
    blk = np.sort(rs.permutation(N)[: N // 20])
    idx = be.to_device(blk.astype(np.int64), np.int64)
    F = torch.pow((E + 1.0) / (O + 1.0), th).contiguous()
    res["assign_kernel_ms"] = timed(lambda: be.harmony_assign(Zc, Y, sig, F, r.codes, R, idx=idx, checked=True), reps)
    S = rt.weights(Zct, Yt, sig)

    def tensor_block():
        Rb = S[idx] * (rt.Phi[idx] @ F.T)
        Rt[idx] = Rb / Rb.sum(dim=1, keepdim=True)

    res["assign_tensor_ms"] = timed(tensor_block, reps)
    del S

    # a whole round
    for name in ("kernel", "tensor"):
        r, Zc, Y, R, E, O = state[name]

        def one_round():
            Yn = H._l2rows(r.gram(R, Zc)).contiguous()
            r.round_blocks(R, Zc, Yn, sig, E, O, Pr, th, np.array_split(rs.permutation(N), 20))
            r.objective(R, Zc, Yn, sig, E, O, th)

        res[f"round_{name}_ms"] = timed(one_round, max(reps // 2, 1))
    del state, kr, tr

    # the whole call
    for name, force in (("kernel", False), ("tensor", True)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = H._harmonize(be, Z, [codes], [B], nclust=K, max_iter_harmony=2, max_iter_kmeans=5, force_tensor=force)
        torch.cuda.synchronize()
        res[f"call_{name}_s"] = time.perf_counter() - t0
        assert out["route"] == name
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    be = HipBackend(0)
    for N in args.cells:
        line = json.dumps(probe(be, N, args.reps))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
