#!/usr/bin/env python
"""Times of muon_amd.tl.snf's device path on synthetic data (self-contained; DESIGN.md 9.9 quotes its output).

Shape: N = 20 000 cells, M = 2 modalities, k = 20, 20 iterations per step (the defaults of ``tl.snf``); the inputs are
cluster-structured points whose pairwise distances are computed on the device.  In a child process with its own time
limit (a step that hangs or faults ends there and nothing else is started on the GPU), stream events, best of 3:

  affinity_ms / normalize_ms / topk_ms / p_build_ms   the set-up kernels of csrc/snf.hip, per modality
  diffuse_ms          one ``Y = (P X)^T`` pass; an iteration is 2 M of them and M normalisations
  iteration_ms        one iteration of the kernel path;  step_ms: all ``--iterations`` of them
  dense_iteration_ms  one iteration of the dense tensor formulation, ``new @ S @ new.T`` through rocBLAS (the
                      straightforward port of the reference): 2 M products of N^3 multiply-adds
  *_tb_s              bytes that HAVE to move (every matrix the kernel reads or writes, once) per second, against the
                      8 TB/s roofline: affinity 5 N^2 doubles (pair pass 2, means 1, density 2), normalize 3 (row sums
                      1, pair pass 2), topk 1, diffuse 2 (one read of X, one write of Y - what the strip-major order is
                      meant to approach; the gather itself touches every row of X about k times)
  iteration_rel_dev   largest relative deviation between the two formulations after one iteration

Usage: python scripts/snf_probe.py [--n 20000] [--k 20] [--iterations 20] [--json PATH]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LIMIT = 540


def child(n: int, k: int, iterations: int) -> dict:
    import numpy as np
    import torch

    from muon_amd._backend import get_backend
    from muon_amd._core import snf as S

    be = get_backend()
    dev = be.device
    M = 2
    g = torch.Generator(device=dev).manual_seed(0)
    eps = float(np.finfo(np.float64).eps)

    def events(fn, reps=3):
        best = None
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn()
            b.record()
            b.synchronize()
            t = a.elapsed_time(b)
            best = t if best is None else min(best, t)
        return best, out

    out = dict(n=n, k=k, M=M, iterations=iterations)
    nn8 = n * n * 8
    tb_s = lambda doubles, ms: round(doubles * nn8 / ms / 1e9, 3)
    W, P = [], []
    for m in range(M):
        centres = torch.randn((8, 10 + m), generator=g, device=dev, dtype=torch.float64) * 2.5
        X = centres[torch.arange(n, device=dev) % 8] + torch.randn((n, 10 + m), generator=g, device=dev, dtype=torch.float64)
        D = S.pairwise_distances(X)
        w = be.empty((n, n), torch.float64)
        be.snf_affinity(D, k, 0.5, eps, out=w)  # (warm-up: the first launch loads the code object)
        ms, _ = events(lambda: be.snf_affinity(D, k, 0.5, eps, out=w))
        out["affinity_ms"], out["affinity_tb_s"] = round(ms, 3), tb_s(5, ms)
        del D
        raw = w.clone()
        ms, _ = events(lambda: be.snf_normalize(raw, out=w))
        out["normalize_ms"], out["normalize_tb_s"] = round(ms, 3), tb_s(3, ms)
        del raw
        ms, _ = events(lambda: be.snf_topk(w, k))
        out["topk_ms"], out["topk_tb_s"] = round(ms, 3), tb_s(1, ms)
        ms, (p, _rowsum) = events(lambda: S.dominate_csr(be, w, k))
        out["p_build_ms"] = round(ms, 3)
        out["p_max_row"] = int((p[0][1:] - p[0][:-1]).max())
        W.append(w)
        P.append(p)

    half = be.empty((n, n), torch.float64)
    nxt = [be.empty((n, n), torch.float64) for _ in range(M)]
    ms, _ = events(lambda: be.snf_diffuse(P[0], [W[1]], half))
    out["diffuse_ms"], out["diffuse_tb_s"] = round(ms, 3), tb_s(2, ms)

    def iteration(src, dst):
        for j in range(M):
            S.diffuse(be, P[j], [src[i] for i in range(M) if i != j], half)
            S.diffuse(be, P[j], [half], nxt[j])
        for j in range(M):
            be.snf_normalize(nxt[j], out=dst[j])

    first = [torch.empty_like(w) for w in W]
    ms, _ = events(lambda: iteration(W, first))
    out["iteration_ms"] = round(ms, 3)

    # the dense port of the same iteration
    new = []
    for m in range(M):
        indptr, cols, vals = P[m]
        rows = torch.repeat_interleave(torch.arange(n, device=dev), indptr[1:] - indptr[:-1])
        dense = torch.zeros((n, n), dtype=torch.float64, device=dev)
        dense[rows, cols.to(torch.int64)] = vals
        new.append(dense)

    def dense_iteration():
        res = []
        for j in range(M):
            s = torch.zeros_like(W[j])
            for i in range(M):
                if i != j:
                    s = s + W[i]
            res.append(S._normalize_torch(new[j] @ (s / (M - 1)) @ new[j].T))
        return res

    ms, ref = events(dense_iteration, reps=2)
    out["dense_iteration_ms"] = round(ms, 3)
    out["iteration_rel_dev"] = max(float(((a - b).abs() / b.abs()).max()) for a, b in zip(first, ref))
    out["dense_over_kernel"] = round(out["dense_iteration_ms"] / out["iteration_ms"], 1)
    del new, ref

    def step():
        cur = [w.clone() for w in W]
        for _ in range(iterations):
            iteration(cur, cur)
        return cur

    ms, _ = events(step, reps=2)
    out["step_ms"] = round(ms, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(child(args.n, args.k, args.iterations)), flush=True)
        return 0
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--n", str(args.n), "--k", str(args.k),
                            "--iterations", str(args.iterations)], capture_output=True, text=True, timeout=LIMIT)
    except subprocess.TimeoutExpired:
        print(f"no result within {LIMIT} s", flush=True)
        return 1
    line = next((ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")), None)
    if r.returncode != 0 or line is None:
        print(f"exit status {r.returncode}\n{r.stderr[-2000:]}", flush=True)
        return 1
    result = json.loads(line[7:])
    print(json.dumps(result), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
