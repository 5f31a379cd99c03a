#!/usr/bin/env python
"""Times of MEFISTO's eigen route (muon_amd/_core/mefisto.py, csrc/gp.hip) on the device (self-contained; DESIGN.md 6.4
quotes its output).

Per N (default 2 000, 10 000, 20 000), in a child process with its own time limit (a step that hangs or faults ends
there and nothing else is started on the GPU), stream events, best of 5, every timed call warmed up once, on a random
N x N f64 matrix (the passes' time does not depend on the values):

  project_ms / posterior_ms     HipBackend.gp_project (u = V^T r) / gp_posterior (m = V (g o u), diag C = (V o V) g)
  tensor_ms                     the tensor route of the same update: V.T @ r, V @ (g * u), (V * V) @ g
  project_frac / posterior_frac (N^2 8 bytes / 8 TB/s, the HBM's peak rate) / the kernel's time: the share of the least
                                time one read of V can take
  tensor_frac                   the same for the three passes together (three reads: 3 N^2 8 bytes)

and, for every N up to --fit-n (default 2 000: the eigendecompositions of a larger grid take minutes), one whole
iteration of a fit with K = 10 factors, two gaussian views of 300 and 200 features and n_grid = 4, under the GP prior,
with the kernels (iter_ms) and with the tensor route (iter_tensor_ms), as host time around a device synchronise.

Usage: python scripts/mefisto_probe.py [--n 2000,10000,20000] [--fit-n 2000] [--json PATH]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LIMIT = 420
HBM_BYTES_PER_S = 8.0e12


def child(n: int, fit: bool) -> dict:
    import numpy as np
    import torch

    from muon_amd._backend import get_backend
    from muon_amd._core.mefisto import SmoothMofaEngine

    be = get_backend()
    f64 = torch.float64

    def events(fn, reps=5):
        fn()
        best = None
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            t = a.elapsed_time(b)
            best = t if best is None else min(best, t)
        return best

    g = torch.Generator(device=be.device).manual_seed(0)
    V = torch.randn((n, n), dtype=f64, device=be.device, generator=g)
    r, gg, u = (torch.randn((n,), dtype=f64, device=be.device, generator=g) for _ in range(3))
    floor_ms = n * n * 8 / HBM_BYTES_PER_S * 1e3
    out = {"n": n, "floor_ms": floor_ms}
    out["project_ms"] = events(lambda: be.gp_project(V, r))
    out["posterior_ms"] = events(lambda: be.gp_posterior(V, gg, u))
    out["tensor_ms"] = events(lambda: (V.T @ r, V @ (gg * u), (V * V) @ gg))
    out["project_frac"] = floor_ms / out["project_ms"]
    out["posterior_frac"] = floor_ms / out["posterior_ms"]
    out["tensor_frac"] = 3 * floor_ms / out["tensor_ms"]
    del V
    if fit:
        rng = np.random.default_rng(0)
        t = np.sort(rng.random(n))
        z = np.column_stack([np.sin(2 * np.pi * (j + 1) * t) for j in range(4)])
        views = [z @ rng.standard_normal((4, d)) + rng.standard_normal((n, d)) for d in (300, 200)]
        for key, kernels in (("iter_ms", True), ("iter_tensor_ms", False)):
            eng = SmoothMofaEngine(be, views, ["gaussian"] * 2, np.zeros(n, dtype=int), 10, t, start_opt=1, n_grid=4,
                                   opt_freq=1000, seed=1)
            eng._kernels = eng._kernels and kernels
            for _ in range(3):  # (iteration 1 holds the one hyperparameter step; 2 runs under the prior it chose)
                eng.step()
            out["gp_factors"] = int(sum(s > 0 for s in eng.s))
            best = None
            for _ in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.step()
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                best = dt if best is None else min(best, dt)
            out[key] = best
            del eng
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="2000,10000,20000")
    ap.add_argument("--fit-n", type=int, default=2000)
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", type=int, default=None)
    args = ap.parse_args()
    if args.child is not None:
        print("RESULT " + json.dumps(child(args.child, args.child <= args.fit_n)), flush=True)
        return 0
    results = []
    for n in (int(x) for x in args.n.split(",")):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), "--fit-n", str(args.fit_n)],
                               capture_output=True, text=True, timeout=LIMIT)
        except subprocess.TimeoutExpired:
            print(f"N = {n}: no answer within {LIMIT} s; stopping here", flush=True)
            return 1
        line = next((l for l in r.stdout.splitlines() if l.startswith("RESULT ")), None)
        if r.returncode != 0 or line is None:
            print(f"N = {n}: exit status {r.returncode}; stopping here\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", flush=True)
            return 1
        results.append(json.loads(line[7:]))
        print(json.dumps(results[-1]), flush=True)
    print("| N | project ms (share) | posterior ms (share) | both ms | three tensor passes ms (share) | iteration ms: kernels / tensor |")
    print("|---|---|---|---|---|---|")
    for r in results:
        it = f"{r['iter_ms']:.2f} / {r['iter_tensor_ms']:.2f}" if "iter_ms" in r else "not measured"
        print(f"| {r['n']} | {r['project_ms']:.3f} ({100 * r['project_frac']:.0f} %) | {r['posterior_ms']:.3f} "
              f"({100 * r['posterior_frac']:.0f} %) | {r['project_ms'] + r['posterior_ms']:.3f} | {r['tensor_ms']:.3f} "
              f"({100 * r['tensor_frac']:.0f} %) | {it} |")
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
