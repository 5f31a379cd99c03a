#!/usr/bin/env python
"""Times of muon_amd.tl.ica's device path on synthetic embeddings (self-contained; DESIGN.md 9.7 quotes its output).

Shapes: 100 000 x 50 and 1 000 000 x 50 (non-Gaussian sources under a random mixing, f64, on the device).  Per shape,
in a child process with its own time limit (a step that hangs or faults ends there and nothing else is started on the
GPU), stream events, best of 5:

  sweep_ms          one fused sweep (HipBackend.ica_sweep, csrc/ica.hip) on the whitened data
  sweep_tensor_ms   the tensor formulation of the same step on the same device (three passes, an n x k temporary)
  ica_ms            a whole tl.ica (_fastica_arrays: device basis in, device sources out) with the kernel
  ica_tensor_ms     the same with the tensor formulation of the sweep
  n_iter            iterations both runs took (equal, or the line says so)

Usage: python scripts/ica_probe.py [--rows 100000,1000000] [--k 50] [--json PATH]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LIMIT = 420


def child(n: int, k: int) -> dict:
    import warnings

    import numpy as np
    import torch

    from muon_amd._backend import get_backend
    from muon_amd._core import ica as I

    be = get_backend()
    dev = be.device
    g = torch.Generator(device=dev).manual_seed(0)
    u = torch.rand((n, k), generator=g, device=dev, dtype=torch.float64)
    S = torch.where(torch.arange(k, device=dev) % 2 == 0, torch.log(u / (1 - u)), (2 * u - 1) ** 3)  # logistic | cubed uniform
    X = (S / S.std(dim=0)) @ torch.randn((k, k), generator=g, device=dev, dtype=torch.float64) + 3.0
    del u, S

    def events(fn, reps=5):
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

    # the whitened data of this basis, as _fastica_arrays builds it
    kp = (k + 15) // 16 * 16
    Xc = X - X.mean(dim=0)
    d, uu = np.linalg.eigh(be.to_host(Xc.T @ Xc))
    K = (uu[:, ::-1] / np.sqrt(d[::-1])).T[:k]
    Z = torch.zeros((n, kp), dtype=torch.float64, device=dev)
    Z[:, :k] = (Xc @ be.to_device(np.ascontiguousarray(K), np.float64).T) * float(np.sqrt(n))
    del Xc
    W = be.to_device(I._sym_decorrelation(np.random.RandomState(0).normal(size=(k, k))), np.float64)
    be.ica_sweep(Z, W, "logcosh", 1.0)
    I._sweep_torch(Z, W, "logcosh", 1.0)
    sweep_ms, (A, gp) = events(lambda: be.ica_sweep(Z, W, "logcosh", 1.0))
    tensor_ms, (At, gpt) = events(lambda: I._sweep_torch(Z, W, "logcosh", 1.0))
    dev_a = float((A - At).abs().max() / At.abs().max())
    del Z

    out = dict(n=n, k=k, sweep_ms=round(sweep_ms, 4), sweep_tensor_ms=round(tensor_ms, 4), sweep_rel_dev=dev_a,
               sweep_gb_s=round(n * kp * 8 / sweep_ms / 1e6, 1))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for key, force in (("ica_ms", False), ("ica_tensor_ms", True)):
            diag = {}
            ms, _ = events(lambda: I._fastica_arrays(X, random_state=0, backend=be, force_tensor=force, diagnostics=diag), 3)
            out[key] = round(ms, 3)
            out["n_iter" if not force else "n_iter_tensor"] = diag["n_iter"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="100000,1000000")
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", type=int, default=None)
    args = ap.parse_args()
    if args.child is not None:
        print("RESULT " + json.dumps(child(args.child, args.k)), flush=True)
        return 0
    results = []
    for n in (int(v) for v in args.rows.split(",")):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), "--k", str(args.k)],
                               capture_output=True, text=True, timeout=LIMIT)
        except subprocess.TimeoutExpired:
            print(f"n = {n}: no result within {LIMIT} s; stopping", flush=True)
            break
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if r.returncode != 0 or line is None:
            print(f"n = {n}: exit status {r.returncode}; stopping\n{r.stderr[-2000:]}", flush=True)
            break
        results.append(json.loads(line[7:]))
        print(json.dumps(results[-1]), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(shapes=results), f, indent=1)
    return 0 if results else 1


if __name__ == "__main__":
    sys.exit(main())
