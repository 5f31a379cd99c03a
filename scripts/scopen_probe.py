#!/usr/bin/env python
"""Times of muon_amd.atac.pp.scopen's device path on synthetic peak matrices (self-contained; DESIGN.md 9.13 quotes its
output).

Shapes: 10 000 x 100 000 and 100 000 x 200 000 cells x peaks, 3 % of the entries stored (``synth_counts``, made on the
device), k = 30.  Per shape, in a child process with its own time limit (a step that hangs or faults ends there and
nothing else is started on the GPU), stream events, best of 5, every timed call warmed up once:

  sweep_w_ms / sweep_h_ms                 one fused sweep (HipBackend.nmf_cd_sweep, csrc/nmf.hip) over the d rows of W /
                                          the n rows of H^T (the H sweep also applies s and writes S H^T)
  sweep_w_tensor_ms / sweep_h_tensor_ms   the tensor formulation of the same steps (_sweep_torch) on the same device
  spmm_w_ms / spmm_h_ms                   the two products of an iteration, A_b^T (S H^T) and A_b W
  iter_ms                                 one whole iteration: two products, two fused sweeps, the violation on the host
  scopen_ms, n_iter                       a whole fit from init="random" with ``max_iter`` iterations at most
                                          (scopen_device: device CSR in, device factors out; no imputed matrix)
  scopen_tensor_ms                        the same with the tensor formulation of the sweep

Usage: python scripts/scopen_probe.py [--shapes 10000x100000,100000x200000] [--k 30] [--max-iter 20] [--json PATH]
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


def child(n: int, d: int, k: int, max_iter: int) -> dict:
    import numpy as np
    import torch

    from muon_amd._atac import scopen as S
    from muon_amd._backend import get_backend

    be = get_backend()
    X = be.synth_counts(0, n, d, n_topics=50, density=0.03, seed=0)

    def events(fn, reps=5):
        fn()
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

    # the operands of an iteration, as scopen_device makes them
    Ab = X.with_values((X.values > 0).to(torch.float64))
    n_open, _ = be.row_col_sums(Ab)
    _rho, s_host = S.scales(np.rint(be.to_host(n_open)), 0.0, 0.5)
    s = be.to_device(s_host, np.float64)
    At = be.transpose(Ab)
    kp = S.pad_width(k)
    W0, Ht0 = S._init_random(be, n, d, k, float(np.dot(s_host, be.to_host(n_open))) / (float(n) * d), 0)
    W, Ht = S._padded(be, W0, kp), S._padded(be, Ht0, kp)
    SHt = Ht * s[:, None]
    eye = torch.eye(k, dtype=torch.float64, device=W.device)
    G_w, G_h = Ht[:, :k].T @ Ht[:, :k] + eye, W[:, :k].T @ W[:, :k] + eye
    out = dict(n=n, d=d, k=k, nnz=int(X.nnz))

    out["spmm_w_ms"], B_w = events(lambda: be.spmm(At, SHt))
    out["spmm_h_ms"], B_h = events(lambda: be.spmm(Ab, W))
    # (a sweep updates its factor in place: both formulations are timed on a scratch factor that is refreshed, outside
    #  the events' window, before every call)
    for name, F, B, G, kw in (("w", W, B_w, G_w, {}), ("h", Ht, B_h, G_h, dict(bscale=s, oscale=s, out=SHt.clone()))):
        scratch = F.clone()

        def run(sweep):
            scratch.copy_(F)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            res = sweep(scratch, B, G, **kw)
            b.record()
            b.synchronize()
            return a.elapsed_time(b), res

        best = {}
        for key, sweep in (("", be.nmf_cd_sweep), ("_tensor", S._sweep_torch)):
            run(sweep)
            times = []
            for _ in range(5):
                t, res = run(sweep)
                times.append(t)
            best[key] = res
            out[f"sweep_{name}{key}_ms"] = min(times)
        out[f"sweep_{name}_viol_rel_dev"] = float(abs(best[""][1] - best["_tensor"][1]) / best["_tensor"][1])

    def iteration():
        g_w, v_w = be.nmf_cd_sweep(W, be.spmm(At, SHt), G_w)
        _g, v_h = be.nmf_cd_sweep(Ht, be.spmm(Ab, W), g_w + eye, bscale=s, oscale=s, out=SHt)
        return float(be.to_host(v_w + v_h)[0])

    out["iter_ms"], _ = events(iteration)
    del W, Ht, SHt, B_w, B_h, Ab, At

    for key, force in (("scopen_ms", False), ("scopen_tensor_ms", True)):
        info = {}
        ms, _ = events(lambda: S.scopen_device(be, X, k, max_iter=max_iter, init="random", force_tensor=force,
                                               diagnostics=info), 2)
        out[key] = ms
        out["n_iter" if not force else "n_iter_tensor"] = info["n_iter"]
        out["last_ratio" if not force else "last_ratio_tensor"] = float(info["ratios"][-1])
    return {k_: (round(v, 4) if isinstance(v, float) and v > 1e-3 else v) for k_, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="10000x100000,100000x200000")
    ap.add_argument("--k", type=int, default=30)
    ap.add_argument("--max-iter", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child is not None:
        n, d = (int(v) for v in args.child.split("x"))
        print("RESULT " + json.dumps(child(n, d, args.k, args.max_iter)), flush=True)
        return 0
    results = []
    for shape in args.shapes.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape, "--k", str(args.k),
                                "--max-iter", str(args.max_iter)], capture_output=True, text=True, timeout=LIMIT)
        except subprocess.TimeoutExpired:
            print(f"{shape}: no result within {LIMIT} s; stopping", flush=True)
            break
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if r.returncode != 0 or line is None:
            print(f"{shape}: exit status {r.returncode}; stopping\n{r.stderr[-2000:]}", flush=True)
            break
        results.append(json.loads(line[7:]))
        print(json.dumps(results[-1]), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(shapes=results), f, indent=1)
    return 0 if results else 1


if __name__ == "__main__":
    sys.exit(main())
