#!/usr/bin/env python
"""Times of muon_amd.prot.pp.dsb's device path on synthetic counts (self-contained; DESIGN.md 9.4 quotes its output).

Base shape: 100 000 cells x 200 proteins (dense f64 counts on the device) and 500 000 empty droplets as a device CSR
(4 stored entries per droplet); also one tenth and ten times that.  Per shape, in a child process with its own time
limit (a step that hangs or faults ends there and nothing else is started on the GPU):

  wall_ms      _dsb_arrays, device matrices in, normalised device matrix out, synchronised (second call)
  moments_ms   the moments kernel (HipBackend.prot_log_moments), stream events, best of 5
  fit_ms       the fit kernel (HipBackend.prot_dsb_fit), stream events, best of 3
  iters        mean / max EM iterations per fit

Where scikit-learn is importable the reference's per-cell loop (two GaussianMixture fits, BIC, :189-198) is timed on
500 cells of the base panel on the host.

Usage: python scripts/prot_probe.py [--scales 0.1,1,10] [--json PATH]
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

N_CELLS, N_PROT, N_EMPTY = 100_000, 200, 500_000
LIMITS = {0.1: 180, 1.0: 300, 10.0: 600}


def child(scale: float) -> dict:
    import numpy as np
    import torch

    from muon_amd._backend import DeviceCSR, get_backend
    from muon_amd._prot import preproc as P

    be = get_backend()
    dev = be.device
    n, ne, d = int(N_CELLS * scale), int(N_EMPTY * scale), N_PROT
    g = torch.Generator(device=dev).manual_seed(0)
    ambient = torch.rand((d,), generator=g, device=dev, dtype=torch.float64) * 6 + 1
    level = torch.rand((n, 1), generator=g, device=dev, dtype=torch.float64) * 4 + 3
    cells = torch.poisson(ambient * level, generator=g)
    pos = torch.rand((n, d), generator=g, device=dev) < 0.25
    cells = cells + pos * torch.poisson(torch.full((n, d), 300.0, dtype=torch.float64, device=dev), generator=g)
    del pos
    # empty droplets: 4 entries per row in distinct ascending columns, small counts
    q = d // 4
    cols = (torch.randint(0, q, (ne, 4), generator=g, device=dev) + torch.arange(4, device=dev) * q).to(torch.int32)
    vals = torch.poisson(torch.full((ne * 4,), 2.0, dtype=torch.float64, device=dev), generator=g) + 1
    empty = DeviceCSR(torch.arange(ne + 1, device=dev, dtype=torch.int64) * 4, cols.reshape(-1).contiguous(), vals, (ne, d))

    def events(fn, reps):
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

    mom_ms, (mean, std) = events(lambda: be.prot_log_moments(empty, 10.0), 5)
    resp = be.to_device(np.random.RandomState(0).uniform(size=(d, 2)), np.float64)
    fit_ms, (_z, _bg, _bic, it) = events(lambda: be.prot_dsb_fit(cells, 10.0, mean, std, resp), 3)
    it = it.double()
    wall = None
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        P._dsb_arrays(cells, empty, random_state=0, backend=be)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
    return dict(scale=scale, n_cells=n, n_proteins=d, n_empty=ne, wall_ms=round(wall, 3), moments_ms=round(mom_ms, 4),
                fit_ms=round(fit_ms, 3), fit_us_per_cell=round(fit_ms * 1e3 / n, 4), iters_mean=round(float(it.mean()), 2),
                iters_max=int(it.max()))


def sklearn_loop(n_cells=500, d=N_PROT):
    try:
        from sklearn.mixture import GaussianMixture
    except ImportError:
        return None
    import warnings

    import numpy as np

    rng = np.random.default_rng(0)
    x = rng.standard_normal((n_cells, d)) + (rng.random((n_cells, d)) < 0.25) * 8.0
    tied = GaussianMixture(n_components=2, covariance_type="tied", init_params="random", random_state=0)
    full = GaussianMixture(n_components=2, covariance_type="full", init_params="random", random_state=0)
    t0 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for c in range(n_cells):
            v = x[c, :, np.newaxis]
            tied.fit(v)
            full.fit(v)
            tied.bic(v) < full.bic(v)
    return dict(sklearn_ms_per_cell=round((time.perf_counter() - t0) * 1e3 / n_cells, 3), n_cells=n_cells, n_proteins=d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", default="0.1,1,10")
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", type=float, default=None)
    args = ap.parse_args()
    if args.child is not None:
        print("RESULT " + json.dumps(child(args.child)), flush=True)
        return 0
    results = []
    for s in (float(v) for v in args.scales.split(",")):
        limit = LIMITS.get(s, 600)
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(s)], capture_output=True,
                               text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"scale {s}: no result within {limit} s; stopping", flush=True)
            break
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if r.returncode != 0 or line is None:
            print(f"scale {s}: exit status {r.returncode}; stopping\n{r.stderr[-2000:]}", flush=True)
            break
        results.append(json.loads(line[7:]))
        print(json.dumps(results[-1]), flush=True)
    ref = sklearn_loop()
    if ref is not None:
        print(json.dumps(ref), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(shapes=results, reference=ref), f, indent=1)
    return 0 if results else 1


if __name__ == "__main__":
    sys.exit(main())
