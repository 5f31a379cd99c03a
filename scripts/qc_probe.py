#!/usr/bin/env python
"""Times of the per-row QC sums (csrc/qc.hip) and of ``muon_amd.pp.qc_metrics(qc_vars=, percent_top=)`` on synthetic
count matrices (self-contained; DESIGN.md 9.16 quotes its output).

Shapes: 100 000 x 20 000 cells x genes, 5 % of the entries stored (the RNA branch's probe shape: rows of ~1000 entries)
and 20 000 x 200 000, 5 % stored (ATAC-like: rows of ~10 000 entries); f32 counts made on the device (``synth_counts``).
Each shape in a child process with its own time limit (a step that hangs or faults ends there and nothing else is started
on the GPU).  Device figures are EVENT-TIMED, not kernel times from a trace: stream events around the calls, best of
``reps`` windows, warmed up once; a kernel runs INNER times back to back inside a window and the figure is the window over
INNER, so launch gaps are in it.  Consecutive calls read the same operand, of which the part that fits the 256 MB
last-level cache need not come from HBM: the shares are an upper estimate of the HBM rate.

  qc_ms, qc_hbm_share                 the QC sweep (k_csr_qc) on the same matrix: 8 B per entry over that time against
                                      the 8 TB/s HBM peak - the yardstick the two new kernels stand next to
  masked1_ms, masked8_ms, *_hbm_share row_masked_sums at M = 1 and M = 8: 8 B per entry (index and value, once) plus the
                                      row pointers and the n x M f64 results
  top_ms, top_read_hbm_share          row_top_sums at (50, 100, 200, 500): the bytes the statement needs - every value
                                      once, 4 B per entry - over that time against the peak;
  top_moved_hbm_share                 the bytes the radix select moves - every value once per digit pass and once for the
                                      sums, 5 x 4 B per entry for f32, from L2 where the row still is there
  masked*_tensor_ms, top_tensor_ms    the tensor formulations of both on the same device (index_add_ per mask; segmented
                                      sort and cumulative sum), and whether they agree bit for bit (counts: exact)
  qc_metrics_s                        the whole ``pp.qc_metrics(adata, qc_vars=["mt"], percent_top=(50, 100, 200, 500))``
                                      call on a matrix that carries its device copy: host clock, the fingerprint check
                                      of the host matrix, both sweeps, the downloads and the frames
  qc_metrics_plain_s                  the same call without the two keywords

Usage: python scripts/qc_probe.py [--shapes 100000x20000,20000x200000] [--density 0.05] [--reps 3] [--json PATH]
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
INNER = 10
HBM_PEAK = 8.0e12
NS = (50, 100, 200, 500)


def child(n: int, d: int, density: float, reps: int) -> dict:
    import numpy as np
    import pandas as pd
    import torch
    from scipy.sparse import csr_matrix

    import muon_amd as mu
    from muon_amd._backend import get_backend
    from muon_amd._core.preproc import masked_sums_tensor, top_sums_tensor
    from muon_amd._hostmatrix import attach_device

    be = get_backend()
    X = be.synth_counts(0, n, d, n_topics=50, density=density, seed=0)
    nnz = int(X.nnz)

    def events(fn, r=reps, inner=1):
        out = fn()
        best = None
        for _ in range(r):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _i in range(inner):
                out = fn()
            b.record()
            b.synchronize()
            t = a.elapsed_time(b) / inner
            best = t if best is None else min(best, t)
        return best, out

    out = dict(n=n, d=d, nnz=nnz, mean_row=round(nnz / n, 1), max_row=int((X.indptr[1:] - X.indptr[:-1]).max()))
    share = lambda nbytes, ms: nbytes / (ms * 1e-3) / HBM_PEAK  # noqa: E731

    out["qc_ms"], _ = events(lambda: be.csr_qc(X), inner=INNER)
    out["qc_hbm_share"] = share(nnz * 8, out["qc_ms"])

    rng = np.random.default_rng(0)
    words = np.zeros(d, dtype=np.uint32)
    for b in range(8):
        words |= (rng.random(d) < 0.05).astype(np.uint32) << np.uint32(b)
    flags = be.to_device(words.view(np.int32), np.int32)
    for M in (1, 8):
        ms, got = events(lambda: be.row_masked_sums(X, flags, M), inner=INNER)
        out[f"masked{M}_ms"] = ms
        out[f"masked{M}_hbm_share"] = share(nnz * 8 + (n + 1) * 8 + n * M * 8 + d * 4, ms)
        out[f"masked{M}_tensor_ms"], want = events(lambda: masked_sums_tensor(X, flags, M), 2)
        out[f"masked{M}_tensor_equal"] = bool(torch.equal(got, want))
        del got, want

    ns = [v for v in NS if v <= d]
    out["top_ms"], got = events(lambda: be.row_top_sums(X, ns), inner=INNER)
    out["top_read_hbm_share"] = share(nnz * 4 + (n + 1) * 8 + n * len(ns) * 8, out["top_ms"])
    out["top_moved_hbm_share"] = share(5 * nnz * 4 + (n + 1) * 8 + n * len(ns) * 8, out["top_ms"])
    out["top_tensor_ms"], want = events(lambda: top_sums_tensor(X, ns), 2)
    out["top_tensor_equal"] = bool(torch.equal(got, want))
    del got, want

    # the whole call, on a host matrix that carries the device copy
    m = csr_matrix((be.to_host(X.values), be.to_host(X.indices), be.to_host(X.indptr)), shape=(n, d))
    m.has_sorted_indices = True
    attach_device(m, X, be)
    ad = mu.AnnData(m, var=pd.DataFrame({"mt": (words & 1).astype(bool)}, index=[f"g{j}" for j in range(d)]))

    def clock(fn, r=reps):
        best = None
        for _ in range(r):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
            best = t if best is None else min(best, t)
        return best

    out["qc_metrics_s"] = clock(lambda: mu.pp.qc_metrics(ad, qc_vars=["mt"], percent_top=ns))
    out["qc_metrics_plain_s"] = clock(lambda: mu.pp.qc_metrics(ad))
    out["pct_counts_mt_median"] = float(np.nanmedian(ad.obs["pct_counts_mt"].values))
    return {k_: (round(v, 4) if isinstance(v, float) else v) for k_, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="100000x20000,20000x200000")
    ap.add_argument("--density", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        n, d = (int(v) for v in args.child.split("x"))
        print("RESULT " + json.dumps(child(n, d, args.density, args.reps)), flush=True)
        return 0
    results = []
    for shape in args.shapes.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape, "--density",
                                str(args.density), "--reps", str(args.reps)],
                               capture_output=True, text=True, timeout=LIMIT)
        except subprocess.TimeoutExpired:
            print(f"{shape}: no result within {LIMIT} s", flush=True)
            return 1
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if r.returncode != 0 or line is None:
            print(f"{shape}: exit status {r.returncode}\n{r.stderr[-3000:]}", flush=True)
            return 1  # (nothing else is started on the GPU after a step that failed)
        results.append(json.loads(line[7:]))
        print(json.dumps(results[-1]), flush=True)
        if args.json:
            with open(args.json, "w") as f:
                json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
