#!/usr/bin/env python
"""Times of pp.qc_metrics + pp.filter_var + pp.filter_obs + atac.pp.tfidf + atac.tl.lsi from a RESIDENT matrix
(self-contained; DESIGN.md 9.5 quotes its output).

Default shape: 250 000 cells x 200 000 peaks of the bench generator (density 0.03), as a host CSR that carries its device
copy - what ``io.read_10x_arrays`` leaves behind.  In a child process with its own time limit (a step that hangs or
faults ends there and nothing else is started on the GPU):

  qc_ms          the QC sweep (HipBackend.csr_qc), stream events, best of 5, after a warm-up call
  sub_ms         count + scan + fill (HipBackend.csr_submatrix) for the selection the filters make, best of 3
  *_frac         the fraction of the 8 TB/s roofline from the algorithmic bytes: 8 B/entry read (qc), 8 B/entry read
                 + 8 B/kept entry written (submatrix)
  api_*_s        wall time of each API call, synchronised; ``api_filtered_s`` = filter_var + filter_obs + tfidf + lsi
  parent_*_s     the same selection made with scipy on the host (what the package did before: a new host matrix without
                 a device copy), then tfidf + lsi, which upload it again

Usage: python scripts/filter_probe.py [--cells 250000] [--peaks 200000] [--comps 50] [--json PATH] [--limit SECONDS]
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

ROOFLINE = 8.0e12  # bytes / s


def child(n: int, d: int, comps: int) -> dict:
    import numpy as np
    import torch
    from scipy.sparse import csr_matrix

    import muon_amd as mu
    from muon_amd._hostmatrix import attach_device
    from muon_amd._backend import get_backend

    be = get_backend()
    X = be.synth_counts(0, n, d)
    nnz = X.nnz

    def events(fn, reps):
        fn()  # warm-up
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

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    qc_ms, (row_nnz, _rs, col_nnz, _cs) = events(lambda: be.csr_qc(X), 5)
    cmask = be.to_host(col_nnz) >= 10
    rmask = be.to_host(row_nnz) >= int(np.median(be.to_host(row_nnz)) * 0.9)
    rows = be.to_device(np.nonzero(rmask)[0].astype(np.int64), np.int64)
    table = (np.cumsum(cmask, dtype=np.int64) - 1).astype(np.int32)
    table[~cmask] = -1
    table = be.to_device(table, np.int32)
    sub_ms, Y = events(lambda: be.csr_submatrix(X, rows, table, int(cmask.sum())), 3)
    kept = Y.nnz
    del Y
    res = dict(n_cells=n, n_peaks=d, nnz=nnz, kept_rows=int(rmask.sum()), kept_cols=int(cmask.sum()), kept_nnz=kept,
               qc_ms=round(qc_ms, 3), qc_frac=round(8.0 * nnz / (qc_ms * 1e-3) / ROOFLINE, 4),
               sub_ms=round(sub_ms, 3), sub_frac=round((8.0 * nnz + 8.0 * kept) / (sub_ms * 1e-3) / ROOFLINE, 4))

    host = csr_matrix((be.to_host(X.values), be.to_host(X.indices), be.to_host(X.indptr)), shape=X.shape)
    host.has_sorted_indices = True
    host.has_canonical_format = True
    attach_device(host, X, be)
    del X
    ad = mu.AnnData(host)
    thr = int(np.median(be.to_host(row_nnz)) * 0.9)
    res["api_qc_s"], _ = wall(lambda: mu.pp.qc_metrics(ad))
    res["api_filter_var_s"], _ = wall(lambda: mu.pp.filter_var(ad, "n_cells_by_counts", lambda x: x >= 10))
    res["api_filter_obs_s"], _ = wall(lambda: mu.pp.filter_obs(ad, "n_genes_by_counts", lambda x: x >= thr))
    res["api_tfidf_s"], _ = wall(lambda: mu.atac.pp.tfidf(ad))
    res["api_lsi_s"], _ = wall(lambda: mu.atac.tl.lsi(ad, n_comps=comps))
    res["api_filtered_s"] = sum(res[k] for k in ("api_filter_var_s", "api_filter_obs_s", "api_tfidf_s", "api_lsi_s"))
    shape = ad.shape
    del ad
    torch.cuda.empty_cache()

    # what the package did before: scipy makes a host matrix without a device copy; tfidf uploads it again
    res["parent_scipy_s"], sub = wall(lambda: host[:, cmask][rmask])
    assert sub.shape == shape
    ad = mu.AnnData(sub)
    res["parent_tfidf_s"], _ = wall(lambda: mu.atac.pp.tfidf(ad))
    res["parent_lsi_s"], _ = wall(lambda: mu.atac.tl.lsi(ad, n_comps=comps))
    res["parent_filtered_s"] = res["parent_scipy_s"] + res["parent_tfidf_s"] + res["parent_lsi_s"]
    # the re-upload alone: the filtered matrix over PCIe
    res["reupload_s"], _ = wall(lambda: be.upload_csr(sub.indptr, sub.indices, sub.data, sub.shape))
    return {k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=250_000)
    ap.add_argument("--peaks", type=int, default=200_000)
    ap.add_argument("--comps", type=int, default=50)
    ap.add_argument("--limit", type=int, default=900)
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(child(args.cells, args.peaks, args.comps)), flush=True)
        return 0
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--cells", str(args.cells), "--peaks",
                            str(args.peaks), "--comps", str(args.comps)], capture_output=True, text=True,
                           timeout=args.limit)
    except subprocess.TimeoutExpired:
        print(f"no result within {args.limit} s", flush=True)
        return 1
    line = next((ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")), None)
    if r.returncode != 0 or line is None:
        print(f"exit status {r.returncode}\n{r.stderr[-3000:]}", flush=True)
        return 1
    result = json.loads(line[7:])
    print(json.dumps(result), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
