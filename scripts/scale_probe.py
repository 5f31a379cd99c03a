#!/usr/bin/env python
"""Times of ``muon_amd.rna.pp.scale`` on a synthetic count matrix (self-contained; DESIGN.md 9.15 quotes its output).

Shapes: 100 000 x 20 000 and 100 000 x 2 000 cells x genes, 5 % of the entries stored (``synth_counts``, made on the
device, then log1p), ``max_value=10``, k = 50.  Each shape in a child process with its own time limit (a step that hangs
or faults ends there and nothing else is started on the GPU).  Device figures are EVENT-TIMED, not kernel times from a
trace: stream events around the calls, best of ``reps`` windows, warmed up once; single kernels run INNER times back to
back inside a window and the figure is the window over INNER, so launch gaps are in it, and consecutive calls read the
same operand, of which the part that fits the 256 MB last-level cache need not come from HBM: the rates are an upper
estimate of the HBM rate.  Whole calls that end on the host (``scale``, ``tl.pca``, the upload) are host-clock times
around work that ends in a device synchronise or a finished copy, best of ``reps``.

  values_ms, values_gbs, values_hbm_share      scale_values (csrc/scale.hip) over all stored entries; its algorithmic bytes
                                               (index, value in, value out: 12 B per entry, plus the three tables once)
                                               over that time, and against the 8 TB/s HBM peak
  dense_chunk_ms, dense_write_gbs, dense_write_hbm_share
                                               scale_dense_rows for one row chunk of the size ``scale`` uses (512 MiB);
                                               the bytes WRITTEN (rows x d x 4) over that time; dense_chunk_rows beside it
  fill_chunk_ms, dense_vs_fill                 torch's ``fill_`` of the same chunk buffer, timed the same way: the plain
                                               write rate of this device in this setting, and its time over the kernel's
  values_tensor_ms, dense_chunk_tensor_ms      the tensor formulations of both on the same device
  scale_s                                      the whole ``rna.pp.scale(adata, max_value=10)`` call on a matrix with a
                                               device copy: moments, every chunk and its device-to-host copy, the sparse
                                               form, the fingerprints; scale_fingerprint_s: the share spent hashing the
                                               dense result (the price of the validity rule), scale_gb: its size
  pca_form_s                                   ``tl.pca`` on that result through the remembered sparse form (no upload;
                                               the fingerprint check of the dense matrix is in it), pca_form_device_ms:
                                               its device part alone (pca_device on S), with products and iterations
  dense_upload_s, dense_route_ms               the route through a dense upload: the n x d matrix to the device, then
                                               centring and torch.pca_lowrank(q = k + 14, niter = 2) there

Usage: python scripts/scale_probe.py [--shapes 100000x20000,100000x2000] [--density 0.05] [--k 50] [--reps 3] [--json PATH]
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

LIMIT = 540
INNER = 20
HBM_PEAK = 8.0e12


def child(n: int, d: int, density: float, k: int, reps: int) -> dict:
    import numpy as np
    import torch
    from scipy.sparse import csr_matrix

    import muon_amd as mu
    from muon_amd._hostmatrix import attach_device
    from muon_amd._backend import get_backend
    from muon_amd._core.pca import pca_device
    from muon_amd._rna import preproc as R

    be = get_backend()
    C = be.synth_counts(0, n, d, n_topics=50, density=density, seed=0)
    X = C.with_values(be.value_sweep(C, log=True))
    del C

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

    def clock(fn, r=reps):
        best = out = None
        for _ in range(r):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
            best = t if best is None else min(best, t)
        return best, out

    out = dict(n=n, d=d, k=k, nnz=int(X.nnz), max_value=10.0)
    sums, _cnt = R.gene_moments_device(be, X, with_e=False)
    mean, std, centre, z, lo, hi = R.scale_tables(sums[0], sums[1], n, True, 10.0)
    tabs = [be.to_device(t, np.float64) for t in (centre, std, z)]

    out["values_ms"], S = events(lambda: be.scale_values(X, *tabs, lo, hi), inner=INNER)
    need = X.nnz * 12 + 3 * d * 8
    out["values_gbs"] = need / (out["values_ms"] * 1e-3) / 1e9
    out["values_hbm_share"] = need / (out["values_ms"] * 1e-3) / HBM_PEAK
    out["values_tensor_ms"], St = events(lambda: R.scale_values_tensor(X, *tabs, lo, hi))
    out["values_tensor_equal"] = bool(torch.equal(S, St))
    del St

    rows = min(n, max(1, R._DENSE_CHUNK_BYTES // (d * 4)))
    buf = be.empty((rows, d), torch.float32)
    out["dense_chunk_rows"] = rows
    out["dense_chunk_ms"], blk = events(lambda: be.scale_dense_rows(X, *tabs, lo, hi, 0, rows, out=buf), inner=5)
    out["dense_write_gbs"] = rows * d * 4 / (out["dense_chunk_ms"] * 1e-3) / 1e9
    out["dense_write_hbm_share"] = rows * d * 4 / (out["dense_chunk_ms"] * 1e-3) / HBM_PEAK
    out["fill_chunk_ms"], _ = events(lambda: buf.fill_(1.0), inner=5)
    out["dense_vs_fill"] = out["fill_chunk_ms"] / out["dense_chunk_ms"]
    blk = be.scale_dense_rows(X, *tabs, lo, hi, 0, rows, out=buf)
    out["dense_chunk_tensor_ms"], blk_t = events(lambda: R.scale_dense_rows_tensor(X, *tabs, lo, hi, 0, rows), 2)
    out["dense_tensor_equal"] = bool(torch.equal(blk, blk_t))
    del blk, blk_t, buf, S

    # the whole call, on a host matrix that carries the device copy
    def fresh():
        m = csr_matrix((be.to_host(X.values), be.to_host(X.indices), be.to_host(X.indptr)), shape=(n, d))
        m.has_sorted_indices = True
        attach_device(m, X, be)
        return mu.AnnData(m)

    best = None
    for _ in range(reps):
        ad = fresh()
        t, _ = clock(lambda: mu.rna.pp.scale(ad, max_value=10.0), 1)
        best = t if best is None else min(best, t)
    out["scale_s"] = best
    out["scale_gb"] = ad.X.nbytes / 1e9
    out["scale_fingerprint_s"], _ = clock(lambda: R._dense_fingerprint(ad.X))

    diag = {}
    out["pca_form_s"], _ = clock(lambda: mu.tl.pca(ad, n_comps=k, diagnostics=diag))
    out["pca_form_converged"], out["pca_form_spmm"] = bool(diag["converged"]), int(diag["spmm"])
    out["pca_form_iterations"] = int(diag["iterations"])
    Sf = R.scaled_form(ad.X)[0]
    out["pca_form_device_ms"], _ = events(lambda: pca_device(be, Sf, k, return_info=True))

    try:
        out["dense_upload_s"], A = clock(lambda: torch.from_numpy(ad.X).to(be.device))

        def dense_route():
            Ac = A - A.mean(dim=0, keepdim=True)
            return torch.pca_lowrank(Ac, q=k + 14, center=False, niter=2)

        out["dense_route_ms"], _ = events(dense_route, 2)
    except Exception as e:  # noqa: BLE001  (the comparison route is torch's own: its failure is reported, not hidden)
        out["dense_error"] = repr(e)[:300]
    return {k_: (round(v, 4) if isinstance(v, float) and v > 1e-3 else v) for k_, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="100000x20000,100000x2000")
    ap.add_argument("--density", type=float, default=0.05)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        n, d = (int(v) for v in args.child.split("x"))
        print("RESULT " + json.dumps(child(n, d, args.density, args.k, args.reps)), flush=True)
        return 0
    results = []
    for shape in args.shapes.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape, "--density",
                                str(args.density), "--k", str(args.k), "--reps", str(args.reps)],
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
