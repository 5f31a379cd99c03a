#!/usr/bin/env python
"""Times of the device steps under muon_amd.atac.tl.rank_peaks_groups on synthetic counts (self-contained; DESIGN.md 9.8
quotes its output).

One shape per run, given on the command line; the steps run in a child process with its own time limit (a step that
hangs or faults ends there and nothing else is started on the GPU).  Stream events, best of 5:

  transpose_ms      X -> X^T as a device CSR (transpose_csr)
  moments_ms        HipBackend.group_moments (csrc/rank.hip): sum, sum of squares and non-zero count per (peak, group)
  moments_tensor_ms the tensor formulation of the same table on the same device
  sort_ms           the per-row sort of X^T by value (two stable sorts per block of rows)
  ranks_ms          HipBackend.rank_sums on the sorted X^T
  ranks_tensor_ms   the tensor formulation of the same
  host_moments_ms / host_ranks_ms
                    the scipy / numpy restatement on the host (boolean-mask copies of the sparse matrix per group;
                    scipy.stats.rankdata per dense column), timed on the first --host-peaks peaks and scaled to all
                    of them (``host_scaled`` says so)

Usage: python scripts/rank_probe.py [--cells 100000] [--peaks 20000] [--density 0.02] [--groups 20] [--json PATH]
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


def child(args) -> dict:
    import numpy as np
    import scipy.sparse as sp
    import torch
    from scipy import stats

    from muon_amd._atac import rank as R
    from muon_amd._backend import get_backend

    be = get_backend()
    n, d, B = args.cells, args.peaks, args.groups
    X = be.synth_counts(0, n, d, density=args.density, seed=1)
    X.values.copy_(torch.log1p(X.values))
    lab = np.random.default_rng(0).integers(0, B, n).astype(np.int32)
    lab_d = be.to_device(lab, np.int32)

    def events(fn, reps=5):
        best, out = None, None
        for _ in range(reps):
            out = None
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn()
            b.record()
            b.synchronize()
            t = a.elapsed_time(b)
            best = t if best is None else min(best, t)
        return best, out

    be.transpose_csr(X)
    t_ms, Xt = events(lambda: be.transpose_csr(X), 3)
    nnz = Xt.nnz
    be.group_moments(Xt, lab_d, B)
    m_ms, mom = events(lambda: be.group_moments(Xt, lab_d, B))
    mt_ms, momt = events(lambda: R._moments_tensor(Xt, lab_d, B), 3)
    s_ms, Xs = events(lambda: R.sort_rows_by_value(Xt), 3)
    be.rank_sums(Xs, lab_d, B)
    r_ms, rk = events(lambda: be.rank_sums(Xs, lab_d, B))
    rt_ms, rkt = events(lambda: R._rank_sums_tensor(Xs, lab_d, B), 3)
    out = dict(cells=n, peaks=d, groups=B, nnz=nnz, transpose_ms=round(t_ms, 3), moments_ms=round(m_ms, 3),
               moments_gb_s=round(nnz * 8 / m_ms / 1e6, 1), moments_tensor_ms=round(mt_ms, 3), sort_ms=round(s_ms, 3),
               ranks_ms=round(r_ms, 3), ranks_gb_s=round(nnz * 8 / r_ms / 1e6, 1), ranks_tensor_ms=round(rt_ms, 3),
               moments_sum_rel_dev=float(((mom[0] - momt[0]).abs().max() / momt[0].abs().max()).item()),
               moments_nnz_equal=bool(torch.equal(mom[2], momt[2])),
               ranksum_equal=bool(torch.equal(rk[0], rkt[0])), zero_rank_equal=bool(torch.equal(rk[1], rkt[1])),
               # (t^3 - t is exact in f64 only while cells^3 < 2^53: above about 208 000 cells the two orders of adding round apart)
               tie_rel_dev=float(((rk[2] - rkt[2]).abs() / rkt[2].abs().clamp_min(1.0)).max().item()))

    # the host restatement on the first peaks
    hp = min(args.host_peaks, d)
    host = sp.csr_matrix((be.to_host(X.values), be.to_host(X.indices), be.to_host(X.indptr)), shape=(n, d))[:, :hp].tocsr()
    t0 = time.perf_counter()
    for b in range(B):
        sub = host[lab == b]
        sub.sum(axis=0), sub.multiply(sub).sum(axis=0), sub.getnnz(axis=0)
    out["host_moments_ms"] = round((time.perf_counter() - t0) * 1e3 * d / hp, 1)
    dense = host.toarray()
    t0 = time.perf_counter()
    ranks = stats.rankdata(dense, axis=0)
    for b in range(B):
        ranks[lab == b].sum(axis=0)
    out["host_ranks_ms"] = round((time.perf_counter() - t0) * 1e3 * d / hp, 1)
    out["host_scaled"] = f"timed on {hp} of {d} peaks"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=100000)
    ap.add_argument("--peaks", type=int, default=20000)
    ap.add_argument("--density", type=float, default=0.02)
    ap.add_argument("--groups", type=int, default=20)
    ap.add_argument("--host-peaks", type=int, default=200)
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(child(args)), flush=True)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT)
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
