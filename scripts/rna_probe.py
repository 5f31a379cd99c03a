#!/usr/bin/env python
"""Times of the RNA branch's device path on a synthetic count matrix (self-contained; DESIGN.md 9.14 quotes its output).

Shape: 100 000 x 20 000 cells x genes, 5 % of the entries stored (``synth_counts``, made on the device), k = 50.  In a
child process with its own time limit (a step that hangs or faults ends there and nothing else is started on the GPU).
Every figure is EVENT-TIMED, not a kernel time from a trace: stream events around the calls, best of ``reps`` windows,
warmed up once.  Single kernels (value sweep of log1p, moments, gram, col_moments, shift_cols, scale_rows) run 20 times
back to back inside a window and the figure is the window over 20: launch gaps are in it, and consecutive calls read
the same operand, of which the part that fits the 256 MB last-level cache need not come from HBM - the bytes/s figures
are an upper estimate of the HBM rate.

  normalize_ms / log1p_ms      the value sweep (HipBackend.value_sweep, csrc/rna.hip) with the row sums before it / alone
  transpose_ms, moments_ms     the CSR of X^T, and the per-gene sums on it (HipBackend.gene_moments); moments_gbs is the
                               bytes the sums need (values, indptr, outputs) over that time, moments_hbm_share against
                               the 8 TB/s HBM peak
  hvg_ms / hvg_tensor_ms       the device part of highly_variable_genes (transposition + kernel) against its tensor
                               formulation (index_add_) on the same device
  pca_ms / lsi_ms              tl.pca's device call (pca_device: moments, centred block Lanczos) against lsi_device on
                               the same matrix; centring_ms and centring_share are their difference, the products of
                               each run beside them (pca_spmm, lsi_spmm)
  *_k49_*                      the same pairs at k - 1, where the centred spectrum of the generator's 50 topics has its gap
  dense_niter{2,6}_ms          the densified route on the same device: centre the n x d f32 matrix, then
                               torch.pca_lowrank(q = k + 14, niter); its angle to tl.pca's top k - 1 subspace beside it;
                               densify_ms apart
  shift_cols_ms, scale_rows_ms the centring of an n x 64 image (col_moments' column sums + shift_cols; col_moments_ms
                               alone beside it, gram_ms: the other source of the column sums) / one scale_rows call on a
                               d x 64 block
  moments_plain_ms             gene_moments without the expm1 pair (what tl.pca asks for)

Usage: python scripts/rna_probe.py [--shape 100000x20000] [--density 0.05] [--k 50] [--reps 3] [--json PATH]
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
INNER = 20  # calls of a single kernel inside one timed window
HBM_PEAK = 8.0e12


def child(n: int, d: int, density: float, k: int, reps: int) -> dict:
    import numpy as np
    import torch

    from muon_amd._atac.tools import lsi_device
    from muon_amd._backend import get_backend
    from muon_amd._core.pca import pca_device
    from muon_amd._rna import preproc as R

    be = get_backend()
    C = be.synth_counts(0, n, d, n_topics=50, density=density, seed=0)

    def events(fn, r=reps, inner=1):
        # ms per call: `inner` calls back to back inside one window of stream events (single kernels: INNER calls, so
        # that the window is long against the launch and the events themselves), best of r windows, warmed up once
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

    out = dict(n=n, d=d, k=k, nnz=int(C.nnz))

    def normalize():
        tot = be.row_col_sums(C)[0]
        pos = tot > 0
        div = torch.where(pos, tot / tot[pos].median(), torch.ones_like(tot))
        return be.value_sweep(C, div=div)

    out["normalize_ms"], vals = events(normalize)
    N = C.with_values(vals)
    out["log1p_ms"], vals = events(lambda: be.value_sweep(N, log=True), inner=INNER)
    X = C.with_values(vals)
    del N, vals

    out["transpose_ms"], Xt = events(lambda: be.transpose(X))
    out["moments_ms"], (sums, _cnt) = events(lambda: be.gene_moments(Xt), inner=INNER)
    out["moments_plain_ms"], _ = events(lambda: be.gene_moments(Xt, with_e=False), inner=INNER)
    need = X.nnz * 4 + (d + 1) * 8 + d * 40
    for key in ("moments", "moments_plain"):
        out[f"{key}_gbs"] = need / (out[f"{key}_ms"] * 1e-3) / 1e9
        out[f"{key}_hbm_share"] = need / (out[f"{key}_ms"] * 1e-3) / HBM_PEAK
    del Xt
    out["hvg_ms"], (s_k, _c) = events(lambda: R.gene_moments_device(be, X))

    class NoKernel:  # the operator set without the moments kernel: gene_moments_device takes the tensor formulation
        gene_moments = gene_moments_max_blocks = None

        def __getattr__(self, name):
            return getattr(be, name)

    out["hvg_tensor_ms"], (s_t, _c) = events(lambda: R.gene_moments_device(NoKernel(), X))
    out["hvg_tensor_rel_dev"] = float(np.max(np.abs(s_k - s_t) / np.maximum(np.abs(s_t), 1e-300)))

    Y = be.randn(n, 64, 1)
    out["shift_cols_ms"], _ = events(lambda: be.shift_cols(Y, be.col_moments(Y, 0, n)[0] / n), inner=INNER)
    out["gram_ms"], _ = events(lambda: be.gram(Y), inner=INNER)
    out["col_moments_ms"], _ = events(lambda: be.col_moments(Y, 0, n), inner=INNER)
    Q = be.randn(d, 64, 2)
    sc = torch.rand(d, device=Q.device) + 0.5
    out["scale_rows_ms"], _ = events(lambda: be.scale_rows(sc, Q), inner=INNER)
    del Y, Q

    # k, and k - 1: the generator plants 50 topics, so the centred matrix has 49 directions above the noise and k = 50
    # cuts its spectrum where it has no gap, k = 49 at the gap
    V_pca = {}
    for kk, tag in ((k, ""), (k - 1, f"_k{k - 1}")):
        for key, fn in (("lsi", lambda: lsi_device(be, X, n_comps=kk, scale_embeddings=False, return_info=True)),
                        ("pca", lambda: pca_device(be, X, kk, return_info=True)),
                        ("pca_scale", lambda: pca_device(be, X, kk, scale=True, return_info=True))):
            ms, res = events(fn)
            out[f"{key}{tag}_ms"] = ms
            out[f"{key}{tag}_spmm"], out[f"{key}{tag}_iterations"] = int(res[-1]["spmm"]), int(res[-1]["iterations"])
            out[f"{key}{tag}_angle_bound"] = float(res[-1]["angle_bound"])
            if key == "pca":
                V_pca[kk] = res[1]
        out[f"centring{tag}_ms"] = out[f"pca{tag}_ms"] - out[f"lsi{tag}_ms"]
        out[f"centring{tag}_share"] = out[f"centring{tag}_ms"] / out[f"pca{tag}_ms"]

    try:
        def densify():
            return torch.sparse_csr_tensor(X.indptr, X.indices.long(), X.values, size=(n, d)).to_dense()

        out["densify_ms"], A = events(densify, 1)

        for niter in (2, 6):
            def dense_route():
                Ac = A - A.mean(dim=0, keepdim=True)
                return torch.pca_lowrank(Ac, q=k + 14, center=False, niter=niter)

            out[f"dense_niter{niter}_ms"], (_u, _s, Vd) = events(dense_route, 2)
            # how far the randomised route is from the converged one: largest principal angle between the top k - 1
            # right vectors (the subspace that has a gap behind it)
            Qa, _ = torch.linalg.qr(V_pca[k - 1].double())
            Qb, _ = torch.linalg.qr(Vd[:, :k - 1].double())
            sv = torch.linalg.svdvals(Qa.T @ Qb).clamp(max=1.0)
            out[f"dense_niter{niter}_angle_to_pca"] = float(torch.acos(sv.min()))
    except Exception as e:  # noqa: BLE001  (the comparison route is torch's own: its failure is reported, not hidden)
        out["dense_error"] = repr(e)[:300]
    return {k_: (round(v, 4) if isinstance(v, float) and v > 1e-3 else v) for k_, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="100000x20000")
    ap.add_argument("--density", type=float, default=0.05)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    n, d = (int(v) for v in args.shape.split("x"))
    if args.child:
        print("RESULT " + json.dumps(child(n, d, args.density, args.k, args.reps)), flush=True)
        return 0
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--shape", args.shape, "--density",
                            str(args.density), "--k", str(args.k), "--reps", str(args.reps)],
                           capture_output=True, text=True, timeout=LIMIT)
    except subprocess.TimeoutExpired:
        print(f"{args.shape}: no result within {LIMIT} s", flush=True)
        return 1
    line = next((ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")), None)
    if r.returncode != 0 or line is None:
        print(f"{args.shape}: exit status {r.returncode}\n{r.stderr[-3000:]}", flush=True)
        return 1
    result = json.loads(line[7:])
    print(json.dumps(result), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
