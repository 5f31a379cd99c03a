#!/usr/bin/env python
"""Times of the pieces ``muon_amd.pp.scrublet`` adds (csrc/scrublet.hip) and of the whole call on synthetic counts, each
next to its tensor formulation on the same device (self-contained; DESIGN.md 9.18 quotes its output).

Shapes: 100 000 x 20 000 cells x genes with 5 % of the entries stored - k_adj = 474, list + buffer = 1992 pairs per
query: the wide merge - and 20 000 x 20 000 - k_adj = 213, 948 pairs: the wave-wide merge of csrc/knn.hip, for
comparison; f32 counts made on the device (``synth_counts``).  Every step of every shape runs in a child process with
its own time limit (a step that hangs or faults ends the probe there and nothing else is started on the GPU).  Device
figures are EVENT-TIMED (stream events around the calls, best of ``reps`` windows after one warm-up), the whole call by
the host clock around a synchronised call.

  synth_ms / synth_tensor_ms       E_sim = E[p0] + E[p1] on the selected genes: ``csr_pair_rows`` (count, scan, fill)
                                   against ``pair_rows_tensor`` (gather, sort by (row, column), segmented sum); equal bytes?
  embed_ms / embed_tensor_ms       the simulated rows' scores: rows to 1e6, the f64 SpMM against D^-1 V and the row shift,
                                   against torch's sparse CSR product of the same operands
  merge_ms / merge_tensor_ms       one merge of list [kc] ++ buffer [cap] for 20 000 queries whose buffers hold kc
                                   candidates, with the merge kernel the shape takes (1992 pairs: ``knn_merge_wide``, 948:
                                   ``knn_merge``), against the tensor formulation (mask, two concatenations, top-k, gather)
  search_ms / search_tensor_ms     ``_candidates_filtered`` for one block of queries of [Z_obs; Z_sim] (30 columns) with
                                   the merge kernel the shape takes, against the same walk with the merges as tensor
                                   operations (mask, two concatenations, top-k over 4 kc columns, gather); same sets?
  call_s / call_tensor_s           ``pp.scrublet(adata)`` on a matrix that carries its device copy, and the same call on
                                   an operator set without ``csr_pair_rows`` and the merge kernels

Usage: python scripts/scrublet_probe.py [--shapes 100000x20000,20000x20000] [--density 0.05] [--reps 2] [--json PATH]
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

STEPS = {"synth": 240, "embed": 300, "merge": 240, "search": 400, "call": 400}  # seconds a step's child process may take
SEARCH_BLOCK = 20000


class Without:
    """the backend without the named operators (``has`` answers False for them)"""

    def __init__(self, be, *names):
        self._be, self._names = be, names

    def __getattr__(self, name):
        if name in self._names:
            raise AttributeError(name)
        return getattr(self._be, name)


def child(step: str, n: int, d: int, density: float, reps: int) -> dict:
    import numpy as np
    import torch
    from scipy.sparse import csr_matrix

    import muon_amd as mu
    from muon_amd._backend import get_backend
    from muon_amd._core import preproc as pp
    from muon_amd._core import scrublet as S
    from muon_amd._hostmatrix import attach_device

    be = get_backend()
    X = be.synth_counts(0, n, d, n_topics=50, density=density, seed=0)

    def events(fn, r=reps):
        out = fn()
        best = None
        for _ in range(r):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn()
            b.record()
            b.synchronize()
            t = a.elapsed_time(b)
            best = t if best is None else min(best, t)
        return best, out

    out = dict(step=step, n=n, d=d, nnz=int(X.nnz))
    n_sim = 2 * n
    k_adj = S.adjusted_k(n, n_sim)
    kc = k_adj + 8
    out.update(k_adj=k_adj, merge_pairs=kc + 3 * kc + 64)

    if step in ("synth", "embed"):
        genes = S.select_genes_device(be, X)
        E = pp.submatrix_device(be, X, None, genes)
        parents = S.draw_parents(n, 2.0, 0)
        p = be.to_device(parents, np.int64)
        out.update(genes=int(genes.sum()), e_nnz=int(E.nnz))
    if step == "synth":
        out["synth_ms"], got = events(lambda: be.csr_pair_rows(E, p))
        out["synth_tensor_ms"], want = events(lambda: S.pair_rows_tensor(E, p))
        out["sim_nnz"] = int(got.nnz)
        out["synth_equal"] = bool(torch.equal(got.indptr, want.indptr) and torch.equal(got.indices, want.indices)
                                  and torch.equal(got.values.view(torch.int32), want.values.view(torch.int32)))
    if step == "embed":
        Es = S.simulate_device(be, E, parents)
        g = torch.Generator(device=Es.values.device)
        g.manual_seed(0)
        M = torch.randn((E.shape[1], 30), dtype=torch.float64, device=Es.values.device, generator=g).contiguous()
        shift = torch.randn((30,), dtype=torch.float64, device=Es.values.device, generator=g)

        def kernels():
            return S._project(be, S._normalise(be, Es, 1e6, False), M) - shift

        def tensors():
            tot = torch.zeros(Es.shape[0], dtype=torch.float64, device=M.device)
            row = torch.repeat_interleave(torch.arange(Es.shape[0], device=M.device), Es.indptr[1:] - Es.indptr[:-1])
            tot.index_add_(0, row, Es.values.double())
            div = torch.where(tot > 0, tot / 1e6, torch.ones_like(tot))
            v = (Es.values.double() / div[row]).float().double()
            A = torch.sparse_csr_tensor(Es.indptr, Es.indices.long(), v, size=Es.shape)
            return A @ M - shift

        out["embed_ms"], got = events(kernels)
        out["embed_tensor_ms"], want = events(tensors)
        out["embed_max_rel_diff"] = float(((got - want).abs().max() / want.abs().max()).item())
    if step == "search":
        g = torch.Generator(device=X.values.device)
        g.manual_seed(1)
        Z = torch.randn((n + n_sim, 30), dtype=torch.float64, device=X.values.device, generator=g)
        Z += 3.0 * torch.randint(0, 4, (n + n_sim, 1), device=Z.device, generator=g)
        sq = (Z * Z).sum(dim=1)
        block = (0, min(SEARCH_BLOCK, n + n_sim))
        none = Without(be, "knn_merge", "knn_merge_wide")
        out["search_queries"] = block[1]
        out["search_ms"], got = events(lambda: pp._candidates_filtered(be, Z, sq, kc, 1 << 28, queries=block))
        out["search_tensor_ms"], want = events(lambda: pp._candidates_filtered(none, Z, sq, kc, 1 << 28, queries=block))
        out["search_same_sets"] = bool(torch.equal(torch.sort(got[0], dim=1).values, torch.sort(want[0], dim=1).values))
    if step == "merge":
        nq, cap = SEARCH_BLOCK, 3 * kc + 64
        g = torch.Generator(device=X.values.device)
        g.manual_seed(2)
        dev = X.values.device
        cur_d = torch.sort(torch.rand((nq, kc), dtype=torch.float64, device=dev, generator=g), dim=1).values
        cur_p = torch.randint(0, 3 * n, (nq, kc), device=dev, generator=g)
        buf_d = torch.rand((nq, cap), dtype=torch.float64, device=dev, generator=g)
        buf_pos = torch.randint(0, 3 * n, (nq, cap), device=dev, generator=g).to(torch.int32)
        cnt = torch.full((nq,), kc, dtype=torch.int32, device=dev)  # (what a panel usually leaves: about kc candidates)
        slot = torch.arange(cap, device=dev)[None, :]
        fn = be.knn_merge if kc + cap <= 1024 else be.knn_merge_wide

        def tensors():
            valid = slot < cnt[:, None]
            d_all = torch.cat([cur_d, torch.where(valid, buf_d, torch.full_like(buf_d, float("inf")))], dim=1)
            p_all = torch.cat([cur_p, buf_pos.long()], dim=1)
            t = torch.topk(d_all, kc, dim=1, largest=False)
            return t.values, torch.gather(p_all, 1, t.indices), t.values.amax(dim=1)

        out["merge_queries"] = nq
        out["merge_ms"], got = events(lambda: fn(cur_d, cur_p, buf_d, buf_pos, cnt))
        out["merge_tensor_ms"], want = events(tensors)
        out["merge_same_distances"] = bool(torch.equal(got[0], torch.sort(want[0], dim=1).values))
    if step == "call":
        m = csr_matrix((be.to_host(X.values), be.to_host(X.indices), be.to_host(X.indptr)), shape=(n, d))
        m.has_sorted_indices = True

        def clock(backend):
            attach_device(m, X, backend)
            ad = mu.AnnData(m)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mu.pp.scrublet(ad, backend=backend)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, ad

        clock(be)  # (warm-up: the first call pays for kernel loading and the allocator's growth)
        out["call_s"], ad = clock(be)
        out["threshold"] = ad.uns["scrublet"].get("threshold")
        out["call_tensor_s"], _ = clock(Without(be, "csr_pair_rows", "knn_merge", "knn_merge_wide"))
    return {k_: (round(v, 4) if isinstance(v, float) else v) for k_, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="100000x20000,20000x20000")
    ap.add_argument("--steps", default=",".join(STEPS))
    ap.add_argument("--density", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--step", default=None)
    args = ap.parse_args()
    if args.child:
        n, d = (int(v) for v in args.child.split("x"))
        print("RESULT " + json.dumps(child(args.step, n, d, args.density, args.reps)), flush=True)
        return 0
    results = []
    for shape in args.shapes.split(","):
        for step in args.steps.split(","):
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape, "--step", step, "--density",
                                    str(args.density), "--reps", str(args.reps)],
                                   capture_output=True, text=True, timeout=STEPS[step])
            except subprocess.TimeoutExpired:
                print(f"{shape} {step}: no result within {STEPS[step]} s", flush=True)
                return 1
            line = next((ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")), None)
            if r.returncode != 0 or line is None:
                print(f"{shape} {step}: exit status {r.returncode}\n{r.stderr[-3000:]}", flush=True)
                return 1  # (nothing else is started on the GPU after a step that failed)
            results.append(json.loads(line[7:]))
            print(json.dumps(results[-1]), flush=True)
            if args.json:
                with open(args.json, "w") as f:
                    json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
