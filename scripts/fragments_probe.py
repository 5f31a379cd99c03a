#!/usr/bin/env python
"""Kernel times and bytes moved of the three fragment tools on a synthetic table (self-contained; DESIGN.md 9.6 quotes
its output).

Default shape: 20 000 cells x 5 000 fragments (1e8 fragments, 24 contigs of 1e8 bp, a tenth of the barcodes are no
cells), generated and sorted ON THE DEVICE; 20 000 gene windows (2 kb upstream, genes of 5-60 kb) and 2 000 TSS.  In a
child process with its own time limit (a step that hangs or faults ends there and nothing else is started on the GPU):

  ranges_ms      mu_frag_ranges over the gene windows                      stream events, best of 3 after a warm-up
  overlap_ms     chunk scan + count + scan + emit (HipBackend.frag_overlap); 2 passes x 20 B per candidate
  csr_ms         key sort + duplicate sum + row pointers (torch), the canonical CSR of the triplets
  pileup_ms      mu_frag_pileup over the TSS windows; 20 B per candidate + two int32 atomics per passing fragment
  scan_ms        mu_frag_pileup_scan; 4 B x n x W read and written
  classes_ms     mu_frag_length_classes; 12 B per fragment + the cell table
  *_gbs          algorithmic bytes / time
  api_*_s        wall time of each public call, synchronised (host maps, uploads and downloads included)

The probe sets no pass / fail time: the feature has no parent to compare against.

Usage: python scripts/fragments_probe.py [--cells 20000] [--per-cell 5000] [--genes 20000] [--tss 2000] [--json PATH]
                                         [--limit SECONDS]
"""
import argparse
import json
import os
import subprocess
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_CONTIGS, CONTIG_LEN = 24, 100_000_000


def child(n_cells: int, per_cell: int, n_genes: int, n_tss: int) -> dict:
    import numpy as np
    import pandas as pd
    import torch

    import muon_amd as mu
    from muon_amd._atac import fragments as fr
    from muon_amd._backend import get_backend
    from muon_amd._core.io import device_csr_from_keys

    be = get_backend()
    dev = be.device
    n_frag = n_cells * per_cell
    n_bar = n_cells + n_cells // 10
    gen = torch.Generator(device=dev).manual_seed(0)
    key = (torch.randint(0, N_CONTIGS, (n_frag,), generator=gen, device=dev) << 32) + \
        torch.randint(0, CONTIG_LEN, (n_frag,), generator=gen, device=dev)
    key = torch.sort(key).values
    chrom, start = (key >> 32).to(torch.int32), (key & 0xFFFFFFFF).to(torch.int32)
    del key
    length = torch.randint(30, 600, (n_frag,), generator=gen, device=dev, dtype=torch.int32)
    end = start + length
    barcode = torch.randint(0, n_bar, (n_frag,), generator=gen, device=dev, dtype=torch.int32)
    score = torch.randint(1, 5, (n_frag,), generator=gen, device=dev, dtype=torch.int32)
    chrom_ptr = np.zeros(N_CONTIGS + 1, dtype=np.int64)
    chrom_ptr[1:] = np.cumsum(be.to_host(torch.bincount(chrom.long(), minlength=N_CONTIGS)))
    names = [f"bc{i}" for i in range(n_bar)]
    table = fr.FragmentTable(chrom, start, end, barcode, score, [f"chr{i + 1}" for i in range(N_CONTIGS)],
                             pd.Index(names), chrom_ptr, int(length.max().item()), 4, be)
    del length

    rng = np.random.default_rng(0)
    genes = pd.DataFrame({"Chromosome": [f"chr{i + 1}" for i in rng.integers(0, N_CONTIGS, n_genes)],
                          "Start": rng.integers(10_000, CONTIG_LEN - 100_000, n_genes)})
    genes["End"] = genes.Start + rng.integers(5_000, 60_000, n_genes)
    ad = mu.AnnData(np.zeros((n_cells, 1), dtype=np.float32), obs=pd.DataFrame(index=pd.Index(names[:n_cells])))
    mu.atac.tl.locate_fragments(ad, table)

    def events(fn, reps=3):
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

    gbs = lambda nbytes, ms: round(nbytes / (ms * 1e-3) / 1e9, 1)  # noqa: E731
    res = dict(n_cells=n_cells, n_fragments=n_frag, n_genes=n_genes, n_tss=n_tss, max_len=table.max_len)
    cell_of = be.to_device(fr.cell_table(ad, table), np.int32)

    # ---- count_fragments_features ---------------------------------------------------
    wchrom, wlo, whi = fr._windows(table, genes.Chromosome.values, genes.Start.values - 2000, genes.End.values)
    res["ranges_ms"], (lo, ln) = events(lambda: fr.window_ranges(table, wchrom, wlo, whi))
    cand = int(ln.sum().item())
    res["overlap_ms"], (keys, vals) = events(
        lambda: fr.overlap_triplets(table, cell_of, n_cells, wlo, whi, lo, ln, n_genes, True))
    res.update(gene_candidates=cand, gene_triplets=int(keys.numel()), overlap_bytes=2 * 20 * cand,
               overlap_gbs=gbs(2 * 20 * cand, res["overlap_ms"]))
    res["csr_ms"], X = events(lambda: device_csr_from_keys(keys, vals.long(), (n_cells, n_genes)))
    res["gene_nnz"] = X.nnz
    del keys, vals, X

    # ---- tss_enrichment ----------------------------------------------------------------
    tss = genes.iloc[:n_tss]
    W = 2001
    wchrom, wlo, whi = fr._windows(table, tss.Chromosome.values, tss.Start.values - 1000, tss.Start.values + 1000)
    lo, ln = fr.window_ranges(table, wchrom, wlo, whi)
    cand = int(ln.sum().item())
    res["pileup_ms"], diff = events(lambda: fr.pileup_diff(table, cell_of, n_cells, wlo, whi, lo, ln, W))
    res.update(tss_candidates=cand, pileup_bytes=20 * cand, pileup_gbs=gbs(20 * cand, res["pileup_ms"]))
    res["scan_ms"], _ = events(lambda: fr.pileup_scan(table, diff, 100, 500))  # (re-scans its own output: same traffic)
    res.update(scan_bytes=2 * 4 * n_cells * W, scan_gbs=gbs(2 * 4 * n_cells * W, res["scan_ms"]))
    del diff

    # ---- nucleosome_signal ---------------------------------------------------------------
    res["classes_ms"], _ = events(lambda: fr.length_classes(table, cell_of, n_cells, n_frag, 147, 294))
    res.update(classes_bytes=12 * n_frag, classes_gbs=gbs(12 * n_frag, res["classes_ms"]))

    # ---- the public calls -------------------------------------------------------------------
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", FutureWarning)
        res["api_count_s"], counts = wall(lambda: mu.atac.tl.count_fragments_features(ad, genes))
    assert counts.shape == (n_cells, n_genes)
    res["api_tss_s"], _ = wall(lambda: mu.atac.tl.tss_enrichment(ad, genes, n_tss=n_tss, random_state=0,
                                                                 return_tss=False))
    res["api_nucleosome_s"], _ = wall(lambda: mu.atac.tl.nucleosome_signal(ad))
    res["tss_score_median"] = float(np.nanmedian(ad.obs["tss_score"].values))  # (no enrichment in uniform fragments: ~1)
    res["nucleosome_signal_median"] = float(np.median(ad.obs["nucleosome_signal"].values))
    return {k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=20_000)
    ap.add_argument("--per-cell", type=int, default=5_000)
    ap.add_argument("--genes", type=int, default=20_000)
    ap.add_argument("--tss", type=int, default=2_000)
    ap.add_argument("--limit", type=int, default=600)
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(child(args.cells, args.per_cell, args.genes, args.tss)), flush=True)
        return 0
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--cells", str(args.cells),
                            "--per-cell", str(args.per_cell), "--genes", str(args.genes), "--tss", str(args.tss)],
                           capture_output=True, text=True, timeout=args.limit)
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
