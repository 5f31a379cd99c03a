#!/usr/bin/env python
"""Times of muon_amd.atac.tl.scan_sequences' steps on random sequences and random count matrices whose lengths follow
JASPAR's (6 - 24 columns, mean 12) (self-contained; DESIGN.md 9.10 quotes its output).

One shape per run, given on the command line; the steps run in a child process with its own time limit (a step that
hangs or faults ends there and nothing else is started on the GPU).

  threshold_s       the host's threshold step for the whole bank (numpy dynamic programme, one matrix after the other)
  room_ms           HipBackend.motif_room (csrc/motif.hip), stream events, best of 3
  kernel_ms         HipBackend.motif_scan: room, count pass, exclusive scan, write pass - a host clock around a call that
                    ends in the read of the hit count and a device synchronise, best of 3 after one warm-up
  scan_ms           scan_sequences_device on the device-resident stream: the above plus the ordering, measured alike
  order_ms          scan_ms - kernel_ms: the two stable sorts and gathers that put the hits into the reference's row order
  tensor_s          the tensor formulation of the same scan on the same device (one run; --tensor-seqs N: on the first N
                    sequences, scaled to all of them, ``tensor_scaled`` says so)
  same_hits         the two paths return equal arrays (on the sequences the tensor formulation saw)
  mfma / useful_flop / mfma_floor_ms
                    v_mfma_f64_16x16x4_f64 issued by one pass (positions / 16 x sum over the bank's tiles of the tile's
                    longest motif), the look-up-and-add count of the statement (2 flop each) and the least time the
                    matrix cores need for the issued instructions at the f64 rate of DESIGN.md 9.10

Usage: python scripts/motif_probe.py [--seqs 100000] [--length 500] [--motifs 746] [--pvalue 1e-4] [--json PATH]
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

LIMIT = 900
F64_MFMA_FLOPS = 78.6e12  # MI355X f64 matrix peak


def random_bank(n, seed=0):
    import numpy as np

    from muon_amd._atac import motifs as Mo

    rng = np.random.default_rng(seed)
    lengths = 6 + rng.binomial(18, 1.0 / 3.0, size=n)  # 6 .. 24, mean 12
    mats = []
    for L in lengths:
        conc = rng.choice([0.05, 0.3, 2.0], size=L)  # sharp, middling and flat columns
        cols = [rng.multinomial(100, rng.dirichlet([c] * 4)) for c in conc]
        mats.append(Mo.log_odds(np.asarray(cols, dtype=np.float64).T))
    return mats


def child(args) -> dict:
    import numpy as np
    import torch

    from muon_amd._atac import motifs as Mo
    from muon_amd._backend import get_backend

    be = get_backend()
    mats = random_bank(args.motifs)
    t0 = time.perf_counter()
    thresholds = [Mo.scan_threshold(m, 4, args.pvalue) for m in mats]
    thr_s = time.perf_counter() - t0
    print(f"thresholds: {thr_s:.1f} s", file=sys.stderr, flush=True)
    scanner = Mo.MotifScanner(be, mats, thresholds)
    plain = Mo.MotifScanner(be, mats, thresholds, use_kernel=False)

    n, L = args.seqs, args.length
    g = torch.Generator(device=be.device).manual_seed(1)
    codes = torch.randint(0, 4, (n * L,), generator=g, device=be.device, dtype=torch.uint8)
    offsets = torch.arange(n + 1, device=be.device, dtype=torch.int64) * L

    def sync():
        torch.cuda.synchronize(be.device)

    be.motif_room(codes, offsets)
    room_ms = None
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        be.motif_room(codes, offsets)
        b.record()
        b.synchronize()
        room_ms = a.elapsed_time(b) if room_ms is None else min(room_ms, a.elapsed_time(b))

    be.motif_scan(codes, offsets, scanner.bank)
    sync()
    kernel_ms = None
    for _ in range(3):
        t0 = time.perf_counter()
        raw = be.motif_scan(codes, offsets, scanner.bank)
        sync()
        dt = (time.perf_counter() - t0) * 1e3
        kernel_ms = dt if kernel_ms is None else min(kernel_ms, dt)
    n_hits = int(raw[0].numel())
    Mo.scan_sequences_device((codes, offsets), scanner)
    sync()
    whole_ms = None
    for _ in range(3):
        t0 = time.perf_counter()
        got = Mo.scan_sequences_device((codes, offsets), scanner)
        sync()
        dt = (time.perf_counter() - t0) * 1e3
        whole_ms = dt if whole_ms is None else min(whole_ms, dt)
    print(f"kernel path: {kernel_ms:.1f} ms, {n_hits} hits", file=sys.stderr, flush=True)

    ts = n if args.tensor_seqs is None else min(args.tensor_seqs, n)
    sub = (codes[:ts * L], offsets[:ts + 1])
    t0 = time.perf_counter()
    want = Mo.scan_sequences_device(sub, plain)
    sync()
    tensor_s = (time.perf_counter() - t0) * n / ts
    m = int(want[0].numel())
    keep = got[0] < ts
    same = all(torch.equal(a[keep], b) for a, b in zip(got, want)) and int(keep.sum()) == m

    tiles = be.to_host(scanner.bank["tile_len"]).astype(np.int64)
    mfma = (n * L // 16) * int(tiles.sum())
    lookups = int(sum(max(L - m_.shape[1] + 1, 0) * m_.shape[1] for m_ in mats)) * n
    out = dict(seqs=n, length=L, motifs=args.motifs, columns=int(sum(m_.shape[1] for m_ in mats)), pvalue=args.pvalue,
               hits=n_hits, threshold_s=round(thr_s, 2), room_ms=round(room_ms, 3), kernel_ms=round(kernel_ms, 2),
               scan_ms=round(whole_ms, 2), order_ms=round(whole_ms - kernel_ms, 2), tensor_s=round(tensor_s, 2), same_hits=bool(same),
               mfma=mfma, useful_flop=2 * lookups, mfma_floor_ms=round(mfma * 2048 / F64_MFMA_FLOPS * 1e3, 2),
               lookups_per_s=round(lookups / (kernel_ms * 1e-3), 0))
    if ts < n:
        out["tensor_scaled"] = f"timed on {ts} of {n} sequences"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=100000)
    ap.add_argument("--length", type=int, default=500)
    ap.add_argument("--motifs", type=int, default=746)
    ap.add_argument("--pvalue", type=float, default=1e-4)
    ap.add_argument("--tensor-seqs", type=int, default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(child(args)), flush=True)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=LIMIT)  # (stderr passes: progress)
    except subprocess.TimeoutExpired:
        print(f"no result within {LIMIT} s", flush=True)
        return 1
    line = next((ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")), None)
    if r.returncode != 0 or line is None:
        print(f"exit status {r.returncode}", flush=True)
        return 1
    result = json.loads(line[7:])
    print(json.dumps(result), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
