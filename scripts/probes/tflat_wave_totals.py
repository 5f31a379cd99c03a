#!/usr/bin/env python
"""CPU model of the tile rule of the flat read-in fill (csrc/tflat.hip): the distribution of a wave's pairs per tile on
the bench generator's own matrix, and the share of tiles that the wave cap 64 R narrows, for several R.  A sibling of
tperm_writeout_model.py (the same draw of a row block of csrc/synth.hip's planted-topic matrix); the tile rule is the
numpy restatement the host test checks (tests/test_tflat_plan_host.py).  What it counts are pairs, not time.
No GPU, no library: numpy only."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests.test_tflat_plan_host import plan_block  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=512, help="rows of a row block")
ap.add_argument("--tile", type=int, default=480, help="widest tile (the bench shape's: 480 columns)")
ap.add_argument("--cols", type=int, default=480 * 48, help="columns drawn per block")
ap.add_argument("--blocks", type=int, default=6)
ap.add_argument("--density", type=float, default=0.03)
ap.add_argument("--rounds", default="8,9,10,12,16")
ap.add_argument("--seed", type=int, default=0)
args = ap.parse_args()

D_PEAKS, N_TOPICS, NW, CAP = 200_000, 50, 16, 9216


def block(rng, density, n_cells, n_peaks):
    """stored[cell, peak] of a random block of the planted-topic matrix (see tperm_writeout_model.py)"""
    depth = np.maximum(50.0, rng.lognormal(np.log(1.15 * density * D_PEAKS), 0.3, n_cells))
    topic = rng.integers(0, N_TOPICS, n_cells)
    bg = rng.gamma(2.0, 1.0, n_peaks)
    w = rng.gamma(2.0, 1.0, (N_TOPICS, n_peaks)) * (rng.random((N_TOPICS, n_peaks)) < 0.05)
    p = 0.5 * bg[None, :] / (2 * D_PEAKS) + 0.5 * w[topic] / (0.1 * D_PEAKS)
    return rng.random((n_cells, n_peaks)) < -np.expm1(-depth[:, None] * p)


rng = np.random.default_rng(args.seed)
blocks = [block(rng, args.density, args.rows, args.cols) for _ in range(args.blocks)]
rw = args.rows // NW
print(f"{args.blocks} row blocks of {args.rows} cells x {args.cols} peaks at density {args.density}, widest tile {args.tile}")
print("| R | wave cap | tiles | narrowed by the wave cap | narrowed by the staging buffer | wave total mean | p99 | max | "
      "rounds used per wave and tile |")
print("|---:|---:|---:|---:|---:|---:|---:|---:|---:|")
for R in [int(x) for x in args.rounds.split(",")]:
    tot, n_tiles, by_wave, by_cap = [], 0, 0, 0
    for st in blocks:
        indptr = np.concatenate([[0], np.cumsum(st.sum(1))])
        indices = np.nonzero(st)[1]
        tiles, counts, why = plan_block(indptr, indices, 0, args.rows, args.cols, args.tile, rw, 64 * R, CAP, reasons=True)
        n_tiles += len(tiles) - 1
        by_wave += sum(1 for w in why if w == "wave")
        by_cap += sum(1 for w in why if w == "stage")
        tot.append(counts.reshape(len(tiles) - 1, NW, rw).sum(2).ravel())
    tot = np.concatenate(tot)
    print(f"| {R} | {64 * R} | {n_tiles} | {100.0 * by_wave / n_tiles:.2f} % | {100.0 * by_cap / n_tiles:.2f} % | "
          f"{tot.mean():.0f} | {np.percentile(tot, 99):.0f} | {tot.max()} | {np.ceil(tot / 64).mean():.2f} |")
