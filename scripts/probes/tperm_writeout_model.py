#!/usr/bin/env python
"""CPU model of the write-out of the table-driven fill (csrc/tperm.hip, r09): instructions per wave and tile of the
write-out BY COLUMN (what `k_t4_fill` in csrc/tpack4.hip does and `k_tperm_move` did before r09) and of the FLAT one, on
the bench generator's own columns.  What it counts are instructions a wave issues, not time: DESIGN 4.1 puts the measured
phases (scripts/probes/tperm_phases.py) next to these counts.

It draws a row block (512 cells) of the bench generator's matrix (csrc/synth.hip: depth ~ max(50, LogNormal(ln(1.15
density d), 0.3)), background Gamma(2, 1) per peak, 50 topics that up-weight 5 % of the peaks by Gamma(2, 1); an entry is
stored where its Poisson count is not 0), cuts it into tiles of `--tile` columns and takes the run lengths L[column].
  By column: a 16-lane group per column, group q of the workgroup's 64 takes columns q, q + 64, q + 128, q + 192 of a batch
    of 256 columns: per batch a wave reads 4 run words, 4 run targets and 4 staged pairs from the LDS and stores 4 times
    (lanes < L active; an instruction whose four columns are all empty is skipped), then per column a tail loop of
    ceil((L - 16) / 16) rounds - one LDS read and one store each - that the wave's four groups walk in lock step.
  Flat: lane i of the workgroup takes pair i, i + 1024, ...: per round a wave reads the staged pair and its column's
    target from the LDS and stores once; wave w has a round as long as 64 w + 1024 r lies below the tile's total.
No GPU, no library: numpy only."""
import argparse

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=512, help="rows of a row block")
ap.add_argument("--tile", type=int, default=512, help="columns of a tile")
ap.add_argument("--tiles", type=int, default=64, help="tiles per sampled block")
ap.add_argument("--blocks", type=int, default=4)
ap.add_argument("--densities", default="0.03")
ap.add_argument("--seed", type=int, default=0)
args = ap.parse_args()

D_PEAKS, N_TOPICS, NW = 200_000, 50, 16


def block(rng, density, n_cells, n_peaks):
    """stored[cell, peak] of a random block of the planted-topic matrix"""
    depth = np.maximum(50.0, rng.lognormal(np.log(1.15 * density * D_PEAKS), 0.3, n_cells))
    topic = rng.integers(0, N_TOPICS, n_cells)
    bg = rng.gamma(2.0, 1.0, n_peaks)
    w = rng.gamma(2.0, 1.0, (N_TOPICS, n_peaks)) * (rng.random((N_TOPICS, n_peaks)) < 0.05)
    p = 0.5 * bg[None, :] / (2 * D_PEAKS) + 0.5 * w[topic] / (0.1 * D_PEAKS)
    return rng.random((n_cells, n_peaks)) < -np.expm1(-depth[:, None] * p)


def by_column(L):
    """(stores, LDS reads, active lanes) of ALL waves for a tile with run lengths L[column]"""
    W = L.size
    stores = reads = lanes = 0
    for c0 in range(0, W, 256):
        Lb = np.zeros(256, dtype=np.int64)
        Lb[: min(256, W - c0)] = L[c0:c0 + 256]
        per = Lb.reshape(4, NW, 4)                       # [u, wave, group of the wave]
        live = (np.arange(c0, c0 + 256).reshape(4, NW, 4)[0] < W).any(axis=1)  # waves with a column in this batch
        reads += 12 * int(live.sum())
        stores += int((per.max(axis=2) > 0).sum())
        lanes += int(np.minimum(per, 16).sum())
        tail = -(-np.maximum(per - 16, 0) // 16)         # rounds of the tail loop per column
        stores += int(tail.max(axis=2).sum())
        reads += int(tail.max(axis=2).sum())
        lanes += int(np.maximum(per - 16, 0).sum())
    return stores, reads, lanes


def flat(L):
    T = int(L.sum())
    rounds = np.maximum(-(-(T - 64 * np.arange(NW)) // 1024), 0)
    return int(rounds.sum()), 2 * int(rounds.sum()), T


rng = np.random.default_rng(args.seed)
print("| density | tile | pairs per tile | pairs per run | write-out | global stores per wave and tile | lanes active | "
      "LDS reads per wave and tile |")
print("|---:|---:|---:|---:|---|---:|---:|---:|")
for dens in [float(x) for x in args.densities.split(",")]:
    acc = {"by column": np.zeros(3), "flat": np.zeros(3)}
    pairs = runs = tiles = 0
    for _ in range(args.blocks):
        stored = block(rng, dens, args.rows, args.tile * args.tiles)
        Ls = stored.sum(axis=0).reshape(args.tiles, args.tile)
        for L in Ls:
            acc["by column"] += by_column(L)
            acc["flat"] += flat(L)
            pairs += int(L.sum())
            runs += int((L > 0).sum())
            tiles += 1
    for name, (s, r, l) in acc.items():
        print(f"| {dens} | {args.tile} | {pairs / tiles:.0f} | {pairs / runs:.1f} | {name} | {s / tiles / NW:.1f} | "
              f"{100.0 * l / (64.0 * s):.0f} % | {r / tiles / NW:.1f} |")
