#!/usr/bin/env python
"""CPU model of the row-stream SpMM's per-pass costs at Q slabs of 256 and 320 columns (csrc/spmm_win.hip, r08): what
was PREDICTED before the 320-column instances were measured (profiles/r08_spmm_slab_step_ab.md has the measurement).

It draws a block of the bench generator's matrix (csrc/synth.hip: depth ~ max(50, LogNormal(ln(1.15 density d), 0.3)),
background Gamma(2, 1) per peak, 50 topics that up-weight 5 % of the peaks by Gamma(2, 1); an entry is stored where its
Poisson count is not 0), sorts the rows by length, takes row-sets of four neighbours - the four rows a wave advances in
lock step - and counts the entries per (row, slab).  A pass gathers the window slots up to the longest of its four rows
in the kernel's batches (4 / 8 / 10 / 12 / 16 slots: "e-steps"); a row with 16 or more entries in the slab fills its
window and the row-set is revisited.  Cycles per pass and wave are DESIGN 4.2's accounting of the 256-column kernel:
32 (window wait) + 199 (stage A) + 261 (barrier + DMA landing) per pass, 80 x width / 256 DMA issue, 868 / 11.8 per
e-step, and a GUESSED 349 per revisit (a stage A and an exposed wait; nobody had measured it).
No GPU, no library: numpy only."""
import argparse

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=2048, help="rows of the sampled block")
ap.add_argument("--slabs", type=int, default=40, help="columns of the block: this many slabs of 1280 = lcm(256, 320)")
ap.add_argument("--densities", default="0.03,0.02,0.04,0.05")
ap.add_argument("--seed", type=int, default=0)
args = ap.parse_args()

D_PEAKS, N_CELLS, N_TOPICS = 200_000, 1_000_000, 50
FIXED, DMA, PER_E, REVISIT = 32 + 199 + 261, 80, 868 / 11.8, 349


def block(rng, density, n_cells, n_peaks):
    """stored[cell, peak] of a random block of the planted-topic matrix"""
    depth = np.maximum(50.0, rng.lognormal(np.log(1.15 * density * D_PEAKS), 0.3, n_cells))
    topic = rng.integers(0, N_TOPICS, n_cells)
    bg = rng.gamma(2.0, 1.0, n_peaks)
    w = rng.gamma(2.0, 1.0, (N_TOPICS, n_peaks)) * (rng.random((N_TOPICS, n_peaks)) < 0.05)
    p = 0.5 * bg[None, :] / (2 * D_PEAKS) + 0.5 * w[topic] / (0.1 * D_PEAKS)
    return rng.random((n_cells, n_peaks)) < -np.expm1(-depth[:, None] * p)


def slots(m):
    """window slots a pass gathers when the longest of its four rows has m (<= 16) entries in the slab"""
    return np.select([m == 0, m <= 4, m <= 8, m <= 10, m <= 12], [0, 4, 8, 10, 12], 16)


def model(stored, width):
    rows = stored[np.argsort(-stored.sum(axis=1), kind="stable")]
    n, c = rows.shape
    cnt = rows.reshape(n, c // width, width).sum(axis=2)                 # entries per (row, slab)
    sets = cnt[: n // 4 * 4].reshape(n // 4, 4, -1)                       # row-sets of four neighbours
    passes = sets.shape[0] * sets.shape[2]
    e_steps = used = revisits = 0
    left = sets.copy()
    first = True
    while True:
        live = left.max(axis=1) > 0 if not first else np.ones(left[:, 0].shape, bool)
        if not live.any():
            break
        take = np.minimum(left, 16)
        e_steps += int(slots(take.max(axis=1))[live].sum())
        used += int(take[np.broadcast_to(live[:, None, :], take.shape)].sum())
        again = (take == 16).any(axis=1) & live                          # a full window: maybe more in this slab
        left = np.where(again[:, None, :], left - take, 0)
        if not first:
            revisits += int(live.sum())
        first = False
    # (a revisit that finds nothing left still costs its stage A: it is counted above, with 0 slots)
    cycles = passes * (FIXED + DMA * width / 256) + PER_E * e_steps + REVISIT * revisits
    return dict(per_row_slab=cnt.mean(), e_per_pass=e_steps / passes, occupancy=used / max(4 * e_steps, 1),
                rev_per_pass=revisits / passes, cyc_per_entry=cycles / cnt[: n // 4 * 4].sum())


rng = np.random.default_rng(args.seed)
cols = 1280 * args.slabs
print("| density | direction | slab | entries per (row, slab) | e-steps per pass | slot occupancy | revisits per pass | "
      "modelled cycles per entry, 320 / 256 |")
print("|---:|---|---:|---:|---:|---:|---:|---:|")
for dens in [float(x) for x in args.densities.split(",")]:
    for name, stored in (("X.Q", block(rng, dens, args.rows, cols)), ("Xt.Y", block(rng, dens, cols, args.rows).T)):
        r = {w: model(stored, w) for w in (256, 320)}
        for w in (256, 320):
            m = r[w]
            ratio = f"{r[320]['cyc_per_entry'] / r[256]['cyc_per_entry']:.3f}" if w == 320 else ""
            print(f"| {dens} | {name} | {w} | {m['per_row_slab']:.1f} | {m['e_per_pass']:.1f} | {m['occupancy']:.3f} | "
                  f"{m['rev_per_pass']:.3f} | {ratio} |")
