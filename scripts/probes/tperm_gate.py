#!/usr/bin/env python
"""The table-driven fill (csrc/tperm.hip) against the fill of csrc/tpack4.hip (tune tperm_off = 1) on the bench's matrix,
one process: cost of the plan + first fill, tiles of the schedule, equality of the two streams, and six fills of each
kernel, twice, interleaved (torch events around the call).  Then the same for the flat read-in (csrc/tflat.hip, tune
tperm_flat = 1) against the table-driven fill: its plan, its tiles, equality, and seven fills of each, the first dropped,
twice, interleaved.  Writes one JSON line (profiles/r07_tperm_gate.json, profiles/r10_tflat_gate_*.json).
Usage: tperm_gate.py [cells] [out.json]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from muon_amd._backend import _p, check, get_backend

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
hip = get_backend()
X = hip.synth_counts(0, n, 200_000, 50, 0.03, 0)
xs, row_dst = hip.stream_layout(X)
with hip._dev_ctx():
    check(hip.lib.mu_csr_stream_fill(int(xs.perm.numel()), _p(xs.perm), _p(X.indptr), _p(X.indices), _p(X.values),
                                     _p(xs.sptr), _p(xs.ent), hip._stream()))
torch.cuda.synchronize()
out = {"n": n, "nnz": int(X.nnz)}
hip.tune("tperm_flat", 0)  # (the first half is the windowed read-in against csrc/tpack4.hip, as in r07)
t0 = time.perf_counter()
new = hip.transpose_stream(X, src=(xs, row_dst))
torch.cuda.synchronize()
out["first_fill_with_plan_s"] = time.perf_counter() - t0
tp = hip._plan_of(X, "tplan")["tperm"]
out["tiles"], out["tile_cols"], out["blocks"] = tp["n_tiles"], tp["tile_cols"], int(tp["toff"].numel() - 1)
widths = torch.diff(tp["tiles"].long())
widths = widths[widths > 0]  # (a block's closing boundary is followed by the next block's first column, 0)
out["tile_width_min_mean_max"] = [int(widths.min()), float(widths.float().mean()), int(widths.max())]
hip.tune("tperm_off", 1)
old = hip.transpose_stream(X, src=(xs, row_dst))
torch.cuda.synchronize()
out["equal"] = bool(torch.equal(old.ent[:X.nnz], new.ent[:X.nnz]) and torch.equal(old.sptr, new.sptr)
                    and torch.equal(old.perm, new.perm))
del old, new


def timeit(off, flat=0, fills=6):  # (flat = 0: the windowed read-in, what "new" meant when this probe was written)
    hip.tune("tperm_off", off)
    hip.tune("tperm_flat", flat)
    ts = []
    for _ in range(fills):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = hip.transpose_stream(X, src=(xs, row_dst))
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
        del r
    return ts


out["old_ms"], out["new_ms"], out["old_ms_again"], out["new_ms_again"] = timeit(1), timeit(0), timeit(1), timeit(0)
hip.tune("tperm_off", 0)
torch.cuda.empty_cache()
# the flat read-in: plan + first fill, its schedule, the same bytes, seven fills of each kernel (the first dropped)
hip.tune("tperm_flat", 1)
torch.cuda.synchronize()
t0 = time.perf_counter()
flat = hip.transpose_stream(X, src=(xs, row_dst))
torch.cuda.synchronize()
out["flat_first_fill_with_plan_s"] = time.perf_counter() - t0
tf = hip._plan_of(X, "tplan")["tperm"]
out["flat_tiles"], out["flat_rounds"] = tf["n_tiles"], int(hip.lib.mu_tflat_rounds())
widths = torch.diff(tf["tiles"].long())
widths = widths[widths > 0]
out["flat_tile_width_min_mean_max"] = [int(widths.min()), float(widths.float().mean()), int(widths.max())]
wave_tot = tf["counts"].view(-1, 32).long().sum(1)
out["flat_wave_total_mean_max"] = [float(wave_tot.float().mean()), int(wave_tot.max())]
hip.tune("tperm_flat", 0)
win = hip.transpose_stream(X, src=(xs, row_dst))
torch.cuda.synchronize()
out["flat_equal"] = bool(torch.equal(win.ent[:X.nnz], flat.ent[:X.nnz]) and torch.equal(win.sptr, flat.sptr)
                         and torch.equal(win.perm, flat.perm))
del win, flat, wave_tot, widths
torch.cuda.empty_cache()
for name, key in (("win_ms7", 0), ("flat_ms7", 1), ("win_ms7_again", 0), ("flat_ms7_again", 1)):
    out[name] = timeit(0, key, 7)[1:]
hip.tune("tperm_flat", 1)
print(json.dumps(out))
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        f.write(json.dumps(out, indent=1))
