#!/usr/bin/env python
"""The table-driven fill (csrc/tperm.hip) against the fill of csrc/tpack4.hip (tune tperm_off = 1) on the bench's matrix,
one process: cost of the plan + first fill, tiles of the schedule, equality of the two streams, and six fills of each
kernel, twice, interleaved (torch events around the call).  Writes one JSON line (profiles/r07_tperm_gate.json).
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


def timeit(off):
    hip.tune("tperm_off", off)
    ts = []
    for _ in range(6):
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
print(json.dumps(out))
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        f.write(json.dumps(out, indent=1))
