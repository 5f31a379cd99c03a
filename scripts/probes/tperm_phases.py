#!/usr/bin/env python
"""Phase accounting of the table-driven fill (csrc/tperm.hip, `mu_tperm_fill_phases`) and of its flat read-in
(csrc/tflat.hip, `mu_tflat_fill_phases`): shader cycles per tile and wave in top wait / header scan / staging / issue of
the next tile's loads (retire + window issue; scan + row search + issue) / barrier / write-out, on the bench generator's
matrix at 125 000 x 200 000 and at the bench shape.  An accounting instance writes the bytes of the production kernel
(checked here); its stamps cost cycles of their own, so the production kernel is timed next to it (torch events, six
fills).  The two kernels have schedules of their own: the tiles differ, so compare cycles per tile x tiles.
Usage: tperm_phases.py [cells ...]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from muon_amd._backend import _p, check, get_backend

NAMES = ["top wait", "header scan", "staging", "retire + window issue", "barrier", "write-out"]
hip = get_backend()
for n in [int(a) for a in sys.argv[1:]] or [125_000, 1_000_000]:
    X = hip.synth_counts(0, n, 200_000, 50, 0.03, 0)
    d = X.shape[1]
    xs, row_dst = hip.stream_layout(X)
    with hip._dev_ctx():
        check(hip.lib.mu_csr_stream_fill(int(xs.perm.numel()), _p(xs.perm), _p(X.indptr), _p(X.indices), _p(X.values),
                                         _p(xs.sptr), _p(xs.ent), hip._stream()))
    for flat in (0, 1):
        hip.tune("tperm_flat", flat)
        names = list(NAMES)
        names[3] = "scan + search + issue" if flat else NAMES[3]
        ref = hip.transpose_stream(X, src=(xs, row_dst))  # (makes the plan; the production kernel's bytes)
        plan = hip._plan_of(X, "tplan")
        tp = plan["tperm"]
        G = int(tp["toff"].numel() - 1)
        cnt = plan["work"][int(hip.lib.mu_tpack4_cnt_offset(n, d, X.nnz)):]
        ent = torch.empty_like(ref.ent)
        acct = torch.zeros((G * 16, 8), dtype=torch.int64, device=ent.device)
        fill, side = (hip.lib.mu_tflat_fill_phases, tp["counts"]) if flat else (hip.lib.mu_tperm_fill_phases, tp["cont"])
        with hip._dev_ctx():
            check(fill(n, d, X.nnz, _p(X.indptr), _p(row_dst), _p(xs.ent), _p(tp["cdst"]), _p(cnt), _p(tp["toff"]),
                       _p(tp["tiles"]), _p(side), _p(tp["slots"]), _p(ent), _p(acct), hip._stream()))
        torch.cuda.synchronize()
        same = bool(torch.equal(ent[:X.nnz], ref.ent[:X.nnz]))
        del ref, ent  # (at the bench shape a stream is 47 GiB: one at a time from here on)
        torch.cuda.empty_cache()
        a = acct.double()
        wave_tiles = float(a[:, 6].sum())  # (tile, wave) pairs
        per = a[:, :6].sum(0) / wave_tiles
        tot = float(per.sum())
        ts = []
        for _ in range(7):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = hip.transpose_stream(X, src=(xs, row_dst))
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
            del r
        ts = ts[1:]  # (the first one allocates its output)
        print(f"{'k_tflat_move' if flat else 'k_tperm_move'}: {n} x {d}, {X.nnz} entries, {G} row blocks, {tp['n_tiles']} "
              f"tiles; accounting instance writes the same bytes: {same}; production fill {min(ts):.2f}-{max(ts):.2f} ms",
              flush=True)
        for name, v in zip(names, per.tolist()):
            print(f"  {name:22s} {v:9.0f} cycles per tile and wave  {100.0 * v / tot:5.1f} %", flush=True)
        print(f"  {'sum':22s} {tot:9.0f}   x tiles / 1e6 = {tot * tp['n_tiles'] / 1e6:.0f}", flush=True)
        assert same
        plan.pop("tperm")  # (and one kernel's table at a time)
        del acct, plan, tp, cnt
        torch.cuda.empty_cache()
    hip.tune("tperm_flat", 1)
    del X, xs, row_dst
    torch.cuda.empty_cache()
