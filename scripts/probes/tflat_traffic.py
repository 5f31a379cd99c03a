#!/usr/bin/env python
"""The flat read-in fill (csrc/tflat.hip, `k_tflat_move`) four times on the bench's matrix for a counter pass: run under
rocprofv3 --pmc FETCH_SIZE (or WRITE_SIZE) and read the k_tflat_move dispatches (scripts/pmc_tflat.sh).  The operands are
made as lsi makes them: the TF-IDF scale sweep emits X's row stream, the first fill plans the table.
Usage: tflat_traffic.py [cells]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from muon_amd._atac.preproc import tfidf_device
from muon_amd._backend import HipBackend

be = HipBackend(0)
cells = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
X = be.synth_counts(0, cells, 200_000, 50, 0.03, 0)
out = torch.empty_like(X.values)
T = tfidf_device(be, X, cells, 3, 1e4, out=out, emit_stream=True)
xs, row_dst = be._xstream_of(T)
be.tune("tperm_flat", 1)
for _ in range(4):
    r = be.transpose_stream(T, src=(xs, row_dst))
    del r
    torch.cuda.synchronize()
tp = be._plan_of(T, "tplan")["tperm"]
assert isinstance(tp, dict) and "counts" in tp, "the flat fill did not run"
print(f"nnz {T.nnz} columns {T.shape[1]} row blocks {int(tp['toff'].numel() - 1)} tiles {tp['n_tiles']}")
