#!/usr/bin/env python
"""bench.py with a tune key preset: before / after step times on ONE build.  `0|1` presets tperm_off (1 = the fill of
csrc/tpack4.hip, 0 = the table-driven fill); `key=value` presets any key, e.g. tperm_flat=1 (the flat read-in of
csrc/tflat.hip).  Usage: tperm_bench_ab.py 0|1|key=value [bench.py arguments]"""
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from muon_amd import _ffi

key, _, value = sys.argv[1].rpartition("=")
assert _ffi.lib().mu_tune_set((key or "tperm_off").encode(), int(value)) == 0
sys.argv = ["bench.py"] + sys.argv[2:]
runpy.run_path(os.path.join(ROOT, "bench.py"), run_name="__main__")
