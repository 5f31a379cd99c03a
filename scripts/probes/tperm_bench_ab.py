#!/usr/bin/env python
"""bench.py with the tune key tperm_off preset (1 = the fill of csrc/tpack4.hip, 0 = the table-driven fill): before /
after step times on ONE build.  Usage: tperm_bench_ab.py 0|1 [bench.py arguments]"""
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from muon_amd import _ffi

assert _ffi.lib().mu_tune_set(b"tperm_off", int(sys.argv[1])) == 0
sys.argv = ["bench.py"] + sys.argv[2:]
runpy.run_path(os.path.join(ROOT, "bench.py"), run_name="__main__")
