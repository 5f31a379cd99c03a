#!/usr/bin/env python
"""Golden record of MEFISTO's option routing by EXECUTING the reference's own ``mofa()``.

The arithmetic of ``smooth_covariate`` is mofapy2's (absent here: parity unpinned) - but what muon hands to it is the
reference's own code (/root/reference/muon/_core/tools.py:529-597): the defaults ``smooth_kwargs`` is merged over, the
``set_covariates`` / ``set_smooth_options`` calls and the shape ``new_values`` takes on its way into ``predict_factor``.
This script runs the whole ``mofa()`` around the recording stand-in of make_mofa_golden.py, extended by those three
calls, on one seeded MuData object for three keyword sets, and writes what was recorded to mefisto_options_golden.npz:
one JSON document under the key ``record`` (this directory holds .npz fixtures and their makers only).
tests/test_mefisto_host.py compares ``muon_amd._core.tools._smooth_options`` with it.

Run (in the build container):  python tests/golden/make_mefisto_golden.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_mofa_golden as mg  # noqa: E402
from muon_amd._containers import AnnData, MuData  # noqa: E402


class SmoothRecorder(mg.RecordingEntryPoint):
    def set_covariates(self, *args, **kw):
        self.calls["set_covariates"] = {"args": list(args), "kwargs": kw}

    def set_smooth_options(self, **kw):
        self.calls["set_smooth_options"] = kw

    def predict_factor(self, **kw):
        self.calls["predict_factor"] = {k: np.asarray(v).tolist() for k, v in kw.items()}


def cases():
    return {
        "defaults": dict(smooth_covariate="time"),
        "list_scaled": dict(smooth_covariate=["time", "depth"], smooth_kwargs={"scale_cov": True, "n_grid": 7}),
        "new_values_1d": dict(smooth_covariate="time", smooth_kwargs={"new_values": [0.25, 0.5, 2.0]}),
    }


def mudata():
    rng = np.random.default_rng(5)
    n = 12
    names = np.array([f"cell{i:02d}" for i in range(n)])
    a1, a2 = AnnData(rng.standard_normal((n, 4))), AnnData(rng.standard_normal((n, 3)))
    a1.obs_names, a2.obs_names = names, names
    md = MuData({"rna": a1, "atac": a2})
    md.obs["time"] = np.arange(n, dtype=np.float64)
    md.obs["depth"] = rng.random(n)
    return md


def main():
    tools = mg.load_reference_tools()
    sys.modules["mofapy2.run.entry_point"].entry_point = SmoothRecorder
    record = {}
    for tag, kw in cases().items():
        tools.mofa(mudata(), use_var=None, n_factors=2, likelihoods="gaussian", quiet=True,
                   outfile=f"/tmp/golden_mefisto_{tag}.hdf5", **kw)
        calls = mg.RecordingEntryPoint.last.calls
        record[tag] = {"keywords": kw, "set_covariates": calls["set_covariates"],
                       "set_smooth_options": calls["set_smooth_options"], "predict_factor": calls.get("predict_factor")}
        print(tag, json.dumps(record[tag]))
    np.savez_compressed(os.path.join(HERE, "mefisto_options_golden.npz"), record=np.asarray(json.dumps(record, sort_keys=True)))
    print("wrote", os.path.join(HERE, "mefisto_options_golden.npz"))


if __name__ == "__main__":
    main()
