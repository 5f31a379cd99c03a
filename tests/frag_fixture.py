"""TEST INFRASTRUCTURE: tests/golden/fragments_golden.npz (the reference's own fragment tools run on an engineered
table, tests/golden/make_fragments_golden.py) as the objects the fragment tests start from."""
import os

import numpy as np
import pandas as pd

from muon_amd import AnnData
from muon_amd import atac as ac

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fragments_golden.npz")
# tss_score and the normalised pileup: both sides divide exact integer sums in f64 and differ by at most three
# roundings (about 7e-16)
RTOL = 1e-13


def load():
    with np.load(PATH) as z:
        return {k: z[k] for k in z.files}


def features(g, tss: bool):
    """The feature frame of the count calls (without the gene on a contig the table lacks) or of the TSS calls."""
    f = pd.DataFrame({"Chromosome": g["feat_chrom"], "Start": g["feat_start"], "End": g["feat_end"]},
                     index=pd.Index(g["feat_names"]))
    return f if tss else f.iloc[:int(g["n_count_features"])]


def adata(g, backend, obs_names=None, with_table=True):
    names = g["obs_names"] if obs_names is None else obs_names
    a = AnnData(np.zeros((len(names), 1)), obs=pd.DataFrame(index=pd.Index(names)))
    if with_table:
        ac.tl.fragments_from_arrays(a, g["chrom"], g["start"], g["end"], g["barcode"], g["score"], backend=backend)
    return a


def max_rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape and np.array_equal(b == 0, a == 0)
    nz = b != 0
    return float(np.max(np.abs(a[nz] - b[nz]) / np.abs(b[nz]))) if nz.any() else 0.0
