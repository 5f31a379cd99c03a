"""TEST INFRASTRUCTURE: tests/golden/fragments_golden.npz (the reference's own fragment tools run on an engineered
table, tests/golden/make_fragments_golden.py) as the objects the fragment tests start from; below them the inputs of
tests/test_gpu_fragments_stride.py, sized by the CU count."""
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


# ---- inputs that make the kernels of csrc/fragments.hip stride (tests/test_gpu_fragments_stride.py; anchored on the
# CPU by tests/test_fragments_host.py) ------------------------------------------------------------------------------
CHUNK = 256  # csrc/fragments.hip's candidates per work item


def wave_grid(n_cus):
    """waves csrc/fragments.hip's wave_grid(n, 4, 16) launches at most: a wave per work item, 4 to a block, 16 blocks per CU"""
    return 64 * n_cus


def thread_grid(n_cus):
    """threads k_frag_length_classes launches at most: 16 blocks of 256 per CU"""
    return 16 * n_cus * 256


def stride_table():
    """(frame of ~2 300 fragments on two contigs, names of 24 cells and of one without fragments): clusters of exactly
    700, 257, 256, 255 and 1 fragments, each further than the longest fragment from the next, one that a window
    starting below 0 covers, and 500 on the second contig; 37 barcodes of which every third is no cell"""
    rng = np.random.default_rng(6)
    rows = []

    def cluster(chrom, lo, hi, count):
        for s in np.sort(rng.integers(lo, hi, count)):
            rows.append((chrom, int(s), int(s) + int(rng.integers(20, 400)), f"b{int(rng.integers(0, 37))}",
                         int(rng.integers(1, 6))))

    cluster("a", 200, 900, 300)
    cluster("a", 100_000, 101_000, 256)
    cluster("a", 200_000, 201_000, 257)
    cluster("a", 300_000, 301_200, 700)
    cluster("a", 400_000, 401_000, 255)
    cluster("a", 500_000, 500_001, 1)
    cluster("b", 50_000, 51_000, 500)
    df = pd.DataFrame(rows, columns=["chrom", "start", "end", "barcode", "score"])
    df = df.sort_values(["chrom", "start"], kind="stable").reset_index(drop=True)
    return df, [f"b{i}" for i in range(37) if i % 3] + ["nobody"]


# (contig, centre, jitter) of the windows of width 1201 one round lays down: whole clusters (candidates 700, 257, 256,
# 255, 1, 300 with lo < 0, 500), two runs of windows without a candidate between them (an empty stretch of contig a and
# a contig the table lacks) and three windows that slide over the large cluster
_ROUND = [("a", 300_600, 0), ("a", 700_000, 0), ("zz", 1000, 0), ("a", 800_000, 0), ("a", 200_500, 0),
          ("a", 100_500, 0), ("a", 400_500, 0), ("a", 900_000, 0), ("a", 500_000, 0), ("a", 400, 0), ("b", 50_500, 0),
          ("a", 300_600, 500), ("a", 300_600, 150), ("b", 50_500, 400)]


def stride_windows(n_chunks_wanted):
    """(contig names, lo, hi int64): rounds of ``_ROUND`` until the windows' candidates, cut into chunks of 256, make
    at least ``n_chunks_wanted`` chunks"""
    df, _ = stride_table()
    max_len = int((df.end - df.start).max())
    rng = np.random.default_rng(7)
    starts = {c: df.start.values[df.chrom.values == c] for c in ("a", "b", "zz")}  # (ascending inside a contig)
    names, lo, n_chunks = [], [], 0
    while n_chunks < n_chunks_wanted:
        for chrom, centre, jitter in _ROUND:
            c = centre + (int(rng.integers(-jitter, jitter + 1)) if jitter else 0)
            names.append(chrom)
            lo.append(c - 600)
            first, behind = np.searchsorted(starts[chrom], [max(c - 600, 0) - max_len + 1, c + 600])
            n_chunks += -(-int(behind - first) // CHUNK)
    lo = np.asarray(lo, dtype=np.int64)
    return np.asarray(names, dtype=object), lo, lo + 1200


SCAN_WIDTHS = (1, 63, 64, 65, 129, 2001)


def scan_cases(n=5, seed=8):
    """(diff int32 [n, W + 1] with entries in [-50, 50], flank, centre distance) for every width around the 64-column
    step of k_frag_pileup_scan, with an empty flank and the widest one, the whole row as centre and the narrowest"""
    rng = np.random.default_rng(seed)
    for W in SCAN_WIDTHS:
        diff = rng.integers(-50, 51, size=(n, W + 1)).astype(np.int32)
        for flank in sorted({0, W // 2}):
            for centre in sorted({0, W // 2}):
                yield diff, flank, centre


def length_class_columns(n, seed=9, n_barcodes=41, n_obs=23):
    """(start, end, barcode, cell_of, n_obs) as raw int32 columns: lengths around the bounds 147 and 294, barcodes from
    -3 to n_barcodes + 2 (out of range on both sides), a table of cells from -1 to n_obs + 1 (no cell on both sides)"""
    rng = np.random.default_rng(seed)
    start = rng.integers(0, 1 << 30, size=n).astype(np.int32)
    length = rng.choice([0, 1, 100, 145, 146, 147, 148, 200, 292, 293, 294, 295, 500], size=n)
    barcode = rng.integers(-3, n_barcodes + 3, size=n).astype(np.int32)
    cell_of = rng.integers(-1, n_obs + 2, size=n_barcodes).astype(np.int32)
    return start, (start + length).astype(np.int32), barcode, cell_of, n_obs
