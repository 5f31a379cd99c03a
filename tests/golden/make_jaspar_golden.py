#!/usr/bin/env python
"""Pack the motif fixtures: 16 JASPAR count matrices of the reference's data directory (muon/_atac/_ref/jaspar), read
where they lie and stored byte for byte, and the 16 rows of its ``motif_to_gene.txt`` that name them.

  6 columns   MA0004.1 MA0006.1          (no attainable threshold at p = 1e-4: 4^-6 > 1e-4)
  8 columns   MA0027.2 MA0031.1 MA0037.3 (with the two above: short enough to enumerate all 4^L words)
  11 columns  MA0002.2 MA0032.2 MA0035.4 MA0036.3 MA0040.1 MA0047.3
  15 - 17     MA0046.2 MA0052.4 MA0009.2 MA0007.3
  24 columns  MA1594.1                   (the longest of the collection)

Data only: every entry of the archive is the content of a file as a uint8 array (``<id>.pfm``, ``motif_to_gene.txt``);
tests/motif_fixture.py writes them back out as files for the parser.

Writes tests/golden/jaspar_golden.npz.  Run (in the build container):  python tests/golden/make_jaspar_golden.py
"""
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/muon/_atac/_ref/jaspar"
IDS = ["MA0004.1", "MA0006.1", "MA0027.2", "MA0031.1", "MA0037.3", "MA0002.2", "MA0032.2", "MA0035.4", "MA0036.3",
       "MA0040.1", "MA0047.3", "MA0046.2", "MA0052.4", "MA0009.2", "MA0007.3", "MA1594.1"]
COLUMNS = [6, 6, 8, 8, 8, 11, 11, 11, 11, 11, 11, 15, 15, 16, 17, 24]


def main():
    out = {}
    for mid, cols in zip(IDS, COLUMNS):
        raw = open(os.path.join(REF, mid + ".pfm"), "rb").read()
        rows = [ln.split() for ln in raw.decode().splitlines() if ln.strip() and not ln.startswith(">")]
        assert len(rows) == 4 and all(len(r) == cols for r in rows), mid
        out[mid + ".pfm"] = np.frombuffer(raw, dtype=np.uint8)
    table = open(os.path.join(REF, "motif_to_gene.txt"), "rb").read().decode().splitlines(keepends=True)
    rows = {ln.split("\t")[0]: ln for ln in table}
    assert all(re.fullmatch(r"[^\t]+\t[^\t]+\n", rows[mid]) for mid in IDS)
    out["motif_to_gene.txt"] = np.frombuffer("".join(rows[mid] for mid in IDS).encode(), dtype=np.uint8)
    np.savez(os.path.join(HERE, "jaspar_golden.npz"), **out)
    print("wrote jaspar_golden.npz:", sum(v.size for v in out.values()), "bytes of fixtures")


if __name__ == "__main__":
    main()
