#!/usr/bin/env python
"""Generate the peak-annotation fixture by EXECUTING the reference's own code.

Loads muon/_atac/tools.py where it lies (the package stubs of make_golden.py, ``muon_amd._containers`` for AnnData /
MuData) and runs ``add_peak_annotation`` (tools.py:83-165), ``rank_peaks_groups`` (:337-373) and with it
``add_genes_peaks_groups`` (:251-334) on the matrix of tests/rank_fixture.py.  scanpy is not installed: the stub's
``tl.rank_genes_groups`` is the dense restatement tests/rank_refs.py.

The annotation table has one row per peak of the fixture, every peak annotated, about 20 % of them with two
``;``-separated genes, distances and peak types, and one peak named in the ``chrX_N_N`` style.

Records the table, the parsed annotation frame (before and after ``add_distance`` turned its distances into strings)
and, for ``add_peak_type = add_distance = False`` ("plain") and ``True`` ("full"), the ranked names and the ``genes`` /
``peak_type`` / ``distance`` arrays of every group.  Data only.

Writes tests/golden/rank_golden.npz.  Run (in the build container):  python tests/golden/make_rank_golden.py
"""
import os
import sys
import types

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True  # (tests/golden holds fixtures and generators only)

from tests import rank_fixture as F  # noqa: E402
from tests import rank_refs  # noqa: E402
from tests.golden import make_golden  # noqa: E402

RANK_KW = dict(method="wilcoxon", n_genes=25)  # what tests/test_rank_host.py passes


def load_reference():
    make_golden._install_stubs()
    tl = types.ModuleType("scanpy.tl")
    tl.rank_genes_groups = rank_refs.scanpy_like
    sys.modules["scanpy"].tl = tl
    sys.modules["scanpy.tl"] = tl
    for name in ("pysam", "tqdm"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["tqdm"].tqdm = lambda it, **kw: it
    make_golden._load("muon._atac.utils", "muon/_atac/utils.py")
    return make_golden._load("muon._atac.tools", "muon/_atac/tools.py")


def annotation_table():
    rng = np.random.default_rng(11)
    kinds = np.array(["promoter", "distal", "intergenic"])
    rows = []
    for j, peak in enumerate(F.var_names()):
        k = 2 if rng.random() < 0.2 else 1
        genes = [f"GENE{int(g):03d}" for g in rng.integers(0, 60, k)]
        rows.append(dict(peak=peak, gene=";".join(genes), distance=";".join(str(int(v)) for v in rng.integers(-5000, 5000, k)),
                         peak_type=";".join(rng.choice(kinds, k))))
    rows[7]["peak"] = rows[7]["peak"].replace(":", "_").replace("-", "_")  # chr1_7000_7500
    table = pd.DataFrame(rows)
    assert (table.gene.str.contains(";")).sum() >= 10
    return table


def frame_parts(frame, prefix):
    out = {f"{prefix}_index_name": np.asarray(frame.index.name), f"{prefix}_index": np.asarray(frame.index, dtype=object),
           f"{prefix}_columns": np.asarray(frame.columns, dtype=object)}
    for c in frame.columns:
        out[f"{prefix}_col_{c}"] = np.asarray(frame[c].tolist(), dtype=object)
    return out


def main():
    tools = load_reference()
    table = annotation_table()
    out = {f"table_{c}": np.asarray(table[c], dtype=object) for c in table.columns}
    for tag, flag in (("plain", False), ("full", True)):
        ad = F.anndata("float64")
        ann = tools.add_peak_annotation(ad, table.copy(), return_annotation=True)
        if not flag:
            out.update(frame_parts(ann, "ann"))
        tools.rank_peaks_groups(ad, "leiden", add_peak_type=flag, add_distance=flag, **RANK_KW)
        res = ad.uns["rank_genes_groups"]
        out[f"{tag}_groups"] = np.asarray(res["genes"].dtype.names, dtype=object)
        for g in res["genes"].dtype.names:
            out[f"{tag}_names_{g}"] = np.asarray(res["names"][g], dtype=object)
            out[f"{tag}_genes_{g}"] = np.asarray(res["genes"][g], dtype=object)
            if flag:
                out[f"{tag}_peak_type_{g}"] = np.asarray(res["peak_type"][g], dtype=object)
                out[f"{tag}_distance_{g}"] = np.asarray(res["distance"][g], dtype=object)
        if flag:
            out.update(frame_parts(ad.uns["atac"]["peak_annotation"], "ann_after"))
    path = os.path.join(HERE, "rank_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
