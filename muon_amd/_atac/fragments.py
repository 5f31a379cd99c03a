"""Fragment tools on the device: ``count_fragments_features``, ``tss_enrichment``, ``nucleosome_signal``.

The reference (/root/reference/muon/_atac/tools.py:746-1201) runs three Python loops over pysam records, one interpreter
iteration per fragment.  Nothing in them depends on another fragment: they are interval overlap, integer counting and a
row scan.  This module takes the ARRAYS a fragments file holds (as ``muon_amd.io`` does for 10x files; opening tabix or
BAM containers is left out), keeps them in device memory as a ``FragmentTable`` and runs the loops there
(csrc/fragments.hip).  What comes out is what the rest of the package consumes: a canonical CSR with its device copy
attached (``tfidf`` starts without an upload) or ``.obs`` columns (``pp.filter_obs`` keys on them).

The table stores barcode CODES, not cell rows: every call maps the table's barcodes to the current rows of ``adata.obs``
on the host and uploads that one small int32 table, so a table outlives ``pp.filter_obs``.

Operator sets without the kernels (the tests' CPU backend) run the tensor forms below, which are also the kernels'
specification.  DESIGN.md 9.6 lists the deviations from the reference.
"""
from __future__ import annotations

import logging
from dataclasses import dataclass
from typing import List, Optional
from warnings import warn

import numpy as np
import pandas as pd
import torch

from .._backend import backend_or_default
from .._containers import AnnData, is_mudata, modality
from .._core.io import device_csr_from_keys
from .._hostmatrix import host_view
from .._operators import has

_NO_FRAGMENTS = "There is no fragments file located yet. Run muon.atac.tl.locate_fragments first."
_I32_MAX = 2 ** 31 - 1


@dataclass
class FragmentTable:
    """A fragments file in device memory: five int32 columns of equal length in file order, grouped by contig and
    non-decreasing in ``start`` inside a contig."""

    chrom: torch.Tensor    # code into ``contigs``
    start: torch.Tensor    # BED, half-open
    end: torch.Tensor
    barcode: torch.Tensor  # code into ``barcodes``
    score: torch.Tensor
    contigs: List[str]     # names in order of first appearance
    barcodes: pd.Index     # the distinct barcodes of the file
    chrom_ptr: np.ndarray  # int64[len(contigs) + 1]: one segment per contig
    max_len: int           # max(end - start)
    max_score: int
    backend: object

    def __len__(self) -> int:
        return int(self.start.numel())

    def __deepcopy__(self, memo):  # (``adata.copy()`` deep-copies .uns: the table is never written to, share it)
        return self

    @property
    def chrom_ptr_device(self) -> torch.Tensor:
        t = self.__dict__.get("_chrom_ptr_d")
        if t is None:
            t = self.__dict__["_chrom_ptr_d"] = self.backend.to_device(self.chrom_ptr, np.int64)
        return t

    def contig_codes(self, names) -> np.ndarray:
        """int32 code of every name, -1 for a contig the table lacks."""
        return pd.Index(self.contigs).get_indexer(pd.Index(names)).astype(np.int32)


# -----------------------------------------------------------------------------------------------------------------
# building the table
# -----------------------------------------------------------------------------------------------------------------
def _int32(a, what):
    a = np.asarray(a)
    if a.size and (a.min() < 0 or a.max() > _I32_MAX):
        raise ValueError(f"fragment {what} must lie in [0, 2^31)")
    return np.ascontiguousarray(a, dtype=np.int32)


def make_table(chrom, start, end, barcode, score=None, *, sort=False, backend=None) -> FragmentTable:
    backend = backend_or_default(backend)
    chrom, barcode = np.asarray(chrom), np.asarray(barcode)
    start, end = _int32(start, "starts"), _int32(end, "ends")
    n = start.shape[0]
    score = np.ones(n, dtype=np.int32) if score is None else _int32(score, "scores")
    if not (chrom.shape == barcode.shape == end.shape == score.shape == (n,)):
        raise ValueError("chrom, start, end, barcode and score must be one-dimensional and of equal length")
    ccode, contigs = pd.factorize(chrom)
    bcode, barcodes = pd.factorize(barcode)
    if (ccode < 0).any() or (bcode < 0).any():
        raise ValueError("fragments with a missing contig or barcode")
    if sort:
        order = np.lexsort((start, ccode))  # stable: ties keep the file's order
        ccode, bcode, start, end, score = ccode[order], bcode[order], start[order], end[order], score[order]
    if n > 1:
        same = ccode[1:] == ccode[:-1]
        if (ccode[1:] < ccode[:-1]).any() or (start[1:][same] < start[:-1][same]).any():
            raise ValueError("fragments must be grouped by contig and sorted by start inside a contig, as in a "
                             "tabix-indexed file (pass sort=True to sort them)")
    chrom_ptr = np.zeros(len(contigs) + 1, dtype=np.int64)
    np.cumsum(np.bincount(ccode, minlength=len(contigs)), out=chrom_ptr[1:])
    length = end.astype(np.int64) - start
    up = backend.to_device
    return FragmentTable(up(ccode, np.int32), up(start, np.int32), up(end, np.int32), up(bcode, np.int32),
                         up(score, np.int32), [str(c) for c in contigs], pd.Index(barcodes), chrom_ptr,
                         int(max(length.max(), 0)) if n else 0, int(score.max()) if n else 0, backend)


def _store(adata, table):
    if "files" not in adata.uns:
        adata.uns["files"] = dict()
    adata.uns["files"]["fragments"] = table


def fragments_from_arrays(data, chrom, start, end, barcode, score=None, *, sort=False, backend=None) -> FragmentTable:
    """Build a ``FragmentTable`` from the five columns of a fragments file and keep it in
    ``.uns["files"]["fragments"]``, where the reference keeps the path (tools.py:679).  ``score=None``: all ones.
    Rows must be grouped by contig and non-decreasing in ``start`` inside a contig, else ``ValueError``;
    ``sort=True`` sorts them stably first."""
    adata = modality(data, "atac")
    table = make_table(chrom, start, end, barcode, score, sort=sort, backend=backend)
    _store(adata, table)
    return table


def read_fragments(path, *, sort=False, backend=None) -> FragmentTable:
    """A plain or gzip fragments TSV (chrom, start, end, barcode[, score]; ``#`` lines skipped), read whole."""
    df = pd.read_csv(path, sep="\t", header=None, comment="#", dtype={0: str, 3: str})
    if df.shape[1] < 4:
        raise ValueError(f"{path}: a fragments file has at least the columns chrom, start, end, barcode")
    score = df[4].values if df.shape[1] > 4 else None
    return make_table(df[0].values, df[1].values, df[2].values, df[3].values, score, sort=sort, backend=backend)


def locate_fragments(data, fragments, return_fragments: bool = False, *, sort=False, backend=None):
    """``muon.atac.tl.locate_fragments`` (tools.py:640): ``fragments`` is a ``FragmentTable`` or the path of a plain or
    gzip fragments TSV of five columns (four: score 1), which is READ here - no tabix index and no pysam are needed.
    The table goes to ``.uns["files"]["fragments"]``."""
    adata = modality(data, "atac")
    table = fragments if isinstance(fragments, FragmentTable) else read_fragments(fragments, sort=sort, backend=backend)
    _store(adata, table)
    if return_fragments:
        return table


def _table_of(adata) -> FragmentTable:
    if "files" not in adata.uns or "fragments" not in adata.uns["files"]:
        raise KeyError(_NO_FRAGMENTS)
    table = adata.uns["files"]["fragments"]
    if not isinstance(table, FragmentTable):
        raise TypeError(".uns['files']['fragments'] holds " + (f"the path {table!r}" if isinstance(table, str) else
                        f"a {type(table).__name__}") + ", not a fragment table: read the file with "
                        "muon_amd.atac.tl.locate_fragments (or fragments_from_arrays) first")
    return table


def cell_table(adata, table: FragmentTable, barcodes: Optional[str] = None) -> np.ndarray:
    """int32[len(table.barcodes)]: barcode code -> current row of ``adata.obs`` (-1: not in this object).  Names come
    from the ``barcodes`` column where it exists (tools.py:1028), else from the index.  Duplicates raise: the reference's
    dict keeps the last one and ``get_loc`` returns a slice."""
    if barcodes and barcodes in adata.obs.columns:
        names, what = pd.Index(adata.obs.loc[:, barcodes].values), f".obs[{barcodes!r}]"
    else:
        names, what = pd.Index(adata.obs.index), ".obs_names"
    if not names.is_unique:
        raise ValueError(f"{what} has duplicate barcodes: fragments cannot be assigned to one cell")
    return names.get_indexer(table.barcodes).astype(np.int32)


# -----------------------------------------------------------------------------------------------------------------
# the device passes: kernels where the operator set has them, tensor forms otherwise
# -----------------------------------------------------------------------------------------------------------------
def ranges_tensor(table: FragmentTable, wchrom, wlo, whi):
    """Window -> candidate range (rng_lo, rng_len int64): start > lo - max_len && start < hi inside the contig."""
    key = (table.chrom.long() << 32) + table.start.long()  # ascending: grouped by code, sorted inside
    c = wchrom.long().clamp(min=0)
    lo = (wlo.long().clamp(min=0) - table.max_len + 1).clamp(min=0)
    hi = whi.long().clamp(min=0)
    a = torch.searchsorted(key, (c << 32) + lo)
    b = torch.maximum(torch.searchsorted(key, (c << 32) + hi), a)
    known = (wchrom >= 0) & (wchrom.long() < len(table.contigs))
    zero = torch.zeros_like(a)
    return torch.where(known, a, zero), torch.where(known, b - a, zero)


def _candidates(table, cell_of, wlo, whi, rng_lo, rng_len):
    """(window, fragment index, cell) of the passing candidates, in window order and file order inside a window."""
    dev = rng_lo.device
    w = torch.repeat_interleave(torch.arange(rng_lo.numel(), device=dev), rng_len)
    first = torch.cumsum(rng_len, 0) - rng_len
    p = rng_lo[w] + (torch.arange(w.numel(), device=dev) - first[w])
    cell = cell_of.long()[table.barcode[p].long()]
    ok = (table.end[p] > wlo[w].clamp(min=0)) & (table.start[p] < whi[w]) & (cell >= 0)
    return w[ok], p[ok], cell[ok]


def overlap_tensor(table, cell_of, wlo, whi, rng_lo, rng_len, n_features, use_score=True):
    w, p, cell = _candidates(table, cell_of, wlo, whi, rng_lo, rng_len)
    vals = table.score[p] if use_score else torch.ones(p.numel(), dtype=torch.int32, device=p.device)
    return cell * int(n_features) + w, vals


def pileup_tensor(table, cell_of, n_obs, wlo, whi, rng_lo, rng_len, width):
    w, p, cell = _candidates(table, cell_of, wlo, whi, rng_lo, rng_len)
    tss = wlo[w].long()
    c0 = (table.start[p].long() - tss).clamp(min=0)
    c1 = (table.end[p].long() - tss).clamp(max=int(width))
    ok = c0 < c1
    s = table.score[p][ok]
    diff = torch.zeros(int(n_obs) * (int(width) + 1), dtype=torch.int32, device=rng_lo.device)
    base = cell[ok] * (int(width) + 1)
    diff.index_add_(0, base + c0[ok], s)
    diff.index_add_(0, base + c1[ok], -s)
    return diff.view(int(n_obs), int(width) + 1)


def scan_tensor(diff, flank_size, center_dist):
    W = diff.shape[1] - 1
    pile = torch.cumsum(diff[:, :W], dim=1)
    diff[:, :W] = pile.to(torch.int32)
    flank = pile[:, :flank_size].sum(dim=1) + pile[:, W - flank_size:].sum(dim=1)
    centre = pile[:, center_dist:W - center_dist].sum(dim=1)
    return torch.stack([flank, centre], dim=1).to(torch.int64)


def length_classes_tensor(table, cell_of, n_obs, n_take, free_bound, mono_bound):
    n_take = max(0, min(int(n_take), len(table)))
    cell = cell_of.long()[table.barcode[:n_take].long()]
    length = table.end[:n_take] - table.start[:n_take]
    cls = torch.where(length < free_bound, 0, torch.where(length < mono_bound, 1, 2))
    ok = (cell >= 0) & (cls < 2)
    cnt = torch.bincount(cell[ok] * 2 + cls[ok], minlength=2 * int(n_obs))
    return cnt.view(int(n_obs), 2).to(torch.int32)


def window_ranges(table, wchrom, wlo, whi):
    be = table.backend
    if has(be, "frag_ranges"):
        return be.frag_ranges(table.start, table.chrom_ptr_device, wchrom, wlo, whi, table.max_len)
    return ranges_tensor(table, wchrom, wlo, whi)


def overlap_triplets(table, cell_of, n_obs, wlo, whi, rng_lo, rng_len, n_features, use_score=True):
    be = table.backend
    if has(be, "frag_overlap"):
        return be.frag_overlap(table.start, table.end, table.barcode, table.score if use_score else None, cell_of,
                               n_obs, wlo, whi, rng_lo, rng_len, n_features)
    return overlap_tensor(table, cell_of, wlo, whi, rng_lo, rng_len, n_features, use_score)


def pileup_diff(table, cell_of, n_obs, wlo, whi, rng_lo, rng_len, width):
    be = table.backend
    if has(be, "frag_pileup"):
        return be.frag_pileup(table.start, table.end, table.barcode, table.score, cell_of, n_obs, wlo, whi, rng_lo,
                              rng_len, width)
    return pileup_tensor(table, cell_of, n_obs, wlo, whi, rng_lo, rng_len, width)


def pileup_scan(table, diff, flank_size, center_dist):
    be = table.backend
    if has(be, "frag_pileup_scan"):
        return be.frag_pileup_scan(diff, flank_size, center_dist)
    return scan_tensor(diff, flank_size, center_dist)


def length_classes(table, cell_of, n_obs, n_take, free_bound, mono_bound):
    be = table.backend
    if has(be, "frag_length_classes"):
        return be.frag_length_classes(table.start, table.end, table.barcode, cell_of, n_obs, n_take, free_bound,
                                      mono_bound)
    return length_classes_tensor(table, cell_of, n_obs, n_take, free_bound, mono_bound)


def _table_backend(table, backend):
    if backend is not None and backend is not table.backend:
        raise ValueError("the fragment table lives on another backend than the one passed")
    return table.backend


def _windows(table, chrom_names, lo, hi):
    """Upload the windows (contig code, lo, hi) as int32; coordinates are clipped to the int32 range (no fragment lies
    outside it)."""
    be = table.backend
    clip = lambda a: np.clip(np.asarray(a, dtype=np.float64), -_I32_MAX, _I32_MAX).astype(np.int32)  # noqa: E731
    return (be.to_device(table.contig_codes(chrom_names), np.int32), be.to_device(clip(lo), np.int32),
            be.to_device(clip(hi), np.int32))


# -----------------------------------------------------------------------------------------------------------------
# public functions
# -----------------------------------------------------------------------------------------------------------------
def get_gene_annotation_from_rna(data) -> pd.DataFrame:
    """/root/reference/muon/_rna/utils.py:7-37: Chromosome / Start / End from the ``interval`` column of the 'rna' .var."""
    adata = modality(data, "rna")
    if "interval" not in adata.var.columns:
        raise ValueError(".var object does not have a column named interval")
    features = pd.DataFrame([s.replace(":", "-", 1).split("-") for s in adata.var.interval])
    features.columns = ["Chromosome", "Start", "End"]
    features["gene_id"] = adata.var.gene_ids.values
    features["gene_name"] = adata.var.index.values
    features.index = adata.var.index
    features = features.loc[~features.Start.isnull()]  # genes without coordinates
    features.Start = features.Start.astype(int)
    features.End = features.End.astype(int)
    return features


def _default_features(data, features):
    if features is not None:
        return features
    if is_mudata(data) and "rna" in data.mod and "interval" in data.mod["rna"].var.columns:
        return get_gene_annotation_from_rna(data)
    raise ValueError(
        "Argument `features` is required. It should be a BED-like DataFrame with gene coordinates and names.")


def count_fragments_features(data, features: Optional[pd.DataFrame] = None, stranded: bool = False,
                             extend_upstream: int = 2e3, extend_downstream: int = 0, count_reads: bool = True, *,
                             values_dtype=np.float32, backend=None):
    """Count fragments overlapping given features (``muon.atac.tl.count_fragments_features``, tools.py:746-891).
    Returns the cells x features AnnData; ``X`` is a canonical CSR of ``values_dtype`` with its device copy attached.

    ``features``: columns (case-insensitive) chr/chrom/chromosome (longer takes precedence), start, end, and strand
    when ``stranded``: a "-" feature is then extended upstream behind its end.  ``count_reads=True`` sums the fragments'
    scores (and warns, like the reference, that the default will change), ``False`` counts fragments.  A feature on a
    contig the table lacks counts nothing."""
    adata = modality(data, "atac")
    features = _default_features(data, features)
    table = _table_of(adata)
    be = _table_backend(table, backend)
    if count_reads:
        warn("From v0.2, by default, unique fragments will be counted instead of reads. See muon#110 for details.",
             FutureWarning, stacklevel=2)
    n, n_features = adata.n_obs, features.shape[0]

    f_cols = np.array([col.lower() for col in features.columns.values])
    for col in ("start", "end"):
        if col not in f_cols:
            raise ValueError(f"No column with feature {col}s could be found")
    chrom_col = next((col for col in ("chromosome", "chrom", "chr") if col in f_cols), None)
    if chrom_col is None:
        raise ValueError("No column with chromosome for features could be found")
    column = lambda name: features[features.columns.values[np.where(f_cols == name)[0][0]]].values  # noqa: E731
    f_start, f_end = column("start").astype(np.float64), column("end").astype(np.float64)
    minus = np.zeros(n_features, dtype=bool)
    if stranded:
        if "strand" not in f_cols:
            raise ValueError("No column with strand for features could be found")
        minus = column("strand") == "-"
    lo = np.where(minus, f_start - extend_downstream, f_start - extend_upstream)
    hi = np.where(minus, f_end + extend_upstream, f_end + extend_downstream)

    logging.info(f"Counting fragments in {n} cells for {n_features} features...")
    wchrom, wlo, whi = _windows(table, column(chrom_col), np.floor(lo), np.ceil(hi))
    cell_of = be.to_device(cell_table(adata, table), np.int32)
    rng_lo, rng_len = window_ranges(table, wchrom, wlo, whi)
    keys, vals = overlap_triplets(table, cell_of, n, wlo, whi, rng_lo, rng_len, n_features, use_score=bool(count_reads))
    X = device_csr_from_keys(keys, vals.long(), (n, n_features))  # (duplicates summed as integers)
    X.values = X.values.to(getattr(torch, np.dtype(values_dtype).name))
    if has(be, "with_slab_ptr"):
        X = be.with_slab_ptr(X)
    return AnnData(host_view(X, be, canonical=True), obs=adata.obs, var=features)


def _check_tss_score(region_size: int, flank_size: int = 100, center_size: int = 1001) -> int:
    """The two errors of ``_calculate_tss_score`` (tools.py:1086-1092); returns ``center_dist``."""
    if center_size > region_size:
        raise ValueError(f"`center_size` ({center_size}) must smaller than the piled up region ({region_size}).")
    if center_size % 2 == 0:
        raise ValueError(f"`center_size` must be an uneven number, but is {center_size}.")
    return (region_size - center_size) // 2  # distance from the edge of data region


def tss_pileup_device(adata, features, extend_upstream=1000, extend_downstream=1000, barcodes=None, backend=None):
    """``_tss_pileup`` (tools.py:987-1068) as a difference array on the device: int32[n_obs, W + 1], W = up + down + 1;
    ``pileup_scan`` turns its first W columns into the pileup."""
    table = _table_of(adata)
    be = _table_backend(table, backend)
    up, down = int(extend_upstream), int(extend_downstream)
    width = up + down + 1
    features = features[features.Chromosome.isin(table.contigs)]  # the chromosomes present in the fragments file
    if features.shape[0] * max(table.max_score, 1) > _I32_MAX:
        raise ValueError(f"{features.shape[0]} regions of scores up to {table.max_score} could overflow the int32 pileup")
    start = features.Start.values.astype(np.int64)
    wchrom, wlo, whi = _windows(table, features.Chromosome.values, start - up, start + down)
    cell_of = be.to_device(cell_table(adata, table, barcodes), np.int32)
    rng_lo, rng_len = window_ranges(table, wchrom, wlo, whi)
    return pileup_diff(table, cell_of, adata.n_obs, wlo, whi, rng_lo, rng_len, width)


def tss_enrichment(data, features: Optional[pd.DataFrame] = None, extend_upstream: int = 1000,
                   extend_downstream: int = 1000, n_tss: int = 2000, return_tss: bool = True, random_state=None,
                   barcodes: Optional[str] = None, *, backend=None):
    """TSS enrichment according to ENCODE guidelines (``muon.atac.tl.tss_enrichment``, tools.py:894-1106): adds
    ``tss_score`` to ``.obs`` and, with ``return_tss``, returns the AnnData of the flank-normalised pileup (cells x
    positions, f64) - without it the pileup never leaves the device.  ``features`` needs Chromosome and Start columns."""
    adata = modality(data, "atac")
    features = _default_features(data, features)
    if features.shape[0] > n_tss:
        # Only use n_tss randomly chosen sites to make function faster
        features = features.sample(n=n_tss, random_state=random_state)
    table = _table_of(adata)
    flank_size, width = 100, int(extend_upstream) + int(extend_downstream) + 1
    center_dist = _check_tss_score(width, flank_size)

    diff = tss_pileup_device(adata, features, extend_upstream, extend_downstream, barcodes, backend)
    be = table.backend
    sums = be.to_host(pileup_scan(table, diff, flank_size, center_dist)).astype(np.int64)
    flank_means = sums[:, 0] / float(2 * flank_size)
    # Replace 0 means with population average (to not have 0 division after)
    flank_means[flank_means == 0] = flank_means.mean()
    if center_dist > 0:
        center_means = sums[:, 1] / float(width - 2 * center_dist)
    else:  # `data.X[:, 0:-0]` is empty in the reference: the mean of nothing
        center_means = np.full(adata.n_obs, np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        tss_scores = center_means / flank_means
    adata.obs["tss_score"] = tss_scores
    logging.info('Added a "tss_score" column to the .obs slot')
    if return_tss:
        anno = pd.DataFrame({"TSS_position": range(-int(extend_upstream), int(extend_downstream) + 1)})
        anno.index = anno.index.astype(str)
        with np.errstate(divide="ignore", invalid="ignore"):
            X = be.to_host(diff[:, :width].contiguous()) / flank_means[:, None]
        tss_pileup = AnnData(X, obs=adata.obs, var=anno)
        tss_pileup.obs["tss_score"] = tss_scores
        return tss_pileup


def nucleosome_signal(data, n=None, nucleosome_free_upper_bound: int = 147, mononuleosomal_upper_bound: int = 294,
                      barcodes: Optional[str] = None, *, backend=None):
    """Ratio of mono-nucleosomal to nucleosome-free fragments per cell (``muon.atac.tl.nucleosome_signal``,
    tools.py:1109-1201) over the first ``n`` fragments of the table (None: 1e4 * number of cells); fragments of unknown
    barcodes use up their turn.  Adds ``nucleosome_signal`` to ``.obs``."""
    adata = modality(data, "atac")
    table = _table_of(adata)
    be = _table_backend(table, backend)
    n = int(adata.n_obs * 1e4) if n is None else int(n)
    cell_of = be.to_device(cell_table(adata, table, barcodes), np.int32)
    bound = lambda b: int(min(max(np.ceil(b), -_I32_MAX), _I32_MAX))  # noqa: E731  (len < b <=> len < ceil(b))
    mat = be.to_host(length_classes(table, cell_of, adata.n_obs, n, bound(nucleosome_free_upper_bound),
                                    bound(mononuleosomal_upper_bound))).astype(np.int64)
    # Prevent division by 0
    mat[mat[:, 0] == 0, :] += 1
    adata.obs["nucleosome_signal"] = mat[:, 1] / mat[:, 0]
    logging.info('Added a "nucleosome_signal" column to the .obs slot')
    return None
