"""``muon.atac.tl.rank_peaks_groups`` (/root/reference/muon/_atac/tools.py:337-373) on the device copy of the matrix.

The reference hands the statistics to ``scanpy.tl.rank_genes_groups`` and then joins the ranked peaks with the peak
annotation (``add_genes_peaks_groups``).  Here the statistics come from two sweeps over X^T as a device CSR
(csrc/rank.hip): per (peak, group) sum, sum of squares and non-zero count for the t-tests, the fold changes and ``pts``;
tie-averaged rank sums per peak for Wilcoxon.  Everything after the two tables - means, variances, scores, p-values,
their adjustment, the ordering - is f64 arithmetic on [n_peaks x n_groups] arrays on the host, stated as scanpy
states it.  The annotation tools are pandas on the host.

Documented differences from the reference / scanpy:
  * ``rank_peaks_groups`` adds the gene columns only when ``uns['atac']['peak_annotation']`` exists; the reference
    raises ``KeyError`` after having ranked.
  * peaks with equal scores are ordered by ascending peak index; scanpy leaves their order to ``argpartition``.
  * ``pts`` counts values that are not zero: an explicitly stored zero is not counted (like ``pp.qc_metrics``).

Out of scope: ``comm`` with more than one rank, ``use_raw=True``, ``method='logreg'``,
``add_peak_annotation_gene_names`` (the motif tools are ``motifs.py``).
"""
from __future__ import annotations

from contextlib import suppress
from typing import Optional

import numpy as np
import torch
from scipy.sparse import issparse

from .._backend import DeviceCSR, backend_or_default
from .._containers import modality
from .._hostmatrix import device_copy
from .._operators import OperatorSet, has, transposed_csr

METHODS = ("t-test", "t-test_overestim_var", "wilcoxon", "logreg")
SORT_BUDGET_BYTES = 1 << 30  # device memory the per-row sort of X^T may hold at a time
_SORT_BYTES_PER_ENTRY = 64   # keys, two permutations and their gathers, 8 B each


# ---------------------------------------------------------------------------------------------------------------------
# the two tables
# ---------------------------------------------------------------------------------------------------------------------
def _row_of(Xt):
    d = Xt.shape[0]
    return torch.repeat_interleave(torch.arange(d, device=Xt.indptr.device), Xt.indptr[1:] - Xt.indptr[:-1])


def _moments_tensor(Xt, labels, n_buckets):
    """``group_moments`` as tensor operations (any number of buckets, operator sets without the kernel)."""
    d, B = Xt.shape[0], int(n_buckets)
    dev = Xt.indptr.device
    lab = labels[Xt.indices.long()].long()
    keep = lab >= 0
    key = (_row_of(Xt) * B + lab)[keep]
    v = Xt.values.to(torch.float64)[keep]
    s = torch.zeros(d * B, dtype=torch.float64, device=dev).index_add_(0, key, v)
    ss = torch.zeros(d * B, dtype=torch.float64, device=dev).index_add_(0, key, v * v)
    cnt = torch.bincount(key[v != 0], minlength=d * B)  # NaN != 0
    return s.view(d, B), ss.view(d, B), cnt.view(d, B)


def _rank_sums_tensor(Xs, labels, n_buckets):
    """``rank_sums`` as tensor operations on the value-sorted X^T."""
    d, B = Xs.shape[0], int(n_buckets)
    dev = Xs.indptr.device
    f = torch.float64
    lab = labels[Xs.indices.long()].long()
    v = Xs.values.to(f)
    keep = (lab >= 0) & (v != 0)
    row, v, lab = _row_of(Xs)[keep], v[keep], lab[keep]
    m = int(row.numel())
    K = torch.bincount(row, minlength=d)
    z = (int((labels >= 0).sum()) - K).to(f)  # the zero block of every row
    neg = torch.zeros(d, dtype=f, device=dev).index_add_(0, row, (v < 0).to(f))
    rs = torch.zeros(d * B, dtype=f, device=dev)
    tie = z ** 3 - z
    if m:
        pos = torch.arange(m, device=dev) - (torch.cumsum(K, 0) - K)[row]
        new = torch.ones(m, dtype=torch.bool, device=dev)
        new[1:] = (row[1:] != row[:-1]) | (v[1:] != v[:-1])
        run = torch.cumsum(new, 0) - 1
        t = torch.bincount(run).to(f)
        rank = (pos[new].to(f) + 0.5 * (t + 1.0))[run] + torch.where(v < 0, torch.zeros_like(v), z[row])
        rs.index_add_(0, row * B + lab, rank)
        tie = tie.index_add(0, row[new], t ** 3 - t)
    return rs.view(d, B), neg + 0.5 * (z + 1.0), tie


def moments_device(backend, Xt, labels, n_buckets):
    if has(backend, "group_moments") and n_buckets <= backend.group_moments_max_groups():
        return backend.group_moments(Xt, labels, n_buckets)
    return _moments_tensor(Xt, labels, n_buckets)


def rank_sums_device(backend, Xs, labels, n_buckets):
    if has(backend, "rank_sums") and n_buckets <= backend.group_moments_max_groups():
        return backend.rank_sums(Xs, labels, n_buckets)
    return _rank_sums_tensor(Xs, labels, n_buckets)


def sort_rows_by_value(Xt, budget_bytes: int = SORT_BUDGET_BYTES):
    """X^T with every row's entries sorted ascending by value (cells permuted alike; equal values keep their order):
    two stable sorts, by value and then by row, over blocks of rows that fit ``budget_bytes`` (the row ids of a block
    are made for that block and count against the budget; nothing of the size of the matrix is held but the result)."""
    d = Xt.shape[0]
    indptr = Xt.indptr.cpu().numpy()
    values, cells = torch.empty_like(Xt.values), torch.empty_like(Xt.indices)
    per_block = max(int(budget_bytes) // _SORT_BYTES_PER_ENTRY, 1)
    lengths = Xt.indptr[1:] - Xt.indptr[:-1]
    j0 = 0
    while j0 < d:
        j1 = int(np.searchsorted(indptr, indptr[j0] + per_block, side="right")) - 1
        j1 = min(max(j1, j0 + 1), d)  # (a row longer than the budget is sorted on its own)
        p0, p1 = int(indptr[j0]), int(indptr[j1])
        if p1 > p0:
            rows = torch.repeat_interleave(torch.arange(j1 - j0, device=lengths.device), lengths[j0:j1])
            o1 = torch.sort(Xt.values[p0:p1], stable=True).indices
            perm = o1[torch.sort(rows[o1], stable=True).indices]
            values[p0:p1] = Xt.values[p0:p1][perm]
            cells[p0:p1] = Xt.indices[p0:p1][perm]
        j0 = j1
    return DeviceCSR(Xt.indptr, cells, values, Xt.shape)


def _dense_transposed(backend, arr):
    """X^T of a dense matrix as a CSR of its non-zero entries (the tensor path's operand)."""
    t = backend.to_device(np.ascontiguousarray(np.asarray(arr).T))
    if t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float64)
    nz = t != 0
    indptr = torch.zeros(t.shape[0] + 1, dtype=torch.int64, device=t.device)
    torch.cumsum(nz.sum(dim=1), 0, out=indptr[1:])
    cells = torch.nonzero(nz)[:, 1].to(torch.int32).contiguous()
    return DeviceCSR(indptr, cells, t[nz].contiguous(), (int(t.shape[0]), int(t.shape[1])))


class _NoKernels(OperatorSet):
    """An operator set seen through its tensor operations alone (a dense matrix takes the tensor path)."""

    def __init__(self, backend):
        self.to_device, self.to_host = backend.to_device, backend.to_host


def _transposed(adata, layer, backend):
    """``(X^T as a device CSR, operator set)``; a sparse matrix leaves its device copy attached."""
    counts = adata.X if layer is None else adata.layers[layer]
    if not issparse(counts):
        backend = backend_or_default(backend)  # raises without a GPU: there is no CPU path in the package
        return _dense_transposed(backend, counts), _NoKernels(backend)
    _host, X, backend = device_copy(counts, backend)
    return transposed_csr(backend, X), backend


# ---------------------------------------------------------------------------------------------------------------------
# host statistics (f64)
# ---------------------------------------------------------------------------------------------------------------------
def _mean_var(s, ss, n):
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = s / n
        var = (ss / n - mean * mean) * (n / (n - 1.0))
    return mean, var


def _adjust(p, corr_method):
    d = p.size
    if corr_method == "bonferroni":
        return np.minimum(p * d, 1.0)
    order = np.argsort(p, kind="stable")
    q = p[order] * d / np.arange(1, d + 1)
    q = np.minimum(np.minimum.accumulate(q[::-1])[::-1], 1.0)
    out = np.empty(d)
    out[order] = q
    return out


def rank_genes_groups(adata, groupby: str, *, groups="all", reference: str = "rest", n_genes: Optional[int] = None,
                      rankby_abs: bool = False, pts: bool = False, key_added: Optional[str] = None,
                      method: Optional[str] = None, corr_method: str = "benjamini-hochberg", tie_correct: bool = False,
                      layer: Optional[str] = None, use_raw: bool = False, comm=None, backend=None) -> None:
    """
    scanpy's ``tl.rank_genes_groups`` for the groups of ``adata.obs[groupby]``, computed on the device copy of the
    matrix; the result goes to ``adata.uns[key_added or 'rank_genes_groups']`` in scanpy's layout (``params`` and the
    record arrays ``names``, ``scores``, ``pvals``, ``pvals_adj``, ``logfoldchanges`` with one field per ranked group;
    with ``pts`` the DataFrames ``pts`` and, against the rest, ``pts_rest``).

    method
            ``'t-test'`` (default), ``'t-test_overestim_var'`` or ``'wilcoxon'``; ``'logreg'`` is not implemented.
    reference
            ``'rest'`` or a category.  Cells with a missing category belong to no group but to the rest.

    A sparse matrix is used where it is resident; otherwise it is uploaded once and the copy stays attached (like
    ``pp.qc_metrics``).  A dense matrix, more than 64 groups and operator sets without the kernels take the tensor
    formulation of the same sums.  See the module docstring for the differences from scanpy and for what is out of
    scope (``use_raw=True``, more than one rank).
    """
    import pandas as pd
    from scipy import stats

    from .._comm import default_comm

    adata = modality(adata, "atac")
    if method is None:
        method = "t-test"
    if method not in METHODS:
        raise ValueError(f"Method must be one of {METHODS}.")
    if method == "logreg":
        raise NotImplementedError("method='logreg' is not implemented")
    if corr_method not in ("benjamini-hochberg", "bonferroni"):
        raise ValueError("Correction method must be one of ('benjamini-hochberg', 'bonferroni').")
    if use_raw:
        raise NotImplementedError("use_raw=True is not implemented: rank a layer or X")
    if getattr(default_comm(comm), "world_size", 1) > 1:
        raise NotImplementedError("rank_genes_groups runs on one rank")

    cat = pd.Categorical(adata.obs[groupby])
    names_all = [str(c) for c in cat.categories]
    codes = np.asarray(cat.codes, dtype=np.int64)
    n_cat = len(names_all)
    missing = bool((codes < 0).any())
    B = n_cat + (1 if missing else 0)
    labels = np.where(codes < 0, n_cat, codes).astype(np.int32)
    counts = np.bincount(labels, minlength=B).astype(np.float64)

    if reference != "rest" and str(reference) not in names_all:
        raise ValueError(f"reference = {reference} needs to be one of groupby = {names_all}.")
    if isinstance(groups, str) and groups == "all":
        selected = list(range(n_cat))
    else:
        if isinstance(groups, (str, int)):
            raise ValueError("Specify a sequence of groups")
        wanted = [str(g) for g in groups]
        unknown = [g for g in wanted if g not in names_all]
        if unknown:
            raise ValueError(f"groups {unknown} are not categories of obs[{groupby!r}]: {names_all}")
        if reference != "rest" and str(reference) not in wanted:
            wanted.append(str(reference))
        selected = [i for i, c in enumerate(names_all) if c in wanted]  # (in category order, like scanpy)
    ref_idx = None if reference == "rest" else names_all.index(str(reference))
    small = [names_all[i] for i in selected if counts[i] < 2]
    if small:
        raise ValueError(f"Could not calculate statistics for groups {', '.join(small)} since they only contain one sample.")
    ranked = [i for i in selected if i != ref_idx]

    Xt, be = _transposed(adata, layer, backend)
    d = Xt.shape[0]
    lab_dev = be.to_device(labels, np.int32)
    s, ss, nz = (be.to_host(t) for t in moments_device(be, Xt, lab_dev, B))
    nz = nz.astype(np.float64)
    n_all = float(labels.size)

    def side(idx):
        """(sum, sumsq, nnz, n) of group ``idx``; None: everything"""
        if idx is None:
            return s.sum(axis=1), ss.sum(axis=1), nz.sum(axis=1), n_all
        return s[:, idx], ss[:, idx], nz[:, idx], counts[idx]

    tot = side(None)
    stats_of = {}
    for g in ranked:
        sg = side(g)
        sr = tuple(a - b for a, b in zip(tot, sg)) if ref_idx is None else side(ref_idx)
        stats_of[g] = (sg, sr)

    scores, pvals = {}, {}
    if method in ("t-test", "t-test_overestim_var"):
        for g in ranked:
            (s_g, ss_g, _, n_g), (s_r, ss_r, _, n_r) = stats_of[g]
            mean_g, var_g = _mean_var(s_g, ss_g, n_g)
            mean_r, var_r = _mean_var(s_r, ss_r, n_r)
            nobs_r = n_g if method == "t-test_overestim_var" else n_r
            with np.errstate(divide="ignore", invalid="ignore"):
                sc, pv = stats.ttest_ind_from_stats(mean1=mean_g, std1=np.sqrt(var_g), nobs1=n_g, mean2=mean_r,
                                                    std2=np.sqrt(var_r), nobs2=nobs_r, equal_var=False)
            scores[g] = np.where(np.isnan(sc), 0.0, sc)
            pvals[g] = np.where(np.isnan(pv), 1.0, pv)
    else:  # wilcoxon
        Xs = sort_rows_by_value(Xt)

        def wilcoxon(g, rs, zr, tie, n_g, n_r, nz_g):
            N = n_g + n_r
            ranksum = rs + (n_g - nz_g) * zr
            T = 1.0 - tie / (N ** 3 - N) if tie_correct else 1.0
            with np.errstate(divide="ignore", invalid="ignore"):
                zs = (ranksum - n_g * (N + 1.0) / 2.0) / np.sqrt(T * n_g * n_r * (N + 1.0) / 12.0)
            zs = np.where(np.isnan(zs), 0.0, zs)
            scores[g], pvals[g] = zs, 2.0 * stats.norm.sf(np.abs(zs))

        if ref_idx is None:  # one launch, every cell labelled
            rs, zr, tie = (be.to_host(t) for t in rank_sums_device(be, Xs, lab_dev, B))
            for g in ranked:
                wilcoxon(g, rs[:, g], zr, tie, counts[g], n_all - counts[g], nz[:, g])
        else:  # one launch per group: group 0, reference 1, every other cell left out
            for g in ranked:
                two = np.full(labels.size, -1, dtype=np.int32)
                two[labels == g] = 0
                two[labels == ref_idx] = 1
                rs, zr, tie = (be.to_host(t) for t in rank_sums_device(be, Xs, be.to_device(two, np.int32), 2))
                wilcoxon(g, rs[:, 0], zr, tie, counts[g], counts[ref_idx], nz[:, g])
        del Xs
    del Xt

    base = None
    with suppress(Exception):
        base = adata.uns["log1p"]["base"]

    def expm1(x):
        return np.expm1(x) if base is None else np.expm1(x * np.log(base))

    var_names = np.asarray(adata.var_names, dtype=object)
    n_top = d if n_genes is None else min(int(n_genes), d)
    cols = {k: [] for k in ("names", "scores", "pvals", "pvals_adj", "logfoldchanges")}
    for g in ranked:
        (s_g, _, _, n_g), (s_r, _, _, n_r) = stats_of[g]
        with np.errstate(divide="ignore", invalid="ignore"):
            lfc = np.log2((expm1(s_g / n_g) + 1e-9) / (expm1(s_r / n_r) + 1e-9))
        key = np.abs(scores[g]) if rankby_abs else scores[g]
        order = np.argsort(-key, kind="stable")[:n_top]  # (equal scores: ascending peak index)
        adj = _adjust(pvals[g], corr_method)
        cols["names"].append(var_names[order])
        cols["scores"].append(scores[g][order].astype(np.float32))
        cols["pvals"].append(pvals[g][order])
        cols["pvals_adj"].append(adj[order])
        cols["logfoldchanges"].append(lfc[order].astype(np.float32))

    fields = [names_all[g] for g in ranked]
    dtypes = {"names": "O", "scores": "float32", "pvals": "float64", "pvals_adj": "float64", "logfoldchanges": "float32"}
    key_out = key_added or "rank_genes_groups"
    out = {"params": dict(groupby=groupby, reference=reference, method=method, use_raw=False, layer=layer,
                          corr_method=corr_method)}
    if pts:
        out["pts"] = pd.DataFrame({names_all[g]: nz[:, g] / counts[g] for g in selected}, index=adata.var_names)
        if ref_idx is None:
            nz_tot = nz.sum(axis=1)
            out["pts_rest"] = pd.DataFrame({names_all[g]: (nz_tot - nz[:, g]) / (n_all - counts[g]) for g in selected},
                                           index=adata.var_names)
    for k, arrs in cols.items():
        out[k] = np.rec.fromarrays(arrs, dtype=[(f, dtypes[k]) for f in fields])
    adata.uns[key_out] = out


# ---------------------------------------------------------------------------------------------------------------------
# peak annotation (pandas; reference _atac/tools.py:83-165, 251-334)
# ---------------------------------------------------------------------------------------------------------------------
def add_peak_annotation(data, annotation, sep: str = "\t", return_annotation: bool = False):
    """
    Parse a peak annotation table into ``.uns['atac']['peak_annotation']``: one row per (peak, gene) pair, indexed by
    gene, with the columns ``peak``, ``distance`` and ``peak_type``.

    annotation
            A DataFrame or the path of a delimited file with the columns ``peak`` (or ``chrom``, ``start``, ``end``),
            ``gene``, ``distance`` and ``peak_type``.  ``;``-separated genes, distances and peak types of one peak
            become one row each; ``chrX_N_N`` peak names become ``chrX:N-N``.
    """
    import pandas as pd

    adata = modality(data, "atac")
    table = annotation if isinstance(annotation, pd.DataFrame) else pd.read_csv(annotation, sep=sep)
    table = table.convert_dtypes()
    if "peak" in table.columns:
        table["peak"] = table["peak"].str.replace("_", ":", n=1).str.replace("_", "-", n=1)
    elif {"chrom", "start", "end"} <= set(table.columns):
        table["peak"] = table["chrom"].astype(str) + ":" + table["start"].astype(str) + "-" + table["end"].astype(str)
    else:
        raise AttributeError("Peak annotation contains neither a peak column nor chrom, start and end columns.")

    if pd.api.types.is_string_dtype(table["distance"]):  # several genes per peak
        by_peak = table.set_index("peak")
        long = [by_peak[c].str.split(";").explode() for c in ("gene", "distance", "peak_type")]
        long[1] = long[1].astype(int)
        table = pd.concat(long, axis=1).reset_index()
    else:
        table = table[["peak", "gene", "distance", "peak_type"]]
    with suppress(ValueError):  # missing values stay as they are
        table["distance"] = table["distance"].astype(int)
    for c in ("peak", "gene", "peak_type"):
        table[c] = table[c].fillna("").astype(object)
    table = table.set_index("gene")

    adata.uns.setdefault("atac", dict())
    adata.uns["atac"]["peak_annotation"] = table
    if return_annotation:
        return table


def add_genes_peaks_groups(data, add_peak_type: bool = False, add_distance: bool = False, *,
                           key: str = "rank_genes_groups") -> None:
    """
    Add the genes of the ranked peaks of every group to ``.uns[key]['genes']`` (a record array like ``names``), and
    with ``add_peak_type`` / ``add_distance`` the dicts ``peak_type`` / ``distance`` of per-group arrays.  Ranked peaks
    without an annotation row are dropped (an inner join); several rows of one peak are joined with ``", "``.
    """
    import pandas as pd

    adata = modality(data, "atac")
    if key not in adata.uns:
        raise KeyError(f"There is no .uns['{key}'] yet. Run rank_genes_groups first.")
    if "atac" not in adata.uns or "peak_annotation" not in adata.uns["atac"]:
        raise KeyError("There is no peak annotation yet. Run muon_amd.atac.tl.add_peak_annotation first.")
    annotation = adata.uns["atac"]["peak_annotation"]
    if "peak" not in annotation.columns:
        raise KeyError("Peak annotation has to contain 'peak' column.")
    res = adata.uns[key]
    gene_col = annotation.index.name
    wanted = [gene_col]
    for flag, col in ((add_peak_type, "peak_type"), (add_distance, "distance")):
        if flag:
            if col not in annotation.columns:
                raise KeyError(f"Peak annotation has to contain '{col}' column.")
            wanted.append(col)
            res[col] = {}
    if add_distance:
        annotation["distance"] = annotation["distance"].astype(str)  # (joined as strings, in the stored table too)
    by_peak = annotation.reset_index(drop=False)[["peak", *wanted]]

    genes = {}
    for group in res["names"].dtype.names:
        ranked = pd.DataFrame({"peak": np.asarray(res["names"][group], dtype=object)})
        joined = ranked.merge(by_peak, on="peak", how="inner", sort=False)
        joined = joined.groupby("peak", sort=False).agg(", ".join)
        genes[group] = joined[gene_col].values
        if add_peak_type:
            res["peak_type"][group] = joined["peak_type"].values
        if add_distance:
            res["distance"][group] = joined["distance"].values
    res["genes"] = pd.DataFrame(genes).to_records(index=False)


def rank_peaks_groups(data, groupby: str, add_peak_type: bool = False, add_distance: bool = False, *, backend=None,
                      **kwargs) -> None:
    """
    Rank peaks in the groups of ``obs[groupby]``: ``rank_genes_groups`` (scanpy's keyword arguments: ``groups``,
    ``reference``, ``n_genes``, ``rankby_abs``, ``pts``, ``key_added``, ``method``, ``corr_method``, ``tie_correct``,
    ``layer``) on the device copy of the peak matrix, followed by ``add_genes_peaks_groups`` when
    ``uns['atac']['peak_annotation']`` exists.  Without an annotation the reference raises ``KeyError`` after the
    ranking; here the ranking alone is the result.
    """
    adata = modality(data, "atac")
    rank_genes_groups(adata, groupby, backend=backend, **kwargs)
    if "peak_annotation" in adata.uns.get("atac", {}):
        add_genes_peaks_groups(adata, add_peak_type=add_peak_type, add_distance=add_distance,
                               key=kwargs.get("key_added") or "rank_genes_groups")
