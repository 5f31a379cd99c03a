"""TEST INFRASTRUCTURE: the matrix of every test of csrc/rank.hip and muon_amd/_atac/rank.py, the label tables, the
end-to-end cases and the comparison with tests/rank_refs.py.

1100 cells x 96 peaks.  The rows of X^T (entries per peak) sit at the edges of the kernels' walk: the 64-entry chunk
(63, 64, 65, 127, 128, 129), the long-row cap of 256 above which a row is split over four waves (255, 256, 257), pieces
that end inside a chunk (1025, 1100), empty rows first and last.  Integer values 1..5 with about 10 % explicitly stored
zeros: every sum is exact in f64 and every rank a multiple of 0.5."""
import functools

import numpy as np
import pandas as pd
import scipy.sparse as sp

N_CELLS, N_PEAKS = 1100, 96
LENGTHS = [0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1024, 1025, 1100, 2, 0]
ROW_CAP = 256  # mu_rank_row_cap(): 255, 256 and 257 are among LENGTHS
EQUAL_PEAK, RUN_PEAK = 13, 11  # the non-integer variant: a column of equal values; a tie run of 300 non-zero values


@functools.lru_cache(maxsize=None)
def matrices(dtype_name="float32", variant="int"):
    """(X cells x peaks, X^T peaks x cells): canonical CSR matrices with explicitly stored zeros"""
    rng = np.random.default_rng(20261018)
    dtype = np.dtype(dtype_name)
    indptr, cells, data = [0], [], []
    for j in range(N_PEAKS):
        k = LENGTHS[j] if j < len(LENGTHS) else int(rng.integers(3, 401))
        c = np.sort(rng.choice(N_CELLS, k, replace=False))
        v = rng.integers(1, 6, k).astype(np.float64)
        v[rng.random(k) < 0.10] = 0
        if variant == "frac":
            v = v * 0.37
            if j == EQUAL_PEAK:
                v[:] = 3 * 0.37
            if j == RUN_PEAK:
                v[rng.choice(k, 300, replace=False)] = 2 * 0.37
        cells.append(c.astype(np.int32))
        data.append(v.astype(dtype))
        indptr.append(indptr[-1] + k)
    Xt = sp.csr_matrix((np.concatenate(data), np.concatenate(cells), np.asarray(indptr, dtype=np.int64)),
                       shape=(N_PEAKS, N_CELLS))
    Xt.has_sorted_indices = True
    X = Xt.T.tocsr()
    X.sort_indices()
    assert X.nnz == Xt.nnz and (X.data == 0).sum() > 500  # the stored zeros survive
    assert list(np.diff(Xt.indptr)[:len(LENGTHS)]) == LENGTHS
    return X, Xt


@functools.lru_cache(maxsize=None)
def labels(name):
    """int32 label per cell and the number of buckets"""
    rng = np.random.default_rng(7)
    if name == "g5":
        lab = rng.integers(0, 5, N_CELLS)
        lab[0], lab[-1] = 0, 4
        return lab.astype(np.int32), 5
    if name == "g2":
        return rng.integers(0, 2, N_CELLS).astype(np.int32), 2
    if name == "g64":  # bucket 63 holds exactly 2 cells
        lab = rng.integers(0, 63, N_CELLS)
        lab[[17, 1001]] = 63
        return lab.astype(np.int32), 64
    if name == "skip":
        lab = rng.integers(0, 5, N_CELLS)
        lab[rng.random(N_CELLS) < 0.05] = -1
        return lab.astype(np.int32), 5
    if name == "g65":  # more buckets than lanes: the tensor formulation
        lab = rng.integers(0, 65, N_CELLS)
        lab[:65] = np.arange(65)
        return lab.astype(np.int32), 65
    raise KeyError(name)


LABEL_VARIANTS = ["g5", "g2", "g64", "skip"]

# the end-to-end cases: keyword arguments of rank_genes_groups ("base": uns['log1p']['base'])
CASES = {
    "t-test": dict(method="t-test"),
    "default-pts": dict(pts=True),
    "overestim-bonferroni": dict(method="t-test_overestim_var", corr_method="bonferroni", pts=True),
    "wilcoxon": dict(method="wilcoxon"),
    "wilcoxon-tie": dict(method="wilcoxon", tie_correct=True, pts=True),
    "t-test-ref": dict(method="t-test", reference="g1", rankby_abs=True),
    "wilcoxon-ref-tie": dict(method="wilcoxon", reference="g1", tie_correct=True, n_genes=10),
    "wilcoxon-ref-groups": dict(method="wilcoxon", reference="g1", groups=["g0", "g3"], corr_method="bonferroni"),
    "t-test-top10-abs-base2": dict(method="t-test", n_genes=10, rankby_abs=True, base=2),
    "wilcoxon-abs": dict(method="wilcoxon", rankby_abs=True),
}


def group_column(with_missing=False):
    lab, _ = labels("g5")
    col = np.array([f"g{b}" for b in lab], dtype=object)
    if with_missing:
        col[np.random.default_rng(3).random(N_CELLS) < 0.03] = None
    return pd.Categorical(col, categories=[f"g{b}" for b in range(5)])


def var_names():
    return [f"chr1:{1000 * j}-{1000 * j + 500}" for j in range(N_PEAKS)]


def anndata(dtype_name="float32", with_missing=False, base=None):
    from muon_amd import AnnData

    X, _ = matrices(dtype_name)
    ad = AnnData(X.copy(), obs=pd.DataFrame({"leiden": group_column(with_missing)},
                                            index=[f"cell{i}" for i in range(N_CELLS)]),
                 var=pd.DataFrame(index=pd.Index(var_names(), dtype=object)))
    if base is not None:
        ad.uns["log1p"] = {"base": base}
    return ad


@functools.lru_cache(maxsize=None)
def expected(case, with_missing=False):
    """tests/rank_refs.py on the dense matrix (computed once per case)"""
    from tests import rank_refs

    kw = dict(CASES[case])
    base = kw.pop("base", None)
    X, _ = matrices("float64")
    col = group_column(with_missing)
    group_of = [None if pd.isna(v) else v for v in col]
    return rank_refs.rank_genes_groups(X.toarray(), np.asarray(var_names(), dtype=object), group_of, log1p_base=base, **kw)


def distinct_positions(scores):
    """positions whose score differs from both neighbours' by more than 1e-9 relative"""
    s = scores.astype(np.float64)
    gap = np.abs(np.diff(s)) > 1e-9 * np.maximum(np.abs(s[1:]), np.abs(s[:-1]))
    ok = np.ones(s.size, dtype=bool)
    ok[1:] &= gap
    ok[:-1] &= gap
    return ok


def distinct_share(case):
    want = expected(case)
    return float(np.mean([distinct_positions(want["scores"][g]).mean() for g in want["scores"].dtype.names]))


def compare(got, want, rtol=1e-10, min_share=0.9, full=True):
    """The record arrays of ``got`` (the package) against ``want`` (tests/rank_refs.py).  Values to ``rtol`` at every
    position; names at the positions whose score is distinct in ``want``, of which there must be ``min_share`` (only
    asked of a full ranking: the top 10 of a |score| ranking may well be few), and as a multiset elsewhere."""
    fields = want["names"].dtype.names
    assert got["names"].dtype.names == fields
    shares = []
    for g in fields:
        np.testing.assert_allclose(got["scores"][g], want["scores"][g], rtol=rtol, atol=0)
        ok = distinct_positions(want["scores"][g])
        shares.append(ok.mean())
        assert list(got["names"][g][ok]) == list(want["names"][g][ok])
        assert sorted(got["names"][g]) == sorted(want["names"][g])
        for k in ("pvals", "pvals_adj", "logfoldchanges"):
            np.testing.assert_allclose(got[k][g][ok], want[k][g][ok], rtol=rtol, atol=0, err_msg=f"{k} {g}")
            np.testing.assert_allclose(np.sort(got[k][g]), np.sort(want[k][g]), rtol=rtol, atol=0, err_msg=f"{k} {g}")
    if full:
        assert np.mean(shares) >= min_share, shares
    for k in ("pts", "pts_rest"):
        assert (k in got) == (k in want)
        if k in want:
            assert list(got[k].columns) == list(want[k].columns) and list(got[k].index) == list(want[k].index)
            np.testing.assert_allclose(got[k].values, want[k].values, rtol=1e-15, atol=0)
