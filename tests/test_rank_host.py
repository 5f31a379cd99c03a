"""muon_amd.atac.tl.rank_peaks_groups without a GPU: the tensor formulation of the two tables through
tests/cpu_backend.CpuTestBackend against the dense restatement tests/rank_refs.py, the restatement against scipy's own
tests, the result layout, the error cases and the annotation tools against tests/golden/rank_golden.npz."""
import os

import numpy as np
import pandas as pd
import pytest
import torch
from scipy import stats

from muon_amd import atac as ac
from muon_amd._atac import rank as R
from muon_amd._hostmatrix import resident
from muon_amd._backend import DeviceCSR
from tests import rank_fixture as F
from tests import rank_refs
from tests.cpu_backend import CpuTestBackend

BE = CpuTestBackend()


# ---- the restatement against scipy --------------------------------------------------------------------------------
def _dense_and_groups():
    X = F.matrices("float64")[0].toarray()
    return X, np.asarray(F.group_column())


def test_restatement_welch_scores_are_scipys():
    """the f64 scores and p-values that the restatement orders and stores (``scores_and_pvalues``), and the stored
    record arrays themselves, against ``scipy.stats.ttest_ind`` on the dense columns"""
    X, col = _dense_and_groups()
    with np.errstate(all="ignore"):
        res = stats.ttest_ind(X[col == "g2"], X[col != "g2"], equal_var=False)
    has_test = ~np.isnan(res.statistic)  # (an empty column has no test: score 0, p-value 1 in the restatement)
    assert has_test.sum() >= F.N_PEAKS - 2
    sc, pv = rank_refs.scores_and_pvalues(X[col == "g2"], X[col != "g2"], "t-test")
    np.testing.assert_allclose(sc[has_test], res.statistic[has_test], rtol=1e-12, atol=0)
    np.testing.assert_allclose(pv[has_test], res.pvalue[has_test], rtol=1e-12, atol=0)
    assert np.all(sc[~has_test] == 0) and np.all(pv[~has_test] == 1)
    want = F.expected("t-test")  # what the package is compared with: the same numbers, ordered
    order = [F.var_names().index(v) for v in want["names"]["g2"]]
    assert np.array_equal(want["scores"]["g2"], sc[order].astype(np.float32))
    assert np.array_equal(want["pvals"]["g2"], pv[order])


def test_restatement_tie_corrected_pvalues_are_mann_whitneys():
    X, col = _dense_and_groups()
    want = F.expected("wilcoxon-tie")
    order = [F.var_names().index(v) for v in want["names"]["g2"]]
    A, Bm = X[col == "g2"], X[col != "g2"]
    keep = np.array([np.unique(X[:, j]).size > 1 for j in order])  # (a constant column has no test)
    p = stats.mannwhitneyu(A[:, order][:, keep], Bm[:, order][:, keep], use_continuity=False, method="asymptotic").pvalue
    np.testing.assert_allclose(want["pvals"]["g2"][keep], p, rtol=1e-12, atol=0)


def test_restatement_benjamini_hochberg_is_scipys():
    p = F.expected("wilcoxon")["pvals"]["g0"]
    np.testing.assert_allclose(rank_refs.benjamini_hochberg(p), stats.false_discovery_control(p), rtol=1e-12, atol=0)


def test_the_fixture_has_the_row_lengths_and_distinct_scores():
    _, Xt = F.matrices("float32")
    lens = set(np.diff(Xt.indptr).tolist())
    assert {0, 1, 63, 64, 65, 127, 128, 129, F.ROW_CAP - 1, F.ROW_CAP, F.ROW_CAP + 1, 1024, 1025, 1100} <= lens
    for case in ("t-test", "wilcoxon", "wilcoxon-tie"):
        assert F.distinct_share(case) >= 0.9, case
    lab, _ = F.labels("g5")
    assert lab[0] != lab[-1]
    assert (F.labels("g64")[0] == 63).sum() == 2
    _, Xf = F.matrices("float64", "frac")
    row = Xf.data[Xf.indptr[F.EQUAL_PEAK]:Xf.indptr[F.EQUAL_PEAK + 1]]
    assert np.unique(row).size == 1
    run = Xf.data[Xf.indptr[F.RUN_PEAK]:Xf.indptr[F.RUN_PEAK + 1]]
    assert np.unique(run[run != 0], return_counts=True)[1].max() >= 200


# ---- the two tables as tensor operations ---------------------------------------------------------------------------
def _device_t(dtype, variant="int"):
    _, Xt = F.matrices(dtype, variant)
    return DeviceCSR(torch.from_numpy(Xt.indptr.astype(np.int64)), torch.from_numpy(Xt.indices.astype(np.int32)),
                     torch.from_numpy(Xt.data.copy()), Xt.shape)


@pytest.mark.parametrize("name", F.LABEL_VARIANTS + ["g65"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_tensor_tables_are_the_dense_ones(dtype, name):
    lab, B = F.labels(name)
    Xt = _device_t(dtype)
    dense = F.matrices(dtype)[0].toarray()
    s, ss, nz = R.moments_device(BE, Xt, torch.from_numpy(lab), B)
    ws, wss, wnz = rank_refs.group_moments(dense, lab, B)
    assert np.array_equal(s.numpy(), ws) and np.array_equal(ss.numpy(), wss) and np.array_equal(nz.numpy(), wnz)
    rs, zr, tie = R.rank_sums_device(BE, R.sort_rows_by_value(Xt, budget_bytes=1 << 16), torch.from_numpy(lab), B)
    wrs, wtie = rank_refs.rank_sums(dense, lab, B)
    n_b = np.bincount(lab[lab >= 0], minlength=B)
    assert np.array_equal(rs.numpy() + (n_b[None, :] - wnz) * zr.numpy()[:, None], wrs)
    assert np.array_equal(tie.numpy(), wtie)


def test_sorted_rows_keep_their_cells():
    Xt = _device_t("float64", "frac")
    Xs = R.sort_rows_by_value(Xt, budget_bytes=1 << 14)
    ip = Xt.indptr.numpy()
    for j in (0, 1, 9, F.RUN_PEAK, 40, F.N_PEAKS - 1):
        v, c = Xt.values.numpy()[ip[j]:ip[j + 1]], Xt.indices.numpy()[ip[j]:ip[j + 1]]
        o = np.argsort(v, kind="stable")
        assert np.array_equal(Xs.values.numpy()[ip[j]:ip[j + 1]], v[o])
        assert np.array_equal(Xs.indices.numpy()[ip[j]:ip[j + 1]], c[o])


# ---- end to end ------------------------------------------------------------------------------------------------------
def _run(case, dtype="float32", with_missing=False, backend=BE, dense=False):
    kw = dict(F.CASES[case])
    ad = F.anndata(dtype, with_missing, kw.pop("base", None))
    if dense:
        ad.X = ad.X.toarray()
    ac.tl.rank_genes_groups(ad, "leiden", backend=backend, **kw)
    return ad


@pytest.mark.parametrize("case", list(F.CASES))
def test_end_to_end_is_the_restatement(case):
    ad = _run(case, "float32" if len(case) % 2 else "float64")
    F.compare(ad.uns["rank_genes_groups"], F.expected(case), full="n_genes" not in F.CASES[case])


@pytest.mark.parametrize("case", ["t-test", "wilcoxon-tie", "wilcoxon-ref-tie"])
def test_missing_categories_belong_to_the_rest_and_a_dense_matrix_ranks_alike(case):
    want = F.expected(case, True)
    F.compare(_run(case, with_missing=True).uns["rank_genes_groups"], want, full=False)
    F.compare(_run(case, with_missing=True, dense=True).uns["rank_genes_groups"], want, full=False)


def test_more_groups_than_lanes_take_the_tensor_formulation():
    class WithKernels(CpuTestBackend):  # an operator set whose kernels must NOT be asked for 65 buckets
        def group_moments_max_groups(self):
            return 64

        def group_moments(self, *a):
            raise AssertionError("65 buckets went to the kernel")

        rank_sums = group_moments

    lab, B = F.labels("g65")
    ad = F.anndata("float32")
    ad.obs["many"] = pd.Categorical([f"c{b:02d}" for b in lab])
    ac.tl.rank_genes_groups(ad, "many", method="wilcoxon", backend=WithKernels())
    res = ad.uns["rank_genes_groups"]
    assert len(res["names"].dtype.names) == 65
    group_of = [f"c{b:02d}" for b in lab]
    want = rank_refs.rank_genes_groups(F.matrices("float64")[0].toarray(), np.asarray(F.var_names(), dtype=object),
                                       group_of, method="wilcoxon")
    for g in ("c00", "c33", "c64"):
        np.testing.assert_allclose(res["scores"][g], want["scores"][g], rtol=1e-10)


def test_the_device_copy_stays_attached_and_is_used_again():
    from tests.test_host_logic import _CountingBackend

    be = _CountingBackend()
    ad = _run("t-test", backend=be)
    assert be.uploads == 1
    assert resident(ad.X, be) is not None
    ac.tl.rank_genes_groups(ad, "leiden", method="wilcoxon", backend=be)
    assert be.uploads == 1


def test_result_layout():
    ad = _run("wilcoxon-tie")
    res = ad.uns["rank_genes_groups"]
    assert res["params"] == dict(groupby="leiden", reference="rest", method="wilcoxon", use_raw=False, layer=None,
                                 corr_method="benjamini-hochberg")
    kinds = dict(names="O", scores="float32", pvals="float64", pvals_adj="float64", logfoldchanges="float32")
    for k, kind in kinds.items():
        assert res[k].dtype.names == ("g0", "g1", "g2", "g3", "g4")
        assert all(res[k].dtype[f] == np.dtype(kind) for f in res[k].dtype.names)
        assert res[k].shape == (F.N_PEAKS,)
    assert isinstance(res["pts"], pd.DataFrame) and isinstance(res["pts_rest"], pd.DataFrame)
    ad = _run("wilcoxon-ref-tie")
    res = ad.uns["rank_genes_groups"]
    assert res["names"].dtype.names == ("g0", "g2", "g3", "g4") and res["names"].shape == (10,)  # the reference is no field
    assert res["params"]["reference"] == "g1" and "pts" not in res
    ad = F.anndata()
    ac.tl.rank_genes_groups(ad, "leiden", key_added="mine", layer=None, backend=BE)
    assert "mine" in ad.uns and "rank_genes_groups" not in ad.uns


def test_errors():
    ad = F.anndata()
    col = np.asarray(F.group_column()).copy()
    col[col == "g4"] = "g0"
    col[5] = "g4"
    ad.obs["lonely"] = pd.Categorical(col)
    with pytest.raises(ValueError, match="only contain one sample"):
        ac.tl.rank_genes_groups(ad, "lonely", backend=BE)
    with pytest.raises(ValueError, match="needs to be one of groupby"):
        ac.tl.rank_genes_groups(ad, "leiden", reference="g9", backend=BE)
    with pytest.raises(NotImplementedError):
        ac.tl.rank_genes_groups(ad, "leiden", method="logreg", backend=BE)
    with pytest.raises(ValueError):
        ac.tl.rank_genes_groups(ad, "leiden", method="median", backend=BE)
    with pytest.raises(NotImplementedError):
        ac.tl.rank_genes_groups(ad, "leiden", use_raw=True, backend=BE)

    class TwoRanks:
        world_size, rank = 2, 0

    with pytest.raises(NotImplementedError, match="one rank"):
        ac.tl.rank_genes_groups(ad, "leiden", comm=TwoRanks(), backend=BE)
    with pytest.raises(TypeError):
        ac.tl.rank_peaks_groups(object(), "leiden")


# ---- the annotation tools against the reference's own output -----------------------------------------------------
@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "rank_golden.npz"), allow_pickle=True)


def _annotation_table(golden):
    return pd.DataFrame({c: golden[f"table_{c}"] for c in ("peak", "gene", "distance", "peak_type")})


def _same_frame(frame, golden, prefix):
    assert frame.index.name == str(golden[f"{prefix}_index_name"])
    assert list(frame.index) == list(golden[f"{prefix}_index"])
    assert list(frame.columns) == list(golden[f"{prefix}_columns"])
    for c in frame.columns:
        assert list(frame[c]) == list(golden[f"{prefix}_col_{c}"]), c


def test_add_peak_annotation_is_the_references(golden):
    ad = F.anndata()
    got = ac.tl.add_peak_annotation(ad, _annotation_table(golden), return_annotation=True)
    assert got is ad.uns["atac"]["peak_annotation"]
    _same_frame(got, golden, "ann")
    assert got["distance"].dtype.kind == "i" and got["peak"].dtype == object


def test_add_peak_annotation_reads_a_file_and_builds_peak_names(golden, tmp_path):
    table = _annotation_table(golden)
    path = tmp_path / "peak_annotation.tsv"
    table.to_csv(path, sep="\t", index=False)
    ad = F.anndata()
    ac.tl.add_peak_annotation(ad, str(path))
    _same_frame(ad.uns["atac"]["peak_annotation"], golden, "ann")
    parts = table["peak"].str.replace("_", ":", n=1).str.replace("_", "-", n=1).str.extract(r"(.+):(\d+)-(\d+)")
    split = table.drop(columns="peak").assign(chrom=parts[0], start=parts[1].astype(int), end=parts[2].astype(int))
    ac.tl.add_peak_annotation(ad, split)
    _same_frame(ad.uns["atac"]["peak_annotation"], golden, "ann")
    with pytest.raises(AttributeError):
        ac.tl.add_peak_annotation(ad, table.drop(columns="peak"))


@pytest.mark.parametrize("flags", [(False, False), (True, True)])
def test_rank_peaks_groups_writes_the_references_gene_columns(golden, flags):
    ad = F.anndata()
    ac.tl.add_peak_annotation(ad, _annotation_table(golden))
    ac.tl.rank_peaks_groups(ad, "leiden", add_peak_type=flags[0], add_distance=flags[1], backend=BE, method="wilcoxon",
                            n_genes=25)
    res = ad.uns["rank_genes_groups"]
    tag = "full" if flags[0] else "plain"
    assert res["genes"].dtype.names == tuple(golden[f"{tag}_groups"])
    for g in res["genes"].dtype.names:
        assert list(res["names"][g]) == list(golden[f"{tag}_names_{g}"])
        assert list(res["genes"][g]) == list(golden[f"{tag}_genes_{g}"])
        if flags[0]:
            assert list(res["peak_type"][g]) == list(golden[f"{tag}_peak_type_{g}"])
            assert list(res["distance"][g]) == list(golden[f"{tag}_distance_{g}"])
    assert ("peak_type" in res) == flags[0] and ("distance" in res) == flags[1]
    if flags[1]:  # (the stored table's distances are strings afterwards, as in the reference)
        _same_frame(ad.uns["atac"]["peak_annotation"], golden, "ann_after")


def test_rank_peaks_groups_without_an_annotation_ranks_alone():
    ad = F.anndata()
    ac.tl.rank_peaks_groups(ad, "leiden", backend=BE)
    assert "genes" not in ad.uns["rank_genes_groups"]
    with pytest.raises(KeyError, match="peak annotation"):
        ac.tl.add_genes_peaks_groups(ad)
    with pytest.raises(KeyError):
        ac.tl.add_genes_peaks_groups(F.anndata())


def test_unannotated_peaks_are_dropped_from_the_gene_columns(golden):
    ad = F.anndata()
    table = _annotation_table(golden)
    ac.tl.add_peak_annotation(ad, table.iloc[::2])
    ac.tl.rank_peaks_groups(ad, "leiden", backend=BE)
    res = ad.uns["rank_genes_groups"]
    assert res["names"].shape == (F.N_PEAKS,) and res["genes"].shape == (F.N_PEAKS // 2,)
