"""muon_amd.atac.tl fragment tools (muon_amd/_atac/fragments.py; reference muon/_atac/tools.py:746-1201) against the
reference's own results on the engineered table of tests/golden/make_fragments_golden.py.  Host logic and the tensor
forms of the kernels on the CPU test operator set; the HIP path is exercised by tests/test_gpu_fragments.py."""
import gzip
import warnings

import numpy as np
import pandas as pd
import pytest
import torch

import muon_amd as mu
from muon_amd import AnnData, MuData
from muon_amd import atac as ac
from muon_amd._atac import fragments as fr
from muon_amd._hostmatrix import resident
from tests import frag_fixture as fx
from tests import frag_refs
from tests.cpu_backend import CpuTestBackend

BE = CpuTestBackend()


@pytest.fixture(scope="module")
def g():
    return fx.load()


def _count(a, feats, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", FutureWarning)
        return ac.tl.count_fragments_features(a, feats, **kw)


# -- the three functions against the reference ------------------------------------------------------------------
@pytest.mark.parametrize("reads", [True, False], ids=["reads", "fragments"])
def test_count_fragments_features_equals_reference(g, reads):
    a = fx.adata(g, BE)
    res = _count(a, fx.features(g, False), count_reads=reads)
    ref = g["counts_reads" if reads else "counts_fragments"]
    assert res.shape == ref.shape and res.obs is a.obs and list(res.var_names) == list(g["feat_names"][:ref.shape[1]])
    X = res.X
    assert X.dtype == np.float32 and X.has_canonical_format and X.has_sorted_indices
    assert np.array_equal(np.asarray(X.todense()).astype(np.int64), ref.astype(np.int64))
    assert (X.data != 0).all() and (np.diff(X.indices)[np.diff(np.repeat(np.arange(X.shape[0]),
                                                                       np.diff(X.indptr))) == 0] > 0).all()


def test_count_result_feeds_tfidf_without_an_upload(g):
    res = _count(fx.adata(g, BE), fx.features(g, False))
    dev = resident(res.X, BE)
    assert dev is not None and dev.shape == res.shape
    assert np.array_equal(dev.values.numpy(), res.X.data) and np.array_equal(dev.indices.numpy(), res.X.indices)
    uploads = []
    orig = BE.upload_csr
    BE.upload_csr = lambda *a, **k: (uploads.append(1), orig(*a, **k))[1]
    try:
        ac.pp.tfidf(res, backend=BE)
    finally:
        del BE.upload_csr
    assert not uploads  # the device copy made by the count was used
    assert np.isfinite(res.X.data).all()


@pytest.mark.parametrize("tag,kw", [("tss_default", dict()),
                                    ("tss_600", dict(extend_upstream=600, extend_downstream=600, n_tss=25,
                                                     random_state=7))])
def test_tss_enrichment_equals_reference(g, tag, kw):
    a = fx.adata(g, BE)
    feats = fx.features(g, True)
    res = ac.tl.tss_enrichment(a, feats, backend=BE, **kw)
    # the integer pileup, through the same sampling call
    sub = feats.sample(n=kw["n_tss"], random_state=kw["random_state"]) if "n_tss" in kw else feats
    up, down = kw.get("extend_upstream", 1000), kw.get("extend_downstream", 1000)
    table = a.uns["files"]["fragments"]
    diff = fr.tss_pileup_device(a, sub, up, down)
    W = up + down + 1
    sums = fr.pileup_scan(table, diff, 100, (W - 1001) // 2)
    pile = diff[:, :W].numpy()
    assert pile.dtype == np.int32 and np.array_equal(pile, g[tag + "_pileup"])
    assert np.array_equal(sums[:, 0].numpy(), pile[:, :100].sum(1, dtype=np.int64) + pile[:, -100:].sum(1, dtype=np.int64))
    assert (sums[-10:, 0] == 0).all()  # cells without a fragment: the zero flank mean is replaced
    e_score, e_norm = fx.max_rel(a.obs["tss_score"].values, g[tag + "_score"]), fx.max_rel(res.X, g[tag + "_norm"])
    print(f"{tag}: max rel err tss_score {e_score:.2e}, normalised pileup {e_norm:.2e}")
    assert e_score <= fx.RTOL and e_norm <= fx.RTOL
    assert res.X.dtype == np.float64 and res.shape == (a.n_obs, W)
    assert np.array_equal(res.var["TSS_position"].values, g[tag + "_position"]) and res.var.index[0] == "0"
    assert np.array_equal(res.obs["tss_score"].values, a.obs["tss_score"].values)


@pytest.mark.parametrize("tag,n", [("nuc_all", None), ("nuc_2500", 2500), ("nuc_2500", 2500.0)])
def test_nucleosome_signal_equals_reference(g, tag, n):
    a = fx.adata(g, BE)
    assert ac.tl.nucleosome_signal(a, n=n, backend=BE) is None
    assert np.array_equal(a.obs["nucleosome_signal"].values, g[tag])
    if n is None:  # the cell without a nucleosome-free fragment gets (0 + 1, mono + 1)
        table = a.uns["files"]["fragments"]
        cls = fr.length_classes(table, torch.from_numpy(fr.cell_table(a, table)), a.n_obs, len(table), 147, 294)
        row = list(a.obs_names).index(str(g["no_free_cell"]))
        assert cls[row, 0] == 0 and a.obs["nucleosome_signal"].values[row] == float(cls[row, 1] + 1)


# -- the table ----------------------------------------------------------------------------------------------------
def test_table_survives_filter_obs(g):
    feats = fx.features(g, False)
    a = fx.adata(g, BE)  # table built BEFORE the filter
    a.obs["keep"] = np.arange(a.n_obs) % 3 != 1
    mu.pp.filter_obs(a, "keep")
    assert a.n_obs < len(g["obs_names"])
    b = fx.adata(g, BE, obs_names=np.asarray(a.obs_names))  # ... and AFTER it
    for x in (a, b):
        ac.tl.tss_enrichment(x, fx.features(g, True), return_tss=False)
        ac.tl.nucleosome_signal(x)
    assert np.array_equal(a.obs["tss_score"].values, b.obs["tss_score"].values)
    assert np.array_equal(a.obs["nucleosome_signal"].values, b.obs["nucleosome_signal"].values)
    ca, cb = _count(a, feats), _count(b, feats)
    assert (ca.X != cb.X).nnz == 0
    keep = np.arange(len(g["obs_names"])) % 3 != 1
    assert np.array_equal(np.asarray(ca.X.todense()), g["counts_reads"][keep])
    assert np.array_equal(a.obs["nucleosome_signal"].values, g["nuc_all"][keep])


def test_barcodes_column_is_honoured(g):
    a = fx.adata(g, BE)
    a.obs["bc"] = np.asarray(a.obs_names)
    a.obs.index = pd.Index([f"cell{i}" for i in range(a.n_obs)])
    ac.tl.nucleosome_signal(a, barcodes="bc")
    assert np.array_equal(a.obs["nucleosome_signal"].values, g["nuc_all"])
    ac.tl.tss_enrichment(a, fx.features(g, True), barcodes="bc", return_tss=False)
    assert fx.max_rel(a.obs["tss_score"].values, g["tss_default_score"]) <= fx.RTOL
    # a column that does not exist: the index is used (reference tools.py:1028-1031), and nothing matches
    ac.tl.nucleosome_signal(a, barcodes="nobody")
    assert (a.obs["nucleosome_signal"].values == 1.0).all()
    a.obs["bc"] = [a.obs["bc"].iloc[0]] * a.n_obs
    with pytest.raises(ValueError, match="duplicate"):
        ac.tl.nucleosome_signal(a, barcodes="bc")


def test_duplicate_obs_names_raise(g):
    names = np.asarray(g["obs_names"]).copy()
    names[1] = names[0]
    a = fx.adata(g, BE, obs_names=names)
    with pytest.raises(ValueError, match="duplicate"):
        _count(a, fx.features(g, False))


@pytest.mark.parametrize("five", [True, False], ids=["five-columns", "four-columns"])
def test_locate_fragments_reads_a_gzip_tsv(g, tmp_path, five):
    path = tmp_path / "fragments.tsv.gz"
    cols = [g["chrom"], g["start"], g["end"], g["barcode"]] + ([g["score"]] if five else [])
    with gzip.open(path, "wt") as f:
        f.write("# id=fixture\n# primary_contig=chr1\n")
        for row in zip(*cols):
            f.write("\t".join(str(x) for x in row) + "\n")
    a = fx.adata(g, BE, with_table=False)
    assert ac.tl.locate_fragments(a, str(path), backend=BE) is None
    t = a.uns["files"]["fragments"]
    ref = fx.adata(g, BE).uns["files"]["fragments"]
    assert isinstance(t, ac.tl.FragmentTable) and t.contigs == ref.contigs == ["chr1", "chr2", "chr3"]
    assert list(t.barcodes) == list(ref.barcodes) and np.array_equal(t.chrom_ptr, ref.chrom_ptr)
    assert t.max_len == ref.max_len == 599 and len(t) == len(g["start"])
    for name in ("chrom", "start", "end", "barcode"):
        assert getattr(t, name).dtype == torch.int32 and torch.equal(getattr(t, name), getattr(ref, name))
    assert torch.equal(t.score, ref.score if five else torch.ones_like(ref.score))
    # a table is taken as it is, and handed back on request
    b = fx.adata(g, BE, with_table=False)
    assert ac.tl.locate_fragments(b, t, return_fragments=True) is t and b.uns["files"]["fragments"] is t


def test_unsorted_input_raises_and_sort_fixes_it(g):
    rng = np.random.default_rng(0)
    p = rng.permutation(len(g["start"]))
    cols = [g[k][p] for k in ("chrom", "start", "end", "barcode", "score")]
    a = fx.adata(g, BE, with_table=False)
    with pytest.raises(ValueError, match="sort"):
        ac.tl.fragments_from_arrays(a, *cols, backend=BE)
    assert "files" not in a.uns
    # sorted inside the contigs, but a contig in two pieces
    half = len(p) // 2
    q = np.concatenate([np.arange(half, len(p)), np.arange(half)])
    with pytest.raises(ValueError, match="grouped"):
        ac.tl.fragments_from_arrays(a, *[g[k][q] for k in ("chrom", "start", "end", "barcode", "score")], backend=BE)
    ac.tl.fragments_from_arrays(a, *cols, sort=True, backend=BE)
    assert _count(a, fx.features(g, False), count_reads=False).X.sum() == g["counts_fragments"].sum()
    assert np.array_equal(np.asarray(_count(a, fx.features(g, False)).X.todense()), g["counts_reads"])
    with pytest.raises(ValueError):
        ac.tl.fragments_from_arrays(a, g["chrom"], g["start"], g["end"][:-1], g["barcode"], backend=BE)
    t = ac.tl.fragments_from_arrays(a, g["chrom"], g["start"], g["end"], g["barcode"], backend=BE)  # score=None
    assert t.max_score == 1 and bool((t.score == 1).all())
    assert np.array_equal(np.asarray(_count(a, fx.features(g, False)).X.todense()), g["counts_fragments"])


def test_return_tss_false_returns_none_and_writes_the_column(g):
    a = fx.adata(g, BE)
    downloads = []
    orig = BE.to_host
    BE.to_host = lambda t, out=None: (downloads.append(tuple(t.shape)), orig(t, out))[1]
    try:
        assert ac.tl.tss_enrichment(a, fx.features(g, True), return_tss=False) is None
    finally:
        del BE.to_host
    assert downloads == [(a.n_obs, 2)]  # the n x W pileup is never downloaded
    assert fx.max_rel(a.obs["tss_score"].values, g["tss_default_score"]) <= fx.RTOL


# -- dispatch, errors and warnings of the reference ---------------------------------------------------------------
def test_mudata_dispatch_and_type_errors(g):
    a = fx.adata(g, BE)
    md = MuData({"atac": a})
    ac.tl.nucleosome_signal(md)
    assert np.array_equal(md.mod["atac"].obs["nucleosome_signal"].values, g["nuc_all"])
    for fn in (ac.tl.nucleosome_signal, ac.tl.tss_enrichment, ac.tl.count_fragments_features):
        with pytest.raises(TypeError, match="Expected AnnData or MuData object with 'atac' modality"):
            fn(MuData({"rna": fx.adata(g, BE, with_table=False)}))
        with pytest.raises(TypeError, match="Expected AnnData"):
            fn(np.zeros((3, 3)))


def test_missing_and_unread_fragments(g):
    feats = fx.features(g, True)
    a = fx.adata(g, BE, with_table=False)
    calls = (lambda x: ac.tl.count_fragments_features(x, feats), lambda x: ac.tl.tss_enrichment(x, feats),
             lambda x: ac.tl.nucleosome_signal(x))
    for call in calls:
        with pytest.raises(KeyError, match="There is no fragments file located yet"):
            call(a)
    a.uns["files"] = {"fragments": "atac_fragments.tsv.gz"}
    for call in calls:
        with pytest.raises(TypeError, match="locate_fragments"):
            call(a)


def test_features_argument(g):
    a = fx.adata(g, BE)
    for fn in (ac.tl.count_fragments_features, ac.tl.tss_enrichment):
        with pytest.raises(ValueError, match="Argument `features` is required"):
            fn(a)
    feats = fx.features(g, False)
    with pytest.warns(FutureWarning, match="unique fragments will be counted"):
        ac.tl.count_fragments_features(a, feats)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ac.tl.count_fragments_features(a, feats, count_reads=False)
    with pytest.raises(ValueError, match="No column with feature starts"):
        _count(a, feats.drop(columns="Start"))
    with pytest.raises(ValueError, match="No column with feature ends"):
        _count(a, feats.drop(columns="End"))
    with pytest.raises(ValueError, match="No column with chromosome"):
        _count(a, feats.drop(columns="Chromosome"))
    with pytest.raises(ValueError, match="No column with strand"):
        _count(a, feats, stranded=True)
    # case-insensitive names; "chromosome" takes precedence over "chr"
    odd = feats.rename(columns={"Chromosome": "CHROMOSOME", "Start": "start", "End": "END"})
    odd["chr"] = "nowhere"
    assert np.array_equal(np.asarray(_count(a, odd).X.todense()), g["counts_reads"])
    # a feature on a contig the table lacks counts nothing
    res = _count(a, fx.features(g, True))
    assert res.X[:, -1].nnz == 0 and np.array_equal(np.asarray(res.X.todense())[:, :-1], g["counts_reads"])


def test_strands_are_honoured(g):
    a = fx.adata(g, BE)
    feats = fx.features(g, False).copy()
    feats["Strand"] = np.where(np.arange(len(feats)) % 2 == 0, "+", "-")
    res = np.asarray(_count(a, feats, stranded=True, extend_upstream=700, extend_downstream=50).X.todense())
    flipped = feats.copy()
    minus = (feats.Strand == "-").values
    # a "-" feature with (up, down) is the unstranded window of (start - down, end + up)
    flipped.loc[minus, "Start"] = feats.Start[minus] - 50 + 700
    flipped.loc[minus, "End"] = feats.End[minus] + 700 - 50
    ref = np.asarray(_count(a, flipped.drop(columns="Strand"), extend_upstream=700, extend_downstream=50).X.todense())
    assert np.array_equal(res, ref)
    plain = np.asarray(_count(a, feats, extend_upstream=700, extend_downstream=50).X.todense())  # stranded=False
    assert not np.array_equal(res, plain)


def test_features_from_the_rna_modality(g):
    a = fx.adata(g, BE)
    feats = fx.features(g, False)
    var = pd.DataFrame({"gene_ids": [f"ENSG{i}" for i in range(len(feats))],
                        "interval": [f"{c}:{s}-{e}" for c, s, e in zip(feats.Chromosome, feats.Start, feats.End)]},
                       index=feats.index)
    rna = AnnData(np.zeros((a.n_obs, len(feats))), obs=pd.DataFrame(index=a.obs_names), var=var)
    res = _count(MuData({"atac": a, "rna": rna}), None)
    assert np.array_equal(np.asarray(res.X.todense()), g["counts_reads"])
    assert list(res.var.columns) == ["Chromosome", "Start", "End", "gene_id", "gene_name"]


def test_tss_score_errors(g):
    a = fx.adata(g, BE)
    with pytest.raises(ValueError, match=r"`center_size` \(1001\) must smaller than the piled up region \(801\)"):
        ac.tl.tss_enrichment(a, fx.features(g, True), extend_upstream=400, extend_downstream=400)
    with pytest.raises(ValueError, match="must be an uneven number, but is 1000"):
        fr._check_tss_score(2001, 100, 1000)
    assert "tss_score" not in a.obs.columns


def test_pileup_overflow_is_refused(g):
    a = fx.adata(g, BE)
    a.uns["files"]["fragments"].max_score = 2 ** 31 - 1
    with pytest.raises(ValueError, match="overflow"):
        ac.tl.tss_enrichment(a, fx.features(g, True))


# -- the tensor forms on the fixture's edges ---------------------------------------------------------------------
def test_candidate_ranges_hit_the_lane_and_chunk_edges(g):
    a = fx.adata(g, BE)
    table = a.uns["files"]["fragments"]
    feats = fx.features(g, True)
    wchrom, wlo, whi = fr._windows(table, feats.Chromosome.values, feats.Start.values - 2000, feats.End.values)
    assert int(wchrom[-1]) == -1 and int(wlo.min()) < 0
    lo, ln = fr.window_ranges(table, wchrom, wlo, whi)
    assert np.array_equal(ln[:-1].numpy(), g["count_candidates"]) and int(ln[-1]) == 0
    assert {0, 1, 63, 64, 65, 255, 256, 257} <= set(ln.tolist()) and int(ln.max()) > 1000
    # every candidate range lies inside its contig's segment
    seg = torch.from_numpy(table.chrom_ptr)
    c = wchrom[:-1].long()
    assert bool((lo[:-1] >= seg[c]).all()) and bool((lo[:-1] + ln[:-1] <= seg[c + 1]).all())


# -- tests/frag_refs.py (brute force) against the tensor forms, and the inputs of tests/test_gpu_fragments_stride.py ----
def _ref_equals_tensor_forms(table, cell_of, n_obs, wchrom, wlo, whi, width):
    """every pass of tests/frag_refs.py against the package's tensor form on one table and one set of windows"""
    col = {k: getattr(table, k).numpy() for k in ("chrom", "start", "end", "barcode", "score")}
    w = [t.numpy() for t in (wchrom, wlo, whi)]
    cells = torch.from_numpy(cell_of)
    n_feat = int(wlo.numel())
    rlo, rln = fr.ranges_tensor(table, wchrom, wlo, whi)
    ln = frag_refs.range_lengths(col["chrom"], col["start"], *w, table.max_len)
    assert np.array_equal(rln.numpy(), ln)
    for use_score in (True, False):
        keys, vals = fr.overlap_tensor(table, cells, wlo, whi, rlo, rln, n_feat, use_score)
        rkeys, rvals = frag_refs.overlap(col["chrom"], col["start"], col["end"], col["barcode"],
                                         col["score"] if use_score else None, cell_of, n_obs, *w, n_feat)
        assert keys.numel() > 0 and np.array_equal(keys.numpy(), rkeys) and np.array_equal(vals.numpy(), rvals)
    if width is not None:
        diff = fr.pileup_tensor(table, cells, n_obs, wlo, whi, rlo, rln, width)
        rdiff = frag_refs.pileup_diff(col["chrom"], col["start"], col["end"], col["barcode"], col["score"], cell_of,
                                      n_obs, *w, width)
        assert np.array_equal(diff.numpy(), rdiff) and int(np.abs(rdiff).sum()) > 0 and int(rdiff.sum()) == 0
        cd = (width - 1001) // 2
        pile, rsums = frag_refs.pileup_scan(rdiff, 100, cd)
        sums = fr.scan_tensor(diff, 100, cd)
        assert np.array_equal(diff[:, :width].numpy(), pile) and np.array_equal(sums.numpy(), rsums)
    for n_take in (len(table), len(table) // 3, 0):
        cls = fr.length_classes_tensor(table, cells, n_obs, n_take, 147, 294)
        assert np.array_equal(cls.numpy(), frag_refs.length_classes(col["start"], col["end"], col["barcode"], cell_of,
                                                                     n_obs, n_take, 147, 294))
    return ln


def test_frag_refs_equal_the_tensor_forms_on_the_engineered_table(g):
    a = fx.adata(g, BE)
    table = a.uns["files"]["fragments"]
    feats = fx.features(g, True)
    cell_of = fr.cell_table(a, table)
    genes = fr._windows(table, feats.Chromosome.values, feats.Start.values - 2000, feats.End.values)
    ln = _ref_equals_tensor_forms(table, cell_of, a.n_obs, *genes, None)
    assert {0, 1, 63, 64, 65, 255, 256, 257} <= set(ln.tolist())
    s = feats.Start.values.astype(np.int64)
    _ref_equals_tensor_forms(table, cell_of, a.n_obs, *fr._windows(table, feats.Chromosome.values, s - 1000, s + 1000), 2001)


def test_stride_table_on_the_tensor_forms():
    """the table and the windows of tests/test_gpu_fragments_stride.py: at the size of a 16-CU part through every
    tensor form, and at the size of a 256-CU part the properties the GPU case asserts"""
    df, obs = fx.stride_table()
    table = fr.make_table(df.chrom.values, df.start.values, df.end.values, df.barcode.values, df.score.values, backend=BE)
    cell_of = pd.Index(obs).get_indexer(table.barcodes).astype(np.int32)
    assert table.contigs == ["a", "b"] and (cell_of == -1).sum() == 13 and len(obs) == 25
    names, lo, hi = fx.stride_windows(2 * fx.wave_grid(16) + 1)
    ln = _ref_equals_tensor_forms(table, cell_of, len(obs), *fr._windows(table, names, lo, hi), 1201)
    assert int((-(-ln // fx.CHUNK)).sum()) >= 2 * fx.wave_grid(16) + 1
    # a 256-CU part: 2 * 64 * 256 + 1 chunks from about 20 000 windows
    names, lo, hi = fx.stride_windows(2 * fx.wave_grid(256) + 1)
    wchrom, wlo, whi = (t.numpy() for t in fr._windows(table, names, lo, hi))
    ln = frag_refs.range_lengths(table.chrom.numpy(), table.start.numpy(), wchrom, wlo, whi, table.max_len)
    assert int((-(-ln // fx.CHUNK)).sum()) >= 2 * 64 * 256 + 1 and 18_000 < len(names) < 26_000
    assert {0, 1, 255, 256, 257} <= set(ln.tolist()) and ln.max() >= 700
    assert (wchrom == -1).any() and (wlo < 0).any()
    empty = ln == 0
    assert (empty[1:-1] & empty[2:] & ~empty[:-2]).any() and not empty[0]


def test_scan_and_length_class_inputs_on_the_tensor_forms():
    n = 0
    for diff, flank, centre in fx.scan_cases():
        W = diff.shape[1] - 1
        pile, sums = frag_refs.pileup_scan(diff, flank, centre)
        d = torch.from_numpy(diff.copy())
        assert np.array_equal(fr.scan_tensor(d, flank, centre).numpy(), sums)
        assert np.array_equal(d[:, :W].numpy(), pile) and np.array_equal(d[:, W].numpy(), diff[:, W])
        assert np.abs(diff).max() <= 50 and diff.shape[0] == 5
        n += 1
    assert n == 4 * len(fx.SCAN_WIDTHS) - 3 and fx.SCAN_WIDTHS == (1, 63, 64, 65, 129, 2001)
    # the raw columns: the tensor form takes neither an out-of-range barcode nor a cell past n_obs, so both are first
    # mapped to "no cell" by hand; the restatement takes the columns as they are
    assert fx.thread_grid(256) == 16 * 256 * 256
    n = 2 * fx.thread_grid(4) + 123
    start, end, barcode, cell_of, n_obs = fx.length_class_columns(n)
    assert (barcode < 0).any() and (barcode >= cell_of.size).any() and (cell_of < 0).any() and (cell_of >= n_obs).any()
    assert {146, 147, 293, 294} <= set((end.astype(np.int64) - start).tolist())
    tame_cells = np.append(np.where(cell_of >= n_obs, -1, cell_of), -1).astype(np.int32)
    tame = np.where((barcode < 0) | (barcode >= cell_of.size), cell_of.size, barcode).astype(np.int32)
    table = type("Columns", (), {"start": torch.from_numpy(start), "end": torch.from_numpy(end),
                                 "barcode": torch.from_numpy(tame), "__len__": lambda self: n})()
    for n_take in (n, n // 3, fx.thread_grid(4) + 1):
        want = frag_refs.length_classes(start, end, barcode, cell_of, n_obs, n_take, 147, 294)
        got = fr.length_classes_tensor(table, torch.from_numpy(tame_cells), n_obs, n_take, 147, 294)
        assert np.array_equal(got.numpy(), want) and (want.sum(axis=0) > 0).all()
