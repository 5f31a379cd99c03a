"""csrc/fragments.hip on the GPU: every pass against its tensor form (muon_amd/_atac/fragments.py), exactly, on the
fixture of tests/golden/make_fragments_golden.py and on a table engineered around the 256-candidate chunk, and the three
public functions end to end against the reference's results (muon/_atac/tools.py:746-1201)."""
import warnings

import numpy as np
import pandas as pd
import pytest
import torch

from muon_amd import AnnData
from muon_amd import atac as ac
from muon_amd._atac import fragments as fr
from muon_amd._hostmatrix import resident
from tests import frag_fixture as fx

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    return fx.load()


def _engineered():
    """~2 000 fragments on two contigs: windows whose candidates number exactly 256 and 257 (one chunk; one chunk and a
    single lane), 0 and 700, a window on a contig the table lacks and one that starts below 0; 37 barcodes of which
    every third is no cell."""
    rng = np.random.default_rng(5)
    rows = []

    def cluster(chrom, lo, hi, count):
        for s in np.sort(rng.integers(lo, hi, count)):
            rows.append((chrom, int(s), int(s) + int(rng.integers(20, 400)), f"b{int(rng.integers(0, 37))}",
                         int(rng.integers(1, 6))))

    cluster("a", 200, 900, 300)            # around the window that starts below 0
    cluster("a", 100_000, 101_000, 256)
    cluster("a", 200_000, 201_000, 257)
    cluster("a", 300_000, 301_200, 700)
    cluster("b", 50_000, 51_000, 500)
    df = pd.DataFrame(rows, columns=["chrom", "start", "end", "barcode", "score"])
    df = df.sort_values(["chrom", "start"], kind="stable")
    # windows of width 1201 (600/600) around these positions
    feats = pd.DataFrame({"Chromosome": ["a", "a", "a", "a", "a", "b", "zz"],
                          "Start": [400, 100_500, 200_500, 300_600, 400_000, 50_500, 1000]})
    obs = [f"b{i}" for i in range(37) if i % 3] + ["nobody"]
    return df, feats, obs


def _windows_of(table, feats, up, down):
    s = feats.Start.values.astype(np.int64)
    return fr._windows(table, feats.Chromosome.values, s - up, s + down)


def _cases(g, hip):
    a = fx.adata(g, hip)
    table = a.uns["files"]["fragments"]
    feats = fx.features(g, True)
    yield "fixture-genes", a, table, fr._windows(table, feats.Chromosome.values, feats.Start.values - 2000,
                                                 feats.End.values), None
    yield "fixture-tss", a, table, _windows_of(table, feats, 1000, 1000), 2001
    df, efeats, obs = _engineered()
    b = AnnData(np.zeros((len(obs), 1)), obs=pd.DataFrame(index=pd.Index(obs)))
    t = ac.tl.fragments_from_arrays(b, df.chrom.values, df.start.values, df.end.values, df.barcode.values,
                                    df.score.values, backend=hip)
    yield "engineered", b, t, _windows_of(t, efeats, 600, 600), 1201


def test_every_pass_equals_its_tensor_form(g, hip):
    for name, a, table, (wchrom, wlo, whi), width in _cases(g, hip):
        cell_of = hip.to_device(fr.cell_table(a, table), np.int32)
        n = a.n_obs
        lo, ln = hip.frag_ranges(table.start, table.chrom_ptr_device, wchrom, wlo, whi, table.max_len)
        rlo, rln = fr.ranges_tensor(table, wchrom, wlo, whi)
        assert lo.dtype == ln.dtype == torch.int64 and torch.equal(ln, rln), name
        assert torch.equal(lo[ln > 0], rlo[rln > 0]), name
        lens = set(ln.tolist())
        if name == "engineered":
            assert {0, 256, 257} <= lens and max(lens) > 512
        elif width is None:
            assert {0, 1, 63, 64, 65, 255, 256, 257} <= lens and max(lens) > 1000
        n_feat = int(wlo.numel())
        for use_score in (True, False):
            keys, vals = fr.overlap_triplets(table, cell_of, n, wlo, whi, lo, ln, n_feat, use_score)
            rkeys, rvals = fr.overlap_tensor(table, cell_of, wlo, whi, rlo, rln, n_feat, use_score)
            assert keys.dtype == torch.int64 and vals.dtype == torch.int32 and keys.numel() == rkeys.numel() > 0
            got = torch.stack([keys, vals.long()], 1).cpu().numpy()
            want = torch.stack([rkeys, rvals.long()], 1).cpu().numpy()
            assert np.array_equal(got[np.lexsort(got.T[::-1])], want[np.lexsort(want.T[::-1])]), name
            assert np.array_equal(got, want), name  # ... and the order is the tensor form's: windows, then file order
        if width is not None:
            diff = fr.pileup_diff(table, cell_of, n, wlo, whi, lo, ln, width)
            rdiff = fr.pileup_tensor(table, cell_of, n, wlo, whi, rlo, rln, width)
            assert diff.shape == (n, width + 1) and torch.equal(diff, rdiff) and int(diff.abs().sum()) > 0, name
            assert int(diff.sum()) == 0
            cd = (width - 1001) // 2
            sums, rsums = hip.frag_pileup_scan(diff, 100, cd), fr.scan_tensor(rdiff, 100, cd)
            assert torch.equal(diff, rdiff) and torch.equal(sums, rsums) and int(sums.sum()) > 0, name
        for n_take in (len(table), len(table) // 3, 0, 10 * len(table)):
            cls = hip.frag_length_classes(table.start, table.end, table.barcode, cell_of, n, n_take, 147, 294)
            assert torch.equal(cls, fr.length_classes_tensor(table, cell_of, n, n_take, 147, 294)), name
        assert int(cls.sum()) > 0


def test_public_functions_equal_the_reference(g, hip):
    a = fx.adata(g, hip)
    for reads in (True, False):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", FutureWarning)
            res = ac.tl.count_fragments_features(a, fx.features(g, False), count_reads=reads)
        ref = g["counts_reads" if reads else "counts_fragments"]
        assert res.X.dtype == np.float32 and res.X.has_canonical_format
        assert np.array_equal(np.asarray(res.X.todense()).astype(np.int64), ref.astype(np.int64))
    dev = resident(res.X, hip)
    assert dev is not None and np.array_equal(dev.values.cpu().numpy(), res.X.data)
    uploads = []
    orig = hip.upload_csr
    hip.upload_csr = lambda *a_, **k: (uploads.append(1), orig(*a_, **k))[1]
    try:
        ac.pp.tfidf(res, backend=hip)
    finally:
        del hip.upload_csr
    assert not uploads and np.isfinite(res.X.data).all()

    for tag, kw in (("tss_default", dict()),
                    ("tss_600", dict(extend_upstream=600, extend_downstream=600, n_tss=25, random_state=7))):
        res = ac.tl.tss_enrichment(a, fx.features(g, True), **kw)
        e_score, e_norm = fx.max_rel(a.obs["tss_score"].values, g[tag + "_score"]), fx.max_rel(res.X, g[tag + "_norm"])
        print(f"{tag}: max rel err tss_score {e_score:.2e}, normalised pileup {e_norm:.2e}")
        assert e_score <= fx.RTOL and e_norm <= fx.RTOL
        assert np.array_equal(res.var["TSS_position"].values, g[tag + "_position"])
    score = a.obs["tss_score"].values.copy()
    assert ac.tl.tss_enrichment(a, fx.features(g, True), return_tss=False, extend_upstream=600, extend_downstream=600,
                                n_tss=25, random_state=7) is None
    assert np.array_equal(a.obs["tss_score"].values, score)

    for tag, n in (("nuc_all", None), ("nuc_2500", 2500)):
        assert ac.tl.nucleosome_signal(a, n=n) is None
        assert np.array_equal(a.obs["nucleosome_signal"].values, g[tag])
