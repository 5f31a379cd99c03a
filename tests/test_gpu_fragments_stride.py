"""csrc/fragments.hip past one grid: more chunks than waves in the three chunk kernels (``c += n_waves``), more cells
than waves and every column count around the 64-column step in k_frag_pileup_scan, more fragments than threads in
k_frag_length_classes - against tests/frag_refs.py, a brute-force numpy statement that shares nothing with the package.
Everything is integer: every comparison is ==.

The grid rules are restated in tests/frag_fixture (``wave_grid``: a wave per work item, 16 blocks of 4 waves per CU;
``thread_grid``: 16 blocks of 256 threads per CU) next to the CU count read from the device, and every case asserts that
its input still crosses the cap (DESIGN.md 9.6 lists the rules and the smallest inputs).  The CPU suite runs the same
inputs through the tensor forms (tests/test_fragments_host.py).

Sensitivity, tried on an MI355X with one-line changes that produce wrong values only: k_frag_overlap_emit taking only
its first stride step fails test_more_chunks_than_waves alone (tests/test_gpu_fragments.py passes); a carry of zero in
k_frag_pileup_scan fails both scan tests here (and tests/test_gpu_fragments.py, whose widths 1201 and 2001 need it)."""
import numpy as np
import pandas as pd
import pytest
import torch

from muon_amd._atac import fragments as fr
from tests import frag_fixture as fx
from tests import frag_refs

pytestmark = pytest.mark.gpu


def _cus(hip):
    return int(torch.cuda.get_device_properties(hip.device).multi_processor_count)


def test_more_chunks_than_waves(hip):
    """ranges, both overlap passes and the pileup over ~20 000 windows of 0, 1, 255, 256, 257, ~700 candidates: every
    wave of the capped grid takes a second chunk, some a third; windows without a candidate lie between the others (chunk_window's
    search crosses runs of equal chunk_ptr), some on a contig the table lacks, some with lo < 0"""
    n_waves = fx.wave_grid(_cus(hip))
    df, obs = fx.stride_table()
    table = fr.make_table(df.chrom.values, df.start.values, df.end.values, df.barcode.values, df.score.values,
                          backend=hip)
    names, lo, hi = fx.stride_windows(2 * n_waves + 1)
    wchrom, wlo, whi = fr._windows(table, names, lo, hi)
    cell_of = pd.Index(obs).get_indexer(table.barcodes).astype(np.int32)  # barcode code -> row, -1: no cell
    n_obs, n_win, width = len(obs), len(names), 1201
    host = {k: getattr(table, k).cpu().numpy() for k in ("chrom", "start", "end", "barcode", "score")}
    w_host = [t.cpu().numpy() for t in (wchrom, wlo, whi)]
    assert (w_host[0] == -1).any() and (w_host[1] < 0).any() and (cell_of == -1).any()

    want_len = frag_refs.range_lengths(host["chrom"], host["start"], *w_host, table.max_len)
    n_chunks = int((-(-want_len // fx.CHUNK)).sum())
    print(f"{n_win} windows, {n_chunks} chunks, {n_waves} waves")
    assert n_chunks >= 2 * n_waves + 1
    assert {0, 1, 255, 256, 257} <= set(want_len.tolist()) and want_len.max() >= 700
    empty = want_len == 0
    assert (empty[1:-1] & empty[2:] & ~empty[:-2]).any() and not empty[0]  # runs of empty windows between others

    rng_lo, rng_len = hip.frag_ranges(table.start, table.chrom_ptr_device, wchrom, wlo, whi, table.max_len)
    assert np.array_equal(rng_len.cpu().numpy(), want_len)

    cell_d = hip.to_device(cell_of, np.int32)
    args = (host["chrom"], host["start"], host["end"], host["barcode"])
    want_keys, want_vals = frag_refs.overlap(*args, host["score"], cell_of, n_obs, *w_host, n_win)
    keys, vals = hip.frag_overlap(table.start, table.end, table.barcode, table.score, cell_d, n_obs, wlo, whi, rng_lo,
                                  rng_len, n_win)
    assert keys.dtype == torch.int64 and vals.dtype == torch.int32 and want_keys.size > n_chunks
    assert np.array_equal(keys.cpu().numpy(), want_keys) and np.array_equal(vals.cpu().numpy(), want_vals)
    keys, vals = hip.frag_overlap(table.start, table.end, table.barcode, None, cell_d, n_obs, wlo, whi, rng_lo,
                                  rng_len, n_win)
    assert np.array_equal(keys.cpu().numpy(), want_keys) and np.array_equal(vals.cpu().numpy(), np.ones_like(want_vals))

    want_diff = frag_refs.pileup_diff(*args, host["score"], cell_of, n_obs, *w_host, width)
    diff = hip.frag_pileup(table.start, table.end, table.barcode, table.score, cell_d, n_obs, wlo, whi, rng_lo,
                           rng_len, width).cpu().numpy()
    assert diff.shape == (n_obs, width + 1) and np.array_equal(diff, want_diff)
    assert int(diff.sum(dtype=np.int64)) == 0 and int(np.abs(diff).sum(dtype=np.int64)) > 0


def _scan_check(hip, diff, flank, centre):
    W = diff.shape[1] - 1
    pile, want = frag_refs.pileup_scan(diff, flank, centre)
    d = hip.to_device(diff, np.int32)
    sums = hip.frag_pileup_scan(d, flank, centre).cpu().numpy()
    got = d.cpu().numpy()
    assert np.array_equal(got[:, :W], pile) and np.array_equal(got[:, W], diff[:, W]), (W, flank, centre)
    assert sums.dtype == np.int64 and np.array_equal(sums, want), (W, flank, centre)


def test_pileup_scan_carry_edges(hip):
    """widths 1, 63, 64, 65, 129, 2001 (under, at and over one and two 64-column steps) with an empty and the widest
    flank, the whole row and the narrowest centre"""
    n = 0
    for diff, flank, centre in fx.scan_cases():
        _scan_check(hip, diff, flank, centre)
        n += 1
    assert n == 4 * len(fx.SCAN_WIDTHS) - 3  # (width 1: W // 2 == 0)


def test_pileup_scan_more_cells_than_waves(hip):
    n_waves = fx.wave_grid(_cus(hip))
    n = 2 * n_waves + 3  # every wave takes a second row, the first three a third
    diff = np.random.default_rng(10).integers(-50, 51, size=(n, 66)).astype(np.int32)
    assert diff.shape[0] >= 2 * n_waves + 1
    _scan_check(hip, diff, 20, 10)


def test_length_classes_more_fragments_than_threads(hip):
    """raw int32 columns: lengths on both sides of 147 and 294, barcodes below 0 and past the table, cells -1 and past
    n_obs; the whole table, a third of it (one stride step for most threads) and one fragment more than the grid"""
    stride = fx.thread_grid(_cus(hip))
    n = 2 * stride + 123
    start, end, barcode, cell_of, n_obs = fx.length_class_columns(n)
    assert (barcode < 0).any() and (barcode >= cell_of.size).any() and (cell_of < 0).any() and (cell_of >= n_obs).any()
    assert {146, 147, 293, 294} <= set(np.unique(end.astype(np.int64) - start).tolist())
    dev = [hip.to_device(a, np.int32) for a in (start, end, barcode, cell_of)]
    for n_take in (n, n // 3, stride + 1):
        got = hip.frag_length_classes(*dev, n_obs, n_take, 147, 294).cpu().numpy()
        want = frag_refs.length_classes(start, end, barcode, cell_of, n_obs, n_take, 147, 294)
        assert got.dtype == np.int32 and np.array_equal(got, want), n_take
        assert (want.sum(axis=0) > 0).all()
