"""The flat read-in fill's slot table in read order (csrc/tflat.hip: `k_tflat_plan<true>` writes a wave's slots into the
CSR range of its rows, tile after tile, in the order the wave's lanes take the pairs; `k_tflat_move` reads them through
a wave-uniform pointer), at the shapes of tests/test_gpu_tflat.py: 160 077 rows, blocks of 512, 200 columns, tiles
forced to 48 columns.  Two checks per case: the plan kernel's ``slots`` of chosen row blocks == the numpy restatement
(`slots_block`, tests/test_tflat_slots_host.py, which fills with it on the CPU), and the flat fill == `k_t4_fill` with
``==``, once more through a buffer of sentinels."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests.test_gpu_kernels import _check_stream, _up
from tests.test_gpu_tflat import N512, _fill, _guarded_flat_fill
from tests.test_gpu_tperm import _same_bytes, _x_stream
from tests.test_tflat_plan_host import NW, plan_block
from tests.test_tflat_slots_host import check_edge_matrix, edge_matrix, slots_block

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _switches_back(hip):
    yield
    for key, default in (("tperm_off", 0), ("tperm_flat", 1), ("tpack4_c", 0)):
        hip.tune(key, default)


def _fills(hip, m):
    """`k_t4_fill` and the flat fill of `m`, equal; returns (device CSR, row stream, the flat fill's table)"""
    X = _up(hip, m)
    assert m.nnz > 0 and hip._use_tpack4(X) and hip._plan_of(X, "tplan") is not None
    src = _x_stream(hip, X)
    ref = _fill(hip, X, src, 1, 0)
    flat = _fill(hip, X, src, 0, 1)
    tp = hip._plan_of(X, "tplan").get("tperm")
    assert isinstance(tp, dict) and "counts" in tp and tp["slots"].numel() == m.nnz
    _same_bytes(hip, ref, flat, m.nnz)
    _guarded_flat_fill(hip, X, src, ref)
    return X, src, tp


def _slots_of_blocks(hip, m, tp, blocks):
    """the plan kernel's slots of the given row blocks == the numpy restatement's"""
    n, d = m.shape
    rpb, _G = hip._t4_geometry(n, d, m.nnz)
    cap, wcap = hip.lib.mu_tperm_stage_pairs(), 64 * hip.lib.mu_tflat_rounds()
    got = hip.to_host(tp["slots"]).view(np.uint16).astype(np.int64)
    for g in blocks:
        r0, r1 = g * rpb, min((g + 1) * rpb, n)
        tiles, counts = plan_block(m.indptr, m.indices, r0, r1, d, tp["tile_cols"], rpb // NW, wcap, cap)
        want = slots_block(m.indptr, m.indices, r0, r1, tiles, counts, rpb // NW)
        assert np.array_equal(got[m.indptr[r0]:m.indptr[r1]], want), g
    return rpb


def test_slots_in_read_order_on_the_edge_matrix(hip):
    """A wave with no pair in a tile between tiles where it has some, on an odd CSR base that puts every round across a
    128-byte line; wave totals of 63, 64, 65 and 64 R; empty rows first, last and in runs inside a wave; an empty row
    block; a ragged last block whose waves without rows share one base."""
    R = hip.lib.mu_tflat_rounds()
    m = edge_matrix(N512, R, np.random.default_rng(71))
    check_edge_matrix(m, R)
    rpb, G = hip._t4_geometry(N512, 200, m.nnz)
    assert rpb == 512 and N512 - (G - 1) * rpb == 333 and m[(G - 1) * rpb:].nnz > 0
    hip.tune("tpack4_c", 48)
    X, _src, tp = _fills(hip, m)
    assert tp["tile_cols"] == 48
    _slots_of_blocks(hip, m, tp, [0, 1, 2, 3, 4, G - 1])
    mt = m.T.tocsr()
    mt.sort_indices()
    hip.tune("tperm_flat", 1)
    _check_stream(hip, hip.transpose_stream(X, src=_src), mt)


@pytest.mark.parametrize("C", [16, 48, 160, 512])
def test_last_column_at_forced_tile_widths(hip, C):
    rng = np.random.default_rng(46)
    m = sp.random(3000, 1000, density=0.03, format="lil", random_state=rng, dtype=np.float32)
    m[::3, 999] = 1.5  # the last column: populated in every block
    m[:, 990:999] = 0  # ... behind empty ones
    m = m.tocsr()
    m.eliminate_zeros()
    m.sort_indices()
    hip.tune("tpack4_c", C)
    _X, _src, tp = _fills(hip, m)
    assert tp["tile_cols"] == C
    rpb, G = hip._t4_geometry(3000, 1000, m.nnz)
    _slots_of_blocks(hip, m, tp, [0, G - 1])


def test_two_fills_from_one_plan_with_other_values(hip):
    rng = np.random.default_rng(72)
    m = sp.random(N512, 200, density=0.03, format="csr", random_state=rng, dtype=np.float32)
    m.sort_indices()
    X, src, tp = _fills(hip, m)
    m2 = m.copy()
    m2.data = rng.standard_normal(m.nnz).astype(np.float32)
    X.values.copy_(torch.from_numpy(m2.data).to(X.values.device))
    src = _x_stream(hip, X)
    ref, flat = _fill(hip, X, src, 1, 0), _fill(hip, X, src, 0, 1)
    assert hip._plan_of(X, "tplan")["tperm"] is tp  # (the same table: nothing was planned again)
    _same_bytes(hip, ref, flat, m.nnz)
    mt = m2.T.tocsr()
    mt.sort_indices()
    _check_stream(hip, flat, mt)
    G = (N512 + 511) // 512
    _slots_of_blocks(hip, m, tp, [0, G // 2, G - 1])
