"""The table-driven fill of X^T's row stream (csrc/tperm.hip: staging slots and tile schedule from the plan) writes the
bytes of the fill it replaces on lsi's hot path (csrc/tpack4.hip, tune ``tperm_off`` = 1): ``ent``, ``sptr`` and ``perm``
byte for byte on every shape of tests/test_gpu_tpack4.py, on ragged / empty / 700-entry rows, dense blocks that do not fit
the staging buffer, tile widths forced to 16, 48, 160 and 512 and one shard-sized matrix; against scipy where that is
cheap; and two fills from one plan with different values."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from muon_amd._backend import _p, check
from tests.test_gpu_kernels import _check_stream, _heavy_rows_csr, _up

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _switches_back(hip):
    yield
    hip.tune("tperm_off", 0)
    hip.tune("tpack4_c", 0)


def _x_stream(hip, X):
    """The row stream of X in the layout made with the device CSR (what the TF-IDF scale sweep writes)."""
    xs, row_dst = hip.stream_layout(X)
    with hip._dev_ctx():
        check(hip.lib.mu_csr_stream_fill(int(xs.perm.numel()), _p(xs.perm), _p(X.indptr), _p(X.indices), _p(X.values),
                                         _p(xs.sptr), _p(xs.ent), hip._stream()))
    return xs, row_dst


def _old_and_new(hip, X, expect_table=True):
    src = _x_stream(hip, X)
    hip.tune("tperm_off", 0)
    new = hip.transpose_stream(X, src=src)
    table = hip._plan_of(X, "tplan").get("tperm")
    assert isinstance(table, dict) == expect_table
    if expect_table:  # every slot lies inside one staging buffer
        assert int(table["slots"].max()) < hip.lib.mu_tperm_stage_pairs()
        assert int(table["slots"].min()) >= 0
    hip.tune("tperm_off", 1)
    old = hip.transpose_stream(X, src=src)
    hip.tune("tperm_off", 0)
    assert old.t4 is not None and new.t4 is not None and torch.equal(old.t4["cnt"], new.t4["cnt"])
    return old, new


def _same_bytes(hip, old, new, nnz):
    assert torch.equal(old.sptr, new.sptr) and torch.equal(old.perm, new.perm) and old.k == new.k
    assert torch.equal(old.ent[:nnz], new.ent[:nnz])


def _compare(hip, m, scipy_too=True):
    X = _up(hip, m)
    assert m.nnz > 0 and hip._use_tpack4(X) and hip._plan_of(X, "tplan") is not None
    old, new = _old_and_new(hip, X)
    _same_bytes(hip, old, new, m.nnz)
    if scipy_too:
        mt = m.T.tocsr()
        mt.sort_indices()
        _check_stream(hip, new, mt)
    return X


@pytest.mark.parametrize("n,d,dens", [(1, 1, 1.0), (7, 5, 0.5), (100, 10, 0.2), (257, 131, 0.08), (300, 9000, 0.01),
                                      (2000, 20000, 0.004), (5000, 700, 0.03), (70, 4097, 0.2), (20000, 3000, 0.03)])
def test_table_path_writes_the_bytes_of_the_old_fill(hip, n, d, dens):
    rng = np.random.default_rng(n * 7 + d)
    _compare(hip, _heavy_rows_csr(n, d, dens, rng, bursts=(n > 8 and d > 40)))


def _bursty(hip, rng):
    """Bursts of 33 .. 400 consecutive columns, empty column ranges, and eight rows of ONE wave with the same 80-column
    burst (more rows over 32 entries than a wave has continuation windows: the plan must narrow the tile).  36 000 rows
    give every wave several rows on any device up to 280 CUs; the rows of the burst are placed by the real geometry."""
    n, d = 36000, 2600
    m = sp.random(n, d, density=0.004, format="lil", random_state=rng, dtype=np.float32)
    for r in rng.choice(n, 200, replace=False):
        c0 = int(rng.integers(0, d - 450))
        L = int(rng.integers(33, 400))
        m[r, c0:c0 + L] = rng.random(L).astype(np.float32) + 0.5
    rpb, _G = hip._t4_geometry(n, d, int(0.004 * n * d))
    rw = rpb // 16
    assert rw >= 8
    for r in range(rpb + 2 * rw, rpb + 2 * rw + 8):  # rows 0 .. 7 of wave 2 of row block 1
        m[r, 100:180] = 1.25
    for r in (3 * rpb + 5 * rw, 3 * rpb + 5 * rw + 1, 3 * rpb + 5 * rw + 3):  # three rows of one wave: 70, 40 and 33 entries
        m[r, 1500:1570] = 0.75
    m[3 * rpb + 5 * rw + 1, 1540:1570] = 0
    m[3 * rpb + 5 * rw + 3, 1533:1570] = 0
    m = m.tocsr()
    m[:, 900:1400] = 0  # empty column ranges
    m[:, 2000:2100] = 0
    m.eliminate_zeros()
    m.sort_indices()
    return m


@pytest.mark.parametrize("C", [0, 16, 48, 160, 512])
def test_bursts_continuations_and_forced_tile_widths(hip, C):
    m = _bursty(hip, np.random.default_rng(100 + C))
    hip.tune("tpack4_c", C)
    _compare(hip, m)


@pytest.mark.parametrize("C", [0, 512])
def test_block_denser_than_the_staging_buffer(hip, C):
    rng = np.random.default_rng(21)
    n, d = 60000, 200
    dense = sp.random(n, 100, density=0.95, format="csr", random_state=rng, dtype=np.float32)
    m = sp.hstack([dense, sp.csr_matrix((n, d - 100), dtype=np.float32)], format="csr")
    m.sort_indices()
    hip.tune("tpack4_c", C)
    _compare(hip, m)


def test_empty_rows_and_row_blocks(hip):
    rng = np.random.default_rng(5)
    m = sp.random(4000, 1500, density=0.03, format="csr", random_state=rng, dtype=np.float32).tolil()
    m[512:1024, :] = 0  # a whole row block
    m[2000:2003, :] = 0
    m = m.tocsr()
    m.eliminate_zeros()
    _compare(hip, m)


def test_two_fills_from_one_plan_with_other_values(hip):
    rng = np.random.default_rng(9)
    m = _heavy_rows_csr(20000, 3000, 0.03, rng)
    X = _compare(hip, m)
    table = hip._plan_of(X, "tplan")["tperm"]
    m2 = m.copy()
    m2.data = rng.standard_normal(m.nnz).astype(np.float32)
    X.values.copy_(torch.from_numpy(m2.data).to(X.values.device))
    old, new = _old_and_new(hip, X)
    assert hip._plan_of(X, "tplan")["tperm"] is table  # (the same table: nothing was planned again)
    _same_bytes(hip, old, new, m.nnz)
    mt = m2.T.tocsr()
    mt.sort_indices()
    _check_stream(hip, new, mt)


def test_tune_key_and_foreign_layouts_keep_the_old_fill(hip):
    rng = np.random.default_rng(3)
    m = _heavy_rows_csr(5000, 700, 0.03, rng)
    X = _up(hip, m)
    hip.tune("tperm_off", 1)
    hip.transpose_stream(X, src=_x_stream(hip, X))
    assert hip._plan_of(X, "tplan").get("tperm") is None
    hip.tune("tperm_off", 0)
    xs, row_dst = _x_stream(hip, X)
    hip.transpose_stream(X, src=(xs, row_dst.clone()))  # (not the plan's layout object: nothing is assumed about it)
    hip.transpose_stream(X)                             # (CSR source)
    assert hip._plan_of(X, "tplan").get("tperm") is None


def test_shard_sized_matrix(hip):
    """125 000 x 200 000 at 3 %: one rank's shard of the flagship shape, from the device-side generator."""
    X = hip.with_slab_ptr(hip.synth_counts(0, 125_000, 200_000, 50, 0.03, 1))
    assert X.values.dtype == torch.float32 and hip._plan_of(X, "tplan") is not None
    old, new = _old_and_new(hip, X)
    _same_bytes(hip, old, new, X.nnz)


def test_table_that_cannot_be_made_keeps_the_old_fill(hip, monkeypatch):
    """No memory for the table (or a refused plan launch): the call succeeds through the old fill, and stays there."""
    rng = np.random.default_rng(4)
    m = _heavy_rows_csr(20000, 3000, 0.03, rng)
    X = _up(hip, m)
    src = _x_stream(hip, X)
    real = hip.empty

    def no_room(shape, dtype, *a, **k):
        if dtype == torch.int16:
            raise torch.OutOfMemoryError("no room for the slot table")
        return real(shape, dtype, *a, **k)

    monkeypatch.setattr(hip, "empty", no_room)
    got = hip.transpose_stream(X, src=src)
    monkeypatch.undo()
    assert hip._plan_of(X, "tplan")["tperm"] is False
    again = hip.transpose_stream(X, src=src)
    assert hip._plan_of(X, "tplan")["tperm"] is False
    mt = m.T.tocsr()
    mt.sort_indices()
    _check_stream(hip, got, mt)
    assert torch.equal(got.ent[:m.nnz], again.ent[:m.nnz])
