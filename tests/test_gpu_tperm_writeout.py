"""The FLAT write-out of the table-driven fill (csrc/tperm.hip: lane i of the workgroup takes staged pair i of a tile and
finds its run through the column the staged word names) at the smallest shapes at which it can go wrong.  Every case: a
small CSR from the host, tfidf's row stream, the table-driven fill - ``ent``, ``sptr`` and ``perm`` byte for byte those of
the fill of csrc/tpack4.hip (tune ``tperm_off`` = 1, which keeps the write-out by column), and the rows of scipy's
transpose: (cell, value) pairs, cells ascending.

A row block has 16 waves of ``rw`` rows, ``rw`` = rows / (16 x compute units) rounded up, at most 32: a matrix of a few
thousand rows has blocks of 16 or 32 rows and tiles of a few dozen pairs; the cases that need whole blocks of 512 rows
(a full staging buffer, a run of 512 pairs, tile totals past 1024) take ``N512`` rows."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests.test_gpu_kernels import _check_stream, _up
from tests.test_gpu_tperm import _compare, _old_and_new, _same_bytes

pytestmark = pytest.mark.gpu

N512 = 160_077  # rows: blocks of 512 on any device up to 312 compute units, and a ragged last block (333 rows)


@pytest.fixture(autouse=True)
def _switches_back(hip):
    yield
    hip.tune("tperm_off", 0)
    hip.tune("tpack4_c", 0)


def _csr(rows, cols, vals, shape):
    m = sp.coo_matrix((np.asarray(vals, dtype=np.float32), (np.asarray(rows), np.asarray(cols))), shape=shape).tocsr()
    m.sort_indices()
    return m


def _tiles_of(hip, X):
    """(first column of every tile incl. the closing boundaries, tiles per block) of X's table."""
    tp = hip._plan_of(X, "tplan")["tperm"]
    return hip.to_host(tp["tiles"]), np.diff(hip.to_host(tp["toff"]))


def test_fewer_pairs_than_one_wave(hip):
    """40 x 24 with 30 entries: every tile total lies in 1 .. 63 (or is 0) - one partial round of the first wave."""
    rng = np.random.default_rng(40)
    at = rng.choice(40 * 24, 30, replace=False)
    m = _csr(at // 24, at % 24, rng.random(30) + 0.5, (40, 24))
    assert m.nnz == 30
    _compare(hip, m)


def test_tile_totals_that_are_no_multiple_of_the_workgroup(hip):
    """Blocks of 512 rows at 2 %: tiles of thousands of pairs - whole rounds of 1024 lanes in batches of four, two and
    one and a partial last round - and a ragged last row block."""
    rng = np.random.default_rng(41)
    m = sp.random(N512, 900, density=0.02, format="csr", random_state=rng, dtype=np.float32)
    m.sort_indices()
    rpb, _G = hip._t4_geometry(N512, 900, m.nnz)
    assert rpb == 512 and N512 % rpb != 0
    X = _compare(hip, m)
    tiles, _per = _tiles_of(hip, X)
    # the first block's first tile: more than one round, and not a whole number of them
    first = int(m[:512, :int(tiles[1])].nnz)
    assert first > 1024 and first % 1024 != 0


def test_block_that_fills_the_staging_buffer_exactly(hip):
    """512 rows x 18 dense columns are mu_tperm_stage_pairs() pairs in ONE tile: the last lane of the last whole round
    reads the buffer's last pair.  (The plan narrows a tile in steps of 16 columns, so a wider dense block - 36 columns,
    below - is cut into tiles of 16, 16 and 4 columns, never 18: the exact fill needs a matrix of 18 columns.)"""
    cap = hip.lib.mu_tperm_stage_pairs()
    rng = np.random.default_rng(42)
    d = 18
    m = sp.csr_matrix((rng.random((N512, d)) + 0.5).astype(np.float32))
    rpb, _G = hip._t4_geometry(N512, d, m.nnz)
    assert rpb * d == cap
    X = _compare(hip, m)
    tiles, per = _tiles_of(hip, X)
    assert np.all(per == 1) and tiles[0] == 0 and tiles[1] == d  # one tile of 18 columns = `cap` pairs per whole block


@pytest.mark.parametrize("n", [512, N512])
def test_dense_block_of_36_columns(hip, n):
    """512 x 36 fully dense (blocks of 16 rows on a whole device), and the same columns over blocks of 512 rows, where
    36 columns do not fit the staging buffer and the schedule halves: tiles of 16 columns = 8192 pairs, eight whole
    rounds."""
    rng = np.random.default_rng(43)
    m = sp.csr_matrix((rng.random((n, 36)) + 0.5).astype(np.float32))
    X = _compare(hip, m)
    if n == N512:
        rpb, _G = hip._t4_geometry(n, 36, m.nnz)
        tiles, per = _tiles_of(hip, X)
        assert rpb == 512 and rpb * 36 > hip.lib.mu_tperm_stage_pairs()
        assert per[0] == 3 and list(tiles[:4]) == [0, 16, 32, 36]


def test_long_run_next_to_short_ones(hip):
    """Per block of 512 rows: 64 columns of ONE pair each, empty columns, one column of 512 pairs, empty columns, 30
    columns of one pair.  Pairs 0 .. 63 of the tile are one wave store over 64 columns, pairs 64 .. 575 eight wave stores
    inside one run; the entries of the empty columns in the run table are never read."""
    d = 200
    rng = np.random.default_rng(44)
    rows, cols = [np.arange(N512)], [np.full(N512, 100)]
    for b in range((N512 + 511) // 512):
        r0, nb = 512 * b, min(512, N512 - 512 * b)
        short = np.concatenate([np.arange(64), np.arange(130, 160)])
        rows.append(r0 + rng.integers(0, nb, short.size))
        cols.append(short)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    m = _csr(rows, cols, rng.random(rows.size) + 0.5, (N512, d))
    rpb, _G = hip._t4_geometry(N512, d, m.nnz)
    assert rpb == 512
    X = _compare(hip, m)
    tiles, per = _tiles_of(hip, X)
    assert per[0] == 1 and tiles[1] == d  # one tile holds them all
    assert np.array_equal(np.diff(m[:512].tocsc().indptr)[[0, 63, 64, 100, 129, 130]], [1, 1, 0, 512, 0, 1])


@pytest.mark.parametrize("n", [3000, N512])
def test_empty_tiles_between_non_empty_ones(hip, n):
    """Tiles forced to 16 columns, every second range of 16 columns empty, then two non-empty ones: both parity sets
    of the staging buffer and of the run table are reused behind a tile of 0 pairs."""
    rng = np.random.default_rng(45)
    m = sp.random(n, 112, density=0.1, format="coo", random_state=rng, dtype=np.float32)
    keep = ~np.isin(m.col // 16, (1, 3, 5))
    m = _csr(m.row[keep], m.col[keep], m.data[keep], (n, 112))
    assert m[:, 16:32].nnz == 0 and m[:, 0:16].nnz > 0 and m[:, 96:112].nnz > 0
    hip.tune("tpack4_c", 16)
    X = _compare(hip, m)
    tiles, per = _tiles_of(hip, X)
    assert per[0] == 7 and list(tiles[:8]) == [0, 16, 32, 48, 64, 80, 96, 112]


@pytest.mark.parametrize("n,d", [(5000, 300), (1000, 77), (33, 2000), (131_072 + 5, 64)])
def test_ragged_row_blocks(hip, n, d):
    """Rows that are no multiple of the row block, and geometries with fewer than 32 rows per wave (1, 2, ... rows on a
    whole device): the cell is rebuilt from wave x rows per wave + the row of the wave."""
    rng = np.random.default_rng(n + d)
    m = sp.random(n, d, density=0.05, format="csr", random_state=rng, dtype=np.float32)
    m.sort_indices()
    rpb, _G = hip._t4_geometry(n, d, m.nnz)
    assert n % rpb != 0
    if n <= 5000:
        assert rpb < 512
    _compare(hip, m)


@pytest.fixture(scope="module")
def last_column_matrix():
    rng = np.random.default_rng(46)
    m = sp.random(3000, 1000, density=0.03, format="lil", random_state=rng, dtype=np.float32)
    m[::3, 999] = 1.5  # the last column: populated in every block
    m[:, 990:999] = 0  # ... behind empty ones
    m = m.tocsr()
    m.eliminate_zeros()
    m.sort_indices()
    return m


@pytest.mark.parametrize("C", [16, 48, 160, 512])
def test_last_column_at_forced_tile_widths(hip, last_column_matrix, C):
    m = last_column_matrix
    assert m[:, m.shape[1] - 1].nnz >= 1000 and m[:, 990:999].nnz == 0
    hip.tune("tpack4_c", C)
    _compare(hip, m)


def test_two_fills_from_one_plan_with_different_values(hip):
    rng = np.random.default_rng(47)
    m = sp.random(N512, 300, density=0.03, format="csr", random_state=rng, dtype=np.float32)
    m.sort_indices()
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
