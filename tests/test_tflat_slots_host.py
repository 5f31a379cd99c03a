"""Where the flat read-in fill keeps its staging slots (csrc/tflat.hip, `k_tflat_plan<true>` writes, `k_tflat_move`
reads), restated in numpy on top of `plan_block`'s tiles and counts (tests/test_tflat_plan_host.py) and checked on the
CPU by filling with it.  tests/test_gpu_tflat_slots.py compares the plan kernel's array with `slots_block`.

A slot's VALUE is the pair's rank among its tile's pairs of the row block in (column, cell) order - the staging buffer
holds a tile as the write-out stores it.  A slot's PLACE follows the read order: a wave's rows are consecutive CSR rows,
so its entries are the CSR range from ``indptr[first row of the wave]`` on (a wave without rows: from the block's end on,
and it never has a pair), and that range holds the wave's slots tile after tile; inside a tile pair i of the wave - its
rows in order, a row's pairs in column order: i = P_r + k, P_r the exclusive prefix of the tile's counts over the wave's
rows - has slot number i.  Lane l of the wave reads pair 64 u + l in round u, so a round is 64 consecutive slots."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests.test_tflat_plan_host import LANES, NW, plan_block


def slots_block(indptr, indices, r0, r1, tiles, counts, rw):
    """The slots of the CSR range [indptr[r0], indptr[r1]) of the row block [r0, r1), ``tiles`` / ``counts`` from
    `plan_block`: ranks per (column, cell) inside a tile, places per (wave, tile, i)."""
    base = int(indptr[r0])
    out = np.full(int(indptr[r1]) - base, -1, dtype=np.int64)
    k = np.arange(r1 - r0)
    wave_of, place = k // rw, (k // rw) * LANES + k % rw
    cur = np.asarray(indptr[r0:r1], dtype=np.int64).copy()
    run = [int(indptr[min(r0 + w * rw, r1)]) - base for w in range(NW)]  # a wave's next free place
    for t in range(len(tiles) - 1):
        n = counts[t][place]
        rows = np.repeat(k, n)  # the tile's pairs, rows in order, a row's pairs in column order: the waves' read order
        q = np.repeat(cur - (np.cumsum(n) - n), n) + np.arange(int(n.sum()))
        cols = np.asarray(indices)[q]
        assert np.all((tiles[t] <= cols) & (cols < tiles[t + 1]))
        rank = np.empty(q.size, dtype=np.int64)
        rank[np.lexsort((rows, cols))] = np.arange(q.size)  # (column, cell) order
        for w in range(NW):
            mine = rank[wave_of[rows] == w]
            out[run[w]:run[w] + mine.size] = mine
            run[w] += mine.size
        cur += n
    assert np.all(out >= 0) and np.array_equal(cur, indptr[r0 + 1:r1 + 1])
    return out


def fill_block(indptr, indices, data, r0, r1, tiles, counts, slots, rw, stage_cap):
    """What the fill does with one row block, from tiles, counts and slots alone: per tile every wave takes its pairs
    i = 0 .. T - 1 (row r = the last with P_r <= i, pair i - P_r behind the row's cursor), puts each into the staging
    buffer at its slot, and the buffer is written out front to back.  Returns the block's (columns, cells, values) in
    the order written; asserts what the write-out relies on: every slot of a tile taken once, (column, cell) order."""
    base = int(indptr[r0])
    cur = np.full(NW * LANES, 0, dtype=np.int64)
    k = np.arange(r1 - r0)
    cur[(k // rw) * LANES + k % rw] = indptr[r0:r1]
    ptr = [int(indptr[min(r0 + w * rw, r1)]) - base for w in range(NW)]
    cols_out, cells_out, vals_out = [], [], []
    for t in range(len(tiles) - 1):
        total = int(counts[t].sum())
        assert total <= stage_cap
        st_col, st_cell = np.full(total, -1, dtype=np.int64), np.full(total, -1, dtype=np.int64)
        st_val = np.zeros(total, dtype=np.asarray(data).dtype)
        for w in range(NW):
            n = counts[t][w * LANES:(w + 1) * LANES]
            pre = np.cumsum(n) - n
            T = int(n.sum())
            i = np.arange(T)
            r = np.searchsorted(pre, i, side="right") - 1
            q = cur[w * LANES + r] + (i - pre[r])
            s = slots[ptr[w] + i]
            assert np.all(st_col[s] == -1) and np.unique(s).size == T
            st_col[s], st_cell[s], st_val[s] = np.asarray(indices)[q], r0 + w * rw + r, np.asarray(data)[q]
            ptr[w] += T
            cur[w * LANES:(w + 1) * LANES] += n
        assert np.all(st_col >= 0)
        assert np.all(np.diff(st_col * (r1 + 1) + st_cell) > 0)  # (column, cell) strictly ascending
        cols_out.append(st_col), cells_out.append(st_cell), vals_out.append(st_val)
    cat = lambda parts, dt: np.concatenate(parts) if parts else np.zeros(0, dtype=dt)  # noqa: E731
    return cat(cols_out, np.int64), cat(cells_out, np.int64), cat(vals_out, np.asarray(data).dtype)


def transpose_by_fill(m, rpb, tile_cols, wave_cap, stage_cap, blocks=None):
    """The transpose of the rows of ``blocks`` (all) of the canonical CSR ``m``, as the numpy fill writes it: blocks in
    order, every column's run of a block behind the runs of the blocks before it."""
    n, d = m.shape
    rw = rpb // NW
    parts = []
    for g in (range((n + rpb - 1) // rpb) if blocks is None else blocks):
        r0, r1 = g * rpb, min((g + 1) * rpb, n)
        tiles, counts = plan_block(m.indptr, m.indices, r0, r1, d, tile_cols, rw, wave_cap, stage_cap)
        slots = slots_block(m.indptr, m.indices, r0, r1, tiles, counts, rw)
        assert slots.size == 0 or slots.max() < stage_cap
        parts.append(fill_block(m.indptr, m.indices, m.data, r0, r1, tiles, counts, slots, rw, stage_cap))
    cols, cells, vals = (np.concatenate([p[j] for p in parts]) for j in range(3))
    order = np.argsort(cols, kind="stable")  # (a column's runs stay in block order, a run in the order written)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=d))])
    return indptr, cells[order], vals[order]


def _same_as_scipy(m, got):
    mt = m.T.tocsr()
    mt.sort_indices()
    indptr, cells, vals = got
    assert np.array_equal(indptr, mt.indptr) and np.array_equal(cells, mt.indices) and np.array_equal(vals, mt.data)


@pytest.mark.parametrize("n,d,dens,rpb,tile_cols,wave_cap,stage_cap", [
    (150, 70, 0.2, 64, 32, 640, 9216), (61, 200, 0.1, 64, 48, 100, 1100), (64, 90, 0.9, 64, 64, 64, 1030),
    (333, 47, 0.3, 32, 16, 64, 1024), (40, 130, 0.02, 16, 512, 768, 9216), (1000, 33, 0.5, 512, 48, 768, 9216)])
def test_numpy_fill_is_the_transpose(n, d, dens, rpb, tile_cols, wave_cap, stage_cap):
    rng = np.random.default_rng(n + d)
    m = sp.random(n, d, density=dens, format="csr", random_state=rng, dtype=np.float32)
    m.sort_indices()
    m.data = (rng.random(m.nnz) + 0.5).astype(np.float32)
    _same_as_scipy(m, transpose_by_fill(m, rpb, tile_cols, wave_cap, stage_cap))


def edge_matrix(n_rows, R, rng):
    """Blocks of 512 rows (16 waves of 32) x 200 columns for tiles of 48 columns and a wave cap of 64 R: one scenario per
    row block.  tests/test_gpu_tflat_slots.py uploads the same matrix with ``n_rows`` = 160 077 (a ragged last block)."""
    d = 200
    rows, cols = [], []

    def put(block, wave, lanes, cs):
        rr, cc = np.meshgrid(512 * block + 32 * wave + np.atleast_1d(lanes), np.atleast_1d(cs), indexing="ij")
        rows.append(rr.ravel()), cols.append(cc.ravel())

    # block 0: wave 2 has pairs in tiles 0 and 2 .. 4 and NONE in tile 1 (columns 48 .. 95); waves 0 and 1 before it
    # hold 3 + 70 pairs, so its CSR base (73) is odd and every round of it lies across a 128-byte line of slots
    put(0, 0, 31, [0, 50, 199])
    put(0, 1, np.arange(10), np.arange(1, 8))
    put(0, 2, np.arange(32), np.concatenate([np.arange(0, 12), np.arange(100, 130)]))
    put(0, 9, [4, 5], np.arange(0, 200, 7))
    # block 1: wave totals of 63, 64, 65, 64 R and 64 R in tile 0, then a wave with none in it
    put(1, 0, np.arange(21), [0, 9, 30])
    put(1, 1, np.arange(32), [5, 6])
    put(1, 2, 0, np.arange(40))
    put(1, 2, 1, np.arange(20, 45))  # (pairs 40 .. 64 of the wave: the row crosses from round 0 into round 1)
    put(1, 3, np.arange(32), np.arange(2 * R))
    put(1, 4, np.arange(31), np.arange(2 * R))
    put(1, 4, 31, np.arange(48 - 2 * R, 48))  # (64 R again, the last row's pairs at the tile's end)
    put(1, 4, 31, np.arange(48, 200, 3))
    put(1, 6, np.arange(32), np.arange(100, 120))
    # block 2: empty rows first, last and in runs inside a wave; waves of one row
    put(2, 7, [5, 6], np.arange(10, 40))
    put(2, 7, 21, np.arange(0, 48))
    put(2, 7, 30, np.arange(3, 200, 2))
    put(2, 8, 31, np.arange(200))
    put(2, 9, 0, np.arange(200))
    put(2, 10, [0, 31], [47, 48, 199])
    # block 3: empty.  The blocks behind: a thin background; the last block is ragged when n_rows is no multiple of 512
    k = int(0.01 * (n_rows - 4 * 512) * d)
    rows.append(rng.integers(4 * 512, n_rows, k)), cols.append(rng.integers(0, d, k))
    m = sp.coo_matrix((np.ones(sum(r.size for r in rows), dtype=np.float32), (np.concatenate(rows), np.concatenate(cols))),
                      shape=(n_rows, d)).tocsr()  # (duplicates add up)
    m.sort_indices()
    m.data = (rng.random(m.nnz) + 0.5).astype(np.float32)
    return m


def check_edge_matrix(m, R):
    """the scenarios are what `edge_matrix` says they are"""
    wave = lambda b, w, c0, c1: int(m[512 * b + 32 * w:512 * b + 32 * w + 32, c0:c1].nnz)  # noqa: E731
    assert [wave(0, 2, c, c + 48) > 0 for c in (0, 48, 96)] == [True, False, True]
    base = int(m.indptr[2 * 32])
    assert base % 2 == 1 and base % 64 != 0 and wave(0, 2, 0, 48) >= 2 * 64  # (slots are 2 bytes: 64 to a line)
    assert [wave(1, w, 0, 48) for w in range(6)] == [63, 64, 65, 64 * R, 64 * R, 0]
    lens = np.diff(m.indptr)[2 * 512 + 7 * 32:2 * 512 + 8 * 32]
    assert lens[0] == 0 and lens[31] == 0 and np.all(lens[7:21] == 0) and lens[21] > 0
    assert m[3 * 512:4 * 512].nnz == 0


def test_numpy_fill_of_the_edge_matrix():
    R = 12
    n_rows = 6 * 512 + 333  # (the same scenario blocks, fewer background blocks; the last has 333 rows: 10 waves and 13 rows)
    m = edge_matrix(n_rows, R, np.random.default_rng(70))
    check_edge_matrix(m, R)
    tiles, counts = plan_block(m.indptr, m.indices, 512, 1024, 200, 48, 32, 64 * R, 9216)
    assert tiles[:2] == [0, 48]  # (64 R is admitted whole)
    _same_as_scipy(m, transpose_by_fill(m, 512, 48, 64 * R, 9216))
    # a ragged last block: the waves behind its rows share one base, the block's end, and never have a pair
    last = m[6 * 512:]
    assert last.nnz > 0
    indptr, cells, vals = transpose_by_fill(m, 512, 48, 64 * R, 9216, blocks=[6])
    _same_as_scipy(last, (indptr, cells - 6 * 512, vals))
