"""The flat read-in of the table-driven fill (csrc/tflat.hip, tune ``tperm_flat`` = 1: the plan records every row's pairs
per tile, lane i of a wave reads the wave's pair i) at the smallest shapes at which it can go wrong.  Every case fills
X^T's row stream three times - ``tperm_off`` = 1 (`k_t4_fill`), ``tperm_flat`` = 0 (`k_tperm_move`), ``tperm_flat`` = 1
(`k_tflat_move`) - and compares ``ent``, ``sptr`` and ``perm`` with ``==``; the new kernel then writes once more into a
buffer of sentinels, which must come back untouched on both sides of the stream.  The plan kernel's tiles and counts are
compared with the numpy restatement of tests/test_tflat_plan_host.py.

A row block has 16 waves of ``rw`` rows, ``rw`` = rows / (16 x compute units) rounded up, at most 32: the cases that
place pairs in a given wave take ``N512`` rows (blocks of 512, wave w of block b = rows 512 b + 32 w ...)."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from muon_amd._backend import _p, check
from tests.test_gpu_kernels import _check_stream, _up
from tests.test_gpu_tperm import _same_bytes, _x_stream
from tests.test_tflat_plan_host import LANES, NW, plan_block

pytestmark = pytest.mark.gpu

N512 = 160_077  # rows: blocks of 512 on any device up to 312 compute units, and a ragged last block (333 rows)
PAD = 4096
SENTINEL = 0x7FC000007FFFFFFF  # (a NaN's bits in the value half)


@pytest.fixture(autouse=True)
def _switches_back(hip):
    yield
    for key, default in (("tperm_off", 0), ("tperm_flat", 1), ("tpack4_c", 0)):
        hip.tune(key, default)


def _csr(rows, cols, shape, rng):
    rows, cols = np.concatenate([np.ravel(r) for r in rows]), np.concatenate([np.ravel(c) for c in cols])
    m = sp.coo_matrix((np.ones(rows.size, dtype=np.float32), (rows, cols)), shape=shape).tocsr()  # (duplicates add up)
    m.sort_indices()
    m.data = (rng.random(m.nnz) + 0.5).astype(np.float32)
    return m


def _fill(hip, X, src, off, flat):
    hip.tune("tperm_off", off)
    hip.tune("tperm_flat", flat)
    return hip.transpose_stream(X, src=src)


def _guarded_flat_fill(hip, X, src, ref):
    """`k_tflat_move` into the middle of a buffer of sentinels: the stream's bytes, nothing before or behind them"""
    plan = hip._plan_of(X, "tplan")
    tp = plan["tperm"]
    n, d = X.shape
    xs, row_dst = src
    buf = torch.full((X.nnz + 2 * PAD,), SENTINEL, dtype=torch.int64, device=ref.ent.device)
    cnt = plan["work"][int(hip.lib.mu_tpack4_cnt_offset(n, d, X.nnz)):]
    with hip._dev_ctx():
        check(hip.lib.mu_tflat_fill(n, d, X.nnz, _p(X.indptr), _p(row_dst), _p(xs.ent), _p(tp["cdst"]), _p(cnt),
                                    _p(tp["toff"]), _p(tp["tiles"]), _p(tp["counts"]), _p(tp["slots"]),
                                    buf.data_ptr() + 8 * PAD, hip._stream()))
    torch.cuda.synchronize()
    assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + X.nnz:] == SENTINEL).all())
    assert torch.equal(buf[PAD:PAD + X.nnz], ref.ent[:X.nnz])


def _compare(hip, m, scipy_too=True):
    """the three fills of `m`; returns (device CSR, its row stream, the flat fill's table)"""
    X = _up(hip, m)
    assert m.nnz > 0 and hip._use_tpack4(X) and hip._plan_of(X, "tplan") is not None
    src = _x_stream(hip, X)
    ref = _fill(hip, X, src, 1, 0)
    win = _fill(hip, X, src, 0, 0)
    assert "cont" in hip._plan_of(X, "tplan")["tperm"]  # (the windowed fill's table ...)
    flat = _fill(hip, X, src, 0, 1)
    tp = hip._plan_of(X, "tplan").get("tperm")  # (... made again for the flat one: the tune key is one of its keys)
    assert isinstance(tp, dict) and "counts" in tp and "cont" not in tp
    assert 0 <= int(tp["slots"].min()) and int(tp["slots"].max()) < hip.lib.mu_tperm_stage_pairs()
    _same_bytes(hip, ref, win, m.nnz)
    _same_bytes(hip, ref, flat, m.nnz)
    _guarded_flat_fill(hip, X, src, ref)
    if scipy_too:
        mt = m.T.tocsr()
        mt.sort_indices()
        _check_stream(hip, flat, mt)
    return X, src, tp


def _plan_of_blocks(hip, m, tp, blocks):
    """the plan kernel's tiles and counts of the given row blocks == the numpy restatement's"""
    n, d = m.shape
    rpb, _G = hip._t4_geometry(n, d, m.nnz)
    toff, tiles = hip.to_host(tp["toff"]), hip.to_host(tp["tiles"])
    counts = hip.to_host(tp["counts"]).view(np.uint16).reshape(-1, NW * LANES)
    cap, wcap = hip.lib.mu_tperm_stage_pairs(), 64 * hip.lib.mu_tflat_rounds()
    out = {}
    for g in blocks:
        want_t, want_c = plan_block(m.indptr, m.indices, g * rpb, min((g + 1) * rpb, n), d, tp["tile_cols"], rpb // NW,
                                    wcap, cap)
        got_t = tiles[toff[g] + g:toff[g + 1] + g + 1].tolist()
        assert got_t == want_t, (g, got_t, want_t)
        assert np.array_equal(counts[toff[g]:toff[g + 1]], want_c), g
        out[g] = (got_t, want_c)
    return out


def _edge_matrix(R, rng, extra):
    """Blocks of 512 rows x 200 columns, tiles forced to 48 columns; one scenario per row block (see the test)."""
    d = 200
    rows, cols = [], []

    def put(block, wave, lanes, cs):
        lanes, cs = np.atleast_1d(lanes), np.atleast_1d(cs)
        rr, cc = np.meshgrid(512 * block + 32 * wave + lanes, cs, indexing="ij")
        rows.append(rr)
        cols.append(cc)

    # block 0: wave 3 has 64 R pairs in tile 0 (32 rows x 2 R columns) (+ `extra` more in another of its columns)
    put(0, 3, np.arange(32), np.arange(2 * R))
    if extra:
        put(0, 3, 0, 2 * R + 5)
    put(0, 9, [4, 5], np.arange(0, 200, 7))
    # block 1: wave totals of 1, 63, 64, 65 and 0 in tile 0, next to a full wave; rows that cross a round boundary
    put(1, 0, 17, 3)
    put(1, 1, np.arange(21), [0, 9, 30])
    put(1, 2, np.arange(32), [5, 6])
    put(1, 3, 0, np.arange(40))
    put(1, 3, 1, np.arange(20, 45))  # pairs 40 .. 64 of the wave: the row crosses from round 0 into round 1
    put(1, 5, np.arange(32), np.arange(2 * R - 1))
    put(1, 5, 31, np.arange(2 * R - 1, 2 * R + 20))  # a row that ends the wave, across the last rounds
    put(1, 6, np.arange(32), np.arange(100, 120))    # (wave 4 has no pair at all; wave 6 none in tile 0)
    # block 2: an empty tile (columns 48 .. 95) between full ones
    for w in range(NW):
        put(2, w, np.arange(0, 32, 3), np.concatenate([np.arange(0, 48, 2), np.arange(96, 200, 3)]))
    # block 3: a whole empty row block
    # block 4: empty rows first, last and in runs - several rows share a prefix value in the search
    put(4, 7, [5, 6], np.arange(10, 40))
    put(4, 7, 21, np.arange(0, 48))
    put(4, 7, 31, np.arange(3, 200, 2))
    put(4, 8, 31, np.arange(200))  # only the wave's last row
    put(4, 9, 0, np.arange(200))   # only its first
    put(4, 10, [0, 31], [47, 48, 199])
    # the blocks behind: a thin random background (the last block is ragged)
    k = int(0.01 * (N512 - 5 * 512) * d)
    rows.append(rng.integers(5 * 512, N512, k))
    cols.append(rng.integers(0, d, k))
    return _csr(rows, cols, (N512, d), rng)


@pytest.mark.parametrize("extra", [0, 1])
def test_wave_totals_at_the_cap_and_at_the_round_edges(hip, extra):
    """`extra` = 0: a wave's total of exactly 64 R - one tile of 48 columns; 1: of 64 R + 1 - the plan narrows that tile.
    The same matrix carries the wave totals 1 / 63 / 64 / 65 / 0, a row across a round boundary, an empty tile, an empty
    row block and the empty rows."""
    R = hip.lib.mu_tflat_rounds()
    assert 8 <= R <= 24
    rng = np.random.default_rng(60 + extra)
    m = _edge_matrix(R, rng, extra)
    rpb, G = hip._t4_geometry(N512, 200, m.nnz)
    assert rpb == 512 and N512 % rpb != 0
    wave = lambda b, w, c0, c1: int(m[512 * b + 32 * w:512 * b + 32 * w + 32, c0:c1].nnz)  # noqa: E731
    assert wave(0, 3, 0, 48) == 64 * R + extra
    assert [wave(1, w, 0, 48) for w in range(5)] == [1, 63, 64, 65, 0] and wave(1, 5, 0, 48) > 600
    assert m[2 * 512:3 * 512, 48:96].nnz == 0 and m[3 * 512:4 * 512].nnz == 0
    hip.tune("tpack4_c", 48)
    X, _src, tp = _compare(hip, m)
    assert tp["tile_cols"] == 48
    got = _plan_of_blocks(hip, m, tp, [0, 1, 2, 3, 4, 5, G - 1])
    # the schedule did what the rule says: block 0's first tile is whole at the cap and narrowed one pair past it
    assert got[0][0][:2] == ([0, 48] if not extra else [0, 16])
    assert got[1][0] == [0, 48, 96, 144, 192, 200] and got[3][0] == [0, 48, 96, 144, 192, 200]


def test_row_with_a_pair_in_every_column_of_a_512_column_tile(hip):
    """One row of 600 pairs (count 512 in the first tile, the 16-bit count's and the search's largest value), alone in
    its wave and next to a busy wave."""
    rng = np.random.default_rng(62)
    d = 600
    rows = [np.full(d, 512 + 32 * 2 + 7), np.repeat(512 + 32 * 3 + np.arange(32), 8)]
    cols = [np.arange(d), np.tile(np.arange(0, 512, 64), 32)]
    k = 40_000
    rows.append(rng.integers(0, N512, k))
    cols.append(rng.integers(0, d, k))
    m = _csr(rows, cols, (N512, d), rng)
    hip.tune("tpack4_c", 512)
    X, _src, tp = _compare(hip, m)
    got = _plan_of_blocks(hip, m, tp, [0, 1, 2])
    assert got[1][0] == [0, 512, 600] and got[1][1][0].reshape(NW, LANES)[2, 7] == 512


@pytest.mark.parametrize("n,d", [(33, 2000), (1000, 77), (5000, 300), (40_001, 90), (100_003, 64), (131_072 + 5, 64)])
def test_ragged_row_blocks(hip, n, d):
    """Rows that are no multiple of the row block, at geometries from one row per wave to 32."""
    rng = np.random.default_rng(n + d)
    m = sp.random(n, d, density=0.05, format="csr", random_state=rng, dtype=np.float32)
    m.sort_indices()
    rpb, G = hip._t4_geometry(n, d, m.nnz)
    assert n % rpb != 0 and 1 <= rpb // NW <= 32
    _X, _src, tp = _compare(hip, m)
    _plan_of_blocks(hip, m, tp, [0, G - 1])


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
    _X, _src, tp = _compare(hip, m)
    assert tp["tile_cols"] == C
    _plan_of_blocks(hip, m, tp, [0])


def test_block_denser_than_the_staging_buffer(hip):
    """36 dense columns over blocks of 512 rows: 18 432 pairs do not fit a staging buffer and 1152 not a wave - tiles of
    16, 16 and 4 columns - and 18 columns exactly fill the buffer (576 pairs per wave)."""
    rng = np.random.default_rng(63)
    m = sp.csr_matrix((rng.random((N512, 36)) + 0.5).astype(np.float32))
    rpb, G = hip._t4_geometry(N512, 36, m.nnz)
    assert rpb == 512 and rpb * 36 > hip.lib.mu_tperm_stage_pairs()
    _X, _src, tp = _compare(hip, m, scipy_too=False)
    got = _plan_of_blocks(hip, m, tp, [0, G - 1])
    assert got[0][0] == [0, 16, 32, 36]
    m18 = sp.csr_matrix(m[:, :18])
    _X, _src, tp = _compare(hip, m18, scipy_too=False)
    assert _plan_of_blocks(hip, m18, tp, [0])[0][0] == [0, 18]


def test_two_fills_from_one_plan_with_other_values(hip):
    rng = np.random.default_rng(64)
    m = sp.random(N512, 300, density=0.03, format="csr", random_state=rng, dtype=np.float32)
    m.sort_indices()
    X, src, tp = _compare(hip, m)
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


def test_foreign_layout_takes_the_old_fill(hip):
    rng = np.random.default_rng(65)
    m = sp.random(5000, 700, density=0.03, format="csr", random_state=rng, dtype=np.float32)
    m.sort_indices()
    X = _up(hip, m)
    xs, row_dst = _x_stream(hip, X)
    ref = _fill(hip, X, (xs, row_dst), 1, 0)
    got = _fill(hip, X, (xs, row_dst.clone()), 0, 1)  # (not the plan's layout object: nothing is assumed about it)
    csr = _fill(hip, X, None, 0, 1)                   # (CSR source)
    plan = hip._plan_of(X, "tplan")
    assert plan.get("tperm") is None
    _same_bytes(hip, ref, got, m.nnz)
    _same_bytes(hip, ref, csr, m.nnz)


def test_plan_that_cannot_be_allocated_takes_the_old_fill(hip, monkeypatch):
    """No memory for the flat fill's table: the call succeeds through `k_tperm_move`, and stays there."""
    rng = np.random.default_rng(66)
    m = sp.random(20000, 3000, density=0.03, format="csr", random_state=rng, dtype=np.float32)
    m.sort_indices()
    X = _up(hip, m)
    src = _x_stream(hip, X)
    ref = _fill(hip, X, src, 1, 0)
    real, refused = hip.empty, []

    def no_room_once(shape, dtype, *a, **k):
        if dtype == torch.int16 and not refused:
            refused.append(shape)
            raise torch.OutOfMemoryError("no room for the slot table")
        return real(shape, dtype, *a, **k)

    monkeypatch.setattr(hip, "empty", no_room_once)
    got = _fill(hip, X, src, 0, 1)
    monkeypatch.undo()
    plan = hip._plan_of(X, "tplan")
    table = plan["tperm"]
    assert len(refused) == 1 and isinstance(table, dict) and "cont" in table and "counts" not in table
    again = _fill(hip, X, src, 0, 1)
    assert plan["tperm"] is table  # (not tried again)
    _same_bytes(hip, ref, got, m.nnz)
    _same_bytes(hip, ref, again, m.nnz)
