"""The tile rule and the per-(tile, row) counts of the flat read-in fill (csrc/tflat.hip, `k_tflat_plan`), restated in
numpy and checked against brute force on the CPU.  tests/test_gpu_tflat.py compares the plan kernel with `plan_matrix`.

A row block is 16 waves x ``rw`` <= 32 rows.  From the tile's first column ``cb`` the tile ends at
``min(cb + tile_cols, n_cols)`` if (a) every wave's pairs in it are <= ``wave_cap`` (64 x the kernel's rounds) and (b)
the block's pairs in it are <= ``stage_cap`` (one staging buffer); otherwise the width is halved, rounded down to a
multiple of 16 and never below 16, and asked again.  16 columns x 32 rows = 512 pairs per wave and 8192 per block always
pass.  ``counts[tile, 32 * wave + lane]`` = pairs of row ``wave * rw + lane`` of the block in the tile (0 for a lane that
has no row)."""
import numpy as np
import pytest

NW, LANES = 16, 32


def _cum(indptr, indices, r0, r1, n_cols):
    """cum[k, c] = entries of row r0 + k in columns < c"""
    dense = np.zeros((r1 - r0, n_cols), dtype=bool)
    for k in range(r1 - r0):
        dense[k, indices[indptr[r0 + k]:indptr[r0 + k + 1]]] = True
    cum = np.zeros((r1 - r0, n_cols + 1), dtype=np.int64)
    np.cumsum(dense, axis=1, out=cum[:, 1:])
    return cum


def halve(width):
    return max(16, width // 2 // 16 * 16)


def plan_block(indptr, indices, r0, r1, n_cols, tile_cols, rw, wave_cap, stage_cap, reasons=False):
    """(tile boundaries closed by n_cols, counts[tiles, 512]) of the row block [r0, r1); with ``reasons`` also what
    narrowed each tile: "" / "wave" / "stage" (the check that failed last before the tile was accepted)."""
    cum = _cum(indptr, indices, r0, r1, n_cols)
    k = np.arange(r1 - r0)
    place = (k // rw) * LANES + k % rw
    tiles, counts, why = [0], [], []
    cb = 0
    while cb < n_cols:
        cend, reason = min(cb + tile_cols, n_cols), ""
        while True:
            row = np.zeros(NW * LANES, dtype=np.int64)
            row[place] = cum[:, cend] - cum[:, cb]
            waves = row.reshape(NW, LANES).sum(1)
            if waves.sum() <= stage_cap and waves.max() <= wave_cap:
                break
            reason = "stage" if waves.sum() > stage_cap else "wave"
            assert cend - cb > 16, "a tile of 16 columns is always admissible"
            cend = cb + halve(cend - cb)
        tiles.append(cend)
        counts.append(row)
        why.append(reason)
        cb = cend
    counts = np.array(counts, dtype=np.int64).reshape(len(tiles) - 1, NW * LANES)
    return (tiles, counts, why) if reasons else (tiles, counts)


def plan_matrix(m, rpb, tile_cols, wave_cap, stage_cap):
    """(toff[G + 1], tiles[T + G], counts[T, 512]) of a scipy CSR, in the layout of mu_tflat_plan's arrays"""
    n, d = m.shape
    rw = rpb // NW
    toff, tiles, counts = [0], [], []
    for r0 in range(0, n, rpb):
        t, c = plan_block(m.indptr, m.indices, r0, min(r0 + rpb, n), d, tile_cols, rw, wave_cap, stage_cap)
        toff.append(toff[-1] + len(t) - 1)
        tiles += t
        counts.append(c)
    return np.array(toff), np.array(tiles), np.concatenate(counts)


# ---- brute force ----------------------------------------------------------------------------------------------------
def _brute(dense, rw, tile_cols, wave_cap, stage_cap):
    """The rule read off the dense block, entry by entry: no prefix sums, no shared helper but `halve`."""
    nr, d = dense.shape
    tiles, counts = [0], []
    cb = 0
    while cb < d:
        width = min(tile_cols, d - cb)
        while True:
            per_wave = [0] * NW
            per_row = [0] * (NW * LANES)
            for r in range(nr):
                for c in range(cb, cb + width):
                    if dense[r, c]:
                        per_wave[r // rw] += 1
                        per_row[(r // rw) * LANES + r % rw] += 1
            if sum(per_wave) <= stage_cap and max(per_wave) <= wave_cap:
                break
            width = halve(width)
        tiles.append(cb + width)
        counts.append(per_row)
        cb += width
    return tiles, np.array(counts, dtype=np.int64).reshape(len(tiles) - 1, NW * LANES)


def _csr_of(dense):
    indptr = np.concatenate([[0], np.cumsum(dense.sum(1))]).astype(np.int64)
    return indptr, np.nonzero(dense)[1].astype(np.int32)


def _patterns():
    rng = np.random.default_rng(7)
    out = []
    for nr, d, dens, rw in [(64, 90, 0.3, 4), (61, 200, 0.1, 4), (32, 47, 0.9, 2), (16, 16, 1.0, 1), (50, 130, 0.02, 4)]:
        out.append((f"random {nr}x{d} at {dens}", rng.random((nr, d)) < dens, rw))
    a = np.zeros((64, 160), dtype=bool)  # one wave (rows 8 .. 11) dense, the others empty: only the wave cap narrows
    a[8:12, :] = True
    out.append(("one dense wave", a, 4))
    b = np.ones((64, 160), dtype=bool)  # everything dense: the staging cap narrows first
    out.append(("dense block", b, 4))
    c = np.zeros((64, 200), dtype=bool)  # empty rows first, last and in runs; an empty tile in the middle
    c[5, :40] = c[6, 150:] = c[40, ::3] = True
    c[:, 64:128] = False
    out.append(("empty rows and an empty tile", c, 4))
    e = np.zeros((30, 100), dtype=bool)  # a ragged block (30 rows of 64), the last column alone
    e[29, 99] = e[0, 0] = True
    out.append(("ragged block, last column", e, 4))
    return out


@pytest.mark.parametrize("name,dense,rw", _patterns(), ids=[p[0] for p in _patterns()])
@pytest.mark.parametrize("tile_cols,wave_cap,stage_cap", [(512, 640, 9216), (48, 100, 1100), (16, 64, 1024), (160, 130, 1500),
                                                           (64, 64, 1030)])
def test_restatement_is_the_rule(name, dense, rw, tile_cols, wave_cap, stage_cap):
    # (the caps admit a 16-column tile of these blocks, as the kernel's do of its own: <= 64 rows, <= 4 per wave)
    assert 16 * rw <= wave_cap and 16 * dense.shape[0] <= stage_cap
    indptr, indices = _csr_of(dense)
    tiles, counts = plan_block(indptr, indices, 0, dense.shape[0], dense.shape[1], tile_cols, rw, wave_cap, stage_cap)
    btiles, bcounts = _brute(dense, rw, tile_cols, wave_cap, stage_cap)
    assert tiles == btiles
    assert np.array_equal(counts, bcounts)
    # every pair is counted once, in the tile its column lies in
    assert counts.sum() == dense.sum()
    for t in range(len(tiles) - 1):
        assert counts[t].sum() == dense[:, tiles[t]:tiles[t + 1]].sum()
        assert counts[t].sum() <= stage_cap and counts[t].reshape(NW, LANES).sum(1).max() <= wave_cap


def test_wave_cap_met_exactly_and_passed_by_one():
    """A wave of 4 rows with 96 pairs in 48 columns: admitted whole at a cap of 96, narrowed to 16 columns at 95."""
    dense = np.zeros((64, 48), dtype=bool)
    dense[4:6, :] = True
    indptr, indices = _csr_of(dense)
    assert plan_block(indptr, indices, 0, 64, 48, 48, 4, 96, 9216)[0] == [0, 48]
    tiles, counts, why = plan_block(indptr, indices, 0, 64, 48, 48, 4, 95, 9216, reasons=True)
    assert tiles == [0, 16, 48] and why == ["wave", ""]  # (48 -> 16; the rest, 32 columns = 64 pairs, is one tile)
    assert counts[0].reshape(NW, LANES)[1, :3].tolist() == [16, 16, 0]
    assert counts[1].reshape(NW, LANES)[1, :3].tolist() == [32, 32, 0]


def test_plan_matrix_lays_blocks_out_one_after_the_other():
    import scipy.sparse as sp

    m = sp.random(150, 70, density=0.2, format="csr", random_state=np.random.default_rng(1), dtype=np.float32)
    m.sort_indices()
    toff, tiles, counts = plan_matrix(m, 64, 32, 640, 9216)
    assert toff.tolist() == [0, 3, 6, 9] and tiles.tolist() == [0, 32, 64, 70] * 3
    assert counts.shape == (9, 512) and counts.sum() == m.nnz
    assert counts[6:].reshape(3, NW, LANES)[:, 6:, :].sum() == 0  # (the last block has 22 rows: waves 0 .. 5)
