"""tests/dense_refs.py proved without a GPU: every case of its tables (row counts for ``cus = 4``) runs through the CPU
operator set of tests/cpu_backend.py with the checking functions tests/test_gpu_dense_edges.py uses, every exact case's
magnitude bound is asserted, the exact Cholesky family's representability argument is asserted, and deliberately wrong
implementations are fed to the same checkers and must be rejected at a named case."""
import numpy as np
import pytest
import torch

from tests import dense_refs as R
from tests.cpu_backend import CpuTestBackend

CUS = 4
BE = CpuTestBackend()


def _all_rows(table):
    return [R.rows(n, CUS) for n in table]


# ---- the tables through the CPU operator set ---------------------------------------------------------------------------
def test_row_tables_sit_at_the_edges():
    assert R.rows("R", CUS) == 16 * 2 * CUS and R.rows("R2", CUS) == 64 * 8 * CUS
    assert _all_rows(R.GRAM_ROWS)[-5:] == [127, 128, 129, 133, 259]
    assert _all_rows(R.APPLY_EDGE_ROWS) == [2047, 2048, 2049, 2065]
    # the work-size rule read backwards (mu_gram_worksize at 10^7 rows, B = 16, on a part with 256 CUs)
    assert R.cus_from_gram_worksize((2 * 256 + 32) * 272 * 8 + 256) == 256
    # 512 rows -> 32 workgroups (direct reduce), 513 -> 33 (fold); 256 rows per row split of skinny_tn, 64 at the most
    assert -(-512 // 16) == 32 and -(-513 // 16) == 33
    assert [R.tn_splits(n, 16, 256) for n in (255, 256, 257, 16384, 16385)] == [1, 1, 2, 64, 64]


@pytest.mark.parametrize("B", R.GRAM_B)
def test_gram_tables(B):
    for n in _all_rows(R.GRAM_ROWS) + [R.rows(R.GRAM_ONE_WG_ROWS, CUS)]:
        assert R.exact_bound(n, 0, np.float64) == 64 * n
        assert R.check_gram(BE, B, n, True) == 0.0 and R.check_gram_cross(BE, B, n, True) == 0.0
    for n in _all_rows(R.GRAM_ROUNDED_ROWS):
        assert R.check_gram(BE, B, n, False) <= 1.0 and R.check_gram_cross(BE, B, n, False) <= 1.0


@pytest.mark.parametrize("B", R.APPLY_B)
def test_apply_and_project_tables(B):
    ns = _all_rows(R.APPLY_ROWS) + (_all_rows(R.APPLY_EDGE_ROWS) if B in R.APPLY_EDGE_B else [])
    assert R.exact_bound(B, 8, np.float32) == 64 * B + 8
    for n in ns:
        for dest, with_bias in R.APPLY_WAYS:
            assert R.check_apply(BE, B, n, True, dest, with_bias) == 0.0
            assert R.check_apply(BE, B, n, False, dest, with_bias) <= 1.0
        assert R.check_project_out(BE, B, n, True) == 0.0
        assert R.check_project_out(BE, B, n, False) <= 1.0


def test_chol_tables():
    for B, w in R.CHOL_RANDOM:
        assert R.check_chol_random(BE, B, w) <= 1.0
    for B, w in R.CHOL_EXACT:
        assert R.check_chol_exact(BE, B, w) == 0.0
    assert R.check_chol_flags(BE) <= 1.0


@pytest.mark.parametrize("B", sorted({B for B, _w in R.CHOL_EXACT}))
def test_exact_cholesky_family_is_representable(B):
    """G = L L^T holds exactly in f64, the stated inverse is the inverse, and every entry of it is exact in f32: in
    integer arithmetic on 4 L, 4 L^-1 and 16 G (the entries are multiples of 1/4, 1/4 and 1/16)."""
    L, Linv, G = R.chol_exact_inputs(B)
    L4, Li4, G16 = (4 * L).astype(np.int64), (4 * Linv).astype(np.int64), (16 * G).astype(np.int64)
    assert np.array_equal(L4, 4 * L) and np.array_equal(Li4, 4 * Linv) and np.array_equal(G16, 16 * G)
    assert np.array_equal(L4 @ L4.T, G16)
    assert np.array_equal(Li4 @ L4, 16 * np.eye(B, dtype=np.int64))
    assert np.array_equal(Linv.astype(np.float32).astype(np.float64), Linv)
    assert set(np.unique(np.abs(Linv))) <= {0.0, 0.25, 0.5, 1.0, 2.0, 4.0}
    sub = np.diag(L, -1) != 0    # sub[i]: row i + 1 depends on row i
    for edge in (16, 32, 48):     # runs of dependent rows across the panel edges that B has
        if edge < B:
            assert sub[edge - 3:edge + 2].all()
            assert Linv[edge + 1, edge - 3] != 0   # ... so the inverse couples the two panels
    assert not sub.all()


@pytest.mark.parametrize("ty", R.SKINNY_TYPES)
def test_skinny_tables(ty):
    CW = R.tile_cols(ty)
    TY, T = R.SKINNY_TYPES[ty]
    nn = [c for t in R.NN_FAST_TILES for c in R.nn_grid_cases(ty, t * CW)]
    nn += [c for D in R.nn_general_cols(ty) for c in R.nn_grid_cases(ty, D)]
    nn += R.nn_big_cases(ty, CUS) + R.nn_ld_cases(ty)
    builds = {(c.build, c.ld > c.D) for c in nn}
    assert builds == {("fast", False), ("fast", True), ("general", False), ("general", True)}
    for c in nn:
        assert R.exact_bound(c.D, 0, T) == 64 * c.D
        assert R.check_skinny_nn(BE, c, True) == 0.0 and R.check_skinny_nn(BE, c, False) <= 1.0
    tn = [c for D in R.TN_COLS for c in R.tn_grid_cases(ty, D)] + R.tn_cap_cases(ty) + R.tn_ld_cases(ty)
    for c in tn:
        assert R.exact_bound(c.n, 0, T) == 64 * c.n
        assert R.check_skinny_tn(BE, c, True) == 0.0 and R.check_skinny_tn(BE, c, False) <= 1.0
    if T == np.float32:   # the largest exact case: skinny_tn in f32 at 16 385 rows
        assert max(64 * c.n for c in tn) == 1048640 < 2 ** 24


def test_guards_see_a_write_outside_the_view():
    view, buf = R.guarded_empty(BE, (5, 16), torch.float32)
    assert R.untouched(buf) and bool(torch.isnan(view).all())
    buf[R.PAD + 5 * 16] = 1.0
    assert not R.untouched(buf)

    class Overrun(CpuTestBackend):
        def gram_cross(self, A, Bm):
            out = self.empty((A.shape[1], A.shape[1]), torch.float64)
            out.copy_(A.double().T @ Bm.double())
            torch.as_strided(out, (1,), (1,), out.storage_offset() + out.numel())[0] = 0.0   # one element past the end
            return out

    with pytest.raises(AssertionError, match="outside its view"):
        R.check_gram_cross(Overrun(), 16, 5, True)


# ---- negative controls: wrong implementations the checkers must reject ---------------------------------------------------
class CrossTransposed(CpuTestBackend):
    def gram_cross(self, A, Bm):
        return Bm.double().T @ A.double()


class LastRowDropped(CpuTestBackend):
    """the ragged last group of four rows loses its last row"""

    def gram(self, A):
        return super().gram(A[:-1] if A.shape[0] % 4 else A)

    def gram_cross(self, A, Bm):
        k = A.shape[0] - 1 if A.shape[0] % 4 else A.shape[0]
        return super().gram_cross(A[:k], Bm[:k])


class LastPartialDropped(CpuTestBackend):
    """the fold (more than 32 workgroups of 16 rows) loses the last workgroup's partial"""

    def gram(self, A):
        wgs = -(-A.shape[0] // 16)
        return super().gram(A[:16 * (wgs - 1)] if wgs > 32 else A)


class LastColumnTileDropped(CpuTestBackend):
    def skinny_nn(self, Y, T16):
        CW = 128 // Y.element_size()
        keep = CW * (-(-Y.shape[1] // CW) - 1) if Y.shape[1] > CW else Y.shape[1]
        return super().skinny_nn(Y[:, :keep], T16[:keep])


class LastSplitDropped(CpuTestBackend):
    def skinny_tn(self, Y, Z16):
        n, D = Y.shape
        S = R.tn_splits(n, D, CUS)
        groups = -(-n // 4)
        keep = n if S == 1 else 4 * (groups * (S - 1) // S)
        return super().skinny_tn(Y[:keep], Z16[:keep])


class HighColumnsZeroed(CpuTestBackend):
    def skinny_nn(self, Y, T16):
        out = super().skinny_nn(Y, T16)
        out[:, 10:] = 0
        return out

    def skinny_tn(self, Y, Z16):
        out = super().skinny_tn(Y, Z16)
        out[:, 10:] = 0
        return out


class PaddingRead(CpuTestBackend):
    """the column bound taken from the leading dimension: one padding column enters the product"""

    def skinny_nn(self, Y, T16):
        n, D = Y.shape
        ld = Y.stride(0) if n > 1 else D
        if ld == D:
            return super().skinny_nn(Y, T16)
        wide = torch.as_strided(Y, (n, D + 1), (ld, 1), Y.storage_offset())
        return wide.to(T16.dtype) @ torch.cat([T16, T16[-1:]])

    def skinny_tn(self, Y, Z16):
        n, D = Y.shape
        ld = Y.stride(0) if n > 1 else D
        if ld == D:
            return super().skinny_tn(Y, Z16)
        wide = torch.as_strided(Y, (n, D + 1), (ld, 1), Y.storage_offset())
        out = wide.to(Z16.dtype).T @ Z16
        return out[:D] + out[D:]


class RaggedRowOneUlpOff(CpuTestBackend):
    """the last row of a ragged 16-row tile comes out 1 ulp (of the f32 result) high"""

    def apply(self, A, M, bias=None, out=None):
        r = A @ M if bias is None else A @ M + bias
        if A.shape[0] % 16:
            r[-1] = torch.nextafter(r[-1], torch.full_like(r[-1], float("inf")))
        if out is None:
            return r
        out.copy_(r)
        return out


def rejected(check, *args):
    with pytest.raises(AssertionError):
        check(*args)


def test_cross_gram_transposed_is_rejected():
    rejected(R.check_gram_cross, CrossTransposed(), 16, 5, True)       # by equality (and by the transpose assertion)
    rejected(R.check_gram_cross, CrossTransposed(), 64, 513, False)
    with pytest.raises(AssertionError, match="Bm\\^T A"):
        R.check_gram_cross(CrossTransposed(), 32, 1, True)


def test_dropped_last_row_is_rejected():
    for n in (1, 3, 5, 513):
        rejected(R.check_gram, LastRowDropped(), 16, n, True)
        rejected(R.check_gram_cross, LastRowDropped(), 64, n, True)
    R.check_gram(LastRowDropped(), 16, 4, True)   # (whole groups: nothing dropped, nothing to reject)


def test_dropped_last_partial_tile_or_split_is_rejected():
    rejected(R.check_gram, LastPartialDropped(), 32, 513, True)
    R.check_gram(LastPartialDropped(), 32, 512, True)
    for ty in R.SKINNY_TYPES:
        CW = R.tile_cols(ty)
        rejected(R.check_skinny_nn, LastColumnTileDropped(), R.NnCase(ty, 17, CW + 1, CW + 1, R.ALIGNED, "general"), True)
        rejected(R.check_skinny_nn, LastColumnTileDropped(), R.NnCase(ty, 17, 2 * CW, 2 * CW, R.ALIGNED, "fast"), True)
        rejected(R.check_skinny_tn, LastSplitDropped(), R.TnCase(ty, 257, 16, 16, R.ALIGNED), True)
        R.check_skinny_tn(LastSplitDropped(), R.TnCase(ty, 256, 16, 16, R.ALIGNED), True)


def test_zeroed_high_columns_are_rejected():
    for ty in R.SKINNY_TYPES:
        CW = R.tile_cols(ty)
        rejected(R.check_skinny_nn, HighColumnsZeroed(), R.NnCase(ty, 1, CW, CW, R.ALIGNED, "fast"), True)
        rejected(R.check_skinny_tn, HighColumnsZeroed(), R.TnCase(ty, 1, 1, 1, R.ALIGNED), True)


def test_reading_the_padding_columns_is_rejected():
    for ty in R.SKINNY_TYPES:
        for case in R.nn_ld_cases(ty):
            rejected(R.check_skinny_nn, PaddingRead(), case, True)
            rejected(R.check_skinny_nn, PaddingRead(), case, False)   # (NaN: over any bound as well)
        for case in R.tn_ld_cases(ty):
            rejected(R.check_skinny_tn, PaddingRead(), case, True)


def test_one_ulp_in_a_ragged_row_is_rejected_by_the_exact_cases_only():
    """1 ulp of the f32 result is <= 2 u |ref| <= 2 u (|A| |M|)_ij: far inside the rounded bound 2 (K + 1) u (|A| |M|)_ij,
    which therefore PASSES this implementation; the exact cases reject it."""
    for B in R.APPLY_B:
        for dest, with_bias in R.APPLY_WAYS:
            rejected(R.check_apply, RaggedRowOneUlpOff(), B, 17, True, dest, with_bias)
            r = R.check_apply(RaggedRowOneUlpOff(), B, 17, False, dest, with_bias)
            assert 0.0 < r <= 1.0
    R.check_apply(RaggedRowOneUlpOff(), 16, 16, True, "fresh", False)   # (a whole tile: nothing perturbed)
