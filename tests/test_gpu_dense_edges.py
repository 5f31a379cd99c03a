"""The matrix-core kernels of LSI and MOFA exactly at their tile edges (csrc/dense.hip, csrc/skinny.hip): ``gram``,
``gram_cross``, ``apply``, ``project_out_block``, ``chol_rinv``, ``skinny_nn`` and ``skinny_tn`` against the references,
case tables and checking functions of tests/dense_refs.py (proved without a GPU by tests/test_dense_refs_host.py).

Exact cases - small integers in the kernel's type - ask for equality of every element with an int64 matmul; rounded
cases ask for the elementwise bound 2 (K + 1) u (|X| |W|)_ij and print the largest observed ratio to it in a MEASURE
line.  Row counts at the grid edges come from the device's CU count, which is first checked against the library's own
work-size rule.  Every operand is a view into NaN-filled surroundings, every output and work buffer lies in such
surroundings too and they must come back untouched.

What the shapes reach:
  gram / gram_cross   n = 512 -> 32 workgroups, the last direct reduce; 513 -> 33, the fold (chunk 2, fifteen empty
                      chunks); R + 1 (R = 16 x 2 x CUs) the first grid-stride step and its prefetch predicate; the tune
                      key gram_wg = 1 halves the cap.  n % 4 and n % 16 ragged, n = 0.
  apply / project     16-row tiles ragged and whole, four waves with and without work, R2 + 1 (R2 = 64 x 8 x CUs) the
                      first grid-stride step.
  chol_rinv           w at the 16-column panel edges, w = 0, B other than 16 / 32 / 64, the exact family across the
                      panel edges, NaN and near-threshold pivots.
  skinny_nn           all six instances: (f32, f64, f64 <- f32 storage) x (FAST, general), FAST with fewer column tiles
                      than waves, leading dimensions larger than D, a start that is not 16-byte aligned, R2 + 1.
  skinny_tn           D at the 128-column block, n at the 256-row split and at the 64-split cap, n = 0, ld > D.
"""
import pytest
import torch

from tests import dense_refs as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cus(hip):
    """The CU count the row tables are built from - and the library must agree about where its edge is."""
    n = int(torch.cuda.get_device_properties(hip.device).multi_processor_count)
    assert R.cus_from_gram_worksize(int(hip.lib.mu_gram_worksize(10 ** 7, 16))) == n
    assert (int(hip.lib.mu_gram_worksize(10 ** 7, 16)) - 256) / (272 * 8) - 32 == 2 * n
    return n


def measure(name, ratio):
    print(f"MEASURE {name} max |err| / bound = {ratio:.2e}")


# ---- gram, gram_cross --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.GRAM_ROWS)
@pytest.mark.parametrize("B", R.GRAM_B)
def test_gram_exact(hip, cus, B, n):
    R.check_gram(hip, B, R.rows(n, cus), True)


@pytest.mark.parametrize("n", R.GRAM_ROWS)
@pytest.mark.parametrize("B", R.GRAM_B)
def test_gram_cross_exact(hip, cus, B, n):
    R.check_gram_cross(hip, B, R.rows(n, cus), True)


@pytest.mark.parametrize("B", R.GRAM_B)
def test_gram_one_workgroup_per_cu(hip, cus, B):
    n = R.rows(R.GRAM_ONE_WG_ROWS, cus)
    try:
        R.check_gram(hip, B, n, True, gram_wg=1)
        R.check_gram_cross(hip, B, n, True, gram_wg=1)
    finally:
        hip.tune("gram_wg", 0)
    assert hip.lib.mu_tune_get(b"gram_wg") == 0


@pytest.mark.parametrize("n", R.GRAM_ROUNDED_ROWS)
@pytest.mark.parametrize("B", R.GRAM_B)
def test_gram_rounded(hip, cus, B, n):
    n = R.rows(n, cus)
    measure(f"gram B={B} n={n}", R.check_gram(hip, B, n, False))
    measure(f"gram_cross B={B} n={n}", R.check_gram_cross(hip, B, n, False))


# ---- apply, project_out_block ------------------------------------------------------------------------------------------
def _apply_all(hip, B, n):
    for dest, with_bias in R.APPLY_WAYS:
        R.check_apply(hip, B, n, True, dest, with_bias)
    R.check_project_out(hip, B, n, True)
    r = max(R.check_apply(hip, B, n, False, dest, with_bias) for dest, with_bias in R.APPLY_WAYS)
    measure(f"apply B={B} n={n}", r)
    measure(f"project_out_block B={B} n={n}", R.check_project_out(hip, B, n, False))


@pytest.mark.parametrize("n", R.APPLY_ROWS)
@pytest.mark.parametrize("B", R.APPLY_B)
def test_apply_and_project_out(hip, B, n):
    _apply_all(hip, B, n)


@pytest.mark.parametrize("n", R.APPLY_EDGE_ROWS)
@pytest.mark.parametrize("B", R.APPLY_EDGE_B)
def test_apply_and_project_out_past_one_grid(hip, cus, B, n):
    _apply_all(hip, B, R.rows(n, cus))


# ---- chol_rinv -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,w", R.CHOL_RANDOM)
def test_chol_rinv_random(hip, B, w):
    measure(f"chol_rinv B={B} w={w}", R.check_chol_random(hip, B, w))


@pytest.mark.parametrize("B,w", R.CHOL_EXACT)
def test_chol_rinv_exact_family(hip, B, w):
    R.check_chol_exact(hip, B, w)


def test_chol_rinv_flags(hip):
    measure("chol_rinv diag(1 .. 1e-10)", R.check_chol_flags(hip))


# ---- skinny_nn -----------------------------------------------------------------------------------------------------------
def _nn(hip, cases, name):
    for case in cases:
        R.check_skinny_nn(hip, case, True)
    measure(name, max(R.check_skinny_nn(hip, case, False) for case in cases))


@pytest.mark.parametrize("tiles", R.NN_FAST_TILES)
@pytest.mark.parametrize("ty", R.SKINNY_TYPES)
def test_skinny_nn_fast(hip, ty, tiles):
    D = tiles * R.tile_cols(ty)
    _nn(hip, R.nn_grid_cases(ty, D), f"skinny_nn {ty} fast D={D}")


@pytest.mark.parametrize("which", range(5))
@pytest.mark.parametrize("ty", R.SKINNY_TYPES)
def test_skinny_nn_general(hip, ty, which):
    D = R.nn_general_cols(ty)[which]
    _nn(hip, R.nn_grid_cases(ty, D), f"skinny_nn {ty} general D={D}")


@pytest.mark.parametrize("ty", R.SKINNY_TYPES)
def test_skinny_nn_past_one_grid(hip, cus, ty):
    _nn(hip, R.nn_big_cases(ty, cus), f"skinny_nn {ty} n=R2+1")


@pytest.mark.parametrize("ty", R.SKINNY_TYPES)
def test_skinny_nn_leading_dimension(hip, ty):
    _nn(hip, R.nn_ld_cases(ty), f"skinny_nn {ty} ld > D")


# ---- skinny_tn -----------------------------------------------------------------------------------------------------------
def _tn(hip, cases, name):
    for case in cases:
        R.check_skinny_tn(hip, case, True)
    measure(name, max(R.check_skinny_tn(hip, case, False) for case in cases))


@pytest.mark.parametrize("D", R.TN_COLS)
@pytest.mark.parametrize("ty", R.SKINNY_TYPES)
def test_skinny_tn(hip, ty, D):
    _tn(hip, R.tn_grid_cases(ty, D), f"skinny_tn {ty} D={D}")


@pytest.mark.parametrize("ty", R.SKINNY_TYPES)
def test_skinny_tn_at_the_split_cap(hip, ty):
    _tn(hip, R.tn_cap_cases(ty), f"skinny_tn {ty} 64 splits")


@pytest.mark.parametrize("ty", R.SKINNY_TYPES)
def test_skinny_tn_leading_dimension(hip, ty):
    _tn(hip, R.tn_ld_cases(ty), f"skinny_tn {ty} ld > D")
