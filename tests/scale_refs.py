"""TEST INFRASTRUCTURE: the plain NumPy statement of ``muon_amd.rna.pp.scale`` and the inputs of its tests
(tests/test_scale_host.py, tests/test_gpu_scale.py, tests/golden/make_scale_golden.py).

``scale_ref`` is the statement: f64 throughout, ``C = clip((A - centre) / std, lo, hi)``, ``z = clip((0 - centre) / std,
lo, hi)``, ``S = C - z``; [lo, hi] is [-max_value, max_value] with ``zero_center``, (-inf, max_value] without, and
``centre`` is ``mean`` with ``zero_center``, 0 without.  ``np.clip`` keeps a NaN.  A kernel that computes the same IEEE
operations in f64 and rounds once agrees with ``C.astype(T)`` / ``S.astype(T)`` bit for bit.
"""
import functools
import os

import numpy as np
import scipy.sparse as sp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scale_golden.npz")
N_CRAFTED = 7
# end to end: rna_fixture's b16 matrix with the crafted columns (without the NaN gene: a PCA has no answer for it)
E2E_CASES = {"b16_clip10": dict(base="b16", max_value=10.0), "b16_clip3": dict(base="b16", max_value=3.0)}


def scale_ref(A, mean, std, max_value=None, zero_center=True):
    """``(C, S, z)`` of the dense f64 matrix ``A`` for the per-gene f64 tables ``mean`` and ``std``."""
    A = np.asarray(A, dtype=np.float64)
    hi = np.inf if max_value is None else float(max_value)
    lo = -hi if zero_center else -np.inf
    centre = np.asarray(mean, dtype=np.float64) if zero_center else np.zeros(A.shape[1])
    with np.errstate(invalid="ignore"):
        C = np.clip((A - centre) / std, lo, hi)
        z = np.clip((0.0 - centre) / std, lo, hi)
        S = C - z
    return C, S, z


def moments_ref(A):
    """``(mean, std)`` per column of dense ``A``: f64, ddof = 1, 0 -> 1; a NaN is left out of its gene's moments (the
    kernel tests want one NaN element, not a NaN column)."""
    A = np.asarray(A, dtype=np.float64)
    mean = np.nanmean(A, axis=0)
    std = np.nanstd(A, axis=0, ddof=1)
    std[std == 0] = 1.0
    return mean, std


def crafted_columns(n, seed=0, with_nan=True):
    """``(dense [n, 7 or 6] f64, stored [n, 7 or 6] bool)``: the genes every scale test appends (n >= 250).
      0  all zero, nothing stored
      1  constant 2.0, stored in every cell (std 0 -> 1)
      2  5.0 in all cells but two: mean / std = sqrt(n / 2) and more, so z itself is clipped at max_value <= 10
      3  small positive values in half of the cells and one outlier of 1000: clipped from above
      4  N(0, 1) in every cell and one value of -1000: negative values, clipped from below
      5  gamma values in a third of the cells, and explicitly stored zeros in another third
      6  N(0, 1) in a fifth of the cells, one of them NaN  (left out without ``with_nan``)
    Values are f32-representable."""
    assert n >= 250
    rng = np.random.default_rng(1000 + seed)
    A = np.zeros((n, N_CRAFTED))
    st = np.zeros((n, N_CRAFTED), dtype=bool)
    A[:, 1], st[:, 1] = 2.0, True
    two = rng.choice(n, 2, replace=False)
    A[:, 2], st[:, 2] = 5.0, True
    A[two, 2], st[two, 2] = 0.0, False
    half = rng.random(n) < 0.5
    A[half, 3], st[half, 3] = rng.random(int(half.sum())) + 0.5, True
    A[rng.integers(n), 3] = 1000.0
    st[:, 3] |= A[:, 3] != 0
    A[:, 4], st[:, 4] = rng.standard_normal(n), True
    A[rng.integers(n), 4] = -1000.0
    u = rng.random(n)
    A[u < 1 / 3, 5] = rng.gamma(2.0, 1.5, int((u < 1 / 3).sum()))
    st[:, 5] = u < 2 / 3  # (the middle third: stored zeros)
    fifth = np.nonzero(rng.random(n) < 0.2)[0]
    A[fifth, 6], st[fifth, 6] = rng.standard_normal(fifth.size), True
    A[fifth[0], 6] = np.nan
    A = A.astype(np.float32).astype(np.float64)
    return (A, st) if with_nan else (A[:, :6], st[:, :6])


def csr_from(A, stored, dtype):
    """The CSR with exactly the entries ``stored`` (explicit zeros included) of dense ``A``: int64 indptr, int32
    sorted column indices, values of ``dtype``."""
    n, d = A.shape
    rows, cols = np.nonzero(stored)  # row-major: sorted columns inside a row
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64)
    m = sp.csr_matrix((A[rows, cols].astype(dtype), cols.astype(np.int32), indptr), shape=(n, d))
    m.has_sorted_indices = True
    return m


def append_crafted(M, seed=0, with_nan=True):
    """CSR ``M`` with the crafted genes appended as its last columns (stored zeros kept)."""
    A, st = crafted_columns(M.shape[0], seed, with_nan)
    M = sp.csr_matrix(M)
    out = sp.hstack([M, csr_from(A, st, M.dtype)], format="csr")
    # hstack drops nothing, but make the stored zeros' survival a fact of the fixture
    assert out.nnz == M.nnz + int(st.sum())
    out.sort_indices()
    out.indptr, out.indices = out.indptr.astype(np.int64), out.indices.astype(np.int32)
    return out


def clip_counts(A, stored, mean, std, max_value):
    """(stored entries clipped from below, from above, genes whose z is clipped) for ``zero_center=True``."""
    with np.errstate(invalid="ignore"):
        t = (A - mean) / std
        z = (0.0 - mean) / std
        return (int((stored & (t < -max_value)).sum()), int((stored & (t > max_value)).sum()),
                int((np.abs(z) > max_value).sum()))


def bits_equal(got, ref):
    """Bit-equal where the reference is a number; NaN exactly where the reference is NaN (a NaN's payload is not part
    of the statement)."""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.dtype != ref.dtype or got.shape != ref.shape:
        return False
    nan = np.isnan(ref)
    if not np.array_equal(np.isnan(got), nan):
        return False
    return np.where(nan, 0, got).tobytes() == np.where(nan, 0, ref).tobytes()


# ---- end to end ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def e2e_matrix(name):
    """The case's input: rna_fixture's log-normalised matrix rounded to f32, with the crafted genes appended (f32 CSR;
    callers copy before they change anything)."""
    from tests import rna_fixture as fx

    return append_crafted(fx.lognorm(E2E_CASES[name]["base"]).astype(np.float32), seed=5, with_nan=False)


@functools.lru_cache(maxsize=None)
def e2e_clipped_dense(name):
    """The dense clipped scaled matrix of the case in f64, from numpy's own f64 moments of the f32 input."""
    A = e2e_matrix(name).astype(np.float64).toarray()
    mean, std = moments_ref(A)
    return scale_ref(A, mean, std, E2E_CASES[name]["max_value"])[0]


@functools.lru_cache(maxsize=None)
def golden(name):
    """{"components" [k, d] f64, "variance" [k], "variance_ratio" [k]} of scikit-learn for the case (stored as
    tests/golden/rna_golden.npz stores them)."""
    with np.load(GOLDEN) as z:
        comp = z[f"{name}/components_hi"].astype(np.float64) + z[f"{name}/components_lo"].astype(np.float64) * 2.0 ** -24
        return {"components": comp, "variance": z[f"{name}/variance"].copy(),
                "variance_ratio": z[f"{name}/variance_ratio"].copy()}


def deviations(name, ad):
    """rna_fixture.deviations' four figures for a scale case: (largest principal angle of PCs, of X_pca, max relative
    deviation of variance, of variance_ratio) against the golden."""
    from oracle.lsi_oracle import max_subspace_angle

    g = golden(name)
    C = e2e_clipped_dense(name)
    expected = (C - C.mean(axis=0)) @ g["components"].T
    return (max_subspace_angle(ad.varm["PCs"], g["components"].T), max_subspace_angle(ad.obsm["X_pca"], expected),
            float(np.max(np.abs(ad.uns["pca"]["variance"] / g["variance"] - 1))),
            float(np.max(np.abs(ad.uns["pca"]["variance_ratio"] / g["variance_ratio"] - 1))))
