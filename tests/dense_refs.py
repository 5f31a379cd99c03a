"""TEST INFRASTRUCTURE: references, case tables and checking functions for the matrix-core kernels of LSI and MOFA
(csrc/dense.hip: gram, gram_cross, apply, project_out_block, chol_rinv; csrc/skinny.hip: skinny_nn, skinny_tn).

Pure numpy and importable without a GPU.  The checks take a backend: tests/test_gpu_dense_edges.py hands them HipBackend
(the kernels), tests/test_dense_refs_host.py hands them the CPU operator set and deliberately wrong implementations, so
the tables and the checkers themselves are proved on a machine without a GPU.

EXACT cases.  Inputs are non-zero integers from [-8, 8] stored in the kernel's type (every column non-zero, nothing
symmetric).  Every product and every partial sum in any order is an integer of magnitude <= 64 K (K: the inner
dimension), + 8 where a bias or a projected block enters; each case asserts that this is below 2^24 (f32 results) or
2^53 (f64 results).  The references are int64 matmuls and the checks ask for equality of every element.

ROUNDED cases.  N(0, 1) data, the columns of the tall operand scaled by 1 + arange as tests/test_gpu_kernels.py does;
the reference is the f64 product of the stored values and the bound is elementwise,
``|got - ref| <= 2 (K + 1) u (|X| |W|)_ij`` (+ |bias| or |Z| inside the bracket where they enter), u = 2^-24 / 2^-53 for
f32 / f64 results.  (K + 1) u bounds a K-term inner product in any summation order; the factor 2 covers the final
rounding to the output type and the f32 conversion of the projection's coefficients.  A check returns the largest
observed ratio to that bound (0.0 for an exact case).

Every input is handed over as a view into a larger buffer whose surroundings hold NaN (floats) or -7 (integers), and
every buffer the backend allocates while a check runs (outputs and work buffers) is placed inside such surroundings
too; they must come back untouched.  Outputs are pre-filled with NaN: an element that is never written is seen.
"""
from collections import namedtuple
from contextlib import contextmanager
from functools import lru_cache

import numpy as np
import torch

from muon_amd._operators import has

U32, U64 = 2.0 ** -24, 2.0 ** -53
PAD = 3            # guard elements at both ends of a float / int32 buffer
PAD_BYTES = 256    # ... of a byte buffer (the work buffers: what follows must stay aligned for f64)
ALIGNED = 4        # element offset of a dense view whose start is 16-byte aligned (f32: 16 B, f64: 32 B)


# ---- row counts at the grid edges, from the CU count ---------------------------------------------------------------
_ROWS = {
    "R-1": lambda c: 32 * c - 1, "R": lambda c: 32 * c, "R+1": lambda c: 32 * c + 1, "R+5": lambda c: 32 * c + 5,
    "2R+3": lambda c: 64 * c + 3, "16cus+5": lambda c: 16 * c + 5,
    "R2-1": lambda c: 512 * c - 1, "R2": lambda c: 512 * c, "R2+1": lambda c: 512 * c + 1,
    "R2+17": lambda c: 512 * c + 17,
}


def rows(sym, cus):
    """R = 16 rows x 2 workgroups x cus: the Gram's first grid-stride step is at R + 1.  R2 = 64 rows x 8 workgroups x
    cus: the same for apply, project_out_block and skinny_nn."""
    return sym if isinstance(sym, int) else _ROWS[sym](cus)


def cus_from_gram_worksize(worksize_at_1e7_rows_b16):
    """What the library's own work-size rule says about its workgroup cap, as a CU count: mu_gram_worksize is
    (blocks + 32) (B B + B) 8 + 256 bytes with blocks = 2 cus at 10^7 rows."""
    q = (worksize_at_1e7_rows_b16 - 256) / (272 * 8) - 32
    return q / 2


# ---- guarded buffers ---------------------------------------------------------------------------------------------------
def _np(t):
    return t.detach().cpu().numpy()


def _fill(dtype):
    return float("nan") if dtype.is_floating_point else (249 if dtype == torch.uint8 else -7)


def _pad(dtype):
    return PAD_BYTES if dtype == torch.uint8 else PAD


def guarded_empty(be, shape, dtype):
    """(view, buffer): a contiguous tensor of ``shape`` inside a buffer with guard elements at both ends; all NaN / -7"""
    numel = int(np.prod(shape, dtype=np.int64))
    p = _pad(dtype)
    buf = torch.full((numel + 2 * p,), _fill(dtype), dtype=dtype, device=be.device)
    return buf[p:p + numel].view(tuple(int(s) for s in shape)), buf


def guarded(be, a):
    """``a`` (numpy) on the backend's device as a view into guarded surroundings"""
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.copy())
    view, buf = guarded_empty(be, a.shape, t.dtype)
    view.copy_(t)
    return view, buf


def strided(be, a, ld, off):
    """the n x D array ``a`` as columns [0, D) of a row-major n x ld matrix that starts ``off`` elements into a NaN
    buffer: padding columns, the space before and the space behind all hold NaN"""
    n, D = a.shape
    assert ld >= D
    t = torch.from_numpy(np.ascontiguousarray(a).copy())
    buf = torch.full((off + max(n, 1) * ld + PAD,), float("nan"), dtype=t.dtype, device=be.device)
    view = torch.as_strided(buf, (n, D), (ld, 1), off)
    view.copy_(t)
    return view, buf


def untouched(buf):
    p = _pad(buf.dtype)
    edge = torch.cat([buf[:p], buf[-p:]])
    return bool(torch.isnan(edge).all()) if buf.dtype.is_floating_point else bool((edge == _fill(buf.dtype)).all())


@contextmanager
def guarded_allocations(be):
    """While this is open, every buffer the backend's wrappers allocate through ``be.empty`` - outputs and work buffers
    - lies in guarded surroundings; on leaving, all of them must have come back untouched."""
    made = []

    def empty(shape, dtype):
        view, buf = guarded_empty(be, shape if isinstance(shape, (tuple, list)) else (shape,), dtype)
        made.append(buf)
        return view

    be.empty = empty  # (an instance attribute in front of the method)
    try:
        yield made
    finally:
        del be.empty
    for buf in made:
        assert untouched(buf), f"a {buf.dtype} buffer of {buf.numel()} elements was written outside its view"


# ---- data --------------------------------------------------------------------------------------------------------------
def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


def ints(rng, shape, dtype):
    """non-zero integers from [-8, 8]: no zero column at any size"""
    return (rng.integers(1, 9, shape) * rng.choice((-1, 1), shape)).astype(dtype)


def normals(rng, shape, dtype, scale_columns=False):
    v = rng.standard_normal(shape)
    if scale_columns:
        v = v * (1 + np.arange(shape[1]))
    return v.astype(dtype)


def exact_bound(inner, extra, result_dtype):
    """the magnitude bound 64 inner + extra of an exact case, asserted to be representable with room in the result type"""
    bound = 64 * int(inner) + int(extra)
    limit = 2 ** 24 if np.dtype(result_dtype) == np.float32 else 2 ** 53
    assert bound < limit, f"exact case out of range: {bound} >= {limit}"
    return bound


def assert_equal(got, ref, what, bound=None):
    """every element equal (a NaN anywhere is a difference); ``bound``: the case's own magnitude bound on the reference"""
    ref = np.asarray(ref)
    if bound is not None:
        assert ref.size == 0 or np.abs(ref).max() <= bound, f"{what}: the reference exceeds its magnitude bound"
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    bad = ~(got.astype(np.float64) == ref.astype(np.float64))
    if bad.any():
        i = tuple(int(x) for x in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {i}: "
                             f"got {got[i]!r}, want {ref[i]!r}")
    return 0.0


def assert_within(got, ref, bound, what):
    """elementwise |got - ref| <= bound (NaN fails); returns the largest ratio to the bound"""
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    err = np.abs(got.astype(np.float64) - ref)
    bad = ~(err <= bound)
    if bad.any():
        i = tuple(int(x) for x in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements over the bound, first at {i}: "
                             f"got {got[i]!r}, want {ref[i]!r}, |err| {err[i]:.3e} > {bound[i]:.3e}")
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


def rounded_bound(K, u, absprod, extra=0.0):
    return 2.0 * (K + 1) * u * (absprod + extra)


# ---- gram, gram_cross --------------------------------------------------------------------------------------------------
GRAM_B = (16, 32, 64)
GRAM_ROWS = (0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 511, 512, 513, 1009, "R-1", "R", "R+1", "R+5", "2R+3")
GRAM_ROUNDED_ROWS = (513, "R+5")
GRAM_ONE_WG_ROWS = "16cus+5"   # with the tune key gram_wg = 1: one workgroup per CU, the second grid-stride step ragged


@lru_cache(maxsize=4)
def gram_inputs(B, n, exact):
    rng = np.random.default_rng((B, n, int(exact), 1))
    if exact:
        A, Bm = ints(rng, (n, B), np.float32), ints(rng, (n, B), np.float32)
        ai, bi = A.astype(np.int64), Bm.astype(np.int64)
        return _frozen(A, Bm, ai.T @ ai, ai.sum(axis=0), ai.T @ bi)
    A, Bm = normals(rng, (n, B), np.float32, True), normals(rng, (n, B), np.float32, True)
    a, b = A.astype(np.float64), Bm.astype(np.float64)
    return _frozen(A, Bm, a.T @ a, a.sum(axis=0), a.T @ b)


@contextmanager
def _tuned(be, key, value):
    if value is None or not has(be, "tune"):
        yield
        return
    be.tune(key, value)
    try:
        yield
    finally:
        be.tune(key, 0)


def check_gram(be, B, n, exact, gram_wg=None):
    """G = A^T A and the column sums.  Exact: equality with int64.  Rounded: the present rtol 1e-12 (atol 1e-9) and the
    elementwise bound (the products of f32 values are exact in f64: only the n - 1 additions round)."""
    A, _Bm, refG, refcs, _refC = gram_inputs(B, n, exact)
    what = f"gram B={B} n={n} {'exact' if exact else 'rounded'}"
    Av, _ = guarded(be, A)
    with _tuned(be, "gram_wg", gram_wg), guarded_allocations(be):
        G, cs = be.gram(Av)
        G, cs = _np(G), _np(cs)
    assert G.dtype == np.float64 and cs.dtype == np.float64
    if exact:
        bound = exact_bound(n, 0, np.float64)
        assert_equal(G, refG, what, bound)
        assert_equal(cs, refcs, what + " column sums", 8 * n)
        return 0.0
    np.testing.assert_allclose(G, refG, rtol=1e-12, atol=1e-9, err_msg=what)
    np.testing.assert_allclose(cs, refcs, rtol=1e-12, atol=1e-9, err_msg=what)
    a = np.abs(A.astype(np.float64))
    r = assert_within(G, refG, rounded_bound(n, U64, a.T @ a), what)
    return max(r, assert_within(cs, refcs, rounded_bound(n, U64, a.sum(axis=0)), what + " column sums"))


def check_gram_cross(be, B, n, exact, gram_wg=None):
    """C = A^T Bm against its own reference, and not the transpose's"""
    A, Bm, _refG, _refcs, refC = gram_inputs(B, n, exact)
    what = f"gram_cross B={B} n={n} {'exact' if exact else 'rounded'}"
    Av, _ = guarded(be, A)
    Bv, _ = guarded(be, Bm)
    with _tuned(be, "gram_wg", gram_wg), guarded_allocations(be):
        C = _np(be.gram_cross(Av, Bv))
    assert C.dtype == np.float64
    if n > 0:
        assert not np.array_equal(refC, refC.T), what + ": the case is symmetric"
        assert not np.array_equal(C, refC.T), what + ": this is Bm^T A"
    if exact:
        return assert_equal(C, refC, what, exact_bound(n, 0, np.float64))
    np.testing.assert_allclose(C, refC, rtol=1e-12, atol=1e-9, err_msg=what)
    return assert_within(C, refC, rounded_bound(n, U64, np.abs(A.astype(np.float64)).T @ np.abs(Bm.astype(np.float64))),
                         what)


# ---- apply, project_out_block ------------------------------------------------------------------------------------------
APPLY_B = (16, 32, 64)
APPLY_ROWS = (1, 15, 16, 17, 63, 64, 65, 257)
APPLY_EDGE_B = (64, 16)
APPLY_EDGE_ROWS = ("R2-1", "R2", "R2+1", "R2+17")
APPLY_WAYS = (("fresh", False), ("fresh", True), ("inplace", False), ("inplace", True))  # (destination, with bias)


@lru_cache(maxsize=2)
def apply_inputs(B, n, exact):
    """A (also the basis block Q of the projection), M, bias, Z, C and the references A M and Z - A C (C: as the
    MFMA sees it, i.e. rounded to f32 - a no-op for the integer C)"""
    rng = np.random.default_rng((B, n, int(exact), 2))
    if exact:
        A, M, b = ints(rng, (n, B), np.float32), ints(rng, (B, B), np.float32), ints(rng, (B,), np.float32)
        Z, C = ints(rng, (n, B), np.float32), ints(rng, (B, B), np.float64)
        ai = A.astype(np.int64)
        return _frozen(A, M, b, Z, C, ai @ M.astype(np.int64), Z.astype(np.int64) - ai @ C.astype(np.int64))
    A, M, b = normals(rng, (n, B), np.float32, True), normals(rng, (B, B), np.float32), normals(rng, (B,), np.float32)
    Z, C = normals(rng, (n, B), np.float32), normals(rng, (B, B), np.float64)
    assert not np.array_equal(C.astype(np.float32).astype(np.float64), C)  # not representable in f32
    a = A.astype(np.float64)
    return _frozen(A, M, b, Z, C, a @ M.astype(np.float64), Z.astype(np.float64) - a @ C.astype(np.float32).astype(np.float64))


def check_apply(be, B, n, exact, dest, with_bias):
    """Out = A M (+ bias) into a fresh guarded ``out`` or in place"""
    A, M, b, _Z, _C, refP, _refZ = apply_inputs(B, n, exact)
    what = f"apply B={B} n={n} {'exact' if exact else 'rounded'} {dest}{' bias' if with_bias else ''}"
    Av, Abuf = guarded(be, A)
    Mv, _ = guarded(be, M)
    bv = guarded(be, b)[0] if with_bias else None
    out, obuf = (Av, Abuf) if dest == "inplace" else guarded_empty(be, (n, B), torch.float32)
    with guarded_allocations(be):
        got = be.apply(Av, Mv, bias=bv, out=out)
    assert got is out and untouched(obuf), what + ": wrote outside the output"
    if dest != "inplace":
        assert np.array_equal(_np(Av), A), what + ": the input changed"
    got = _np(got)
    assert got.dtype == np.float32
    ref = refP + (b.astype(refP.dtype) if with_bias else 0)
    if exact:
        return assert_equal(got, ref, what, exact_bound(B, 8, np.float32))
    absprod = np.abs(A.astype(np.float64)) @ np.abs(M.astype(np.float64))
    return assert_within(got, ref, rounded_bound(B, U32, absprod, np.abs(b.astype(np.float64)) if with_bias else 0.0),
                         what)


def check_project_out(be, B, n, exact):
    """Z <- Z - Q C, C in f64: integer-valued (exact) or not representable in f32 (rounded; the reference rounds C to
    f32 first, as include/muon_amd.h documents)"""
    Q, _M, _b, Z, C, _refP, refZ = apply_inputs(B, n, exact)
    what = f"project_out_block B={B} n={n} {'exact' if exact else 'rounded'}"
    Qv, _ = guarded(be, Q)
    Cv, _ = guarded(be, C)
    Zv, Zbuf = guarded(be, Z)
    with guarded_allocations(be):
        got = be.project_out_block(Qv, Cv, Zv)
    assert got is Zv and untouched(Zbuf), what + ": wrote outside the block"
    assert np.array_equal(_np(Qv), Q), what + ": the basis block changed"
    got = _np(got)
    if exact:
        return assert_equal(got, refZ, what, exact_bound(B, 8, np.float32))
    absprod = np.abs(Q.astype(np.float64)) @ np.abs(C.astype(np.float32).astype(np.float64))
    return assert_within(got, refZ, rounded_bound(B, U32, absprod, np.abs(Z.astype(np.float64))), what)


# ---- chol_rinv -----------------------------------------------------------------------------------------------------------
CHOL_RANDOM = ((64, 0), (64, 1), (64, 15), (64, 16), (64, 17), (64, 31), (64, 33), (64, 48), (64, 49), (64, 63),
               (64, 64), (32, 17), (16, 16), (37, 20), (10, 10), (1, 1))
CHOL_EXACT = ((64, 64), (64, 33), (32, 32))
CHOL_RTOL = 2e-6   # the present bound: |M - ref| <= 2e-6 max|ref|


@lru_cache(maxsize=None)
def chol_random_inputs(B, w):
    """(A, G, ref): a 4B x B normal block, its Gram, and inv(cholesky(G[:w, :w]).T) in the leading block of zeros"""
    rng = np.random.default_rng(B * 100 + w)
    A = rng.standard_normal((4 * B, B))
    G = A.T @ A
    ref = np.zeros((B, B))
    if w:
        ref[:w, :w] = np.linalg.inv(np.linalg.cholesky(G[:w, :w]).T)
    return _frozen(A, G, ref)


@lru_cache(maxsize=None)
def chol_exact_inputs(B):
    """The exact family G = L L^T, L = D (I - S): S has 0/1 entries on the first sub-diagonal only, with runs of ones
    across the panel edges 15|16, 31|32, 47|48 of the blocked factorisation, D is diagonal with powers of two in
    [1/4, 4].  Every intermediate of a right-looking Cholesky and of the triangular inverse is a small integer times a
    power of two, so the kernel's L, its L^-1 = (I + S + S^2 + ..) D^-1 and R^-1 = (L^-1)^T are exact in f64, and the
    entries of R^-1 - 0 or 1 / d_j - are exact in f32.  Returns (L, Linv, G); the leading w x w block of G is the
    product of the leading blocks of L, so one matrix serves every w."""
    rng = np.random.default_rng(1000 + B)
    s = rng.integers(0, 2, B - 1)
    for lo, hi in ((12, 20), (28, 35), (44, 51)):   # s[i] = 1: row i + 1 depends on row i
        s[lo:min(hi, B - 1)] = 1
    s[20:22] = 0
    d = 2.0 ** rng.integers(-2, 3, B)
    S = np.diag(s.astype(np.float64), -1)
    L = np.diag(d) @ (np.eye(B) - S)
    chain = np.eye(B)
    for i in range(1, B):      # (I - S)^-1: [i][j] = 1 where s[j] .. s[i - 1] are all ones
        for j in range(i - 1, -1, -1):
            if not s[j]:
                break
            chain[i, j] = 1.0
    Linv = chain @ np.diag(1.0 / d)
    return _frozen(L, Linv, L @ L.T)


def chol_exact_ref(B, w):
    _L, Linv, _G = chol_exact_inputs(B)
    ref = np.zeros((B, B))
    ref[:w, :w] = Linv[:w, :w].T
    return ref


def run_chol(be, G, w):
    """(M, flag) of chol_rinv on a guarded copy of G, the flag starting at 0 in guarded surroundings too"""
    Gv, _ = guarded(be, G)
    flag, fbuf = guarded(be, np.zeros(1, dtype=np.int32))
    with guarded_allocations(be), np.errstate(over="ignore", invalid="ignore"):  # (the CPU stand-in on NaN input)
        M = _np(be.chol_rinv(Gv, w, flag))
    assert untouched(fbuf), "chol_rinv wrote around its flag"
    assert M.dtype == np.float32 and M.shape == G.shape
    return M, int(_np(flag)[0])


def assert_chol_shape(M, w, what):
    B = M.shape[0]
    assert np.all(M[np.tril_indices(B, -1)] == 0) and np.all(M[w:] == 0) and np.all(M[:, w:] == 0), \
        what + ": not zero below the diagonal and outside the leading block"


def check_chol_random(be, B, w):
    A, G, ref = chol_random_inputs(B, w)
    what = f"chol_rinv random B={B} w={w}"
    M, flag = run_chol(be, G, w)
    assert flag == 0, what + ": flagged"
    M = M.astype(np.float64)
    assert_chol_shape(M, w, what)
    atol = CHOL_RTOL * (np.abs(ref).max() if w else 0.0)
    r = assert_within(M, ref, np.full(ref.shape, atol), what)
    Qm = A @ M
    assert np.allclose((Qm.T @ Qm)[:w, :w], np.eye(w), atol=1e-4), what + ": (A M)^T (A M) is not the identity"
    return r


def check_chol_exact(be, B, w):
    _L, _Linv, G = chol_exact_inputs(B)
    what = f"chol_rinv exact B={B} w={w}"
    M, flag = run_chol(be, G, w)
    assert flag == 0, what + ": flagged"
    assert_chol_shape(M, w, what)
    return assert_equal(M, chol_exact_ref(B, w), what)


def check_chol_flags(be):
    """NaN inside the leading block (on the diagonal; below it) sets the flag; NaN outside it changes nothing; a pivot
    three orders above the kernel's threshold (dmax 1e-13) passes, one three orders below it is flagged and clamped."""
    B, w = 64, 40
    _A, G, _ref = chol_random_inputs(64, 64)
    clean, flag = run_chol(be, G, w)
    assert flag == 0
    for i, j in ((7, 7), (33, 5)):
        Gn = G.copy()
        Gn[i, j] = np.nan
        _M, flag = run_chol(be, Gn, w)
        assert flag == 1, f"chol_rinv: NaN at G[{i}][{j}] inside the leading {w} x {w} block is not flagged"
    Gn = G.copy()
    Gn[w:, :] = np.nan
    Gn[:, w:] = np.nan
    M, flag = run_chol(be, Gn, w)
    assert flag == 0, "chol_rinv: NaN outside the leading block is flagged"
    assert M.tobytes() == clean.tobytes(), "chol_rinv: NaN outside the leading block changes the result"
    d = np.ones(B)
    d[-1] = 1e-10
    M, flag = run_chol(be, np.diag(d), B)
    assert flag == 0, "chol_rinv: a pivot of 1e-10 dmax is flagged"
    ref = np.diag(1.0 / np.sqrt(d))
    r = assert_within(M.astype(np.float64), ref, np.full(ref.shape, CHOL_RTOL * ref.max()), "chol_rinv diag(1 .. 1e-10)")
    d[-1] = 1e-16
    M, flag = run_chol(be, np.diag(d), B)
    assert flag == 1, "chol_rinv: a pivot of 1e-16 dmax is not flagged"
    assert np.all(np.isfinite(M)), "chol_rinv: a clamped pivot left something non-finite"
    return r


# ---- skinny_nn, skinny_tn ------------------------------------------------------------------------------------------------
SKINNY_TYPES = {"f32": (np.float32, np.float32), "f64": (np.float64, np.float64), "f64_f32": (np.float32, np.float64)}


def tile_cols(ty):
    """CW: the columns of one 128-byte tile of the STORED type"""
    return 128 // np.dtype(SKINNY_TYPES[ty][0]).itemsize


def nn_build(ptr, ld, D, elem):
    """the build mu_skinny_nn* picks at launch (csrc/skinny.hip, nn_fast): branch-free loads need a 16-byte aligned
    start, a leading dimension of whole 16-byte pieces and a D of whole 128-byte tiles"""
    return "fast" if ptr % 16 == 0 and (ld * elem) % 16 == 0 and D > 0 and (D * elem) % 128 == 0 else "general"


NN_FAST_TILES = (1, 2, 3, 4, 5, 9)                  # D = tiles CW: fewer tiles than waves at 1, 2, 3
NN_ROWS = (1, 15, 16, 17, 63, 64, 65, 129)
NnCase = namedtuple("NnCase", "ty n D ld off build")
TnCase = namedtuple("TnCase", "ty n D ld off")


def nn_general_cols(ty):
    CW = tile_cols(ty)
    return (1, 3, CW - 1, CW + 1, 4 * CW + 1)


def nn_grid_cases(ty, D):
    build = "fast" if D % tile_cols(ty) == 0 else "general"
    return [NnCase(ty, n, D, D, ALIGNED, build) for n in NN_ROWS]


def nn_big_cases(ty, cus):
    n = rows("R2+1", cus)   # one 64-row step past the workgroup cap: the kernel's grid-stride loop
    return [NnCase(ty, n, tile_cols(ty), tile_cols(ty), ALIGNED, "fast"), NnCase(ty, n, 3, 3, ALIGNED, "general")]


def nn_ld_cases(ty):
    """Y as a column slice of a wider NaN-filled matrix.  (With ld = D no general shape has a leading dimension of whole
    16-byte pieces: the last case is the general build WITH its 16-byte loads and a ragged last piece.)"""
    CW = tile_cols(ty)
    D = 4 * CW
    return [NnCase(ty, 65, D, D + 8, ALIGNED, "fast"),           # whole pieces, aligned start: stays fast
            NnCase(ty, 65, D, D + 7, ALIGNED, "general"),        # odd leading dimension
            NnCase(ty, 65, D, D + 8, ALIGNED + 1, "general"),    # the start moved by one element
            NnCase(ty, 17, 2 * CW, 2 * CW + 24, ALIGNED, "fast"),
            NnCase(ty, 65, D + 1, D + 8, ALIGNED, "general")]


TN_COLS = (1, 15, 16, 17, 127, 128, 129, 257)        # 128 columns per workgroup
TN_ROWS = (0, 1, 3, 4, 5, 15, 16, 17, 255, 256, 257, 513)   # one row split per 256 rows
TN_CAP_ROWS = (16384, 16385)                          # at D = 16: 64 and 65 splits wanted, 64 is the cap


def tn_grid_cases(ty, D):
    return [TnCase(ty, n, D, D, ALIGNED) for n in TN_ROWS]


def tn_cap_cases(ty):
    return [TnCase(ty, n, 16, 16, ALIGNED) for n in TN_CAP_ROWS]


def tn_ld_cases(ty):
    return [TnCase(ty, 257, D, ld, off) for D in (17, 128) for ld, off in ((D + 8, ALIGNED), (D + 7, ALIGNED),
                                                                           (D + 8, ALIGNED + 1))]


def tn_splits(n, D, cus):
    """the row splits of mu_skinny_tn* (csrc/skinny.hip, tn_splits): ~8 workgroups per CU, >= 256 rows each, <= 64"""
    cbs = -(-D // 128)
    return max(1, min(-(-8 * cus // cbs), -(-n // 256), 64))


@lru_cache(maxsize=8)
def skinny_inputs(ty, n, D, exact):
    """Y [n x D] in the stored type, T16 [D x 16] and Z16 [n x 16] in the result type - all 16 columns in use - and the
    references Y T16 and Y^T Z16"""
    TY, T = SKINNY_TYPES[ty]
    rng = np.random.default_rng((n, D, int(exact), 3))
    if exact:
        Y, T16, Z16 = ints(rng, (n, D), TY), ints(rng, (D, 16), T), ints(rng, (n, 16), T)
        yi = Y.astype(np.int64)
        return _frozen(Y, T16, Z16, yi @ T16.astype(np.int64), yi.T @ Z16.astype(np.int64))
    Y, T16, Z16 = normals(rng, (n, D), TY, True), normals(rng, (D, 16), T), normals(rng, (n, 16), T)
    y = Y.astype(np.float64)
    return _frozen(Y, T16, Z16, y @ T16.astype(np.float64), y.T @ Z16.astype(np.float64))


def _unit(ty):
    return U32 if SKINNY_TYPES[ty][1] == np.float32 else U64


def check_skinny_nn(be, case, exact):
    ty, n, D, ld, off, build = case
    Y, T16, _Z16, ref, _refT = skinny_inputs(ty, n, D, exact)
    what = f"skinny_nn {case} {'exact' if exact else 'rounded'}"
    Yv, _ = strided(be, Y, ld, off)
    # the build this case is meant for, from the documented rule with the numbers the launch sees
    assert nn_build(Yv.data_ptr(), ld if n > 1 else D, D, Y.itemsize) == build, what + ": not the build it names"
    Tv, _ = guarded(be, T16)
    with guarded_allocations(be):
        got = _np(be.skinny_nn(Yv, Tv))
    assert got.dtype == SKINNY_TYPES[ty][1]
    if exact:
        return assert_equal(got, ref, what, exact_bound(D, 0, got.dtype))
    return assert_within(got, ref, rounded_bound(D, _unit(ty), np.abs(Y.astype(np.float64)) @ np.abs(T16.astype(np.float64))),
                         what)


def check_skinny_tn(be, case, exact):
    """... and for the mixed instance the present identity: the bytes of tn on the widened copy of the stored values"""
    ty, n, D, ld, off = case
    Y, _T16, Z16, _ref, ref = skinny_inputs(ty, n, D, exact)
    what = f"skinny_tn {case} {'exact' if exact else 'rounded'}"
    Yv, _ = strided(be, Y, ld, off)
    Zv, _ = guarded(be, Z16)
    with guarded_allocations(be):
        got = _np(be.skinny_tn(Yv, Zv))
        if ty == "f64_f32":
            wide = _np(be.skinny_tn(guarded(be, Y.astype(np.float64))[0], Zv))
            assert got.tobytes() == wide.tobytes(), what + ": not the bytes of the f64 kernel on the widened copy"
    assert got.dtype == SKINNY_TYPES[ty][1]
    if exact:
        return assert_equal(got, ref, what, exact_bound(n, 0, got.dtype))
    return assert_within(got, ref, rounded_bound(n, _unit(ty), np.abs(Y.astype(np.float64)).T @ np.abs(Z16.astype(np.float64))),
                         what)
