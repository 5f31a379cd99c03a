"""muon_amd.tl.snf on the device: the kernels of csrc/snf.hip against their definitions at the tile edges (64 x 64 tiles,
64 lanes, four waves: N = 2, 63, 64, 65, 127, 129, 257), bit-equal repeats, routing, and every case of
tests/golden/snf_golden.npz (the reference's own ``snf`` executing) end to end on the kernel path.

Every matrix handed to a kernel is the N x N view of a buffer three columns wider whose padding holds NaN: the kernels
mask by index.

``snf_diffuse`` is compared BIT FOR BIT with numpy: P holds 64ths, the terms of X hold multiples of (number of terms) /
8, all small, so the mean, every product and every partial sum are exact in f64 in any order.

The affinity's element-wise bound, relative, in units of u = 2^-53, with z = D / (sigma sig) <= 3 / sigma:
  * D <- (D + D^T) / 2 is one IEEE addition and an exact halving on both sides: the same bits;
  * means_i: at most k positive values added in two different orders (k - 1 roundings each), a division and the
    addition of eps on each side: the two differ by at most 2 (k + 1) u =: g;
  * sig adds positive terms, so it inherits g, plus the roundings of its five operations on each side: g + 10 u;
    scale = sigma sig: g + 12 u; y = D / scale: g + 14 u;
  * the exponent y^2 / 2 then differs by (2 (g + 14 u) + 2 u) z^2 / 2 ABSOLUTELY, which is the relative difference of
    its exponential: (g + 15 u) z^2; both exponentials are good to an ulp (2 u each): 4 u;
  * / sqrt(2 pi): 2 u; / scale: g + 12 u and the two roundings, g + 14 u; (dens + dens^T) / 2 is exact.
  Sum: ((2 k + 22) + (2 k + 17) z^2) u.

The normalisation: r_i = sum - diagonal from two summation orders of n values differs by 2 (n - 1) u S_i / r_i
relatively (S_i = sum |x_ij|; the subtraction amplifies by S_i / r_i) plus its own rounding; x_ij / (2 r_i) adds a
rounding, the mean of the two scaled values one more on each side: (2 (n - 1) max(S_i / r_i, S_j / r_j) + 8) u.

Fixture parity: index arrays equal the fixture's exactly for every case.  The project's convention for the value
bound is ten times the deviation measured on an MI355X, entered per case in PARITY_MEASURED (and DESIGN.md 9.9), and
never below one ulp of 1 (a measured 0 or half-ulp figure times ten is no bound); a case without a figure is held to the
host test's 1e-12.  Every case prints MEASURE."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import snf_fixture as fx
from muon_amd import tl
from muon_amd._core import snf as S

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
EDGES = (2, 63, 64, 65, 127, 129, 257)
HOST_BOUND = 1e-12
# largest deviation measured on an MI355X per case: (W rows rel, distances abs, connectivities rel); None: not yet
PARITY_MEASURED = {
    "n21_k20": (8.07e-16, 5.55e-17, 8.07e-16), "n65_k5": (1.29e-15, 5.55e-17, 1.07e-15),
    "n129_k64": (8.79e-16, 5.55e-17, 1.03e-15), "n150_k10": (9.59e-15, 2.78e-16, 4.53e-15),
    "n257_k20": (1.56e-15, 5.55e-17, 9.77e-16),
}


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "snf_golden.npz"))


def padded(hip, A):
    """A on the device as the n x n view of a buffer three columns wider, NaN in the padding."""
    n = A.shape[0]
    buf = torch.full((n, n + 3), float("nan"), dtype=torch.float64, device=hip.device)
    buf[:, :n] = hip.to_device(np.ascontiguousarray(A), np.float64)
    return buf[:, :n]


def padding_untouched(view):
    n = view.shape[0]
    base = torch.as_strided(view, (n, n + 3), (n + 3, 1))
    return bool(torch.isnan(base[:, n:]).all())


def device_csr(hip, P):
    c = sp.csr_matrix(P)
    c.sort_indices()
    return (hip.to_device(c.indptr, np.int64), hip.to_device(c.indices, np.int32), hip.to_device(c.data, np.float64))


# ---- snf_diffuse ---------------------------------------------------------------------------------------------------------
def p_pattern(kind, n, rng):
    """Dense P in 64ths.  k1 / k20 / k64: that many entries per column, the diagonal among them; hub: k20 plus a row
    with n entries and a row whose only entry is its diagonal."""
    P = np.zeros((n, n))
    val = lambda size: rng.integers(1, 64, size) / 64.0
    if kind == "diag":
        P[np.arange(n), np.arange(n)] = val(n)
        return P
    k = min({"k1": 1, "k20": 20, "k64": 64, "hub": 20}[kind], n)
    for j in range(n):
        rows = rng.choice(n, k, replace=False)
        if j not in rows:
            rows[0] = j
        P[rows, j] = val(k)
    if kind == "hub":
        P[0, :] = val(n)
        lonely = n - 1
        P[lonely, :] = 0
        P[lonely, lonely] = 0.5
        assert (P[0] != 0).all() and (P[lonely] != 0).sum() == 1
    return P


@pytest.mark.parametrize("terms", (1, 2, 7))
@pytest.mark.parametrize("n", EDGES)
def test_diffuse_bit_for_bit_against_its_definition(hip, n, terms):
    rng = np.random.default_rng(100 * n + terms)
    Xs = [rng.integers(-16, 17, (n, n)) * terms / 8.0 for _ in range(terms)]
    X = np.zeros((n, n))
    for x in Xs:
        X = X + x
    X = X / terms
    assert np.array_equal(X * 8, np.round(X * 8))  # the mean is exact
    dX = [padded(hip, x) for x in Xs]
    for kind in ("diag", "hub", "k1", "k20", "k64"):
        P = p_pattern(kind, n, rng)
        csr = device_csr(hip, P)
        half, full = padded(hip, np.zeros((n, n))), padded(hip, np.zeros((n, n)))
        hip.snf_diffuse(csr, dX, half)
        assert np.array_equal(hip.to_host(half), (P @ X).T), (kind, "one pass")
        hip.snf_diffuse(csr, [half], full)
        assert np.array_equal(hip.to_host(full), P @ X @ P.T), (kind, "two passes")
        assert padding_untouched(half) and padding_untouched(full)


def test_diffuse_refuses_more_terms_than_it_adds_and_its_own_output(hip):
    from muon_amd._ffi import MuonAmdError

    n = 8
    csr = device_csr(hip, np.eye(n))
    X = padded(hip, np.ones((n, n)))
    with pytest.raises(MuonAmdError, match="nmat must be 1..8"):
        hip.snf_diffuse(csr, [X] * 9, padded(hip, np.zeros((n, n))))
    with pytest.raises(MuonAmdError, match="Y must not be one of the terms"):
        hip.snf_diffuse(csr, [X], X)
    # S.diffuse pre-sums past the limit
    Xs = [padded(hip, np.full((n, n), float(i))) for i in range(9)]
    out = S.diffuse(hip, csr, Xs, padded(hip, np.zeros((n, n))))
    assert np.array_equal(hip.to_host(out), np.full((n, n), 4.0))


# ---- snf_topk and the scaling of P ------------------------------------------------------------------------------------------
def distinct_matrix(n, rng, symmetric):
    """n x n with all values distinct (negative ones and a zero among them).  symmetric: positive, and the diagonal
    holds the largest value of its row, as after ``_normalize`` - every dominate set keeps it, no row of z is empty."""
    if symmetric:
        iu = np.triu_indices(n)
        vals = (rng.permutation(iu[0].size) + 1.0) / iu[0].size
        W = np.zeros((n, n))
        W[iu] = vals
        W = W + np.triu(W, 1).T
        W[np.arange(n), np.arange(n)] += 1.0
        return W
    return (rng.permutation(n * n).reshape(n, n) - n) / float(n)


@pytest.mark.parametrize("k", (1, 5, 20, 63, 64))
def test_topk_equals_argsort(hip, k):
    for n in sorted({k + 1, *[e for e in EDGES if e > k]}):
        rng = np.random.default_rng(1000 * k + n)
        W = distinct_matrix(n, rng, symmetric=False)
        idx, val = hip.snf_topk(padded(hip, W), k)
        order = np.argsort(-W, axis=1, kind="stable")[:, :k]
        assert np.array_equal(hip.to_host(idx), order), n
        assert np.array_equal(hip.to_host(val), np.take_along_axis(W, order, axis=1)), n


@pytest.mark.parametrize("n,k", [(2, 1), (21, 20), (65, 5), (129, 64), (130, 65), (257, 20)])
def test_dominate_set_scaling_to_4_ulp_and_its_route(hip, n, k):
    rng = np.random.default_rng(n + k)
    W = distinct_matrix(n, rng, symmetric=True)
    diag = {}
    (indptr, cols, vals), rowsum = S.dominate_csr(hip, padded(hip, W), k, diag)
    assert diag["topk"] == ["kernel" if k <= 64 else "tensor"]
    ref = fx.np_dominateset(W, k)
    P = sp.csr_matrix((hip.to_host(vals), hip.to_host(cols), hip.to_host(indptr)), shape=(n, n))
    assert P.has_sorted_indices and np.array_equal(np.diff(P.indptr), (ref != 0).sum(axis=1))
    Pd = P.toarray()
    assert np.array_equal(Pd != 0, ref != 0) and (Pd != 0).sum(axis=0).tolist() == [k] * n
    assert np.all(np.abs(Pd - ref) <= 4 * np.spacing(np.abs(ref)))


# ---- snf_affinity, snf_normalize ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", EDGES)
def test_affinity_against_its_numpy_statement(hip, n):
    rng = np.random.default_rng(n)
    for k, sigma in ((min(5, n - 1), 0.5), (min(64, n - 1), 0.3), (min(127, n - 1), 0.5)):
        D = rng.uniform(0.5, 4.0, (n, n))  # asymmetric, a non-zero diagonal
        if n >= 63:
            D[3, 10:] = np.inf  # a row with fewer finite values than k + 1 where k >= 9: the finite mean
            D[7, 20] = np.inf
        ref = fx.np_affinity(D.copy(), k, sigma)
        Ds = (D + D.T) / 2
        np.fill_diagonal(Ds, 0)
        srt = np.sort(Ds, axis=1)[:, 1:k + 1]
        means = np.array([r[~np.isinf(r)].mean() for r in srt]) + fx.EPS
        with np.errstate(invalid="ignore"):
            z = Ds / (sigma * (np.add.outer(means, means) / 3 + Ds / 3 + fx.EPS))
        for in_place in (False, True):
            src = padded(hip, D)
            out = hip.snf_affinity(src, k, sigma, fx.EPS, out=src if in_place else padded(hip, np.zeros((n, n))))
            W = hip.to_host(out)
            assert padding_untouched(out)
            assert np.array_equal(np.isnan(W), np.isnan(ref))
            ok = ~np.isnan(ref)
            assert n < 63 or (~ok).sum() > 0
            bound = ((2 * k + 22) + (2 * k + 17) * z[ok] ** 2) * U
            dev = np.abs(W[ok] - ref[ok]) / ref[ok]
            print(f"MEASURE snf affinity n={n} k={k}: max deviation / bound {float(np.max(dev / bound)):.3g}")
            assert np.all(dev <= bound)
            assert np.array_equal(W, W.T, equal_nan=True)


@pytest.mark.parametrize("n", EDGES)
def test_normalize_against_its_numpy_statement(hip, n):
    rng = np.random.default_rng(n)
    X = rng.uniform(0.0, 1.0, (n, n))
    X[n // 2, :] = 0.0
    X[n // 2, n // 2] = 0.75  # off-diagonal sum 0: r = 1
    ref = fx.np_normalize(X.copy())
    r = X.sum(axis=1) - X.diagonal()
    amp = np.where(r == 0, 1.0, np.abs(X).sum(axis=1) / np.where(r == 0, 1.0, r))
    bound = (2 * (n - 1) * np.maximum.outer(amp, amp) + 8) * U
    out = hip.snf_normalize(padded(hip, X), out=padded(hip, np.zeros((n, n))))
    W = hip.to_host(out)
    same = padded(hip, X)
    hip.snf_normalize(same, out=same)
    assert np.array_equal(W, hip.to_host(same))  # in place: the same bits
    assert padding_untouched(out) and padding_untouched(same)
    assert np.array_equal(W, W.T) and np.all(np.diag(W) == 0.5)
    dev = np.abs(W - ref) / np.where(ref == 0, 1.0, np.abs(ref))
    print(f"MEASURE snf normalize n={n}: max deviation / bound {float(np.max(dev / bound)):.3g}")
    assert np.all(dev <= bound)


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def run_case(hip, case, **extra):
    md, diag = fx.mudata(case, **extra), {}
    assert tl.snf(md, backend=hip, diagnostics=diag, **fx.call_kwargs(case)) is None
    return md, diag


@pytest.fixture(scope="module")
def case_runs(hip):
    return {case: run_case(hip, case) for case in fx.CASES}


@pytest.mark.parametrize("case", list(fx.CASES))
def test_fixture_parity_on_the_kernel_path(gold, case_runs, case):
    md, diag = case_runs[case]
    c = fx.CASES[case]
    assert diag["path"] == "kernel" and diag["affinity"] == "kernel" and diag["topk"] == ["kernel"] * c["M"]
    assert diag["diffuse_terms"] == c["M"] - 1  # (n257_k20: the sum over two pointers is formed on read)
    for counts in diag["p_row_counts"]:
        assert counts.sum() == c["n"] * c["k"] and counts.min() >= 1
    devs = fx.check_against_fixture(gold, case, md, diag, "device")
    measured = PARITY_MEASURED[case]
    bounds = (HOST_BOUND,) * 3 if measured is None else tuple(max(10 * m, 2.0 ** -52) for m in measured)
    assert all(d <= b for d, b in zip(devs, bounds)), (devs, bounds)


def test_two_runs_agree_bit_for_bit(hip, case_runs):
    md, diag = run_case(hip, "n257_k20")
    first_md, first = case_runs["n257_k20"]
    assert np.array_equal(diag["W"], first["W"])
    assert np.array_equal(md.obsp["distances"].data, first_md.obsp["distances"].data)


def test_sparse_distances_are_computed_on_the_device(hip, case_runs):
    md, diag = run_case(hip, "n65_k5", sparse=("m0", "m1"))
    assert diag["distances"] == ["computed", "computed"] and diag["path"] == "kernel"
    ref = case_runs["n65_k5"][1]["W"]
    dev = float(np.max(np.abs(diag["W"] - ref) / ref))
    print(f"MEASURE snf computed distances against the dense input: {dev:.3g} (0: the same bits)")
    assert dev <= HOST_BOUND
    assert np.array_equal(md.obsp["snf_distances"].indices, case_runs["n65_k5"][0].obsp["snf_distances"].indices)
