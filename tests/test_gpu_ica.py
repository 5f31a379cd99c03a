"""muon_amd.tl.ica on the device: the fused sweep of csrc/ica.hip against its numpy f64 definition, bit-equal repeats,
argument checks, routing, and every case of tests/golden/ica_golden.npz (the reference's own ``ica`` executing with the
real scikit-learn) end to end.

The sweep's bound is derived, element-wise: |A - A_ref|_ij <= (n + 16) 2^-53 (|G|^T |Z|)_ij and the same form for gp
with sum |g'|.  The test data are dyadic rationals (Z in eighths, W in sixteenths), so y = Z W^T is EXACT in f64 in any
summation order: what is left is libm's few ulps in g and g' (the + 16) and one rounding per added row (the n); the
reference sums are taken in extended precision so that the bound is the kernel's alone.  The padding columns of Z
hold NaN: the kernel masks by index and must not read them into a result.

Fixture parity: equal iteration counts, the warning and the number of kernel calls are conditions.  The project's
convention for the value bound is ten times the deviation measured on an MI355X.  NOT YET MEASURED: no MI355X could be
reached while this file was written, so PARITY_MEASURED holds None and, until a figure is entered, a case is held to
the coarse bound of tests/test_ica_host.py instead (tol / 100 = 1e-6 of max |S|: the stopping rule leaves the iterate
about tol away from the fixed point, two f64 computations of the same iterates stay orders of magnitude below that);
every case prints its deviation as MEASURE so that the figures can be entered here and in DESIGN.md 9.7.  k6_f32 is
compared with scikit-learn's result on the float64 copy of the float32 basis, bound one float32 epsilon of max |S| (the
f64 answer rounded once: half an epsilon, plus the f64 deviation)."""
import os
import warnings

import numpy as np
import pytest
import torch

from tests import ica_fixture as fx
from muon_amd import AnnData, tl
from muon_amd._core import ica as I
from muon_amd._ffi import MuonAmdError

pytestmark = pytest.mark.gpu

# max |X_ica - fixture| / max |fixture| measured on an MI355X, per f64 case (None: not yet measured, see above)
COARSE_BOUND = 1e-6
PARITY_MEASURED = {
    "k6_logcosh": None, "k6_exp": None, "k6_cube": None, "k8of19": None, "k17": None, "k33": None, "k64": None,
    "k6_iter3": None, "k6_alpha": None, "k6_arb": None, "k6_scale": None, "k6_defl": None,
}
F32_EPS = 2.0 ** -23


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "ica_golden.npz"))


def _g(y, fun, alpha):
    if fun == "logcosh":
        t = np.tanh(alpha * y)
        return t, alpha * (1 - t ** 2)
    if fun == "exp":
        e = np.exp(-(y ** 2) / 2)
        return y * e, (1 - y ** 2) * e
    return y ** 3, 3 * y ** 2


def _definition(Z, W, fun, alpha):
    """(A, gp, |G|^T |Z|, sum |g'|): g and g' in f64 from the exact y, the sums over the rows in extended precision."""
    y = Z @ W.T
    assert np.array_equal(y, (Z.astype(np.longdouble) @ W.T.astype(np.longdouble)).astype(np.float64))  # y is exact
    g, gp = _g(y, fun, alpha)
    gl, zl = g.astype(np.longdouble), Z.astype(np.longdouble)
    return ((gl.T @ zl).astype(np.float64), gp.astype(np.longdouble).sum(axis=0).astype(np.float64),
            (np.abs(gl).T @ np.abs(zl)).astype(np.float64), np.abs(gp).astype(np.longdouble).sum(axis=0).astype(np.float64))


def _operands(n, k, seed):
    """Dyadic Z [n, k] with zeros, whole zero rows and rows that push |y| past 40 (tanh saturates, g' = 0 exactly;
    exp(-y^2 / 2) underflows); a dyadic, non-orthogonal W."""
    rng = np.random.default_rng(seed)
    Z = np.round(rng.standard_normal((n, k)) * 8) / 8
    Z[rng.random((n, k)) < 0.1] = 0.0
    Z[rng.random(n) < 0.05] = 0.0
    big = rng.random(n) < 0.08
    Z[big] *= 64.0
    if n >= 15:
        Z[n // 2] = 0.0
        Z[n - 1] = 64.0 * np.sign(rng.standard_normal(k))
    W = np.round(rng.standard_normal((k, k)) * 16) / 16
    W[np.arange(k), np.arange(k)] += 1.0
    return Z, W


def _padded(hip, Z, k):
    """Z on the device in a buffer two columns wider than kp, everything past column k NaN; the [n, kp] view of it."""
    n = Z.shape[0]
    kp = (k + 15) // 16 * 16
    buf = torch.full((n, kp + 2), float("nan"), dtype=torch.float64, device=hip.device)
    buf[:, :k] = hip.to_device(Z, np.float64)
    return buf[:, :kp]


SWEEPS = [
    # n, k, fun, alpha, max_blocks
    (1, 1, "logcosh", 1.0, 0), (1, 64, "exp", 1.0, 0), (15, 2, "exp", 1.0, 0), (16, 15, "cube", 1.0, 0),
    (63, 16, "logcosh", 1.5, 0), (64, 17, "exp", 1.0, 0), (65, 33, "logcosh", 1.0, 0), (65, 64, "cube", 1.0, 0),
    (64, 48, "logcosh", 1.0, 0), (1031, 1, "exp", 1.0, 3), (1031, 17, "logcosh", 1.0, 3), (1031, 33, "exp", 1.0, 3),
    (1031, 48, "cube", 1.0, 3), (1031, 63, "logcosh", 1.5, 3), (1031, 64, "exp", 1.0, 3), (1031, 64, "logcosh", 1.0, 0),
]


@pytest.mark.parametrize("n,k,fun,alpha,max_blocks", SWEEPS)
def test_sweep_against_its_definition(hip, n, k, fun, alpha, max_blocks):
    Z, W = _operands(n, k, seed=1000 * n + k)
    A_ref, gp_ref, A_mag, gp_mag = _definition(Z, W, fun, alpha)
    if n >= 15:
        assert np.abs(Z @ W.T).max() > 40 and (Z == 0).all(axis=1).any()
    A, gp = hip.ica_sweep(_padded(hip, Z, k), hip.to_device(W, np.float64), fun, alpha, max_blocks)
    A, gp = hip.to_host(A), hip.to_host(gp)
    assert A.shape == (k, k) and gp.shape == (k,)
    assert np.isfinite(A).all() and np.isfinite(gp).all()
    unit = (n + 16) * 2.0 ** -53
    with np.errstate(divide="ignore", invalid="ignore"):
        ra = np.where(A_mag > 0, np.abs(A - A_ref) / (unit * A_mag), np.where(A == A_ref, 0.0, np.inf))
        rg = np.where(gp_mag > 0, np.abs(gp - gp_ref) / (unit * gp_mag), np.where(gp == gp_ref, 0.0, np.inf))
    print(f"MEASURE ica sweep n={n} k={k} {fun} alpha={alpha} max_blocks={max_blocks}: error / bound A {ra.max():.3g}, "
          f"gp {rg.max():.3g}")
    assert ra.max() <= 1.0 and rg.max() <= 1.0


@pytest.mark.parametrize("fun,alpha", [("logcosh", 1.0), ("logcosh", 1.5), ("exp", 1.0), ("cube", 1.0)])
def test_padded_rows_and_components_count_for_nothing(hip, fun, alpha):
    """n = 65 (one row into the second tile), k = 17 (one component into the second block): every row is zero - where
    g'(0) = alpha (logcosh) or 1 (exp), so gp COUNTS the rows that take part - but three that saturate (g' = 0)."""
    n, k = 65, 17
    Z = np.zeros((n, k))
    sat = [3, 40, 64]
    Z[sat] = 64.0
    W = np.abs(_operands(4, k, seed=5)[1]) + 1.0  # positive: y = 64 * row sum >= 64 * 17
    A, gp = hip.ica_sweep(_padded(hip, Z, k), hip.to_device(W, np.float64), fun, alpha)
    A, gp = hip.to_host(A), hip.to_host(gp)
    y = 64.0 * W.sum(axis=1)
    if fun == "logcosh":
        want_gp, want_A = np.full(k, alpha * (n - 3)), np.full((k, k), 3 * 64.0)
    elif fun == "exp":
        want_gp, want_A = np.full(k, float(n - 3)), np.zeros((k, k))
    else:
        want_gp, want_A = 3 * (3 * y ** 2), np.repeat((3 * 64.0 * y ** 3)[:, None], k, axis=1)
    assert np.array_equal(gp, want_gp), (gp, want_gp)
    assert np.array_equal(A, want_A)


def test_repeats_agree_bit_for_bit(hip):
    Z, W = _operands(1031, 64, seed=7)
    Z = Z + np.random.default_rng(8).standard_normal(Z.shape)  # (full mantissas: the order of the sums matters)
    Zd, Wd = _padded(hip, Z, 64), hip.to_device(W, np.float64)
    for max_blocks in (0, 3):
        a, b = hip.ica_sweep(Zd, Wd, "logcosh", 1.0, max_blocks), hip.ica_sweep(Zd, Wd, "logcosh", 1.0, max_blocks)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # against the tensor formulation, where y is no longer exact: both sides round y within k u (|Z| |W|^T) of each
    # other, tanh is 1-Lipschitz, and each sum over the rows rounds as in the bound of the sweep test
    t = I._sweep_torch(Zd, Wd, "logcosh", 1.0)
    Zk, u = Zd[:, :64], 2.0 ** -53
    mag = float((torch.tanh(Zk @ Wd.T).abs().T @ Zk.abs()).max())
    ymag, zsum = float((Zk.abs() @ Wd.abs().T).max()), float(Zk.abs().sum(dim=0).max())
    bound = 2 * (1031 + 16) * u * mag + 2 * 64 * u * ymag * zsum
    dev = float((a[0] - t[0]).abs().max())
    print(f"MEASURE ica sweep against the tensor formulation at 1031 x 64: max |dA| {dev:.3g} (bound {bound:.3g}, "
          f"max |A| {float(t[0].abs().max()):.3g})")
    assert dev <= bound


def test_bad_arguments_raise(hip):
    assert hip.ica_max_components() == 64
    Z = torch.zeros((40, 80), dtype=torch.float64, device=hip.device)
    W65 = torch.eye(65, dtype=torch.float64, device=hip.device)
    with pytest.raises(MuonAmdError, match="k must be"):
        hip.ica_sweep(Z, W65, "logcosh")
    W17 = torch.eye(17, dtype=torch.float64, device=hip.device)
    with pytest.raises(MuonAmdError, match="ldz"):
        hip.ica_sweep(Z[:, :17].contiguous(), W17, "logcosh")  # not padded to 32 columns
    with pytest.raises(MuonAmdError, match="ldz"):
        hip.ica_sweep(Z[:, :17], W17, "logcosh")  # a view narrower than the padded width
    flat = torch.zeros((40 * 32 + 1,), dtype=torch.float64, device=hip.device)
    with pytest.raises(MuonAmdError, match="aligned"):
        hip.ica_sweep(flat[1:].view(40, 32), W17, "logcosh")
    odd = torch.zeros((40, 33), dtype=torch.float64, device=hip.device)
    with pytest.raises(MuonAmdError, match="aligned"):
        hip.ica_sweep(odd[:, :32], W17, "logcosh")  # an odd leading dimension: rows off the 16-byte grid
    with pytest.raises(ValueError, match="fun must be"):
        hip.ica_sweep(Z[:, :32], W17, "tanh")
    # the raw entry point: a short workspace, an unknown fun
    A = torch.zeros((17, 17), dtype=torch.float64, device=hip.device)
    gp = torch.zeros((17,), dtype=torch.float64, device=hip.device)
    wb = int(hip.lib.mu_ica_worksize(40, 17, 0))
    assert wb == (32 * 32 + 32) * 8 and int(hip.lib.mu_ica_worksize(1031, 64, 3)) == 3 * (64 * 64 + 64) * 8
    work = torch.zeros((wb,), dtype=torch.uint8, device=hip.device)
    args = lambda fun, nbytes: (40, 17, 80, Z.data_ptr(), W17.data_ptr(), fun, 1.0, A.data_ptr(), gp.data_ptr(),
                                work.data_ptr(), nbytes, 0, None)
    assert hip.lib.mu_ica_sweep_f64(*args(0, wb - 8)) == -1 and b"work buffer too small" in hip.lib.mu_last_error()
    assert hip.lib.mu_ica_sweep_f64(*args(3, wb)) == -1 and b"fun must be" in hip.lib.mu_last_error()
    torch.cuda.synchronize()


class _Spy:
    """Forwards to a backend and counts the calls of the sweep kernel."""

    def __init__(self, be):
        self._be, self.calls = be, {"ica_sweep": 0}

    def __getattr__(self, name):
        got = getattr(self._be, name)
        if name in self.calls:
            def counted(*a, **k):
                self.calls[name] += 1
                return got(*a, **k)

            return counted
        return got


def _adata(X):
    return AnnData(np.zeros((X.shape[0], 1)), obsm={"X_pca": X})


def test_routing(hip):
    rng = np.random.default_rng(2)
    X = fx.sources(300, 65, rng) @ rng.standard_normal((65, 65))
    spy, diag = _Spy(hip), {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tl.ica(_adata(X), random_state=1, max_iter=2, backend=spy, diagnostics=diag)  # k = 65: past the kernel
    assert spy.calls["ica_sweep"] == 0 and diag["n_iter"] == 2
    spy, diag = _Spy(hip), {}
    tl.ica(_adata(fx.basis("k6")), random_state=fx.SEED, backend=spy, diagnostics=diag)
    assert spy.calls["ica_sweep"] == diag["n_iter"] > 1
    spy = _Spy(hip)
    tl.ica(_adata(fx.basis("k6")), random_state=fx.SEED, algorithm="deflation", backend=spy)
    assert spy.calls["ica_sweep"] == 0


@pytest.mark.parametrize("case", list(fx.CASES))
def test_fixture_case_end_to_end_on_the_device(gold, hip, case):
    X = fx.case_input(case)
    ad, diag, spy = _adata(X.copy()), {}, _Spy(hip)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        assert tl.ica(ad, random_state=fx.SEED, backend=spy, diagnostics=diag, **fx.CASES[case][2]) is None
    S = ad.obsm["X_ica"]
    ref = fx.rebuild(gold, case, X.astype(np.float64))
    assert diag["n_iter"] == int(gold[f"{case}_n_iter"][0])
    assert any(issubclass(w.category, tl.ConvergenceWarning) for w in caught) == (case in fx.NOT_CONVERGING)
    assert spy.calls["ica_sweep"] == (0 if case == "k6_defl" else diag["n_iter"])
    assert S.dtype == X.dtype and S.shape == ref.shape
    dev = float(np.abs(S.astype(np.float64) - ref).max() / np.abs(ref).max())
    measured = PARITY_MEASURED.get(case)
    bound = F32_EPS if case == "k6_f32" else (COARSE_BOUND if measured is None else 10 * measured)
    print(f"MEASURE ica device {case}: n_iter {diag['n_iter']}, max |dS| / max |S| = {dev:.4g} (bound {bound:.3g}), "
          f"last lim {diag['lim']:.4g}")
    assert dev <= bound
