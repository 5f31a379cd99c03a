"""The Gauss-Seidel sweeps of the two-pass MOFA engine, mu_mofa_update_w and mu_mofa_update_z (csrc/mofa.hip), called
directly and compared with a float64 numpy restatement of the oracle's loops (oracle/mofa_oracle.py, the W and Z
sections of run()), at the shapes where the kernels can go wrong: K at and around the register widths 16 and 32 of the
two instantiations, feature / sample counts around the 128-thread block, and G up to the largest group count the
kernel's LDS tile holds at that K.

Data are O(1) with strictly diagonally dominant Grams (off-diagonal row sums <= 0.8, diagonals in [1, 2), second
moments above the diagonals), so one sweep amplifies no rounding error.  f32 runs take inputs rounded to f32; the
reference runs in f64 on the rounded values.  Error = max |got - ref| / max |ref| per output array.  Largest errors
measured on an MI355X over the whole grid: update_w f64 3.4e-15, f32 5.2e-6 (both at K = 2, G = 1250: the longest
sums over groups); update_z f64 7.4e-16, f32 2.1e-7.  The tolerances hold a margin of about 10x over those.
Rows past D (N) carry a sentinel that must come back untouched, and a second launch must give the same bits."""
import numpy as np
import pytest
import torch

from muon_amd._core.mofa_engine import LDS_TILE_BYTES

pytestmark = pytest.mark.gpu

TOL_W = {torch.float64: 4e-14, torch.float32: 6e-5}
TOL_Z = {torch.float64: 1e-14, torch.float32: 3e-6}
KS = [1, 2, 15, 16, 17, 31, 32]
SIZES = [1, 127, 128, 129, 4099]
PAD = 3  # sentinel rows past D (N)
SENTINEL = 7.25


def _gmax_w(K):
    return LDS_TILE_BYTES // (8 * (K * K + K))


def _gmax_z(M, K):
    return LDS_TILE_BYTES // (8 * M * (K * K + 2 * K))


def _groups(gmax):
    return sorted({1, min(3, gmax), gmax})


def _gram(rng, G, K):
    """G symmetric K x K matrices: off-diagonal row sums <= 0.8, diagonal in [1, 2)."""
    off = rng.uniform(-1, 1, (G, K, K))
    off = 0.5 * (off + off.transpose(0, 2, 1)) * (0.8 / max(K - 1, 1))
    idx = np.arange(K)
    off[:, idx, idx] = 1.0 + rng.random((G, K))
    return off


def _rounded(dtype, *arrays):
    """The inputs as the kernel sees them, in f64."""
    npdt = np.float32 if dtype == torch.float32 else np.float64
    return [a.astype(npdt).astype(np.float64) for a in arrays]


def _err(got, ref):
    return float(np.max(np.abs(got - ref)) / max(float(np.max(np.abs(ref))), 1e-300))


# ---- W: one thread per feature ------------------------------------------------------------------------------------------
def ref_update_w(B, tau, Gz, Z2, alpha, lth, l1mth, spikeslab, EW):
    """oracle/mofa_oracle.py, the W section of one iteration for one view, in f64."""
    G, D, K = B.shape
    EW = EW.copy()
    EW2, gamma, EWh2, sig2 = (np.zeros((D, K)) for _ in range(4))
    for k in range(K):
        t = np.zeros(D)
        q = np.zeros(D)
        for g in range(G):
            cross = EW @ Gz[g][:, k] - EW[:, k] * Gz[g][k, k]
            t += tau[g] * (B[g][:, k] - cross)
            q += tau[g] * Z2[g][k]
        prec = q + alpha[k]
        s2 = 1.0 / prec
        mu = t * s2
        if spikeslab:
            lam = lth[k] - l1mth[k] + 0.5 * np.log(alpha[k]) - 0.5 * np.log(prec) + 0.5 * t * t * s2
            gam = 1.0 / (1.0 + np.exp(-lam))
        else:
            gam = np.ones(D)
        EW[:, k] = gam * mu
        EW2[:, k] = gam * (mu * mu + s2)
        gamma[:, k] = gam
        EWh2[:, k] = gam * (mu * mu + s2) + (1.0 - gam) / alpha[k]
        sig2[:, k] = s2
    return {"EW": EW, "EW2": EW2, "gamma": gamma, "EWh2": EWh2, "sig2": sig2}


def w_case(seed, D, K, G, dtype):
    rng = np.random.default_rng(seed)
    B = rng.uniform(-1, 1, (G, D, K))
    tau = rng.uniform(0.5, 1.5, (G, D))
    Gz = _gram(rng, G, K)
    Z2 = np.diagonal(Gz, axis1=1, axis2=2) + rng.uniform(0.1, 0.5, (G, K))
    alpha = rng.uniform(0.5, 2.0, K)
    p = rng.uniform(0.2, 0.8, K)
    lth, l1mth = np.log(p), np.log1p(-p)
    EW = rng.uniform(-1, 1, (D, K))
    return _rounded(dtype, B, tau, Gz, Z2, alpha, lth, l1mth, EW)


def run_update_w(hip, dtype, inputs, spikeslab):
    B, tau, Gz, Z2, alpha, lth, l1mth, EW = inputs
    G, D, K = B.shape
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device=hip.device, dtype=dtype)
    outs = {n: torch.full((D + PAD, K), SENTINEL, dtype=dtype, device=hip.device)
            for n in ("EW", "EW2", "gamma", "EWh2", "sig2")}
    outs["EW"][:D] = dev(EW)
    hip.mofa_update_w(dev(B), dev(tau), dev(Gz), dev(Z2), dev(alpha), dev(lth), dev(l1mth), spikeslab, outs["EW"],
                      outs["EW2"], outs["gamma"], outs["EWh2"], outs["sig2"])
    torch.cuda.synchronize(hip.device)
    return {n: t.cpu() for n, t in outs.items()}


def check_update_w(hip, dtype, D, K, G, spikeslab, seed=0):
    """Returns the largest error against the f64 reference; asserts the sentinels and run-to-run bits."""
    inputs = w_case(seed, D, K, G, dtype)
    got = run_update_w(hip, dtype, inputs, spikeslab)
    again = run_update_w(hip, dtype, inputs, spikeslab)
    ref = ref_update_w(*inputs[:7], spikeslab, inputs[7])
    err = 0.0
    for n, r in ref.items():
        assert torch.equal(got[n], again[n]), ("not bit-identical from run to run", n)
        assert bool((got[n][D:] == SENTINEL).all()), ("row past D written", n)
        err = max(err, _err(got[n][:D].double().numpy(), r))
    return err


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("gsel", ["1", "3", "max"])
@pytest.mark.parametrize("K", KS)
def test_update_w_matches_f64_gauss_seidel(hip, K, gsel, dtype):
    G = {"1": 1, "3": min(3, _gmax_w(K)), "max": _gmax_w(K)}[gsel]
    for D in SIZES:
        for ss in (True, False):
            err = check_update_w(hip, dtype, D, K, G, ss, seed=D * 7 + G)
            assert err <= TOL_W[dtype], (D, K, G, ss, err)


# ---- Z: one thread per sample -------------------------------------------------------------------------------------------
def ref_update_z(A, pres, grp, Gw, dw2, alphaz, corr, EZ):
    """oracle/mofa_oracle.py, the Z section of one iteration (group by group; the sparse view's centring term `corr` is
    taken off A of the samples present), in f64."""
    M, N, K = A.shape
    G = alphaz.shape[0]
    EZ = EZ.copy()
    EZ2, sig2 = np.zeros((N, K)), np.zeros((N, K))
    co = np.zeros((M, G, K)) if corr is None else corr
    for g in range(G):
        i = np.nonzero(grp == g)[0]
        for k in range(K):
            num = np.zeros(len(i))
            prec = np.full(len(i), alphaz[g, k])
            for m in range(M):
                mk = pres[m, i]
                cross = EZ[i] @ Gw[m, g][:, k] - EZ[i, k] * Gw[m, g][k, k]
                num += mk * (A[m][i, k] - co[m, g, k] - cross)
                prec += mk * dw2[m, g][k]
            EZ[i, k] = num / prec
            sig2[i, k] = 1.0 / prec
            EZ2[i, k] = EZ[i, k] ** 2 + 1.0 / prec
    return {"EZ": EZ, "EZ2": EZ2, "sig2": sig2}


def z_case(seed, N, K, M, G, dtype, with_corr):
    rng = np.random.default_rng(seed)
    A = rng.uniform(-1, 1, (M, N, K))
    pres = (rng.random((M, N)) < 0.8).astype(np.float64)
    if N >= 3:
        pres[:, N // 2] = 0.0  # a sample absent from every view
    grp = rng.integers(0, G, N).astype(np.int32)
    grp[0] = G - 1  # the last group's Grams (the end of the tile) are read; the order is not sorted
    if N > 1:
        grp[-1] = 0
    Gw = _gram(rng, M * G, K).reshape(M, G, K, K)
    dw2 = np.diagonal(Gw, axis1=2, axis2=3) + rng.uniform(0.1, 0.5, (M, G, K))
    alphaz = rng.uniform(0.5, 2.0, (G, K))
    corr = rng.uniform(-0.5, 0.5, (M, G, K)) if with_corr else None
    EZ = rng.uniform(-1, 1, (N, K))
    A, pres, Gw, dw2, alphaz, EZ = _rounded(dtype, A, pres, Gw, dw2, alphaz, EZ)
    if corr is not None:
        (corr,) = _rounded(dtype, corr)
    return A, pres, grp, Gw, dw2, alphaz, corr, EZ


def run_update_z(hip, dtype, inputs):
    A, pres, grp, Gw, dw2, alphaz, corr, EZ = inputs
    M, N, K = A.shape
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device=hip.device, dtype=dtype)
    outs = {n: torch.full((N + PAD, K), SENTINEL, dtype=dtype, device=hip.device) for n in ("EZ", "EZ2", "sig2")}
    outs["EZ"][:N] = dev(EZ)
    hip.mofa_update_z(dev(A), dev(pres), torch.from_numpy(grp).to(hip.device), dev(Gw), dev(dw2), dev(alphaz),
                      outs["EZ"], outs["EZ2"], outs["sig2"], corr=None if corr is None else dev(corr))
    torch.cuda.synchronize(hip.device)
    return {n: t.cpu() for n, t in outs.items()}


def check_update_z(hip, dtype, N, K, M, G, with_corr, seed=0):
    inputs = z_case(seed, N, K, M, G, dtype, with_corr)
    got = run_update_z(hip, dtype, inputs)
    again = run_update_z(hip, dtype, inputs)
    ref = ref_update_z(*inputs)
    err = 0.0
    for n, r in ref.items():
        assert torch.equal(got[n], again[n]), ("not bit-identical from run to run", n)
        assert bool((got[n][N:] == SENTINEL).all()), ("row past N written", n)
        err = max(err, _err(got[n][:N].double().numpy(), r))
    if N >= 3:  # the absent sample: no data term, the prior alone
        g = inputs[2][N // 2]
        assert torch.equal(got["EZ"][N // 2], torch.zeros(K, dtype=dtype))
        np.testing.assert_allclose(got["sig2"][N // 2].double().numpy(), 1.0 / inputs[5][g], rtol=TOL_Z[dtype])
    return err


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("gsel", ["1", "3", "max"])
@pytest.mark.parametrize("K", KS)
def test_update_z_matches_f64_gauss_seidel(hip, K, gsel, M, dtype):
    gmax = _gmax_z(M, K)
    G = {"1": 1, "3": min(3, gmax), "max": gmax}[gsel]
    for N in SIZES:
        for with_corr in (False, True):
            err = check_update_z(hip, dtype, N, K, M, G, with_corr, seed=N * 7 + G + M)
            assert err <= TOL_Z[dtype], (N, K, M, G, with_corr, err)

