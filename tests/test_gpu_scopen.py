"""muon_amd.atac.pp.scopen on the device: the fused coordinate-descent sweep of csrc/nmf.hip against a NumPy restatement
in the stated order (tests/scopen_fixture.sweep_numpy), bit-equal repeats, the grid cap, routing, and every case of
tests/golden/scopen_golden.npz (the reference's own ``scopen`` executing over scikit-learn's coordinate descent) end to
end.

The sweep: the updated factor and the scaled copy are BIT-EQUAL to the restatement (the order and the roundings of the
k-term sum are the kernel's contract).  The two sums have derived bounds against extended precision, valid for any
order: |viol - S| <= rows k 2^-53 S with S the sum of the restatement's own terms (all >= 0), and
|gram - ref|_ab <= (rows + 16) 2^-53 (|W|^T |W|)_ab.  The padding columns of W and B hold NaN: W's must come back
untouched and nothing NaN may reach a result.

Fixture parity: equal iteration counts are a condition (the generator keeps the deciding ratios 1e-3 clear of tol).  The
value bound is the project's convention, ten times the deviation measured on an MI355X (max |delta| / max |.| over
X_scopen, varm["scopen"] and the imputed matrix, PARITY_MEASURED below and DESIGN.md 9.13), against the golden and never
against the host route."""
import numpy as np
import pytest
import torch

from tests import scopen_fixture as fx
from muon_amd import atac
from muon_amd._ffi import MuonAmdError

pytestmark = pytest.mark.gpu

# max |result - fixture| / max |fixture| measured on an MI355X, per case
PARITY_MEASURED = {
    "k6": 1.85e-15, "k6_a0": 2.86e-15, "k6_rho": 1.85e-15, "k6_iter5": 1.86e-15, "k6_dense": 1.85e-15,
    "k6_messy": 2.67e-15, "k6_mudata": 1.85e-15, "k17": 2.5e-15, "k30": 4.2e-13, "k33": 3.0e-15, "k64": 7.62e-14,
    "k65": 1.61e-13,
}
U = 2.0 ** -53

# (rows, k, ldw = ldb, max_blocks)
SHAPES = [(1, 1, 16, 0), (63, 2, 16, 0), (64, 16, 16, 0), (65, 17, 32, 0), (130, 30, 32, 0), (257, 33, 64, 0),
          (70, 64, 64, 0), (1000, 30, 32, 2)]


@pytest.fixture(scope="module")
def gold():
    return fx.load_gold()


def _operands(rows, k, ld, seed):
    """W with zeros under gradients of both signs, a G with one zero on its diagonal (k >= 2), NaN in every padding
    column of W and B."""
    rng = np.random.default_rng(seed)
    W = rng.random((rows, k))
    W[rng.random((rows, k)) < 0.35] = 0.0
    M = rng.standard_normal((k + 3, k))
    G = M.T @ M / (k + 3)
    if k >= 2:
        G[k // 2, k // 2] = 0.0
    B = rng.standard_normal((rows, k)) * 2.0
    Wp, Bp = np.full((rows, ld), np.nan), np.full((rows, ld), np.nan)
    Wp[:, :k], Bp[:, :k] = W, B
    return Wp, Bp, G, rng.uniform(0.5, 2.0, rows), rng.uniform(0.5, 2.0, rows)


def _restated(Wp, Bp, G, k, bscale, l1, oscale):
    """(W new, Wout, S, gram, |W|^T |W|): the restatement's factor, its scaled copy, and the two sums in extended
    precision."""
    W = Wp[:, :k].copy()
    b = Bp[:, :k] * bscale[:, None] if bscale is not None else Bp[:, :k].copy()
    if l1 != 0:
        b = b - l1
    terms = np.zeros(W.shape[0])
    fx.sweep_numpy(W, b, G, terms)
    assert (terms >= 0).all()
    Wl = W.astype(np.longdouble)
    out = W * oscale[:, None] if oscale is not None else W.copy()
    return W, out, terms.astype(np.longdouble).sum(), (Wl.T @ Wl), (np.abs(Wl).T @ np.abs(Wl))


def _call(hip, Wp, Bp, G, *, bscale=None, l1=0.0, oscale=None, ldo=None, max_blocks=0):
    dev = lambda a: None if a is None else hip.to_device(np.ascontiguousarray(a), np.float64)  # noqa: E731
    W, out = dev(Wp), None
    if ldo is not None:
        out = hip.to_device(np.full((Wp.shape[0], ldo), np.nan), np.float64)
    gram, viol = hip.nmf_cd_sweep(W, dev(Bp), dev(G), bscale=dev(bscale), l1=l1, oscale=dev(oscale), out=out,
                                  max_blocks=max_blocks)
    return hip.to_host(W), None if out is None else hip.to_host(out), hip.to_host(gram), float(hip.to_host(viol)[0])


def _check(got, ref, Wp, k, rows):
    W, out, gram, viol = got
    W_ref, out_ref, S, gram_ref, gram_abs = ref
    assert np.array_equal(W[:, :k], W_ref), "the updated factor is bit-equal to the restatement"
    assert np.array_equal(np.isnan(W[:, k:]), np.ones_like(W[:, k:], dtype=bool)), "W's padding is untouched"
    if out is not None:
        assert np.array_equal(out[:, :k], out_ref) and not out[:, k:].any(), "Wout bit-equal, its padding zero"
    assert np.isfinite(gram).all() and np.isfinite(viol)
    assert abs(np.longdouble(viol) - S) <= rows * k * U * S
    assert (np.abs(gram.astype(np.longdouble) - gram_ref) <= (rows + 16) * U * gram_abs).all()
    if k >= 2:
        assert np.array_equal(W[:, k // 2], Wp[:, k // 2]), "a coordinate with G[t,t] = 0 stays put"


@pytest.mark.parametrize("variant", ["scaled", "plain_l1", "no_out"])
@pytest.mark.parametrize("rows,k,ld,max_blocks", SHAPES)
def test_sweep_against_the_restatement(hip, rows, k, ld, max_blocks, variant):
    Wp, Bp, G, bs, osc = _operands(rows, k, ld, seed=rows + k)
    kw = dict(scaled=dict(bscale=bs, oscale=osc, ldo=ld), plain_l1=dict(l1=0.125, ldo=ld), no_out=dict(l1=0.0))[variant]
    ref = _restated(Wp, Bp, G, k, kw.get("bscale"), kw.get("l1", 0.0), kw.get("oscale"))
    zeros = Wp[:, :k] == 0
    if rows * k >= 100:  # the data exercise what they claim: zeros that stay and zeros that leave, entries clamped to zero
        assert (ref[0][zeros] == 0).any() and (ref[0][zeros] > 0).any() and (ref[0][~zeros] == 0).any()
    got = _call(hip, Wp, Bp, G, max_blocks=max_blocks, **kw)
    _check(got, ref, Wp, k, rows)
    again = _call(hip, Wp, Bp, G, max_blocks=max_blocks, **kw)
    for a, b in zip(got, again):
        assert a is b is None or np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), "two calls agree bit for bit"


@pytest.mark.parametrize("ldo", [17, 40])
def test_second_output_of_another_width(hip, ldo):
    rows, k, ld = 65, 17, 32
    Wp, Bp, G, bs, osc = _operands(rows, k, ld, seed=3)
    ref = _restated(Wp, Bp, G, k, bs, 0.0, osc)
    _check(_call(hip, Wp, Bp, G, bscale=bs, oscale=osc, ldo=ldo), ref, Wp, k, rows)


def test_one_block_against_the_default_grid(hip):
    rows, k, ld = 1000, 30, 32
    Wp, Bp, G, bs, osc = _operands(rows, k, ld, seed=9)
    ref = _restated(Wp, Bp, G, k, bs, 0.0, osc)
    one = _call(hip, Wp, Bp, G, bscale=bs, oscale=osc, ldo=ld, max_blocks=1)
    full = _call(hip, Wp, Bp, G, bscale=bs, oscale=osc, ldo=ld, max_blocks=0)
    _check(one, ref, Wp, k, rows)
    _check(full, ref, Wp, k, rows)
    assert np.array_equal(one[0], full[0], equal_nan=True) and np.array_equal(one[1], full[1])


def test_no_rows_and_refused_arguments(hip):
    k = 5
    G = hip.to_device(np.eye(k), np.float64)
    W = hip.zeros((0, 16), torch.float64)
    gram, viol = hip.nmf_cd_sweep(W, hip.zeros((0, 16), torch.float64), G)
    assert not hip.to_host(gram).any() and hip.to_host(viol)[0] == 0.0
    W = hip.zeros((4, 16), torch.float64)
    with pytest.raises(MuonAmdError, match="ldb must cover k"):
        hip.nmf_cd_sweep(W, hip.zeros((4, 4), torch.float64), G)
    with pytest.raises(MuonAmdError, match="ldo must cover k"):
        hip.nmf_cd_sweep(W, hip.zeros((4, 16), torch.float64), G, out=hip.zeros((4, 4), torch.float64))
    with pytest.raises(MuonAmdError, match="k must be 1..64"):
        hip.nmf_cd_sweep(hip.zeros((4, 80), torch.float64), hip.zeros((4, 80), torch.float64),
                         hip.to_device(np.eye(65), np.float64))
    assert hip.nmf_max_components() == 64


class _Counting:
    """Forwards everything to the backend and counts the calls of the named operators."""

    def __init__(self, be, *names):
        self._be, self.calls = be, {n: 0 for n in names}

    def __getattr__(self, name):
        attr = getattr(self._be, name)
        if name in self.calls and attr is not None:
            def counted(*a, **k):
                self.calls[name] += 1
                return attr(*a, **k)
            return counted
        return attr


def _rel(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max()) / float(np.abs(b).max())


@pytest.mark.parametrize("case", list(fx.CASES))
def test_fixture_case_end_to_end(hip, gold, case):
    data, adata, kw = fx.case_data(case)
    be, diag = _Counting(hip, "spmm", "nmf_cd_sweep"), {}
    atac.pp.scopen(data, backend=be, init=(gold[f"{case}_W0"], gold[f"{case}_H0"]), diagnostics=diag, **kw)
    W, H, full = gold[f"{case}_W"], gold[f"{case}_H"], fx.rebuild_imputed(gold, case)
    m = int(gold[f"{case}_n_iter"][0])
    assert diag["n_iter"] == m and len(diag["ratios"]) == len(gold[f"{case}_ratios"])
    assert np.abs(diag["rho"] - gold[f"{case}_rho"]).max() <= 1e-15
    if kw["n_components"] <= 64:
        assert diag["route"] == "kernel" and be.calls == {"spmm": 2 * m, "nmf_cd_sweep": 2 * m}
    else:
        assert diag["route"] == "tensor" and be.calls["nmf_cd_sweep"] == 0
    devs = dict(X_scopen=_rel(adata.obsm["X_scopen"], H.T), scopen=_rel(adata.varm["scopen"], W),
                imputed=_rel(adata.X, full))
    print(f"MEASURE scopen device {case}: n_iter {m} " + " ".join(f"{k} {v:.3g}" for k, v in devs.items()))
    assert max(devs.values()) <= 10 * PARITY_MEASURED[case], devs


def test_default_start_on_the_device(hip, gold):
    """init="nndsvd" end to end: three iterations from the package's own SVD against the restated loop from
    numpy.linalg.svd's triplets.  The starts differ by the f32 rounding of the SVD's operand (6e-8 relative,
    tests/test_scopen_host.py), and NNDSVD zeroes entries below 1e-6: an entry next to that threshold may fall on either
    side, a step of 1e-6.  Bound: ten such steps (measured on an MI355X: 2.4e-8)."""
    from muon_amd._atac import scopen as S

    X = fx.dense_x("k6", gold["k6_rho"])
    Un, sv, Vt = np.linalg.svd(X, full_matrices=False)
    W0, Ht0 = S._nndsvd(torch.from_numpy(Un[:, :6].copy()), torch.from_numpy(sv[:6].copy()), torch.from_numpy(Vt[:6].T.copy()))
    W, H, _n, _r = fx.cd_numpy(X, W0.numpy(), Ht0.numpy().T.copy(), l2_w=1.0, l2_h=1.0, max_iter=3)
    data, adata, kw = fx.case_data("k6")
    diag = {}
    atac.pp.scopen(data, backend=hip, max_iter=3, impute=False, diagnostics=diag, **kw)
    devs = (_rel(adata.varm["scopen"], W), _rel(adata.obsm["X_scopen"], H.T))
    print(f"MEASURE scopen device nndsvd k6 after 3 iterations: W {devs[0]:.3g} H {devs[1]:.3g}")
    assert diag["route"] == "kernel" and max(devs) <= 1e-5
