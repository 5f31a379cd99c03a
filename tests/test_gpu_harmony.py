"""muon_amd.pp.harmony_integrate on the device: the kernels of csrc/harmony.hip against their NumPy definitions, then
the whole call on the kernel route against the NumPy restatement (tests/harmony_refs.py; parity with harmonypy is not
pinned), byte-equal repeats and routing.

Bounds, derived:

  * harmony_gram.  On dyadic data (eighths, |values| small) every product and every partial sum is exact in f64, so the
    result is BIT-EQUAL to NumPy's in any order.  On general data an output element is a sum of n_s products, added
    in some order over tiles and slots: |out - ref|_ij <= (n_s + 16) 2^-53 (|R|^T |Z|)_ij against a reference summed in
    extended precision (one rounding per added term is the n_s, the + 16 is slack for the products' own roundings).
  * harmony_assign.  The operands are dyadic, so the distances D = 2 (1 - Zc . Y) are exact whatever the order of the
    matrix cores' sums; the exponent t = -D / sigma is one correctly rounded division on both sides (exact for sigma =
    0.125), t - max is exact or one rounding.  What is left per weight: libm's exp (a few ulps) and the product with
    F (one rounding), relative; the sum over K weights adds at most K roundings of a partial sum that never exceeds
    the total; the division is one more.  Every entry lies in [0, 1], so |R - ref| <= (K + 16) 2^-52 absolute, with the
    reference's exp, sum and division taken in extended precision.

  * harmony_objective.  With dyadic Zc and Y the distances are exact; each term group is a sum of N K terms, each
    computed with a few roundings (libm's log among them), added in some order: |sum - ref| <= (N K + 16) 2^-53 times
    the sum of the absolute terms, per group, against terms and sums taken in extended precision.
  * harmony_correct.  An element is Z minus a K-term sum: |Zcorr - ref| <= (K + 2) 2^-53 (|Z| + |R| |W|) element-wise;
    the rows of Zc have norm 1 to 4 ulps (a d-term sum of squares, a root and a division, all correctly rounded).

The padding of every operand holds NaN: the kernels mask by index.  Rows that a call does not name keep a sentinel."""
import collections

import numpy as np
import pandas as pd
import pytest
import torch

from tests import harmony_refs as hr
from muon_amd import AnnData, pp
from muon_amd._core import harmony as H

pytestmark = pytest.mark.gpu
LD = np.longdouble


def _padded(hip, A, extra=3):
    """A on the device as the [n, w] view of a buffer ``extra`` columns wider, everything past column w NaN."""
    n, w = A.shape
    buf = torch.full((n, w + extra), float("nan"), dtype=torch.float64, device=hip.device)
    buf[:, :w] = hip.to_device(A, np.float64)
    return buf[:, :w]


def _r_padded(hip, Rm, K):
    """R [n, K] in a buffer [n, kp + 2] whose columns from K on are NaN; the [n, kp] view."""
    n = Rm.shape[0]
    kp = (K + 15) // 16 * 16
    buf = torch.full((n, kp + 2), float("nan"), dtype=torch.float64, device=hip.device)
    buf[:, :K] = hip.to_device(Rm, np.float64)
    return buf[:, :kp]


def _segments(kind, n):
    if kind == "one":
        return [0, n]
    if kind == "empties":  # an empty first, middle and last segment, a one-row segment, segments that straddle a tile
        return sorted([0, 0, min(1, n), n // 3, n // 3, min(n // 3 + 70, n), n, n])
    raise AssertionError(kind)


GRAMS = [
    # n, K, d, segments, with an index list
    (1, 1, 1, "one", False), (63, 15, 3, "one", False), (64, 16, 4, "one", False), (65, 17, 5, "one", False),
    (200, 100, 50, "one", False), (200, 128, 64, "one", False), (200, 17, 16, "empties", False),
    (200, 100, 17, "empties", False), (65, 1, 64, "empties", False), (200, 128, 1, "empties", True),
    (63, 16, 50, "one", True), (1, 128, 64, "empties", False),
]


@pytest.mark.parametrize("n,K,d,kind,with_idx", GRAMS)
def test_gram_against_its_definition(hip, n, K, d, kind, with_idx):
    rng = np.random.default_rng(1000 * n + 10 * K + d)
    seg = _segments(kind, n)
    assert seg == sorted(seg) and seg[0] == 0 and seg[-1] == n
    rows = rng.permutation(n) if with_idx else np.arange(n)
    idx = hip.to_device(rows.astype(np.int64), np.int64) if with_idx else None
    kp, dp = (K + 15) // 16 * 16, (d + 15) // 16 * 16
    for dyadic in (True, False):
        if dyadic:
            Rm, Z = np.round(rng.standard_normal((n, K)) * 8) / 8, np.round(rng.standard_normal((n, d)) * 8) / 8
        else:
            Rm, Z = rng.random((n, K)), rng.standard_normal((n, d))
        out = hip.to_host(hip.harmony_gram(_r_padded(hip, Rm, K), _padded(hip, Z), seg, K, idx=idx))
        assert out.shape == (len(seg) - 1, kp, dp) and np.isfinite(out).all()
        assert not out[:, K:, :].any() and not out[:, :, d:].any()  # the padding is zero
        worst = 0.0
        for s in range(len(seg) - 1):
            r = rows[seg[s]:seg[s + 1]]
            ref = (Rm[r].astype(LD).T @ Z[r].astype(LD)).astype(np.float64)
            if dyadic:
                assert np.array_equal(out[s, :K, :d], ref), (s, "not bit-equal on exact data")
            else:
                mag = np.abs(Rm[r]).T @ np.abs(Z[r])
                unit = (len(r) + 16) * 2.0 ** -53
                err = np.abs(out[s, :K, :d] - ref)
                assert (err <= unit * mag).all(), (s, float((err / np.maximum(unit * mag, 1e-300)).max()))
                worst = max(worst, float((err / np.maximum(unit * mag, 1e-300)).max()) if len(r) else 0.0)
    print(f"MEASURE harmony gram n={n} K={K} d={d} {kind} idx={with_idx}: error / bound {worst:.3g}")


def test_gram_repeats_are_byte_equal_and_bad_indices_are_refused(hip):
    rng = np.random.default_rng(7)
    Rm, Z = hip.to_device(rng.random((5000, 112)), np.float64), hip.to_device(rng.standard_normal((5000, 50)), np.float64)
    seg = [0, 1200, 1200, 3100, 5000]
    a, b = hip.harmony_gram(Rm, Z, seg, 100), hip.harmony_gram(Rm, Z, seg, 100)
    assert torch.equal(a, b)
    ref = (hip.to_host(Rm)[:1200, :100].T @ hip.to_host(Z)[:1200])
    assert np.abs(hip.to_host(a)[0, :100, :50] - ref).max() <= 1e-11
    for bad in ([-1, 3], [0, 5000]):
        with pytest.raises(IndexError):
            hip.harmony_gram(Rm, Z, [0, 2], 100, idx=hip.to_device(np.asarray(bad, dtype=np.int64), np.int64))
    with pytest.raises(Exception, match="mu_harmony_gram_f64"):
        hip.harmony_gram(Rm, Z, [0, 3000, 2000, 5000], 100)


def _assign_reference(Zc, Y, sigma, F, codes):
    D = 2 * (1 - Zc @ Y.T)
    assert np.array_equal(D, (2 * (1 - Zc.astype(LD) @ Y.T.astype(LD))).astype(np.float64))  # the distances are exact
    T = -D / sigma  # (one correctly rounded division, as on the device)
    Tl = T.astype(LD)
    W = np.exp(Tl - Tl.max(axis=1, keepdims=True)) * F[:, codes].T.astype(LD)
    return (W / W.sum(axis=1, keepdims=True)).astype(np.float64)


ASSIGNS = [
    # n, nb, K, d, B, sigma, F ("one" or "wide"), scale of the operands
    (70, 0, 16, 5, 2, 0.125, "one", 1), (70, 1, 1, 3, 1, 0.125, "wide", 1), (70, 15, 16, 4, 2, 0.125, "one", 1),
    (70, 16, 17, 5, 2, 0.125, "wide", 1), (70, 17, 100, 50, 64, 0.125, "wide", 1), (70, 63, 100, 17, 2, 0.125, "one", 1),
    (70, 65, 17, 64, 64, 0.125, "wide", 1), (300, 65, 100, 16, 2, 0.01, "wide", 8), (70, 70, 16, 1, 1, 0.125, "one", 1),
    (70, 65, 1, 50, 2, 0.01, "wide", 8), (200, 200, 128, 64, 2, 0.125, "wide", 1),
]


@pytest.mark.parametrize("n,nb,K,d,B,sigma,fkind,scale", ASSIGNS)
def test_assign_against_its_definition(hip, n, nb, K, d, B, sigma, fkind, scale):
    rng = np.random.default_rng(100 * n + nb + K + d)
    Zc = np.round(rng.standard_normal((n, d)) * 8 * scale / np.sqrt(d)) / 8
    Y = np.round(rng.standard_normal((K, d)) * 8 * scale / np.sqrt(d)) / 8
    sig = np.full(K, sigma)
    F = np.ones((K, B)) if fkind == "one" else 10.0 ** rng.uniform(-6, 6, size=(K, B))
    codes = rng.integers(B, size=n)
    block = np.sort(rng.permutation(n)[:nb])
    if B == 2 and nb >= 15:
        codes[block] = 0  # level 1 has no cell in the block ...
        if nb >= 17:
            codes[block[-1]] = 1  # ... or exactly one
    all_rows = nb == n
    idx = None if all_rows else hip.to_device(block.astype(np.int64), np.int64)
    kp = (K + 15) // 16 * 16
    Rd = torch.full((n, kp + 2), 7.5, dtype=torch.float64, device=hip.device)
    hip.harmony_assign(_padded(hip, Zc), hip.to_device(Y, np.float64), hip.to_device(sig, np.float64),
                       hip.to_device(F, np.float64), hip.to_device(codes.astype(np.int32), np.int32), Rd[:, :kp], idx=idx)
    out = hip.to_host(Rd)
    others = np.setdiff1d(np.arange(n), block)
    assert (out[others] == 7.5).all() and (out[:, kp:] == 7.5).all()  # rows outside the block keep the sentinel
    assert not out[block, K:kp].any()  # the padding columns are written zero
    if nb == 0:
        return
    ref = _assign_reference(Zc[block], Y, sig, F, codes[block])
    got = out[block, :K]
    err = np.abs(got - ref).max()
    print(f"MEASURE harmony assign n={n} nb={nb} K={K} d={d} B={B} sigma={sigma} F={fkind}: "
          f"error / bound {err / ((K + 16) * 2.0 ** -52):.3g}")
    assert np.isfinite(got).all() and err <= (K + 16) * 2.0 ** -52
    if K == 1:
        assert (got == 1.0).all()  # exactly
    if sigma == 0.01:
        assert K == 1 or ((got > 0).sum(axis=1) == 1).any()  # all but one weight underflow


def test_assign_repeats_are_byte_equal_and_bad_indices_are_refused(hip):
    rng = np.random.default_rng(11)
    n, K, d, B = 3000, 100, 50, 4
    Zc = rng.standard_normal((n, d))
    Zc /= np.sqrt((Zc * Zc).sum(1, keepdims=True))
    Y = Zc[rng.permutation(n)[:K]].copy()
    args = (hip.to_device(Zc, np.float64), hip.to_device(Y, np.float64), hip.to_device(np.full(K, 0.1), np.float64),
            hip.to_device(rng.uniform(0.5, 2, size=(K, B)), np.float64),
            hip.to_device(rng.integers(B, size=n).astype(np.int32), np.int32))
    a, b = (torch.zeros((n, 112), dtype=torch.float64, device=hip.device) for _ in range(2))
    hip.harmony_assign(*args, a)
    hip.harmony_assign(*args, b)
    assert torch.equal(a, b) and bool((a[:, :100].sum(dim=1) - 1).abs().max() < 1e-14)
    for bad in ([-1], [n]):
        with pytest.raises(IndexError):
            hip.harmony_assign(*args, a, idx=hip.to_device(np.asarray(bad, dtype=np.int64), np.int64))


OBJECTIVES = [(1, 1, 1, 1), (17, 16, 4, 2), (65, 17, 5, 3), (200, 100, 50, 4), (130, 128, 64, 64), (63, 15, 17, 2)]


@pytest.mark.parametrize("n,K,d,B", OBJECTIVES)
def test_objective_against_its_definition(hip, n, K, d, B):
    rng = np.random.default_rng(n + K + d + B)
    Zc = np.round(rng.standard_normal((n, d)) * 8 / np.sqrt(d)) / 8
    Y = np.round(rng.standard_normal((K, d)) * 8 / np.sqrt(d)) / 8
    Rm = rng.random((n, K))
    Rm[rng.random((n, K)) < 0.2] = 0.0  # exact zeros: 0 log 0 = 0
    sig = rng.uniform(0.05, 0.2, size=K)
    G = rng.standard_normal((K, B))
    codes = rng.integers(B, size=n)
    out = hip.to_host(hip.harmony_objective(_padded(hip, Zc), hip.to_device(Y, np.float64), _r_padded(hip, Rm, K),
                                            hip.to_device(sig, np.float64), hip.to_device(G, np.float64),
                                            hip.to_device(codes.astype(np.int32), np.int32)))
    D = 2 * (1 - Zc @ Y.T)
    assert np.array_equal(D, (2 * (1 - Zc.astype(LD) @ Y.T.astype(LD))).astype(np.float64))
    Rl, sl = Rm.astype(LD), sig.astype(LD)
    terms = [Rl * D.astype(LD), sl * (Rl * np.log(np.where(Rl > 0, Rl, 1))), sl * (Rl * G[:, codes].T.astype(LD))]
    unit = (n * K + 16) * 2.0 ** -53
    ratios = []
    for got, t in zip(out, terms):
        ref, mag = float(t.sum()), float(np.abs(t).sum())
        assert np.isfinite(got) and abs(got - ref) <= unit * mag
        ratios.append(abs(got - ref) / (unit * mag) if mag else 0.0)
    print(f"MEASURE harmony objective n={n} K={K} d={d} B={B}: error / bound {max(ratios):.3g}")


CORRECTS = [(1, 1, 1, 1), (17, 16, 4, 2), (65, 17, 5, 3), (200, 100, 50, 4), (130, 128, 64, 64), (63, 15, 17, 2)]


@pytest.mark.parametrize("n,K,d,B", CORRECTS)
def test_correct_against_its_definition(hip, n, K, d, B):
    rng = np.random.default_rng(7 * n + K + d + B)
    Z, Rm, W = rng.standard_normal((n, d)) * 3, rng.random((n, K)), rng.standard_normal((B, K, d))
    codes = np.sort(rng.integers(B, size=n))  # sorted by level; with B = 64 most levels are empty or hold one cell
    seg = np.searchsorted(codes, np.arange(B + 1))
    Zcorr, Zc = hip.harmony_correct(_padded(hip, Z), _r_padded(hip, Rm, K), hip.to_device(W, np.float64), seg)
    Zcorr, Zc = hip.to_host(Zcorr), hip.to_host(Zc)
    ref = Z.astype(LD) - np.einsum("ik,ikd->id", Rm.astype(LD), W[codes].astype(LD))
    mag = np.abs(Z) + np.einsum("ik,ikd->id", Rm, np.abs(W[codes]))
    unit = (K + 2) * 2.0 ** -53
    err = np.abs(Zcorr - ref.astype(np.float64))
    norms = np.sqrt((Zc.astype(LD) ** 2).sum(axis=1))
    print(f"MEASURE harmony correct n={n} K={K} d={d} B={B}: error / bound {float((err / (unit * mag)).max()):.3g}, "
          f"|norm - 1| {float(np.abs(norms - 1).max() / 2.0 ** -52):.3g} ulps")
    assert Zcorr.shape == Zc.shape == (n, d) and np.isfinite(Zcorr).all() and (err <= unit * mag).all()
    assert float(np.abs(norms - 1).max()) <= 4 * 2.0 ** -52
    assert np.abs(Zc * np.sqrt((Zcorr ** 2).sum(1, keepdims=True)) - Zcorr).max() <= 1e-14 * np.abs(Zcorr).max()


def test_objective_and_correct_repeat_byte_equal(hip):
    rng = np.random.default_rng(13)
    n, K, d, B = 3000, 100, 50, 4
    Z = hip.to_device(rng.standard_normal((n, d)), np.float64)
    Zc = Z / torch.sqrt((Z * Z).sum(dim=1, keepdim=True))
    Rm = hip.to_device(rng.random((n, 112)), np.float64)
    codes = np.sort(rng.integers(B, size=n))
    args = (Zc, Zc[:K].contiguous(), Rm, hip.to_device(np.full(K, 0.1), np.float64),
            hip.to_device(rng.standard_normal((K, B)), np.float64), hip.to_device(codes.astype(np.int32), np.int32))
    assert torch.equal(hip.harmony_objective(*args), hip.harmony_objective(*args))
    W = hip.to_device(rng.standard_normal((B, K, d)), np.float64)
    seg = np.searchsorted(codes, np.arange(B + 1))
    a, b = hip.harmony_correct(Z, Rm, W, seg), hip.harmony_correct(Z, Rm, W, seg)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(Exception, match="mu_harmony_correct_f64"):
        hip.harmony_correct(Z, Rm, W, [0, 10, 5, 20, n])


# ---- the whole call --------------------------------------------------------------------------------------------------------
class _Counting:
    """Forwards to a backend and counts the calls of its harmony operators."""

    def __init__(self, be):
        self._be, self.calls = be, collections.Counter()

    def __getattr__(self, name):
        attr = getattr(self._be, name)
        if name in ("harmony_gram", "harmony_assign", "harmony_objective", "harmony_correct"):
            def counted(*a, **kw):
                self.calls[name] += 1
                return attr(*a, **kw)
            return counted
        return attr


@pytest.mark.parametrize("name", sorted(hr.CASES))
def test_end_to_end_against_the_restatement(hip, name):
    Z, codes, _, _ = hr.case(name)
    be = _Counting(hip)
    res = H._harmonize(be, Z, [codes], [hr.CASES[name][3]], nclust=hr.CASES[name][4])
    assert res["route"] == "kernel" and be.calls["harmony_assign"] > 20 and be.calls["harmony_gram"] > 40
    assert be.calls["harmony_objective"] == sum(res["kmeans_rounds"]) + 1 and be.calls["harmony_correct"] == res["n_iter"]
    hr.check_case(name, res, "device")


def test_repeated_calls_are_byte_equal_and_the_tensor_route_agrees(hip):
    Z, codes, ref, own = hr.case("n300")
    a = H._harmonize(hip, Z, [codes], [2], nclust=10)
    b = H._harmonize(hip, Z, [codes], [2], nclust=10)
    assert a["Z_corr"].tobytes() == b["Z_corr"].tobytes() and a["R"].tobytes() == b["R"].tobytes()
    t = H._harmonize(hip, Z, [codes], [2], nclust=10, force_tensor=True)
    assert t["route"] == "tensor" and t["kmeans_rounds"] == ref["kmeans_rounds"]
    assert hr.deviation(t["Z_corr"], ref["Z_corr"]) <= 100 * own


def test_two_keys_and_65_levels_take_the_tensor_route(hip):
    be = _Counting(hip)
    Z, codes, ref, own = hr.levels65()
    res = H._harmonize(be, Z, [codes], [65], nclust=8, max_iter_harmony=2)
    assert res["route"] == "tensor" and res["kmeans_rounds"] == ref["kmeans_rounds"]
    assert hr.deviation(res["Z_corr"], ref["Z_corr"]) <= 100 * own
    Z, _, batch = hr.planted(600, 8, 3, 2)
    donor = np.random.default_rng(5).integers(3, size=600)
    kw = dict(sigma=0.1, nclust=12, max_iter_harmony=2)
    Phi = hr.one_hot([batch, donor], [2, 3])
    ref = hr.harmony_ref(Z, Phi, theta=2.0, lamb=1.0, **kw)
    ext = hr.harmony_ref(Z, Phi, theta=2.0, lamb=1.0, dtype=np.longdouble, **kw)
    res = H._harmonize(be, Z, [batch, donor], [2, 3], **kw)
    assert res["route"] == "tensor" and res["kmeans_rounds"] == ref["kmeans_rounds"] == ext["kmeans_rounds"]
    assert hr.deviation(res["Z_corr"], ref["Z_corr"]) <= 100 * hr.deviation(ext["Z_corr"], ref["Z_corr"])
    assert not be.calls  # no kernel ran


def test_arguments_on_the_kernel_route(hip):
    """theta = 0 leaves the R of a plain soft k-means; theta, lamb as lists, tau and a sigma vector run and equal the
    restatement; an f32 basis comes back as f32 within one f32 epsilon of the f64 answer; pp.knn runs on the result"""
    Z, codes, _, _ = hr.case("n300")
    res = H._harmonize(hip, Z, [codes], [2], theta=0.0, nclust=10, max_iter_harmony=1)
    Zc = Z / np.sqrt((Z * Z).sum(1, keepdims=True))
    T = -(2 * (1 - Zc @ res["Y"].T)) / 0.1
    S = np.exp(T - T.max(1, keepdims=True))
    assert res["route"] == "kernel" and np.abs(res["R"] - S / S.sum(1, keepdims=True)).max() <= 26 * 2.0 ** -52

    sig = np.linspace(0.08, 0.15, 10)
    kw = dict(sigma=sig, nclust=10, tau=5, max_iter_harmony=2)
    ref = hr.harmony_ref(Z, hr.one_hot([codes], [2]), theta=np.repeat(1.5, 2), lamb=np.repeat(0.5, 2), **kw)
    res = H._harmonize(hip, Z, [codes], [2], theta=[1.5], lamb=[0.5], **kw)
    assert res["route"] == "kernel" and res["kmeans_rounds"] == ref["kmeans_rounds"]
    assert hr.deviation(res["Z_corr"], ref["Z_corr"]) < 1e-10

    obs = pd.DataFrame({"batch": codes})
    Z32 = Z.astype(np.float32)
    a64 = AnnData(np.zeros((300, 1)), obs=obs.copy(), obsm={"X_pca": Z32.astype(np.float64)})
    a32 = AnnData(np.zeros((300, 1)), obs=obs.copy(), obsm={"X_pca": Z32.copy()})
    assert pp.harmony_integrate(a64, "batch", nclust=10, backend=hip) is None
    info = pp.harmony_integrate(a32, "batch", nclust=10, backend=hip, return_info=True)
    out, want = a32.obsm["X_pca_harmony"], a64.obsm["X_pca_harmony"]
    assert out.dtype == np.float32 and info["nclust"] == 10 and info["n_iter"] == len(info["kmeans_rounds"])
    assert np.abs(out - want).max() <= 2.0 ** -23 * np.abs(want).max()
    pp.knn(a64, n_neighbors=15, use_rep="X_pca_harmony", backend=hip)
    assert a64.obsp["distances"].shape == (300, 300)
