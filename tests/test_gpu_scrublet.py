"""csrc/scrublet.hip on the GPU: the pair merge byte for byte against the restatement of tests/scrublet_refs.py on
parent rows built around the wave's 64 lanes, the wide merge against a stable two-key sort around its limits, the search
stage of pp.scrublet through the wide merge against brute force, and pp.scrublet end to end on the resident copy."""
import numpy as np
import pytest
import torch

import muon_amd as mu
from muon_amd import _ffi
from muon_amd._backend import DeviceCSR
from muon_amd._core import scrublet as S
from muon_amd._hostmatrix import resident
from tests import scrublet_refs as R
from tests.cpu_backend import CpuTestBackend

pytestmark = pytest.mark.gpu

# A launch of the pair kernels has at most 256 CUs x 16 workgroups x 4 waves = 16 384 waves (wave_grid in
# csrc/scrublet.hip): with N_STRIDE simulated rows every wave walks its row loop at least twice
N_STRIDE = 2 * 16384 + 5


def _device_csr(hip, E):
    return DeviceCSR(hip.to_device(E.indptr, np.int64), hip.to_device(E.indices, E.indices.dtype),
                     hip.to_device(E.data, np.float32), E.shape)


def _same_bytes(hip, got, want):
    assert np.array_equal(hip.to_host(got.indptr), want[0])
    assert hip.to_host(got.indices).tobytes() == want[1].tobytes()
    assert hip.to_host(got.values).tobytes() == want[2].tobytes()


# ---- the pair merge ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index_dtype", ["int32", "int64"])
def test_pair_merge_is_the_restatement_byte_for_byte_and_repeats(hip, index_dtype):
    """lengths 0, 1, 63, 64, 65, 129, 520 in every pairing: disjoint, identical, nested, interleaved, all matches in
    the last 64-entry step (and, in the reversed pair, in the first: the carried prefix count), explicit zeros"""
    E, parents = R.pair_case(index_dtype)
    assert set(R.PAIR_LENGTHS) <= set(np.diff(E.indptr).tolist())
    want = R.simulate(E, parents)
    X, p = _device_csr(hip, E), hip.to_device(parents, np.int64)
    got = hip.csr_pair_rows(X, p)
    assert got.indices.dtype == X.indices.dtype and got.shape == (len(parents), E.shape[1])
    _same_bytes(hip, got, want)
    _same_bytes(hip, hip.csr_pair_rows(X, p), want)
    _same_bytes(hip, S.pair_rows_tensor(X, p), want)  # the tensor formulation on the device: the same bytes


def test_pair_merge_with_more_rows_than_a_launch_has_waves(hip):
    E, _ = R.pair_case("int32")
    rng = np.random.default_rng(2)
    short = np.flatnonzero(np.diff(E.indptr) <= 65)
    parents = rng.choice(short, size=(N_STRIDE, 2)).astype(np.int64)
    assert parents.shape[0] == 32773
    _same_bytes(hip, hip.csr_pair_rows(_device_csr(hip, E), hip.to_device(parents, np.int64)), R.simulate(E, parents))


def test_pair_merge_refuses_other_types_and_takes_no_rows(hip):
    E, parents = R.pair_case("int32")
    X = _device_csr(hip, E)
    with pytest.raises(TypeError):
        hip.csr_pair_rows(X.with_values(X.values.double()), hip.to_device(parents, np.int64))
    with pytest.raises(TypeError):
        hip.csr_pair_rows(X, hip.to_device(parents, np.int64).int())
    got = hip.csr_pair_rows(X, hip.to_device(parents[:0], np.int64))
    assert got.shape == (0, E.shape[1]) and got.nnz == 0 and hip.to_host(got.indptr).tolist() == [0]
    # a parent outside the matrix: an empty row, nothing read
    bad = np.array([[0, E.shape[0]], [-1, 3], [5, 6]], dtype=np.int64)
    got = hip.csr_pair_rows(X, hip.to_device(bad, np.int64))
    want = R.simulate(E, bad[2:])
    assert hip.to_host(got.indptr).tolist() == [0, 0, 0, int(want[0][-1])]
    assert hip.to_host(got.values).tobytes() == want[2].tobytes()


# ---- the wide merge ---------------------------------------------------------------------------------------------------------------
_N_Q = 9


def _merge_case(total, kc, kind, seed):
    """list [kc] ++ buffer [cap = total - kc] of _N_Q queries; cnt cycles through 0, cap, cap + 1 (overflowed) and
    values between"""
    rng = np.random.default_rng(seed)
    cap = total - kc
    pos = np.stack([rng.permutation(1 << 20)[:total] for _ in range(_N_Q)])
    if kind == "equal":
        d = np.full((_N_Q, total), 2.5)
    else:
        d = rng.integers(0, max(4, total // 3), size=(_N_Q, total)).astype(np.float64) / 8.0  # many exact ties
        if kind == "inf":
            d[rng.random(d.shape) < 0.3] = np.inf
    cur_d, cur_p = d[:, :kc].copy(), pos[:, :kc].astype(np.int64)
    buf_d, buf_pos = d[:, kc:].copy(), pos[:, kc:].astype(np.int32)
    cnt = np.array([0, cap, cap + 1, cap // 2, 1, cap, cap + 1000, 0, cap - 1][:_N_Q], dtype=np.int32)
    return cur_d, cur_p, buf_d, buf_pos, cnt


def _run_merge(hip, fn, case):
    dev = [hip.to_device(a, a.dtype) for a in case]
    out = fn(*dev)
    assert hip.to_host(dev[4]).tobytes() == case[4].tobytes()  # the caller's count is left as it is
    return [hip.to_host(t) for t in out]


@pytest.mark.parametrize("kind", ["ties", "equal", "inf"])
@pytest.mark.parametrize("total", [1025, 2048, 4097, 8192])
def test_wide_merge_against_a_stable_two_key_sort(hip, total, kind):
    for kc in (1, total // 5, total - 1):
        case = _merge_case(total, kc, kind, seed=total + kc)
        want = R.merge_reference(*case)
        got = _run_merge(hip, hip.knn_merge_wide, case)
        for g, w in zip(got, want):
            assert g.tobytes() == w.tobytes(), (total, kc, kind)


@pytest.mark.parametrize("kc", [1, 241, 1023])
def test_both_merges_return_identical_arrays_where_both_take_the_shape(hip, kc):
    for kind in ("ties", "inf"):
        case = _merge_case(1024, kc, kind, seed=kc)
        a, b = _run_merge(hip, hip.knn_merge, case), _run_merge(hip, hip.knn_merge_wide, case)
        for x, y, w in zip(a, b, R.merge_reference(*case)):
            assert x.tobytes() == y.tobytes() == w.tobytes()
    small = _merge_case(40, 8, "ties", seed=1)  # (below one wave's width)
    for x, y in zip(_run_merge(hip, hip.knn_merge, small), _run_merge(hip, hip.knn_merge_wide, small)):
        assert x.tobytes() == y.tobytes()


def test_wide_merge_refuses_8193_pairs(hip):
    assert hip.knn_merge_wide_max() == 8192
    case = _merge_case(8193, 100, "ties", seed=0)
    with pytest.raises(_ffi.MuonAmdError, match="8192"):
        hip.knn_merge_wide(*[hip.to_device(a, a.dtype) for a in case])


# ---- the search stage ---------------------------------------------------------------------------------------------------------------
class _Counting:
    """the backend with its merge calls counted"""

    def __init__(self, be):
        self._be = be
        self.calls = {"knn_merge": 0, "knn_merge_wide": 0}

    def __getattr__(self, name):
        f = getattr(self._be, name)
        if name in self.calls:
            def counted(*a):
                self.calls[name] += 1
                return f(*a)
            return counted
        return f


@pytest.fixture(scope="module")
def search_case():
    """3000 observed + 6000 simulated rows, n_neighbors = 90: k_adj = 270, kc + cap = 278 + 898 = 1176 - the smallest
    size the filter path accepts (n >= 8192) with a list and buffer past the wave-wide merge"""
    rng = np.random.default_rng(7)
    Zo = rng.standard_normal((3000, 10)) + 3.0 * rng.integers(0, 3, (3000, 1))
    Zs = rng.standard_normal((6000, 10)) + 3.0 * rng.random((6000, 1)) * 2
    k_adj = R.adjusted_k(3000, 6000, 90)
    assert k_adj == 270
    want, gap = R.sim_neighbours_by_partition(Zo, Zs, k_adj)
    return Zo, Zs, k_adj, want, gap >= 1e-9


def test_search_stage_through_the_wide_merge(hip, search_case):
    Zo, Zs, k_adj, want, keep = search_case
    assert keep.mean() >= 0.99
    proxy = _Counting(hip)
    res = S.scrublet_scores_device(proxy, hip.to_device(Zo, np.float64), hip.to_device(Zs, np.float64), k_adj)
    assert res["route"] == "filtered" and proxy.calls["knn_merge_wide"] >= 1 and proxy.calls["knn_merge"] == 0
    assert np.array_equal(res["n_sim_neigh"][keep], want[keep])
    Ld, se = R.scores(want[keep][:200], k_adj, 2.0)
    np.testing.assert_allclose(res["scores"][keep][:200], Ld, rtol=1e-12, atol=0)
    # blocks of queries (a budget that holds about a third of them): the same counts
    blocks = _Counting(hip)
    per_query = (3 * 278 + 64) * 12 + 2 * 278 * 16
    again = S.scrublet_scores_device(blocks, hip.to_device(Zo, np.float64), hip.to_device(Zs, np.float64), k_adj,
                                     buffer_budget=3100 * per_query)
    assert blocks.calls["knn_merge_wide"] == 3 * proxy.calls["knn_merge_wide"]
    assert np.array_equal(again["n_sim_neigh"], res["n_sim_neigh"])


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
# No margin can be derived for what a different eigensolver does to the result, so it was measured: the
# restatement with its own dense SVD against the restatement with pca_host (ARPACK, f64), on planted_doublets(seed = 11 +
# s) with random_state = s and solver_seed = s for s = 0 .. 4.  Largest share of cells whose predicted_doublet differs: 0.
# Largest |delta doublet_score|: 0.  (Both f64 solvers give every one of the 5 x 4950 rows the same neighbour count.)  The
# device route gets twice that spread against the restatement: 0 and 0.
SPREAD_CALLS, SPREAD_SCORE = 0.0, 0.0


def measure_solver_spread(seeds=range(5)):
    """The measurement behind SPREAD_CALLS and SPREAD_SCORE (CPU only, about a minute; not run by the suite)."""
    calls = score = 0.0
    for s in seeds:
        X, _ = R.planted_doublets(seed=11 + s)
        a = R.scrublet(X, random_state=s, solver="svd")
        b = R.scrublet(X, random_state=s, solver="pca_host", solver_seed=s)
        calls = max(calls, float((a["predicted_doublet"] != b["predicted_doublet"]).mean()))
        score = max(score, float(np.abs(a["doublet_score"] - b["doublet_score"]).max()))
    return calls, score


def test_end_to_end_on_planted_doublets(hip):
    """Three planted clusters and 10 % true heterotypic doublets (tests/scrublet_refs.planted_doublets).  Both routes find
    a threshold, the true doublets score higher than the singlets on both, and the device route stays within twice the
    measured solver spread of the restatement (the figures above: 0 cells, 0 in the score).  Measured on the MI355X:
    device route 0 cells and 0 in the score, threshold 0.16417 as restated; the CPU route (the f32 Lanczos process
    through CpuTestBackend) differs in one score by one neighbour, 0.0058 - it is not held to the bound."""
    X, is_dbl = R.planted_doublets()
    ref = R.scrublet(X)
    dev, cpu = mu.AnnData(X.copy()), mu.AnnData(X.copy())
    mu.pp.scrublet(dev, backend=hip)
    mu.pp.scrublet(cpu, backend=CpuTestBackend())
    assert "threshold" in ref
    for name, ad in (("device", dev), ("cpu", cpu)):
        score = ad.obs["doublet_score"].values
        print(name, "threshold", ad.uns["scrublet"].get("threshold"), "restated", ref["threshold"],
              "share of calls that differ", float((ad.obs["predicted_doublet"].values != ref["predicted_doublet"]).mean())
              if "predicted_doublet" in ad.obs.columns else None,
              "largest |delta score|", float(np.abs(score - ref["doublet_score"]).max()),
              "rows whose score differs", int((score != ref["doublet_score"]).sum()),
              "mean score of doublets / singlets", float(score[is_dbl].mean()), float(score[~is_dbl].mean()))
    for ad in (dev, cpu):
        assert "threshold" in ad.uns["scrublet"] and "predicted_doublet" in ad.obs.columns
        score = ad.obs["doublet_score"].values
        assert score[is_dbl].mean() > score[~is_dbl].mean()
    assert np.array_equal(dev.uns["scrublet"]["doublet_parents"], ref["doublet_parents"])
    assert (dev.obs["predicted_doublet"].values != ref["predicted_doublet"]).mean() <= 2 * SPREAD_CALLS
    assert np.abs(dev.obs["doublet_score"].values - ref["doublet_score"]).max() <= 2 * SPREAD_SCORE


def test_the_filtered_matrix_keeps_its_device_copy():
    """scrublet -> filter_obs on predicted_doublet -> normalize_total: one upload"""
    from muon_amd._backend import get_backend

    be = get_backend()
    X, _ = R.planted_doublets()
    ad = mu.AnnData(X.copy())
    uploads = []
    orig = be.upload_csr
    be.upload_csr = lambda *a, **k: (uploads.append(1), orig(*a, **k))[1]
    try:
        mu.pp.scrublet(ad, threshold=0.2)
        assert len(uploads) == 1 and resident(ad.X, be) is not None
        assert ad.X.data.tobytes() == X.data.tobytes()
        called = ad.obs["predicted_doublet"].values.copy()
        assert 0 < called.sum() < called.size
        mu.pp.filter_obs(ad, "predicted_doublet", lambda x: ~x)
        want = X[~called]
        Rc = resident(ad.X, be)
        assert Rc is not None and Rc.shape == want.shape
        assert np.array_equal(be.to_host(Rc.indptr), want.indptr) and np.array_equal(be.to_host(Rc.indices), want.indices)
        assert be.to_host(Rc.values).tobytes() == want.data.tobytes()
        mu.rna.pp.normalize_total(ad)
        assert len(uploads) == 1 and resident(ad.X, be) is not None
    finally:
        be.upload_csr = orig
