"""TEST INFRASTRUCTURE: plain references and edge-shape inputs for the neighbour-search and WNN kernels
(csrc/knn.hip: k_knn_filter, k_knn_merge; csrc/wnn.hip: k_wnn_bandwidth, k_umap_strengths).

Every reference here is numpy / python sets / scipy in f64 and shares no code with muon_amd.  The checks take a
backend: tests/test_gpu_knn_edges.py hands them HipBackend (the kernels), tests/test_wnn.py hands them the CPU
operator set and ``_FilterEmulation`` (the tensor paths), so the references themselves are checked on a machine
without a GPU.  References are computed once per input (``lru_cache``) and handed out read-only."""
from concurrent.futures import ThreadPoolExecutor
from functools import lru_cache

import numpy as np
import scipy.sparse as sp
import torch
from scipy.spatial.distance import cdist

from muon_amd._core import preproc as pp
from muon_amd._operators import has
from oracle import wnn_oracle


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays if len(arrays) > 1 else arrays[0]


def lattice(rng, n, p):
    """integer coordinates, uniform in [-8, 8], as f64: squared norms, dot products and |c|^2 - 2 q.c are exact in
    f64 in any summation order (all below 2^53 by a wide margin), so distances can be compared bit for bit"""
    return rng.integers(-8, 9, (n, p)).astype(np.float64)


class CountingBackend:
    """A backend with its filter and merge calls counted, and the panels whose buffers overflowed."""

    def __init__(self, be):
        self._be = be
        self.calls = {"knn_filter": 0, "knn_merge": 0}
        self.overflowed_panels = 0

    def __getattr__(self, name):
        f = getattr(self._be, name)  # (AttributeError where the backend lacks it: `has` answers as for the backend)
        if name == "knn_merge" and f is not None:  # (None: declared, not implemented by this backend)
            def counted(*a):
                self.calls[name] += 1
                return f(*a)
            return counted
        return f

    def knn_filter(self, Xq, Xc, sqq, sqc, thr, self_pos, c_lo, c_hi, buf_pos, buf_d, cnt):
        self.calls["knn_filter"] += 1
        self._be.knn_filter(Xq, Xc, sqq, sqc, thr, self_pos, c_lo, c_hi, buf_pos, buf_d, cnt)
        self.overflowed_panels += int(bool((cnt > buf_pos.shape[1]).any()))


# ---- 1. knn_filter against exact integer arithmetic --------------------------------------------------------------
FILTER_P_PADS = (4, 12, 60, 64, 132, 156)
FILTER_N_Q = (1, 63, 64, 65, 200)
FILTER_PANELS = ((0, 0), (5, 5), (0, 1), (7, 70), (64, 128), (1, 66), (130, 300))
FILTER_CAPS = (1, 8, 64)
FILTER_N_CAND = 300
_DUPS = (0, 65, 131, 299)  # candidate positions that repeat query 0: one inside every non-empty panel
_UNTOUCHED_POS, _UNTOUCHED_D, _UNTOUCHED_CNT = -1, -7.0, 77


def filter_inputs(p_pad, square, n_q, seed):
    """(Xq, Xc, self_pos, D): lattice operands and their exact squared distances [n_q, 300] (int64 arithmetic).
    ``square``: the queries ARE the first n_q candidates and self_pos is real; else 300 candidates of their own and
    self_pos = -1.  Query 0 is repeated at other candidate positions (distance 0, not the query itself)."""
    rng = np.random.default_rng(seed)
    Xc = lattice(rng, FILTER_N_CAND, p_pad)
    if square:
        Xc[[d for d in _DUPS if d]] = Xc[0]
        Xq, self_pos = Xc[:n_q], np.arange(n_q, dtype=np.int32)
    else:
        Xq = lattice(rng, n_q, p_pad)
        Xc[list(_DUPS)] = Xq[0]
        self_pos = np.full(n_q, -1, dtype=np.int32)
    qi, ci = Xq.astype(np.int64), Xc.astype(np.int64)
    D = (qi * qi).sum(axis=1)[:, None] + (ci * ci).sum(axis=1)[None, :] - 2 * (qi @ ci.T)
    assert D.min() >= 0 and (not square or not np.diag(D[:, :n_q]).any())
    return Xq, Xc, self_pos, D.astype(np.float64)


def filter_thresholds(rng, D, self_pos, c_lo, c_hi, rot):
    """per row one of: +inf, -1, an integer that IS one of the row's distances (inside the panel where it has
    one: the tie is real), that integer + 0.5; the four kinds rotate over the rows and with ``rot``"""
    n_q = D.shape[0]
    kind = (np.arange(n_q) + rot) % 4
    thr = np.where(kind == 0, np.inf, -1.0)
    for i in np.nonzero(kind >= 2)[0]:
        js = np.arange(c_lo, c_hi)
        js = js[js != self_pos[i]]
        if not js.size:  # (an empty panel, or one that holds the query alone)
            js = np.arange(D.shape[1])[np.arange(D.shape[1]) != self_pos[i]]
        thr[i] = D[i, js[rng.integers(js.size)]] + (0.5 if kind[i] == 3 else 0.0)
    return thr, kind


def check_filter(be, p_pad, square, n_qs=FILTER_N_Q, panels=FILTER_PANELS, caps=FILTER_CAPS):
    """``be.knn_filter`` on every (n_q, panel, cap) against the exact evaluation"""
    rng = np.random.default_rng(1000 * p_pad + square)
    rot = 0
    for n_q in n_qs:
        Xq, Xc, self_pos, D = filter_inputs(p_pad, square, n_q, seed=p_pad + 7 * n_q + square)
        Xc_d = be.to_device(Xc)
        Xq_d = Xc_d if (square and n_q == FILTER_N_CAND) else Xc_d[:n_q] if square else be.to_device(Xq)
        assert Xq_d.is_contiguous() and (not square or Xq_d.data_ptr() == Xc_d.data_ptr())
        sqc_d = (Xc_d * Xc_d).sum(dim=1)
        sqq_d = (Xq_d * Xq_d).sum(dim=1)
        sp_d = be.to_device(self_pos, np.int32)
        pos = np.arange(FILTER_N_CAND)[None, :]
        for c_lo, c_hi in panels:
            for cap in caps:
                thr, kind = filter_thresholds(rng, D, self_pos, c_lo, c_hi, rot)
                rot += 1
                bp = torch.full((n_q, cap), _UNTOUCHED_POS, dtype=torch.int32, device=be.device)
                bd = torch.full((n_q, cap), _UNTOUCHED_D, dtype=torch.float64, device=be.device)
                cnt = torch.full((n_q,), _UNTOUCHED_CNT, dtype=torch.int32, device=be.device)
                be.knn_filter(Xq_d, Xc_d, sqq_d, sqc_d, be.to_device(thr), sp_d, c_lo, c_hi, bp, bd, cnt)
                bp, bd, cnt = bp.cpu().numpy(), bd.cpu().numpy(), cnt.cpu().numpy()
                tag = f"p_pad={p_pad} square={square} n_q={n_q} panel=({c_lo},{c_hi}) cap={cap}"
                ok = (D < thr[:, None]) & (pos >= c_lo) & (pos < c_hi) & (pos != self_pos[:, None])
                assert np.array_equal(cnt, ok.sum(axis=1)), tag
                inside = (self_pos >= c_lo) & (self_pos < c_hi)
                full = kind == 0  # thr = +inf: the whole panel but the query itself
                assert np.array_equal(cnt[full], ((c_hi - c_lo) - inside)[full]), tag
                assert not cnt[kind == 1].any(), tag  # thr = -1: nothing
                if c_hi == c_lo:
                    assert not cnt.any() and (bp == _UNTOUCHED_POS).all() and (bd == _UNTOUCHED_D).all(), tag
                m = np.minimum(cnt, cap)
                stored = np.arange(cap)[None, :] < m[:, None]
                # nothing is written past the count
                assert (bp[~stored] == _UNTOUCHED_POS).all() and (bd[~stored] == _UNTOUCHED_D).all(), tag
                for i in np.nonzero(m)[0]:
                    got = bp[i, :m[i]].astype(np.int64)
                    assert got.min() >= c_lo and got.max() < c_hi and ok[i, got].all(), (tag, i)
                    assert np.unique(got).size == m[i], (tag, i)
                    assert torch.equal(torch.from_numpy(bd[i, :m[i]]), torch.from_numpy(D[i, got])), (tag, i)
                    if cnt[i] <= cap:
                        assert set(got.tolist()) == set(np.nonzero(ok[i])[0].tolist()), (tag, i)
                if thr[0] > 0:  # the duplicates of query 0 pass: distance 0 at another position
                    for dpos in _DUPS:
                        if c_lo <= dpos < c_hi and dpos != self_pos[0]:
                            assert D[0, dpos] == 0 and ok[0, dpos], tag
                            assert cnt[0] > cap or dpos in bp[0, :m[0]], tag


# ---- 2. brute-force search ---------------------------------------------------------------------------------------
def clustered_rows(n, p, seed):
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, 15, n)
    return rng.standard_normal((15, p))[lab] * 1.5 + rng.standard_normal((n, p))


def brute_knn(X, k):
    """scipy's cdist and a stable argsort by (distance, index), row block by row block.  Only the entries up to a
    row's k-th smallest distance are sorted - the first k of a stable argsort of the whole row are among them, in
    the same order."""
    n = X.shape[0]

    def block(lo):
        D = cdist(X[lo:lo + 512], X)
        r = np.arange(D.shape[0])
        D[r, lo + r] = np.inf
        kth = np.partition(D, k - 1, axis=1)[:, k - 1]
        idx, dst = np.empty((D.shape[0], k), dtype=np.int64), np.empty((D.shape[0], k))
        for i in r:
            c = np.nonzero(D[i] <= kth[i])[0]  # (ascending index)
            o = c[np.argsort(D[i, c], kind="stable")[:k]]
            idx[i], dst[i] = o, D[i, o]
        return idx, dst

    with ThreadPoolExecutor(8) as ex:  # (cdist releases the interpreter lock)
        out = list(ex.map(block, range(0, n, 512)))
    return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])


def check_gate(be, p):
    """``pp.device_knn`` at n = 8192, k = 5 against the brute-force search; returns the number of filter calls"""
    n, k = 8192, 5
    X = clustered_rows(n, p, seed=p)
    want_i, want_d = brute_knn(X, k)
    proxy = CountingBackend(be)
    got_i, got_d = pp.device_knn(be.to_device(X), k, "euclidean", backend=proxy)
    assert torch.allclose(got_d.cpu(), torch.from_numpy(want_d), rtol=0, atol=1e-11)
    same = float((got_i.cpu() == torch.from_numpy(want_i)).double().mean())
    assert same >= 0.9999, same
    return proxy.calls["knn_filter"]


# ---- 3. _candidates_filtered -------------------------------------------------------------------------------------
_K_REF = 301  # neighbours kept per reference row: kc <= 300 and the one after


@lru_cache(maxsize=None)
def search_case(kind, n, p):
    """(X, idx, d): rows and, per row, the 301 nearest other rows by (squared distance from coordinate
    differences in f64, index) - brute force.  kind: "gauss" or "lattice" (massive exact ties: d is what it has
    to be, idx one of the valid choices where the 302nd distance ties)."""
    rng = np.random.default_rng(n + p)
    X = rng.standard_normal((n, p)) if kind == "gauss" else lattice(rng, n, p)
    D = cdist(X, X, metric="sqeuclidean")
    np.fill_diagonal(D, np.inf)
    idx = np.sort(np.argpartition(D, _K_REF, axis=1)[:, :_K_REF + 1], axis=1)  # the 302 smallest, by index
    idx = np.take_along_axis(idx, np.argsort(np.take_along_axis(D, idx, axis=1), axis=1, kind="stable"), axis=1)[:, :_K_REF]
    return _frozen(X, idx, np.take_along_axis(D, idx, axis=1))


def _run_candidates(be, X, kc, cap):
    Xd = be.to_device(X.copy())
    proxy = CountingBackend(be)
    got_i, got_d = pp._candidates_filtered(proxy, Xd, (Xd * Xd).sum(dim=1), kc, 1 << 26, cap=cap)
    assert got_i.shape == (X.shape[0], kc) and got_d.shape == (X.shape[0], kc)
    n_panels = 0  # the panel walk of `_candidates_filtered`: [p0, 2 p0), [2 p0, 4 p0), ...
    c = max(2048, 4 * kc)
    while c < X.shape[0]:
        n_panels, c = n_panels + 1, 2 * c
    assert proxy.calls["knn_filter"] == n_panels
    cap = cap or 3 * kc + 64
    if has(be, "knn_merge"):  # the fused merge runs exactly where list and buffer fit the kernel's LDS
        assert proxy.calls["knn_merge"] == (n_panels if kc + cap <= 1024 else 0)
    return got_i.cpu().numpy(), got_d.cpu().numpy(), proxy


def check_candidates_separated(be, n, p, kc, cap=None):
    """Gaussian rows: identical neighbour SETS (the reference's kc-th and (kc+1)-th distances are 1e-9 apart, the
    two evaluation orders 1e-13), distances to 1e-11"""
    X, ref_i, ref_d = search_case("gauss", n, p)
    assert (ref_d[:, kc] - ref_d[:, kc - 1]).min() > 1e-9  # (a condition on the input)
    got_i, got_d, proxy = _run_candidates(be, X, kc, cap)
    assert np.array_equal(np.sort(got_i, axis=1), np.sort(ref_i[:, :kc], axis=1))
    np.testing.assert_allclose(np.sort(got_d, axis=1), ref_d[:, :kc], rtol=0, atol=1e-11)
    return proxy


def check_candidates_tied(be, n=4500, kc=5, cap=3):
    """lattice rows in three dimensions (about as many rows as lattice points: duplicates, ties everywhere) and a
    buffer of 3: every panel overflows and is redone densely.  The arithmetic is exact."""
    X, _ref_i, ref_d = search_case("lattice", n, 3)
    got_i, got_d, proxy = _run_candidates(be, X, kc, cap)
    assert proxy.overflowed_panels == proxy.calls["knn_filter"] == 2  # (cnt > cap).any() in every panel
    assert torch.equal(torch.from_numpy(np.sort(got_d, axis=1)), torch.from_numpy(ref_d[:, :kc].copy()))
    assert not (got_i == np.arange(n)[:, None]).any()
    s = np.sort(got_i, axis=1)
    assert (s[:, 1:] != s[:, :-1]).all()
    true_d = ((X[:, None, :] - X[got_i]) ** 2).sum(axis=2)
    assert (true_d <= ref_d[:, kc - 1:kc]).all()
    return proxy


# ---- 4. wnn_bandwidth against the set-based definition -----------------------------------------------------------
def bandwidth_reference(X, indptr, indices, n_bw, cells=None):
    """csigma of the cells (default: all), oracle/wnn_oracle.py `neighbors` statement by statement - kNN sets as
    python sets, the key N (1 - jaccard distance) + (bbox - euclid) / bbox with N = n as the kernel and
    ``_bandwidths`` write it, selection by (key, id) - with NaN where a cell has no candidate.  A cell's candidates
    are looked up through the reverse lists instead of scanning all j (the others have no overlap and are skipped
    by the oracle too).  Also returns the smallest relative gap between a cell's n_bw-th and (n_bw + 1)-th keys."""
    n = len(indptr) - 1
    sets = [set(indices[indptr[i]:indptr[i + 1]].tolist()) for i in range(n)]
    listers = [set() for _ in range(n)]
    for i, s in enumerate(sets):
        for u in s:
            listers[u].add(i)
    bbox = np.linalg.norm(np.ptp(X, axis=0))
    cells = range(n) if cells is None else cells
    out, gap = np.full(len(cells), np.nan), np.inf
    for o, i in enumerate(cells):
        J = sorted(set().union(*[listers[u] for u in sets[i]]) - {i})
        if not J:
            continue
        E = np.linalg.norm(X[i] - X[J], axis=1)
        cand = []
        for j, e in zip(J, E):
            jac_dist = 1.0 - len(sets[i] & sets[j]) / len(sets[i] | sets[j])
            if jac_dist < 1.0:
                cand.append(((n - jac_dist * n) + (bbox - e) / bbox, j, e))
        cand.sort(key=lambda t: (t[0], t[1]))
        if cand:
            out[o] = np.mean([c[2] for c in cand[:n_bw]])
        if len(cand) > n_bw:
            gap = min(gap, (cand[n_bw][0] - cand[n_bw - 1][0]) / cand[n_bw][0])
    return out, gap


def _csr(rows, n):
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    indices = np.asarray([c for r in rows for c in r], dtype=np.int32)
    return sp.csr_matrix((np.ones(indices.size), indices, indptr), shape=(n, n))


@lru_cache(maxsize=None)
def irregular_graph(n, p):
    """rows of 0 to 9 sorted unique columns (row 1 and every eleventh row empty, every seventh row lists itself; at
    n <= 5 the other rows have two columns at least, so that some cells do share a neighbour)"""
    rng = np.random.default_rng(100 * n + p)
    rows = []
    for i in range(n):
        deg = 0 if (i == 1 or i % 11 == 10) else min(n, int(rng.integers(2 if n <= 5 else 0, 10)))
        r = set(rng.choice(n, size=deg, replace=False).tolist())
        if i % 7 == 0 and deg:
            r.add(i)
            if len(r) > 9:
                r.remove(max(r - {i}))
        rows.append(sorted(r))
    return _frozen(rng.standard_normal((n, p))), _csr(rows, n)


@lru_cache(maxsize=None)
def tied_graph():
    """cells 0..19 are one point twenty times over, with one neighbour list: from any other cell their keys are
    bit-identical, and n_bw cuts through the group - the selection follows the cell id"""
    X, G = irregular_graph(67, 5)
    X = X.copy()
    X[:20] = X[0]
    rows = [G.indices[G.indptr[i]:G.indptr[i + 1]].tolist() for i in range(67)]
    for i in range(20):
        rows[i] = [25, 30, 31]
    return _frozen(X), _csr(rows, 67)


_HUB_SALT = {8193: 200000}  # seeds moved to where every sampled cell's 20th and 21st keys are 1e-9 apart (relative)


@lru_cache(maxsize=None)
def hub_graph(listers, private=True):
    """cell 0 is listed by cells 1..listers: each of them gathers listers - 1 entries, the size of its sort.
    ``private``: every third lister also lists a cell of its own (another degree, another Jaccard distance), and
    the hub lists two cells nobody else lists; else the listers list nothing else and the hub's row is empty."""
    rng = np.random.default_rng(listers + _HUB_SALT.get(listers, 0))
    extra = listers // 3 + 3 if private else 0
    n = 1 + listers + extra
    rows = [[] for _ in range(n)]
    for i in range(1, listers + 1):
        rows[i] = [0] + ([listers + 1 + i // 3] if private and i % 3 == 0 else [])
    if private:
        rows[0] = [n - 2, n - 1]
    return _frozen(rng.standard_normal((n, 4))), _csr(rows, n)


def hub_sample(G, listers):
    """about 50 cells: the hub, the first and the last lister, a cell listed by one lister only, others at random"""
    rng = np.random.default_rng(3)
    picked = {0, 1, listers, G.shape[0] - 1} | set(rng.integers(1, listers + 1, 46).tolist())
    return sorted(picked)


def check_bandwidth(be, X, G, n_bw, cells=None, min_gap=1e-9, direct=True, expect_over=False):
    """``pp._bandwidths`` (and, with ``direct``, ``be.wnn_bandwidth`` itself) against the set-based definition"""
    want, gap = bandwidth_reference(X, G.indptr, G.indices, n_bw, cells)
    if min_gap is not None:
        assert gap > min_gap, gap  # (a condition on the input: the selection is decided far above the rounding)
    want = torch.from_numpy(want)
    sel = slice(None) if cells is None else torch.as_tensor(list(cells))
    Xd = be.to_device(X.copy())
    if direct:
        R = G.T.tocsr()
        bbox = float(np.linalg.norm(np.ptp(X, axis=0)))
        cs, over = be.wnn_bandwidth(Xd, be.to_device(G.indptr, np.int64), be.to_device(G.indices, np.int32),
                                    be.to_device(R.indptr, np.int64), be.to_device(R.indices, np.int32), n_bw, bbox)
        assert over == expect_over
        if not over:
            assert torch.allclose(cs.cpu()[sel], want, rtol=1e-12, atol=0, equal_nan=True)
    got = pp._bandwidths(be, Xd, G, n_bw)
    assert torch.allclose(got.cpu()[sel], want, rtol=1e-12, atol=0, equal_nan=True)
    return want


# ---- 5. umap_strengths against the oracle ------------------------------------------------------------------------
@lru_cache(maxsize=None)
def umap_case(n, k):
    """(idx, dist, want): a neighbour table with the edge rows of smooth_knn_dist and the oracle's CSR for it.
    Rows 3.. (and the last rows, which fall into the kernel's second block at n = 257): distances all zero (sigma
    floored by the table's mean), zero with one positive entry, equal throughout, spread over 1e-6 .. 1e6 (sigma
    floored by the row's mean), the cell itself outside slot 0."""
    rng = np.random.default_rng(10 * n + k)
    d = np.sort(rng.gamma(2.0, 1.0, (n, k)), axis=1)
    d[:, 0] = 0.0
    idx = np.zeros((n, k), dtype=np.int64)
    if n > 1:
        for i in range(n):  # the cell itself in slot 0, k - 1 distinct others
            idx[i, 0] = i
            idx[i, 1:] = (i + 1 + rng.choice(n - 1, size=k - 1, replace=False)) % n
        spread = np.geomspace(1e-6, 1e6, k - 1)
        for base in (3, n - 5):
            d[base, :] = 0.0
            d[base + 1, :] = 0.0
            d[base + 1, k - 1] = 0.8
            d[base + 2, :] = 0.7
            d[base + 3, 1:] = spread
            idx[base + 4, 0], idx[base + 4, k - 1] = idx[base + 4, k - 1], idx[base + 4, 0]
        d[::50, 1:min(4, k)] = 0.0  # duplicated points
    # a condition on the input: no exponent of the oracle lies where exp underflows to zero (-745.13: there one
    # more rounding of the exponent decides between the last denormal and a zero that is not stored, i.e. the pattern)
    d32 = d.astype(np.float32).astype(np.float64)
    sigma, rho = wnn_oracle.smooth_knn_dist(d32, float(k))
    x = (d32 - rho[:, None]) / sigma[:, None]
    assert not ((x > 744.0) & (x < 746.5)).any()
    want = wnn_oracle.fuzzy_simplicial_set(idx, d, n, k)
    want.sort_indices()
    return _frozen(idx, d) + (want,)


def check_umap(be, n, k, backend):
    """``pp.fuzzy_simplicial_set`` (``backend``: the kernel; None: the tensor bisection) against the numpy oracle"""
    idx, d, want = umap_case(n, k)
    got = pp.fuzzy_simplicial_set(be.to_device(idx.copy(), np.int64), be.to_device(d.copy()), n, k, backend=backend)
    got.sort_indices()
    assert got.shape == want.shape == (n, n)
    assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
    assert got.nnz == 0 or np.abs(got.data - want.data).max() < 1e-6
