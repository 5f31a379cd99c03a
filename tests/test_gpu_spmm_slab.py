"""The row-stream SpMM with 320-column Q slabs (k_spmm_wide / k_spmm_wide_rng, csrc/spmm_win.hip) against the
256-column instances on the same operand: a row's entries are accumulated in column order whatever the slab width, so
the products must be equal bit for bit - and both within f32 accumulation of a dense f64 product (the tolerance
tests/test_gpu_kernels.py uses for the same product).  The shapes are the smallest at which the wide kernel can go
wrong: slab edges, partial workgroups, windows of 16 that overflow inside a 320-column slab and across its edge."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch

pytestmark = pytest.mark.gpu

TOL = 2e-6  # f32 accumulation, relative to |X| |Q| (tests/test_gpu_kernels.py: test_spmm_stream_matches_f64_and_csr_kernel)
KS = [6, 7, 8]  # the layouts that have a 320-column instance


def _csr(rows, d, rng):
    """rows: list of column arrays (sorted, unique) -> canonical f32 CSR with values in (0.5, 1.5) u -(0.5, 1.5)."""
    indptr = np.zeros(len(rows) + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    indices = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows] + [np.zeros(0, np.int32)])
    vals = ((0.5 + rng.random(indices.size)) * rng.choice([-1.0, 1.0], size=indices.size)).astype(np.float32)
    m = sp.csr_matrix((vals, indices, indptr), shape=(len(rows), d))
    assert m.has_sorted_indices
    return m


def _background(n, d, dens, rng):
    return [np.flatnonzero(rng.random(d) < dens) for _ in range(n)]


def _up(hip, m):
    return hip.upload_csr(m.indptr, m.indices, m.data, m.shape)


def _both_widths(hip, fn):
    """fn() at forced 256 and forced 320 columns."""
    out = []
    try:
        for w in (256, 320):
            hip.tune("spmm_slab", w)
            out.append(fn())
    finally:
        hip.tune("spmm_slab", 0)
    return out


def _check(hip, m, P, Q, K):
    assert P.k == K and hip.spmm_slab(P.k, P.n_pos, 64) == 320  # (the wide instance is what runs by default)
    Qd = hip.to_device(Q)
    Yn, Yw = _both_widths(hip, lambda: hip.spmm(P, Qd))
    assert torch.equal(Yn, Yw)
    ref = m.astype(np.float64) @ Q.astype(np.float64)
    scale = np.abs(m).astype(np.float64) @ np.abs(Q).astype(np.float64) + 1e-30
    Y = hip.to_host(Yw)
    assert np.max(np.abs(Y - ref) / scale) < TOL
    assert np.all(Y[np.diff(m.indptr) == 0] == 0)


@pytest.mark.parametrize("d", [1, 319, 320, 321, 640, 641, 1607])
def test_slab_edges(hip, d):
    """Entries at the first and last column of every 320-column slab and at n_cols - 1: the `col < s_hi` boundary, a last
    slab narrower than 320 and the (clamped) copy of the slab past the end."""
    rng = np.random.default_rng(d)
    K, n = 6, 64 * 6 + 9
    marks = np.array(sorted({c for c in (0, 319, 320, 639, 640, d - 1) if c < d}))
    rows = _background(n, d, 0.03, rng)
    rows[0] = marks                                      # the marks alone
    rows[1] = np.union1d(rows[1], marks)                 # ... among others
    rows[2] = np.arange(d)                               # every column: every window full
    rows[3] = np.zeros(0, np.int64)
    rows[n - 1] = marks[-1:]                             # the last column alone, in the partial last workgroup
    m = _csr(rows, d, rng)
    Q = rng.standard_normal((d, 64)).astype(np.float32)
    X = _up(hip, m)
    _check(hip, m, hip.stream(X, K=K), Q, K)
    _check(hip, m, hip.stream(X, sort_rows=False, K=K), Q, K)


@pytest.mark.parametrize("K", KS)
def test_workgroup_edges(hip, K):
    """64 K 2 + 5 rows: a partial last workgroup; the dealt layout pads it with positions that hold no row (perm = -1);
    empty rows; and, in matrix order, a workgroup none of whose rows has an entry in the slab [320, 640)."""
    rng = np.random.default_rng(K)
    n, d = 64 * K * 2 + 5, 1000
    rows = _background(n, d, 0.04, rng)
    for r in range(64 * K, 2 * 64 * K):  # workgroup 1 of the matrix-order layout
        rows[r] = rows[r][(rows[r] < 320) | (rows[r] >= 640)]
    for r in (0, 7, 64 * K, n - 1):
        rows[r] = np.zeros(0, np.int64)
    m = _csr(rows, d, rng)
    Q = rng.standard_normal((d, 64)).astype(np.float32)
    X = _up(hip, m)
    P = hip.stream(X, K=K)
    assert P.n_pos % (64 * K) == 0 and int((P.perm < 0).sum()) == P.n_pos - n > 0
    _check(hip, m, P, Q, K)
    _check(hip, m, hip.stream(X, sort_rows=False, K=K), Q, K)


COUNTS = (15, 16, 17, 32, 33, 49)


def _overflow_rows(K, d, rng):
    """Matrix-order layout: position p of workgroup 0 is (wave, row-set, group) = (p // 4K, p % 4K // 4, p % 4).
    Row-set 0 is revisited at the mid point of a slab, row-set K - 1 at its end."""
    n = 64 * K + 64 * K // 2  # a second, partial workgroup of ordinary rows
    rows = _background(n, d, 0.03, rng)
    tail = lambda: 1290 + np.flatnonzero(rng.random(d - 1290) < 0.05)  # (something in the last slabs as well)

    def put(wave, k, g, cols):
        rows[(wave * K + k) * 4 + g] = np.union1d(np.asarray(cols), tail())

    for i, c in enumerate(COUNTS):  # waves 0 .. 5
        put(i, 0, 0, np.arange(330, 330 + c))                            # exactly c inside the slab [320, 640)
        put(i, K - 1, 1, np.arange(639 - c + 1, 640))                    # ... up to its last column
        put(i, 2, 2, np.arange(640 - c // 2, 640 + c - c // 2))          # c across the edge 640
        put(i, K - 1, 3, np.arange(320 - (c - c // 2), 320 + c // 2))    # c across the edge 320
        put(i, 0, 1, np.arange(960 - c // 2, 960 + c - c // 2))          # c across the edge 960 (mid-point revisit)
    for g in range(4):
        put(6, 0, g, np.arange(10 * g, 10 * g + 40 + g))                 # all four rows of a row-set: mid point
        put(7, K - 1, g, np.arange(400 + g, 400 + g + 17 + 16 * g))      # ... and at the end of the slab
    for wave, k in ((8, 0), (9, K - 1), (10, 1), (11, K - 2)):           # one row-set overflowing slab after slab
        put(wave, k, 0, np.concatenate([np.arange(5, 25), np.arange(321, 321 + 33), np.arange(700, 717),
                                        np.arange(960, 960 + 50)]))
    put(12, 0, 0, np.arange(0, 1280))                                    # every window of four slabs in a row
    put(12, K - 1, 0, np.arange(100, 1500))
    return rows


@pytest.mark.parametrize("K", KS)
def test_window_overflow_at_the_wide_slab(hip, K):
    """Rows with 15 .. 49 entries inside one 320-column slab and across its edges - a window holds 16, a 17th entry in a
    slab is a revisit of the row-set - in row-set 0 (revisited at the mid point), row-set K - 1 (at the end of the slab),
    in all four rows of a row-set, and in consecutive slabs (the strict waits behind a revisit's request)."""
    rng = np.random.default_rng(100 + K)
    d = 1607
    m = _csr(_overflow_rows(K, d, rng), d, rng)
    for c in COUNTS:
        assert np.any(np.diff(m[:, 320:640].indptr) == c)
    Q = rng.standard_normal((d, 64)).astype(np.float32)
    X = _up(hip, m)
    _check(hip, m, hip.stream(X, sort_rows=False, K=K), Q, K)
    _check(hip, m, hip.stream(X, K=K), Q, K)


@pytest.mark.parametrize("K,sort_rows", [(6, True), (7, False), (8, True)])
def test_ranged_product(hip, K, sort_rows):
    """mu_spmm_stream_ranges_slab_f32 on ranges that start at multiples of neither 256 nor 320, one shorter than a slab,
    two ranges per workgroup and three values of blockIdx.y; the table holds where a row's entries of a range begin."""
    rng = np.random.default_rng(200 + K)
    n, d = 64 * K + 70, 2400
    rows = _background(n, d, 0.03, rng)
    rows[1] = np.arange(d)  # every window full, in every range
    rows[2] = np.zeros(0, np.int64)
    rows[5] = np.arange(30, 700)
    m = _csr(rows, d, rng)
    bounds = np.array([37, 150, 611, 1000, 1333, 2003, 2400])  # six ranges: [37, 150) is shorter than a slab
    n_rg, per_wg = len(bounds) - 1, 2
    ny = n_rg // per_wg
    tbl = np.stack([np.diff(m[:, :b].indptr) for b in bounds]).astype(np.uint32)  # [boundary, row]: entries before it
    q_off = np.concatenate([[0], np.cumsum(np.diff(bounds))])
    Qc = rng.standard_normal((int(q_off[-1]), 64)).astype(np.float32)  # compact: range r's columns at rows q_off[r] ..
    h = (C.c_int32 * (5 * n_rg))()
    for r in range(n_rg):
        h[5 * r:5 * r + 5] = [int(bounds[r]), int(bounds[r + 1]), int(q_off[r]), r, r + 1]
    P = hip.stream(_up(hip, m), sort_rows=sort_rows, K=K)
    assert P.k == K and hip.spmm_slab_ranged(P.k) == 320
    Qd, tbl_d = hip.to_device(Qc), hip.to_device(tbl.view(np.int32)).contiguous()
    perm_p = None if P.perm is None else P.perm.data_ptr()
    out = []
    for w in (256, 320):
        Y = hip.zeros((ny, n, 64), torch.float32)
        rc = hip.lib.mu_spmm_stream_ranges_slab_f32(P.n_pos, P.sptr.data_ptr(), P.ent.data_ptr(), perm_p, P.k,
                                                    Qd.data_ptr(), Qc.shape[0], Y.data_ptr(), n * 64, tbl_d.data_ptr(), n,
                                                    n_rg, h, per_wg, w, None)
        assert rc == 0, hip.lib.mu_last_error()
        torch.cuda.synchronize()
        out.append(Y)
    assert torch.equal(out[0], out[1])
    Yw = hip.to_host(out[1])
    m64, a64 = m.astype(np.float64).tocsc(), abs(m).astype(np.float64).tocsc()
    for y in range(ny):
        ref, scale = np.zeros((n, 64)), np.full((n, 64), 1e-30)
        for r in range(y * per_wg, (y + 1) * per_wg):
            q = Qc[q_off[r]:q_off[r + 1]].astype(np.float64)
            ref += m64[:, bounds[r]:bounds[r + 1]] @ q
            scale += a64[:, bounds[r]:bounds[r + 1]] @ np.abs(q)
        assert np.max(np.abs(Yw[y] - ref) / scale) < TOL, y


def test_lsi_is_bit_identical_at_both_widths(hip):
    """lsi_device on the 3000 x 2500 planted matrix of the lsi tests, its products forced to K = 6 row-sets per wave (a
    matrix this small is dealt for K = 1, which has no wide instance): U, stdev and V equal bit for bit."""
    from muon_amd._atac.tools import lsi_device
    from oracle import tfidf_oracle
    from tests.synth import planted_topics_csr

    X = planted_topics_csr(3000, 2500, n_topics=80, density=0.03, seed=3, dtype=np.float32)
    T = tfidf_oracle.canonical(tfidf_oracle.tfidf(X)).astype(np.float32)
    Xd = hip.upload_csr(T.indptr, T.indices, T.data, T.shape)
    host = lambda a: hip.to_host(a) if torch.is_tensor(a) else np.asarray(a)
    try:
        hip.tune("spmm_k", 6)
        assert hip.spmm_slab(1, 3008, 64) == 320
        (Un, sn, Vn, _), (Uw, sw, Vw, _) = _both_widths(hip, lambda: lsi_device(hip, Xd, n_comps=50, return_info=True))
    finally:
        hip.tune("spmm_k", 0)
    assert np.array_equal(host(Un), host(Uw)) and np.array_equal(host(sn), host(sw)) and np.array_equal(host(Vn), host(Vw))
    assert np.all(np.isfinite(host(sw))) and host(Vw).shape == (2500, 50)


def test_query_and_error_paths(hip):
    lib = hip.lib
    ok = lib.mu_spmm_stream_slab_ok
    assert [ok(64, K, 320) for K in range(0, 10)] == [0, 0, 0, 0, 0, 0, 1, 1, 1, 0]
    assert [ok(64, K, 256) for K in range(0, 10)] == [0, 1, 1, 1, 1, 1, 1, 1, 1, 0]
    assert ok(32, 6, 320) == 0 and ok(16, 8, 320) == 0 and ok(32, 6, 256) == 1 and ok(48, 6, 256) == 0
    assert ok(64, 6, 288) == 0 and ok(64, 6, 0) == 0 and ok(64, 6, 512) == 0
    one = C.c_int64(0)
    P = C.byref(one)  # (the arguments are checked before anything is launched or read)
    i64 = C.c_int64
    f32 = lambda K, B, w: lib.mu_spmm_stream_slab_f32(i64(10), i64(10), P, P, None, K, P, B, P, w, None)
    assert f32(6, 32, 320) == -1 and b"320-column" in lib.mu_last_error()
    assert f32(5, 64, 320) == -1 and b"K = 5" in lib.mu_last_error()
    assert f32(6, 64, 288) == -1 and b"256 or 320" in lib.mu_last_error()
    assert f32(6, 48, 256) == -1 and b"B must be" in lib.mu_last_error()
    assert lib.mu_spmm_stream_slab_f32(i64(10), i64(10), None, None, None, 6, None, 64, None, 320, None) == -1
    h = (C.c_int32 * 5)(0, 10, 0, 0, 1)
    rng = lambda K, w, nr=1, hh=h: lib.mu_spmm_stream_ranges_slab_f32(i64(10), P, P, None, K, P, i64(10), P, i64(0), P, i64(10),
                                                                   nr, hh, 1, w, None)
    assert rng(5, 320) == -1 and b"K = 5" in lib.mu_last_error()
    assert rng(6, 288) == -1 and b"256 or 320" in lib.mu_last_error()
    assert rng(0, 320) == -1 and rng(6, 320, 33) == -1 and rng(6, 320, 1, None) == -1
    try:  # a forced width without an instance is the other width, not an error
        hip.tune("spmm_slab", 320)
        assert hip.spmm_slab(5, 1000, 64) == 256 and hip.spmm_slab(6, 1000, 32) == 256
        assert hip.spmm_slab(6, 1000, 64, torch.float64) == 256 and hip.spmm_slab(8, 1000, 64) == 320
        assert hip.spmm_slab_ranged(7) == 320 and hip.spmm_slab_ranged(5) == 256
    finally:
        hip.tune("spmm_slab", 0)
