"""muon_amd.rna.pp.scale on the device: the two kernels of csrc/scale.hip at their edges, the moments that feed their
tables, and ``scale -> tl.pca`` end to end against tests/golden/scale_golden.npz (scikit-learn 1.7.2 on the dense clipped
matrix in f64).

  * kernels: given the same f64 tables the outputs are BIT-EQUAL to the NumPy statement of tests/scale_refs.py (IEEE
    subtraction, division and comparison in f64, one rounding, no contraction: there is no tolerance), NaN exactly where
    the statement has NaN; repeats are byte-equal; guard elements around every output block come back untouched.  Every
    matrix carries the crafted genes and asserts that entries are clipped at each side and that a z is itself clipped.
    Shapes: the widths and row lengths at which a 64-lane wave and its 1024-column LDS segment change rounds (rows of
    1000 entries in 1037 columns: batches of 64 entries that straddle a segment's end), three truly empty rows, and a
    tall matrix with more rows than the dense kernel's grid has waves (8 workgroups of 4 per CU) and more entries than
    the value kernel's grid covers in one round.
  * moments: ``var["mean"]`` / ``var["std"]`` of the whole call against a ``np.longdouble`` restatement, with the bound
    tests/test_gpu_rna.py derives for the sums - |sum - ref| <= (len + 64) 2^-53 sum|terms| - carried through the mean,
    the variance and the square root (``_moment_bounds``).
  * end to end: rna_fixture's ``b16`` matrix with the crafted genes, ``max_value`` 10 and 3: the dense ``X`` bit-equal
    to the statement fed the call's own ``var["mean"]`` / ``var["std"]``; ``tl.pca`` on the remembered form by
    rna_fixture.deviations' four figures against the golden, never against the host route.  The bounds are ten times the
    worst case measured on an MI355X (PARITY_MEASURED) under the ceiling of tests/test_gpu_rna.py: no
    angle bound above 1e-4, no variance rtol above 1e-5.
"""
import numpy as np
import pytest
import torch

import muon_amd as mu
from muon_amd import AnnData, rna
from muon_amd._backend import DeviceCSR
from muon_amd._rna import preproc as rp
from tests import scale_refs as sr

pytestmark = pytest.mark.gpu

# (angle of PCs, angle of X_pca, variance, variance_ratio) measured on an MI355X, per case
PARITY_MEASURED = {
    "b16_clip10": (2.49e-07, 2.19e-07, 1.04e-08, 1.04e-08), "b16_clip3": (1.04e-06, 4.07e-07, 1.87e-08, 1.76e-08),
}
ANGLE = min(10 * max(max(v[:2]) for v in PARITY_MEASURED.values()), 1e-4)   # 1.04e-5
VAR_RTOL = min(10 * max(max(v[2:]) for v in PARITY_MEASURED.values()), 1e-5)  # 1.87e-7
assert ANGLE <= 1e-4 and VAR_RTOL <= 1e-5
U53 = 2.0 ** -53
LENS = (0, 1, 63, 64, 65, 257, 1000)
MAX_VALUES = (None, 10, 1.5)
GUARD = 64
# (width of the random part, rows at least): the issue's widths; the LDS segment's edge (1024 columns in all, one more,
# four segments exactly and one more, nine segments); a tall matrix for the grid-stride rounds of both kernels
SHAPES = [(1, 300), (63, 300), (64, 300), (65, 300), (257, 300), (1030, 300),
          (1024 - sr.N_CRAFTED, 300), (1025 - sr.N_CRAFTED, 300), (4096 - sr.N_CRAFTED, 300),
          (4097 - sr.N_CRAFTED, 300), (9000, 300), (257, 9000)]


def _edge_matrix(d_r, n_min, dtype):
    """(CSR, dense f64, stored mask, rows used for the tables): rows of 0, 1, 63, 64, 65, 257 and 1000 random entries
    (those that fit) in mixed order, values of both signs with explicitly stored zeros, the crafted genes appended, and
    three truly empty rows at the end (left out of the tables, so that the constant gene stays constant)."""
    rng = np.random.default_rng(d_r * 7 + n_min)
    lens = [l for l in LENS if l <= d_r]
    lens = np.array(lens * -(-n_min // len(lens)))
    rng.shuffle(lens)
    n = lens.size
    A = np.zeros((n + 3, d_r + sr.N_CRAFTED))
    st = np.zeros(A.shape, dtype=bool)
    for i, l in enumerate(lens):
        c = rng.choice(d_r, l, replace=False)
        v = rng.standard_normal(l) * 3
        v[rng.random(l) < 0.1] = 0
        A[i, c], st[i, c] = v.astype(np.float32), True
    A[:n, d_r:], st[:n, d_r:] = sr.crafted_columns(n, seed=d_r)
    M = sr.csr_from(A, st, dtype)
    assert M.nnz == int(st.sum()) and (np.diff(M.indptr)[n:] == 0).all()
    return M, A, st, n


def _guarded(hip, numel, dtype):
    buf = torch.full((numel + 2 * GUARD,), -77.0, dtype=dtype, device=hip.device)
    return buf, buf[GUARD:GUARD + numel]


def _guards_intact(buf):
    return bool((buf[:GUARD] == -77.0).all()) and bool((buf[-GUARD:] == -77.0).all())


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("d_r,n_min", SHAPES)
def test_kernels_bit_equal_to_the_statement(hip, d_r, n_min, dtype):
    M, A, st, n_tab = _edge_matrix(d_r, n_min, dtype)
    n, d = M.shape
    X = hip.upload_csr(M.indptr, M.indices, M.data, M.shape, slab_ptr=False)
    tdt = X.values.dtype
    mean, std = sr.moments_ref(A[:n_tab])
    rows_of, cols_of = np.repeat(np.arange(n), np.diff(M.indptr)), M.indices
    ranges = [(0, n), (5, n - 7), (9, 9), (11, 12), (n - 4, n), (0, 0), (n, n)]
    for mv in MAX_VALUES:
        C, S, z = sr.scale_ref(A, mean, std, mv)
        if mv is not None:
            below, above, zclip = sr.clip_counts(A, st, mean, std, mv)
            assert below > 0 and above > 0 and zclip > 0, (below, above, zclip)
        assert np.isnan(C).sum() == 1
        lo, hi = (-np.inf, np.inf) if mv is None else (-float(mv), float(mv))
        tabs = [hip.to_device(t, np.float64) for t in (mean, std, z)]

        # the values: S on the stored entries
        ref = S[rows_of, cols_of].astype(dtype)
        buf, out = _guarded(hip, X.nnz, tdt)
        got = hip.scale_values(X, *tabs, lo, hi, out=out)
        assert got.data_ptr() == out.data_ptr() and _guards_intact(buf)
        assert sr.bits_equal(hip.to_host(got), ref)
        again = hip.scale_values(X, *tabs, lo, hi)
        assert hip.to_host(again).tobytes() == hip.to_host(got).tobytes()
        assert hip.to_host(X.values).tobytes() == M.data.tobytes()
        Xc = DeviceCSR(X.indptr, X.indices, X.values.clone(), X.shape)  # in place
        hip.scale_values(Xc, *tabs, lo, hi, out=Xc.values)
        assert hip.to_host(Xc.values).tobytes() == hip.to_host(got).tobytes()

        # the dense rows: C, whole rows, for ranges inside the matrix, empty ones and a single row
        Cd = C.astype(dtype)
        for r0, r1 in ranges:
            buf, flat = _guarded(hip, (r1 - r0) * d, tdt)
            blk = hip.scale_dense_rows(X, *tabs, lo, hi, r0, r1, out=flat.view(r1 - r0, d))
            assert _guards_intact(buf), (r0, r1)
            g = hip.to_host(blk)
            assert sr.bits_equal(g, Cd[r0:r1]), (mv, r0, r1)
            twice = hip.scale_dense_rows(X, *tabs, lo, hi, r0, r1)
            assert hip.to_host(twice).tobytes() == g.tobytes()

    # zero_center=False: mean = z = 0, the lower side open - it stays sparse
    zero = hip.to_device(np.zeros(d), np.float64)
    _C, S0, z0 = sr.scale_ref(A, mean, std, 1.5, zero_center=False)
    assert not np.nan_to_num(z0).any()
    got = hip.to_host(hip.scale_values(X, zero, tabs[1], zero, -np.inf, 1.5))
    assert sr.bits_equal(got, S0[rows_of, cols_of].astype(dtype)) and np.nanmin(got) < -1.5 and np.nanmax(got) == 1.5


def test_arguments_are_checked_before_any_launch(hip):
    from muon_amd._ffi import MuonAmdError

    M, A, _st, n_tab = _edge_matrix(65, 300, np.float32)
    X = hip.upload_csr(M.indptr, M.indices, M.data, M.shape, slab_ptr=False)
    tabs = [hip.to_device(np.ones(M.shape[1]), np.float64) for _ in range(3)]
    with pytest.raises(MuonAmdError):
        hip.scale_values(X, *tabs, 2.0, -2.0)
    with pytest.raises(MuonAmdError):
        hip.scale_dense_rows(X, *tabs, 2.0, -2.0, 0, 4)
    with pytest.raises(AssertionError):
        hip.scale_dense_rows(X, *tabs, -2.0, 2.0, 3, M.shape[0] + 1)


def _moment_bounds(M):
    """(mean, its bound, std, its bound) per gene in longdouble from the stored values of CSR ``M`` (n cells), for sums
    that satisfy |s - S| <= (len + 64) u sum|terms| (tests/test_gpu_rna.py), u = 2^-53, carried through
        mean = fl(s1 / n)                                        d_mean <= e1 / n + u |mean|
        var  = fl(fl(fl(s2 / n) - fl(mean^2)) * fl(n / (n - 1)))
               d_var <= (e2 / n + 2 |mean| d_mean + d_mean^2 + 2 u (S2 / n + mean^2)) n / (n - 1) + 4 u var
        std  = fl(sqrt(var)):  |sqrt(a) - sqrt(b)| = |a - b| / (sqrt(a) + sqrt(b))  =>  d_std <= d_var / std + u std."""
    n = M.shape[0]
    T = M.T.tocsr()
    L = np.longdouble
    out = []
    for j in range(M.shape[1]):
        x = T.data[T.indptr[j]:T.indptr[j + 1]].astype(L)
        slack = (x.size + 64) * L(U53)
        S1, S2 = x.sum(), (x * x).sum()
        e1, e2 = slack * np.abs(x).sum(), slack * S2
        mean = S1 / n
        d_mean = e1 / n + U53 * abs(mean)
        var = (S2 / n - mean ** 2) * n / (n - L(1))
        d_var = (e2 / n + 2 * abs(mean) * d_mean + d_mean ** 2 + 2 * U53 * (S2 / n + mean ** 2)) * n / (n - L(1)) + 4 * U53 * var
        std = np.sqrt(max(var, L(0)))
        out.append((mean, d_mean, std, (d_var / std + U53 * std) if std > 0 else L(0)))
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_moments_of_the_whole_call(hip, dtype):
    M = sr.e2e_matrix("b16_clip10").astype(dtype)
    ad = AnnData(M.copy())
    rna.pp.scale(ad, max_value=10, backend=hip)
    mean, std = ad.var["mean"].values, ad.var["std"].values
    worst = 0.0
    for j, (m, dm, s, ds) in enumerate(_moment_bounds(M)):
        assert abs(np.longdouble(mean[j]) - m) <= dm, j
        if s == 0 or ds >= s:  # no variance the sums can resolve (the all-zero and the constant gene): 0 -> 1
            assert std[j] == 1.0 or std[j] <= ds, j
            continue
        assert abs(np.longdouble(std[j]) - s) <= ds, j
        worst = max(worst, float(abs(np.longdouble(std[j]) - s) / ds))
    print(f"MOMENTS {np.dtype(dtype).name}: worst |std - ref| / bound = {worst:.3f}")
    assert std[M.shape[1] - 6] == 1.0 and std[M.shape[1] - 5] == 1.0 and mean[M.shape[1] - 5] == 2.0


class _Spy:
    """Forwards to an operator set and counts the calls of its operators."""

    def __init__(self, inner):
        self._inner, self.calls = inner, {}

    def __getattr__(self, name):
        attr = getattr(self._inner, name)
        if not callable(attr):
            return attr

        def counted(*a, **k):
            self.calls[name] = self.calls.get(name, 0) + 1
            return attr(*a, **k)

        return counted


@pytest.mark.parametrize("name", list(sr.E2E_CASES))
def test_scale_then_pca_golden(hip, name, monkeypatch):
    mv = sr.E2E_CASES[name]["max_value"]
    M = sr.e2e_matrix(name)
    monkeypatch.setattr(rp, "_DENSE_CHUNK_BYTES", 400 * M.shape[1] * 4)  # four chunks, the last one short
    spy = _Spy(hip)
    ad = AnnData(M.copy())
    rna.pp.scale(ad, max_value=mv, backend=spy)
    assert spy.calls["upload_csr"] == 1 and spy.calls["gene_moments"] == 1 and spy.calls["scale_values"] == 1
    assert spy.calls["scale_dense_rows"] == 4

    A = M.astype(np.float64).toarray()
    st = np.zeros(A.shape, dtype=bool)
    st[np.repeat(np.arange(M.shape[0]), np.diff(M.indptr)), M.indices] = True
    mean, std = ad.var["mean"].values, ad.var["std"].values
    below, above, zclip = sr.clip_counts(A, st, mean, std, mv)
    assert below > 0 and above > 0 and zclip > 0
    C, _S, _z = sr.scale_ref(A, mean, std, mv)
    assert type(ad.X) is np.ndarray and ad.X.flags.c_contiguous and ad.X.dtype == np.float32
    assert ad.X.tobytes() == C.astype(np.float32).tobytes()

    diag = {}
    mu.tl.pca(ad, n_comps=11, oversample=5, diagnostics=diag, backend=spy)
    assert spy.calls["upload_csr"] == 1  # the remembered form: no upload
    assert diag["block"] == 16 and diag["converged"]
    a_pcs, a_x, v, r = sr.deviations(name, ad)
    print(f"PARITY {name}: ({a_pcs:.2e}, {a_x:.2e}, {v:.2e}, {r:.2e}) iterations {diag['iterations']} spmm {diag['spmm']}")
    assert a_pcs < ANGLE and a_x < ANGLE and v < VAR_RTOL and r < VAR_RTOL

    # twice: byte-equal, the dense matrix and the decomposition
    bd = AnnData(M.copy())
    rna.pp.scale(bd, max_value=mv, backend=hip)
    mu.tl.pca(bd, n_comps=11, oversample=5, backend=hip)
    assert bd.X.tobytes() == ad.X.tobytes() and bd.obsm["X_pca"].tobytes() == ad.obsm["X_pca"].tobytes()


def test_zero_center_false_keeps_the_device_copy(hip):
    from muon_amd._hostmatrix import resident

    M = sr.e2e_matrix("b16_clip3")
    spy = _Spy(hip)
    ad = AnnData(M.copy())
    rna.pp.scale(ad, zero_center=False, max_value=3.0, backend=spy)
    assert spy.calls["scale_values"] == 1 and "scale_dense_rows" not in spy.calls
    t = M.data.astype(np.float64) / ad.var["std"].values[M.indices]
    assert ad.X.data.tobytes() == np.minimum(t, 3.0).astype(np.float32).tobytes() and (t > 3.0).any()
    Xd = resident(ad.X, spy)
    assert Xd is not None and np.array_equal(hip.to_host(Xd.values), ad.X.data)
