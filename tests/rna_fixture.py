"""TEST INFRASTRUCTURE: the inputs of the RNA tests (tests/test_rna_host.py, tests/test_gpu_rna.py) and the loader of
their golden (tests/golden/rna_golden.npz, written by tests/golden/make_rna_golden.py with scikit-learn).

Inputs are not stored: they are regenerated from ``tests/synth.planted_topics_csr(..., density=0.08, seed=3)`` and
log-normalised in f64 by the plain statements below.  The golden holds scikit-learn's ``components_``,
``explained_variance_`` and ``explained_variance_ratio_`` only; the expected ``X_pca`` is (centred matrix) @ components,
computed here in f64.  Components are stored as an f32 head and an f16 tail scaled by 2^24 (2^-35 relative: far below
anything the tests resolve) so that the archive stays under 1 MB.
"""
import functools
import os

import numpy as np
import scipy.sparse as sp

from tests.synth import planted_topics_csr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rna_golden.npz")

# name -> cells, genes, topics, k, scale, zero_center, masked, and the block width the case runs at with `oversample`
# (lsi's rule: the narrowest of 16 / 32 / 64 that holds k + oversample); k = topics - 1, where the centred spectrum has
# its gap (the uncentred one has it one further down: the mean direction comes first)
CASES = {
    "b16": dict(n=1500, d=900, topics=12, k=11, scale=False, zero_center=True, masked=False, block=16, oversample=5),
    "b16_scale": dict(n=1500, d=900, topics=12, k=11, scale=True, zero_center=True, masked=False, block=16, oversample=5),
    "b32": dict(n=900, d=700, topics=21, k=20, scale=False, zero_center=True, masked=False, block=32, oversample=12),
    "b32_scale": dict(n=900, d=700, topics=21, k=20, scale=True, zero_center=True, masked=False, block=32, oversample=12),
    "b64": dict(n=1200, d=1000, topics=51, k=50, scale=False, zero_center=True, masked=False, block=64, oversample=14),
    "wide": dict(n=700, d=1300, topics=8, k=7, scale=False, zero_center=True, masked=False, block=16, oversample=9),
    "masked": dict(n=1500, d=900, topics=12, k=11, scale=False, zero_center=True, masked=True, block=16, oversample=5),
    "uncentred": dict(n=1500, d=900, topics=12, k=12, scale=False, zero_center=False, masked=False, block=16, oversample=4),
}


@functools.lru_cache(maxsize=None)
def counts(n, d, topics):
    """The raw counts (f32 CSR); callers copy before they change anything."""
    return planted_topics_csr(n, d, n_topics=topics, density=0.08, seed=3, dtype=np.float32)


def case_counts(name):
    c = CASES[name]
    return counts(c["n"], c["d"], c["topics"])


def normalize_f64(X, target_sum=None):
    """x / (total / target) in f64: target = the median of the totals > 0, a cell with total 0 keeps its values."""
    X = sp.csr_matrix(X, dtype=np.float64, copy=True)
    tot = np.asarray(X.sum(axis=1)).reshape(-1)
    target = np.median(tot[tot > 0]) if target_sum is None else target_sum
    div = np.where(tot > 0, tot / target, 1.0)
    X.data = X.data / np.repeat(div, np.diff(X.indptr))
    return X, tot


def log1p_f64(X, base=None):
    X = sp.csr_matrix(X, dtype=np.float64, copy=True)
    X.data = np.log1p(X.data)
    if base is not None:
        X.data = X.data / np.log(base)
    return X


@functools.lru_cache(maxsize=None)
def lognorm(name):
    """The case's log-normalised matrix (f64 CSR); callers copy / cast, never change it."""
    return log1p_f64(normalize_f64(case_counts(name))[0])


def mask_of(name):
    """The ``highly_variable`` column of the masked case: a fixed pseudo-random 60 % of the genes."""
    c = CASES[name]
    if not c["masked"]:
        return None
    return np.random.default_rng(11).random(c["d"]) < 0.6


def prepared_dense(name):
    """The dense f64 matrix scikit-learn decomposes: the masked columns of the log-normalised matrix, centred (and
    scaled by the ddof = 1 standard deviation, 0 -> 1) unless the case is uncentred."""
    c = CASES[name]
    A = lognorm(name).toarray()
    m = mask_of(name)
    if m is not None:
        A = A[:, m]
    if c["zero_center"]:
        A = A - A.mean(axis=0)
    if c["scale"]:
        s = A.std(axis=0, ddof=1)
        s[s == 0] = 1.0
        A = A / s
    return A


def run_case(mu, name, backend, **kw):
    """``tl.pca`` on the case's log-normalised matrix (rounded to f32) at the case's block width.  Returns (adata, the
    process' diagnostics)."""
    c = CASES[name]
    ad = mu.AnnData(lognorm(name).astype(np.float32))
    m = mask_of(name)
    if m is not None:
        ad.var["highly_variable"] = m
    diag = {}
    mu.tl.pca(ad, n_comps=c["k"], scale=c["scale"], zero_center=c["zero_center"], oversample=c["oversample"],
              diagnostics=diag, backend=backend, **kw)
    return ad, diag


def deviations(name, ad):
    """(largest principal angle of PCs, of X_pca, max relative deviation of variance, of variance_ratio) against the
    golden."""
    from oracle.lsi_oracle import max_subspace_angle

    g, m = golden(name), mask_of(name)
    pcs = ad.varm["PCs"]
    if m is not None:
        assert not pcs[~m].any()  # zero rows outside the mask
        pcs = pcs[m]
    return (max_subspace_angle(pcs, g["components"].T), max_subspace_angle(ad.obsm["X_pca"], expected_x_pca(name)),
            float(np.max(np.abs(ad.uns["pca"]["variance"] / g["variance"] - 1))),
            float(np.max(np.abs(ad.uns["pca"]["variance_ratio"] / g["variance_ratio"] - 1))))


def uncanonical(C, kind):
    """Canonical CSR ``C`` as a valid CSR that is not canonical, the way scipy's products and slices hand matrices out:
    every row's entries in reversed order ("unsorted"), or every third entry split into two stored parts
    ("duplicates": x - 0.25 and 0.25; exact for counts)."""
    if kind == "unsorted":
        order = np.concatenate([np.arange(C.indptr[i], C.indptr[i + 1])[::-1] for i in range(C.shape[0])])
        M = sp.csr_matrix((C.data[order], C.indices[order], C.indptr.copy()), shape=C.shape)
        assert not M.has_sorted_indices
    else:
        row, pick = np.repeat(np.arange(C.shape[0]), np.diff(C.indptr)), np.arange(C.nnz) % 3 == 0
        rows = np.concatenate([row, row[pick]])
        cols = np.concatenate([C.indices, C.indices[pick]])
        vals = np.concatenate([np.where(pick, C.data - 0.25, C.data), np.full(int(pick.sum()), 0.25)]).astype(C.dtype)
        order = np.argsort(rows, kind="stable")
        indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=C.shape[0]))]).astype(np.int64)
        M = sp.csr_matrix((vals[order], cols[order].astype(np.int32), indptr), shape=C.shape)
        assert M.nnz > C.nnz and not M.has_canonical_format
    assert np.array_equal(M.toarray(), C.toarray())
    return M


def split_store(a):
    """f64 array -> (f32 head, f16 tail * 2^24)."""
    hi = a.astype(np.float32)
    lo = ((a - hi.astype(np.float64)) * 2.0 ** 24).astype(np.float16)
    return hi, lo


@functools.lru_cache(maxsize=None)
def golden(name):
    """{"components" [k, d_used] f64, "variance" [k], "variance_ratio" [k]} of scikit-learn for the case."""
    with np.load(GOLDEN) as z:
        comp = z[f"{name}/components_hi"].astype(np.float64) + z[f"{name}/components_lo"].astype(np.float64) * 2.0 ** -24
        return {"components": comp, "variance": z[f"{name}/variance"].copy(),
                "variance_ratio": z[f"{name}/variance_ratio"].copy()}


@functools.lru_cache(maxsize=None)
def expected_x_pca(name):
    """(prepared matrix) @ components^T in f64: what ``obsm["X_pca"]`` spans."""
    return prepared_dense(name) @ golden(name)["components"].T
