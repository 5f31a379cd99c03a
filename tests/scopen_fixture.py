"""TEST INFRASTRUCTURE: the seeded inputs and the case table of the scOpen fixture (tests/golden/scopen_golden.npz),
shared by its generator (tests/golden/make_scopen_golden.py) and by tests/test_scopen_host.py / tests/test_gpu_scopen.py.
The inputs are regenerated from the seed wherever they are needed: the fixture stores results only."""
import numpy as np
import scipy.sparse as sp

from muon_amd._containers import AnnData, MuData

ROW_STEP = 37   # every 37th row of the imputed matrix is stored, the rest is rebuilt from W and H
TOL = 1e-4      # the reference's stopping ratio (scikit-learn's default, which its wrapper does not change)
MARGIN = 1e-3   # the deciding ratios of a converging case stay this far (relatively) from TOL on either side

# data set -> (n cells, d peaks, planted topics, generator seed): the seeds are the first for which every converging
# case on the data set meets MARGIN (the generator asserts it)
DATA = {"a": (257, 403, 6, 7), "b": (193, 330, 6, 7), "c": (129, 200, 6, 7)}

# case -> (data set, form of X, keyword arguments of scopen)
CASES = {
    "k6": ("a", "csr", dict(n_components=6)),
    "k6_a0": ("a", "csr", dict(n_components=6, alpha=0)),
    "k6_rho": ("a", "csr", dict(n_components=6, min_rho=0.1, max_rho=0.4)),
    "k6_iter5": ("a", "csr", dict(n_components=6, max_iter=5)),
    "k6_dense": ("a", "dense", dict(n_components=6)),
    "k6_messy": ("a", "messy", dict(n_components=6)),
    "k6_mudata": ("a", "mudata", dict(n_components=6)),
    "k17": ("b", "csr", dict(n_components=17)),
    "k30": ("a", "csr", dict(n_components=30, max_iter=80)),
    "k33": ("b", "csr", dict(n_components=33)),
    "k64": ("c", "csr", dict(n_components=64, max_iter=60)),
    "k65": ("c", "csr", dict(n_components=65, max_iter=20)),
}


def load_gold() -> dict:
    """The fixture as a dict; an array the generator found bit-equal to an earlier one is stored as that one's name."""
    import os

    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scopen_golden.npz")) as z:
        gold = {k: z[k] for k in z.files}
    for k in [k for k in gold if k.endswith("_same_as")]:
        gold[k[:-len("_same_as")]] = gold[str(gold.pop(k))]
    return gold


def counts(name: str) -> np.ndarray:
    """Dense int64 counts [n, d]: every cell has one of the planted topics, a topic opens its own sixth of the peaks
    often and the rest rarely, and the cells' depths spread over a factor of four (so the rho of the cells differ)."""
    n, d, topics, seed = DATA[name]
    rng = np.random.default_rng(seed)
    topic = rng.integers(0, topics, n)
    own = rng.integers(0, topics, d)
    depth = rng.uniform(0.5, 2.0, n)
    lam = depth[:, None] * np.where(own[None, :] == topic[:, None], 0.9, 0.06)
    C = rng.poisson(lam)
    C[np.arange(n), rng.integers(0, d, n)] += 1  # no empty cell
    return C.astype(np.int64)


def messy(C: np.ndarray) -> sp.csr_matrix:
    """The same matrix as ``toarray()`` gives it - but for ONE negative entry where C is zero - as an int32 CSR with
    rows in descending column order, every count >= 2 stored as two entries, and explicitly stored zeros."""
    n, d = C.shape
    rng = np.random.default_rng(5)
    zr, zc = np.nonzero(C == 0)
    pick = rng.choice(zr.size, size=41, replace=False)
    rows, cols, vals = [], [], []
    for i, j in zip(*np.nonzero(C)):
        c = int(C[i, j])
        for v in ((c - 1, 1) if c >= 2 else (c,)):
            rows.append(i), cols.append(j), vals.append(v)
    for q, p in enumerate(pick):
        rows.append(zr[p]), cols.append(zc[p]), vals.append(-3 if q == 0 else 0)
    rows, cols, vals = np.asarray(rows), np.asarray(cols), np.asarray(vals, dtype=np.int32)
    order = np.lexsort((-cols, rows))
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    m = sp.csr_matrix((vals[order], cols[order].astype(np.int32), indptr), shape=(n, d))
    assert not m.has_canonical_format
    return m


def case_data(case: str):
    """(the object ``scopen`` is called on, the AnnData that receives the results, keyword arguments)."""
    name, form, kw = CASES[case]
    C = counts(name)
    if form == "dense":
        X = C.astype(np.float32)
    elif form == "messy":
        X = messy(C)
    else:
        X = sp.csr_matrix(C.astype(np.float32))
    adata = AnnData(X)
    if form == "mudata":
        rna = AnnData(np.zeros((C.shape[0], 3), dtype=np.float32))
        return MuData({"rna": rna, "atac": adata}), adata, dict(kw)
    return adata, adata, dict(kw)


def dense_x(case: str, rho: np.ndarray) -> np.ndarray:
    """The d x n matrix the reference factorises, rebuilt from the seeded counts and the fixture's rho."""
    C = counts(CASES[case][0])
    return (C.T > 0) * (1 / (1 - rho))


def rebuild_imputed(gold, case: str) -> np.ndarray:
    """The reference's imputed n x d matrix from the stored factors; the stored rows are checked against it."""
    W, H = gold[f"{case}_W"], gold[f"{case}_H"]
    full = np.clip(W @ H, 0, 1).T
    stored = gold[f"{case}_X_rows"]
    assert np.abs(full[::ROW_STEP] - stored).max() <= 1e-12
    return full


def cd_numpy(X, W, H, *, l2_w, l2_h, tol=TOL, max_iter=500):
    """A sparse-free, row-sequential NumPy restatement of ``_fit_coordinate_descent`` with the sweep's stated order (the
    k-term sum ascending, product and sum two roundings): (W, H, n_iter, ratios).  Slow: small cases only."""
    W, Ht = W.copy(), np.ascontiguousarray(H.T)
    ratios, v0, n_iter = [], 0.0, 0
    for n_iter in range(1, max_iter + 1):
        v = sweep_numpy(W, X @ Ht, Ht.T @ Ht + l2_w * np.eye(W.shape[1]))
        v += sweep_numpy(Ht, X.T @ W, W.T @ W + l2_h * np.eye(W.shape[1]))
        if n_iter == 1:
            v0 = v
        if v0 == 0:
            break
        ratios.append(v / v0)
        if ratios[-1] <= tol:
            break
    return W, Ht.T, n_iter, np.asarray(ratios)


def sweep_numpy(W, B, G, terms=None):
    """One sweep over the rows of W in place (vectorised over the rows, which are independent; the r-sum ascending
    with two roundings per term): the sum of |projected gradient| in row order, or its terms [rows] in ``terms``."""
    rows, k = W.shape
    v = np.zeros(rows)
    for t in range(k):
        grad = -B[:, t]
        for r in range(k):
            grad = grad + G[t, r] * W[:, r]
        wt = W[:, t]
        v += np.abs(np.where(wt == 0, np.minimum(0.0, grad), grad))
        if G[t, t] != 0:
            W[:, t] = np.maximum(wt - grad / G[t, t], 0.0)
    if terms is not None:
        terms[...] = v
    return float(np.sum(v))
