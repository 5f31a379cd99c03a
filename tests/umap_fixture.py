"""TEST INFRASTRUCTURE: the seeded graphs of the UMAP tests (tests/test_umap_host.py, tests/test_gpu_umap.py), the
quality fixture and the MuData of the golden record (tests/golden/make_umap_golden.py -> umap_golden.npz)."""
import functools

import numpy as np
import scipy.sparse as sp

from muon_amd._containers import AnnData, MuData

GROUP = 16  # lanes per vertex of k_umap_epoch
BLOCK_VERTICES = 16  # vertices per workgroup


# ---- the quality fixture: three Gaussian blobs in 8-D, n = 450, a symmetrised 10-NN graph -------------------------------------
QUALITY = dict(n=450, dim=8, blobs=3, k=10, n_epochs=200, trust_neighbors=15, seed=5)
QUALITY_SEEDS = (0, 1, 2, 3, 4)
AB = (0.58303002, 1.33416699)  # (spread 1, min_dist 0.5)


def blobs(n, blocks, dim, seed, scale=6.0):
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(blocks, dim)) * scale
    truth = np.arange(n) % blocks
    return centres[truth] + rng.normal(size=(n, dim)), truth


def knn_connectivities(X, k):
    """A symmetric fuzzy graph of the k nearest neighbours: w = exp(-(d - d_1) / mean d) per directed entry, then the
    probabilistic union w + w^T - w w^T (umap's symmetrisation; the bandwidth is simplified)."""
    n = X.shape[0]
    k = min(k, n - 1)
    d = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(-1))
    np.fill_diagonal(d, np.inf)
    idx = np.argsort(d, axis=1, kind="stable")[:, :k]
    dk = np.take_along_axis(d, idx, axis=1)
    w = np.exp(-(dk - dk[:, :1]) / dk.mean(axis=1, keepdims=True))
    A = sp.csr_matrix((w.reshape(-1), (np.repeat(np.arange(n), k), idx.reshape(-1))), shape=(n, n))
    T = A.T.tocsr()
    A = (A + T - A.multiply(T)).tocsr()
    A.sort_indices()
    return A


@functools.lru_cache(maxsize=None)
def quality_data():
    q = QUALITY
    return blobs(q["n"], q["blobs"], q["dim"], q["seed"])[0]


@functools.lru_cache(maxsize=None)
def quality_graph():
    return knn_connectivities(quality_data(), QUALITY["k"])


def quality_initial(seed):
    """The random initialisation of the quality runs, rescaled as every initialisation is."""
    Y = np.random.default_rng(seed).uniform(-10, 10, (QUALITY["n"], 2))
    return 10.0 * (Y - Y.min(axis=0)) / (Y.max(axis=0) - Y.min(axis=0))


def trust(Y):
    from sklearn.manifold import trustworthiness

    return float(trustworthiness(quality_data(), np.asarray(Y, dtype=np.float64), n_neighbors=QUALITY["trust_neighbors"]))


def anndata_of(A, **obsm) -> AnnData:
    ad = AnnData(np.zeros((A.shape[0], 1)))
    ad.obs.index = [f"c{i}" for i in range(A.shape[0])]
    ad.obsp["connectivities"] = A.copy()
    ad.uns["neighbors"] = {"connectivities_key": "connectivities", "distances_key": "distances", "params": {}}
    ad.obsm.update(obsm)
    return ad


def mudata_of(A, n_mods=2) -> MuData:
    """A MuData whose global slots hold the graph, as pp.neighbors leaves them."""
    n = A.shape[0]
    mods = {}
    for m in range(n_mods):
        ad = AnnData(np.zeros((n, 1 + m)))
        ad.obs.index = [f"c{i}" for i in range(n)]
        mods[f"m{m}"] = ad
    md = MuData(mods)
    md.obsp["connectivities"] = A.copy()
    md.obsp["distances"] = A.copy()
    md.uns["neighbors"] = {"connectivities_key": "connectivities", "distances_key": "distances",
                           "params": {"use_rep": {f"m{m}": -1 for m in range(n_mods)},
                                      "n_pcs": {f"m{m}": -1 for m in range(n_mods)}}}
    return md


# ---- the edge-shape graphs of one epoch ------------------------------------------------------------------------------------
def row_lengths_graph(lengths, n, rng, E_of=None):
    """``(indptr, cols, E)``: row v holds ``lengths[v]`` sorted distinct columns (self included where they fall); E by
    ``E_of(count)`` (default: seeded periods of 1 .. 6 epochs, in 2^-16 units, so that only some are active)."""
    indptr, cols = [0], []
    for v in range(n):
        d = min(int(lengths[v]), n)
        cols.append(np.sort(rng.choice(n, d, replace=False)))
        indptr.append(indptr[-1] + d)
    cols = np.concatenate(cols).astype(np.int32) if cols else np.zeros(0, np.int32)
    E = rng.integers(1 << 16, 6 << 16, cols.size).astype(np.int64) if E_of is None else E_of(cols.size)
    return np.asarray(indptr, dtype=np.int64), cols, np.asarray(E, dtype=np.int64)


def epoch_cases():
    """name -> dict(indptr, cols, E, Y?, rate, e, n_epochs): the shapes where the kernel can go wrong."""
    G, B = GROUP, BLOCK_VERTICES
    out = {}
    rng = np.random.default_rng(101)
    # n = 1: one vertex, one entry onto itself, negatives that can only hit k == v
    out["n1"] = dict(indptr=np.array([0, 1], np.int64), cols=np.array([0], np.int32), E=np.array([1 << 16], np.int64),
                     rate=5, e=1, n_epochs=10)
    # one workgroup plus one vertex; an empty row; rows of 1, G - 1, G, G + 1, 2 G + 1 entries; e = 1
    lens = np.array([0, 1, G - 1, G, G + 1, 2 * G + 1, 3, 0, 7, 2, 5, G, 1, 1, 4, 9, 6])
    assert lens.size == B + 1
    ip, c, E = row_lengths_graph(lens, lens.size, rng)
    E[::3] = 1 << 16  # (a period of one epoch: active at e = 1, where every longer period still waits)
    out["rows_first_epoch"] = dict(indptr=ip, cols=c, E=E, rate=5, e=1, n_epochs=50)
    # the same shapes late in the schedule (e = n_epochs), with an entry whose period is beyond it: never active
    E2 = E.copy()
    E2[3] = 51 << 16
    out["rows_last_epoch"] = dict(indptr=ip, cols=c, E=E2, rate=5, e=50, n_epochs=50)
    # a hub row of >= 1000 entries among short rows
    n = 1100
    lens = rng.integers(0, 6, n)
    lens[37] = 1040
    ip, c, E = row_lengths_graph(lens, n, rng)
    out["hub"] = dict(indptr=ip, cols=c, E=E, rate=5, e=7, n_epochs=50)
    # all weights equal: every entry active in every epoch; rate 0 and rate 20
    lens = rng.integers(1, 2 * G + 2, 70)
    ip, c, E = row_lengths_graph(lens, 70, rng, E_of=lambda m: np.full(m, 1 << 16))
    out["all_active_rate0"] = dict(indptr=ip, cols=c, E=E, rate=0, e=3, n_epochs=20)
    out["all_active_rate20"] = dict(indptr=ip, cols=c, E=E, rate=20, e=3, n_epochs=20)
    # two coincident points joined by an entry (d2 == 0), n = 3: negatives hit k == v often
    Y = np.array([[1.0, 2.0, 3.0, 0.5], [1.0, 2.0, 3.0, 0.5], [4.0, 0.5, 2.5, 1.5]])
    out["coincident_n3"] = dict(indptr=np.array([0, 2, 4, 6], np.int64), cols=np.array([1, 2, 0, 2, 0, 1], np.int32),
                                E=np.full(6, 1 << 16, np.int64), Y=Y, rate=20, e=2, n_epochs=5)
    return out


def epoch_positions(case, dim, seed=7):
    n = int(case["indptr"].size) - 1
    if "Y" in case:
        return np.ascontiguousarray(case["Y"][:, :dim])
    return np.random.default_rng(seed).uniform(0, 10, (n, dim))


EPOCH_PARAMS = dict(a=AB[0], b=AB[1], gamma=1.0, seed=42)


def cliques(sizes):
    """Disjoint cliques without self-loops, weight 1."""
    n = sum(sizes)
    A = np.zeros((n, n))
    o = 0
    for s in sizes:
        A[o:o + s, o:o + s] = 1.0
        o += s
    np.fill_diagonal(A, 0.0)
    return sp.csr_matrix(A)


# ---- the record of the reference's own `umap` (tests/golden/make_umap_golden.py -> umap_golden.npz) --------------------------
GOLDEN_N = 12
GOLDEN_CASES = {
    "defaults": dict(),
    "keywords": dict(min_dist=0.1, spread=2.0, n_components=3, maxiter=30, alpha=0.5, gamma=2.0, negative_sample_rate=3,
                     init_pos="random", random_state=7, a=1.5, b=0.9),
    "copy": dict(copy=True, random_state=0),
    "neighbors_key": dict(neighbors_key="wnn"),
    "missing_key": dict(neighbors_key="nope"),
}


def golden_mudata() -> MuData:
    """Two modalities that cover every observation (the reference's imputation line is not reached)."""
    rng = np.random.default_rng(60)
    A = sp.random(GOLDEN_N, GOLDEN_N, density=0.4, random_state=rng, format="csr")
    A = (A + A.T).tocsr()
    md = mudata_of(A)
    for m, ad in enumerate(md.mod.values()):
        ad.X = rng.standard_normal(ad.shape)
    md.obsp["wnn_connectivities"] = (A * 0.5).tocsr()
    md.obsp["wnn_distances"] = A.copy()
    md.uns["wnn"] = {"connectivities_key": "wnn_connectivities", "distances_key": "wnn_distances",
                     "params": {"use_rep": {"m0": -1, "m1": "X"}, "n_pcs": {"m0": -1, "m1": 5}}}
    return md


def golden_embedding(n_components):
    """What the recording stand-in for scanpy's umap writes into ``.obsm["X_umap"]``."""
    return (np.arange(GOLDEN_N * n_components, dtype=np.float32).reshape(GOLDEN_N, n_components) / 8).astype(np.float32)
