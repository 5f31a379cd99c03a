"""TEST INFRASTRUCTURE: the seeded graphs of the clustering tests (tests/test_cluster_host.py, tests/test_gpu_cluster.py)
and the restatement's answer for each, computed once per process (tests/cluster_refs.py).

Graphs are directed k-nearest-neighbour graphs of Gaussian mixtures (a row holds its k neighbours, so they are
asymmetric), stored values 1, or multiples of 1/64 where a case is weighted: with dyadic resolutions and layer weights
every product and sum inside a score is then exact in f64 in any order."""
import functools

import numpy as np
import scipy.sparse as sp

from muon_amd._containers import AnnData, MuData
from tests import cluster_refs as R


def mixture(n, blocks, scale, seed, dim=4):
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(blocks, dim)) * scale
    truth = np.arange(n) % blocks
    return centres[truth] + rng.normal(size=(n, dim)), truth


def knn_graph(X, k, values="ones", seed=0):
    """Directed kNN CSR.  ``values``: "ones", "64ths" (seeded multiples of 1/64) or "float" (exp(-d), umap-like)."""
    n = X.shape[0]
    k = min(k, n - 1)
    d = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    idx = np.argsort(d, axis=1, kind="stable")[:, :k]
    rows = np.repeat(np.arange(n), k)
    cols = idx.reshape(-1)
    if values == "ones":
        v = np.ones(n * k)
    elif values == "64ths":
        v = np.random.default_rng(seed).integers(1, 65, n * k) / 64.0
    else:
        v = np.exp(-np.sqrt(d[rows, cols]))
    return sp.csr_matrix((v, (rows, cols)), shape=(n, n))


def planted(n, blocks, scale, k, seed, values="ones"):
    X, truth = mixture(n, blocks, scale, seed)
    return knn_graph(X, k, values, seed), truth


def _case_graphs(name):
    if name == "n1":
        return [sp.csr_matrix((1, 1))]
    if name == "n2":
        return [sp.csr_matrix(np.array([[0.0, 1.0], [0.0, 0.0]]))]
    if name == "n65":
        return [planted(65, 3, 4.0, 5, 11)[0]]
    if name == "n300_L2":
        return [planted(300, 5, 3.0, 10, 12)[0], planted(300, 5, 2.0, 8, 13)[0]]
    if name == "n300_w64_L2":
        return [planted(300, 5, 3.0, 10, 34, "64ths")[0], planted(300, 4, 2.5, 6, 35, "64ths")[0]]
    if name == "n120_L5":
        return [planted(120, 4, 2.0 + 0.5 * l, 6, 20 + l)[0] for l in range(5)]
    if name == "isolated":
        A = planted(65, 3, 4.0, 5, 16)[0].tolil()
        for v in (0, 7, 31, 63, 64):
            A[v, :] = 0
            A[:, v] = 0
        return [sp.csr_matrix(A), sp.csr_matrix((65, 65))]
    if name == "selfloops_asym":
        rng = np.random.default_rng(17)
        A = planted(65, 3, 3.0, 6, 17, "64ths")[0].tolil()
        for v in range(0, 65, 3):
            A[v, v] = rng.integers(1, 65) / 64.0
        B = sp.random(65, 65, density=0.06, random_state=18, format="csr")
        B.data = np.random.default_rng(19).integers(1, 65, B.nnz) / 64.0
        return [sp.csr_matrix(A), B]
    if name == "float":
        return [planted(200, 4, 3.0, 10, 21, "float")[0], planted(200, 4, 3.0, 10, 22, "float")[0]]
    raise KeyError(name)


# case -> call arguments (resolution, mod_weights, weighted)
CASES = {
    "n1": dict(resolution=None, mod_weights=None, weighted=False),
    "n2": dict(resolution=None, mod_weights=None, weighted=False),
    "n65": dict(resolution=1.0, mod_weights=None, weighted=False),
    "n300_L2": dict(resolution=[1.0, 0.5], mod_weights={"m1": 2.0}, weighted=False),
    "n300_w64_L2": dict(resolution={"m0": 0.5, "m1": 1.5}, mod_weights=[1.0, 0.25], weighted=True),
    "n120_L5": dict(resolution=0.75, mod_weights=[1, 2, 1, 0.5, 1], weighted=False),
    "isolated": dict(resolution=None, mod_weights=None, weighted=False),
    "selfloops_asym": dict(resolution=1.0, mod_weights=[1.0, 0.5], weighted=True),
    "float": dict(resolution=1.0, mod_weights=None, weighted=True),
}
EXACT_CASES = [c for c in CASES if c != "float"]
ALGORITHMS = ("leiden", "louvain")


@functools.lru_cache(maxsize=None)
def graphs(name):
    return tuple(_case_graphs(name))


def mudata(name) -> MuData:
    mods = {}
    for m, A in enumerate(graphs(name)):
        ad = AnnData(np.zeros((A.shape[0], 1)))
        ad.obs.index = [f"c{i}" for i in range(A.shape[0])]
        ad.obsp["connectivities"] = A.copy()
        mods[f"m{m}"] = ad
    return MuData(mods)


def call_kwargs(name):
    c = CASES[name]
    kw = dict(resolution=c["resolution"], mod_weights=c["mod_weights"])
    if c["weighted"]:
        kw["partition_kwargs"] = {"weights": "weight"}
    return kw


def layer_parameters(name):
    """(lambdas, gammas) per layer as plain floats, resolved by hand from CASES."""
    c, L = CASES[name], len(graphs(name))
    res, w = c["resolution"], c["mod_weights"]
    gam = [1.0] * L if res is None else ([float(res[f"m{l}"]) for l in range(L)] if isinstance(res, dict) else
                                         ([float(x) for x in res] if isinstance(res, list) else [float(res)] * L))
    lam = [1.0] * L if w is None else ([float(w.get(f"m{l}", 1)) for l in range(L)] if isinstance(w, dict) else
                                       [float(x) for x in w])
    return lam, gam


def entries(name, directed):
    return [R.layer_entries(A, CASES[name]["weighted"], directed) for A in graphs(name)]


@functools.lru_cache(maxsize=None)
def restated(name, algorithm, directed, random_state=0, n_iterations=1):
    """The restatement's ``(membership, Q, Q(singletons), margins)`` for a case: computed once, never changed."""
    lam, gam = layer_parameters(name)
    g = R.build(graphs(name)[0].shape[0], entries(name, directed), lam, gam)
    member, q, q0, margins = R.optimise(g, algorithm, random_state, n_iterations)
    return tuple(member), q, q0, dict(margins)


def labels_of(md, key):
    return md.obs[key].to_numpy().astype(str).astype(np.int64)


GOLDEN_N = 28
GOLDEN_IMPROVEMENT = 12.625
# ---- the record of the reference's own `_cluster` (tests/golden/make_cluster_golden.py -> cluster_golden.npz) --------------
# case -> the call's arguments
GOLDEN_CASES = {
    "leiden_scalar": dict(algorithm="leiden", resolution=0.75, mod_weights=2.0, random_state=0),
    "louvain_scalar": dict(algorithm="louvain", resolution=0.75, mod_weights=2.0, random_state=5),
    "leiden_list": dict(algorithm="leiden", resolution=[0.5, 2.0], mod_weights=[1.0, 0.25], random_state=7),
    "leiden_mapping": dict(algorithm="leiden", resolution={"m0": 0.5, "m1": 1.5}, mod_weights={"m0": 3.0, "m1": 0.5},
                           random_state=1),
    "leiden_none": dict(algorithm="leiden", resolution=None, mod_weights=None, random_state=0),
    "louvain_none_undirected": dict(algorithm="louvain", resolution=None, mod_weights=None, random_state=3, directed=False,
                                    key_added="groups"),
    "leiden_weights_missing_modality": dict(algorithm="leiden", resolution=1.0, mod_weights={"m1": 2.0}, random_state=0),
    "leiden_resolution_missing_modality": dict(algorithm="leiden", resolution={"m0": 0.5}, mod_weights=None, random_state=0),
    "leiden_neighbors_key": dict(algorithm="leiden", resolution=1.0, mod_weights=None, random_state=0, neighbors_key="nn"),
}


def golden_membership():
    """14 communities of sizes 2, in an order that is not sorted."""
    return [(5 * i + 3) % 14 for i in range(GOLDEN_N)]


def golden_mudata() -> MuData:
    mods = {}
    for m in range(2):
        rng = np.random.default_rng(40 + m)
        A = sp.random(GOLDEN_N, GOLDEN_N, density=0.2, random_state=rng, format="csr")
        ad = AnnData(np.zeros((GOLDEN_N, 1)))
        ad.obs.index = [f"c{i}" for i in range(GOLDEN_N)]
        ad.obsp["connectivities"] = A
        ad.obsp["nn_connectivities"] = A.T.tocsr()
        ad.uns["nn"] = {"connectivities_key": "nn_connectivities"}
        mods[f"m{m}"] = ad
    return MuData(mods)
