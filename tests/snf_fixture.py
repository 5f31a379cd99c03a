"""TEST INFRASTRUCTURE: the seeded inputs and the case table of the SNF fixture (tests/golden/snf_golden.npz), shared by
its generator (tests/golden/make_snf_golden.py) and by tests/test_snf_host.py / tests/test_gpu_snf.py, and the numpy
statements of the reference's nested functions (/root/reference/muon/_core/tools.py:793-861) that the kernel tests
compare with.

Inputs: cluster-structured coordinates rounded to integers, ``round(1024 x)``, p = 6 + m features for modality m.
Distances are ``sqrt(sum(delta^2)) / 1024`` by the direct formula: the squares and their sums are exact integers, so
the distance matrix is the same bits on any machine, and the fixture needs to store no n x n input (not even the
coordinates: they are regenerated from the seed)."""
import json

import numpy as np
from scipy.sparse import issparse

from muon_amd._containers import AnnData, MuData

ROW_STEP = 8  # every 8th row of the fused W is stored

# case -> n, k, iterations, M, sigma, seed, key_added, neighbor_keys (None: the default key in every modality)
CASES = {
    "n21_k20": dict(n=21, k=20, it=2, M=2, sigma=0.5, seed=1, key_added=None, keys=None),
    "n65_k5": dict(n=65, k=5, it=3, M=2, sigma=0.5, seed=2, key_added="snf", keys={"m0": "nn_a", "m1": "neighbors"}),
    "n129_k64": dict(n=129, k=64, it=4, M=2, sigma=0.5, seed=3, key_added=None, keys=None),
    "n150_k10": dict(n=150, k=10, it=5, M=2, sigma=0.3, seed=4, key_added=None, keys="nn_s"),
    "n257_k20": dict(n=257, k=20, it=20, M=3, sigma=0.5, seed=5, key_added=None, keys=None),
}
EPS = float(np.finfo(np.float64).eps)


def coordinates(case: str, m: int) -> np.ndarray:
    """Integer coordinates [n, 6 + m] of modality m: four Gaussian clusters, in 1024ths."""
    c = CASES[case]
    rng = np.random.default_rng(1000 * c["seed"] + m)
    p = 6 + m
    centres = rng.normal(scale=2.5, size=(4, p))
    labels = np.arange(c["n"]) % 4 if m == 0 else rng.integers(0, 4, c["n"])
    x = centres[labels] + rng.normal(size=(c["n"], p))
    return np.round(1024 * x).astype(np.int64)


def distances(C: np.ndarray) -> np.ndarray:
    d = C[:, None, :] - C[None, :, :]
    return np.sqrt((d * d).sum(axis=-1).astype(np.float64)) / 1024


def key_of(case: str, mod: str) -> str:
    keys = CASES[case]["keys"]
    if keys is None:
        return "neighbors"
    return keys if isinstance(keys, str) else keys[mod]


def mudata(case: str, sparse=()) -> MuData:
    """The MuData object of a case.  Modality m0 names its representation (``use_rep="X_rep"``), the others leave it
    to the default (their X).  ``sparse``: modalities whose ``.obsp`` holds a 3-nearest-neighbour CSR instead of the
    dense matrix (what scanpy writes)."""
    import scipy.sparse as sp

    c = CASES[case]
    mods = {}
    for m in range(c["M"]):
        name = f"m{m}"
        C = coordinates(case, m)
        X = C / 1024.0
        D = distances(C)
        params = {"n_neighbors": 15, "method": "umap"}
        if m == 0:
            ad = AnnData(np.zeros((c["n"], 1)), obsm={"X_rep": X})
            params["use_rep"] = "X_rep"
        else:
            ad = AnnData(X)
        dk = "distances" if key_of(case, name) == "neighbors" else key_of(case, name) + "_distances"
        ad.uns[key_of(case, name)] = {"params": params, "distances_key": dk, "connectivities_key": "unused"}
        if name in sparse:
            keep = np.argsort(D, axis=1)[:, 1:4]
            G = np.zeros_like(D)
            np.put_along_axis(G, keep, np.take_along_axis(D, keep, axis=1), axis=1)
            ad.obsp[dk] = sp.csr_matrix(G)
        else:
            ad.obsp[dk] = D
        mods[name] = ad
    return MuData(mods)


def call_kwargs(case: str) -> dict:
    c = CASES[case]
    return dict(n_neighbors=c["k"], neighbor_keys=c["keys"], key_added=c["key_added"], n_iterations=c["it"],
                sigma=c["sigma"])


def slot_names(case: str):
    ka = CASES[case]["key_added"]
    return ("neighbors", "distances", "connectivities") if ka is None else (ka, ka + "_distances", ka + "_connectivities")


def params_json(neighbors_dict: dict) -> str:
    return json.dumps(neighbors_dict, sort_keys=True)


def check_against_fixture(gold, case, md, diag, label):
    """The comparison tests/test_snf_host.py and tests/test_gpu_snf.py share: asserts that the index arrays of both
    graphs equal the fixture's exactly, prints and returns the largest deviations (stored rows of W relative, distances
    absolute, connectivities relative)."""
    c = CASES[case]
    key, dk, ck = slot_names(case)
    W = diag["W"]
    ref_rows = gold[f"{case}_W_rows"]
    assert W.shape == (c["n"], c["n"]) and W.dtype == np.float64
    dev_w = float(np.max(np.abs(W[::ROW_STEP] - ref_rows) / np.abs(ref_rows)))
    d, g = md.obsp[dk], md.obsp[ck]
    dev_d = float(np.max(np.abs(d.data - gold[f"{case}_distances_data"])))
    dev_c = float(np.max(np.abs(g.data - gold[f"{case}_connectivities_data"]) / np.abs(gold[f"{case}_connectivities_data"])))
    print(f"MEASURE snf {label} {case}: W rows {dev_w:.3g} rel, distances {dev_d:.3g} abs, connectivities {dev_c:.3g} rel")
    for name, m in (("distances", d), ("connectivities", g)):
        assert issparse(m) and m.shape == (c["n"], c["n"])
        assert np.array_equal(m.indptr, gold[f"{case}_{name}_indptr"]), name
        assert np.array_equal(m.indices, gold[f"{case}_{name}_indices"]), name
    return dev_w, dev_d, dev_c


# ---- numpy statements of the reference's nested functions -----------------------------------------------------------------
def np_affinity(dist: np.ndarray, k: int, sigma: float, eps: float = EPS) -> np.ndarray:
    dist = (dist + dist.T) / 2
    np.fill_diagonal(dist, 0)
    srt = np.sort(dist, axis=1)[:, 1:k + 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        means = np.array([np.mean(r[~np.isinf(r)]) if (~np.isinf(r)).any() else np.nan for r in srt]) + eps
        sig = np.add.outer(means, means) / 3 + dist / 3 + eps
        scale = sigma * sig
        y = dist / scale
        dens = np.exp(-y ** 2 / 2.0) / np.sqrt(2 * np.pi) / scale  # scipy.stats.norm(0, scale).pdf(dist)
    return (dens + dens.T) / 2


def np_normalize(x: np.ndarray) -> np.ndarray:
    r = x.sum(axis=1) - x.diagonal()
    r[r == 0] = 1
    x = x / (2 * r[:, None])
    np.fill_diagonal(x, 0.5)
    return (x + x.T) / 2


def np_dominateset(x: np.ndarray, k: int) -> np.ndarray:
    z = x.copy()
    for j in range(x.shape[1]):
        z[np.argsort(x[:, j])[: x.shape[0] - k], j] = 0
    return z / z.sum(axis=1)
