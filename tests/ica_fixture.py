"""TEST INFRASTRUCTURE: the seeded inputs and the case table of the FastICA fixture (tests/golden/ica_golden.npz),
shared by its generator (tests/golden/make_ica_golden.py) and by tests/test_ica_host.py / tests/test_gpu_ica.py.
The inputs are regenerated from the seed wherever they are needed: the fixture stores results only."""
import numpy as np

SEED = 11          # random_state of every case
ROW_STEP = 37      # k33 / k64: every 37th row of X_ica is stored, the rest is rebuilt from components_ and mean_

# data set -> (n samples, f features, generator seed); k19: 8 sources in 19 features under a little Gaussian noise
# (the seeds are the first for which every case on the data set converges with the margins the generator asserts)
DATA = {"k6": (1031, 6, 2), "k19": (1031, 19, 2), "k17": (1031, 17, 1), "k33": (2500, 33, 2), "k64": (4000, 64, 1)}
N_SOURCES = {"k19": 8}
NOISE = 0.05

# case -> (data set, float32 basis, keyword arguments of tl.ica beyond random_state)
CASES = {
    "k6_logcosh": ("k6", False, {}),
    "k6_exp": ("k6", False, dict(fun="exp")),
    "k6_cube": ("k6", False, dict(fun="cube")),
    "k8of19": ("k19", False, dict(n_components=8)),
    "k17": ("k17", False, {}),
    "k33": ("k33", False, {}),
    "k64": ("k64", False, {}),
    "k6_iter3": ("k6", False, dict(max_iter=3)),
    "k6_alpha": ("k6", False, dict(fun_args={"alpha": 1.5})),
    "k6_arb": ("k6", False, dict(whiten="arbitrary-variance")),
    "k6_scale": ("k6", False, dict(scale=True)),
    "k6_defl": ("k6", False, dict(algorithm="deflation")),
    "k6_f32": ("k6", True, {}),
}
SUBSAMPLED = ("k33", "k64")
NOT_CONVERGING = ("k6_iter3",)


def sources(n: int, k: int, rng) -> np.ndarray:
    """n x k independent non-Gaussian sources, eight families in turn, each standardised."""
    cols = []
    for j in range(k):
        kind = j % 8
        if kind == 0:
            s = rng.laplace(size=n)
        elif kind == 1:
            s = rng.uniform(-1, 1, n) ** 3
        elif kind == 2:
            s = rng.choice([-1.0, 1.0], n) * rng.exponential(size=n) ** 1.5
        elif kind == 3:
            s = rng.standard_t(5, n)
        elif kind == 4:
            s = rng.gamma(2.0, 1.0, n) - 2.0
        elif kind == 5:
            s = rng.uniform(-1, 1, n)
        elif kind == 6:
            s = rng.laplace(size=n) * (rng.random(n) < 0.2)
        else:
            s = rng.logistic(size=n)
        cols.append((s - s.mean()) / s.std())
    return np.stack(cols, axis=1)


def basis(name: str) -> np.ndarray:
    """The f64 basis of a data set: sources mixed by a seeded Gaussian matrix, plus an offset."""
    n, f, seed = DATA[name]
    rng = np.random.default_rng(seed)
    ns = N_SOURCES.get(name, f)
    S = sources(n, ns, rng)
    M = rng.standard_normal((f, ns))
    X = S @ M.T + rng.standard_normal(f) * 3.0
    if ns < f:
        X = X + NOISE * rng.standard_normal((n, f))
    return X


def case_input(case: str) -> np.ndarray:
    name, f32, _ = CASES[case]
    X = basis(name)
    return X.astype(np.float32) if f32 else X


def rebuild(gold, case: str, X: np.ndarray) -> np.ndarray:
    """The reference's X_ica of a case: stored in full, or rebuilt from components_ and mean_ where only every
    ROW_STEP-th row is stored (those rows are checked against the rebuilt ones)."""
    if case not in SUBSAMPLED:
        return gold[f"{case}_X_ica"]
    full = (X - gold[f"{case}_mean"]) @ gold[f"{case}_components"].T
    stored = gold[f"{case}_X_ica_rows"]
    assert np.abs(full[::ROW_STEP] - stored).max() <= 1e-12 * np.abs(stored).max()
    return full
