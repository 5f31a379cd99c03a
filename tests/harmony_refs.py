"""TEST INFRASTRUCTURE: the NumPy restatement of muon_amd.pp.harmony_integrate's statement (the docstring of
muon_amd/_core/harmony.py), independent of the package's tensors and kernels: dense Phi, plain loops, the
cluster-by-cluster correction, in the number type ``dtype`` (np.float64, or np.longdouble for the tests' measure of
the statement's own rounding).  Also the planted data generator and the mixing measure the tests share."""
import numpy as np


def planted(N, d, C, B, shift=1.5, noise=0.5, seed=1):
    """C planted groups in d dimensions, every cell moved by its batch's offset; returns (Z, labels, codes)."""
    rng = np.random.default_rng(seed)
    cent = rng.normal(size=(C, d)) * 4
    sh = rng.normal(size=(B, d))
    sh -= sh.mean(0)
    sh *= shift
    labels = rng.integers(C, size=N)
    codes = rng.choice(B, size=N)
    Z = cent[labels] + sh[codes] + rng.normal(size=(N, d)) * noise
    return Z, labels, codes


def one_hot(codes_list, n_levels):
    N = len(codes_list[0])
    Phi = np.zeros((N, int(sum(n_levels))))
    off = 0
    for c, nl in zip(codes_list, n_levels):
        Phi[np.arange(N), off + np.asarray(c)] = 1.0
        off += nl
    return Phi


def same_batch_share(X, codes, k=15):
    """Mean share of a cell's k nearest neighbours (Euclidean, itself left out) that carry its own batch code."""
    X = np.asarray(X, dtype=np.float64)
    sq = (X * X).sum(1)
    D = sq[:, None] + sq[None, :] - 2.0 * (X @ X.T)
    np.fill_diagonal(D, np.inf)
    nn = np.argpartition(D, k, axis=1)[:, :k]
    return float((codes[nn] == codes[:, None]).mean())


def _l2rows(X):
    return X / np.sqrt((X * X).sum(axis=1, keepdims=True))


def _inverse(A):
    """inv(A) by Gauss-Jordan elimination with partial pivoting, in A's number type (np.linalg has no longdouble)."""
    n = A.shape[0]
    M = np.concatenate([A.copy(), np.eye(n, dtype=A.dtype)], axis=1)
    for c in range(n):
        p = c + int(np.argmax(np.abs(M[c:, c])))
        if p != c:
            M[[c, p]] = M[[p, c]]
        M[c] = M[c] / M[c, c]
        for r in range(n):
            if r != c:
                M[r] = M[r] - M[r, c] * M[c]
    return M[:, n:]


def _objective(R, D, sigma, th, E, O, Phi):
    logR = np.log(np.where(R > 0, R, 1))
    G = (th * np.log((O + 1) / (E + 1))) @ Phi.T  # [K, N]
    return (R * D).sum() + (sigma * (R * logR)).sum() + (sigma * (R * G.T)).sum()


def harmony_ref(Z, Phi, *, theta, lamb, sigma, nclust=None, tau=0, block_size=0.05, max_iter_harmony=10,
                max_iter_kmeans=20, epsilon_cluster=1e-5, epsilon_harmony=1e-4, random_state=0, dtype=np.float64):
    """``theta``, ``lamb``: one value per LEVEL (column of Phi); ``sigma``: a scalar or a K-vector.  Returns a dict with
    Z_corr, R, Y (the last round's centres), kmeans_rounds, n_iter, converged, objective_harmony, nclust."""
    Z = np.asarray(Z).astype(dtype)
    Phi = np.asarray(Phi).astype(dtype)
    N, d = Z.shape
    B = Phi.shape[1]
    K = int(nclust) if nclust is not None else int(min(np.round(N / 30.0), 100))
    rs = np.random.RandomState(random_state)
    Nb = Phi.sum(0)
    Pr = Nb / N
    th = np.broadcast_to(np.asarray(theta, dtype=dtype), (B,)).copy()
    if tau > 0:
        th = th * (1 - np.exp(-(Nb / (K * tau)) ** 2))
    lam = np.broadcast_to(np.asarray(lamb, dtype=dtype), (B,)).copy()
    sigma = np.broadcast_to(np.asarray(sigma, dtype=dtype), (K,)).copy()
    two, one = dtype(2), dtype(1)
    Zc = _l2rows(Z)

    # the start
    seeds = [int(rs.randint(N))]
    d2 = None
    for _ in range(1, K):
        dist = np.maximum(two * (one - Zc @ Zc[seeds[-1]]), 0)
        d2 = dist if d2 is None else np.minimum(d2, dist)
        c = np.cumsum(d2)
        seeds.append(min(int(np.searchsorted(c, rs.random_sample() * c[-1], side="right")), N - 1))
    Y = Zc[seeds].copy()
    labels = None
    for _ in range(25):
        new = np.argmax(Zc @ Y.T, axis=1)
        if labels is not None and np.array_equal(new, labels):
            break
        labels = new
        onehot = np.zeros((N, K), dtype=dtype)
        onehot[np.arange(N), labels] = 1
        sums = onehot.T @ Zc
        count = np.bincount(labels, minlength=K)
        for k in range(K):
            if count[k] > 0:
                Y[k] = sums[k] / np.sqrt((sums[k] * sums[k]).sum())

    def weights(Y):
        D = two * (one - Zc @ Y.T)
        T = -D / sigma
        return D, np.exp(T - T.max(axis=1, keepdims=True))

    D, S = weights(Y)
    R = S / S.sum(axis=1, keepdims=True)
    E = np.outer(R.sum(0), Pr)
    O = R.T @ Phi
    obj_k = [_objective(R, D, sigma, th, E, O, Phi)]
    obj_h = [obj_k[0]]
    n_blocks = int(np.ceil(1.0 / block_size))
    rounds, converged = [], False
    Phi_moe = np.concatenate([np.ones((N, 1), dtype=dtype), Phi], axis=1)
    ridge = np.diag(np.concatenate([np.zeros(1, dtype=dtype), lam]))
    Zcorr = Z.copy()
    for _ in range(max_iter_harmony):
        r = -1
        for r in range(max_iter_kmeans):
            Y = _l2rows(R.T @ Zc)
            D, S = weights(Y)
            for b in np.array_split(rs.permutation(N), n_blocks):
                E -= np.outer(R[b].sum(0), Pr)
                O -= R[b].T @ Phi[b]
                F = ((E + 1) / (O + 1)) ** th
                Rb = S[b] * (Phi[b] @ F.T)
                R[b] = Rb / Rb.sum(axis=1, keepdims=True)
                E += np.outer(R[b].sum(0), Pr)
                O += R[b].T @ Phi[b]
            obj_k.append(_objective(R, D, sigma, th, E, O, Phi))
            if r > 3:
                old, new = sum(obj_k[-6:-3]), sum(obj_k[-3:])
                if (old - new) / abs(old) < epsilon_cluster:
                    break
        rounds.append(r + 1)
        obj_h.append(obj_k[-1])
        Zcorr = Z.copy()
        for k in range(K):
            PR = Phi_moe * R[:, k:k + 1]
            A = PR.T @ Phi_moe + ridge
            W = _inverse(A) @ (PR.T @ Z)
            W[0] = 0
            Zcorr -= R[:, k:k + 1] * (Phi_moe @ W)
        Zc = _l2rows(Zcorr)
        if (obj_h[-2] - obj_h[-1]) / abs(obj_h[-2]) < epsilon_harmony:
            converged = True
            break
    return {"Z_corr": Zcorr, "R": R, "Y": Y, "kmeans_rounds": rounds, "n_iter": len(rounds), "converged": converged,
            "objective_harmony": [float(v) for v in obj_h], "nclust": K}


# ---- the end-to-end cases the host and the device tests share ------------------------------------------------------------
# name: (N, d, C, B, nclust, cap of the same-batch share among 15 nearest neighbours after the correction)
CASES = {"n600": (600, 8, 3, 2, None, 0.65), "n900": (900, 12, 4, 3, 17, 0.45), "n300": (300, 5, 3, 2, 10, 0.65)}
_cache = {}


def case(name):
    """(Z, codes, the f64 restatement's result, its deviation from the longdouble run as a share of max |Z_corr|) of
    an end-to-end case, computed once."""
    if name not in _cache:
        N, d, C, B, nclust, _ = CASES[name]
        Z, _, codes = planted(N, d, C, B)
        Phi = one_hot([codes], [B])
        kw = dict(theta=2.0, lamb=1.0, sigma=0.1, nclust=nclust)
        ref = harmony_ref(Z, Phi, **kw)
        ext = harmony_ref(Z, Phi, dtype=np.longdouble, **kw)
        assert ext["kmeans_rounds"] == ref["kmeans_rounds"] and ext["n_iter"] == ref["n_iter"]
        _cache[name] = (Z, codes, ref, deviation(ext["Z_corr"], ref["Z_corr"]))
    return _cache[name]


def deviation(A, ref):
    return float(np.abs(np.asarray(A, dtype=np.float64) - ref).max() / np.abs(ref).max())


def check_case(name, res, label):
    """The conditions of an end-to-end case on a result of ``_harmonize``: the restatement's round and iteration
    counts, the value bound (100 times the restatement's own f64-versus-longdouble deviation: the measured thing is a
    proxy - extended precision, not the summation order and the libm that differ -, hence one order more than the
    project's ten), and the cap of the same-batch share."""
    Z, codes, ref, own = case(name)
    dev = deviation(res["Z_corr"], ref["Z_corr"])
    share0, share = same_batch_share(Z, codes), same_batch_share(res["Z_corr"], codes)
    print(f"MEASURE harmony {label} {name}: rounds {res['kmeans_rounds']} n_iter {res['n_iter']} deviation {dev:.3g} "
          f"(restatement f64 vs longdouble {own:.3g}) same-batch share {share0:.2f} -> {share:.2f}")
    assert res["kmeans_rounds"] == ref["kmeans_rounds"] and res["n_iter"] == ref["n_iter"]
    assert res["converged"] == ref["converged"] and res["nclust"] == ref["nclust"]
    assert dev <= 100 * own
    assert share0 > 0.95 and share <= CASES[name][5]


def levels65():
    """(Z, codes, the f64 restatement's result, its f64-versus-longdouble deviation) of 650 cells in 65 levels of one
    key, 8 clusters, two iterations; computed once."""
    if "levels65" not in _cache:
        Z, _, _ = planted(650, 5, 3, 2)
        codes = np.random.default_rng(3).permutation(np.arange(650) % 65)
        kw = dict(theta=2.0, lamb=1.0, sigma=0.1, nclust=8, max_iter_harmony=2)
        ref = harmony_ref(Z, one_hot([codes], [65]), **kw)
        ext = harmony_ref(Z, one_hot([codes], [65]), dtype=np.longdouble, **kw)
        assert ext["kmeans_rounds"] == ref["kmeans_rounds"]
        _cache["levels65"] = (Z, codes, ref, deviation(ext["Z_corr"], ref["Z_corr"]))
    return _cache["levels65"]
