"""TEST INFRASTRUCTURE: plain-Python / numpy restatements of muon_amd/_core/umap.py's statement - the integer schedule,
one epoch per vertex and per entry in the stated sum order, the spectral initialisation, ``find_ab`` - and
``sequential_layout``, umap-learn's published per-edge loop, which only tests/golden/make_umap_golden.py runs (to record
the trustworthiness the Jacobi form is held against)."""
import math

import numpy as np

S = 1 << 16
M64 = (1 << 64) - 1
GROUP = 16
SPECTRAL_STEPS = 40
SPECTRAL_OVERSAMPLE = 4


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def negative_index(seed, e, j, s, n):
    h = splitmix64((splitmix64(splitmix64((seed + e) & M64) ^ j) + s) & M64)
    return ((h >> 32) * n) >> 32


def periods(w, n_epochs):
    """``(kept mask, E)`` of the weights of the stored entries, plain Python."""
    w = [float(x) for x in w]
    w_max = max(w) if w else 0.0
    keep = [w_max > 0 and x > 0 and x >= w_max / n_epochs for x in w]
    E = [int(round((w_max / x) * 65536.0)) for x, k in zip(w, keep) if k]
    return np.asarray(keep, dtype=bool), E


def schedule(E, e, rate):
    """``(active, negatives)`` of an entry of period E (Python int) at epoch e."""
    c1, c0 = (e * S) // E, ((e - 1) * S) // E
    if not c1 > c0:
        return False, 0
    p = -((-(c1 - 1) * E) // S)  # ceil
    return True, (e * S * rate) // E - (p * S * rate) // E


def _clip(x):
    return min(4.0, max(-4.0, x))


def _d2(yv, yx):
    d2 = 0.0
    for p, q in zip(yv, yx):
        d2 = d2 + (p - q) * (p - q)
    return d2


def epoch(Y, indptr, cols, E, e, n_epochs, rate, a, b, gamma, alpha_e, seed):
    """Y_{t+1} from Y = Y_t: per vertex, lanes of GROUP, entries g, g + GROUP, ..., the xor butterfly."""
    Y = np.asarray(Y, dtype=np.float64)
    n, dim = Y.shape
    out = Y.copy()
    for v in range(n):
        yv = [float(x) for x in Y[v]]
        lanes = [[0.0] * dim for _ in range(GROUP)]
        for g in range(GROUP):
            acc = lanes[g]
            for j in range(int(indptr[v]) + g, int(indptr[v + 1]), GROUP):
                active, nneg = schedule(int(E[j]), e, rate)
                if not active:
                    continue
                yu = [float(x) for x in Y[int(cols[j])]]
                d2 = _d2(yv, yu)
                if d2 > 0.0:
                    pw = math.pow(d2, b)
                    coef = (-2.0 * a * b * (pw / d2)) / (1.0 + a * pw)
                    for d in range(dim):
                        acc[d] = acc[d] + _clip(coef * (yv[d] - yu[d]))
                for s in range(nneg):
                    k = negative_index(seed, e, j, s, n)
                    if k == v:
                        continue
                    yk = [float(x) for x in Y[k]]
                    d2 = _d2(yv, yk)
                    if d2 > 0.0:
                        pw = math.pow(d2, b)
                        coef = (2.0 * gamma * b) / ((0.001 + d2) * (1.0 + a * pw))
                        for d in range(dim):
                            acc[d] = acc[d] + _clip(coef * (yv[d] - yk[d]))
        off = GROUP // 2
        while off > 0:
            lanes = [[lanes[g][d] + lanes[g ^ off][d] for d in range(dim)] for g in range(GROUP)]
            off //= 2
        for d in range(dim):
            out[v, d] = yv[d] + alpha_e * lanes[0][d]
    return out


def rescale(Y):
    Y = np.asarray(Y, dtype=np.float64)
    out = np.zeros_like(Y)
    for d in range(Y.shape[1]):
        lo, hi = Y[:, d].min(), Y[:, d].max()
        if hi > lo:
            out[:, d] = 10.0 * (Y[:, d] - lo) / (hi - lo)
    return out


def spectral_init(n, rows, cols, w, dim, rng, noise=True):
    """The spectral initialisation before the rescaling, with a dense operator."""
    m = dim + 1 + SPECTRAL_OVERSAMPLE
    if n <= m:
        return rng.uniform(-10, 10, (n, dim))
    A = np.zeros((n, n))
    for r, c, x in zip(rows, cols, w):
        A[r, c] += x
    deg = A.sum(axis=1)
    dinv = np.array([1.0 / math.sqrt(x) if x > 0 else 0.0 for x in deg])
    Op = (np.eye(n) + dinv[:, None] * A * dinv[None, :]) / 2
    Q = np.linalg.qr(rng.standard_normal((n, m)))[0]
    for _ in range(SPECTRAL_STEPS):
        Q = np.linalg.qr(Op @ Q)[0]
    H = Q.T @ (Op @ Q)
    vals, vecs = np.linalg.eigh((H + H.T) / 2)
    order = np.argsort(-vals, kind="stable")
    V = Q @ vecs[:, order[1:dim + 1]]
    for d in range(dim):
        if V[np.argmax(np.abs(V[:, d])), d] < 0:
            V[:, d] = -V[:, d]
    top = np.abs(V).max()
    if top > 0:
        V = V * (10.0 / top)
    if noise:
        V = V + rng.normal(0.0, 1e-4, (n, dim))
    return V


def find_ab(spread, min_dist):
    """umap-learn's find_ab_params by a second route to the same fit: scipy's ``least_squares`` on the residuals."""
    from scipy.optimize import least_squares

    x = np.linspace(0, spread * 3, 300)
    y = np.where(x < min_dist, 1.0, np.exp(-(x - min_dist) / spread))
    fit = least_squares(lambda p: 1.0 / (1.0 + p[0] * x ** (2 * p[1])) - y, np.ones(2), method="lm", xtol=1e-14,
                        ftol=1e-14, gtol=1e-14)
    return float(fit.x[0]), float(fit.x[1])


def sequential_layout(Y0, rows, cols, w, n_epochs, a, b, gamma=1.0, alpha=1.0, rate=5, seed=0):
    """umap-learn's published ``optimize_layout_euclidean`` loop (one thread, ``move_other=True``, its per-entry state
    ``epoch_of_next_sample`` / ``epoch_of_next_negative_sample``), negatives from a seeded numpy generator."""
    Y = np.array(Y0, dtype=np.float64)
    n, dim = Y.shape
    rng = np.random.default_rng(seed)
    w = np.asarray(w, dtype=np.float64)
    keep = w >= w.max() / n_epochs
    rows, cols, w = np.asarray(rows)[keep], np.asarray(cols)[keep], w[keep]
    eps = w.max() / w
    eps_neg = eps / rate
    nxt, nxt_neg = eps.copy(), eps_neg.copy()
    lr = alpha
    for it in range(n_epochs):
        for i in range(len(w)):
            if nxt[i] > it:
                continue
            j, k = int(rows[i]), int(cols[i])
            cur, oth = Y[j], Y[k]
            d2 = float(((cur - oth) ** 2).sum())
            if d2 > 0.0:
                coef = (-2.0 * a * b * d2 ** (b - 1.0)) / (a * d2 ** b + 1.0)
                g = np.clip(coef * (cur - oth), -4.0, 4.0)
                cur += g * lr
                oth -= g * lr
            nxt[i] += eps[i]
            for _ in range(int((it - nxt_neg[i]) / eps_neg[i])):
                k = int(rng.integers(n))
                oth = Y[k]
                d2 = float(((cur - oth) ** 2).sum())
                if d2 > 0.0:
                    coef = (2.0 * gamma * b) / ((0.001 + d2) * (a * d2 ** b + 1.0))
                    cur += np.clip(coef * (cur - oth), -4.0, 4.0) * lr
                elif j != k:
                    cur += 4.0 * lr
            nxt_neg[i] += int((it - nxt_neg[i]) / eps_neg[i]) * eps_neg[i]
        lr = alpha * (1.0 - (it + 1) / n_epochs)
    return Y
