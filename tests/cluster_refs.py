"""TEST INFRASTRUCTURE: a plain python restatement of the optimiser of muon_amd/_core/cluster.py (its module docstring
is the statement), with per-vertex dictionaries and python floats - nothing vectorised, nothing shared with the product
- and a brute-force Q from the definition.

``optimise`` also returns the smallest decision margins it met, each relative to the scale of what was compared:
``runner_up`` (best score minus the next candidate's), ``own`` (best score minus the own community's where they
differ) and ``q_step`` (|Q after a sweep - Q before|, the guard of step 3).  A case whose margins are large against
the rounding of f64 sums has labels that no summation order can change."""
import numpy as np

MAX_SWEEPS = 50


def layer_entries(A, use_weights, directed):
    """[(i, j, a)] of a scipy matrix: stored non-zeros, value 1 unless ``use_weights``; undirected: both directions."""
    import scipy.sparse as sp

    C = sp.csr_matrix(A)
    C.sum_duplicates()
    C = C.tocoo()
    out = []
    for i, j, a in zip(C.row.tolist(), C.col.tolist(), C.data.tolist()):
        if a != 0:
            out.append((i, j, float(a) if use_weights else 1.0))
    if not directed:
        out = out + [(j, i, a) for i, j, a in out]
    return out


class Graph:
    def __init__(self, nv, adj, selfw, P, coef):
        self.nv, self.adj, self.selfw, self.P, self.coef = nv, adj, selfw, P, coef


def build(n, layers, lambdas, gammas):
    """``layers``: a list of entry lists.  S = sum_l lambda_l (A_l + A_l^T) as a dict per vertex, its diagonal aside."""
    adj = [dict() for _ in range(n)]
    selfw = [0.0] * n
    P = [[0.0] * (2 * len(layers)) for _ in range(n)]
    coef = []
    for l, (ent, lam, gam) in enumerate(zip(layers, lambdas, gammas)):
        m = 0.0
        for i, j, a in ent:
            P[i][2 * l] += a
            P[j][2 * l + 1] += a
            m += a
            for u, v in ((i, j), (j, i)):
                if u == v:
                    selfw[u] += lam * a
                else:
                    adj[u][v] = adj[u].get(v, 0.0) + lam * a
        coef.append((gam * lam) / m if m != 0 else 0.0)
    return Graph(n, adj, selfw, P, coef)


def totals(g, labels):
    K = [[0.0] * len(g.P[0]) for _ in range(g.nv)] if g.nv else []
    size = [0] * g.nv
    for v in range(g.nv):
        size[labels[v]] += 1
        for t, x in enumerate(g.P[v]):
            K[labels[v]][t] += x
    return K, size


def quality(g, labels):
    inner = [0.0] * g.nv
    for v in range(g.nv):
        inner[labels[v]] += g.selfw[v]
        for u, w in g.adj[v].items():
            if labels[u] == labels[v]:
                inner[labels[v]] += w
    K, _ = totals(g, labels)
    q = 0.0
    for c in range(g.nv):
        pen = 0.0
        for l, cf in enumerate(g.coef):
            pen += cf * (K[c][2 * l] * K[c][2 * l + 1])
        q += inner[c] / 2 - pen
    return q


def scores_of(g, v, labels, K, size, bound):
    """{candidate: score} of vertex v after the swap guard, and the own community."""
    a = labels[v]
    w = {a: 0.0}
    for u, x in sorted(g.adj[v].items()):
        if bound is not None and bound[u] != bound[v]:
            continue
        w[labels[u]] = w.get(labels[u], 0.0) + x
    out = {}
    for C, wc in w.items():
        if C != a and size[a] == 1 and size[C] == 1 and C > a:
            continue
        pen = 0.0
        for l, cf in enumerate(g.coef):
            kin_c, kout_c = K[C][2 * l + 1], K[C][2 * l]
            if C == a:
                kin_c, kout_c = kin_c - g.P[v][2 * l + 1], kout_c - g.P[v][2 * l]
            pen += cf * (g.P[v][2 * l] * kin_c + g.P[v][2 * l + 1] * kout_c)
        out[C] = wc - pen
    return out, a


def decide(g, v, labels, K, size, bound, margins):
    sc, a = scores_of(g, v, labels, K, size, bound)
    ranked = sorted(sc.items(), key=lambda t: (-t[1], t[0]))
    best, bs = ranked[0]
    scale = max(1.0, max(abs(s) for s in sc.values()))
    if len(ranked) > 1 and ranked[1][1] != bs:
        margins["runner_up"] = min(margins["runner_up"], (bs - ranked[1][1]) / scale)
    if bs != sc[a]:
        margins["own"] = min(margins["own"], (bs - sc[a]) / scale)
    if best != a and bs > sc[a]:
        return best, bs
    return a, sc[a]


def sweep(g, cls, labels, bound, only_single, margins):
    labels = list(labels)
    moves = 0
    for r in range(4):
        K, size = totals(g, labels)
        prop = list(labels)
        for v in range(g.nv):
            if cls[v] != r or (only_single and size[labels[v]] != 1):
                continue
            prop[v] = decide(g, v, labels, K, size, bound, margins)[0]
        if only_single:
            moved = [prop[v] != labels[v] for v in range(g.nv)]
            for v in range(g.nv):
                if moved[v] and size[prop[v]] == 1 and moved[prop[v]]:
                    prop[v] = labels[v]
        moves += sum(1 for v in range(g.nv) if prop[v] != labels[v])
        labels = prop
    return labels, moves


def local_moving(g, cls, labels, margins):
    q = quality(g, labels)
    for _ in range(MAX_SWEEPS):
        new, moves = sweep(g, cls, labels, None, False, margins)
        if moves == 0:
            break
        qn = quality(g, new)
        margins["q_step"] = min(margins["q_step"], abs(qn - q) / max(1.0, abs(q), abs(qn)))
        if not qn > q:
            break
        labels, q = new, qn
    return labels


def refine(g, cls, bound, margins):
    ref = list(range(g.nv))
    while True:
        ref, moves = sweep(g, cls, ref, bound, True, margins)
        if moves == 0:
            return ref


def aggregate(g, refined, labels):
    ids = sorted(set(refined))
    newid = {c: i for i, c in enumerate(ids)}
    cv = [newid[c] for c in refined]
    nc = len(ids)
    adj = [dict() for _ in range(nc)]
    selfw = [0.0] * nc
    inner = [0.0] * nc
    P = [[0.0] * len(g.P[0]) for _ in range(nc)]
    comm = [0] * nc
    for v in range(g.nv):
        selfw[cv[v]] += g.selfw[v]
        comm[cv[v]] = labels[v]
        for t, x in enumerate(g.P[v]):
            P[cv[v]][t] += x
        for u, w in sorted(g.adj[v].items()):
            if cv[u] == cv[v]:
                inner[cv[v]] += w
            else:
                adj[cv[v]][cv[u]] = adj[cv[v]].get(cv[u], 0.0) + w
    selfw = [s + i for s, i in zip(selfw, inner)]
    smallest = {}
    for c in range(nc):
        smallest.setdefault(comm[c], c)
    return Graph(nc, adj, selfw, P, g.coef), cv, [smallest[comm[c]] for c in range(nc)]


def renumber(member):
    n = len(member)
    groups = {}
    for v, c in enumerate(member):
        groups.setdefault(c, []).append(v)
    order = sorted(groups.values(), key=lambda vs: (-len(vs), vs[0]))
    out = [0] * n
    for i, vs in enumerate(order):
        for v in vs:
            out[v] = i
    return out


def optimise(g0, algorithm, random_state, n_iterations=1):
    """``(membership list, Q(final), Q(singletons), margins)``."""
    rng = np.random.default_rng(random_state)
    margins = {"runner_up": float("inf"), "own": float("inf"), "q_step": float("inf")}
    member = list(range(g0.nv))
    for _ in range(n_iterations):
        g, labels = g0, member
        vmap = list(range(g0.nv))
        while True:
            cls = (rng.permutation(g.nv) % 4).tolist()
            start = labels
            labels = local_moving(g, cls, labels, margins)
            if labels == start:
                break
            refined = refine(g, cls, labels, margins) if algorithm == "leiden" else labels
            g, cv, labels = aggregate(g, refined, labels)
            vmap = [cv[x] for x in vmap]
        member = [labels[x] for x in vmap]
    member = renumber(member)
    return member, quality(g0, member), quality(g0, list(range(g0.nv))), margins


def brute_force_q(n, layers, lambdas, gammas, member):
    """Q = sum_l lambda_l sum_c [ sum_{i,j in c} A_ij - gamma Kout_c Kin_c / m ] from dense matrices."""
    member = np.asarray(member)
    q = 0.0
    for ent, lam, gam in zip(layers, lambdas, gammas):
        A = np.zeros((n, n))
        for i, j, a in ent:
            A[i, j] += a
        m = A.sum()
        if m == 0:
            continue
        ql = 0.0
        for c in np.unique(member):
            idx = np.nonzero(member == c)[0]
            ql += A[np.ix_(idx, idx)].sum() - gam * A[idx].sum() * A[:, idx].sum() / m
        q += lam * ql
    return q
