"""muon_amd.tl.leiden / muon_amd.tl.louvain on the device: ``cluster_move`` against a brute-force statement of one
sub-round, ``cluster_segsum`` against numpy, and every graph of tests/cluster_fixture.py end to end on the kernel path
against the plain-python restatement (tests/cluster_refs.py).

``cluster_move``: proposals must be equal and scores BIT-equal.  Weights and strengths are multiples of 1/64 (small), the
coefficients dyadic, so w(v, C), K, every product kout Kin and every partial sum are exact in f64 in any order: the
kernel's chunked butterfly sums and numpy's give the same bits.  Shapes: the wave (64 lanes: nv and degrees 63 / 64 /
65), more than one chunk (degree 200, a hub adjacent to all), the direct-addressed table (nv <= 512) and the hashed one,
the table at its capacity (own community + 511 neighbouring ones: answered) and one past it (reported, not answered).
Every array handed to the kernel is a view into a larger buffer whose surroundings hold NaN (f64) or -7 (integers); the
outputs' surroundings must come back untouched.

``cluster_segsum``: 64ths again, bit-equal to numpy; float rows twice, bit-equal to each other."""
import numpy as np
import pytest
import torch

from tests import cluster_fixture as fx
from muon_amd import tl
from muon_amd._core import cluster as C

pytestmark = pytest.mark.gpu

PAD = 3


def padded(hip, a):
    """``a`` on the device as a view of a buffer PAD elements longer at both ends (NaN / -7 around it)."""
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.reshape(-1))
    fill = float("nan") if a.dtype == np.float64 else -7
    buf = torch.full((t.numel() + 2 * PAD,), fill, dtype=t.dtype, device=hip.device)
    buf[PAD:PAD + t.numel()] = t.to(hip.device)
    return buf[PAD:PAD + t.numel()].view(a.shape), buf


def surroundings_untouched(buf):
    edge = torch.cat([buf[:PAD], buf[-PAD:]])
    return bool(torch.isnan(edge).all()) if buf.dtype == torch.float64 else bool((edge == -7).all())


# ---- cluster_move -------------------------------------------------------------------------------------------------------
def rows_graph(nv, degrees, rng, unit=False):
    """A CSR whose row v holds ``degrees[v]`` distinct neighbours != v, values in 64ths (``unit``: all 1/2)."""
    indptr, cols, vals = [0], [], []
    for v in range(nv):
        d = min(int(degrees[v]), nv - 1)
        nb = rng.choice(nv - 1, d, replace=False)
        nb = np.sort(nb + (nb >= v))
        cols.append(nb)
        vals.append(np.full(d, 0.5) if unit else rng.integers(1, 65, d) / 64.0)
        indptr.append(indptr[-1] + d)
    return (np.asarray(indptr, dtype=np.int64), np.concatenate(cols).astype(np.int32) if cols else np.zeros(0, np.int32),
            np.concatenate(vals) if vals else np.zeros(0))


def brute_sub_round(nv, indptr, cols, vals, lab, bound, P, coef, verts, only_single):
    """One sub-round from its statement (muon_amd/_core/cluster.py, step 2): ``(prop, score)`` for the vertices of verts."""
    L = len(coef)
    size = np.bincount(lab, minlength=nv)
    K = np.zeros((nv, 2 * L))
    for v in range(nv):
        K[lab[v]] += P[v]
    prop, score = lab.copy(), np.zeros(nv)
    for v in verts:
        a = lab[v]
        if only_single and size[a] != 1:
            continue
        nb, w = cols[indptr[v]:indptr[v + 1]], vals[indptr[v]:indptr[v + 1]]
        if bound is not None:
            keep = bound[nb] == bound[v]
            nb, w = nb[keep], w[keep]
        scores = {}
        for Cc in sorted({a} | set(lab[nb].tolist())):
            if Cc != a and size[a] == 1 and size[Cc] == 1 and Cc > a:
                continue
            Kc = K[Cc] - (P[v] if Cc == a else 0.0)
            pen = 0.0
            for l in range(L):
                pen = pen + coef[l] * (P[v, 2 * l] * Kc[2 * l + 1] + P[v, 2 * l + 1] * Kc[2 * l])
            scores[Cc] = float(w[lab[nb] == Cc].sum()) - pen
        best = min(scores, key=lambda c: (-scores[c], c))
        if best != a and scores[best] > scores[a]:
            prop[v], score[v] = best, scores[best]
        else:
            score[v] = scores[a]
    return prop, score, K, size


def snapshot(kind, nv, rng):
    if kind == "singletons":
        return np.arange(nv, dtype=np.int32)
    if kind == "one":
        return np.full(nv, nv // 2, dtype=np.int32)
    if kind == "few":
        return rng.choice(np.arange(0, nv, max(1, nv // 7)), nv).astype(np.int32)
    mixed = np.arange(nv, dtype=np.int32)  # half singletons, the rest in communities of a few
    take = rng.random(nv) < 0.5
    mixed[take] = rng.choice(np.nonzero(take)[0][:max(1, take.sum() // 4)], take.sum())
    return mixed


def run_move(hip, nv, indptr, cols, vals, lab, bound, P, coef, verts, only_single):
    prop_ref, score_ref, K, size = brute_sub_round(nv, indptr, cols, vals, lab, bound, P, coef, verts, only_single)
    d = {}
    bufs = {}
    for name, a in (("verts", np.asarray(verts, dtype=np.int32)), ("indptr", indptr), ("cols", cols), ("vals", vals),
                    ("lab", lab), ("size", size.astype(np.int32)), ("P", P), ("K", K), ("prop", lab.copy()),
                    ("score", np.zeros(nv))):
        d[name], bufs[name] = padded(hip, a)
    d["bound"] = None if bound is None else padded(hip, bound)[0]
    flag = torch.zeros((1,), dtype=torch.int32, device=hip.device)
    hip.cluster_move(d["verts"], d["indptr"], d["cols"], d["vals"], d["lab"], d["bound"], d["size"], d["P"], d["K"], coef,
                     only_single, d["prop"], d["score"], flag)
    assert surroundings_untouched(bufs["prop"]) and surroundings_untouched(bufs["score"])
    return d, int(flag[0]), prop_ref, score_ref


def strengths(nv, L, rng):
    return rng.integers(0, 200, (nv, 2 * L)) / 64.0


COEF = [2.0 ** -9, 2.0 ** -8, 3 * 2.0 ** -11, 2.0 ** -10]
DEGREES = [0, 1, 63, 64, 65, 200]


@pytest.mark.parametrize("nv", [1, 2, 63, 64, 65, 257])
@pytest.mark.parametrize("kind", ["singletons", "one", "few", "mixed"])
def test_move_equals_the_brute_force_sub_round(hip, nv, kind):
    rng = np.random.default_rng(100 * nv + len(kind))
    degrees = [DEGREES[v % len(DEGREES)] for v in range(nv)]
    if nv > 2:
        degrees[nv // 2] = nv - 1  # a hub adjacent to all
    indptr, cols, vals = rows_graph(nv, degrees, rng)
    lab = snapshot(kind, nv, rng)
    for L in (1, 2, 4):
        P = strengths(nv, L, rng)
        for cls in range(2):
            verts = np.arange(cls, nv, 2)
            d, flag, prop_ref, score_ref = run_move(hip, nv, indptr, cols, vals, lab, None, P, COEF[:L], verts, False)
            assert flag == 0
            assert np.array_equal(d["prop"].cpu().numpy(), prop_ref), (nv, kind, L)
            assert np.array_equal(d["score"].cpu().numpy(), score_ref), (nv, kind, L)  # bit-equal
    if kind in ("few", "mixed") and nv > 2:
        assert (prop_ref != lab).any()  # the case moves something


@pytest.mark.parametrize("nv", [2, 65, 257])
@pytest.mark.parametrize("L", [1, 4])
def test_move_in_refinement_bound_and_only_single(hip, nv, L):
    rng = np.random.default_rng(7 * nv + L)
    degrees = [DEGREES[(v + 2) % len(DEGREES)] for v in range(nv)]
    indptr, cols, vals = rows_graph(nv, degrees, rng)
    bound = (rng.integers(0, 3, nv) * (nv // 3)).astype(np.int32)
    lab = snapshot("mixed", nv, rng)
    P = strengths(nv, L, rng) / 8
    for use_bound in (False, True):
        for only_single in (False, True):
            d, flag, prop_ref, score_ref = run_move(hip, nv, indptr, cols, vals, lab, bound if use_bound else None, P,
                                                    COEF[:L], np.arange(nv), only_single)
            assert flag == 0
            assert np.array_equal(d["prop"].cpu().numpy(), prop_ref) and np.array_equal(d["score"].cpu().numpy(), score_ref)
            if only_single:
                sizes = np.bincount(lab, minlength=nv)
                assert np.array_equal(prop_ref[sizes[lab] != 1], lab[sizes[lab] != 1])


def test_move_score_ties_go_to_the_smallest_id(hip):
    nv = 130
    rng = np.random.default_rng(5)
    indptr, cols, vals = rows_graph(nv, [64 + (v % 3) for v in range(nv)], rng, unit=True)
    lab = (np.arange(nv) % 8 * 9 + 1).astype(np.int32)  # eight communities met about eight times each: equal sums abound
    P = np.zeros((nv, 2))  # no penalty: score = w, multiples of 1/2
    d, flag, prop_ref, score_ref = run_move(hip, nv, indptr, cols, vals, lab, None, P, [1.0], np.arange(nv), False)
    ties = 0
    for v in range(nv):
        w = np.bincount(lab[cols[indptr[v]:indptr[v + 1]]], minlength=nv) * 0.5
        ties += int((w == w.max()).sum() > 1)
    assert ties >= 5  # the case holds ties for the best
    assert flag == 0 and np.array_equal(d["prop"].cpu().numpy(), prop_ref) and np.array_equal(d["score"].cpu().numpy(), score_ref)


@pytest.mark.parametrize("nv,hub_degree,reports", [(512, 511, False), (600, 511, False), (600, 512, True), (513, 512, True)])
def test_move_table_at_capacity_and_one_past_it(hip, nv, hub_degree, reports):
    """All singletons: the hub's table needs its own community and one entry per neighbour.  512 entries fit (by the
    community id when nv <= 512, by the hash beyond); 513 make the kernel report and leave the hub where it is."""
    assert hip.cluster_max_table() == 512 and hip.cluster_max_layers() == 4
    rng = np.random.default_rng(nv + hub_degree)
    degrees = [3] * nv
    hub = nv - 1  # the largest id: every neighbouring singleton is a candidate under the swap guard
    degrees[hub] = hub_degree
    indptr, cols, vals = rows_graph(nv, degrees, rng)
    lab = np.arange(nv, dtype=np.int32)
    P = strengths(nv, 2, rng) / 16
    quiet = np.arange(0, nv - 1, 5)
    d, flag, prop_ref, score_ref = run_move(hip, nv, indptr, cols, vals, lab, None, P, COEF[:2], quiet, False)
    assert flag == 0 and np.array_equal(d["prop"].cpu().numpy(), prop_ref)
    verts = np.concatenate([quiet, [hub]])
    d, flag, prop_ref, score_ref = run_move(hip, nv, indptr, cols, vals, lab, None, P, COEF[:2], verts, False)
    got, got_s = d["prop"].cpu().numpy(), d["score"].cpu().numpy()
    assert np.array_equal(got[quiet], prop_ref[quiet]) and np.array_equal(got_s[quiet], score_ref[quiet])
    if reports:
        assert flag == 1 and got[hub] == hub and got_s[hub] == 0.0
    else:
        assert flag == 0 and got[hub] == prop_ref[hub] and got_s[hub] == score_ref[hub] and prop_ref[hub] != hub


def test_the_tensor_formulation_on_the_device_gives_the_kernels_bits(hip):
    case = "n300_w64_L2"
    lam, gam = fx.layer_parameters(case)
    layers = [C._edges(A, True) for A in fx.graphs(case)]
    g = C._build_graph(hip, layers, lam, gam, True)
    rng = np.random.default_rng(2)
    labels = torch.from_numpy(snapshot("mixed", g.nv, rng)).to(hip.device)
    K, size = C._totals(hip, g, labels)
    active = torch.from_numpy(rng.random(g.nv) < 0.4).to(hip.device)
    prop_t, score_t = C._move_tensor(hip, g, labels, None, False, active, K, size)
    prop_k, score_k = labels.clone(), torch.zeros((g.nv,), dtype=torch.float64, device=hip.device)
    flag = torch.zeros((1,), dtype=torch.int32, device=hip.device)
    hip.cluster_move(torch.nonzero(active).reshape(-1).to(torch.int32), g.indptr, g.cols, g.vals, labels, None, size, g.P, K,
                     g.coef, False, prop_k, score_k, flag)
    assert int(flag[0]) == 0 and torch.equal(prop_t, prop_k) and torch.equal(score_t, score_k)
    assert int((prop_k != labels).sum()) > 10


# ---- cluster_segsum -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 5])
def test_segsum_equals_numpy_bit_for_bit(hip, w):
    rng = np.random.default_rng(w)
    lengths = [1, 63, 64, 65, 0, 1000, 2, 0, 0]  # an empty segment inside and an empty tail
    ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    vals = rng.integers(-500, 500, (int(ptr[-1]), w)) / 64.0
    want = np.stack([vals[ptr[s]:ptr[s + 1]].sum(axis=0) for s in range(len(lengths))])
    v, _ = padded(hip, vals)
    p, _ = padded(hip, ptr)
    got = hip.cluster_segsum(v, p)
    assert got.shape == (len(lengths), w) and np.array_equal(got.cpu().numpy(), want)
    floats = torch.from_numpy(rng.standard_normal((int(ptr[-1]), w))).to(hip.device)
    first = hip.cluster_segsum(floats, p)
    assert torch.equal(first, hip.cluster_segsum(floats, p))
    ref = np.stack([floats.cpu().numpy()[ptr[s]:ptr[s + 1]].sum(axis=0) for s in range(len(lengths))])
    assert np.abs(first.cpu().numpy() - ref).max() <= 1000 * 2.0 ** -53 * 1000  # (n u sum|x|, coarse: order differs)
    assert hip.cluster_segsum(torch.zeros((0, w), dtype=torch.float64, device=hip.device),
                              torch.zeros((1,), dtype=torch.int64, device=hip.device)).shape == (0, w)


# ---- end to end ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(fx.CASES))
def test_every_fixture_graph_on_the_kernel_path_gives_the_restatements_labels(hip, case):
    for alg in fx.ALGORITHMS:
        for directed in (True, False):
            member = fx.restated(case, alg, directed)[0]
            md, diag = fx.mudata(case), {}
            getattr(tl, alg)(md, directed=directed, backend=hip, diagnostics=diag, **fx.call_kwargs(case))
            assert np.array_equal(fx.labels_of(md, alg), np.asarray(member)), (case, alg, directed)
            layers = len(fx.graphs(case))
            want = "kernel" if layers <= hip.cluster_max_layers() else "tensor"
            assert diag["levels"][0]["route"] == want and diag["path"] == want
            assert not any(l.get("overflow") for l in diag["levels"])


@pytest.mark.parametrize("alg", fx.ALGORITHMS)
def test_two_runs_are_byte_equal(hip, alg):
    case = "float"
    out = []
    for _ in range(2):
        md, diag = fx.mudata(case), {}
        getattr(tl, alg)(md, backend=hip, diagnostics=diag, **fx.call_kwargs(case))
        out.append((fx.labels_of(md, alg).tobytes(), np.float64(diag["q"]).tobytes(),
                    np.float64(md.uns[alg]["params"]["partition_improvement"]).tobytes()))
    assert out[0] == out[1]
