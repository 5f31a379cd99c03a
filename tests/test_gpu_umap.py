"""muon_amd.tl.umap on the device: one epoch of ``k_umap_epoch`` (through ``HipBackend.umap_epoch``) against the plain-
Python restatement (tests/umap_refs.py) and against the tensor formulation on the same device, for DIM 2 and 3, on the
graphs of tests/umap_fixture.epoch_cases(): n = 1; one workgroup of sixteen vertices plus one vertex; an empty row; rows
of 1, G - 1, G, G + 1 and 2 G + 1 entries (G = 16 lanes per vertex); a hub row of 1040 entries; all weights equal (every
entry active); an entry never active; negative_sample_rate 0 and 20; two coincident points joined by an entry; n = 3,
where negatives hit k == v often; the first epoch and the last.  Then repeats, the routing of n_components = 4, the public
function on the quality fixture and end to end behind pp.neighbors.

Bound of one epoch: f64, coordinates in [0, 10], clipped forces, a few ulp per term (the device's ``pow`` and libm's may
differ in the last place) and at most ~10^3 terms per row: 1e-10 absolute, for the kernel against the restatement (same
sum order) and against the tensor formulation (another order).

The launch is a one-dimensional grid of ceil(n / 16) workgroups (n < 2^31: below 2^27 of them, one grid dimension
holds 2^31 - 1): the geometry has no edge at 65 535 blocks, so there is no test past it.

Every array handed to the kernel is a view into a larger buffer whose surroundings hold NaN (f64) or -7 (integers); the
output's surroundings must come back untouched."""
import os

import numpy as np
import pytest
import torch

from tests import umap_fixture as fx
from tests import umap_refs as R
from muon_amd import AnnData, MuData, tl
from muon_amd._core import preproc as pp
from muon_amd._core import umap as U

pytestmark = pytest.mark.gpu

PAD = 3
ALPHA_E = 0.7


def padded(hip, a):
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.reshape(-1))
    fill = float("nan") if a.dtype == np.float64 else -7
    buf = torch.full((t.numel() + 2 * PAD,), fill, dtype=t.dtype, device=hip.device)
    buf[PAD:PAD + t.numel()] = t.to(hip.device)
    return buf[PAD:PAD + t.numel()].view(a.shape), buf


def surroundings_untouched(buf):
    edge = torch.cat([buf[:PAD], buf[-PAD:]])
    return bool(torch.isnan(edge).all()) if buf.dtype == torch.float64 else bool((edge == -7).all())


def kernel_epoch(hip, case, Y):
    p = fx.EPOCH_PARAMS
    d, bufs = {}, {}
    for name, a in (("indptr", case["indptr"]), ("cols", case["cols"]), ("E", case["E"]), ("Y", Y),
                    ("out", np.full(Y.shape, np.nan))):
        d[name], bufs[name] = padded(hip, a)
    got = hip.umap_epoch(d["indptr"], d["cols"], d["E"], case["e"], case["n_epochs"], case["rate"], p["a"], p["b"],
                         p["gamma"], ALPHA_E, p["seed"], d["Y"], d["out"])
    torch.cuda.synchronize()
    assert surroundings_untouched(bufs["out"]) and torch.equal(d["Y"].cpu(), torch.from_numpy(Y))
    return got.cpu().numpy()


def graph_of(be, case):
    n = int(case["indptr"].size) - 1
    rows = np.repeat(np.arange(n), np.diff(case["indptr"]))
    return U._Graph(be, n, rows, case["cols"], np.ones(case["cols"].size), case["E"])


def tensor_epoch(be, case, Y):
    p = fx.EPOCH_PARAMS
    Yd = be.to_device(np.ascontiguousarray(Y), np.float64)
    out = U._epoch_tensor(be, graph_of(be, case), Yd, case["e"], case["n_epochs"], case["rate"], p["a"], p["b"], p["gamma"],
                          ALPHA_E, p["seed"])
    return be.to_host(out)


def restated_epoch(case, Y):
    p = fx.EPOCH_PARAMS
    return R.epoch(Y, case["indptr"], case["cols"], case["E"], case["e"], case["n_epochs"], case["rate"], p["a"], p["b"],
                   p["gamma"], ALPHA_E, p["seed"])


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("name", sorted(fx.epoch_cases()))
def test_one_kernel_epoch_equals_the_restatement_and_the_tensor_formulation(hip, name, dim):
    case = fx.epoch_cases()[name]
    Y = fx.epoch_positions(case, dim)
    ref = restated_epoch(case, Y)
    got = kernel_epoch(hip, case, Y)
    ten = tensor_epoch(hip, case, Y)
    print(f"MEASURE umap kernel epoch {name} dim {dim}: max |kernel - restatement| {np.abs(got - ref).max():.3e}, "
          f"|kernel - tensor| {np.abs(got - ten).max():.3e}, max step {np.abs(ref - Y).max():.3e}")
    assert np.isfinite(got).all()
    assert np.abs(got - ref).max() <= 1e-10
    assert np.abs(got - ten).max() <= 1e-10
    if name == "n1":
        np.testing.assert_array_equal(got, Y)
    else:
        assert np.abs(ref - Y).max() > 1e-3
    # rows without an active entry keep their coordinates
    for v in np.nonzero(np.diff(case["indptr"]) == 0)[0]:
        np.testing.assert_array_equal(got[v], Y[v])


def test_arguments_are_checked_before_any_launch(hip):
    case = fx.epoch_cases()["coincident_n3"]
    g = graph_of(hip, case)
    Y = hip.to_device(fx.epoch_positions(case, 2), np.float64)
    out = torch.empty_like(Y)
    from muon_amd._ffi import MuonAmdError

    with pytest.raises(MuonAmdError, match="epoch must be"):
        hip.umap_epoch(g.indptr, g.cols, g.E, 6, 5, 5, 1.0, 1.0, 1.0, 1.0, 0, Y, out)
    with pytest.raises(MuonAmdError, match="rate must be"):
        hip.umap_epoch(g.indptr, g.cols, g.E, 1, 5, 5000, 1.0, 1.0, 1.0, 1.0, 0, Y, out)
    with pytest.raises(MuonAmdError, match="n_components"):
        hip.umap_epoch(g.indptr, g.cols, g.E, 1, 5, 5, 1.0, 1.0, 1.0, 1.0, 0, torch.zeros((3, 4), dtype=torch.float64,
                       device=hip.device), torch.zeros((3, 4), dtype=torch.float64, device=hip.device))
    with pytest.raises(ValueError, match="two buffers"):
        hip.umap_epoch(g.indptr, g.cols, g.E, 1, 5, 5, 1.0, 1.0, 1.0, 1.0, 0, Y, Y)
    with pytest.raises(TypeError, match="cols"):
        hip.umap_epoch(g.indptr, g.cols64, g.E, 1, 5, 5, 1.0, 1.0, 1.0, 1.0, 0, Y, out)
    assert hip.umap_max_components() == 3


@pytest.mark.parametrize("dim", [2, 3])
def test_twenty_epochs_run_twice_are_byte_equal_and_finite(hip, dim):
    A = fx.knn_connectivities(fx.blobs(1000, 4, 6, 3)[0], 12)
    g = U._Graph(hip, 1000, *U.edges(A, 20))
    Y0 = U.initial_positions(hip, g, "random", dim, 11)
    a, b = fx.AB
    runs = []
    for _ in range(2):
        d = {}
        Y = U.layout(hip, g, Y0, 20, 1.0, 1.0, 5, a, b, 11, d)
        assert d["path"] == "kernel"
        runs.append(hip.to_host(Y))
    assert np.isfinite(runs[0]).all() and runs[0].tobytes() == runs[1].tobytes()
    assert np.abs(runs[0] - Y0).max() > 0.1


def test_four_components_take_the_tensor_formulation_and_agree_with_the_restatement(hip):
    case = fx.epoch_cases()["rows_last_epoch"]
    Y = fx.epoch_positions(case, 4)
    ten, ref = tensor_epoch(hip, case, Y), restated_epoch(case, Y)
    assert np.abs(ten - ref).max() <= 1e-10 and np.abs(ref - Y).max() > 1e-3
    A = fx.knn_connectivities(fx.blobs(60, 2, 4, 1)[0], 5)
    ad, d = fx.anndata_of(A), {}
    tl.umap(ad, n_components=4, maxiter=10, backend=hip, diagnostics=d)
    assert d["path"] == "tensor" and ad.obsm["X_umap"].shape == (60, 4) and np.isfinite(ad.obsm["X_umap"]).all()


def test_public_umap_on_the_quality_fixture(hip, golden_dir):
    gold = np.load(os.path.join(golden_dir, "umap_golden.npz"))
    seq = np.asarray(gold["sequential_trust"])
    floor = float(seq.min() - (seq.max() - seq.min()))
    a, b = fx.AB
    runs = []
    for _ in range(2):
        ad, d = fx.anndata_of(fx.quality_graph()), {}
        tl.umap(ad, maxiter=fx.QUALITY["n_epochs"], init_pos="random", random_state=0, a=a, b=b, backend=hip, diagnostics=d)
        assert d["path"] == "kernel"
        runs.append(ad.obsm["X_umap"])
    X = runs[0]
    t = fx.trust(X)
    print(f"MEASURE umap quality (kernel): trustworthiness {t:.6f}, sequential {seq.tolist()}, floor {floor:.6f}, extent "
          f"{np.abs(X).max():.3f}")
    assert X.dtype == np.float32 and X.shape == (fx.QUALITY["n"], 2)
    assert np.isfinite(X).all() and np.abs(X).max() <= 60.0  # (the extent of tests/test_umap_host.py)
    assert X.tobytes() == runs[1].tobytes()
    assert t >= floor


def test_end_to_end_behind_pp_neighbors(hip):
    from tests.test_wnn import two_modalities

    lab, x1, x2 = two_modalities(260, 4)
    md = MuData({"rna": AnnData(x1.copy()), "atac": AnnData(x2.copy())})
    for m in md.mod.values():
        pp.knn(m, n_neighbors=15, use_rep="X", backend=hip)
    pp.neighbors(md, n_multineighbors=50, backend=hip)
    d = {}
    assert tl.umap(md, maxiter=100, backend=hip, diagnostics=d) is None
    X = md.obsm["X_umap"]
    assert d["path"] == "kernel" and X.dtype == np.float32 and X.shape == (260, 2) and np.isfinite(X).all()
    assert md.uns["umap"]["params"]["random_state"] == 42 and d["entries"] > 260
    # the embedding keeps the graph's neighbourhoods: an observation's graph neighbours are nearer than the rest
    C = md.obsp["connectivities"].tocsr()
    D = np.sqrt(((X[:, None, :].astype(np.float64) - X[None, :, :]) ** 2).sum(-1))
    near = np.mean([D[v, C.indices[C.indptr[v]:C.indptr[v + 1]]].mean() for v in range(260)])
    print(f"MEASURE umap end to end: mean distance to graph neighbours {near:.3f}, to everybody {D.mean():.3f}")
    assert near < 0.5 * D.mean()
    out = tl.umap(md, maxiter=100, copy=True, backend=hip)
    assert out is not md and out.obsm["X_umap"].tobytes() == X.tobytes()
