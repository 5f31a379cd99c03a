"""csrc/knn.hip (k_knn_filter, k_knn_merge) and csrc/wnn.hip (k_wnn_bandwidth, k_umap_strengths) at their tile
edges, each against a plain f64 reference of the same operation (tests/knn_edge_refs.py: exact integer arithmetic,
brute-force searches, python sets, the numpy oracle) - not against this project's tensor formulation.  The same
references run against the tensor paths and the filter's torch emulation in tests/test_wnn.py."""
import numpy as np
import pytest
import torch

from muon_amd._ffi import MuonAmdError
from tests import knn_edge_refs as ref

pytestmark = pytest.mark.gpu


# ---- 1. knn_filter against exact integer arithmetic --------------------------------------------------------------
@pytest.mark.parametrize("square", [False, True], ids=["distinct", "square"])
@pytest.mark.parametrize("p_pad", ref.FILTER_P_PADS)
def test_filter_kernel_is_exact_on_lattice_points(hip, p_pad, square):
    """n_q in {1, 63, 64, 65, 200} (square: also all 300, Xq is Xc) x seven panels x cap in {1, 8, 64}, thresholds
    +inf, -1, a distance of the row itself (the comparison is strict) and that distance + 0.5: counts, stored
    positions and distances equal the integer evaluation bit for bit.  p_pad 4: two of a row's four loader threads
    idle; 60 -> 64: past 64 KiB of dynamic LDS; 156: the widest operand the LDS tiles take."""
    ref.check_filter(hip, p_pad, square, n_qs=ref.FILTER_N_Q + ((ref.FILTER_N_CAND,) if square else ()))


def test_filter_kernel_refuses_operands_wider_than_its_tiles(hip):
    """p_pad = 160 needs more LDS than a workgroup has: the library's error, nothing launched (the buffers and
    the counts stay as they were)"""
    X = hip.to_device(ref.lattice(np.random.default_rng(0), 64, 160))
    sq = (X * X).sum(dim=1)
    thr = torch.full((64,), float("inf"), dtype=torch.float64, device=hip.device)
    self_pos = torch.arange(64, dtype=torch.int32, device=hip.device)
    bp = torch.full((64, 8), -1, dtype=torch.int32, device=hip.device)
    bd = torch.full((64, 8), -7.0, dtype=torch.float64, device=hip.device)
    cnt = torch.full((64,), 77, dtype=torch.int32, device=hip.device)
    with pytest.raises(MuonAmdError, match="too wide for the LDS tiles"):
        hip.knn_filter(X, X, sq, sq, thr, self_pos, 0, 64, bp, bd, cnt)
    torch.cuda.synchronize()
    assert bool((bp == -1).all()) and bool((bd == -7.0).all()) and bool((cnt == 77).all())


# ---- 2. the gate of device_knn -----------------------------------------------------------------------------------
@pytest.mark.parametrize("p,filtered", [(156, True), (157, False)])
def test_device_knn_sends_the_widest_legal_operand_to_the_filter_and_no_wider(hip, p, filtered):
    """_KNN_FILTER_MAX_P: 156 columns go through the filter kernel, 157 (padded: 160, which the kernel refuses)
    through the tiled search - and both equal scipy's cdist + a stable argsort by (distance, index)"""
    calls = ref.check_gate(hip, p)
    assert (calls > 0) == filtered and (filtered or calls == 0)


# ---- 3. _candidates_filtered with the real kernels ---------------------------------------------------------------
@pytest.mark.parametrize("n", [2500, 4500])  # one filter panel [2048, 2500); two, the second one ragged
@pytest.mark.parametrize("p", [3, 64])
@pytest.mark.parametrize("kc", [5, 40])
def test_candidate_search_equals_brute_force(hip, n, p, kc):
    ref.check_candidates_separated(hip, n, p, kc)


def test_candidate_search_redoes_overflowed_rows_with_the_real_kernels(hip):
    """cap = 3 on tied lattice rows: every panel overflows; filter, fused merge and the dense redo together
    return the exact kc smallest distances"""
    ref.check_candidates_tied(hip)


@pytest.mark.parametrize("p", [3, 64])
def test_candidate_search_without_the_fused_merge(hip, p):
    """kc = 300: list ++ buffer (300 + 964) exceeds the merge kernel's 1024 slots - the filter kernel feeds
    torch's top-k"""
    proxy = ref.check_candidates_separated(hip, 4500, p, 300, cap=3 * 300 + 64)
    assert proxy.calls["knn_merge"] == 0


# ---- 4. wnn_bandwidth against the set-based definition -----------------------------------------------------------
@pytest.mark.parametrize("n_bw", [1, 20, 64])
@pytest.mark.parametrize("p", [1, 63, 64, 65, 256])
@pytest.mark.parametrize("n", [3, 5, 67, 300])
def test_bandwidth_kernel_on_irregular_graphs(hip, n, p, n_bw):
    """rows of 0 to 9 neighbours, empty rows (NaN), rows that list themselves; at n = 5 every cell has fewer
    candidates than n_bw and the mean runs over those it has"""
    X, G = ref.irregular_graph(n, p)
    want = ref.check_bandwidth(hip, X, G, n_bw)
    assert bool(torch.isnan(want).any()) and bool(torch.isfinite(want).any())


@pytest.mark.parametrize("n_bw", [1, 10, 20])
def test_bandwidth_kernel_with_tied_keys(hip, n_bw):
    X, G = ref.tied_graph()
    ref.check_bandwidth(hip, X, G, n_bw, min_gap=None)


@pytest.mark.parametrize("listers", [63, 64, 65, 66, 4095, 4096, 4097, 4098])
def test_bandwidth_kernel_at_the_sizes_of_its_sort(hip, listers):
    """a lister gathers listers - 1 entries: 62 .. 65 and 4094 .. 4097 straddle the powers of two the bitonic
    sort is padded to"""
    X, G = ref.hub_graph(listers)
    ref.check_bandwidth(hip, X, G, 20, cells=None if listers < 100 else ref.hub_sample(G, listers))


def test_bandwidth_kernel_fills_its_buffer_to_the_last_entry(hip):
    """8193 listers: each gathers exactly 8192 entries, the buffer's size - no overflow, the kernel's values"""
    X, G = ref.hub_graph(8193, private=False)
    want = ref.check_bandwidth(hip, X, G, 20, cells=ref.hub_sample(G, 8193), expect_over=False)
    assert bool(torch.isnan(want[0])) and bool(torch.isfinite(want[1:]).all())  # (the hub lists nothing)


def test_bandwidth_kernel_flags_one_entry_more_than_its_buffer(hip):
    """8194 listers: 8193 entries - the flag, and `_bandwidths` returns the reference's values all the same"""
    X, G = ref.hub_graph(8194, private=False)
    ref.check_bandwidth(hip, X, G, 20, cells=ref.hub_sample(G, 8194), expect_over=True)


# ---- 5. umap_strengths against the oracle ------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3, 21])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_umap_strengths_kernel_equals_the_oracle(hip, n, k):
    """oracle/wnn_oracle.py (numpy loops) at the edges of the kernel's 256-row blocks, with rows of all-zero,
    single-positive, constant and 1e-6 .. 1e6 distances and a cell that lists itself outside slot 0"""
    ref.check_umap(hip, n, k, backend=hip)
