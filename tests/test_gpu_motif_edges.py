"""csrc/motif.hip where tests/test_gpu_motif.py does not reach: motifs of every length 1..32, the halo of a position
tile and the room at the cap, thresholds a score attains exactly, position tiles in which every window is a hit, and
streams with more position tiles than the grid has workgroups (the ``pt += gridDim.x`` stride of k_motif_scan with its
skipped pairs, and the stride of k_motif_room).

The banks are dyadic (tests/motif_fixture.dyadic_bank: multiples of 1/64 in [-8, 2], at most 32 columns), so every
partial sum is exact in f64 and every comparison here is ==: rows, scores bit for bit, a second call byte for byte.
The reference is tests/motif_refs.scan_stream, a numpy sliding window that shares nothing with the package.  Besides
the ordered result of ``scan_sequences_device`` every case checks ``hip.motif_scan``'s raw output before the host
sort: sorted by (stream position, motif) it has no duplicate and is the reference's set - a wrong slot overwrites one
hit and leaves another slot uninitialised, whatever the host ordering would make of it.

The grid rules are restated in tests/motif_fixture (``scan_grid_x``, ``room_grid``) next to the CU count read from the
device; each stride case asserts that it still crosses its cap (DESIGN.md 9.10 lists the rules and the smallest
streams).  The CPU suite runs the same cases through the tensor formulation (tests/test_motif_host.py).

Sensitivity, tried on an MI355X with one-line changes to k_motif_scan that produce wrong values only (output buffers
zero-filled for the trial): without the sum of ``s_wcnt[w]`` over the waves below, or with ``incl`` for ``incl - n``,
every scan test here fails at the raw slots (tests/test_gpu_motif.py's denser p = 1e-2 scans fail too); ``b[j]`` loaded
only for j < 24 fails every test but the two stride ones and none of tests/test_gpu_motif.py; ``>`` for ``>=`` fails the
every-length, halo, equality and scan-stride tests and none of tests/test_gpu_motif.py; a write pass that takes only
its first stride step fails test_more_position_tiles_than_workgroups alone."""
import numpy as np
import pytest
import torch

from muon_amd._atac import motifs as Mo
from tests import motif_fixture as F
from tests import motif_refs

pytestmark = pytest.mark.gpu


def _cus(hip):
    return int(torch.cuda.get_device_properties(hip.device).multi_processor_count)


def _check(hip, case, n_tiles):
    """scan ``case`` on the kernel: the raw slots, the ordered result and a second call against the restatement"""
    seq, mot, pos, score = case.want()
    scanner = Mo.MotifScanner(hip, case.matrices, case.thresholds)
    assert scanner.tensor == [] and scanner.bank["n_tiles"] == n_tiles
    dev = (hip.to_device(case.codes, np.uint8), hip.to_device(case.offsets, np.int64))
    # the slots as the kernel filled them, first: a slot left unwritten holds anything, and only the host looks here
    rseq, rmot, rpos, rscore = (t.cpu().numpy() for t in hip.motif_scan(dev[0], dev[1], scanner.bank))
    assert rseq.size == seq.size  # (n_hits: the sum of the count pass)
    assert rseq.size == 0 or (rseq.min() >= 0 and rseq.max() < case.offsets.size - 1)
    order = np.lexsort((rmot, case.offsets[rseq] + rpos))
    gpos, kmot, kscore = (case.offsets[rseq] + rpos)[order], rmot[order].astype(np.int64), rscore[order]
    assert kmot.size == 0 or (kmot.min() >= 0 and kmot.max() < len(case.matrices))
    assert np.all(np.diff(gpos * len(case.matrices) + kmot) > 0)  # no (position, motif) twice, padding motifs included
    wpos, wmot = case.want_keys()
    worder = np.lexsort((wmot, wpos))
    assert np.array_equal(gpos, wpos[worder]) and np.array_equal(kmot, wmot[worder])
    assert np.array_equal(kscore, score[worder]) and np.array_equal(rseq[order], seq[worder])
    # the ordered result
    got = Mo.scan_sequences_device(dev, scanner)
    host = [t.cpu().numpy() for t in got]
    assert [h.dtype for h in host] == [np.int32, np.int32, np.int32, np.float64]
    print(f"{len(seq)} hits expected, {len(host[0])} found")
    assert np.array_equal(host[0], seq) and np.array_equal(host[1], mot) and np.array_equal(host[2], pos)
    assert np.array_equal(host[3], score)
    for a, b in zip(host, Mo.scan_sequences_device(dev, scanner)):
        assert a.tobytes() == b.cpu().numpy().tobytes()
    return scanner


def test_every_length_1_to_32(hip):
    """one motif per length in a shuffled caller order (two tiles of the bank, ``orig`` no identity) over sequences of
    lengths 1, 31, 32, 33, 255, 256, 257, 288 with empty ones and scattered invalid codes"""
    assert hip.motif_max_len() == F.CAP and hip.motif_group() == F.GROUP and hip.motif_tile() == F.TILE
    case = F.case_every_length()
    assert sorted(case.lengths.tolist()) == list(range(1, F.CAP + 1)) and case.lengths.tolist() != sorted(case.lengths)
    F.assert_every_motif_hits_and_misses(case)
    scanner = _check(hip, case, 2)
    assert scanner.bank["orig"].cpu().tolist() != list(range(32))


@pytest.mark.parametrize("L", [32, 25])
def test_halo_and_room_at_the_cap(hip, L):
    """the best word of the L-column motif at the last position of a tile (its other L - 1 bases are halo bytes; room
    == L, for L = 32 the cap itself), cut by a sequence end, spoilt by an invalid code in its last column, and ending
    with a stream that is no multiple of the tile"""
    case = F.case_halo(L, hip.motif_tile())
    F.assert_halo_plants(case, hip.motif_tile())
    _check(hip, case, 2)


@pytest.mark.parametrize("L", [1, 16, 32])
def test_threshold_at_equality(hip, L):
    """thr = s, a score some window attains exactly: a hit; thr = nextafter(s): none, and every other row stays"""
    at, above = F.case_equality(L)
    F.assert_equality_pair(at, above)
    _check(hip, at, 2)
    _check(hip, above, 2)


@pytest.mark.parametrize("alternate", [False, True], ids=["all", "alternating"])
def test_full_density(hip, alternate):
    """every admissible window a hit (thresholds -inf; alternating with +inf by motif: lane masks full in some columns
    and empty in others): 16 set bits per lane, hits in all four waves, 4 096 hits in one (motif tile, position tile)
    pair; the second motif tile holds one motif and 15 padding slots"""
    case = F.case_density(alternate, hip.motif_tile())
    F.assert_density(case, alternate, hip.motif_tile())
    _check(hip, case, 2)


def test_more_position_tiles_than_workgroups(hip):
    """k_motif_scan takes three stride steps in some workgroups; with both empty and non-empty pairs in every motif
    tile, the write pass skips and recomputes inside one workgroup's stride"""
    cus, tile = _cus(hip), hip.motif_tile()
    case = F.case_scan_stride(cus, tile)
    n_ptiles = -(-case.total // tile)
    grid_x = min(F.scan_grid_x(cus, 3), n_ptiles)  # motif_grid_x(n_ptiles, 3)
    print(f"{cus} CUs: grid_x {grid_x}, {n_ptiles} position tiles, {case.total} positions")
    assert n_ptiles >= 2 * grid_x + 1 and case.total % tile != 0
    F.assert_stride_mixture(case, tile)
    _check(hip, case, 3)


def test_room_with_more_positions_than_threads(hip):
    cus = _cus(hip)
    codes, offsets = F.room_stride_stream(cus)
    assert codes.size >= 2 * F.room_grid(cus) * 256 + 1  # every thread of k_motif_room takes a third position
    room = hip.motif_room(hip.to_device(codes, np.uint8), hip.to_device(offsets, np.int64)).cpu().numpy()
    want = np.minimum(motif_refs.stream_room(codes, offsets), hip.motif_max_len())
    assert {0, 1, hip.motif_max_len()} <= set(np.unique(want).tolist())
    assert room.dtype == np.uint8 and np.array_equal(room, want)
