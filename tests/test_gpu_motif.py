"""csrc/motif.hip on the GPU: the scan of tests/motif_fixture.py's sequences (random ones of lengths around the window,
the sub-tile and the position tile, plus hand-built edge cases) against the brute-force restatement
tests/motif_refs.py.

Asked: the hit rows identical to the restatement's, in order; scores to atol 1e-12 (at most 33 additions of partial
sums below 33 * 14: 33 * 462 * 2^-53 = 1.7e-12 worst case for the 33-column motif, 9e-13 for the 24 columns of the
longest kernel motif of THIS fixture - and both paths add in the restatement's order, so equality is what is expected); a second call
byte-equal; the kernel path and the tensor formulation identical.  A window whose exact score lies within 1e-9 of its
threshold could legitimately differ: the restatement's margin over every admissible window of the fixture is asserted
to be larger, so no case is left out.  Measured on the CPU for the whole fixture (hand-built cases included): 20 hits
at 1e-4 and 1 435 at 1e-2; smallest |score - threshold| 6.9e-4 and 4.8e-4.

Not here but in tests/test_gpu_motif_edges.py, on exact (dyadic) banks and with ==: kernel motifs of 25 to 32 columns
and of one column (the kernel takes up to ``motif_max_len()`` = 32), thresholds a score attains exactly, position tiles
in which every window is a hit, and streams with more position tiles than the grid has workgroups (this fixture's 40
position tiles never make a workgroup take a second one)."""
import numpy as np
import pytest
import torch

from muon_amd import atac as ac
from muon_amd._atac import motifs as Mo
from tests import motif_fixture as F

pytestmark = pytest.mark.gpu


def _rows(arrays):
    seq, mot, pos, score = (t.cpu() for t in arrays)
    return list(zip(seq.tolist(), mot.tolist(), pos.tolist())), score.numpy()


def _check(arrays, want):
    rows, score = _rows(arrays)
    assert rows == [r[:3] for r in want]
    np.testing.assert_allclose(score, np.array([r[3] for r in want], dtype=np.float64), rtol=0, atol=1e-12)


def test_caps(hip):
    assert hip.motif_max_len() >= 24 and hip.motif_max_len() + 1 == F.LONG_COLUMNS
    assert hip.motif_tile() == F.TILE and hip.motif_group() == 16


def test_room(hip):
    seqs = ["ACGTNACG", "", "AC", "A" * 40 + "n", "ACG"]
    codes, offsets = Mo.encode_sequences(seqs)
    room = hip.motif_room(hip.to_device(codes, np.uint8), hip.to_device(offsets, np.int64)).cpu()
    want = Mo._room_tensor(torch.from_numpy(codes), torch.from_numpy(offsets)).clamp(max=hip.motif_max_len())
    assert room.tolist() == want.tolist()


@pytest.mark.parametrize("pvalue", F.PVALUES)
def test_scan_is_the_restatements(hip, pvalue):
    """the whole bank: 17 motifs on the kernel (two tiles of the bank), the 33-column one on the tensor formulation
    inside the same call"""
    ids, mats = F.bank()
    seqs = list(F.sequences(hip.motif_tile()))
    want, margin = F.expected(pvalue, None, hip.motif_tile())
    print(f"p={pvalue}: {len(want)} hits, smallest |score - threshold| {margin:.3e}")
    assert margin > 1e-9
    scanner = ac.tl.prepare_motif_scanner(mats, pvalue=pvalue, backend=hip)
    assert scanner.bank is not None and scanner.bank["n_tiles"] == 2
    assert [i for i, _ in scanner.tensor] == [ids.index("SYN33")]
    got = ac.tl.scan_sequences_device(seqs, scanner)
    _check(got, want)
    again = ac.tl.scan_sequences_device(seqs, scanner)
    for a, b in zip(got, again):
        assert a.dtype == b.dtype and torch.equal(a, b)
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    # the tensor formulation of every motif on the same device: identical, scores bit for bit
    plain = ac.tl.prepare_motif_scanner(mats, pvalue=pvalue, backend=hip, use_kernel=False)
    assert plain.bank is None and len(plain.tensor) == len(mats)
    for a, b in zip(got, ac.tl.scan_sequences_device(seqs, plain)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("n_motifs", [1, 15, 16, 17])
def test_bank_sizes(hip, n_motifs):
    ids, mats = F.sub_bank(n_motifs)
    seqs = list(F.sequences(hip.motif_tile()))
    want, margin = F.expected(1e-2, n_motifs, hip.motif_tile())
    assert margin > 1e-9 and len(want) > 0
    scanner = ac.tl.prepare_motif_scanner(mats, pvalue=1e-2, backend=hip)
    assert scanner.bank["n_tiles"] == -(-n_motifs // 16) and not scanner.tensor
    _check(ac.tl.scan_sequences_device(seqs, scanner), want)


def test_frame_on_the_device_path(hip):
    ids, mats = F.bank()
    seqs = list(F.sequences(hip.motif_tile()))
    want, _ = F.expected(1e-4, None, hip.motif_tile())
    meta = Mo.parse_motif_ids(jaspar_dir=F.jaspar_dir())
    got = ac.tl.scan_sequences(seqs, matrices=mats, motifs=ids, motif_meta=meta, backend=hip)
    assert list(got.columns) == ["motif_id", "sequence", "position", "score", "tf_gene_name"]
    assert got["sequence"].tolist() == [seqs[r[0]] for r in want]
    assert got["motif_id"].tolist() == [ids[r[1]] for r in want]
    assert got["position"].tolist() == [r[2] for r in want]
    # a pre-encoded stream that is already on the device
    codes, offsets = Mo.encode_sequences(seqs)
    dev = (hip.to_device(codes, np.uint8), hip.to_device(offsets, np.int64))
    enc = ac.tl.scan_sequences(dev, matrices=mats, motifs=ids, backend=hip)
    assert enc["sequence"].tolist() == [r[0] for r in want] and enc["position"].tolist() == [r[2] for r in want]


def test_nothing_to_scan(hip):
    ids, mats = F.sub_bank(3)
    scanner = ac.tl.prepare_motif_scanner(mats, backend=hip)
    for seqs in ([], [""], ["", ""], ["NNNNNNNNNNNN"], ["ACG"]):
        got = ac.tl.scan_sequences_device(seqs, scanner)
        assert all(int(t.numel()) == 0 for t in got)
        assert [t.dtype for t in got] == [torch.int32, torch.int32, torch.int32, torch.float64]
