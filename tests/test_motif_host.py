"""muon_amd.atac.tl's motif tools without a GPU: the host arithmetic (parser, log-odds, the threshold's dynamic
programme) against the brute-force restatement tests/motif_refs.py, the tensor formulation of the scan through
tests/cpu_backend.CpuTestBackend against the restatement's sliding window, the frame layouts, the reference's assertion
cases and get_sequences.

Bound on the scores: at most 24 + 9 additions (the longest fixture motif has 33 columns) - the issue derives 1e-12 from
24 additions of partial sums no larger than 24 * 14: 24 * 336 * 2^-53 = 9e-13; the tensor formulation adds in the
restatement's order, so the scores are in fact equal, and 1e-12 is what is asked."""
import gzip
import math

import numpy as np
import pandas as pd
import pytest
import torch

from muon_amd import AnnData
from muon_amd import atac as ac
from muon_amd._atac import motifs as Mo
from tests import motif_fixture as F
from tests import motif_refs
from tests.cpu_backend import CpuTestBackend

BE = CpuTestBackend()


# ---- thresholds ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pvalue", F.PVALUES)
@pytest.mark.parametrize("mid", F.SHORT)
def test_dp_threshold_against_the_enumeration_of_all_words(mid, pvalue):
    M = F.jaspar_matrices()[F.IDS.index(mid)]
    T = Mo.threshold_total(M, 4, pvalue)
    assert T == motif_refs.dp_total(M, pvalue)
    assert Mo.threshold_from_p(M, 4, pvalue) == T / 1000.0
    S = motif_refs.rounded(M)
    highest = int(S.max(axis=0).sum())
    at, below = motif_refs.enumerated_tails(M, [T, T - 1])
    print(f"{mid} p={pvalue}: T={T} highest={highest} tail(T)={at:.3e} tail(T-1)={below:.3e}")
    assert at <= pvalue < below
    if T <= highest:  # (flat background: every probability is a multiple of 4^-L, the DP's sums are exact)
        tail, lowest, _ = motif_refs.dp_tails(M)
        assert tail[T - lowest] == at


def test_the_enumeration_helper_is_the_plain_loop():
    M = F.jaspar_matrices()[0]  # 6 columns: 4096 words
    T = motif_refs.dp_total(M, 1e-2)
    assert motif_refs.enumerated_tails(M, [T, T - 1]) == [motif_refs.enumerated_tail(M, T), motif_refs.enumerated_tail(M, T - 1)]


@pytest.mark.parametrize("mid", ["MA0004.1", "MA0006.1"])
def test_six_columns_have_no_attainable_threshold_at_1e_4(mid):
    """4^-6 = 2.44e-4 > 1e-4: even the best word alone is too likely"""
    M = F.jaspar_matrices()[F.IDS.index(mid)]
    highest = int(motif_refs.rounded(M).max(axis=0).sum())
    assert Mo.threshold_total(M, 4, 1e-4) == highest + 1
    assert Mo.threshold_from_p(M, 4, 1e-4) == (highest + 1) / 1000.0 and Mo.scan_threshold(M, 4, 1e-4) == math.inf
    word = F.consensus(M)
    hits = ac.tl.scan_sequences([word, "ACGT" * 10 + word], matrices=[M], motifs=[mid], backend=BE)
    assert len(hits) == 0 and list(hits.columns) == Mo.COLUMNS


@pytest.mark.parametrize("pvalue", F.PVALUES)
def test_every_threshold_is_the_restatements(pvalue):
    ids, mats = F.bank()
    assert [Mo.threshold_from_p(M, 4, pvalue) for M in mats] == [motif_refs.threshold(M, pvalue) for M in mats]
    assert [Mo.scan_threshold(M, 4, pvalue) for M in mats] == list(F.thresholds(pvalue))
    scanner = ac.tl.prepare_motif_scanner(mats, pvalue=pvalue, backend=BE)
    assert scanner.thresholds.tolist() == list(F.thresholds(pvalue))


def test_threshold_with_a_skewed_background():
    M = F.jaspar_matrices()[2]
    bg = [0.3, 0.2, 0.2, 0.3]
    T = Mo.threshold_total(M, bg, 1e-2)
    assert T == motif_refs.dp_total(M, 1e-2, bg)
    at, below = motif_refs.enumerated_tails(M, [T, T - 1], bg)
    assert at <= 1e-2 * (1 + 1e-12) and below > 1e-2 * (1 - 1e-12)  # (65536 products summed in another order)


# ---- the parser ---------------------------------------------------------------------------------------------------
def test_parser_against_hand_computed_log_odds_of_MA0004_1(tmp_path):
    got = Mo.parse_motif_matrices([F.files()[0]])
    assert got["motifs"] == ["MA0004.1"]
    M = got["matrices"][0]
    assert M.shape == (4, 6) and M.dtype == np.float64
    # every column of MA0004.1 sums to 20; the counts are 4 19 0 0 0 0 / 16 0 20 0 0 0 / 0 1 0 20 0 20 / 0 0 0 0 20 0
    def lo(c):
        return math.log((c + 1e-4 * 0.25) / (20 + 1e-4)) - math.log(0.25)

    want = np.array([[lo(4), lo(19), lo(0), lo(0), lo(0), lo(0)], [lo(16), lo(0), lo(20), lo(0), lo(0), lo(0)],
                     [lo(0), lo(1), lo(0), lo(20), lo(0), lo(20)], [lo(0), lo(0), lo(0), lo(0), lo(20), lo(0)]])
    np.testing.assert_allclose(M, want, rtol=1e-15, atol=0)
    assert abs(M[2, 3] - math.log(4.0)) < 1e-5 and abs(M[0, 2] - math.log(1e-4 / 20.0001)) < 1e-12
    # a header line is skipped; the id is the base name without .pfm (also when it ends in p, f or m)
    p = tmp_path / "amp.pfm"
    p.write_text(">amp some motif\n" + open(F.files()[0]).read())
    again = Mo.parse_motif_matrices([str(p)])
    assert again["motifs"] == ["amp"] and np.array_equal(again["matrices"][0], M)


def test_parser_takes_a_directory_and_says_that_jaspar_does_not_ship():
    with pytest.raises(ValueError, match="jaspar_dir"):
        Mo.parse_motif_matrices()
    got = Mo.parse_motif_matrices(jaspar_dir=F.jaspar_dir())
    assert got["motifs"] == sorted(F.IDS)
    for mid, M in zip(got["motifs"], got["matrices"]):
        np.testing.assert_allclose(M, F.jaspar_matrices()[F.IDS.index(mid)], rtol=1e-15, atol=0)
    meta = Mo.parse_motif_ids(jaspar_dir=F.jaspar_dir())
    assert meta.index.name == "motif_id" and list(meta.columns) == ["tf_gene_name"] and len(meta) == 16
    assert meta.loc["MA0004.1", "tf_gene_name"] == "Arnt"
    with pytest.raises(ValueError, match="jaspar_dir"):
        ac.tl.scan_sequences(["ACGT"], backend=BE)


# ---- encoding -----------------------------------------------------------------------------------------------------
def test_encoding():
    codes, offsets = Mo.encode_sequences(["ACGT", "acgt", "", "NnXR-", "A"])
    assert codes.dtype == np.uint8 and offsets.dtype == np.int64
    assert codes.tolist() == [0, 1, 2, 3, 0, 1, 2, 3, 4, 4, 4, 4, 4, 0]
    assert offsets.tolist() == [0, 4, 8, 8, 13, 14]
    room = Mo._room_tensor(torch.from_numpy(codes), torch.from_numpy(offsets))
    assert room.tolist() == [4, 3, 2, 1, 4, 3, 2, 1, 0, 0, 0, 0, 0, 1]


def test_short_empty_and_invalid_sequences_have_no_hits():
    ids, mats = F.sub_bank(16)
    M = mats[ids.index("MA0035.4")]
    w = F.consensus(M)
    seqs = ["", w[:-1], w, w.lower(), w[:5] + "N" + w[6:], "N" * 40]
    hits = ac.tl.scan_sequences(seqs, matrices=[M], motifs=["MA0035.4"], backend=BE)
    assert hits["sequence"].tolist() == [w, w.lower()] and hits["position"].tolist() == [0, 0]
    assert hits["score"].tolist() == [motif_refs.scan([w], [M], [0.0])[0][0][3]] * 2
    none = ac.tl.scan_sequences([], matrices=[M], motifs=["MA0035.4"], backend=BE)
    assert len(none) == 0 and list(none.columns) == Mo.COLUMNS


# ---- the scan through the CPU operator set (the tensor formulation) ----------------------------------------------
@pytest.mark.parametrize("pvalue", F.PVALUES)
def test_scan_is_the_restatements(pvalue):
    ids, mats = F.bank()
    seqs = list(F.sequences())
    rows, margin = F.expected(pvalue)
    print(f"p={pvalue}: {len(rows)} hits, smallest |score - threshold| {margin:.3e}")
    assert margin > 1e-9  # no window of the fixture sits where one rounding could move it across its threshold
    got = ac.tl.scan_sequences(seqs, matrices=mats, motifs=ids, pvalue=pvalue, backend=BE)
    assert list(got.columns) == Mo.COLUMNS
    assert got["sequence"].tolist() == [seqs[r[0]] for r in rows]
    assert got["motif_id"].tolist() == [ids[r[1]] for r in rows]
    assert got["position"].tolist() == [r[2] for r in rows]
    np.testing.assert_allclose(got["score"].to_numpy(), [r[3] for r in rows], rtol=0, atol=1e-12)
    # the hand-built cases did what they are there for
    by_motif = {(r[0], r[1]): [] for r in rows}
    for r in rows:
        by_motif[(r[0], r[1])].append(r[2])
    long_ = ids.index("MA1594.1")
    first_hand = 3 + len(F.RANDOM_LENGTHS)
    assert by_motif[(0, long_)][-1] == F.TILE - 24
    assert by_motif[(first_hand, long_)][0] == 0 and by_motif[(first_hand, long_)][-1] == 24 + 30
    for s in (first_hand + 2, first_hand + 3, first_hand + 4):
        assert (s, long_) not in by_motif
    assert (first_hand + 7, ids.index("SYN33")) in by_motif


def test_encoded_input_and_the_device_arrays():
    ids, mats = F.bank()
    seqs = list(F.sequences())
    rows, _ = F.expected(1e-2)
    scanner = ac.tl.prepare_motif_scanner(mats, pvalue=1e-2, backend=BE)
    assert scanner.bank is None and len(scanner.tensor) == len(mats)
    enc = Mo.encode_sequences(seqs)
    seq, mot, pos, score = ac.tl.scan_sequences_device(enc, scanner)
    assert (seq.dtype, mot.dtype, pos.dtype, score.dtype) == (torch.int32, torch.int32, torch.int32, torch.float64)
    assert seq.tolist() == [r[0] for r in rows] and mot.tolist() == [r[1] for r in rows]
    assert pos.tolist() == [r[2] for r in rows]
    again = ac.tl.scan_sequences_device(enc, scanner)
    assert all(torch.equal(a, b) for a, b in zip((seq, mot, pos, score), again))
    frame = ac.tl.scan_sequences(enc, motif_scanner=scanner, motifs=ids)
    assert frame["sequence"].tolist() == [r[0] for r in rows]  # (no strings to show: the index)
    # a chunk boundary inside a window changes nothing
    parts = Mo._scan_tensor(torch.from_numpy(enc[0]), torch.from_numpy(enc[1]), scanner.tensor, scanner.thresholds, chunk=97)
    whole = Mo._scan_tensor(torch.from_numpy(enc[0]), torch.from_numpy(enc[1]), scanner.tensor, scanner.thresholds)
    key = lambda t: sorted(zip(t[0].tolist(), t[1].tolist(), t[2].tolist()))  # noqa: E731
    assert key(parts) == key(whole)
    with pytest.raises(ValueError, match="offsets"):
        ac.tl.scan_sequences_device((enc[0], enc[1][:-1]), scanner)


def test_frame_layouts():
    ids, mats = F.sub_bank(16)
    seqs = list(F.sequences())
    meta = Mo.parse_motif_ids(jaspar_dir=F.jaspar_dir())
    plain = ac.tl.scan_sequences(seqs, matrices=mats, motifs=ids, pvalue=1e-2, backend=BE)
    joined = ac.tl.scan_sequences(seqs, matrices=mats, motifs=ids, motif_meta=meta, pvalue=1e-2, backend=BE)
    assert list(plain.columns) == ["sequence", "motif_id", "position", "score"]
    assert list(joined.columns) == ["motif_id", "sequence", "position", "score", "tf_gene_name"]
    assert len(joined) == len(plain) > 0  # rows in left order
    for c in ("sequence", "motif_id", "position", "score"):
        assert joined[c].tolist() == plain[c].tolist()
    assert joined["tf_gene_name"].tolist() == [meta.loc[m, "tf_gene_name"] for m in plain["motif_id"]]
    want = pd.DataFrame([(r.sequence, r.motif_id, r.position, r.score) for r in plain.itertuples()],
                        columns=["sequence", "motif_id", "position", "score"]).set_index("motif_id").join(meta, how="left").reset_index()
    pd.testing.assert_frame_equal(joined, want)
    # the default collection brings its own metadata
    default = ac.tl.scan_sequences(seqs, pvalue=1e-2, backend=BE, jaspar_dir=F.jaspar_dir())
    assert list(default.columns) == list(joined.columns) and len(default) == len(plain)
    # max_hits is accepted and limits nothing
    assert len(ac.tl.scan_sequences(seqs, matrices=mats, motifs=ids, pvalue=1e-2, max_hits=1, backend=BE)) == len(plain)


def test_the_references_assertions():
    ids, mats = F.sub_bank(2)
    with pytest.raises(AssertionError, match="Both a list of matrices"):
        ac.tl.scan_sequences(["ACGT"], matrices=mats, backend=BE)
    scanner = ac.tl.prepare_motif_scanner(mats, backend=BE)
    with pytest.raises(AssertionError, match="corresponds to the matrices"):
        ac.tl.scan_sequences(["ACGT"], motif_scanner=scanner)
    with pytest.raises(ValueError, match="one motif ID per matrix"):
        ac.tl.scan_sequences(["ACGT"], motif_scanner=scanner, motifs=ids[:1])
    with pytest.raises(ValueError, match="pseudocount"):
        Mo.threshold_from_p(Mo.log_odds(Mo.read_pfm(F.files()[0]), pseudocount=0.0))  # ln 0 in it


# ---- get_sequences ------------------------------------------------------------------------------------------------
FASTA = ">chr1 first record\nACGTACGTAC\nGTTTGA\n>chr2\nnnnnACGT\n>chrM extra\nGGGCCC\n"


@pytest.mark.parametrize("zipped", [False, True])
def test_get_sequences(tmp_path, zipped):
    path = tmp_path / ("genome.fa.gz" if zipped else "genome.fa")
    if zipped:
        with gzip.open(path, "wt") as f:
            f.write(FASTA)
    else:
        path.write_text(FASTA)
    ad = AnnData(np.zeros((2, 4), dtype=np.float32))
    ad.var_names = ["chr1:0-4", "chr1:8-16", "chr2:2-8", "chrM:5-6"]  # (chr1:8-16 ends at the record's last base)
    got = ac.tl.get_sequences(ad, fasta_file=str(path))
    assert got == ["ACGT", "ACGTTTGA", "nnACGT", "C"]
    assert ad.uns["files"]["genome"] == str(path)
    assert ac.tl.get_sequences(ad, bed="chr2\t4\t8\nchr1\t15\t16\n") == ["ACGT", "A"]  # (the recorded genome)
    bed = tmp_path / "peaks.bed"
    bed.write_text("chrM\t0\t3\tname\n")
    assert ac.tl.get_sequences(ad, bed_file=str(bed)) == ["GGG"]
    with pytest.raises(ValueError, match="leaves the record"):
        ac.tl.get_sequences(ad, bed="chr1\t10\t17\n")
    with pytest.raises(ValueError, match="no such record"):
        ac.tl.get_sequences(ad, bed="chr9\t0\t1\n")


def test_get_sequences_error_cases(tmp_path):
    ad = AnnData(np.zeros((2, 1), dtype=np.float32))
    with pytest.raises(TypeError, match="Expected AnnData or MuData"):
        ac.tl.get_sequences(np.zeros(3), fasta_file="x")
    with pytest.raises(FileNotFoundError, match="Genome file has to be provided"):
        ac.tl.get_sequences(ad)
    with pytest.raises(FileNotFoundError, match="does not exist"):
        ac.tl.get_sequences(ad, fasta_file=str(tmp_path / "missing.fa"))
    assert "files" not in ad.uns


# ---- the library ----------------------------------------------------------------------------------------------------
def test_entry_points():
    from muon_amd import _ffi

    lib = _ffi.lib()
    assert lib.mu_version() >= 805
    assert (lib.mu_motif_max_len(), lib.mu_motif_tile(), lib.mu_motif_group()) == (32, F.TILE, 16)
    assert F.LONG_COLUMNS == lib.mu_motif_max_len() + 1
    assert lib.mu_motif_room(8, 0, None, None, None, None) == -1 and b"n_seq >= 1" in lib.mu_last_error()
    assert lib.mu_motif_room(8, 1, None, None, None, None) == -1 and b"null pointer" in lib.mu_last_error()
    assert lib.mu_motif_count(8, 1, 0, *[None] * 8) == -1 and b"motif tiles" in lib.mu_last_error()
    assert lib.mu_motif_count(8, 1, 1, *[None] * 8) == -1 and b"null pointer" in lib.mu_last_error()
    assert lib.mu_motif_write(8, 1, 1, *[None] * 10, -1, *[None] * 5) == -1 and b"negative hit count" in lib.mu_last_error()
    assert lib.mu_motif_write(8, 1, 1, *[None] * 10, 4, *[None] * 5) == -1 and b"null pointer" in lib.mu_last_error()


# ---- the vectorised restatement and the cases of tests/test_gpu_motif_edges.py, without a GPU ---------------------
@pytest.mark.parametrize("pvalue", F.PVALUES)
def test_scan_stream_is_the_row_by_row_restatement(pvalue):
    """motif_refs.scan_stream (one sliding window over the whole stream, admissibility from the room) against
    motif_refs.scan (sequence by sequence) on the fixture: rows equal, scores bit for bit"""
    ids, mats = F.bank()
    seqs = list(F.sequences())
    rows, _ = F.expected(pvalue)
    codes = np.concatenate([motif_refs.encode(s) for s in seqs]).astype(np.uint8)
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    seq, mot, pos, score = motif_refs.scan_stream(codes, offsets, mats, F.thresholds(pvalue))
    assert list(zip(seq.tolist(), mot.tolist(), pos.tolist())) == [r[:3] for r in rows] and len(rows) > 0
    assert score.tobytes() == np.array([r[3] for r in rows], dtype=np.float64).tobytes()
    room = motif_refs.stream_room(codes, offsets)
    assert room.tolist() == Mo._room_tensor(torch.from_numpy(codes), torch.from_numpy(offsets)).tolist()


def _tensor_scan_equals(case):
    """the tensor formulation on the CPU operator set against the restatement, exactly"""
    scanner = Mo.MotifScanner(BE, case.matrices, case.thresholds)
    assert scanner.bank is None
    got = [t.numpy() for t in Mo.scan_sequences_device((case.codes, case.offsets), scanner)]
    for a, b in zip(got, case.want()):
        assert np.array_equal(a, b)
    return len(got[0])


def test_dyadic_banks_are_exact():
    for M in F.dyadic_bank([1, 7, 32], 0):
        q = M * 64
        assert np.array_equal(q, np.round(q)) and M.min() >= -8 and M.max() <= 2
        assert all(np.sum(M[:, j] == M[:, j].max()) == 1 for j in range(M.shape[1]))
    # 32 columns of multiples of 1/64 up to 8 in magnitude: every partial sum fits in 15 bits, whatever the order
    assert 32 * 8 * 64 < 2 ** 53


def test_edge_cases_on_the_tensor_formulation():
    """every case of tests/test_gpu_motif_edges.py that needs no large stream: the properties each exists for, asserted
    from the restatement, and the tensor formulation equal to the restatement"""
    case = F.case_every_length()
    assert sorted(case.lengths.tolist()) == list(range(1, F.CAP + 1))
    assert np.diff(case.offsets).tolist() == F.EDGE_LENGTHS and int(np.sum(case.codes == 4)) == 7
    F.assert_every_motif_hits_and_misses(case)
    assert set(F.tile_of_motif(case.lengths).tolist()) == {0, 1}
    assert _tensor_scan_equals(case) > 0
    for L in (32, 25):
        halo = F.case_halo(L)
        F.assert_halo_plants(halo)
        assert _tensor_scan_equals(halo) > 0
    for L in (1, 16, 32):
        at, above = F.case_equality(L)
        F.assert_equality_pair(at, above)
        assert _tensor_scan_equals(at) > _tensor_scan_equals(above)
    for alternate in (False, True):
        dense = F.case_density(alternate)
        F.assert_density(dense, alternate)
        assert _tensor_scan_equals(dense) == F.pair_counts(dense).sum()


def test_stride_cases_cross_the_grid_of_a_256_cu_part():
    case = F.case_scan_stride(256)
    assert (case.grid_x, case.n_ptiles, case.total) == (683, 1407, 360115)
    assert -(-case.total // F.TILE) >= 2 * F.scan_grid_x(256, 3) + 1 and len(case.matrices) == 33
    assert sorted(set(case.lengths.tolist())) == list(range(4, 13)) and F.tile_of_motif(case.lengths).max() == 2
    seq_len = np.diff(case.offsets)
    assert (seq_len == 0).sum() > 100 and len(set(seq_len.tolist())) > 100
    assert 0.001 < np.mean(case.codes == 4) < 0.003
    F.assert_stride_mixture(case)
    head = case.head(200)  # the tensor formulation on the first 200 sequences
    assert head.total > 20 * F.TILE and _tensor_scan_equals(head) > 0
    codes, offsets = F.room_stride_stream(256)
    assert codes.size == 2 * 16 * 256 * 256 + 300
    room = Mo._room_tensor(torch.from_numpy(codes), torch.from_numpy(offsets))
    assert np.array_equal(room.numpy(), motif_refs.stream_room(codes, offsets))
