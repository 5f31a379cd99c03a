"""TEST INFRASTRUCTURE: the motif fixture - the 16 JASPAR matrices of tests/golden/jaspar_golden.npz, two synthetic ones, and the
sequences (random ones plus hand-built edge cases) that tests/test_motif_host.py and tests/test_gpu_motif.py scan; below
them the exact (dyadic) banks, the edge streams and the cases of tests/test_gpu_motif_edges.py."""
import atexit
import functools
import os
import shutil
import tempfile

import numpy as np

from tests import motif_refs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jaspar_golden.npz")
IDS = ["MA0004.1", "MA0006.1", "MA0027.2", "MA0031.1", "MA0037.3", "MA0002.2", "MA0032.2", "MA0035.4", "MA0036.3",
       "MA0040.1", "MA0047.3", "MA0046.2", "MA0052.4", "MA0009.2", "MA0007.3", "MA1594.1"]
SHORT = IDS[:5]  # up to 8 columns: the enumeration is affordable
LENGTHS = {"MA0004.1": 6, "MA0006.1": 6, "MA0027.2": 8, "MA0031.1": 8, "MA0037.3": 8, "MA0002.2": 11, "MA0032.2": 11,
           "MA0035.4": 11, "MA0036.3": 11, "MA0040.1": 11, "MA0047.3": 11, "MA0046.2": 15, "MA0052.4": 15,
           "MA0009.2": 16, "MA0007.3": 17, "MA1594.1": 24}
RANDOM_LENGTHS = [5, 6, 23, 24, 25, 63, 64, 65, 127, 128, 129, 300, 511, 1000] + [200] * 26
PVALUES = (1e-4, 1e-2)
TILE = 256       # csrc/motif.hip's position tile (tests/test_gpu_motif.py checks it against the cap query)
LONG_COLUMNS = 33  # one more than the kernel's longest motif


@functools.lru_cache(maxsize=None)
def jaspar_dir():
    """a directory with the archive's files written back out: 16 ``.pfm`` files and ``motif_to_gene.txt``, byte for byte
    the reference's (tests/golden/make_jaspar_golden.py); removed when the interpreter exits"""
    d = tempfile.mkdtemp(prefix="muon_amd_jaspar_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    with np.load(GOLDEN) as z:
        for name in z.files:
            with open(os.path.join(d, name), "wb") as f:
                f.write(z[name].tobytes())
    return d


def files():
    return [os.path.join(jaspar_dir(), i + ".pfm") for i in IDS]


@functools.lru_cache(maxsize=None)
def jaspar_matrices():
    return tuple(motif_refs.log_odds(motif_refs.read_counts(f)) for f in files())


def _synthetic(columns, seed):
    """a peaked random count matrix: one base holds 70-97 of a column's 100 counts"""
    rng = np.random.default_rng(seed)
    c = np.zeros((4, columns))
    for j in range(columns):
        top = int(rng.integers(70, 98))
        rest = rng.multinomial(100 - top, [1 / 3] * 3)
        c[:, j] = np.insert(rest, int(rng.integers(0, 4)), top)
    return motif_refs.log_odds(c)


@functools.lru_cache(maxsize=None)
def bank():
    """(ids, matrices): the 16 JASPAR matrices, a synthetic 10-column one (the 17th for the kernel: a second tile of
    the bank) and a synthetic 33-column one (past the kernel's cap: the tensor formulation inside the same call)"""
    ids = IDS + ["SYN10", "SYN33"]
    return ids, list(jaspar_matrices()) + [_synthetic(10, 10), _synthetic(LONG_COLUMNS, 33)]


def sub_bank(n):
    """the first n motifs the kernel takes (n <= 17)"""
    ids, mats = bank()
    return ids[:n], mats[:n]


def consensus(M):
    return "".join("ACGT"[b] for b in np.argmax(M, axis=0))


def _letters(rng, n):
    return "".join("ACGT"[b] for b in rng.integers(0, 4, size=n))


@functools.lru_cache(maxsize=None)
def random_sequences():
    rng = np.random.default_rng(0)
    return tuple(_letters(rng, n) for n in RANDOM_LENGTHS)


@functools.lru_cache(maxsize=None)
def sequences(tile=TILE):
    """The scanned list.  First three sequences that END with a consensus word at stream positions ``tile``,
    ``2 tile - 1`` and ``3 tile + 1`` (the position-tile edge and a base either side); then the random ones; then the
    hand-built cases (see the comments)."""
    ids, mats = bank()
    rng = np.random.default_rng(1)
    w11 = consensus(mats[ids.index("MA0035.4")])   # 11 columns
    w24 = consensus(mats[ids.index("MA1594.1")])   # 24 columns
    w17 = consensus(mats[ids.index("MA0007.3")])
    w33 = consensus(mats[ids.index("SYN33")])
    out = [_letters(rng, tile - 24) + w24,            # ends at stream position tile
           _letters(rng, tile - 1 - 11) + w11,        # ends at 2 tile - 1
           _letters(rng, tile + 2 - 17) + w17]        # ends at 3 tile + 1
    assert [len(s) for s in out] == [tile, tile - 1, tile + 2]
    out += list(random_sequences())
    out += [
        w24 + _letters(rng, 30) + w24,                # the consensus at position 0 and at the last window
        w11,                                          # a sequence that is exactly one window
        _letters(rng, 20) + w24[:12], w24[12:] + _letters(rng, 20),   # the consensus split over two sequences: no hit
        w24[:12] + "N" + w24[13:],                    # an N in its middle: no hit
        w17[:8].lower() + w17[8:] + "n" + w17,        # lower case counts; the N ends the first word's room
        "",                                           # an empty sequence between two others
        _letters(rng, 40) + w33 + _letters(rng, 5),   # the long motif's consensus: the tensor formulation
        "NNNNNNNN",
    ]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def thresholds(pvalue):
    return tuple(motif_refs.scan_threshold(M, pvalue) for M in bank()[1])


@functools.lru_cache(maxsize=None)
def expected(pvalue, n_motifs=None, tile=TILE):
    """(rows, margin) of the restatement for the first ``n_motifs`` motifs of the bank (None: all of it)"""
    mats = bank()[1][:n_motifs]
    return motif_refs.scan(sequences(tile), mats, thresholds(pvalue)[:len(mats)])


# ---- exact banks and edge streams (tests/test_gpu_motif_edges.py; anchored on the CPU by tests/test_motif_host.py) ----
# Every entry of a dyadic matrix is a multiple of 1/64 in [-8, 2]: with at most 32 columns every partial sum is a
# multiple of 1/64 below 2^9 in magnitude, exact in f64 in any order, so a scan is compared with ==, thresholds that
# a score attains included.
CAP = 32     # csrc/motif.hip's longest motif
GROUP = 16   # ... and its motifs per tile of the bank


class Case:
    """One scan: a code stream with its offsets, a bank in the caller's order and the thresholds the test chose."""

    def __init__(self, codes, offsets, matrices, thresholds, **marks):
        self.codes = np.ascontiguousarray(codes, dtype=np.uint8)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        self.matrices = list(matrices)
        self.thresholds = np.asarray(thresholds, dtype=np.float64)
        self.lengths = np.array([M.shape[1] for M in self.matrices], dtype=np.int64)
        self.__dict__.update(marks)
        self._want = None

    @property
    def total(self):
        return int(self.codes.size)

    def want(self):
        """(sequence, motif, position, score) of the restatement, computed once"""
        if self._want is None:
            self._want = motif_refs.scan_stream(self.codes, self.offsets, self.matrices, self.thresholds)
        return self._want

    def want_keys(self):
        """the restatement's hits as (stream position, motif) pairs"""
        seq, mot, pos, _ = self.want()
        return self.offsets[seq] + pos, mot

    def head(self, n_seq):
        """the same scan over the first ``n_seq`` sequences only"""
        off = self.offsets[:n_seq + 1]
        return Case(self.codes[:off[-1]], off, self.matrices, self.thresholds)


def dyadic_bank(lengths, seed):
    """one 4 x L matrix per entry of ``lengths``: multiples of 1/64 in [-8, 2], the largest of a column only once (the
    best word is unique)"""
    rng = np.random.default_rng(seed)
    out = []
    for L in lengths:
        q = rng.integers(-512, 129, size=(4, int(L)))
        for j in range(int(L)):
            while np.sum(q[:, j] == q[:, j].max()) > 1:
                q[:, j] = rng.integers(-512, 129, size=4)
        out.append(q / 64.0)
    return out


def best_word(M):
    """(codes of the best word, its exact score added j-ascending)"""
    w = np.argmax(M, axis=0).astype(np.uint8)
    s = 0.0
    for j in range(M.shape[1]):
        s = s + M[w[j], j]
    return w, s


def code_stream(seq_lengths, seed, invalid=0.0):
    """(codes, offsets): random bases in sequences of the given lengths (0: an empty one); every code is invalid (4)
    with probability ``invalid``"""
    rng = np.random.default_rng(seed)
    offsets = np.zeros(len(seq_lengths) + 1, dtype=np.int64)
    np.cumsum(np.asarray(seq_lengths, dtype=np.int64), out=offsets[1:])
    codes = rng.integers(0, 4, size=int(offsets[-1])).astype(np.uint8)
    if invalid > 0:
        codes[rng.random(codes.size) < invalid] = 4
    return codes, offsets


def uneven_lengths(total, seed, mean=180):
    """sequence lengths that sum to ``total``: uneven (1 to about 4 ``mean``), every ninth one empty"""
    rng = np.random.default_rng(seed)
    out, left = [], int(total)
    while left > 0:
        n = 0 if len(out) % 9 == 4 else min(left, int(rng.integers(1, 2 * mean)) * int(rng.integers(1, 3)))
        out.append(n)
        left -= n
    return out + [0]


def kth_largest_thresholds(codes, offsets, matrices, keep):
    """per motif the ``keep[i]``-th largest score over its admissible windows (ties hit too): a value a window attains
    exactly, so ``score >= threshold`` is decided at equality for at least one window of every motif"""
    codes = np.minimum(np.asarray(codes), 4).astype(np.intp)
    room = motif_refs.stream_room(codes, offsets)
    thr = np.full(len(matrices), np.inf)
    for i, M in enumerate(matrices):
        score, ok = motif_refs.stream_scores(codes, room, M)
        s = np.sort(score[ok])[::-1]
        if s.size:
            thr[i] = s[min(int(keep[i]), s.size) - 1]
    return thr


def tile_of_motif(lengths, group=GROUP):
    """the bank tile every motif of the caller's order lands in: sorted by length (stable), ``group`` to a tile"""
    order = np.argsort(np.asarray(lengths), kind="stable")
    tile = np.empty(len(order), dtype=np.int64)
    tile[order] = np.arange(len(order)) // group
    return tile


def pair_counts(case, tile=TILE, group=GROUP):
    """hits of the restatement per (motif tile, position tile): int64 [n motif tiles, n position tiles]"""
    gpos, mot = case.want_keys()
    n_mt = -(-len(case.matrices) // group)
    n_pt = -(-case.total // tile)
    flat = tile_of_motif(case.lengths, group)[mot] * n_pt + gpos // tile
    return np.bincount(flat, minlength=n_mt * n_pt).reshape(n_mt, n_pt)


def scan_grid_x(n_cus, n_mtiles):
    """csrc/motif.hip's motif_grid_x before it is capped by the number of position tiles: the chip eight deep"""
    return -(-8 * n_cus // n_mtiles)


def room_grid(n_cus):
    """blocks of 256 positions k_motif_room is capped at"""
    return 16 * n_cus


EDGE_LENGTHS = [1, 31, 32, 33, 255, 0, 256, 257, 288, 0]


def edge_stream(seed=11):
    """sequences around the motif cap, the wave's 64 positions and the position tile, an empty one in the middle and
    one at the end, seven invalid codes scattered over the longer ones"""
    codes, offsets = code_stream(EDGE_LENGTHS, seed)
    rng = np.random.default_rng(seed + 1)
    codes[rng.choice(np.arange(int(offsets[4]), codes.size), size=7, replace=False)] = 4
    return codes, offsets


@functools.lru_cache(maxsize=None)
def case_every_length():
    """32 motifs, one per length 1..32, in a shuffled caller order; every threshold is the score at the top 3 % of the
    motif's admissible windows (short motifs have too few words for that: their best word's share)"""
    order = np.random.default_rng(3).permutation(CAP) + 1
    mats = dyadic_bank(order, 21)
    codes, offsets = edge_stream()
    room = motif_refs.stream_room(codes, offsets)
    keep = [max(1, int(0.03 * np.sum(room >= L))) for L in order]
    return Case(codes, offsets, mats, kth_largest_thresholds(codes, offsets, mats, keep))


@functools.lru_cache(maxsize=None)
def case_halo(L, tile=TILE):
    """The every-length bank, every threshold the score of the motif's best word, and the best word of the
    ``L``-column motif planted four times in random bases: at tile position ``tile - 1`` of position tile 0 (all of
    its other bases come from the halo: a hit), at ``tile - 1`` of tile 1 with its last base in the next sequence
    (none), at ``tile - 1`` of tile 2 with code 4 in its last column (none), and ending with the stream, whose length
    is no multiple of the tile (a hit).  ``planted``: the four stream positions."""
    base = case_every_length()
    M = base.matrices[int(np.flatnonzero(base.lengths == L)[0])]
    word, _ = best_word(M)
    total = 4 * tile + 100
    planted = [tile - 1, 2 * tile - 1, 3 * tile - 1, total - L]
    codes = np.random.default_rng(100 + L).integers(0, 4, size=total).astype(np.uint8)
    for g in planted:
        codes[g:g + L] = word
    codes[planted[2] + L - 1] = 4
    offsets = np.array([0, tile + 144, planted[1] + L - 1, total], dtype=np.int64)
    thr = [best_word(m)[1] for m in base.matrices]
    return Case(codes, offsets, base.matrices, thr, planted=planted, motif=int(np.flatnonzero(base.lengths == L)[0]))


DENSE_LENGTHS = [1, 4, 8, 31, 32, 2, 3, 5, 6, 7, 12, 16, 20, 24, 28, 30, 32]


@functools.lru_cache(maxsize=None)
def case_density(alternate, tile=TILE):
    """17 motifs (two tiles, the second one motif and 15 padding slots); one valid sequence of 3 tiles + 40 and one
    with an invalid code at every 7th position; thresholds -inf (every admissible window hits), or alternating -inf and
    +inf by motif"""
    mats = dyadic_bank(DENSE_LENGTHS, 22)
    codes, offsets = code_stream([3 * tile + 40, 300], 23)
    codes[int(offsets[1]) + 6::7] = 4
    thr = np.full(len(mats), -np.inf)
    if alternate:
        thr[1::2] = np.inf
    return Case(codes, offsets, mats, thr)


STRIDE_LENGTHS = [4 + (9 * i) // 33 for i in range(33)]  # 4..12, three tiles


@functools.lru_cache(maxsize=None)
def case_scan_stride(n_cus, tile=TILE):
    """33 motifs of 4..12 columns (three tiles) over ``2 grid_x + 41`` position tiles less 77 positions, many uneven
    sequences, 0.2 % invalid codes.  A motif keeps about 0.7 hits per 16 position tiles (the motif that has the third
    tile to itself: 0.7 per position tile), so in every motif tile a good share of the (motif tile, position tile)
    pairs is empty and a good share is not."""
    mats = dyadic_bank(STRIDE_LENGTHS, 24)
    grid_x = scan_grid_x(n_cus, 3)
    n_pt = 2 * grid_x + 41
    total = n_pt * tile - 77
    codes, offsets = code_stream(uneven_lengths(total, 25), 26, invalid=0.002)
    keep = [max(1, round(0.7 * n_pt / GROUP))] * 32 + [max(1, round(0.7 * n_pt))]
    thr = kth_largest_thresholds(codes, offsets, mats, keep)
    # the best word of a 4- or 5-column motif alone turns up in most position tiles (total / 4^L of them): these
    # cannot hit here, but for the first 5-column one, or the first motif tile would have no empty pair
    lengths = np.array(STRIDE_LENGTHS)
    thr[(lengths == 4) | ((lengths == 5) & (np.arange(33) != STRIDE_LENGTHS.index(5)))] = np.inf
    return Case(codes, offsets, mats, thr, grid_x=grid_x, n_ptiles=n_pt)


@functools.lru_cache(maxsize=None)
def room_stride_stream(n_cus, tile=TILE):
    """(codes, offsets) of ``2 * 16 CUs * 256 + 300`` positions: k_motif_room's threads take three positions each"""
    total = 2 * room_grid(n_cus) * 256 + 300
    return code_stream(uneven_lengths(total, 27, mean=400), 28, invalid=0.002)


@functools.lru_cache(maxsize=None)
def case_equality(L):
    """(at, above): the every-length scan with the threshold of the ``L``-column motif set to a score ``s`` that one
    of its windows attains exactly while others score higher - the median of its admissible scores - and to the next
    f64 above ``s``"""
    base = case_every_length()
    i = int(np.flatnonzero(base.lengths == L)[0])
    codes = np.minimum(base.codes, 4).astype(np.intp)
    score, ok = motif_refs.stream_scores(codes, motif_refs.stream_room(codes, base.offsets), base.matrices[i])
    s = float(np.sort(score[ok])[ok.sum() // 2])
    at, above = base.thresholds.copy(), base.thresholds.copy()
    at[i], above[i] = s, np.nextafter(s, np.inf)
    return (Case(base.codes, base.offsets, base.matrices, at, motif=i, score=s),
            Case(base.codes, base.offsets, base.matrices, above, motif=i, score=s))


# ---- what the restatement says about the cases: the properties each case exists for -------------------------------
def assert_every_motif_hits_and_misses(case):
    """every motif has a hit, and an admissible window that is none"""
    _, mot, _, _ = case.want()
    hits = np.bincount(mot, minlength=len(case.matrices))
    room = motif_refs.stream_room(case.codes, case.offsets)
    admissible = np.array([int(np.sum(room >= L)) for L in case.lengths])
    assert np.all(hits >= 1) and np.all(hits < admissible), (hits, admissible)


def assert_halo_plants(case, tile=TILE):
    """of the four planted words the first and the last are hits, the two in the middle are not"""
    gpos, mot = case.want_keys()
    mine = set(gpos[mot == case.motif].tolist())
    a, b, c, d = case.planted
    assert [g % tile for g in (a, b, c)] == [tile - 1] * 3 and case.total % tile != 0
    assert d + int(case.lengths[case.motif]) == case.total
    assert a in mine and d in mine and b not in mine and c not in mine


def assert_equality_pair(at, above):
    """``at`` holds windows of the motif that score exactly the threshold; ``above`` is ``at`` without them"""
    _, mot, _, score = at.want()
    tied = (mot == at.motif) & (score == at.score)
    assert at.thresholds[at.motif] == at.score < above.thresholds[at.motif]
    assert tied.sum() >= 1 and np.sum((mot == at.motif) & (score > at.score)) >= 1
    for a, b in zip(at.want(), above.want()):
        assert np.array_equal(a[~tied], b)


def assert_density(case, alternate, tile=TILE):
    """a (motif tile, position tile) pair holds all 16 * 256 hits (half of them when every other motif cannot hit),
    and the count is the number of admissible windows"""
    counts = pair_counts(case, tile)
    assert counts.shape[0] == 2 and len(case.matrices) == GROUP + 1
    room = motif_refs.stream_room(case.codes, case.offsets)
    live = np.isfinite(case.thresholds) | (case.thresholds < 0)  # -inf: every admissible window
    assert counts.sum() == sum(int(np.sum(room >= L)) for L in case.lengths[live])
    assert counts[0].max() == (GROUP * tile if not alternate else GROUP * tile // 2)
    assert counts[1].max() == (tile if live[np.argsort(case.lengths, kind="stable")[GROUP]] else 0)


def assert_stride_mixture(case, tile=TILE):
    """more than 10 % of the (motif tile, position tile) pairs have no hit and more than 10 % have one - overall, and
    inside every motif tile (a workgroup keeps its motif tile for its whole stride)"""
    counts = pair_counts(case, tile)
    empty = (counts == 0).mean(axis=1)
    assert counts.shape[0] == 3
    assert 0.1 < (counts == 0).mean() < 0.9 and np.all(empty > 0.1) and np.all(empty < 0.9), empty
