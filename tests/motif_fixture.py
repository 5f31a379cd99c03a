"""TEST INFRASTRUCTURE: the motif fixture - the 16 JASPAR matrices of tests/golden/jaspar_golden.npz, two synthetic ones, and the
sequences (random ones plus hand-built edge cases) that tests/test_motif_host.py and tests/test_gpu_motif.py scan."""
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
