"""The motif tools of ``muon.atac.tl`` (/root/reference/muon/_atac/tools.py:381-566): ``scan_sequences`` with its
helpers and ``get_sequences``, with the scan itself on the device (csrc/motif.hip).

The reference hands the arithmetic to MOODS; MOODS is not a dependency here and its arithmetic is STATED (DESIGN.md
9.10; parity with MOODS itself is not pinned by a test).  All of it is f64:

  alphabet    ``A C G T`` -> 0..3, lower case like upper case, every other character invalid (code 4).
  log-odds    ``M[b, j] = ln((c[b, j] + ps bg[b]) / (sum_b c[b, j] + ps)) - ln(bg[b])`` of a count matrix ``c``.
  threshold   ``S = round-half-away-from-zero(precision M)`` as integers; the distribution of ``sum_j S[b_j, j]`` under
              independent background draws is built exactly by dynamic programming (bases added in the order A C G T);
              the tail is summed from the largest total downwards; ``T`` is the smallest integer total with
              ``P(total >= T) <= pvalue`` (largest total + 1 if there is none: the motif cannot hit - a scanner
              then compares with +inf, ``scan_threshold``); ``threshold = T / precision``.  Host, numpy: one
              implementation serves every path.
  hit         window ``pos .. pos + L - 1`` lies inside its sequence, holds no invalid character, and the j-ascending
              sum ``M[base[pos + j], j]`` (the unrounded M) is ``>= threshold``.  Forward strand only.
  order       sequence as given, then motif as given, then position ascending.

Documented differences from the reference:
  * the JASPAR collection does not ship with the package: ``files=None`` / ``matrices=None`` need ``jaspar_dir``;
  * ``max_hits`` is accepted and ignored (the reference hands it to MOODS as the scanner's WINDOW SIZE: it limits
    nothing there either);
  * no hits give an empty frame with the reference's columns (the reference raises on the empty frame);
  * a motif id is the file's base name without ``.pfm`` (the reference's ``rstrip('.pfm')`` also eats trailing
    ``p``, ``f``, ``m`` and ``.`` characters of the name itself);
  * ``get_sequences`` reads the FASTA on the host without pybedtools; an interval that leaves its record raises.

Out of scope: the reverse strand, a peaks x motifs matrix, tabix / indexed FASTA access.
"""
from __future__ import annotations

import gzip
import os
from collections.abc import Iterable
from glob import glob
from typing import Optional

import numpy as np
import torch

from .._backend import backend_or_default
from .._containers import modality
from .._operators import has

COLUMNS = ["sequence", "motif_id", "position", "score"]
TENSOR_CHUNK = 1 << 22  # stream positions the tensor formulation scores at a time

_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _i


def _background(background):
    if not isinstance(background, Iterable):
        n = int(background)
        return np.full(n, 1.0 / n)
    return np.asarray(list(background), dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# matrices and thresholds (host)
# ---------------------------------------------------------------------------------------------------------------------
def read_pfm(filename) -> np.ndarray:
    """The 4 x L count matrix of a ``.pfm`` file: four lines of counts for A, C, G, T; a ``>`` header is skipped."""
    rows = []
    with open(filename) as f:
        for line in f:
            line = line.strip()
            if not line or line.startswith(">"):
                continue
            rows.append([float(tok) for tok in line.split()])
    if len(rows) != 4 or len({len(r) for r in rows}) != 1 or not rows[0]:
        raise ValueError(f"{filename}: expected four rows of counts of one length")
    return np.asarray(rows, dtype=np.float64)


def log_odds(counts, background=4, pseudocount: float = 1e-4) -> np.ndarray:
    """``ln((c + ps bg) / (column sum + ps)) - ln(bg)`` of a 4 x L count matrix."""
    c = np.asarray(counts, dtype=np.float64)
    bg = _background(background)
    if c.ndim != 2 or c.shape[0] != bg.size:
        raise ValueError("counts: one row per letter of the background")
    with np.errstate(divide="ignore"):
        return np.log((c + pseudocount * bg[:, None]) / (c.sum(axis=0) + pseudocount)[None, :]) - np.log(bg)[:, None]


def parse_motif_matrices(files=None, background=4, pseudocount: float = 1e-4, *, jaspar_dir: Optional[str] = None):
    """
    Log-odds matrices of ``.pfm`` files: ``{"motifs": [ids], "matrices": [4 x L arrays]}``; the id of a motif is its
    file's base name without ``.pfm``.  The JASPAR collection does not ship with the package: without ``files`` the
    ``.pfm`` files of ``jaspar_dir`` are taken (sorted by name).
    """
    if isinstance(files, (str, os.PathLike)):
        files = [files]
    if files is None:
        if jaspar_dir is None:
            raise ValueError("the JASPAR collection does not ship with muon_amd: pass `files` or `jaspar_dir`, "
                             "a directory of .pfm files")
        files = sorted(glob(os.path.join(os.fspath(jaspar_dir), "*.pfm")))
        if not files:
            raise ValueError(f"no .pfm files in {jaspar_dir!r}")
    files = [os.fspath(f) for f in files]
    ids = [os.path.basename(f)[:-4] if f.endswith(".pfm") else os.path.basename(f) for f in files]
    return {"motifs": ids, "matrices": [log_odds(read_pfm(f), background, pseudocount) for f in files]}


def parse_motif_ids(filename=None, *, jaspar_dir: Optional[str] = None):
    """The two-column table motif id -> transcription factor gene name, indexed by ``motif_id``."""
    import pandas as pd

    if filename is None:
        if jaspar_dir is None:
            raise ValueError("the JASPAR collection does not ship with muon_amd: pass `filename` or `jaspar_dir`")
        filename = os.path.join(os.fspath(jaspar_dir), "motif_to_gene.txt")
    motifs = pd.read_csv(filename, sep="\t", header=None)
    motifs.columns = ["motif_id", "tf_gene_name"]
    return motifs.set_index("motif_id")


def _score_distribution(matrix, background, precision):
    """(probabilities of every integer total from ``lowest`` upwards, lowest) of the rounded matrix."""
    M = np.asarray(matrix, dtype=np.float64)
    bg = _background(background)
    if M.ndim != 2 or M.shape[0] != bg.size or M.shape[1] < 1:
        raise ValueError("matrix: one row per letter of the background, at least one column")
    x = precision * M
    if not np.all(np.isfinite(x)):
        raise ValueError("matrix: not finite (a zero count needs a pseudocount)")
    S = (np.sign(x) * np.floor(np.abs(x) + 0.5)).astype(np.int64)  # half away from zero
    dist = np.ones(1)
    lowest = 0
    for j in range(S.shape[1]):
        lo, hi = int(S[:, j].min()), int(S[:, j].max())
        new = np.zeros(dist.size + hi - lo)
        for b in range(S.shape[0]):  # A, C, G, T
            o = int(S[b, j]) - lo
            new[o:o + dist.size] += bg[b] * dist
        dist = new
        lowest += lo
    return dist, lowest


def threshold_total(matrix, background=4, pvalue: float = 1e-4, precision: float = 1000.0) -> int:
    """``T``: the smallest integer total of the rounded matrix with ``P(total >= T) <= pvalue`` (largest + 1: none)."""
    dist, lowest = _score_distribution(matrix, background, precision)
    tails = np.cumsum(dist[::-1])  # tails[i] = P(total >= highest - i): ascending
    k = int(np.searchsorted(tails, pvalue, side="right"))  # the first k tails are <= pvalue
    highest = lowest + dist.size - 1
    return highest - (k - 1) if k > 0 else highest + 1


def threshold_from_p(matrix, background=4, pvalue: float = 1e-4, precision: float = 1000.0) -> float:
    """The score threshold of ``pvalue`` for a log-odds matrix (see the module docstring)."""
    return threshold_total(matrix, background, pvalue, precision) / precision


def scan_threshold(matrix, background=4, pvalue: float = 1e-4, precision: float = 1000.0) -> float:
    """What a scanner compares the scores of ``matrix`` with: ``threshold_from_p``, or ``+inf`` when even the largest
    rounded total is too likely (T = largest + 1): such a motif cannot hit.  (The unrounded scores are not bound by the
    rounded totals - the best word of MA0004.1 scores 8.0433 against (8042 + 1) / 1000 - so the comparison alone would
    not keep that promise.)"""
    dist, lowest = _score_distribution(matrix, background, precision)
    T = threshold_total(matrix, background, pvalue, precision)
    return T / precision if T <= lowest + dist.size - 1 else float("inf")


# ---------------------------------------------------------------------------------------------------------------------
# the scanner
# ---------------------------------------------------------------------------------------------------------------------
class MotifScanner:
    """A motif bank on the device, ready to scan: what ``prepare_motif_scanner`` returns.

    ``matrices`` / ``lengths`` / ``thresholds`` are in the caller's order (host).  ``bank`` holds the motifs the kernel
    takes - at most ``motif_max_len()`` columns, every value finite - sorted by length, padded to tiles of
    ``motif_group()`` motifs, with their thresholds (None: the operator set has no kernel, or no motif qualifies);
    ``tensor`` lists the others as ``(index, [5 x L] table with a zero row for the invalid code)`` for the tensor
    formulation.  ``use_kernel=False`` puts every motif on the tensor formulation."""

    def __init__(self, backend, matrices, thresholds, *, use_kernel: Optional[bool] = None, max_hits: int = 10):
        self.backend = backend
        self.matrices = [np.ascontiguousarray(m, dtype=np.float64) for m in matrices]
        for m in self.matrices:
            if m.ndim != 2 or m.shape[0] != 4 or m.shape[1] < 1:
                raise ValueError("every matrix is 4 x L with L >= 1")
        self.n_motifs = len(self.matrices)
        self.lengths = np.asarray([m.shape[1] for m in self.matrices], dtype=np.int64)
        self.thresholds = np.asarray(thresholds, dtype=np.float64).reshape(-1)
        if self.thresholds.size != self.n_motifs:
            raise ValueError("one threshold per matrix")
        self.max_hits = max_hits  # kept for the signature; limits nothing
        has_kernel = has(backend, "motif_scan")
        if use_kernel is None:
            use_kernel = has_kernel
        elif use_kernel and not has_kernel:
            raise ValueError("this operator set has no motif kernel")
        cap = backend.motif_max_len() if use_kernel else 0
        on_kernel = [i for i, m in enumerate(self.matrices) if m.shape[1] <= cap and np.all(np.isfinite(m))]
        taken = set(on_kernel)
        self.bank = self._pack(on_kernel) if on_kernel else None
        self.tensor = []
        for i, m in enumerate(self.matrices):
            if i not in taken:
                table = np.zeros((5, m.shape[1]))
                table[:4] = m
                self.tensor.append((i, backend.to_device(table, np.float64)))

    def _pack(self, idx):
        be = self.backend
        cap, group = be.motif_max_len(), be.motif_group()
        order = sorted(idx, key=lambda i: self.lengths[i])  # (stable: equal lengths keep the caller's order)
        n_tiles = -(-len(order) // group)
        bank = np.zeros((n_tiles, cap, 4, group))
        mlen = np.full(n_tiles * group, 255, dtype=np.int32)
        thr = np.full(n_tiles * group, np.inf)
        orig = np.zeros(n_tiles * group, dtype=np.int32)
        for s, i in enumerate(order):
            L = int(self.lengths[i])
            bank[s // group, :L, :, s % group] = self.matrices[i].T
            mlen[s], thr[s], orig[s] = L, self.thresholds[i], i
        tile_len = np.where(mlen.reshape(n_tiles, group) == 255, 0, mlen.reshape(n_tiles, group)).max(axis=1)
        return {"n_tiles": n_tiles, "bank": be.to_device(bank, np.float64),
                "tile_len": be.to_device(tile_len.astype(np.int32), np.int32), "mlen": be.to_device(mlen, np.int32),
                "thr": be.to_device(thr, np.float64), "orig": be.to_device(orig, np.int32)}


def prepare_motif_scanner(matrices=None, background=4, pvalue: float = 1e-4, max_hits: int = 10, *, backend=None,
                          jaspar_dir: Optional[str] = None, use_kernel: Optional[bool] = None) -> MotifScanner:
    """
    A ``MotifScanner`` for log-odds ``matrices`` (4 x L arrays; None: the ``.pfm`` files of ``jaspar_dir``) with the
    score thresholds of ``pvalue`` under ``background``.  ``max_hits`` is ignored: the reference hands it to MOODS as
    the scanner's window size, where it limits nothing either.
    """
    if matrices is None:
        matrices = parse_motif_matrices(files=None, background=background, jaspar_dir=jaspar_dir)["matrices"]
    thresholds = [scan_threshold(m, background, pvalue) for m in matrices]
    return MotifScanner(backend_or_default(backend), matrices, thresholds, use_kernel=use_kernel, max_hits=max_hits)


# ---------------------------------------------------------------------------------------------------------------------
# sequences
# ---------------------------------------------------------------------------------------------------------------------
def encode_sequences(sequences):
    """``(codes uint8 [total], offsets int64 [n + 1])`` of a list of strings: A C G T (either case) -> 0..3, else 4."""
    seqs = [sequences] if isinstance(sequences, str) else list(sequences)
    lens = np.fromiter((len(s) for s in seqs), dtype=np.int64, count=len(seqs))
    offsets = np.zeros(len(seqs) + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    raw = np.frombuffer("".join(seqs).encode("latin-1", "replace"), dtype=np.uint8)
    return _CODE[raw], offsets


def _is_encoded(sequences) -> bool:
    return (isinstance(sequences, tuple) and len(sequences) == 2
            and all(isinstance(a, (np.ndarray, torch.Tensor)) for a in sequences))


def _to_stream(backend, sequences):
    """(codes, offsets) on the device, checked."""
    if _is_encoded(sequences):
        codes, offsets = sequences
    else:
        codes, offsets = encode_sequences(sequences)
    if not isinstance(codes, torch.Tensor):
        codes = backend.to_device(np.asarray(codes), np.uint8)
    if not isinstance(offsets, torch.Tensor):
        offsets = backend.to_device(np.asarray(offsets), np.int64)
    if codes.dtype != torch.uint8 or offsets.dtype != torch.int64 or codes.dim() != 1 or offsets.dim() != 1:
        raise TypeError("encoded sequences: codes uint8 [total], offsets int64 [n + 1]")
    total = int(codes.numel())
    if offsets.numel() < 1:
        raise ValueError("offsets: n + 1 entries")
    if offsets.numel() > 1:
        step = offsets[1:] - offsets[:-1]
        ok = int(offsets[0]) == 0 and int(offsets[-1]) == total and bool((step >= 0).all())
    else:
        ok = int(offsets[0]) == 0 and total == 0
    if not ok:
        raise ValueError("offsets: 0 first, ascending, the stream's length last")
    return codes.contiguous(), offsets.contiguous()


def _room_tensor(codes, offsets):
    """Valid codes from every stream position to the next invalid one or the end of its sequence (int64, uncapped)."""
    total = int(codes.numel())
    dev = codes.device
    p = torch.arange(total, dtype=torch.int64, device=dev)
    ends = torch.repeat_interleave(offsets[1:], offsets[1:] - offsets[:-1])
    stop = torch.where(codes >= 4, p, torch.full_like(p, total))
    nxt = torch.flip(torch.cummin(torch.flip(stop, [0]), 0).values, [0])
    return torch.minimum(nxt, ends) - p


def _scan_tensor(codes, offsets, tables, thresholds, chunk: int = TENSOR_CHUNK):
    """The tensor formulation: for every motif of ``tables`` ((index, [5 x L] device table) pairs) the j-ascending f64
    sum of ``table[:, j][codes[pos + j]]`` over a sliding view, compared with the threshold and the room.  Returns the
    hits ``(global position int64, motif int64, score f64)`` in no promised order."""
    total = int(codes.numel())
    dev = codes.device
    room = _room_tensor(codes, offsets)
    gp, mi, sc = [], [], []
    longest = max((int(t.shape[1]) for _, t in tables), default=1)
    for c0 in range(0, total, max(int(chunk), 1)):
        c1 = min(total, c0 + int(chunk))
        view = codes[c0:min(total, c1 + longest - 1)].long()
        for i, table in tables:
            L = int(table.shape[1])
            n = min(c1, total - L + 1) - c0
            if n <= 0:
                continue
            score = table[:, 0][view[0:n]]
            for j in range(1, L):
                score = score + table[:, j][view[j:j + n]]
            hit = torch.nonzero((score >= float(thresholds[i])) & (room[c0:c0 + n] >= L)).reshape(-1)
            if hit.numel():
                gp.append(hit + c0)
                mi.append(torch.full_like(hit, i))
                sc.append(score[hit])
    if not gp:
        e = torch.empty(0, dtype=torch.int64, device=dev)
        return e, e.clone(), torch.empty(0, dtype=torch.float64, device=dev)
    return torch.cat(gp), torch.cat(mi), torch.cat(sc)


def scan_sequences_device(sequences, motif_scanner: MotifScanner, *, backend=None):
    """
    The hits of ``motif_scanner``'s bank in ``sequences`` (a list of strings or an encoded ``(codes, offsets)`` pair, on
    the host or on the device) as four device arrays ``(sequence index int32, motif index int32, position int32,
    score f64)``, ordered by sequence, then motif (the caller's order), then position.  Motifs the kernel does not take
    (longer than ``motif_max_len()``, or not finite) are scored by the tensor formulation inside the same call; two
    calls return byte-equal arrays.
    """
    be = motif_scanner.backend if backend is None else backend
    codes, offsets = _to_stream(be, sequences)
    n_seq = int(offsets.numel()) - 1
    dev = codes.device
    parts = []
    if int(codes.numel()) and n_seq >= 1:
        if motif_scanner.bank is not None:
            seq, mot, pos, score = be.motif_scan(codes, offsets, motif_scanner.bank)
            parts.append((offsets[seq.long()] + pos.long(), mot.long(), score))
        if motif_scanner.tensor:
            parts.append(_scan_tensor(codes, offsets, motif_scanner.tensor, motif_scanner.thresholds))
    if not parts or not sum(int(p[0].numel()) for p in parts):
        e = torch.empty(0, dtype=torch.int32, device=dev)
        return e, e.clone(), e.clone(), torch.empty(0, dtype=torch.float64, device=dev)
    gpos, mot, score = (torch.cat([p[k] for p in parts]) for k in range(3))
    seq = torch.searchsorted(offsets, gpos, right=True) - 1  # (empty sequences own no position)
    # (position in the stream, motif) names a hit: sorted by it and then, stably, by (sequence, motif), the rows are in
    # the reference's loop order whatever order the hits were found in
    o1 = torch.sort(gpos, stable=True).indices
    o2 = torch.sort((seq * motif_scanner.n_motifs + mot)[o1], stable=True).indices
    perm = o1[o2]
    seq, gpos = seq[perm], gpos[perm]
    return (seq.to(torch.int32), mot[perm].to(torch.int32), (gpos - offsets[seq]).to(torch.int32),
            score[perm].contiguous())


def scan_sequences(sequences, motif_scanner=None, matrices=None, motifs=None, motif_meta=None, background=4,
                   pvalue: float = 1e-4, max_hits: int = 10, *, backend=None, jaspar_dir: Optional[str] = None):
    """
    Scan sequences (e.g. peaks) for motifs on the device.

    sequences
            A list of strings, or an encoded ``(codes, offsets)`` pair (``encode_sequences``); the ``sequence`` column
            then holds the sequence's index instead of its string.
    motif_scanner, matrices, motifs, motif_meta, background, pvalue
            As in the reference: a prepared scanner with its motif ids, or log-odds matrices with their ids, or neither
            for the JASPAR collection - which does not ship with the package: ``jaspar_dir`` names a directory with
            its ``.pfm`` files and ``motif_to_gene.txt``.
    max_hits
            Ignored.  The reference hands it to MOODS as the scanner's window size; it limits nothing there either.

    Returns the reference's DataFrame: ``sequence, motif_id, position, score``, one row per hit, by sequence, motif and
    position; with ``motif_meta`` left-joined on ``motif_id`` (``motif_id`` first, ``tf_gene_name`` last).  No hits give
    an empty frame with these columns (the reference raises).
    """
    import pandas as pd

    if motifs is None:
        assert (
            matrices is None
        ), "Both a list of matrices and a corresponding list of motif IDs should be provided — or none to use the built-in ones, unless a scanner is provided."

    if motif_scanner is None:
        if matrices is None:
            parsed = parse_motif_matrices(files=None, background=background, jaspar_dir=jaspar_dir)
            motifs, matrices = parsed["motifs"], parsed["matrices"]
            if motif_meta is None:  # for the default scanner, the default metadata
                motif_meta = parse_motif_ids(jaspar_dir=jaspar_dir)
        else:
            assert (
                motifs is not None
            ), "A list of motif IDs should be provided if building a scanner from matrices"
        motif_scanner = prepare_motif_scanner(matrices=matrices, background=background, pvalue=pvalue,
                                              max_hits=max_hits, backend=backend)
    else:
        assert (
            motifs is not None
        ), "A list of motif IDs should be provided that corresponds to the matrices that the motif scanner was built on."
    if len(motifs) != motif_scanner.n_motifs:
        raise ValueError("one motif ID per matrix of the scanner")

    be = motif_scanner.backend
    encoded = _is_encoded(sequences)
    if not encoded:
        sequences = [sequences] if isinstance(sequences, str) else list(sequences)
    seq, mot, pos, score = (be.to_host(t) for t in scan_sequences_device(sequences, motif_scanner))
    names = seq.astype(np.int64) if encoded else np.asarray(sequences, dtype=object)[seq]
    matches = pd.DataFrame({"sequence": names, "motif_id": np.asarray(list(motifs), dtype=object)[mot],
                            "position": pos.astype(np.int64), "score": score}, columns=COLUMNS)
    if motif_meta is not None:
        matches = matches.set_index("motif_id").join(motif_meta, how="left").reset_index()
    return matches


# ---------------------------------------------------------------------------------------------------------------------
# sequences of the peaks from a FASTA file (host)
# ---------------------------------------------------------------------------------------------------------------------
def _read_fasta(path, wanted):
    """{record name: sequence} of the records of ``wanted`` (the name is the header up to the first blank)."""
    with open(path, "rb") as f:
        zipped = f.read(2) == b"\x1f\x8b"
    out, name, parts = {}, None, []
    with (gzip.open(path, "rt") if zipped else open(path, "rt")) as f:
        for line in f:
            if line.startswith(">"):
                if name is not None:
                    out[name] = "".join(parts)
                head = line[1:].split()
                name = head[0] if head and head[0] in wanted else None
                parts = []
            elif name is not None:
                parts.append(line.strip())
    if name is not None:
        out[name] = "".join(parts)
    return out


def get_sequences(data, bed: Optional[str] = None, fasta_file: Optional[str] = None, bed_file: Optional[str] = None):
    """
    The sequences of BED intervals (default: every feature, named ``chrX:NNN-NNN``) from a plain or gzip FASTA file,
    in the order of the intervals, with ``bedtools getfasta`` semantics: start 0-based, end exclusive.  The genome is
    ``fasta_file`` (recorded in ``.uns['files']['genome']``) or the one recorded there before.
    """
    adata = modality(data, "atac")

    if "files" not in adata.uns or "genome" not in adata.uns["files"]:
        if fasta_file is None:
            raise FileNotFoundError("Genome file has to be provided with `fasta_file` or recorded in "
                                    ".uns['files']['genome'].")
        if not os.path.exists(fasta_file):
            raise FileNotFoundError(f"File {fasta_file} does not exist")
        if "files" not in adata.uns:
            adata.uns["files"] = dict()
        adata.uns["files"]["genome"] = fasta_file
    else:
        fasta_file = adata.uns["files"]["genome"]

    if bed_file is not None:
        assert bed is None
        with open(bed_file) as f:
            bed = f.read()
    elif bed is None:
        bed = "\n".join(i.replace(":", "-", 1).replace("-", "\t", 2) for i in adata.var.index.values)

    intervals = []
    for line in bed.splitlines():
        line = line.strip()
        if not line or line.startswith(("#", "track", "browser")):
            continue
        tok = line.split("\t") if "\t" in line else line.split()
        if len(tok) < 3:
            raise ValueError(f"not a BED line: {line!r}")
        intervals.append((tok[0], int(tok[1]), int(tok[2])))
    records = _read_fasta(fasta_file, {c for c, _, _ in intervals})
    sequences = []
    for chrom, start, end in intervals:
        if chrom not in records:
            raise ValueError(f"{chrom}: no such record in {fasta_file}")
        if not 0 <= start <= end <= len(records[chrom]):
            raise ValueError(f"{chrom}:{start}-{end} leaves the record ({len(records[chrom])} bases)")
        sequences.append(records[chrom][start:end])
    return sequences
