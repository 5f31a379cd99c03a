"""Device-side operator set used by the tfidf / lsi / mofa host code.

``HipBackend`` forwards every operator to a hand-written gfx950 kernel through the C-ABI
(``_ffi``).  Device memory, streams and collectives are PyTorch-ROCm plumbing: tensors are
only containers whose ``data_ptr()`` is handed to the kernels.  There is no CPU
implementation in this package - constructing ``HipBackend`` without a GPU raises.
(The multi-process *host logic* is exercised on CPU by tests that inject their own
operator set; see tests/cpu_backend.py.)  Which operators there are, and which of them a set may leave out, is
declared once in ``_operators.OperatorSet``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple, Union

import contextlib
import ctypes
import os

import numpy as np
import torch

from . import _ffi
from ._ffi import F32, F64, check
from ._operators import OperatorSet


@dataclass(slots=True)
class CsrPlans:
    """What the backend derives from the INDEX ARRAYS of a device CSR alone, keyed once by the arrays it describes.
    Every CSR that shares those arrays (``with_values``) shares this object; a CSR with other arrays (compacted zeros,
    a transposition) has none of it."""

    key: tuple                                # key_of() of the arrays described
    slab_ptr: Optional[torch.Tensor] = None   # include/muon_amd.h mu_csr_slab_ptr
    xplan: Optional[dict] = None              # where the rows go in the row stream of X (HipBackend._make_xplan)
    # the transposition's count phase and the layout of X^T's stream (_make_tplan); its "tperm" entry, once a fill has
    # asked for it (_tperm_of): the slot table of the table-driven fill, or False = tried, no memory
    tplan: Optional[dict] = None
    wplan: Optional[tuple] = None             # (the warm start's slice plan, (n_s, max_ranges))

    @staticmethod
    def key_of(X: "DeviceCSR") -> tuple:
        n, d = X.shape
        return (X.indptr.data_ptr(), X.indices.data_ptr(), n, d, X.nnz)

    @staticmethod
    def of(X: "DeviceCSR") -> Optional["CsrPlans"]:
        """X's plans if they describe X's index arrays as they are (the one validity rule)."""
        plans = X.plans
        return plans if plans is not None and plans.key == CsrPlans.key_of(X) else None


@dataclass(slots=True)
class DeviceCSR:
    """CSR resident in HBM: indptr int64[n+1], indices int32[nnz], values f32|f64[nnz]."""

    indptr: torch.Tensor
    indices: torch.Tensor
    values: torch.Tensor
    shape: Tuple[int, int]
    plans: Optional[CsrPlans] = None
    # (row stream of this CSR, row_dst, values.data_ptr()) as the TF-IDF scale sweep wrote it: apart from `plans`
    # because it mirrors the values too
    xstream: Optional[tuple] = None
    canonical_as_given: bool = False  # _core.io.canonicalize: the arrays were canonical as they came

    @property
    def nnz(self) -> int:
        return int(self.indices.numel())

    @property
    def dtype(self):
        return self.values.dtype

    def with_values(self, values: torch.Tensor) -> "DeviceCSR":
        # (the plans describe the index arrays, which the new object shares: by reference, so that a plan made through
        #  either object serves both)
        return DeviceCSR(self.indptr, self.indices, values, self.shape, plans=self.plans)


@dataclass
class DeviceStream:
    """Row stream of a CSR (include/muon_amd.h): the (column, value) pairs, 8 bytes each, row after
    row in the launch order of the SpMM - position p holds row perm[p] (-1 = none; None = identity)
    at ent[sptr[p] : sptr[p+1]], no padding; k = the row-sets-per-wave the layout was dealt for.
    SpMM-only."""

    sptr: torch.Tensor
    ent: torch.Tensor
    shape: Tuple[int, int]
    nnz: int
    perm: Optional[torch.Tensor] = None
    k: int = 0
    # fourth-generation transposition only: the count pass' prefix table (uint32 [(blocks + 1), rows of this stream]: entries
    # of a row in the source's row blocks before g) and the rows per block - what a ranged product on this stream reads
    t4: Optional[dict] = None
    # ... and the device int32[1] copy of the fill's error word, queued behind the fill (HipBackend.raise_tpack4)
    t4_err: Optional[torch.Tensor] = None

    @property
    def n_pos(self) -> int:
        return int(self.sptr.numel()) - 1


@dataclass
class DeviceEll:
    """Sliced-ELL operand of the narrow-block SpMM (csrc/spmm_ell.hip, include/muon_amd.h): rows in launch order
    (``perm``: position -> row, -1 none), groups of 16 positions (one wave each), columns in slabs of 1024;
    ``hdr[group, slab]`` = the windows (4 steps of 16 entries; 384 bytes: 64 f32 values | 64 u16 offsets) of the
    group in that slab;
    ``wave_base[group]`` = the group's first window in ``ent``.  SpMM-only, B = 16."""

    hdr: torch.Tensor
    wave_base: torch.Tensor
    ent: torch.Tensor
    perm: torch.Tensor
    shape: Tuple[int, int]
    nnz: int
    slots: int = 0
    waves: int = 15  # row-owning waves per workgroup of the launch (mu_spmm_ell16_waves; not part of the layout)
    slab_cols: int = 1024  # 1024: against f32 blocks (64-byte Q rows); 512: against f64 blocks (128-byte Q rows)


@dataclass
class SplitOperand:
    """An f64-valued matrix as two operands of one layout (row streams or sliced ELL) with f32 stored values:
    v = hi + lo with hi = fl32(v), lo = fl32(v - hi) (exact to 2^-48); ``lo`` is None when every value is exact in f32
    (counts, f32 input).  SpMM-only, against f64 dense blocks."""

    hi: Union[DeviceStream, DeviceEll]
    lo: Union[DeviceStream, DeviceEll, None]

    @property
    def shape(self):
        return self.hi.shape

    @property
    def nnz(self) -> int:
        return self.hi.nnz


_NULL_CTX = contextlib.nullcontext()


def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.float64:
        return F64
    raise TypeError(f"unsupported value dtype {t.dtype}")


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _n_slab_ptr(n: int, d: int) -> int:
    return n * (-(-d // 8192) + 1)


def _sum_parts(part: torch.Tensor) -> torch.Tensor:
    """The sum of the partial products part[0], part[1], ... in that order (fixed order: deterministic)."""
    return part[0] if part.shape[0] == 1 else part.sum(dim=0)


def _split_hi(values: torch.Tensor):
    """(hi, rest) of f64 values: hi = fl32(v) and what it leaves, rest = v - hi (f64)."""
    hi = values.to(torch.float32)
    return hi, values - hi.to(torch.float64)


def _split_lo(rest: torch.Tensor) -> Optional[torch.Tensor]:
    """lo = fl32(rest) of ``_split_hi``, or None when every value was exact in f32.  Synchronises (it reads whether some
    rest is not zero): a caller with work to queue on hi alone queues that first."""
    return rest.to(torch.float32) if bool((rest != 0).any().item()) else None


def _split_build(X: DeviceCSR, build) -> Tuple[SplitOperand, ...]:
    """``build`` (CSR with f32 values -> tuple of operands) on the hi part of an f64-valued CSR and, when some value is
    not exact in f32, on its lo part: one SplitOperand per operand.  The work on hi is queued before ``_split_lo``
    synchronises."""
    assert X.values.dtype == torch.float64
    hi, rest = _split_hi(X.values)
    b_hi = build(X.with_values(hi))
    lo = _split_lo(rest)
    del rest
    b_lo = build(X.with_values(lo)) if lo is not None else (None,) * len(b_hi)
    return tuple(SplitOperand(a, b) for a, b in zip(b_hi, b_lo))


def _mofa_pad_width(K: int) -> int:
    """Columns of a zero-padded moment block of the poisson passes (include/muon_amd.h): 4 / 8 / 16 / 32, and 16 for
    9 <= K <= 12 too - 64-byte rows let the stored-entry pass read a row in one cache-line look-up (r06)."""
    return 16 if 8 < K <= 16 else next(k for k in (4, 8, 32) if k >= K)


def _mofa_pad(E: torch.Tensor, slot: str, K: int, ld: int, pads: Optional[dict]) -> torch.Tensor:
    """E [rows, K] with its rows padded with zeros to ``ld`` columns (E itself where it is that already).
    ``pads`` (a dict the caller owns, e.g. the engine of a fit): a padded buffer per (role, shape) whose columns
    K .. ld - 1 are zeroed once - a pass copies the K columns in, one kernel instead of a fill and a copy.
    Calls are ordered on one stream and a pass has consumed its operands when the next one overwrites them;
    the buffers live as long as the caller (a captured iteration keeps pointing at them)."""
    if K == ld and E.is_contiguous():
        return E
    key = (slot, int(E.shape[0]), ld, K, E.dtype)
    P = pads.get(key) if pads is not None else None
    if P is None:
        P = torch.zeros((E.shape[0], ld), dtype=E.dtype, device=E.device)
        if pads is not None:
            pads[key] = P
    P[:, :K].copy_(E)
    return P


def pick_block(width: int) -> int:
    for b in (16, 32, 64):
        if width <= b:
            return b
    raise NotImplementedError(
        f"block width {width} > 64 is not supported yet (n_comps + oversample must be <= 64)"
    )


SLAB_NARROW, SLAB_WIDE = 256, 320


def spmm_slab_cols(lib, B: int, K: int, dtype, force: int = 0, mode: int = 0, ranged: bool = False) -> int:
    """Q slab width of a row-stream product (csrc/spmm_win.hip): 256 columns, or 320 where the library has such an
    instance - f32 blocks of 64 columns on a layout of K >= 6 row-sets per wave (mu_spmm_stream_slab_ok); the products
    are bit-identical.  ``K`` is the K the launch will run with, ``force`` the tune key spmm_slab: 0 decide, 256 / 320
    that width where an instance exists (a forced 320 without one falls back to 256, it is never an error).
    ``mode`` is the tune key spmm_mode: the timing ablations are 256-column instances, except the cycle accounting
    (mode 64) at K = 8, which exists at both widths.
    The rule: 320 wherever it exists.  Measured (profiles/r08_spmm_slab_step_ab.md): the plain products at
    10^6 x 200 000 (X Q at K = 6, X^T Y at K = 7), 125 000 x 200 000, 600 000 x 200 000 at density 0.05 and on the
    unstructured generator - 320 is faster on every one; the ``ranged`` products of the warm start at the 10^6 x 200 000
    shapes (K = 8 and K = 7) - 320 does not lose there (3-4 % less on average, inside the spread of six launches).
    No shape was found where 320 is slower, so there is no density gate."""
    if force not in (0, SLAB_NARROW, SLAB_WIDE):
        raise ValueError(f"spmm_slab must be 0, {SLAB_NARROW} or {SLAB_WIDE}, not {force}")
    if dtype != torch.float32 or force == SLAB_NARROW:
        return SLAB_NARROW
    if mode != 0 and not (mode == 64 and K == 8 and not ranged):
        return SLAB_NARROW
    return SLAB_WIDE if lib.mu_spmm_stream_slab_ok(int(B), int(K), SLAB_WIDE) == 1 else SLAB_NARROW


def ell16_layout(X: DeviceCSR, waves: int = 15, slab_cols: int = 1024, slab_ptr_fn=None, fill_fn=None) -> "DeviceEll":
    """The sliced-ELL layout of csrc/spmm_ell.hip (built once per fit).  See DeviceEll / include/muon_amd.h for the
    format.  ``slab_cols`` = 1024 for f32 blocks, 512 for f64 blocks (a slab is 64 KiB of Q rows).  As tensor
    operations on X's device - the specification, and what runs without the library - or, with ``slab_ptr_fn`` and
    ``fill_fn`` (HipBackend.slab_ptr_width / ._ell16_fill), per (row, slab) only: the windows themselves are written by
    mu_ell16_fill (r04's dozen tensor passes over every entry took 30 ms per operand at 3.1e8 entries)."""
    assert slab_cols in (1024, 512) and X.values.dtype == torch.float32
    n, d = X.shape
    dev = X.indices.device
    S = -(-d // slab_cols)
    shift = 10 if slab_cols == 1024 else 9
    row_shift = 6 if slab_cols == 1024 else 7
    lens = X.indptr[1:] - X.indptr[:-1]
    order = torch.argsort(lens, descending=True, stable=True)       # position -> row: alike rows share a group
    n_groups = -(-n // 16)
    n_pos = n_groups * 16
    perm = torch.full((n_pos,), -1, dtype=torch.int32, device=dev)
    perm[:n] = order.to(torch.int32)
    inv = torch.empty((n,), dtype=torch.int64, device=dev)
    inv[order] = torch.arange(n, device=dev)
    sp = None
    if slab_ptr_fn is not None:
        # entries per (row, slab) off the slab pointers (binary searches: mu_csr_slab_ptr_width) - r04 histogrammed
        # every entry (torch.bincount: 20 ms of the 80 ms a fit's set-up took at 3.1e8 entries)
        sp = slab_ptr_fn(X, slab_cols).view(n, S + 1)
        cnt = torch.zeros((n_pos, S), dtype=torch.int64, device=dev)
        cnt[inv] = sp[:, 1:] - sp[:, :-1]
    else:
        rows = torch.repeat_interleave(torch.arange(n, device=dev), lens)
        pos = inv[rows]
        sl = (X.indices >> shift).to(torch.int64)
        cnt = torch.bincount(pos * S + sl, minlength=n_pos * S).view(n_pos, S)  # entries per (position, slab)
    nwin = (cnt.view(n_groups, 16, S).amax(dim=1) + 3) // 4                       # [group, slab]: the longest row
    flat = nwin.reshape(-1)
    wbase = torch.zeros(flat.numel() + 1, dtype=torch.int64, device=dev)
    torch.cumsum(flat, 0, out=wbase[1:])
    total = int(wbase[-1].item())
    win_base = wbase[:-1].view(n_groups, S)
    hdr = nwin.to(torch.int32).contiguous()
    wave_base = win_base[:, 0].contiguous()
    if sp is not None and fill_fn is not None:
        ent = torch.empty((total + 8, 384), dtype=torch.uint8, device=dev)        # (+ 8: the ring reads ahead)
        ent[total:].zero_()
        fill_fn(X, slab_cols, sp, perm, hdr, win_base.contiguous(), ent)
        return DeviceEll(hdr, wave_base, ent, perm, (n, d), X.nnz, total * 64, int(waves), int(slab_cols))
    if sp is not None:
        rows = torch.repeat_interleave(torch.arange(n, device=dev), lens)
        pos = inv[rows]
        sl = (X.indices >> shift).to(torch.int64)
    # rank of an entry inside its (row, slab): the rows are sorted by column, so slabs follow each other
    start = torch.cumsum(cnt, dim=1) - cnt                                        # [position, slab] exclusive
    e = torch.arange(X.nnz, device=dev)
    rank = e - X.indptr[:-1][rows] - start[pos, sl]
    dest = (win_base[pos // 16, sl] + rank // 4) * 64 + 4 * (pos % 16) + rank % 4
    vals = torch.zeros(((total + 8) * 64,), dtype=torch.float32, device=dev)      # (+ 8: the ring reads ahead)
    offs = torch.zeros(((total + 8) * 64,), dtype=torch.int16, device=dev)
    vals[dest] = X.values
    off = (X.indices.to(torch.int32) & (slab_cols - 1)) << row_shift              # u16 bit pattern in an int16
    offs[dest] = torch.where(off >= 32768, off - 65536, off).to(torch.int16)
    ent = torch.cat([vals.view(torch.uint8).view(-1, 256), offs.view(torch.uint8).view(-1, 128)], dim=1).contiguous()
    del vals, offs
    return DeviceEll(hdr, wave_base, ent, perm, (n, d), X.nnz, total * 64, int(waves), int(slab_cols))


class HipBackend(OperatorSet):
    name = "hip"

    def __init__(self, device: Optional[int] = None):
        _ffi.require_gpu()
        self.lib = _ffi.lib()
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", int(device))
        self._tri_index = {}  # (K, device) -> positions of the K x K entries in the packed upper triangle

    # -- plumbing -------------------------------------------------------------
    def _stream(self):
        """Raw handle of torch's current stream on this device (a few hundred of these per small lsi()
        call: the raw-handle query is ~10x cheaper than building a torch.cuda.Stream object)."""
        raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)
        if raw is not None:
            return raw(self.device.index)
        return torch.cuda.current_stream(self.device).cuda_stream

    def _dev_ctx(self):
        """Context that makes this backend's device current - a no-op object when it already is (the
        usual case: one process per GPU), instead of two device switches per kernel launch."""
        if torch.cuda.current_device() == self.device.index:
            return _NULL_CTX
        return torch.cuda.device(self.device)

    def _launch(self, fn, *args) -> None:
        """Call the stream-taking library entry ``fn`` (as in ``self.lib.mu_gram_f32``): a tensor among ``args`` goes as
        its ``data_ptr()``, everything else (None, ints, floats, bytes, ctypes arrays, ``byref``) as it is; the raw handle
        of the stream that is current NOW is appended, this backend's device is current around the call, and a status
        other than 0 raises.  The one place that decides which stream and which device a launch goes to."""
        Tensor = torch.Tensor
        with self._dev_ctx():
            check(fn(*[a.data_ptr() if isinstance(a, Tensor) else a for a in args], self._stream()))

    def _work(self, size, floor: int = 0):
        """(work, wb): a uint8 work buffer for the ``size`` bytes a ``*_worksize`` query answered, and that size as the
        int the library is handed.  ``floor``: the fewest bytes allocated (a kernel that is handed a buffer of no size
        still wants an address)."""
        wb = int(size)
        return self.empty((max(wb, floor),), torch.uint8), wb

    def empty(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.device)

    def zeros(self, shape, dtype):
        return torch.zeros(shape, dtype=dtype, device=self.device)

    def to_device(self, arr, dtype=None) -> torch.Tensor:
        """Host array -> device tensor (optionally converted to ``dtype`` on the way).  Big arrays -
        the CSR of a whole experiment is tens of GB - go through pinned staging buffers filled by a
        few host threads while the previous chunk is on the bus (scripts/probes/upload_probe.py);
        a pageable ``.to(device)`` stages the same bytes on one thread."""
        a = np.asarray(arr)
        want = np.dtype(dtype) if dtype is not None else a.dtype
        if a.nbytes >= self._UPLOAD_PIPELINE_MIN and a.ndim == 1:
            return self._upload_pipelined(a, want)
        a = np.ascontiguousarray(a, dtype=want)
        if 0 < a.nbytes <= self._UPLOAD_SMALL_MAX:
            return self._upload_small(a)
        return torch.as_tensor(a).to(self.device, non_blocking=False)

    _UPLOAD_SMALL_MAX = 1 << 20

    def _upload_small(self, a: np.ndarray) -> torch.Tensor:
        """Coefficient blocks and the like (the LSI loop uploads a few per expansion): through a ring of pinned
        buffers with a non-blocking copy.  A pageable ``.to(device)`` blocks the host until the stream has reached
        the copy - 0.5 ms each at 125k x 200k, eight per step, with the launches queued behind them starting late (r04)."""
        ring = self.__dict__.setdefault("_small_ring", {"bufs": [], "i": 0})
        if not ring["bufs"]:
            ring["bufs"] = [[torch.empty((self._UPLOAD_SMALL_MAX,), dtype=torch.uint8, pin_memory=True), None]
                            for _ in range(16)]
        slot = ring["bufs"][ring["i"] % len(ring["bufs"])]
        ring["i"] += 1
        if slot[1] is not None:
            slot[1].synchronize()  # the copy that used this buffer 16 uploads ago
        flat = slot[0][:a.nbytes]
        flat.numpy()[:] = a.reshape(-1).view(np.uint8)
        tdt = torch.from_numpy(np.empty(0, dtype=a.dtype)).dtype
        out = torch.empty((a.size,), dtype=tdt, device=self.device)
        out.view(torch.uint8).copy_(flat, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        slot[1] = ev
        return out.reshape(a.shape)

    _UPLOAD_PIPELINE_MIN = 256 << 20
    _UPLOAD_CHUNK = 64 << 20      # bytes per staging buffer
    _UPLOAD_THREADS = 4

    def _upload_pipelined(self, a: np.ndarray, want: np.dtype) -> torch.Tensor:
        from concurrent.futures import ThreadPoolExecutor

        tdt = torch.from_numpy(np.empty(0, dtype=want)).dtype
        n = a.shape[0]
        out = torch.empty((n,), dtype=tdt, device=self.device)
        per = max(1, self._UPLOAD_CHUNK // want.itemsize)
        st = self.__dict__.get("_upload_state")
        if st is None:
            # staging is raw bytes: int32 / float32 / int64 uploads of one call sequence share the three
            # pinned buffers, the copy stream and the thread pool (they were keyed by dtype
            # and rebuilt - 3 x 64 MiB of pinning - whenever the dtype changed)
            bufs = [torch.empty((self._UPLOAD_CHUNK,), dtype=torch.uint8).pin_memory() for _ in range(3)]
            st = self._upload_state = {"bufs": bufs, "stream": torch.cuda.Stream(self.device),
                                       "pool": ThreadPoolExecutor(self._UPLOAD_THREADS)}
        copy_stream, pool = st["stream"], st["pool"]
        bufs = [b[: per * want.itemsize].view(tdt) for b in st["bufs"]]
        nps = [b.numpy() for b in bufs]
        events = [None, None, None]
        T = self._UPLOAD_THREADS
        cur = torch.cuda.current_stream(self.device)
        # `out` comes from the caching allocator on the CURRENT stream: the block may still be in use
        # by kernels queued there; the copies run on a private stream, so order them behind those
        copy_stream.wait_stream(cur)

        def fill(dst, src):
            np.copyto(dst, src, casting="unsafe")  # (memcpy or a converting loop; releases the GIL)

        for i, lo in enumerate(range(0, n, per)):
            hi = min(n, lo + per)
            b = i % 3
            if events[b] is not None:
                events[b].synchronize()  # the bus is done with this staging buffer
            m = hi - lo
            cuts = [m * t // T for t in range(T + 1)]
            list(pool.map(lambda t: fill(nps[b][cuts[t]:cuts[t + 1]], a[lo + cuts[t]:lo + cuts[t + 1]]), range(T)))
            with torch.cuda.stream(copy_stream):
                out[lo:hi].copy_(bufs[b][:m], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(copy_stream)
            events[b] = ev
        cur.wait_stream(copy_stream)
        out.record_stream(copy_stream)
        copy_stream.synchronize()  # the staging buffers are reused by the next call
        return out

    def to_host(self, t: torch.Tensor, out: Optional[np.ndarray] = None) -> np.ndarray:
        """Device tensor -> host array.  Big 1-d tensors (the TF-IDF values of a whole experiment are GBs) come down
        through the pinned staging buffers of the upload path, chunk by chunk, a few host threads copying one chunk
        out while the next is on the bus: `.cpu()` on pageable memory ran at 11 GB/s in the API benchmark (r04,
        `bench.py --workload c3_api`)."""
        t = t.detach()
        if out is not None:
            # into the caller's array (pages that exist already: a fresh 6 GB array costs 225 ms of first-touch faults
            # on top of its bytes - scripts/probes/host_alloc_probe.py)
            want = torch.empty((0,), dtype=t.dtype).numpy().dtype
            if out.dtype != want or out.shape != tuple(t.shape) or not out.flags.c_contiguous or not out.flags.writeable:
                raise TypeError("to_host(out=): a writeable contiguous array of the tensor's shape and type")
        if t.ndim == 1 and t.is_cuda and t.is_contiguous() and t.numel() * t.element_size() >= self._UPLOAD_PIPELINE_MIN:
            return self._download_pipelined(t, out)
        if out is not None:
            np.copyto(out, t.cpu().numpy())
            return out
        return t.cpu().numpy()

    def _download_pipelined(self, t: torch.Tensor, out: Optional[np.ndarray] = None) -> np.ndarray:
        from concurrent.futures import ThreadPoolExecutor

        n = t.numel()
        if out is None:
            out = np.empty((n,), dtype=torch.empty((0,), dtype=t.dtype).numpy().dtype)
        item = t.element_size()
        per = max(1, self._UPLOAD_CHUNK // item)
        st = self.__dict__.get("_upload_state")
        if st is None:
            bufs = [torch.empty((self._UPLOAD_CHUNK,), dtype=torch.uint8).pin_memory() for _ in range(3)]
            st = self._upload_state = {"bufs": bufs, "stream": torch.cuda.Stream(self.device),
                                       "pool": ThreadPoolExecutor(self._UPLOAD_THREADS)}
        copy_stream, pool = st["stream"], st["pool"]
        bufs = [b[: per * item].view(t.dtype) for b in st["bufs"]]
        nps = [b.numpy() for b in bufs]
        T = self._UPLOAD_THREADS
        cur = torch.cuda.current_stream(self.device)
        copy_stream.wait_stream(cur)  # the tensor's producers are queued on the current stream
        chunks = [(lo, min(n, lo + per)) for lo in range(0, n, per)]
        events = [None] * len(chunks)

        def start(i):
            lo, hi = chunks[i]
            with torch.cuda.stream(copy_stream):
                bufs[i % 3][: hi - lo].copy_(t[lo:hi], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(copy_stream)
            events[i] = ev

        def drain(i):
            lo, hi = chunks[i]
            events[i].synchronize()
            m = hi - lo
            cuts = [m * k // T for k in range(T + 1)]
            list(pool.map(lambda k: np.copyto(out[lo + cuts[k]:lo + cuts[k + 1]], nps[i % 3][cuts[k]:cuts[k + 1]]), range(T)))

        for i in range(min(2, len(chunks))):  # two chunks on the bus / being copied out, a third buffer idle-safe
            start(i)
        for i in range(len(chunks)):
            drain(i)
            if i + 2 < len(chunks):
                start(i + 2)  # reuses the buffer of chunk i - 1, drained in the previous turn
        t.record_stream(copy_stream)
        return out

    def upload_csr(self, indptr, indices, values, shape, values_dtype=None, slab_ptr: bool = True) -> DeviceCSR:
        """Host CSR -> HBM.  Index arrays become int64 / int32 and the values ``values_dtype`` on the
        way (scipy keeps int64 column indices beyond 2^31 stored entries; a separate ``astype`` of
        such an array is a single-threaded pass over tens of GB)."""
        X = DeviceCSR(
            self.to_device(indptr, np.int64),
            self.to_device(indices, np.int32),
            self.to_device(values, values_dtype),
            (int(shape[0]), int(shape[1])),
        )
        return self.with_slab_ptr(X) if slab_ptr else X

    def with_slab_ptr(self, X: DeviceCSR) -> DeviceCSR:
        """Attach the slab pointers of X's index arrays (include/muon_amd.h mu_csr_slab_ptr): searched once where the
        device CSR is made - inside the clock of whoever makes it (upload, ingest) - and read by every sweep of tfidf and
        by lsi's transposition afterwards.  Needs sorted rows (every producer here uploads canonical CSR)."""
        n, d = X.shape
        if n == 0 or d == 0 or X.nnz == 0 or self._slab_ptr_of(X) is not None:
            return X
        sp = self.empty((_n_slab_ptr(n, d),), torch.int64)
        self._launch(self.lib.mu_csr_slab_ptr, n, d, X.indptr, X.indices, sp)
        X.plans = CsrPlans(CsrPlans.key_of(X), slab_ptr=sp)
        return self.with_plans(X)

    def with_plans(self, X: DeviceCSR) -> DeviceCSR:
        """The rest of what lsi's operand building derives from the INDEX ARRAYS alone, made once where the device CSR is
        made (r05; the same rule as the slab pointers: whoever makes the CSR - upload, ingest - pays inside its own clock):
        `xplan` - where the rows go in the row stream of X (launch_layout of the row lengths, scanned; what the TF-IDF
        scale sweep needs to write that stream) - and `tplan` - the transposition's count phase (entries per (row block,
        column), their prefixes, the column totals) and the layout of X^T's stream.  Keyed by the arrays they describe;
        a result whose zeros were compacted has other arrays and none of this."""
        n, d = X.shape
        if n == 0 or d == 0 or X.nnz == 0:
            return X
        plans = CsrPlans.of(X)
        if plans is None:
            plans = X.plans = CsrPlans(CsrPlans.key_of(X))
        try:
            if plans.xplan is None:
                plans.xplan = self._make_xplan(X, None)
            if plans.tplan is None and self._use_tpack4(X):
                plans.tplan = self._make_tplan(X, None, True)
        except NotImplementedError:  # (_stream_sptr: a layout the stream SpMM does not take - X goes without the plan)
            pass
        return X

    def _make_xplan(self, X: DeviceCSR, K: Optional[int]) -> dict:
        """Where the rows of X go in its row stream: launch_layout of the row lengths, scanned."""
        perm, inv, K, sptr = self._dealt_sptr(X.indptr[1:] - X.indptr[:-1], K)
        return dict(perm=perm, inv=inv, K=K, sptr=sptr, row_dst=sptr[inv.long()].contiguous())

    def _dealt_sptr(self, lens: torch.Tensor, K: Optional[int]):
        """(perm, inv, K, sptr) of a row stream whose rows, ``lens`` entries long, are dealt by launch_layout: the
        lengths scattered to their positions, scanned."""
        perm, inv, K = self.launch_layout(lens, K)
        plens = torch.zeros((int(perm.numel()),), dtype=torch.int64, device=self.device)
        plens[inv.long()] = lens
        return perm, inv, K, self._stream_sptr(plens, K)

    def _make_tplan(self, X: DeviceCSR, K: Optional[int], sort_rows: bool) -> dict:
        """The count phase of the tile-staged transposition of X (csrc/tpack4.hip) and the layout of X^T's row stream."""
        n, d = X.shape
        col_nnz = self.empty((max(d, 1),), torch.int64)
        work, wb = self._work(self.lib.mu_tpack4_worksize(n, d, X.nnz))
        self._launch(self.lib.mu_tpack4_count, n, d, X.nnz, X.indptr, X.indices, col_nnz, work, wb, self._slab_ptr_of(X))
        lens = col_nnz[:d]
        if sort_rows and d > 0:
            perm, inv, K, sptr = self._dealt_sptr(lens, K)
        else:
            perm, inv, K = None, None, max(1, int(K or self.lib.mu_spmm_stream_k(d)))
            sptr = self._stream_sptr(lens, K)
        return dict(work=work, wb=wb, perm=perm, inv=inv, K=K, sptr=sptr)

    @staticmethod
    def _plan_of(X: DeviceCSR, name: str):
        """Field ``name`` of X's plans (None: not made, or the plans describe other arrays)."""
        plans = CsrPlans.of(X)
        return None if plans is None else getattr(plans, name)

    # -- TF-IDF (reference preproc.py:92-117) -----------------------------------------
    def row_col_sums(self, X: DeviceCSR, keep_work: bool = False):
        """(row sums, column sums), f64.  ``keep_work``: also the sweep's work buffer, whose head holds the slab pointers
        the sweep searched - what ``tfidf_scale(work=)`` of the SAME matrix then does not search again (None when X
        brought its own table: nothing was searched)."""
        n, d = X.shape
        rowsum = self.empty((n,), torch.float64)
        colsum = self.empty((d,), torch.float64)
        work, wb = self._work(self.lib.mu_csr_row_col_sums_worksize(n, d))
        sp = self._slab_ptr_of(X)
        self._launch(self.lib.mu_csr_row_col_sums_sp, _dt(X.values), n, d, X.indptr, X.indices, X.values, rowsum, colsum,
                     work, wb, sp)
        if keep_work:
            return rowsum, colsum, (work if sp is None else None)
        return rowsum, colsum

    def idf(self, colsum: torch.Tensor, n_obs: float, flags: int, dtype) -> torch.Tensor:
        d = colsum.numel()
        out = self.empty((d,), dtype)
        self._launch(self.lib.mu_tfidf_idf, _dt(out), d, float(n_obs), colsum, flags, out)
        return out

    def can_emit_stream(self, X: DeviceCSR) -> bool:
        """The TF-IDF scale sweep can write the row stream of its result (f32, a shape the stream SpMM takes)."""
        return X.values.dtype == torch.float32 and X.nnz > 0 and self.can_stream(X, 64)

    def stream_layout(self, X: DeviceCSR, K: Optional[int] = None):
        """Where the rows of X go in its row stream (launch_layout: needs the row LENGTHS only, so it can be made before
        the values exist) and an empty stream to fill: (DeviceStream, row_dst) with row_dst[r] = pair index of row r's
        first pair."""
        n, d = X.shape
        plan = (self._plan_of(X, "xplan") if K is None else None) or self._make_xplan(X, K)
        ent = self.empty((max(X.nnz, 1),), torch.int64)
        return DeviceStream(plan["sptr"], ent, (n, d), X.nnz, plan["perm"], plan["K"]), plan["row_dst"]

    @staticmethod
    def _xstream_of(X: DeviceCSR):
        """(row stream, row_dst) the TF-IDF scale sweep left with X, if they describe X's arrays as they are."""
        got = X.xstream
        if got is None or CsrPlans.of(X) is None or got[2] != X.values.data_ptr():
            return None
        return got[0], got[1]

    def tfidf_scale(self, X: DeviceCSR, rowsum, idf, scale: float, flags: int, out=None, emit=None, work=None,
                    gather: bool = False):
        """``emit`` = (DeviceStream, row_dst) from stream_layout: the sweep also writes the result's row stream.
        ``work``: what ``row_col_sums(X, keep_work=True)`` of the same X returned - the slab pointers at its head are
        read instead of searched again.  ``gather``: the per-lane gather kernel (comparison / tests)."""
        if out is None:
            out = torch.empty_like(X.values)
        zc = self.zeros((1,), torch.int64)
        n, d = X.shape
        sp = self._slab_ptr_of(X)
        if emit is None and (gather or sp is not None):
            if gather:
                self._launch(self.lib.mu_tfidf_scale, _dt(X.values), n, X.indptr, X.indices, X.values, rowsum, idf,
                             float(scale), flags, out, zc)
            else:
                self._launch(self.lib.mu_tfidf_scale_sweep_sp, _dt(X.values), n, d, X.indptr, X.indices, X.values, rowsum,
                             idf, float(scale), flags, out, zc, sp)
            return out, zc
        # the sweeps that search the slab pointers into the head of a work buffer, or find them there (`have`)
        have, wb = False, 0
        if sp is not None:
            work = None
        else:
            have, wb = work is not None, int(self.lib.mu_csr_row_col_sums_worksize(n, d))
            if not have:
                work = self.empty((wb,), torch.uint8)
            elif work.numel() != wb:
                raise ValueError("tfidf_scale(work=): not the work buffer of a sum sweep of this matrix")
        if emit is not None:
            assert X.values.dtype == torch.float32
            self._launch(self.lib.mu_tfidf_scale_sweep_stream, n, d, X.indptr, X.indices, X.values, rowsum, idf,
                         float(scale), flags, out, zc, work, wb, int(have), sp, emit[1], emit[0].ent)
        else:
            self._launch(self.lib.mu_tfidf_scale_sweep, _dt(X.values), n, d, X.indptr, X.indices, X.values, rowsum, idf,
                         float(scale), flags, out, zc, work, wb, int(have))
        return out, zc

    def slab_ptr_from_work(self, X: DeviceCSR, work: torch.Tensor) -> torch.Tensor:
        """The slab pointers of a table-less X after its scale sweep: a copy of the head of the sweep's work buffer,
        apart from the column partials that follow them.  They also serve the transposition of the same index arrays
        (transpose_stream cuts the same 8192-column slabs)."""
        return work[:8 * _n_slab_ptr(*X.shape)].view(torch.int64).clone()

    def compact_nonzero(self, X: DeviceCSR) -> DeviceCSR:
        n = X.shape[0]
        row_nnz = self.empty((n,), torch.int64)
        new_indptr = self.empty((n + 1,), torch.int64)
        self._launch(self.lib.mu_csr_count_nonzero, _dt(X.values), n, X.indptr, X.values, row_nnz)
        self._launch(self.lib.mu_exclusive_scan_i64, n, row_nnz, new_indptr)
        new_nnz = int(new_indptr[-1].item())
        new_indices = self.empty((new_nnz,), torch.int32)
        new_values = self.empty((new_nnz,), X.values.dtype)
        self._launch(self.lib.mu_csr_compact_nonzero, _dt(X.values), n, X.indptr, X.indices, X.values, new_indptr,
                     new_indices, new_values)
        return DeviceCSR(new_indptr, new_indices, new_values, X.shape)

    # -- QC metrics and filtering (reference _core/preproc.py:675-881) ----------------
    def csr_qc(self, X: DeviceCSR):
        """(row_nnz int64, rowsum f64, col_nnz int64, colsum f64) of X in one sweep (csrc/filter.hip): the counts are
        of the stored values that are not zero (NaN counts), the sums are ``row_col_sums``' bit for bit."""
        n, d = X.shape
        row_nnz, rowsum = self.empty((n,), torch.int64), self.empty((n,), torch.float64)
        col_nnz, colsum = self.empty((d,), torch.int64), self.empty((d,), torch.float64)
        work, wb = self._work(self.lib.mu_csr_qc_worksize(n, d))
        self._launch(self.lib.mu_csr_qc, _dt(X.values), n, d, X.indptr, X.indices, X.values, row_nnz, rowsum, col_nnz,
                     colsum, work, wb, self._slab_ptr_of(X))
        return row_nnz, rowsum, col_nnz, colsum

    def row_masked_sums(self, X: DeviceCSR, flags: torch.Tensor, M: int) -> torch.Tensor:
        """f64 [n, M]: per row of X the sum of the stored values whose column has bit q of ``flags`` (int32 [d], read as
        32 unsigned bits; 1 <= M <= 32) set, q < M; one read of the row serves every mask (csrc/qc.hip)."""
        n, d = X.shape
        if flags.dtype != torch.int32 or int(flags.numel()) != d or not 1 <= int(M) <= 32:
            raise TypeError("row_masked_sums: flags int32[n_cols of X], 1 <= M <= 32")
        out = self.empty((n, int(M)), torch.float64)
        self._launch(self.lib.mu_csr_row_masked_sums, _dt(X.values), n, d, int(X.values.numel()), X.indptr, X.indices,
                     X.values, flags.contiguous(), int(M), out)
        return out

    def row_top_sums(self, X: DeviceCSR, ns) -> torch.Tensor:
        """f64 [n, len(ns)]: per row of X the sum of its min(n, stored entries) largest stored values, for the strictly
        ascending ``ns`` (1 to 8 of them, each in 1 .. n_cols); rows of any length (csrc/qc.hip)."""
        n, d = X.shape
        ns = [int(v) for v in ns]
        out = self.empty((n, len(ns)), torch.float64)
        self._launch(self.lib.mu_csr_row_top_sums, _dt(X.values), n, d, int(X.values.numel()), X.indptr, X.values, len(ns),
                     (ctypes.c_int64 * max(len(ns), 1))(*ns), out)
        return out

    def csr_submatrix(self, X: DeviceCSR, rows: torch.Tensor, col_table: torch.Tensor, n_cols: int) -> DeviceCSR:
        """Rows ``rows`` (int64, ascending: new row -> old row) and the columns ``col_table`` keeps (int32[d]: old ->
        new column, -1 dropped; ``n_cols`` of them) of X: stored order inside the rows, explicit zeros kept, values bit
        for bit (csrc/filter.hip).  The result has index arrays of its own and so none of X's derived tables (they
        describe other arrays); a caller that knows the rows to be sorted asks ``with_slab_ptr`` for new ones."""
        n, d = X.shape
        k = int(rows.numel())
        if rows.dtype != torch.int64 or col_table.dtype != torch.int32 or int(col_table.numel()) != d:
            raise TypeError("csr_submatrix: rows int64, col_table int32[n_cols of X]")
        rows, col_table = rows.contiguous(), col_table.contiguous()
        row_nnz = self.empty((k,), torch.int64)
        new_indptr = self.zeros((k + 1,), torch.int64)
        self._launch(self.lib.mu_csr_submatrix_count, n, d, k, X.indptr, X.indices, rows, col_table, row_nnz)
        if k:
            self._launch(self.lib.mu_exclusive_scan_i64, k, row_nnz, new_indptr)
        new_nnz = int(new_indptr[-1].item())
        new_indices = self.empty((new_nnz,), torch.int32)
        new_values = self.empty((new_nnz,), X.values.dtype)
        self._launch(self.lib.mu_csr_submatrix_fill, _dt(X.values), n, d, k, X.indptr, X.indices, X.values, rows, col_table,
                     new_indptr, new_indices, new_values)
        return DeviceCSR(new_indptr, new_indices, new_values, (k, int(n_cols)))

    # -- fragment tools (reference _atac/tools.py:746-1201; csrc/fragments.hip) ------
    @staticmethod
    def _i32(*tensors):
        for t in tensors:
            if t is not None and (t.dtype != torch.int32 or not t.is_contiguous()):
                raise TypeError("fragment kernels take contiguous int32 columns")

    def frag_ranges(self, start, chrom_ptr, wchrom, wlo, whi, max_len: int):
        """(rng_lo, rng_len) int64 per window: the candidates start > lo - max_len && start < hi of the window's contig."""
        self._i32(start, wchrom, wlo, whi)
        if chrom_ptr.dtype != torch.int64:
            raise TypeError("frag_ranges: chrom_ptr int64")
        n_win = int(wchrom.numel())
        rng_lo, rng_len = self.empty((n_win,), torch.int64), self.empty((n_win,), torch.int64)
        self._launch(self.lib.mu_frag_ranges, n_win, int(chrom_ptr.numel()) - 1, wchrom, wlo, whi, chrom_ptr.contiguous(),
                     start, int(max_len), rng_lo, rng_len)
        return rng_lo, rng_len

    def _frag_chunks(self, rng_len):
        """(chunk_ptr int64[n_win + 1], n_chunks): the windows' candidates cut into work items of 256."""
        n_win = int(rng_len.numel())
        chunk = int(self.lib.mu_frag_chunk())
        per = torch.div(rng_len + (chunk - 1), chunk, rounding_mode="floor")
        chunk_ptr = self.zeros((n_win + 1,), torch.int64)
        if n_win:
            self._launch(self.lib.mu_exclusive_scan_i64, n_win, per, chunk_ptr)
        return chunk_ptr, int(chunk_ptr[-1].item())

    def frag_overlap(self, start, end, barcode, score, cell_of, n_obs: int, wlo, whi, rng_lo, rng_len, n_features: int):
        """(keys int64, vals int32) of the fragments that overlap their window and belong to a cell: key = cell *
        n_features + window, value = score (None: 1); window order, file order inside a window."""
        self._i32(start, end, barcode, score, cell_of, wlo, whi)
        n_win, nb = int(wlo.numel()), int(cell_of.numel())
        chunk_ptr, n_chunks = self._frag_chunks(rng_len)
        cnt = self.empty((n_chunks,), torch.int64)
        off = self.zeros((n_chunks + 1,), torch.int64)
        self._launch(self.lib.mu_frag_overlap_count, n_win, n_chunks, chunk_ptr, rng_lo, rng_len, wlo, whi, start, end,
                     barcode, cell_of, nb, int(n_obs), cnt)
        if n_chunks:
            self._launch(self.lib.mu_exclusive_scan_i64, n_chunks, cnt, off)
        total = int(off[-1].item())
        keys, vals = self.empty((total,), torch.int64), self.empty((total,), torch.int32)
        if total:
            self._launch(self.lib.mu_frag_overlap_emit, n_win, n_chunks, chunk_ptr, rng_lo, rng_len, wlo, whi, start, end,
                         barcode, score, cell_of, nb, int(n_obs), int(n_features), off, keys, vals)
        return keys, vals

    def frag_pileup(self, start, end, barcode, score, cell_of, n_obs: int, wlo, whi, rng_lo, rng_len, width: int):
        """Difference array int32[n_obs, width + 1] of the windows' pileup: +score at a fragment's first column, -score
        behind its last one (columns count from ``wlo``)."""
        self._i32(start, end, barcode, score, cell_of, wlo, whi)
        n_win, nb = int(wlo.numel()), int(cell_of.numel())
        diff = self.zeros((int(n_obs), int(width) + 1), torch.int32)
        chunk_ptr, n_chunks = self._frag_chunks(rng_len)
        self._launch(self.lib.mu_frag_pileup, n_win, n_chunks, chunk_ptr, rng_lo, rng_len, wlo, whi, start, end, barcode,
                     score, cell_of, nb, int(n_obs), int(width), diff)
        return diff

    def frag_pileup_scan(self, diff, flank_size: int, center_dist: int):
        """Scan the rows of ``diff`` (int32[n, W + 1]) into the pileup IN PLACE; returns int64[n, 2]: the sums of the
        flank columns and of the centre columns."""
        self._i32(diff)
        n, w1 = diff.shape
        sums = self.zeros((n, 2), torch.int64)
        self._launch(self.lib.mu_frag_pileup_scan, n, w1 - 1, int(flank_size), int(center_dist), diff, sums)
        return sums

    def frag_length_classes(self, start, end, barcode, cell_of, n_obs: int, n_take: int, free_bound: int,
                            mono_bound: int):
        """int32[n_obs, 2]: fragments among the first ``n_take`` shorter than ``free_bound`` / the others shorter than
        ``mono_bound``, per cell."""
        self._i32(start, end, barcode, cell_of)
        n_take = max(0, min(int(n_take), int(start.numel())))
        classes = self.zeros((int(n_obs), 2), torch.int32)
        self._launch(self.lib.mu_frag_length_classes, n_take, start, end, barcode, cell_of, int(cell_of.numel()), int(n_obs),
                     int(free_bound), int(mono_bound), classes)
        return classes

    def binarize_values(self, values: torch.Tensor) -> None:
        self._launch(self.lib.mu_binarize_values, _dt(values), values.numel(), values)

    # -- LSI building blocks (reference tools.py:53 -> scipy svds) ---------------------
    @staticmethod
    def _slab_ptr_of(X: DeviceCSR):
        """The slab pointers that came with X (``with_slab_ptr``, ``tfidf_device``), if they describe X's index arrays."""
        sp = HipBackend._plan_of(X, "slab_ptr")
        return sp if sp is not None and sp.numel() == _n_slab_ptr(*X.shape) else None

    def transpose(self, X: DeviceCSR) -> DeviceCSR:
        n, d = X.shape
        nnz = X.nnz
        t_indptr = self.empty((d + 1,), torch.int64)
        t_indices = self.empty((nnz,), torch.int32)
        t_values = torch.empty_like(X.values)
        work, wb = self._work(self.lib.mu_csr_transpose_worksize(n, d, nnz))
        self._launch(self.lib.mu_csr_transpose, _dt(X.values), n, d, nnz, X.indptr, X.indices, X.values, t_indptr, t_indices,
                     t_values, work, wb)
        return DeviceCSR(t_indptr, t_indices, t_values, (d, n))

    def transpose_csr(self, X: DeviceCSR) -> DeviceCSR:
        """CSR of X^T straight from the CSR of X (f32; stable: cells ascending inside every row =>
        canonical rows), through the tile-staged transposition of csrc/tpack4.hip."""
        n, d = X.shape
        assert X.values.dtype == torch.float32
        col_nnz = self.empty((max(d, 1),), torch.int64)
        t_indptr = self.zeros((d + 1,), torch.int64)
        t_indices = self.empty((max(X.nnz, 1),), torch.int32)[:X.nnz]
        t_values = self.empty((max(X.nnz, 1),), torch.float32)[:X.nnz]
        if self._use_tpack4(X):
            work, wb = self._work(self.lib.mu_tpack4_worksize(n, d, X.nnz))
            self._launch(self.lib.mu_tpack4_count, n, d, X.nnz, X.indptr, X.indices, col_nnz, work, wb,
                         self._slab_ptr_of(X))
            self._launch(self.lib.mu_exclusive_scan_i64, d, col_nnz, t_indptr)
            self._launch(self.lib.mu_tpack4_fill_csr, n, d, X.nnz, X.indptr, X.indices, X.values, None, None, t_indptr,
                         t_indices, t_values, work, wb)
            self.raise_tpack4(self._note_tpack4(work, n, d, X.nnz).item())  # (set-up / ingest paths: a synchronisation is affordable)
            return DeviceCSR(t_indptr, t_indices, t_values, (d, n))
        # (2^31 rows, a row block of 2^29 entries: the general stable transposition, csrc/transpose.hip)
        return self.transpose(X)

    def can_stream(self, X: DeviceCSR, B: int) -> bool:
        """The row-stream SpMM exists for f32 values and B in (16, 32, 64)."""
        return X.values.dtype == torch.float32 and B in (16, 32, 64) and X.shape[0] > 0 and X.shape[1] > 0

    def _stream_sptr(self, lens_by_pos: torch.Tensor, K: int):
        n_pos = int(lens_by_pos.numel())
        sptr = self.zeros((n_pos + 1,), torch.int64)
        self._launch(self.lib.mu_exclusive_scan_i64, n_pos, lens_by_pos, sptr)
        # cursors are 32-bit byte offsets from the first pair of the workgroup's 64 K rows
        per_wg = 64 * K
        span = sptr[per_wg::per_wg] - sptr[:-per_wg:per_wg] if n_pos > per_wg else sptr[-1:] - sptr[:1]
        if span.numel() and int(span.max().item()) * 8 >= (1 << 32) - 256:
            raise NotImplementedError("row stream: the rows of one workgroup span 4 GiB or more")
        return sptr

    def stream(self, X: DeviceCSR, sort_rows: bool = True, K: Optional[int] = None) -> DeviceStream:
        """Row stream of X for the SpMM of the iteration (a streaming copy, once per lsi call)."""
        n, d = X.shape
        assert X.values.dtype == torch.float32
        want_k = K
        perm, K, n_pos = None, max(1, int(want_k or self.lib.mu_spmm_stream_k(n))), n
        if sort_rows and n > 0:
            perm, _inv, K = self.launch_layout(X.indptr[1:] - X.indptr[:-1], want_k)
            n_pos = int(perm.numel())
        lens = self.empty((max(n_pos, 1),), torch.int64)[:n_pos]
        self._launch(self.lib.mu_csr_stream_len, n_pos, perm, X.indptr, lens)
        sptr = self._stream_sptr(lens, K)
        ent = self.empty((max(X.nnz, 1),), torch.int64)
        self._launch(self.lib.mu_csr_stream_fill, n_pos, perm, X.indptr, X.indices, X.values, sptr, ent)
        return DeviceStream(sptr, ent, (n, d), X.nnz, perm, K)

    def _use_tpack4(self, X: DeviceCSR) -> bool:
        """The tile-staged transposition (csrc/tpack4.hip) unless the shape needs the general one (2^31 rows, a row block
        of 2^29 entries; tune tpack4_off = 1 forces it: tests)."""
        n, d = X.shape
        return self.lib.mu_tune_get(b"tpack4_off") != 1 and bool(self.lib.mu_tpack4_supported(n, d, X.nnz))

    keep_tpack4_work = False  # tests / probes: keep the last fill's work buffer so that tpack4_status() can read its error word

    def _note_tpack4(self, work, n, d, nnz) -> torch.Tensor:
        """After a fourth-generation fill: the device int32[1] copy of its error word."""
        # (never by default: a work buffer kept across calls is a second 1.8 GB block at 1e6 x 200k - the next call's
        #  allocation then misses the caching allocator's pool: a hipMalloc inside every step, measured at 300 ms)
        self._tpack4_work = (work, (n, d, nnz)) if self.keep_tpack4_work else None
        # the fill's error word (1: bitmap and count pass disagree, 2: a tile could not be narrowed - a
        # silently wrong X^T) was read by tests only.  A 4-byte copy of it, queued behind the fill, goes with the stream
        # (DeviceStream.t4_err) to the consumer's next synchronisation (lsi: with the first Gram fetch; transpose_csr:
        # right away).
        off = int(self.lib.mu_tpack4_err_offset(n, d, nnz))
        return work[off:off + 4].view(torch.int32).clone()

    @staticmethod
    def raise_tpack4(err: int) -> None:
        if int(err) != 0:
            raise _ffi.MuonAmdError(f"mu_tpack4_fill: the transposition tripped an internal invariant (error word {int(err)}: "
                                    "1 = bitmap and count pass disagree, 2 = a tile could not be narrowed); X^T would be wrong")

    def tpack4_status(self) -> int:
        """Error word of the last fourth-generation fill (0 = fine; synchronises: tests and probes)."""
        got = self.__dict__.get("_tpack4_work")
        if got is None:
            return 0
        work, (n, d, nnz) = got
        err = ctypes.c_int(0)
        check(self.lib.mu_tpack4_status(_p(work), n, d, nnz, ctypes.byref(err)))
        return int(err.value)

    def transpose_stream(self, X: DeviceCSR, sort_rows: bool = True, before_fill=None,
                         K: Optional[int] = None, src=None) -> DeviceStream:
        """Row stream of X^T straight from X (no CSR of X^T; stable: cells ascending inside every row).
        ``src`` = (row stream of X, row_dst): the rows are read from the stream as contiguous pairs instead of from
        the CSR arrays (r05).  ``before_fill``: called once the count phase is done and before the fill is queued."""
        n, d = X.shape
        assert X.values.dtype == torch.float32
        if not self._use_tpack4(X):
            # (shapes the tile-staged transposition refuses: the CSR of X^T from the general kernel, then a streaming copy)
            if before_fill is not None:
                before_fill()
            return self.stream(self.transpose(X), sort_rows=sort_rows, K=K)
        # count phase and layout: made with the device CSR (with_plans: the fill is all that is left) or here
        cached = self._plan_of(X, "tplan") if (sort_rows and K is None) else None
        plan = cached or self._make_tplan(X, K, sort_rows)
        ent = self.empty((max(X.nnz, 1),), torch.int64)
        if before_fill is not None:
            before_fill()
        xs_ent, xs_dst = (src[0].ent, src[1]) if src is not None else (None, None)
        tp = self._tperm_of(X, cached, xs_ent, xs_dst) if (cached is not None and src is not None) else None
        if tp is not None and "counts" in tp:
            # (the same with the rows' counts per tile in the plan: the flat read-in, csrc/tflat.hip)
            cnt = plan["work"][int(self.lib.mu_tpack4_cnt_offset(n, d, X.nnz)):]
            self._launch(self.lib.mu_tflat_fill, n, d, X.nnz, X.indptr, xs_dst, xs_ent, tp["cdst"], cnt, tp["toff"],
                         tp["tiles"], tp["counts"], tp["slots"], ent)
        elif tp is not None:
            # (lsi's hot path: the slots and the tile schedule come from the plan, csrc/tperm.hip)
            cnt = plan["work"][int(self.lib.mu_tpack4_cnt_offset(n, d, X.nnz)):]
            self._launch(self.lib.mu_tperm_fill, n, d, X.nnz, X.indptr, xs_dst, xs_ent, tp["cdst"], cnt, tp["toff"],
                         tp["tiles"], tp["cont"], tp["slots"], ent)
        else:
            self._launch(self.lib.mu_tpack4_fill_stream, n, d, X.nnz, X.indptr, X.indices, X.values, xs_dst, xs_ent,
                         plan["sptr"], plan["inv"], ent, plan["work"], plan["wb"])
        err = self._note_tpack4(plan["work"], n, d, X.nnz)
        return DeviceStream(plan["sptr"], ent, (d, n), X.nnz, plan["perm"], plan["K"],
                            self._t4_prefix(plan["work"], n, d, X.nnz), err)

    def _tperm_of(self, X: DeviceCSR, plan, xs_ent, xs_dst):
        """The table of the table-driven fill for X's row stream as `xplan` lays it out, or None (tune tperm_off = 1, a
        stream laid out otherwise, phase accounting asked for, no memory for the table: the fill of csrc/tpack4.hip).
        ``plan``: X's cached `tplan`; the table is its "tperm" entry.  Tune tperm_flat = 1 asks for the table of the flat
        read-in (csrc/tflat.hip: its own tiles, the rows' counts per tile, the slots; no continuation words); 0, or a flat
        table that cannot be made, for that of the windowed read-in (csrc/tperm.hip).  Made with the FIRST fill that can
        use it and kept on the transposition plan: it costs 2 bytes per stored entry, which only lsi's operand building
        gets back - a TF-IDF-only caller never pays for it."""
        lib = self.lib
        got = plan.get("tperm")
        if got is False:  # (no memory for the table when it was tried: the old fill from then on)
            return None
        xplan = self._plan_of(X, "xplan")
        if (lib.mu_tune_get(b"tperm_off") == 1 or lib.mu_tune_get(b"tpack_dbg") > 0 or xplan is None
                or xs_dst is not xplan["row_dst"]):
            return None
        flat = lib.mu_tune_get(b"tperm_flat") == 1
        # (the widest tile follows the tune key of t4_geometry, the table's kind tperm_flat: a table recorded under other
        #  keys is made again)
        keys = (lib.mu_tune_get(b"tpack4_c"), flat)
        if got is not None and got["keys"] == keys:
            return got if ("counts" in got or xs_ent.data_ptr() % 256 == 0) else None
        got = self._tperm_table(X, plan, xs_dst, True) if flat else None
        if got is None:
            if xs_ent.data_ptr() % 256 != 0:  # (the windows of csrc/tperm.hip are 256-byte blocks of the stream)
                return None
            got = self._tperm_table(X, plan, xs_dst, False)
        if got is None:
            plan["tperm"] = False
            return None
        plan["tperm"] = dict(got, keys=keys)
        return plan["tperm"]

    def _tperm_table(self, X: DeviceCSR, plan, xs_dst, flat):
        """The arrays of mu_tflat_plan (``flat``: tiles, counts per (tile, row), slots) or of mu_tperm_plan (tiles,
        continuation rows, slots), or None when they cannot be made: no memory, a refused launch, a row that is not
        canonical."""
        lib = self.lib
        n, d = X.shape
        _rpb, G, Ct = self._t4_tiling(n, d, X.nnz)
        Ct = min(Ct, 512)
        try:
            ntile = self.empty((G,), torch.int32)
            if flat:
                err = torch.zeros((1,), dtype=torch.int32, device=self.device)
                self._launch(lib.mu_tflat_plan, n, d, X.nnz, X.indptr, X.indices, None, Ct, None, ntile, None, None, None,
                             err)
            else:
                self._launch(lib.mu_tperm_plan, n, d, X.nnz, X.indptr, X.indices, None, Ct, None, ntile, None, None, None)
            toff = torch.zeros((G + 1,), dtype=torch.int64, device=self.device)
            toff[1:] = torch.cumsum(ntile.long(), 0)
            T = int(toff[-1].item())
            tiles = self.empty((T + G,), torch.int32)
            slots = self.empty((X.nnz,), torch.int16)
            if flat:
                side = dict(counts=self.empty((512 * T,), torch.int16))
                self._launch(lib.mu_tflat_plan, n, d, X.nnz, X.indptr, X.indices, xs_dst, Ct, toff, None, tiles,
                             side["counts"], slots, err)
                if int(err.item()) != 0:
                    raise RuntimeError("mu_tflat_plan: a row is not canonical")
            else:
                side = dict(cont=self.empty((16 * T,), torch.int32))
                self._launch(lib.mu_tperm_plan, n, d, X.nnz, X.indptr, X.indices, xs_dst, Ct, toff, None, tiles,
                             side["cont"], slots)
            inv = plan["inv"]
            cdst = (plan["sptr"][inv.long()] if inv is not None else plan["sptr"][:d]).contiguous()
        except (RuntimeError, MemoryError):  # (torch's out-of-memory errors and a refused launch are RuntimeErrors)
            return None
        return dict(tile_cols=Ct, toff=toff, tiles=tiles, slots=slots, cdst=cdst, n_tiles=T, **side)

    def _t4_tiling(self, n, d, nnz):
        """(rows per row block, row blocks, columns of the widest tile) of the tile-staged transposition of this shape:
        the one query of mu_tpack4_geometry."""
        rpb, G, Ct = ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_int(0)
        check(self.lib.mu_tpack4_geometry(n, d, nnz, ctypes.byref(rpb), ctypes.byref(G), ctypes.byref(Ct)))
        return int(rpb.value), int(G.value), int(Ct.value)

    def _t4_geometry(self, n, d, nnz):
        """(rows per row block, row blocks): what the ranged products and the tests ask for."""
        return self._t4_tiling(n, d, nnz)[:2]

    def _t4_prefix(self, work, n, d, nnz):
        rpb, G = self._t4_geometry(n, d, nnz)
        off = int(self.lib.mu_tpack4_cnt_offset(n, d, nnz))
        # (a view: the work buffer lives as long as the stream that carries it)
        cnt = work[off:off + 4 * (G + 1) * d].view(torch.int32)
        return dict(cnt=cnt, rpb=rpb, blocks=G, stride=d)

    # -- the cell slice of lsi's warm start (r06: no operands of its own) --------------------------------
    def slice_plan(self, X: DeviceCSR, n_s: int, max_ranges: int = 16):
        """Which cells the warm start's slice holds: <= 16 ranges of whole ROW BLOCKS of the transposition (so that the
        slice's cells are a contiguous piece of every row of X^T, found through the count pass' prefix table), spread
        evenly over this shard's cells (files list cells sample by sample: the first cells may be one batch), about
        ``n_s`` cells together.  Host integers only - the ranges and where they lie in the CSR (one read of <= 32 row
        pointers) - cached with the index arrays they describe, like the other plans: a second call reads nothing from
        the device.  None when the shape does not take the ranged products (no fourth-generation transposition, no slab
        pointers)."""
        n, d = X.shape
        if n_s <= 0 or X.values.dtype != torch.float32 or not self._use_tpack4(X) or self._slab_ptr_of(X) is None:
            return None
        # (cached with the plans: `with_values` hands them - by reference - from the counts to every TF-IDF result, so
        #  the plan made in the first call serves the later ones)
        plans, key = CsrPlans.of(X), (int(n_s), int(max_ranges))
        if plans.wplan is not None and plans.wplan[1] == key:
            return plans.wplan[0]
        rpb, G = self._t4_geometry(n, d, X.nnz)
        if G < 1:
            return None
        blocks = max(1, min(G, int(round(n_s / rpb))))
        R = max(1, min(int(max_ranges), blocks))
        per = max(1, min(int(round(blocks / R)), G // R))  # (blocks per range; ranges G // R blocks apart: no overlap)
        g0s = [(r * G) // R for r in range(R)]
        rows = [(g0 * rpb, min((g0 + per) * rpb, n)) for g0 in g0s]
        edges = X.indptr[torch.tensor([v for ab in rows for v in ab], device=X.indptr.device)].tolist()
        plan = dict(rpb=rpb, ranges=[dict(g0=g0, g1=g0 + per, row0=a, row1=b, lo=int(edges[2 * i]), hi=int(edges[2 * i + 1]))
                                     for i, (g0, (a, b)) in enumerate(zip(g0s, rows))])
        plan["n_s"] = sum(r["row1"] - r["row0"] for r in plan["ranges"])
        plan["nnz_s"] = sum(r["hi"] - r["lo"] for r in plan["ranges"])
        plans.wplan = (plan, key)
        return plan

    def slice_stream(self, X: DeviceCSR, plan) -> dict:
        """Compact row stream of the slice's rows (mu_csr_slice_stream: range after range, rows in their own order) with
        the table of its 8192-column super-slab boundaries - the operand of X_S Q (spmm_slice)."""
        n, d = X.shape
        rg = plan["ranges"]
        n_s, nnz_s = plan["n_s"], plan["nnz_s"]
        S1 = -(-d // 8192) + 1
        sptr = self.empty((n_s + 1,), torch.int64)
        ent = self.empty((max(nnz_s, 1),), torch.int64)
        rel = self.empty((S1 * max(n_s, 1),), torch.int32)
        arr = lambda key, f=None: (ctypes.c_int64 * len(rg))(*[(f(r) if f else r[key]) for r in rg])  # noqa: E731
        self._launch(self.lib.mu_csr_slice_stream, len(rg), arr("row0"), arr(None, lambda r: r["row1"] - r["row0"]),
                     arr("lo"), arr("hi"), d, X.indptr, X.indices, X.values, self._slab_ptr_of(X), sptr, ent, rel)
        # K and the split of the column super-slabs over blockIdx.y: enough workgroups for two rounds of the chip
        n_cus = torch.cuda.get_device_properties(self.device).multi_processor_count
        K = 8
        while K > 1 and -(-n_s // (64 * K)) * (S1 - 1) < 2 * n_cus:
            K //= 2
        wgs = -(-n_s // (64 * K))
        ny = max(1, min(S1 - 1, 16, -(-2 * n_cus // max(wgs, 1))))  # (<= 16 column groups: the launch takes 32 ranges)
        group = -(-(S1 - 1) // ny)  # consecutive super-slabs of one blockIdx.y: one contiguous column range
        return dict(sptr=sptr, ent=ent, rel=rel, n_s=n_s, nnz_s=nnz_s, K=K, group=group, d=d, S=S1 - 1)

    def spmm_slice(self, S: dict, Q: torch.Tensor) -> torch.Tensor:
        """Y_S = X_S Q [n_s x B] on the compact slice stream, column super-slabs split over the chip, partial products
        summed in fixed order.  B = 16 / 32 / 64; the kernel exists for 64 columns only: a narrower Q is zero-padded to
        64 and the leading B columns of the product returned (the padded ones are exact zeros)."""
        d, n_s = S["d"], S["n_s"]
        B = Q.shape[1] if Q.dim() == 2 else 0
        assert Q.shape == (d, B) and B in (16, 32, 64) and Q.dtype == torch.float32 and Q.is_contiguous()
        if B < 64:
            return self.spmm_slice(S, self._pad64(Q))[:, :B].contiguous()
        ns, g = S["S"], S["group"]
        ny = -(-ns // g)
        part = self.empty((ny, n_s, 64), torch.float32)
        h = (ctypes.c_int32 * (5 * ny))()
        for r in range(ny):  # (the super-slabs r g .. (r + 1) g - 1 are contiguous in the columns and in every row)
            h[5 * r:5 * r + 5] = [r * g * 8192, min((r + 1) * g * 8192, d), r * g * 8192, r * g, min((r + 1) * g, ns)]
        self._launch(self.lib.mu_spmm_stream_ranges_slab_f32, n_s, S["sptr"], S["ent"], None, S["K"], Q, d, part, n_s * 64,
                     S["rel"], n_s, ny, h, 1, self.spmm_slab_ranged(S["K"]))
        return _sum_parts(part)

    def _pad64(self, A: torch.Tensor) -> torch.Tensor:
        """The f32 block A [rows, B < 64] in the leading columns of a zeroed 64-column block: the one width the ranged
        products exist for."""
        P = self.zeros((A.shape[0], 64), torch.float32)
        P[:, :A.shape[1]] = A
        return P

    def spmm_slab_ranged(self, k_layout: int) -> int:
        """The slab width of a ranged product (B = 64, f32; the ranged entry takes the layout's K as it is and has no
        ablation modes)."""
        return spmm_slab_cols(self.lib, 64, k_layout, torch.float32, self.lib.mu_tune_get(b"spmm_slab"), ranged=True)

    def spmm_slice_t(self, Xt: DeviceStream, plan, Ys: torch.Tensor) -> torch.Tensor:
        """Z = X_S^T Y_S [d x B] on the row stream of X^T as it is: the slice's cells are <= 16 contiguous pieces of
        every row, found through the transposition's count prefixes (Xt.t4).  B = 16 / 32 / 64, a narrower Y_S
        zero-padded to the kernel's 64 columns like in spmm_slice."""
        d, n = Xt.shape
        t4, rg = Xt.t4, plan["ranges"]
        B = Ys.shape[1] if Ys.dim() == 2 else 0
        assert t4 is not None and t4["rpb"] == plan["rpb"] and Ys.shape == (plan["n_s"], B) and B in (16, 32, 64) \
            and Ys.dtype == torch.float32 and Ys.is_contiguous()
        if B < 64:
            return self.spmm_slice_t(Xt, plan, self._pad64(Ys))[:, :B].contiguous()
        Z = self.empty((d, 64), torch.float32)
        h = (ctypes.c_int32 * (5 * len(rg)))()
        q_off = 0
        for i, r in enumerate(rg):
            h[5 * i:5 * i + 5] = [r["row0"], r["row1"], q_off, r["g0"], r["g1"]]
            q_off += r["row1"] - r["row0"]
        self._launch(self.lib.mu_spmm_stream_ranges_slab_f32, Xt.n_pos, Xt.sptr, Xt.ent, Xt.perm, Xt.k, Ys, plan["n_s"], Z,
                     0, t4["cnt"], t4["stride"], len(rg), h, len(rg), self.spmm_slab_ranged(Xt.k))
        return Z

    def split_streams(self, X: DeviceCSR):
        """(row streams of X, row streams of X^T) for an f64-valued CSR: see SplitOperand."""
        return _split_build(X, lambda P: (self.stream(P), self.transpose_stream(P)))

    def launch_layout(self, lens: torch.Tensor, K: Optional[int] = None):
        """Where the rows go in a row stream (include/muon_amd.h): sorted by length (descending,
        stable) and dealt round robin - row-set q of the sorted order goes to workgroup q % n_wg,
        inside it to wave (q // n_wg) % 16 and row-set slot (q // n_wg) // 16 - so that the four rows
        a wave advances in lock step have similar lengths and every workgroup and wave gets the same
        mix.  Returns (perm int32[n_pos], inv int32[n], K)."""
        n = int(lens.numel())
        K = max(1, int(K or self.lib.mu_spmm_stream_k(n)))
        W = 16  # waves of a workgroup
        per_wg = 4 * W * K
        n_wg = max(1, (n + per_wg - 1) // per_wg)
        # One workgroup per CU runs at a time (128 KiB of LDS) and the dealt workgroups take equally
        # long, so the launch proceeds in rounds of n_cus workgroups: a last round that is 3/4 empty
        # costs a full one.  Dealing the same rows over a whole number of rounds (the last row-set
        # slots of every wave stay empty instead) makes every round shorter: Xt*Y at 200k rows
        # 447 -> 512 workgroups, X*Q at 1e6 rows 1954 -> 2048.
        n_cus = torch.cuda.get_device_properties(self.device).multi_processor_count
        if n_wg > n_cus and not self.__dict__.get("_no_round_fill"):
            n_wg = -(-n_wg // n_cus) * n_cus
        elif 5 * n_wg >= 4 * n_cus and not self.__dict__.get("_no_round_fill"):
            # a little less than one round: every CU takes a workgroup (100 000 rows at K = 7: 224 -> 256
            # workgroups of 391 rows; empty row slots are cheap).  A/B on one box: MOFA c4 -1 %, c3shard -0.3 %;
            # at 157 of 256 workgroups (10k x 30k) it cost 1 %: hence the 4 / 5 threshold.
            n_wg = n_cus
        n_pos = n_wg * per_wg
        order = torch.argsort(lens, descending=True, stable=True)
        i = torch.arange(n, device=lens.device)
        q, j = i // 4, i % 4
        b, t = q % n_wg, q // n_wg
        w, k = t % W, t // W
        pos = ((b * W + w) * K + k) * 4 + j
        perm = torch.full((n_pos,), -1, dtype=torch.int32, device=lens.device)
        perm[pos] = order.to(torch.int32)
        inv = torch.empty((n,), dtype=torch.int32, device=lens.device)
        inv[order] = pos.to(torch.int32)
        return perm, inv, K

    # -- sliced-ELL operand of the narrow-block SpMM (csrc/spmm_ell.hip) ---------------------------
    def ell16_fits(self, X, wide: bool) -> bool:
        """The sliced-ELL kernels address both dense operands with 32-bit byte offsets (64-byte rows of an f32 block,
        128-byte rows of an f64 one): X and X^T must both stay under 4 GiB of dense rows, and neither is empty."""
        return min(X.shape) > 0 and max(X.shape) * (128 if wide else 64) < (1 << 32)

    def ell16(self, X: DeviceCSR, wide: bool = False):
        """Lay a canonical CSR out for mu_spmm_ell16_f32 / _f64 (once per fit: the operand of MOFA's sparse views is
        multiplied hundreds of times).  f32 values -> DeviceEll; ``wide`` (against f64 blocks): 512-column slabs,
        and f64 values -> SplitOperand (hi + lo)."""
        if not self.ell16_fits(X, wide):
            raise NotImplementedError(f"sliced ELL: a {X.shape[0]} x {X.shape[1]} operand does not fit (ell16_fits)")
        waves = int(self.lib.mu_spmm_ell16_waves(X.shape[0]))

        def layout(P):
            return ell16_layout(P, waves, 512 if wide else 1024, self.slab_ptr_width, self._ell16_fill)

        if X.values.dtype == torch.float32:
            return layout(X)
        assert wide
        return _split_build(X, lambda P: (layout(P),))[0]

    def ell16_pair(self, X: DeviceCSR, wide: bool = False):
        """(layout of X, layout of X^T) - both operands of a fit.  The transposed CSR comes from the tile-staged
        transposition (f32 values; an f64-valued matrix is transposed as its hi and lo parts, the second only when
        some value is not exact in f32) instead of the general kernel behind `transpose`."""
        def pair(P):
            return self.ell16(P, wide), self.ell16(self.transpose_csr(P), wide)

        if X.values.dtype == torch.float32:
            return pair(X)
        assert wide
        return _split_build(X, pair)

    def col_moments(self, Y: torch.Tensor, a: int, b: int):
        """(sum, sum of squares) per column over rows a .. b-1 of a dense row-major f32 / f64 block: f64 sums, one pass."""
        assert Y.dim() == 2 and Y.is_contiguous() and Y.dtype in (torch.float32, torch.float64)
        D = int(Y.shape[1])
        chunks = max(1, int(self.lib.mu_dense_col_moments_chunks(b - a, D)))
        part = self.empty((chunks, 2, D), torch.float64)
        self._launch(self.lib.mu_dense_col_moments, _dt(Y), int(a), int(b), D, Y, chunks, part)
        s = part.sum(dim=0)
        return s[0], s[1]

    def _ell16_fill(self, X, slab_cols, sp, perm, hdr, win_base, ent):
        self._launch(self.lib.mu_ell16_fill, int(perm.numel()) // 16, X.shape[1], X.nnz, int(slab_cols), X.indices, X.values,
                     sp, perm, hdr, win_base, ent)

    def slab_ptr_width(self, X: DeviceCSR, width: int) -> torch.Tensor:
        """First entry of every row at or behind every multiple of ``width`` columns (+ the row's end)."""
        n, d = X.shape
        sp = self.empty((n * (-(-d // width) + 1),), torch.int64)
        self._launch(self.lib.mu_csr_slab_ptr_width, n, d, int(width), X.indptr, X.indices, sp)
        return sp

    def spmm_ell(self, E: DeviceEll, Q: torch.Tensor, out=None, accumulate: bool = False) -> torch.Tensor:
        n, d = E.shape
        wide = Q.dtype == torch.float64
        if Q.shape != (d, 16) or Q.dtype not in (torch.float32, torch.float64) or not Q.is_contiguous():
            raise TypeError("the sliced-ELL SpMM needs a contiguous f32 / f64 block of 16 columns")
        if E.slab_cols != (512 if wide else 1024):
            raise TypeError("sliced-ELL operand laid out for the other block type (slab width)")
        if accumulate and not wide:
            raise TypeError("accumulating sliced-ELL products exist for f64 blocks only")
        if out is None:
            assert not accumulate
            out = self.empty((n, 16), Q.dtype)
        # r06: an operand of a few thousand rows (one rank's shard of a sharded fit) is a few dozen workgroups that each
        # pull all of Q through their LDS - its column slabs are split over blockIdx.y, the partial products summed in
        # order (mu_spmm_ell16_parts: one part for every shape that fills a round of the chip by its rows)
        wv, parts = ctypes.c_int(0), ctypes.c_int(1)
        check(self.lib.mu_spmm_ell16_parts(n, d, int(wide), ctypes.byref(wv), ctypes.byref(parts)))
        if parts.value > 1:
            slabs = -(-d // E.slab_cols)
            ny = -(-slabs // -(-slabs // parts.value))
            part = self.empty((ny, n, 16), Q.dtype)
            fn = self.lib.mu_spmm_ell16_parts_f64 if wide else self.lib.mu_spmm_ell16_parts_f32
            self._launch(fn, wv.value, parts.value, int(E.perm.numel()), d, E.hdr, E.wave_base, E.ent, E.perm, Q, part,
                         n * 16)
            if accumulate:
                out += part.sum(dim=0)
            else:
                torch.sum(part, dim=0, out=out)
            return out
        if wide:
            self._launch(self.lib.mu_spmm_ell16_f64, E.waves, int(E.perm.numel()), d, E.hdr, E.wave_base, E.ent, E.perm, Q,
                         out, int(bool(accumulate)))
        else:
            self._launch(self.lib.mu_spmm_ell16_f32, E.waves, int(E.perm.numel()), d, E.hdr, E.wave_base, E.ent, E.perm, Q,
                         out)
        return out

    def stream_both(self, X: DeviceCSR):
        """(row stream of X, row stream of X^T).  The two builders are independent; the streaming
        copy of X (HBM bound) runs on a second stream under the transposition, whose fill is
        instruction bound and leaves half of every CU's wave slots free."""
        have = self._xstream_of(X)
        if have is not None and self._use_tpack4(X):
            # r05: the TF-IDF scale sweep wrote X's stream already; the transposition reads its rows from there
            Xs, row_dst = have
            return Xs, self.transpose_stream(X, src=(Xs, row_dst))
        cur = torch.cuda.current_stream(self.device)
        side = self.__dict__.get("_side_stream")
        if side is None:
            side = self._side_stream = torch.cuda.Stream(self.device)
        got = []

        def start_copy():
            # right before the fill: the count phase of the transposition (binary searches and a
            # histogram, latency bound) slowed down 4x next to the streaming copy, the fill does not
            side.wait_stream(cur)
            wg = 2  # (A/B on one box, c3: 32 -> 451, 4 -> 449, 2 -> 441 ms per step)
            with torch.cuda.stream(side):
                self.tune("pack_wg", wg)  # few workgroups per CU: the fill's 1024-thread groups must fit next to them
                # ... and the unpipelined loop: the pipelined copy is faster alone (22.5 -> 20-21.6 ms at 1e6 x 200k) and
                # costs the fill more next to it (both together 87 -> 95 ms; scripts/probes/stream_pipe_probe.py)
                self.tune("stream_pipe", 1)
                try:
                    got.append(self.stream(X))
                finally:
                    self.tune("pack_wg", 0)
                    self.tune("stream_pipe", 0)

        Xt = self.transpose_stream(X, before_fill=start_copy)
        Xs = got[0]
        cur.wait_stream(side)
        for t in (Xs.sptr, Xs.ent, Xs.perm):
            if t is not None:
                t.record_stream(cur)
        return Xs, Xt

    def fetch_async(self, tensors):
        """Start device -> host copies of small tensors into pinned staging buffers; ``wait()`` on
        the returned handle blocks only until these copies are done - work queued on the stream
        afterwards keeps running (the host-side Ritz step of the LSI hides under the next SpMM)."""
        # a staging buffer belongs to ONE handle until its wait() has copied the data out (several fetches can be in
        # flight: the pipelined LSI loop starts the next block's fetch before it reads the current one)
        pool = self.__dict__.setdefault("_pinned_free", {})
        bufs = []
        for t in tensors:
            free = pool.setdefault((tuple(t.shape), t.dtype), [])
            buf = free.pop() if free else torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            bufs.append(buf)
            buf.copy_(t, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        return _Fetch(bufs, ev, pool)

    def tune(self, key: str, value: int) -> None:
        check(self.lib.mu_tune_set(key.encode(), int(value)))

    def tune_keys(self) -> dict:
        """{name: default} of the library's tune keys (csrc/common.hpp: MU_TUNE_KEYS)."""
        lib = self.lib
        return {lib.mu_tune_name(i).decode(): lib.mu_tune_default(i) for i in range(lib.mu_tune_count())}

    def spmm_slab(self, k_layout: int, n_pos: int, B: int, dtype=torch.float32) -> int:
        """The slab width for a product on a row stream dealt for ``k_layout`` row-sets per wave (0: the library picks
        K from n_pos) - spmm_slab_cols with the K in effect (tune key spmm_k) and the tune key spmm_slab."""
        lib = self.lib
        K = lib.mu_tune_get(b"spmm_k")
        if not 1 <= K <= 8:
            K = k_layout if 1 <= k_layout <= 8 else lib.mu_spmm_stream_k(n_pos)
        return spmm_slab_cols(lib, B, K, dtype, lib.mu_tune_get(b"spmm_slab"), lib.mu_tune_get(b"spmm_mode"))

    def spmm(self, X, Q: torch.Tensor, out=None, accumulate: bool = False) -> torch.Tensor:
        n, d = X.shape
        B = Q.shape[1]
        assert Q.shape[0] == d and Q.dtype in (torch.float32, torch.float64) and Q.is_contiguous()
        if isinstance(X, SplitOperand):
            # f64 values as two f32 operands: X Q = X_hi Q + X_lo Q, accumulated in f64
            out = self.spmm(X.hi, Q, out=out, accumulate=accumulate)
            if X.lo is not None:
                self.spmm(X.lo, Q, out=out, accumulate=True)
            return out
        if isinstance(X, DeviceEll):
            return self.spmm_ell(X, Q, out=out, accumulate=accumulate)
        if isinstance(X, DeviceStream):
            wide = Q.dtype == torch.float64
            if B not in ((16, 32) if wide else (16, 32, 64)):
                raise TypeError("the row-stream SpMM needs a dense block of width 16, 32 or 64 (f64: 16 or 32)")
            if accumulate and not wide:
                raise TypeError("accumulating row-stream products exist for f64 blocks only")
            if out is None:
                assert not accumulate
                out = self.empty((n, B), Q.dtype)
            if wide:
                self._launch(self.lib.mu_spmm_stream_f64, X.n_pos, d, X.sptr, X.ent, X.perm, X.k, Q, B, out,
                             int(bool(accumulate)))
            else:
                self._launch(self.lib.mu_spmm_stream_slab_f32, X.n_pos, d, X.sptr, X.ent, X.perm, X.k, Q, B, out,
                             self.spmm_slab(X.k, X.n_pos, B))
            return out
        if X.values.dtype != Q.dtype:
            raise TypeError("spmm needs values and dense block of one dtype")
        if out is None:
            out = self.empty((n, B), Q.dtype)
        fn = self.lib.mu_spmm_f32 if Q.dtype == torch.float32 else self.lib.mu_spmm_f64
        self._launch(fn, n, d, X.indptr, X.indices, X.values, Q, B, out, 0)
        return out

    def gram(self, A: torch.Tensor):
        n, B = A.shape
        assert A.dtype == torch.float32 and A.is_contiguous()
        G = self.empty((B, B), torch.float64)
        cs = self.empty((B,), torch.float64)
        work, wb = self._work(self.lib.mu_gram_worksize(n, B))
        self._launch(self.lib.mu_gram_f32, n, B, A, G, cs, work, wb)
        return G, cs

    def gram_cross(self, A: torch.Tensor, Bm: torch.Tensor) -> torch.Tensor:
        """C = A^T Bm in f64 (A, Bm n x B f32)."""
        n, B = A.shape
        assert Bm.shape == A.shape and A.dtype == torch.float32 and Bm.dtype == torch.float32
        assert A.is_contiguous() and Bm.is_contiguous()
        Cm = self.empty((B, B), torch.float64)
        work, wb = self._work(self.lib.mu_gram_worksize(n, B))
        self._launch(self.lib.mu_gram_cross_f32, n, B, A, Bm, Cm, work, wb)
        return Cm

    def apply(self, A: torch.Tensor, M: torch.Tensor, bias=None, out=None) -> torch.Tensor:
        n, B = A.shape
        assert M.shape == (B, B) and M.dtype == torch.float32 and M.is_contiguous()
        if out is None:
            out = torch.empty_like(A)
        self._launch(self.lib.mu_dense_apply_f32, n, B, A, M, bias, out)
        return out

    def project_out_block(self, Q: torch.Tensor, C: torch.Tensor, Z: torch.Tensor) -> torch.Tensor:
        """Z -= Q C in place (C: the f64 B x B coefficients Q^T Z of gram_cross)."""
        n, B = Q.shape
        assert Z.shape == Q.shape and C.shape == (B, B) and C.dtype == torch.float64 and C.is_contiguous()
        assert Q.dtype == torch.float32 and Z.dtype == torch.float32 and Z.is_contiguous() and Q.is_contiguous()
        self._launch(self.lib.mu_dense_project_out_f32, n, B, Q, C, Z)
        return Z

    def chol_rinv(self, G: torch.Tensor, w: int, flag: torch.Tensor) -> torch.Tensor:
        """R^-1 (f32, B x B, upper) of the leading w x w block of the f64 Gram G = R^T R, on the
        device; ``flag`` (int32[1]) is set when a pivot was not safely positive."""
        B = G.shape[0]
        assert G.dtype == torch.float64 and G.is_contiguous() and flag.dtype == torch.int32
        M = self.empty((B, B), torch.float32)
        self._launch(self.lib.mu_chol_rinv_f64, B, int(w), G, M, flag)
        return M

    def randn(self, rows: int, B: int, seed: int) -> torch.Tensor:
        out = self.empty((rows, B), torch.float32)
        self._launch(self.lib.mu_randn_f32, rows * B, int(seed) & (2**64 - 1), out)
        return out

    # -- MOFA+: tall-skinny products of a dense view with 16-column factor blocks ------------------
    skinny_mixed = True  # f64 products of a dense view stored in f32 (mu_skinny_*_f64_f32)

    def skinny_nn(self, Y: torch.Tensor, T16: torch.Tensor) -> torch.Tensor:
        """Y [n x D] (row slice of a row-major matrix) times T16 [D x 16] -> [n x 16].  Y may be stored in f32
        under an f64 block: the product is the f64 one."""
        n, D = Y.shape
        mixed = Y.dtype == torch.float32 and T16.dtype == torch.float64
        assert T16.shape == (D, 16) and (mixed or T16.dtype == Y.dtype) and T16.is_contiguous() and Y.stride(1) == 1
        out = self.empty((n, 16), T16.dtype)
        ld = Y.stride(0) if n > 1 else D
        if mixed:
            self._launch(self.lib.mu_skinny_nn_f64_f32, n, D, ld, Y, T16, out)
        else:
            self._launch(self.lib.mu_skinny_nn, _dt(Y), n, D, ld, Y, T16, out)
        return out

    def skinny_tn(self, Y: torch.Tensor, Z16: torch.Tensor) -> torch.Tensor:
        """Y^T [D x n] times Z16 [n x 16] -> [D x 16] (Y stored in f32 under an f64 block: the f64 product)."""
        n, D = Y.shape
        mixed = Y.dtype == torch.float32 and Z16.dtype == torch.float64
        assert Z16.shape == (n, 16) and (mixed or Z16.dtype == Y.dtype) and Z16.is_contiguous() and Y.stride(1) == 1
        out = self.empty((D, 16), Z16.dtype)
        work, wb = self._work(self.lib.mu_skinny_tn_worksize(_dt(Z16), n, D))
        ld = Y.stride(0) if n > 1 else D
        if mixed:
            self._launch(self.lib.mu_skinny_tn_f64_f32, n, D, ld, Y, Z16, out, work, wb)
        else:
            self._launch(self.lib.mu_skinny_tn, _dt(Y), n, D, ld, Y, Z16, out, work, wb)
        return out

    # -- MOFA+ coordinate updates (reference tools.py:585 -> mofapy2 node updates) -----------
    def mofa_update_w(self, B, tau, Gz, Z2, alpha, lth, l1mth, spikeslab, EW, EW2, gamma, EWh2, sig2):
        G, D, K = B.shape
        self._launch(self.lib.mu_mofa_update_w, _dt(EW), D, K, G, B, tau, Gz, Z2, alpha, lth, l1mth, int(bool(spikeslab)),
                     EW, EW2, gamma, EWh2, sig2)

    def mofa_update_z(self, A, pres, grp, Gw, dw2, alphaz, EZ, EZ2, sig2, corr=None):
        M, N, K = A.shape
        G = alphaz.shape[0]
        self._launch(self.lib.mu_mofa_update_z, _dt(EZ), N, K, M, G, A, pres, grp, Gw, dw2, alphaz, corr, EZ, EZ2, sig2)

    def mofa_rowstats_work(self, K: int) -> torch.Tensor:
        return self.empty((int(self.lib.mu_mofa_rowstats_work_doubles(int(K))),), torch.float64)

    def mofa_rowstats(self, E, E2, r0, r1, work, wgt=None, aux=None, scale_out=False, out_pad=None, col0=0,
                      out_t=None, gram=None, s2=None, s1=None):
        """One pass over rows r0..r1 of the factor / weight block E (include/muon_amd.h)."""
        K = E.shape[1]
        ld = int(out_pad.shape[1]) if out_pad is not None else 0
        ld_t = int(out_t.shape[1]) if out_t is not None else 0
        self._launch(self.lib.mu_mofa_rowstats, _dt(E), int(r0), int(r1), K, E, E2, wgt, aux, int(bool(scale_out)), out_pad,
                     ld, int(col0), out_t, ld_t, gram, s2, s1, work)

    def umap_strengths(self, dist, idx, target: float, mean_all: float):
        """Membership strengths of a neighbour table [n, k] (include/muon_amd.h): a thread per row."""
        n, k = dist.shape
        assert dist.dtype == torch.float64 and idx.dtype == torch.int64 and dist.is_contiguous() and idx.is_contiguous()
        out = self.empty((n, k), torch.float64)
        self._launch(self.lib.mu_umap_strengths_f64, int(n), int(k), dist, idx, float(target), float(mean_all), out)
        return out

    def wnn_bandwidth(self, X, g_indptr, g_indices, r_indptr, r_indices, n_bw: int, bbox: float):
        """csigma of muon.pp.neighbors, a wave per cell (include/muon_amd.h); returns (csigma, overflowed)."""
        n, p = X.shape
        out = self.empty((n,), torch.float64)
        over = self.zeros((1,), torch.int32)
        self._launch(self.lib.mu_wnn_bandwidth_f64, int(n), int(p), X, g_indptr, g_indices, r_indptr, r_indices, int(n_bw),
                     float(bbox), out, over)
        return out, bool(int(over.item()))

    def knn_filter(self, Xq, Xc, sqq, sqc, thr, self_pos, c_lo, c_hi, buf_pos, buf_d, cnt):
        """Candidates of positions [c_lo, c_hi) that beat the queries' thresholds (include/muon_amd.h)."""
        self._launch(self.lib.mu_knn_filter_f64, int(Xq.shape[0]), int(c_lo), int(c_hi), int(Xq.shape[1]), Xq, Xc, sqq, sqc,
                     thr, self_pos, int(buf_pos.shape[1]), buf_pos, buf_d, cnt)

    def knn_merge(self, cur_d, cur_p, buf_d, buf_pos, cnt):
        """list ++ buffer -> (the kc smallest distances ascending, their positions, the new thresholds)
        (include/muon_amd.h mu_knn_merge_f64)."""
        n, kc = cur_d.shape
        out_d, out_p = torch.empty_like(cur_d), torch.empty_like(cur_p)
        thr = self.empty((n,), torch.float64)
        self._launch(self.lib.mu_knn_merge_f64, int(n), int(kc), int(buf_d.shape[1]), cur_d, cur_p, buf_d, buf_pos, cnt,
                     out_d, out_p, thr)
        return out_d, out_p, thr

    def knn_merge_wide_max(self) -> int:
        """The largest kc + cap ``knn_merge_wide`` takes."""
        return int(self.lib.mu_knn_merge_wide_max())

    def knn_merge_wide(self, cur_d, cur_p, buf_d, buf_pos, cnt):
        """``knn_merge`` for kc + cap up to ``knn_merge_wide_max()``: a workgroup per query (csrc/scrublet.hip,
        include/muon_amd.h mu_knn_merge_wide_f64); identical arrays where both take the shape."""
        n, kc = cur_d.shape
        out_d, out_p = torch.empty_like(cur_d), torch.empty_like(cur_p)
        thr = self.empty((n,), torch.float64)
        self._launch(self.lib.mu_knn_merge_wide_f64, int(n), int(kc), int(buf_d.shape[1]), cur_d, cur_p, buf_d, buf_pos,
                     cnt, out_d, out_p, thr)
        return out_d, out_p, thr

    def csr_pair_rows(self, X: DeviceCSR, parents: torch.Tensor) -> DeviceCSR:
        """Row s of the result = row parents[s, 0] + row parents[s, 1] of the canonical device CSR ``X`` (f32 values;
        indices int32, or int64 and then the result's are too; ``parents`` int64 [n_sim, 2] on the device): the union
        of the two patterns, columns ascending, nothing pruned, the f32 sum where both store the column
        (csrc/scrublet.hip).  Index arrays of its own, so none of X's derived tables."""
        n, d = X.shape
        if (parents.dtype != torch.int64 or parents.dim() != 2 or parents.shape[1] != 2
                or X.values.dtype != torch.float32 or X.indices.dtype not in (torch.int32, torch.int64)):
            raise TypeError("csr_pair_rows: f32 values, int32 or int64 indices, parents int64 [n_sim, 2]")
        parents = parents.contiguous()
        k = int(parents.shape[0])
        ib = 8 if X.indices.dtype == torch.int64 else 4
        row_nnz = self.empty((k,), torch.int64)
        new_indptr = self.zeros((k + 1,), torch.int64)
        self._launch(self.lib.mu_csr_pair_rows_count, ib, n, k, X.indptr, X.indices, parents, row_nnz)
        if k:
            self._launch(self.lib.mu_exclusive_scan_i64, k, row_nnz, new_indptr)
        new_nnz = int(new_indptr[-1].item())
        new_indices = self.empty((new_nnz,), X.indices.dtype)
        new_values = self.empty((new_nnz,), torch.float32)
        self._launch(self.lib.mu_csr_pair_rows_fill, ib, n, k, X.indptr, X.indices, X.values, parents, new_indptr,
                     new_indices, new_values)
        return DeviceCSR(new_indptr, new_indices, new_values, (k, int(d)))

    def densify_rows(self, X: DeviceCSR, lo: int, hi: int) -> torch.Tensor:
        """Rows [lo, hi) of a device CSR as a dense chunk (include/muon_amd.h)."""
        out = self.empty((hi - lo, X.shape[1]), X.values.dtype)
        self._launch(self.lib.mu_csr_densify_rows, _dt(X.values), int(lo), int(hi), int(X.shape[1]), X.indptr, X.indices,
                     X.values, out)
        return out

    # -- muon.prot.pp.dsb (csrc/prot.hip) ----------------------------------------------------------------------------
    def prot_max_proteins(self) -> int:
        """The widest protein panel the two kernels below take (wider panels: the tensor formulation)."""
        return int(self.lib.mu_prot_max_proteins())

    def prot_log_moments(self, X, pseudocount: float):
        """(mean, std with ddof = 1) per column of log(X + pseudocount), f64 (include/muon_amd.h).  X: a DeviceCSR as it
        is (no densifying) or a dense [n, d] tensor, f32 / f64; pseudocount > 0."""
        n, d = (int(s) for s in X.shape)
        mean, std = self.empty((d,), torch.float64), self.empty((d,), torch.float64)
        work, wb = self._work(self.lib.mu_prot_moments_worksize(n, d), floor=8)
        if isinstance(X, DeviceCSR):
            self._launch(self.lib.mu_prot_log_moments_csr, _dt(X.values), n, d, X.indptr, X.indices, X.values,
                         float(pseudocount), mean, std, work, wb)
        else:
            assert X.is_contiguous()
            self._launch(self.lib.mu_prot_log_moments_dense, _dt(X), n, d, X, float(pseudocount), mean, std, work, wb)
        return mean, std

    def prot_dsb_fit(self, X, pseudocount: float, mean, std, resp):
        """Scaled rows and the two Gaussian-mixture fits of every cell, a wave per cell (include/muon_amd.h).
        ``resp``: uniform draws, [d, 2] (one matrix for every fit) or [n, 2, d, 2] (cell, tied | full); ``std`` None =
        mean_subtract.  Returns (scaled [n, d] f64, bgmean [n], bic [n, 2], n_iter [n, 2] int32)."""
        n, d = (int(s) for s in X.shape)
        assert mean.dtype == torch.float64 and mean.numel() == d and resp.dtype == torch.float64 and resp.is_contiguous()
        assert std is None or (std.dtype == torch.float64 and std.numel() == d)
        if resp.dim() == 2:
            assert tuple(resp.shape) == (d, 2)
            cs = ms = 0
        else:
            assert tuple(resp.shape) == (n, 2, d, 2)
            cs, ms = 4 * d, 2 * d
        scaled = self.empty((n, d), torch.float64)
        bg = self.empty((n,), torch.float64)
        bic = self.empty((n, 2), torch.float64)
        niter = self.empty((n, 2), torch.int32)
        if isinstance(X, DeviceCSR):
            self._launch(self.lib.mu_prot_dsb_fit, _dt(X.values), n, d, None, X.indptr, X.indices, X.values,
                         float(pseudocount), mean, std, resp, cs, ms, scaled, bg, bic, niter)
        else:
            assert X.is_contiguous()
            self._launch(self.lib.mu_prot_dsb_fit, _dt(X), n, d, X, None, None, None, float(pseudocount), mean, std, resp,
                         cs, ms, scaled, bg, bic, niter)
        return scaled, bg, bic, niter

    # -- muon.tl.ica (csrc/ica.hip) ----------------------------------------------------------------------------------
    _ICA_FUN = {"logcosh": 0, "exp": 1, "cube": 2}

    def ica_max_components(self) -> int:
        """The most components the fused sweep takes (more: the tensor formulation)."""
        return int(self.lib.mu_ica_max_components())

    def ica_sweep(self, Z, W, fun: str, alpha: float = 1.0, max_blocks: int = 0):
        """One fixed-point sweep of parallel FastICA (include/muon_amd.h): with y = Z[:, :k] W^T, returns
        (A = g(y)^T Z[:, :k] [k, k], gp = column sums of g'(y) [k]), f64.  Z: [n, >= k rounded up to 16] f64 with unit
        column stride; columns past k are ignored.  Two calls with the same arguments agree bit for bit."""
        n, k = int(Z.shape[0]), int(W.shape[0])
        if fun not in self._ICA_FUN:
            raise ValueError(f"fun must be one of {sorted(self._ICA_FUN)}, got {fun!r}")
        assert Z.dtype == torch.float64 and W.dtype == torch.float64 and tuple(W.shape) == (k, k) and W.is_contiguous()
        assert Z.dim() == 2 and (Z.shape[1] == 0 or Z.stride(1) == 1)
        ld = int(Z.stride(0)) if n > 1 else int(Z.shape[1])
        A, gp = self.empty((k, k), torch.float64), self.empty((k,), torch.float64)
        work, wb = self._work(
            self.lib.mu_ica_worksize(n, k, int(max_blocks)) if 1 <= k <= self.ica_max_components() else 0, floor=8)
        if min(int(Z.shape[1]), ld) < (k + 15) // 16 * 16:
            ld = int(Z.shape[1])  # (a view narrower than the padded width: the library refuses it by its ldz)
        self._launch(self.lib.mu_ica_sweep_f64, n, k, ld, Z, W, self._ICA_FUN[fun], float(alpha), A, gp, work, wb,
                     int(max_blocks))
        return A, gp

    # -- muon_amd.pp.harmony_integrate (csrc/harmony.hip) --------------------------------------------------------------
    def harmony_limits(self) -> dict:
        """The most clusters, basis columns and levels (= segments of a gram) the kernels take; everything else is the
        tensor formulation."""
        return {"clusters": int(self.lib.mu_harmony_max_clusters()), "dims": int(self.lib.mu_harmony_max_dims()),
                "levels": int(self.lib.mu_harmony_max_levels())}

    @staticmethod
    def _harmony_idx(idx, n: int, checked: bool):
        """The optional int64 list of row numbers; unless the caller has ``checked`` it, it is checked here, on the
        host, before any launch."""
        if idx is None:
            return None
        if idx.dtype != torch.int64 or idx.dim() != 1 or not idx.is_contiguous():
            raise TypeError("idx: a contiguous int64 tensor of row numbers")
        if not checked and int(idx.numel()) and not (0 <= int(idx.min()) and int(idx.max()) < n):
            raise IndexError(f"idx: a row number outside [0, {n})")
        return idx

    def harmony_gram(self, R, Z, seg_ptr, K: Optional[int] = None, idx=None, checked: bool = False):
        """``out[s] = R_s[:, :K]^T Z_s`` for every row segment (include/muon_amd.h): f64 [n_seg, kp, dp], kp and dp K
        and Z's width rounded up to 16, the padding zero.  ``seg_ptr``: HOST offsets (a sequence of n_seg + 1 ascending
        ints) into the rows, or into ``idx`` (int64 row numbers on the device) where given.  R [n, >= K] and Z [n, d]
        f64 with unit column stride; columns of R at or past K are masked by index.  Two calls agree byte for byte."""
        f64 = torch.float64
        if R.dtype != f64 or Z.dtype != f64 or R.dim() != 2 or Z.dim() != 2 or int(R.shape[0]) != int(Z.shape[0]):
            raise TypeError("R [n, >= K] and Z [n, d]: float64 tensors with the same number of rows")
        n, d = int(Z.shape[0]), int(Z.shape[1])
        K = int(R.shape[1]) if K is None else int(K)
        if (n > 1 and (R.stride(1) != 1 or Z.stride(1) != 1)) or K > int(R.shape[1]):
            raise TypeError("R and Z: unit column stride, K columns of R at the least")
        idx = self._harmony_idx(idx, n, checked)
        m = n if idx is None else int(idx.numel())
        seg = [int(v) for v in seg_ptr]
        n_seg = len(seg) - 1
        lim = self.harmony_limits()
        inside = 1 <= K <= lim["clusters"] and 1 <= d <= lim["dims"] and 1 <= n_seg <= lim["levels"]
        h_seg = (ctypes.c_int64 * max(len(seg), 1))(*seg)
        kp, dp = (K + 15) // 16 * 16, (d + 15) // 16 * 16
        out = self.empty((max(n_seg, 0), kp, dp), f64)
        work, wb = self._work(self.lib.mu_harmony_gram_worksize(m, n_seg, K, d) if inside else 0, floor=8)
        ldr = int(R.stride(0)) if n > 1 else int(R.shape[1])
        ldz = int(Z.stride(0)) if n > 1 else d
        self._launch(self.lib.mu_harmony_gram_f64, n, m, K, d, R, ldr, Z, ldz, idx, n_seg, h_seg, out, work, wb)
        return out

    def harmony_assign(self, Zc, Y, sigma, F, codes, R, idx=None, checked: bool = False) -> None:
        """The soft assignment of the cells ``idx`` (None: all), IN PLACE in R [n, >= kp] (include/muon_amd.h):
        ``R[c, :K] = rownormalise_L1(exp(-D / sigma - rowmax) * F[:, codes[c]])`` with ``D = 2 (1 - Zc Y^T)``, the columns
        K .. kp - 1 zero, every other row untouched.  Zc [n, d], Y [K, d], sigma [K], F [K, B] f64; codes int32 [n]."""
        f64 = torch.float64
        for t in (Zc, Y, sigma, F, R):
            if t.dtype != f64:
                raise TypeError("Zc, Y, sigma, F and R: float64 tensors")
        n, d, K = int(Zc.shape[0]), int(Zc.shape[1]), int(Y.shape[0])
        if (tuple(Y.shape) != (K, d) or tuple(sigma.shape) != (K,) or F.dim() != 2 or int(F.shape[0]) != K
                or not (Y.is_contiguous() and sigma.is_contiguous() and F.is_contiguous())):
            raise TypeError("Y [K, d], sigma [K] and F [K, B]: contiguous")
        if codes.dtype != torch.int32 or tuple(codes.shape) != (n,) or not codes.is_contiguous():
            raise TypeError("codes: a contiguous int32 tensor, one level per cell")
        if R.dim() != 2 or int(R.shape[0]) != n or (n > 1 and (R.stride(1) != 1 or Zc.stride(1) != 1)):
            raise TypeError("R [n, >= K rounded up to 16] and Zc [n, d]: unit column stride")
        B = int(F.shape[1])
        idx = self._harmony_idx(idx, n, checked)
        nb = n if idx is None else int(idx.numel())
        ldr = int(R.stride(0)) if n > 1 else int(R.shape[1])
        if int(R.shape[1]) < (K + 15) // 16 * 16:
            ldr = int(R.shape[1])  # (narrower than the padded width: the library refuses it by its ldr)
        ldz = int(Zc.stride(0)) if n > 1 else d
        self._launch(self.lib.mu_harmony_assign_f64, n, K, d, B, nb, Zc, ldz, Y, sigma, F, codes, idx, R, ldr)

    def harmony_objective(self, Zc, Y, R, sigma, G, codes):
        """The three terms of Harmony's objective (include/muon_amd.h) as an f64 tensor [3]: ``sum(R D)``,
        ``sum(sigma_k R log R)`` with 0 log 0 = 0 and ``sum(sigma_k R_ik G[k, codes[i]])``, ``D = 2 (1 - Zc Y^T)``, over
        the first K = Y's rows columns of R [n, >= K]; one read of R.  Two calls agree byte for byte."""
        f64 = torch.float64
        for t in (Zc, Y, R, sigma, G):
            if t.dtype != f64:
                raise TypeError("Zc, Y, R, sigma and G: float64 tensors")
        n, d, K = int(Zc.shape[0]), int(Zc.shape[1]), int(Y.shape[0])
        if (tuple(Y.shape) != (K, d) or tuple(sigma.shape) != (K,) or G.dim() != 2 or int(G.shape[0]) != K
                or not (Y.is_contiguous() and sigma.is_contiguous() and G.is_contiguous())):
            raise TypeError("Y [K, d], sigma [K] and G [K, B]: contiguous")
        if codes.dtype != torch.int32 or tuple(codes.shape) != (n,) or not codes.is_contiguous():
            raise TypeError("codes: a contiguous int32 tensor, one level per cell")
        if R.dim() != 2 or int(R.shape[0]) != n or int(R.shape[1]) < K or (n > 1 and (R.stride(1) != 1 or Zc.stride(1) != 1)):
            raise TypeError("R [n, >= K] and Zc [n, d]: unit column stride")
        out = self.empty((3,), f64)
        work, wb = self._work(self.lib.mu_harmony_objective_worksize(n), floor=8)
        ldr = int(R.stride(0)) if n > 1 else int(R.shape[1])
        ldz = int(Zc.stride(0)) if n > 1 else d
        self._launch(self.lib.mu_harmony_objective_f64, n, K, d, int(G.shape[1]), Zc, ldz, Y, R, ldr, sigma, G, codes, out,
                     work, wb)
        return out

    def harmony_correct(self, Z, R, W, seg_ptr):
        """Harmony's correction for cells sorted by level (include/muon_amd.h): returns ``(Zcorr, Zc)`` [n, d] f64 with
        ``Zcorr[c] = Z[c] - R[c, :K] @ W[g]`` for the cells c of level g, rows ``seg_ptr[g] .. seg_ptr[g + 1] - 1`` (HOST
        offsets, B + 1 ascending ints from 0 to n), and ``Zc`` its rows divided by their 2-norms.  W [B, K, d]."""
        f64 = torch.float64
        if Z.dtype != f64 or R.dtype != f64 or W.dtype != f64 or Z.dim() != 2 or R.dim() != 2 or W.dim() != 3:
            raise TypeError("Z [n, d], R [n, >= K] and W [B, K, d]: float64 tensors")
        n, d = int(Z.shape[0]), int(Z.shape[1])
        B, K = int(W.shape[0]), int(W.shape[1])
        if (int(W.shape[2]) != d or not W.is_contiguous() or int(R.shape[0]) != n or int(R.shape[1]) < K
                or (n > 1 and (R.stride(1) != 1 or Z.stride(1) != 1))):
            raise TypeError("W [B, K, d] contiguous; R and Z: n rows, unit column stride, K columns of R at the least")
        seg = [int(v) for v in seg_ptr]
        if len(seg) != B + 1:
            raise ValueError(f"seg_ptr: {B + 1} offsets for {B} levels, got {len(seg)}")
        h_seg = (ctypes.c_int64 * (B + 1))(*seg)
        Zcorr, Zc = self.empty((n, d), f64), self.empty((n, d), f64)
        ldr = int(R.stride(0)) if n > 1 else int(R.shape[1])
        ldz = int(Z.stride(0)) if n > 1 else d
        self._launch(self.lib.mu_harmony_correct_f64, n, K, d, B, Z, ldz, R, ldr, W, h_seg, Zcorr, Zc, d)
        return Zcorr, Zc

    # -- muon.atac.pp.scopen (csrc/nmf.hip) ----------------------------------------------------------------------------
    def nmf_max_components(self) -> int:
        """The most components the fused coordinate-descent sweep takes (more: the tensor formulation)."""
        return int(self.lib.mu_nmf_max_components())

    def nmf_cd_sweep(self, W, B, G, *, bscale=None, l1: float = 0.0, oscale=None, out=None, max_blocks: int = 0):
        """One coordinate-descent sweep of bounded NMF over the rows of ``W`` (include/muon_amd.h), IN PLACE: k = G's
        size, W [rows, >= k] and B [rows, >= k] f64 with unit column stride (columns past k are left alone), G [k, k]
        with the l2 term on its diagonal; the right-hand side of row i is ``B[i] * bscale[i] - l1``.  ``out`` [rows, >= k]
        receives ``oscale[i] * W[i]`` (``oscale`` None: a copy), its columns past k zero.  Returns (gram = W^T W of the
        updated factor [k, k], viol = the sum of |projected gradient| [1]).  Two calls with the same arguments agree bit
        for bit."""
        k, rows = int(G.shape[0]), int(W.shape[0])
        f64 = torch.float64
        assert W.dtype == f64 and B.dtype == f64 and G.dtype == f64 and tuple(G.shape) == (k, k) and G.is_contiguous()
        assert W.dim() == 2 and B.dim() == 2 and int(B.shape[0]) == rows
        assert (W.shape[1] == 0 or W.stride(1) == 1) and (B.shape[1] == 0 or B.stride(1) == 1)

        def ld(t):  # (a view narrower than k: the library refuses it by its leading dimension)
            return int(t.stride(0)) if rows > 1 and int(t.shape[1]) >= k else int(t.shape[1])

        for v in (bscale, oscale):
            assert v is None or (v.dtype == f64 and tuple(v.shape) == (rows,) and v.is_contiguous())
        if out is not None:
            assert out.dtype == f64 and out.dim() == 2 and int(out.shape[0]) == rows and out.is_contiguous()
        assert oscale is None or out is not None
        gram, viol = self.empty((k, k), f64), self.empty((1,), f64)
        work, wb = self._work(
            self.lib.mu_nmf_cd_worksize(rows, k, int(max_blocks)) if 1 <= k <= self.nmf_max_components() else 0, floor=8)
        self._launch(self.lib.mu_nmf_cd_sweep_f64, rows, k, W, ld(W), B, ld(B), bscale, G, float(l1), oscale, out,
                     0 if out is None else int(out.shape[1]), gram, viol, work, wb, int(max_blocks))
        return gram, viol

    # -- muon.tl.mofa with smooth_covariate (csrc/gp.hip) --------------------------------------------------------------
    @staticmethod
    def _gp_square(V, *vs):
        f64 = torch.float64
        assert V.dtype == f64 and V.dim() == 2 and V.shape[0] == V.shape[1]
        n = int(V.shape[0])
        assert n <= 1 or (V.stride(1) == 1 and V.stride(0) >= n)
        for v in vs:
            assert v.dtype == f64 and tuple(v.shape) == (n,) and v.is_contiguous() and v.device == V.device
        return n, (int(V.stride(0)) if n > 1 else n)

    def gp_project(self, V, r):
        """``V^T r`` for the n x n f64 matrix ``V`` (row-major; a row stride of n or more) and the f64 vector ``r``: one
        pass over V, every sum in the order include/muon_amd.h states - two calls agree bit for bit."""
        n, ldv = self._gp_square(V, r)
        u = self.empty((n,), torch.float64)
        work, wb = self._work(self.lib.mu_gp_project_worksize(n), floor=8)
        self._launch(self.lib.mu_gp_project_f64, n, V, ldv, r, u, work, wb)
        return u

    def gp_posterior(self, V, g, u):
        """``(V (g o u), (V o V) g)`` from one pass over the n x n f64 matrix ``V``: the posterior mean and the
        diagonal of the posterior covariance of a factor on MEFISTO's eigen route.  Two calls agree bit for bit."""
        n, ldv = self._gp_square(V, g, u)
        m, dc = self.empty((n,), torch.float64), self.empty((n,), torch.float64)
        self._launch(self.lib.mu_gp_posterior_f64, n, V, ldv, g, u, m, dc)
        return m, dc

    # -- muon_amd.rna.pp / muon_amd.tl.pca (csrc/rna.hip) --------------------------------------------------------------
    def gene_moments_max_blocks(self) -> int:
        """The workgroups ``gene_moments`` launches at most when no cap is given."""
        return int(self.lib.mu_gene_moments_max_blocks())

    def gene_moments(self, Xt: DeviceCSR, c: float = 1.0, with_e: bool = True, max_blocks: int = 0):
        """``(sums f64 [4, d], nnz int64 [d])`` of the rows of ``Xt`` (X^T as a CSR: one row per gene): sum x, sum x^2,
        sum e, sum e^2 with e = expm1(x * c) (the last two rows zero without ``with_e``) and the count of stored values
        that are not zero.  All arithmetic in f64; two calls agree bit for bit (include/muon_amd.h)."""
        d = int(Xt.shape[0])
        assert Xt.indptr.dtype == torch.int64 and int(Xt.indptr.numel()) == d + 1 and Xt.indptr.is_contiguous()
        assert Xt.values.is_contiguous()
        sums, cnt = self.zeros((4, d), torch.float64), self.empty((d,), torch.int64)
        self._launch(self.lib.mu_gene_moments, _dt(Xt.values), d, int(Xt.values.numel()), Xt.indptr, Xt.values, float(c),
                     int(bool(with_e)), sums, cnt, int(max_blocks))
        return sums, cnt

    def value_sweep(self, X: DeviceCSR, div=None, log: bool = False, log_div: float = 0.0, out=None):
        """The stored values of ``X`` through ``x / div[row]`` (``div`` f64 [n] or None), then ``log1p`` when ``log``,
        then ``/ log_div`` (ln(base); 0: natural): f64 arithmetic, one rounding to the storage type.  ``out`` may be
        ``X.values`` itself; returns the values tensor written."""
        n = int(X.shape[0])
        v = X.values
        assert X.indptr.dtype == torch.int64 and int(X.indptr.numel()) == n + 1 and X.indptr.is_contiguous()
        assert v.is_contiguous() and (div is None or (div.dtype == torch.float64 and tuple(div.shape) == (n,)
                                                      and div.is_contiguous()))
        if out is None:
            out = torch.empty_like(v)
        assert out.dtype == v.dtype and out.shape == v.shape and out.is_contiguous()
        self._launch(self.lib.mu_rna_value_sweep, _dt(v), n, int(v.numel()), X.indptr, v, out, div, int(bool(log)),
                     float(log_div))
        return out

    def shift_cols(self, Y: torch.Tensor, m: torch.Tensor) -> torch.Tensor:
        """``Y[:, j] -= float32(m[j])`` IN PLACE: Y [n, B] f32 row-major, B in {16, 32, 64}, m f64 [B]."""
        n, B = Y.shape
        assert Y.dtype == torch.float32 and Y.is_contiguous() and Y.data_ptr() % 16 == 0
        assert m.dtype == torch.float64 and tuple(m.shape) == (B,) and m.is_contiguous()
        self._launch(self.lib.mu_shift_cols_f32, int(n), int(B), Y, m)
        return Y

    def scale_rows(self, s: torch.Tensor, Q: torch.Tensor, out=None) -> torch.Tensor:
        """``out = s[:, None] * Q`` (one f32 product per element): Q [d, B] f32 row-major, B in {16, 32, 64}, s f32 [d];
        ``out`` may be ``Q``."""
        d, B = Q.shape
        if out is None:
            out = torch.empty_like(Q)
        assert Q.dtype == torch.float32 and Q.is_contiguous() and Q.data_ptr() % 16 == 0
        assert out.dtype == torch.float32 and out.shape == Q.shape and out.is_contiguous() and out.data_ptr() % 16 == 0
        assert s.dtype == torch.float32 and tuple(s.shape) == (d,) and s.is_contiguous()
        self._launch(self.lib.mu_scale_rows_f32, int(d), int(B), s, Q, out)
        return out

    # -- muon_amd.rna.pp.scale (csrc/scale.hip) ------------------------------------------------------------------------
    @staticmethod
    def _scale_tables(X: DeviceCSR, mean, std, z):
        d = int(X.shape[1])
        for t in (mean, std, z):
            assert t.dtype == torch.float64 and tuple(t.shape) == (d,) and t.is_contiguous()
        assert X.indices.dtype == torch.int32 and X.indices.is_contiguous() and X.values.is_contiguous()
        assert int(X.indices.numel()) == int(X.values.numel())
        return d

    def scale_values(self, X: DeviceCSR, mean, std, z, lo: float, hi: float, out=None) -> torch.Tensor:
        """``T(clip((x - mean[c]) / std[c], lo, hi) - z[c])`` for every stored value of ``X``: f64 arithmetic, the clip
        by comparisons, one rounding to the storage type (include/muon_amd.h).  ``mean``, ``std``, ``z``: f64 [d].
        ``out`` may be ``X.values`` itself; returns the values tensor written."""
        d = self._scale_tables(X, mean, std, z)
        v = X.values
        if out is None:
            out = torch.empty_like(v)
        assert out.dtype == v.dtype and out.shape == v.shape and out.is_contiguous()
        self._launch(self.lib.mu_scale_values, _dt(v), int(v.numel()), d, X.indices, v, out, mean, std, z, float(lo),
                     float(hi))
        return out

    def scale_dense_rows(self, X: DeviceCSR, mean, std, z, lo: float, hi: float, row_lo: int, row_hi: int,
                         out=None) -> torch.Tensor:
        """Rows [row_lo, row_hi) of the dense clipped scaled matrix as a ``[row_hi - row_lo, d]`` block of the storage
        type: ``T(z[j])`` where nothing is stored, ``T(clip((x - mean[j]) / std[j], lo, hi))`` where an entry is
        (include/muon_amd.h).  ``out``: a contiguous block of that shape to write into."""
        d = self._scale_tables(X, mean, std, z)
        n, row_lo, row_hi = int(X.shape[0]), int(row_lo), int(row_hi)
        assert X.indptr.dtype == torch.int64 and int(X.indptr.numel()) == n + 1 and X.indptr.is_contiguous()
        assert 0 <= row_lo <= row_hi <= n
        if out is None:
            out = self.empty((row_hi - row_lo, d), X.values.dtype)
        assert out.dtype == X.values.dtype and tuple(out.shape) == (row_hi - row_lo, d) and out.is_contiguous()
        self._launch(self.lib.mu_scale_dense_rows, _dt(X.values), n, d, int(X.values.numel()), row_lo, row_hi, X.indptr,
                     X.indices, X.values, mean, std, z, float(lo), float(hi), out)
        return out

    # -- muon.tl.snf (csrc/snf.hip) ----------------------------------------------------------------------------------
    def free_memory(self) -> int:
        """Bytes the device can still hand out: what the driver reports free plus what torch's allocator holds unused."""
        with self._dev_ctx():
            free, _total = torch.cuda.mem_get_info(self.device)
            held = torch.cuda.memory_reserved(self.device) - torch.cuda.memory_allocated(self.device)
        return int(free) + int(held)

    def snf_max_k(self) -> int:
        """The widest dominate set ``snf_topk`` selects (more: ``torch.topk``)."""
        return int(self.lib.mu_snf_max_k())

    def snf_affinity_max_k(self) -> int:
        """The most neighbours ``snf_affinity`` averages over (more: the tensor formulation)."""
        return int(self.lib.mu_snf_affinity_max_k())

    def snf_max_terms(self) -> int:
        """The most matrices ``snf_diffuse`` adds while it reads (more: pre-summed by the caller)."""
        return int(self.lib.mu_snf_max_terms())

    @staticmethod
    def _snf_square(t, name: str):
        """(n, leading dimension) of an n x n f64 matrix or of the n x n view of a wider buffer."""
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.float64 and t.dim() == 2 and t.shape[0] == t.shape[1]):
            raise TypeError(f"{name}: a square float64 tensor")
        n = int(t.shape[0])
        if n > 1 and (t.stride(1) != 1 or t.stride(0) < n):
            raise ValueError(f"{name}: rows must be contiguous")
        return n, (int(t.stride(0)) if n > 1 else max(n, 1))

    def snf_affinity(self, D, k: int, sigma: float, eps: float, out=None):
        """The reference's ``_affinity_matrix(D, k, sigma)`` (include/muon_amd.h); ``out`` may be D itself."""
        n, ldd = self._snf_square(D, "D")
        out = self.empty((n, n), torch.float64) if out is None else out
        n2, ldw = self._snf_square(out, "out")
        if n2 != n:
            raise ValueError("out: the shape of D")
        means = self.empty((max(n, 1),), torch.float64)
        self._launch(self.lib.mu_snf_affinity_f64, n, int(k), ldd, D, ldw, out, float(sigma), float(eps), means)
        return out

    def snf_normalize(self, X, out=None):
        """The reference's ``_normalize(X)``: symmetric bit for bit, diagonal 0.5; ``out`` may be X itself."""
        n, ldx = self._snf_square(X, "X")
        out = self.empty((n, n), torch.float64) if out is None else out
        n2, ldo = self._snf_square(out, "out")
        if n2 != n:
            raise ValueError("out: the shape of X")
        r = self.empty((max(n, 1),), torch.float64)
        self._launch(self.lib.mu_snf_normalize_f64, n, ldx, X, ldo, out, r)
        return out

    def snf_topk(self, W, k: int):
        """``(idx int32 [n, k], val f64 [n, k])``: the k largest of every row of W with their columns, descending."""
        n, ldw = self._snf_square(W, "W")
        idx = self.empty((n, int(k)), torch.int32)
        val = self.empty((n, int(k)), torch.float64)
        self._launch(self.lib.mu_snf_topk_f64, n, int(k), ldw, W, idx, val)
        return idx, val

    def snf_p_scale(self, indptr, cols, vals):
        """On the CSR of z: ``rowsum[i]`` = sum of row i in stored order; every entry (i, j) of ``vals`` is divided by
        ``rowsum[j]`` in place.  Returns ``rowsum``."""
        if indptr.dtype != torch.int64 or cols.dtype != torch.int32 or vals.dtype != torch.float64:
            raise TypeError("indptr int64, cols int32, vals float64")
        assert indptr.is_contiguous() and cols.is_contiguous() and vals.is_contiguous() and cols.numel() == vals.numel()
        n = int(indptr.numel()) - 1
        rowsum = self.empty((max(n, 1),), torch.float64)
        self._launch(self.lib.mu_snf_p_scale_f64, n, int(vals.numel()), indptr, cols, vals, rowsum)
        return rowsum[:n]

    def snf_diffuse(self, P, terms, out):
        """``out = (P X)^T``: P = ``(indptr int64, cols int32, vals f64)`` a CSR with n rows, X the mean of ``terms`` (n x n
        f64 matrices with one leading dimension, added in list order while they are read).  ``out`` is none of them."""
        indptr, cols, vals = P
        if indptr.dtype != torch.int64 or cols.dtype != torch.int32 or vals.dtype != torch.float64:
            raise TypeError("P: indptr int64, cols int32, vals float64")
        assert indptr.is_contiguous() and cols.is_contiguous() and vals.is_contiguous() and cols.numel() == vals.numel()
        n, ldy = self._snf_square(out, "out")
        if int(indptr.numel()) != n + 1:
            raise ValueError("P: one row per row of out")
        lds = set()
        for t in terms:
            nt, ld = self._snf_square(t, "term")
            if nt != n:
                raise ValueError("terms: the shape of out")
            lds.add(ld)
        if len(lds) > 1:
            raise ValueError("terms: one leading dimension")
        ptrs = (ctypes.c_void_p * max(len(terms), 1))(*[t.data_ptr() for t in terms])
        self._launch(self.lib.mu_snf_diffuse_f64, n, len(terms), ptrs, lds.pop() if lds else max(n, 1), indptr, cols, vals,
                     ldy, out)
        return out

    # -- muon.atac.tl.rank_peaks_groups (csrc/rank.hip) --------------------------------------------------------------
    def group_moments_max_groups(self) -> int:
        """The most buckets the two kernels take (more: the tensor formulation)."""
        return int(self.lib.mu_group_moments_max_groups())

    def rank_row_cap(self) -> int:
        """Rows of X^T longer than this are split over the waves of a workgroup."""
        return int(self.lib.mu_rank_row_cap())

    def _rank_args(self, Xt: DeviceCSR, labels, n_buckets: int):
        d, n = Xt.shape
        if labels.dtype != torch.int32 or int(labels.numel()) != n:
            raise TypeError("labels: int32, one per column of Xt")
        if not 1 <= int(n_buckets) <= self.group_moments_max_groups():
            raise ValueError(f"n_buckets must be 1..{self.group_moments_max_groups()}, got {n_buckets}")
        if Xt.indptr.dtype != torch.int64 or Xt.indices.dtype != torch.int32:
            raise TypeError("Xt: indptr int64, indices int32")
        return d, n, Xt.indptr.contiguous(), Xt.indices.contiguous(), Xt.values.contiguous(), labels.contiguous()

    def group_moments(self, Xt: DeviceCSR, labels, n_buckets: int):
        """``(sum f64, sumsq f64, nnz int64)``, each [d, n_buckets], of the rows of ``Xt`` (X^T as a CSR: rows are the
        features, indices the cells) per bucket of ``labels`` (int32 per cell: 0 .. n_buckets - 1, or -1 = the cell is
        left out).  ``nnz`` counts the stored values that are not zero (NaN counts).  Two calls agree bit for bit."""
        d, n, indptr, cells, values, labels = self._rank_args(Xt, labels, n_buckets)
        B = int(n_buckets)
        s, ss = self.empty((d, B), torch.float64), self.empty((d, B), torch.float64)
        cnt = self.empty((d, B), torch.int64)
        self._launch(self.lib.mu_group_moments, _dt(values), d, n, int(cells.numel()), B, indptr, cells, values, labels, s,
                     ss, cnt)
        return s, ss, cnt

    def rank_sums(self, Xt_sorted: DeviceCSR, labels, n_buckets: int):
        """``(ranksum [d, n_buckets], zero_rank [d], tie [d])``, f64, of ``Xt_sorted``: X^T as a CSR whose rows are
        sorted ascending by VALUE (indices permuted alike).  Ranks are tie-averaged over the cells with a label >= 0; the
        implicit and the stored zeros are one tie block at ``zero_rank``; ``ranksum`` covers the stored non-zero entries
        of every bucket, ``tie`` is the sum of t^3 - t over the tie blocks.  Two calls agree bit for bit."""
        d, n, indptr, cells, values, labels = self._rank_args(Xt_sorted, labels, n_buckets)
        B = int(n_buckets)
        n_kept = int((labels >= 0).sum().item())
        rs = self.empty((d, B), torch.float64)
        zr, tie = self.empty((d,), torch.float64), self.empty((d,), torch.float64)
        self._launch(self.lib.mu_rank_sums, _dt(values), d, n, int(cells.numel()), B, n_kept, indptr, cells, values, labels,
                     rs, zr, tie)
        return rs, zr, tie

    # -- muon.tl.leiden / muon.tl.louvain (csrc/cluster.hip) ---------------------------------------------------------
    def cluster_max_table(self) -> int:
        """Entries of a wave's community table in ``cluster_move``: the own community and the distinct neighbouring ones
        (a vertex with more makes the kernel report, and its level runs the tensor formulation)."""
        return int(self.lib.mu_cluster_max_table())

    def cluster_max_layers(self) -> int:
        """The most layers ``cluster_move`` scores (more: the tensor formulation)."""
        return int(self.lib.mu_cluster_max_layers())

    def cluster_move(self, verts, indptr, cols, vals, labels, bound, size, P, K, coef, only_single: bool, prop, score,
                     overflow):
        """One sub-round of the local moving (include/muon_amd.h): for every vertex of ``verts`` (int32) the proposal goes
        to ``prop[v]`` and the score of the community it names to ``score[v]``; ``overflow[0]`` becomes 1 where a vertex
        met more distinct communities than ``cluster_max_table()``.  ``bound`` may be None."""
        nv = int(labels.numel())
        L = len(coef)
        i32 = [("verts", verts), ("cols", cols), ("labels", labels), ("size", size), ("prop", prop), ("overflow", overflow)]
        if bound is not None:
            i32.append(("bound", bound))
        for name, t in i32:
            if t.dtype != torch.int32 or not t.is_contiguous():
                raise TypeError(f"{name}: a contiguous int32 tensor")
        for name, t in (("vals", vals), ("P", P), ("K", K), ("score", score)):
            if t.dtype != torch.float64 or not t.is_contiguous():
                raise TypeError(f"{name}: a contiguous float64 tensor")
        if indptr.dtype != torch.int64 or not indptr.is_contiguous() or int(indptr.numel()) != nv + 1:
            raise TypeError("indptr: a contiguous int64 tensor of nv + 1 offsets")
        if cols.numel() != vals.numel():
            raise ValueError("cols and vals: one entry each per edge")
        if tuple(P.shape) != (nv, 2 * L) or tuple(K.shape) != (nv, 2 * L):
            raise ValueError("P and K: [nv, 2 L]")
        if any(int(t.numel()) != nv for t in (size, prop, score)) or (bound is not None and int(bound.numel()) != nv):
            raise ValueError("size, prop, score and bound: one entry per vertex")
        if int(overflow.numel()) < 1:
            raise ValueError("overflow: at least one entry")
        h_coef = (ctypes.c_double * max(L, 1))(*[float(c) for c in coef])
        self._launch(self.lib.mu_cluster_move_f64, int(verts.numel()), verts, nv, int(vals.numel()), indptr, cols, vals,
                     labels, bound, size, L, P, K, h_coef, 1 if only_single else 0, prop, score, overflow)
        return prop, score

    def cluster_segsum(self, vals, ptr):
        """``out[s] = sum(vals[ptr[s]:ptr[s + 1]])`` for f64 rows [n, w] and int64 offsets [nseg + 1], in a fixed order."""
        if vals.dtype != torch.float64 or vals.dim() != 2 or not vals.is_contiguous():
            raise TypeError("vals: a contiguous float64 [n, w] tensor")
        if ptr.dtype != torch.int64 or ptr.dim() != 1 or not ptr.is_contiguous() or int(ptr.numel()) < 1:
            raise TypeError("ptr: a contiguous int64 tensor of nseg + 1 offsets")
        n, w = int(vals.shape[0]), int(vals.shape[1])
        nseg = int(ptr.numel()) - 1
        out = self.empty((nseg, w), torch.float64)
        if w == 0:
            return out
        self._launch(self.lib.mu_cluster_segsum_f64, n, nseg, w, vals, ptr, out)
        return out

    # -- muon.tl.umap (csrc/umap.hip) -----------------------------------------------------------------------------------
    def umap_max_components(self) -> int:
        """The most embedding dimensions ``umap_epoch`` has an instance for (2 and 3; others: the tensor formulation)."""
        return int(self.lib.mu_umap_max_components())

    def umap_epoch(self, indptr, cols, E, epoch: int, n_epochs: int, rate: int, a: float, b: float, gamma: float,
                   alpha_e: float, seed: int, Y_in, Y_out):
        """One epoch of the layout as a Jacobi step (include/muon_amd.h): ``Y_out = Y_in + alpha_e F(Y_in)`` over the CSR
        (``indptr`` int64 [n + 1], ``cols`` int32, ``E`` int64 periods in 2^-16 epochs); ``seed`` is taken modulo 2^64."""
        if Y_in.dim() != 2 or Y_in.shape != Y_out.shape:
            raise ValueError("Y_in and Y_out: two [n, n_components] tensors of one shape")
        n, dim = int(Y_in.shape[0]), int(Y_in.shape[1])
        for name, t in (("Y_in", Y_in), ("Y_out", Y_out)):
            if t.dtype != torch.float64 or not t.is_contiguous():
                raise TypeError(f"{name}: a contiguous float64 tensor")
        if n and Y_in.data_ptr() == Y_out.data_ptr():
            raise ValueError("Y_in and Y_out: two buffers")
        if indptr.dtype != torch.int64 or not indptr.is_contiguous() or int(indptr.numel()) != n + 1:
            raise TypeError("indptr: a contiguous int64 tensor of n + 1 offsets")
        if cols.dtype != torch.int32 or not cols.is_contiguous():
            raise TypeError("cols: a contiguous int32 tensor")
        if E.dtype != torch.int64 or not E.is_contiguous():
            raise TypeError("E: a contiguous int64 tensor")
        if cols.numel() != E.numel():
            raise ValueError("cols and E: one entry each per edge")
        self._launch(self.lib.mu_umap_epoch_f64, n, int(cols.numel()), indptr, cols, E, dim, int(epoch), int(n_epochs),
                     int(rate), float(a), float(b), float(gamma), float(alpha_e), int(seed) & 0xFFFFFFFFFFFFFFFF, Y_in, Y_out)
        return Y_out

    # -- muon.atac.tl.scan_sequences (csrc/motif.hip) ----------------------------------------------------------------
    def motif_max_len(self) -> int:
        """The longest motif the kernel takes (longer ones: the tensor formulation)."""
        return int(self.lib.mu_motif_max_len())

    def motif_tile(self) -> int:
        """Stream positions a workgroup of the scan takes per step."""
        return int(self.lib.mu_motif_tile())

    def motif_group(self) -> int:
        """Motifs per tile of the bank."""
        return int(self.lib.mu_motif_group())

    def motif_room(self, codes, offsets):
        """uint8 per stream position: valid codes from there to the next invalid one or the end of its sequence,
        capped at ``motif_max_len()``."""
        total, n_seq = int(codes.numel()), int(offsets.numel()) - 1
        if codes.dtype != torch.uint8 or offsets.dtype != torch.int64 or n_seq < 1:
            raise TypeError("codes uint8 [total], offsets int64 [n_seq + 1], n_seq >= 1")
        codes, offsets = codes.contiguous(), offsets.contiguous()
        room = self.empty((total,), torch.uint8)
        self._launch(self.lib.mu_motif_room, total, n_seq, codes, offsets, room)
        return room

    def motif_scan(self, codes, offsets, bank):
        """The hits of a packed motif bank (``MotifScanner.bank``: ``n_tiles``, ``bank`` [n_tiles, cap, 4, group] f64,
        ``tile_len`` [n_tiles], ``mlen`` / ``thr`` / ``orig`` [n_tiles * group]) in the code stream ``codes`` (uint8, 4 =
        invalid) with ``offsets`` (int64 [n_seq + 1], 0 first, ascending, ``codes.numel()`` last - the caller's
        promise): ``(sequence int32, motif int32 - the bank's ``orig`` -, position int32, score f64)`` in the kernel's
        slot order, which is the same on every call.  Count pass, exclusive scan, write pass: no atomics."""
        total, n_seq = int(codes.numel()), int(offsets.numel()) - 1
        nt, cap, group = int(bank["n_tiles"]), self.motif_max_len(), self.motif_group()
        B, tl, ml, th, og = (bank[k].contiguous() for k in ("bank", "tile_len", "mlen", "thr", "orig"))
        if tuple(B.shape) != (nt, cap, 4, group) or B.dtype != torch.float64:
            raise TypeError("bank: f64 [n_tiles, motif_max_len(), 4, motif_group()]")
        for t, dt, n in ((tl, torch.int32, nt), (ml, torch.int32, nt * group), (th, torch.float64, nt * group),
                         (og, torch.int32, nt * group)):
            if t.dtype != dt or int(t.numel()) != n:
                raise TypeError("bank: tile_len int32 [n_tiles]; mlen int32, thr f64, orig int32 [n_tiles * group]")
        room = self.motif_room(codes, offsets)
        codes, offsets = codes.contiguous(), offsets.contiguous()
        n_ptiles = -(-total // self.motif_tile())
        counts = self.empty((nt * n_ptiles,), torch.int32)
        self._launch(self.lib.mu_motif_count, total, n_seq, nt, codes, room, B, tl, ml, th, counts)
        ends = torch.cumsum(counts, 0, dtype=torch.int64)
        n_hits = int(ends[-1].item()) if ends.numel() else 0
        base = (ends - counts).contiguous()
        seq, mot, pos = (self.empty((n_hits,), torch.int32) for _ in range(3))
        score = self.empty((n_hits,), torch.float64)
        if n_hits:
            self._launch(self.lib.mu_motif_write, total, n_seq, nt, codes, room, offsets, B, tl, ml, th, og, counts, base,
                         n_hits, seq, mot, pos, score)
        return seq, mot, pos, score

    def mofa_jaakkola(self, zeta, a, b):
        """Bernoulli pseudo-data precision 2 lambda(xi), xi^2 = zeta^2 + a - b, written over ``a``."""
        assert zeta.is_contiguous() and a.is_contiguous() and b.is_contiguous() and a.shape == zeta.shape == b.shape
        self._launch(self.lib.mu_mofa_jaakkola, _dt(zeta), int(zeta.numel()), zeta, a, b, a)
        return a

    def mofa_poisson_pseudo(self, zeta, Y, kappa, mode: int):
        """Poisson pseudo-data (mode 0) / likelihood terms (mode 1) of a dense chunk, in place of zeta."""
        n, D = zeta.shape
        assert zeta.is_contiguous() and Y.is_contiguous() and Y.shape == zeta.shape and Y.dtype == zeta.dtype
        self._launch(self.lib.mu_mofa_poisson_pseudo, _dt(zeta), int(n), int(D), int(mode), zeta, Y, kappa, zeta)
        return zeta

    mofa_poisson_lik_with_b = True  # (mode 3 of mofa_poisson_pass)

    def mofa_poisson_pass(self, mode: int, E_own, E_other, kappa, X: DeviceCSR, pads: Optional[dict] = None):
        """One pass of a poisson view without anything N x D (csrc/mofa_poisson.hip, include/muon_amd.h): mode 0 ->
        a = R <W> [N, K] (E_own = <Z>, E_other = <W>, X = the view), mode 1 -> b = R^T <Z> [D, K] (E_own = <W>, E_other =
        <Z>, X = the view's transpose), mode 2 -> per-sample likelihood terms [N], mode 3 -> mode 1 with the per-feature
        likelihood terms as column K: [D, K + 1]."""
        n_own, K = E_own.shape
        n_other = E_other.shape[0]
        assert E_other.shape[1] == K and E_own.dtype == E_other.dtype and 1 <= K <= 32
        assert X.shape == (n_own, n_other) and X.values.dtype == E_own.dtype
        ld = _mofa_pad_width(K)
        E_own, E_other = _mofa_pad(E_own, "own", K, ld, pads), _mofa_pad(E_other, "other", K, ld, pads)
        blk = int(self.lib.mu_mofa_poisson_blocks_for(_dt(E_own), int(mode), K, n_own, n_other))
        nb = -(-n_other // blk)
        part = self.empty((nb, n_own) if mode == 2 else (nb, n_own, K + 1 if mode == 3 else K), E_own.dtype)
        self._launch(self.lib.mu_mofa_poisson_dense_ld, _dt(E_own), int(mode), n_own, n_other, K, ld, blk, E_own, E_other,
                     kappa, part)
        out = _sum_parts(part).contiguous()
        self._launch(self.lib.mu_mofa_poisson_sparse_ld, _dt(E_own), int(mode), n_own, K, ld, X.indptr, X.indices, X.values,
                     E_own, E_other, out)
        return out

    def mofa_softplus_sweep(self, E_own, E_other, pads: Optional[dict] = None):
        """out[own] = - sum_other ln(1 + e^zeta), zeta = <e_own> . <e_other>: the dense sweep of mofa_poisson_pass(2, ...)
        alone (the likelihood of a bernoulli view needs it without the poisson correction over the stored entries)"""
        n_own, K = E_own.shape
        n_other = E_other.shape[0]
        assert E_other.shape[1] == K and E_own.dtype == E_other.dtype and 1 <= K <= 32
        ld = _mofa_pad_width(K)
        E_own, E_other = _mofa_pad(E_own, "own", K, ld, pads), _mofa_pad(E_other, "other", K, ld, pads)
        blk = int(self.lib.mu_mofa_poisson_blocks_for(_dt(E_own), 2, K, n_own, n_other))
        nb = -(-n_other // blk)
        part = self.empty((nb, n_own), E_own.dtype)
        self._launch(self.lib.mu_mofa_poisson_dense_ld, _dt(E_own), 2, n_own, n_other, K, ld, blk, E_own, E_other, None, part)
        return _sum_parts(part)

    def mofa_jaakkola_sweep(self, E_own, E2_own, E_other, E2_other):
        """The precision-weighted moment sums of a bernoulli view without anything N x D (csrc/mofa_bernoulli.hip,
        include/muon_amd.h): out[own] = sum_other Omega(own, other) <m m^T>_other as [n_own, K, K], Omega the Jaakkola
        precision of the pair.  E / E2: first / second moments [rows, K], K <= 16."""
        n_own, K = E_own.shape
        n_other = E_other.shape[0]
        assert 1 <= K <= 16 and E_other.shape[1] == K and E_own.dtype == E_other.dtype
        args = [t.contiguous() for t in (E_own, E2_own, E_other, E2_other)]
        ldm = int(self.lib.mu_mofa_jaakkola_cols(K))
        pc = K * (K + 1) // 2
        M = self.empty((n_other, ldm), E_own.dtype)
        blk = int(self.lib.mu_mofa_jaakkola_blocks(_dt(E_own), K, n_own, n_other))
        nb = -(-n_other // blk)
        part = self.empty((nb, n_own, pc), E_own.dtype)
        self._launch(self.lib.mu_mofa_pack_moments, _dt(E_own), n_other, K, ldm, args[2], args[3], M)
        self._launch(self.lib.mu_mofa_jaakkola_sweep, _dt(E_own), n_own, n_other, K, blk, args[0], args[1], args[2], args[3],
                     M, ldm, part)
        packed = _sum_parts(part)
        idx = self._tri_index.get((K, packed.device))
        if idx is None:
            pos = {}
            for k in range(K):
                for l in range(k, K):
                    pos[(k, l)] = len(pos)
            idx = torch.tensor([pos[(min(k, l), max(k, l))] for k in range(K) for l in range(K)], dtype=torch.int64,
                               device=packed.device)
            self._tri_index[(K, packed.device)] = idx
        return packed.index_select(1, idx).view(n_own, K, K)

    def mofa_gs_update(self, Tm, b, prior, lth, l1mth, spikeslab, E, E2, gamma, Eh2, sig2):
        """Gauss-Seidel sweep over the factors of every row with row-wise K x K statistics (include/muon_amd.h);
        prior / lth / l1mth: f64 [K]."""
        n, K = E.shape
        assert Tm.is_contiguous() and b.is_contiguous() and E.is_contiguous() and E2.is_contiguous() and sig2.is_contiguous()
        self._launch(self.lib.mu_mofa_gs_update, _dt(E), int(n), int(K), Tm, b, prior, lth, l1mth, int(bool(spikeslab)), E, E2,
                     gamma, Eh2, sig2)

    def mofa_elbo_work(self, K: int) -> torch.Tensor:
        return self.empty((int(self.lib.mu_mofa_elbo_work_doubles(int(K))),), torch.float64)

    def mofa_tau_elbo(self, yy, Ngm, EW, EW2, B, Gz, Z2, a0, b0, tau, ltau, elbo, work):
        """tau / <ln tau> of one view from the sufficient statistics; adds the likelihood and tau-node
        terms to the f64 device scalar ``elbo`` (include/muon_amd.h)."""
        G, D, K = B.shape
        self._launch(self.lib.mu_mofa_tau_elbo, _dt(EW), D, K, G, yy, Ngm, EW, EW2, B, Gz, Z2, float(a0), float(b0), tau, ltau,
                     elbo, work)

    def mofa_stats_resid(self, yy, EW, EW2, B, Q, S):
        """S[d] = yy[d] - 2 <w_d> . B[d] + sum Q[d] * <w w^T>_d in f64 (include/muon_amd.h): yy, S f64 [D]; EW, EW2, B [D, K];
        Q [D or 1, K^2]"""
        D, K = EW.shape
        assert yy.dtype == torch.float64 and S.dtype == torch.float64 and yy.is_contiguous() and S.is_contiguous()
        assert EW.is_contiguous() and EW2.is_contiguous() and B.is_contiguous() and Q.is_contiguous()
        assert B.shape == (D, K) and Q.shape[1] == K * K and Q.shape[0] in (1, D) and B.dtype == EW.dtype == Q.dtype
        self._launch(self.lib.mu_mofa_stats_resid, _dt(EW), int(D), int(K), int(Q.shape[0]), yy, EW, EW2, B, Q, S)

    def mofa_tau_finish(self, S, Ngd, a0, b0, tau, ltau, elbo, work):
        """tau / <ln tau> from the expected squared residuals and counts of every (group, feature) (f64, same shape as
        tau); adds the likelihood and tau-node terms to the f64 device scalar ``elbo`` (include/muon_amd.h)."""
        assert S.dtype == torch.float64 and Ngd.dtype == torch.float64 and S.is_contiguous() and Ngd.is_contiguous()
        assert tau.is_contiguous() and ltau.is_contiguous() and tau.numel() == S.numel() == Ngd.numel() == ltau.numel()
        self._launch(self.lib.mu_mofa_tau_finish, _dt(tau), int(S.numel()), S, Ngd, float(a0), float(b0), tau, ltau, elbo, work)

    def mofa_w_elbo(self, EWh2, gamma, sig2, ard, spikeslab, a_alpha, a0, b0, th_a0, th_b0, alpha, lalpha,
                    lth, l1mth, elbo, work):
        D, K = EWh2.shape
        self._launch(self.lib.mu_mofa_w_elbo, _dt(EWh2), D, K, int(bool(ard)), int(bool(spikeslab)), EWh2, gamma, sig2,
                     float(a_alpha), float(a0), float(b0), float(th_a0), float(th_b0), alpha, lalpha, lth, l1mth, elbo, work)

    def mofa_z_sums(self, EZ2, sig2, n0, n1, out, work):
        K = EZ2.shape[1]
        self._launch(self.lib.mu_mofa_z_sums, _dt(EZ2), int(n0), int(n1), K, EZ2, sig2, out, work)

    def mofa_z_elbo(self, zs, Ng, ard, a0, b0, alpha_z, lalpha_z, elbo):
        G, _two, K = zs.shape
        self._launch(self.lib.mu_mofa_z_elbo, _dt(alpha_z), K, G, int(bool(ard)), zs, Ng, float(a0), float(b0), alpha_z,
                     lalpha_z, elbo)

    # -- synthetic data (bench / tests) ---------------------------------------------
    def synth_counts(self, row0: int, n_rows: int, n_cols: int, n_topics: int = 50,
                     density: float = 0.03, seed: int = 0) -> DeviceCSR:
        row_nnz = self.empty((n_rows,), torch.int64)
        indptr = self.empty((n_rows + 1,), torch.int64)
        self._launch(self.lib.mu_synth_row_nnz, row0, n_rows, n_cols, n_topics, density, seed, row_nnz)
        self._launch(self.lib.mu_exclusive_scan_i64, n_rows, row_nnz, indptr)
        nnz = int(indptr[-1].item())
        indices = self.empty((nnz,), torch.int32)
        values = self.empty((nnz,), torch.float32)
        self._launch(self.lib.mu_synth_fill, row0, n_rows, n_cols, n_topics, density, seed, indptr, indices, values)
        # (the generator stands where ingest stands: the slab pointers of its index arrays are made here, once)
        return self.with_slab_ptr(DeviceCSR(indptr, indices, values, (n_rows, n_cols)))


class _Fetch:
    def __init__(self, bufs, event, pool=None):
        self.bufs, self.event, self.pool = bufs, event, pool

    def wait(self):
        self.event.synchronize()
        out = [b.numpy().copy() for b in self.bufs]
        if self.pool is not None:  # the staging buffers go back to the pool (an abandoned handle keeps its own)
            for b in self.bufs:
                self.pool.setdefault((tuple(b.shape), b.dtype), []).append(b)
            self.bufs, self.pool = [], None
        return out

    def release(self):
        """Give the staging buffers back without reading them (an abandoned fetch).  Safe without waiting: the next
        copy into a buffer is queued on the same stream behind this one, and its reader waits for its own event."""
        if self.pool is not None:
            for b in self.bufs:
                self.pool.setdefault((tuple(b.shape), b.dtype), []).append(b)
            self.bufs, self.pool = [], None


_default_backend = None


def get_backend():
    """The process-wide HipBackend on the current device (raises without a GPU)."""
    global _default_backend
    if _default_backend is None or _default_backend.device.index != torch.cuda.current_device():
        _default_backend = HipBackend()
    return _default_backend


def backend_or_default(backend):
    """``backend`` if one was passed, else the process-wide one (raises without a GPU: there is no CPU path)."""
    return get_backend() if backend is None else backend
