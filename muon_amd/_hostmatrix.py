"""Where a user's scipy matrix meets its device copy.

This module owns:

  * residency: ``attach_device`` leaves a DeviceCSR with a host CSR under ``DEVICE_ATTR``, ``resident`` hands it back
    while the same backend asks and a fingerprint over every byte of the matrix still matches;
  * canonicalisation before an upload: ``canonical_csr``, ``canonical_csr_deferred``, ``upload_canonical``;
  * the two directions an operator takes: ``device_copy`` (host matrix -> device CSR, attached where the matrix is the
    caller's own) and ``host_view`` (device CSR -> host matrix that carries it);
  * the opt-in takeover of a replaced matrix's arrays (``_dies_with_rebinding`` and its calibration).

It imports nothing from the operator packages (``_atac``, ``_core``, ``_rna``, ``_prot``): they import from here, at
module top.
"""
from __future__ import annotations

import numpy as np
from scipy.sparse import csr_matrix, issparse

from ._backend import backend_or_default
from ._operators import has

DEVICE_ATTR = "_muon_amd_device"


_HASH_CHUNK = 1 << 26  # 64 MiB per task


def _digest_fn():
    """xxh3-64 when the ``xxhash`` package is there (~10 GB/s per thread), else blake2b from the
    standard library (~1 GB/s per thread; both release the GIL on large buffers).  Logged once."""
    global _DIGEST
    if _DIGEST is None:
        try:
            import xxhash

            _DIGEST = xxhash.xxh3_64_intdigest
        except ImportError:
            import hashlib
            import logging

            logging.getLogger("muon_amd").info(
                "xxhash is not installed: fingerprints of resident matrices use hashlib.blake2b (slower)")
            _DIGEST = lambda buf: int.from_bytes(hashlib.blake2b(buf, digest_size=8).digest(), "little")  # noqa: E731
    return _DIGEST


_DIGEST = None


_POOL = None


def _pool():
    """One thread pool for the host-side passes over whole matrices (hashing, copies), made once: starting threads
    costs ~12 ms each next to busy workers - r04 made a fresh 16-thread pool for every array it hashed, 0.7 s of the
    API path at 250 000 cells (scripts/probes/api_profile.py)."""
    global _POOL
    if _POOL is None:
        import os
        from concurrent.futures import ThreadPoolExecutor

        _POOL = ThreadPoolExecutor(max_workers=max(4, min(32, os.cpu_count() or 4)), thread_name_prefix="muon_amd_host")
    return _POOL


def _host_threads() -> int:
    """Cores this process may actually use: the affinity mask, capped by a cgroup CPU quota (a container with 256
    visible cores and a quota of 16 runs 64 threads slower than 16)."""
    import os

    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            n = min(n, max(1, int(int(q) / int(per))))
    except Exception:  # noqa: BLE001  (no cgroup v2 file: keep the affinity count)
        pass
    return max(1, min(n, 32))


def _native_hash():
    """libmuon_amd's multi-threaded host digest (mu_host_hash64) when the library is there; None otherwise."""
    global _NATIVE
    if _NATIVE is None:
        try:
            import ctypes as C

            from . import _ffi

            lib = _ffi.lib()
            T = _host_threads()

            def h(b):
                out = C.c_uint64(0)
                _ffi.check(lib.mu_host_hash64(b.ctypes.data, b.size, T, 0, C.byref(out)))
                return int(out.value)

            _NATIVE = h
        except Exception:  # noqa: BLE001
            _NATIVE = False
    return _NATIVE or None


_NATIVE = None


def _hash_arrays(arrays) -> tuple:
    """64-bit digests over ALL bytes of every array (xxh3: ~10 GB/s per thread; every 64 MiB chunk of every array is
    one task of the shared pool, a chunk's digests are combined in order): the price of trusting a resident copy."""
    views = [np.ascontiguousarray(a).view(np.uint8).reshape(-1) for a in arrays]
    native = _native_hash()
    if native is not None:
        # one call per array, every core of the process inside it (the Python xxhash binding holds the GIL: one core,
        # 35-39 GB/s whatever the number of threads - scripts/probes/hash_rate.py)
        return tuple(native(b) for b in views)
    digest = _digest_fn()
    tasks = [(i, o) for i, b in enumerate(views) for o in range(0, max(b.size, 1), _HASH_CHUNK)]
    if sum(b.size for b in views) <= _HASH_CHUNK:
        parts = [digest(views[i][o:o + _HASH_CHUNK]) for i, o in tasks]
    else:
        parts = list(_pool().map(lambda t: digest(views[t[0]][t[1]:t[1] + _HASH_CHUNK]), tasks))
    out = []
    for i in range(len(views)):
        mine = [p for (j, _o), p in zip(tasks, parts) if j == i]
        out.append(mine[0] if len(mine) == 1 else digest(np.asarray(mine, dtype=np.uint64).view(np.uint8)))
    return tuple(out)


def _hash_array(a: np.ndarray) -> int:
    return _hash_arrays([a])[0]


def _copy_array(a: np.ndarray) -> np.ndarray:
    """``a.copy()`` on a few threads for the index arrays of a whole experiment (6e9 int32 = 25 GB: a single-threaded
    memcpy is seconds; np.copyto releases the GIL)."""
    a = np.ascontiguousarray(a)
    if a.nbytes < (64 << 20):
        return a.copy()
    out = np.empty_like(a)
    T = 16
    cuts = [a.size * k // T for k in range(T + 1)]
    list(_pool().map(lambda k: np.copyto(out[cuts[k]:cuts[k + 1]], a[cuts[k]:cuts[k + 1]]), range(T)))
    return out


def _refs_seen(obj) -> int:
    import sys

    return sys.getrefcount(obj)


class _Box:
    pass


def _matrix_refs(m, held_by_caller: int) -> int:
    """What ``_refs_seen`` reports for ``m`` inside a callee with _dies_with_rebinding's signature (the twin the
    calibration calls: same arguments, same call path down to sys.getrefcount)."""
    return _refs_seen(m)


def _probe_call(box):
    # the calibration twin of the production call site (_atac.preproc.tfidf's `_dies_with_rebinding(counts, 2)`): the
    # matrix comes out of a container attribute into the local `counts`, `host` is a second local name for it, the
    # callee gets the local and the literal 2.  Reference counts are measured through that exact shape: keep both alike.
    counts = box.X
    host = counts
    return _matrix_refs(counts, 2), host is counts


_CALIBRATION = None


def _calibrate_refs():
    """The interpreter's own references, MEASURED on this interpreter instead of assumed (CPython 3.11+
    moves call arguments into the callee's frame without a second reference, 3.14 borrows locals - a hard-coded
    "+ 2" is one version's truth): (a) an array held by ONE container attribute, passed as an attribute lookup;
    (b) a matrix held by one container attribute and two locals of the caller, seen from a callee with
    _dies_with_rebinding's signature through the same call path.  Then the SELF-TEST of the whole decision on throw-away
    matrices: a sole owner must be taken over, a matrix with one more owner (a layer entry, a variable, a second
    matrix on the same arrays) must not.  ``ok`` False = the counts cannot be trusted here: never take over."""
    global _CALIBRATION
    if _CALIBRATION is not None:
        return _CALIBRATION
    b = _Box()
    b.x = np.empty(1)
    attr = _refs_seen(b.x)
    b.X = csr_matrix(np.eye(3, dtype=np.float32))
    matrix2, _ = _probe_call(b)
    _CALIBRATION = {"attr": attr, "matrix2": matrix2, "ok": True}  # (provisional: the self-test runs through it)

    def fresh():
        bx = _Box()
        m = csr_matrix(np.eye(4, dtype=np.float32))
        # (scipy leaves views of the constructor's arrays behind; own them like a matrix read from a file does)
        m.data, m.indices, m.indptr = m.data.copy(), m.indices.copy(), m.indptr.copy()
        bx.X = m
        m = None
        return bx

    def decide(bx):
        counts = bx.X
        host = counts
        return _dies_with_rebinding(counts, 2), host is counts

    ok = decide(fresh())[0] is True
    bx = fresh()
    bx.layers = {"counts": bx.X}            # one more owner: a layer
    ok = ok and decide(bx)[0] is False
    bx = fresh()
    keep = bx.X                              # ... a variable
    ok = ok and decide(bx)[0] is False
    keep = None
    bx = fresh()
    arr = bx.X.data                          # ... one of its arrays
    ok = ok and decide(bx)[0] is False
    arr = None
    bx = fresh()
    other = csr_matrix((bx.X.data, bx.X.indices, bx.X.indptr), shape=bx.X.shape)  # ... a second matrix on the arrays
    ok = ok and decide(bx)[0] is False
    other = None
    _CALIBRATION["ok"] = bool(ok)
    return _CALIBRATION


def _reuse_host_enabled(reuse_host) -> bool:
    """The takeover is OPT-IN (r06; it was on by default in r05): ``tfidf(..., reuse_host=True)`` or
    ``MUON_AMD_REUSE_HOST=1``.  A holder of a raw pointer into the old matrix (ctypes, a C extension, an
    ``__array_interface__`` consumer) is invisible to reference counts, and the reference never mutates the matrix it
    replaces (preproc.py:121-127): the default must not either."""
    import os

    if reuse_host is None:
        return os.environ.get("MUON_AMD_REUSE_HOST", "0") == "1"
    return bool(reuse_host)


def _dies_with_rebinding(m, held_by_caller: int) -> bool:
    """True when host CSR ``m`` and its three arrays are referenced by NOTHING but the container attribute the caller is
    about to rebind (plus ``held_by_caller`` local names of the caller): the result may then take the matrix's index
    arrays over and be downloaded into its value array - nobody holding a Python reference can observe the difference,
    and a 250 000 x 200 000 experiment saves a 6 GB copy, 12 GB of first-touch page faults and the release of the 12 GB
    it replaces (34 ms per GB on the bench host: 430 of the API path's 1090 ms, profiles/r05_api_profile.txt).
    Anything else that holds the matrix or one of its arrays - ``adata.layers["counts"] = adata.X``, a view, a variable
    of the user's - counts as a reference and turns this off.  The reference rebinds ``adata.X`` to a new matrix
    (preproc.py:121-127); an owner of the old one must keep seeing the counts.  Only reached when the caller opted in
    (_reuse_host_enabled); the expected counts are measured on this interpreter and self-tested (_calibrate_refs)."""
    if type(m) is not csr_matrix:
        return False
    cal = _calibrate_refs()
    if not cal["ok"]:
        return False
    attr = cal["attr"]
    if _refs_seen(m) != cal["matrix2"] + (held_by_caller - 2):
        return False
    for name in ("data", "indices", "indptr"):
        a = m.__dict__.get(name)
        if type(a) is not np.ndarray or not a.flags.writeable or not a.flags.c_contiguous or a.ndim != 1:
            return False
        if a.base is not None:
            # scipy's constructors leave `indices[:nnz]`-style views behind: a view of an array that owns its memory
            # and that nothing but the view refers to is as good as that array
            b = a.base
            ok = type(b) is np.ndarray and b.base is None and b.flags.owndata and b.flags.writeable
            b = None
            if not ok or _refs_seen(a.base) != attr:
                return False
        elif not a.flags.owndata:
            return False
        a = None
        if _refs_seen(getattr(m, name)) != attr:
            return False
    return True


def _fingerprint(m: csr_matrix):
    """Identity of a host CSR: shape, dtype and a hash of EVERY byte of data, indices and indptr.
    Any in-place edit between two calls - a single entry, a permuted index array - invalidates the
    resident copy (r01 sampled 2^16 values and could serve stale HBM data)."""
    return (m.shape, int(m.nnz), m.data.dtype.str, m.indices.dtype.str, m.indptr.dtype.str) + _hash_arrays(
        [m.data, m.indices, m.indptr])


def attach_device(m: csr_matrix, dev_csr, backend) -> None:
    """Remember the device-resident copy of host matrix ``m`` (binarize -> tfidf ->
    lsi pays PCIe for the upload once)."""
    try:
        setattr(m, DEVICE_ATTR, (dev_csr, backend, _fingerprint(m)))
    except Exception:  # noqa: BLE001  (objects without a __dict__)
        pass


def resident(m, backend):
    """The DeviceCSR attached to ``m`` by an earlier call if it still describes ``m``, else None."""
    if not issparse(m):
        return None
    ent = getattr(m, DEVICE_ATTR, None)
    if ent is None or ent[1] is not backend or m.format != "csr":
        return None
    if ent[2] != _fingerprint(m):
        try:
            delattr(m, DEVICE_ATTR)
        except Exception:  # noqa: BLE001
            pass
        return None
    return ent[0]


def _is_canonical(m) -> bool:
    return (issparse(m) and m.format == "csr" and m.dtype in (np.float32, np.float64)
            and m.has_canonical_format and m.has_sorted_indices)


def _is_canonical_csc(m) -> bool:
    return (issparse(m) and m.format == "csc" and m.dtype in (np.float32, np.float64)
            and m.has_canonical_format and m.has_sorted_indices)


def _flags_unknown(m) -> bool:
    """scipy caches ``has_canonical_format`` / ``has_sorted_indices`` in private attributes; a matrix that has never
    been asked (a fresh ``.copy()``, a matrix assembled from arrays) answers with a single-threaded scan of every
    entry - 0.34 s at 1.6e9 entries, inside every tfidf() call of r04."""
    return getattr(m, "_has_canonical_format", None) is None


def canonical_csr_deferred(counts):
    """``(host CSR, checked)``: like ``canonical_csr`` but a float CSR whose canonical flags scipy has not computed yet
    is handed on UNCHECKED (``checked`` False) - the caller uploads it and lets the device say in milliseconds whether
    its rows are sorted and free of duplicates (``_core.io.canonicalize``), falling back to ``canonical_csr`` if not."""
    if (issparse(counts) and counts.format == "csr" and counts.dtype in (np.float32, np.float64)
            and _flags_unknown(counts)):
        return counts, False
    return canonical_csr(counts), True


def upload_canonical(backend, counts, values_dtype=None):
    """Host matrix -> (host canonical CSR, DeviceCSR with its slab pointers)."""
    host, checked = canonical_csr_deferred(counts)
    if not checked and has(backend, "with_slab_ptr"):
        # (the one upward call of this module: a call-time import, _core.io imports this module at its top)
        from ._core.io import canonicalize

        X = backend.upload_csr(host.indptr, host.indices, host.data, host.shape, values_dtype=values_dtype,
                               slab_ptr=False)
        if canonicalize(backend, X).canonical_as_given:
            host.has_canonical_format = True  # (verified entry by entry on the device: scipy need not scan it again)
            return host, backend.with_slab_ptr(X)
        del X  # unsorted rows or duplicates: the host route (it copies, sorts and sums like scipy)
    host = canonical_csr(counts)
    return host, backend.upload_csr(host.indptr, host.indices, host.data, host.shape, values_dtype=values_dtype)


def canonical_csr(counts) -> csr_matrix:
    """Host-side *layout* normalisation before upload (no arithmetic on values):
    CSR, duplicates summed, sorted column indices, int32 indices, int64 indptr, and the
    dtype promotion the reference's first statement performs (ints -> float64)."""
    if issparse(counts):
        m = counts.tocsr()
        if m is counts and not (m.dtype in (np.float32, np.float64) and m.has_canonical_format
                                and m.has_sorted_indices):
            m = m.copy()  # sum_duplicates / sort_indices below work in place: not on the caller's arrays
        # (already canonical float CSR: returned as is, no copy - at 6e9 entries the copy alone is
        #  75 GB of host memory and a single-threaded memcpy; callers only read it)
    else:
        m = csr_matrix(np.asarray(counts))  # dense branch (:97-99,113-114) ends in CSR too
    if m.dtype not in (np.float32, np.float64):
        m = m.astype(np.float64)  # 1.0 / n_peaks is float64 and promotes integer counts
    if not m.has_canonical_format:
        m.sum_duplicates()  # also sorts
    if not m.has_sorted_indices:
        m.sort_indices()
    return m



def resident_copy(m, backend=None):
    """(DeviceCSR, backend) of the valid device copy attached to host matrix ``m``, else (None, backend).  Without a
    ``backend`` argument the copy's own backend serves: no backend is constructed for a host-only matrix."""
    ent = getattr(m, DEVICE_ATTR, None) if issparse(m) else None
    if ent is None:
        return None, backend
    be = ent[1] if backend is None else backend
    return resident(m, be), be


def device_copy(m, backend=None, *, host_route=False):
    """``(host, DeviceCSR, backend)`` for sparse ``m``: how an operator takes its matrix.  ``host`` is the CANONICAL host
    matrix the device CSR mirrors (same index arrays): ``m`` itself when it has a valid device copy (a resident copy is
    canonical) or is canonical, else a canonicalised copy.  Without a valid copy ``m`` is uploaded once, and the copy
    stays attached to ``m`` when ``host`` is ``m``.  ``host_route``: without a copy and without a ``backend`` argument
    nothing is uploaded and no backend constructed - ``(canonical_csr(m), None, None)``."""
    X, be = resident_copy(m, backend)
    if X is not None:
        return m, X, be
    if backend is None and host_route:
        return canonical_csr(m), None, None
    be = backend_or_default(be)
    host, X = upload_canonical(be, m)
    if host is m:  # (a canonicalised temporary is nobody's matrix: nothing to leave the copy with)
        attach_device(m, X, be)
    return host, X, be


def host_view(X, backend, *, data=None, indices=None, indptr=None, canonical=False):
    """The host CSR of device CSR ``X``, with ``X`` attached: how an operator gives a result back.  Arrays that already
    exist on the host are passed in and reused, the others are downloaded.  ``X`` has sorted rows (every device CSR an
    operator keeps has); ``canonical`` also vouches for the absence of duplicates."""
    arrays = [backend.to_host(t) if a is None else a
              for a, t in ((data, X.values), (indices, X.indices), (indptr, X.indptr))]
    host = csr_matrix(tuple(arrays), shape=X.shape)
    host.has_sorted_indices = True
    if canonical:
        host.has_canonical_format = True
    attach_device(host, X, backend)
    return host
