"""muon.atac.pp.tfidf / binarize on MI355X.

Host side mirrors /root/reference/muon/_atac/preproc.py:16-152 (same signature, same
errors and warnings, same in-place write-back); the arithmetic (:92-117) runs as HIP
kernels through the C-ABI (csrc/tfidf.hip).  Extra keyword-only arguments (``comm``,
``n_obs``, ``match_scipy_order``, ``keep_on_device``) default to the reference's behaviour.
The host matrix and its device copy are _hostmatrix's (residency, canonicalisation, the takeover of a replaced matrix).
"""
from __future__ import annotations

from typing import Optional, Union
from warnings import warn

import numpy as np
from scipy.sparse import csr_matrix, issparse

from .._backend import CsrPlans, backend_or_default
from .._comm import default_comm
from .._containers import modality, view_to_actual
from .._ffi import TFIDF_LOG_IDF, TFIDF_LOG_TF, TFIDF_LOG_TFIDF
from .._hostmatrix import (DEVICE_ATTR, _copy_array, _dies_with_rebinding, _is_canonical, _is_canonical_csc,
                           _reuse_host_enabled, attach_device, resident, upload_canonical)
from .._operators import has, transposed_csr


def _flags(log_tf, log_idf, log_tfidf):
    return (TFIDF_LOG_TF if log_tf else 0) | (TFIDF_LOG_IDF if log_idf else 0) | (
        TFIDF_LOG_TFIDF if log_tfidf else 0
    )


def _effective_scale(scale_factor) -> float:
    # preproc.py:101: the multiply is skipped for None / 0 / 1
    if scale_factor is None or scale_factor == 0 or scale_factor == 1:
        return 1.0
    return float(scale_factor)


def tfidf_device(backend, X, n_obs, flags: int, scale: float, comm=None, out=None, emit_stream: bool = True):
    """Device-resident TF-IDF of a (row shard of a) CSR.  Returns a DeviceCSR that shares
    indptr / indices with ``X`` unless zeros had to be dropped.

    Pipeline: one reduction sweep (row sums, LDS-staged column sums), an all-reduce of the
    d column sums when rows are sharded, the idf vector, one fused scale pass."""
    from .._trace import phase

    comm = default_comm(comm)
    # HipBackend's sweeps hand the slab pointers they search from the sum pass to the scale pass and on to the result
    # (`keep_work`, `work`); other operator sets (CPU tests) have the plain forms only
    hands_on = has(backend, "slab_ptr_from_work")
    work = None
    with phase("tfidf/sums"):
        if hands_on:
            rowsum, colsum, work = backend.row_col_sums(X, keep_work=True)  # (work None: X came with its table)
        else:
            rowsum, colsum = backend.row_col_sums(X)
        comm.all_reduce_sum(colsum)
        idf = backend.idf(colsum, float(n_obs), flags, X.values.dtype)
    # r05: the scale sweep also writes the ROW STREAM of the result - the operand layout of lsi's products - while it has
    # every entry in registers (the layout needs the row lengths only); lsi then skips its streaming copy of X and
    # transposes from the stream.  Operator sets without the kernel (CPU tests) simply do not offer it.
    emit = sp = None
    kw = {} if work is None else {"work": work}
    with phase("tfidf/scale"):
        if emit_stream and has(backend, "can_emit_stream") and backend.can_emit_stream(X):
            emit = kw["emit"] = backend.stream_layout(X)
        vals, zero_count = backend.tfidf_scale(X, rowsum, idf, scale, flags, out=out, **kw)
        if work is not None:
            sp = backend.slab_ptr_from_work(X, work)
        del work, kw  # (the work buffer dies with the scale sweep)
    res = X.with_values(vals)
    if int(zero_count.item()) != 0:
        # scipy's SpGEMM drops entries whose product is exactly 0
        res = backend.compact_nonzero(res)
    else:
        # the result shares X's index arrays: the slab pointers the sweeps searched go with it (with the result only: X
        # keeps searching), lsi's transposition cuts the same 8192-column slabs (csrc/tpack4.hip) and does not search
        # them again.  (sp None: X came with its table, `with_values` handed it on.)
        if sp is not None:
            res.plans = CsrPlans(CsrPlans.key_of(res), slab_ptr=sp)
        if emit is not None:  # (mirrors these arrays: a result whose zeros were compacted has no stream)
            res.xstream = (emit[0], emit[1], res.values.data_ptr())
    return res


def _reverse_rows(m: csr_matrix) -> csr_matrix:
    """Emit every row in descending column order (what two scipy SpGEMMs + one sparse
    log1p leave behind for the default flags); data follows the indices."""
    indptr = m.indptr.astype(np.int64)
    nnz = m.nnz
    row_of = np.repeat(np.arange(m.shape[0], dtype=np.int64), np.diff(indptr))
    pos = np.arange(nnz, dtype=np.int64)
    perm = indptr[row_of] + (indptr[row_of + 1] - 1 - pos)
    out = csr_matrix((m.data[perm], m.indices[perm], m.indptr.copy()), shape=m.shape)
    out.has_sorted_indices = False
    return out


def tfidf(
    data,
    log_tf: bool = True,
    log_idf: bool = True,
    log_tfidf: bool = False,
    scale_factor: Union[int, float] = 1e4,
    inplace: bool = True,
    copy: bool = False,
    from_layer: Optional[str] = None,
    to_layer: Optional[str] = None,
    *,
    comm=None,
    n_obs: Optional[int] = None,
    match_scipy_order: bool = False,
    keep_on_device: bool = True,
    reuse_host: Optional[bool] = None,
    backend=None,
):
    """
    Transform peak counts with TF-IDF (Term Frequency - Inverse Document Frequency).

    TF: peak counts are normalised by total number of counts per cell
    DF: total number of counts for each peak
    IDF: number of cells divided by DF

    By default, log(TF) * log(IDF) is returned.  Signature, validation and write-back follow
    the reference (preproc.py:16-129); see the module docstring for the extra keywords.

    comm
            ``TorchDistComm`` when ``data`` holds this rank's row (cell) shard.
    n_obs
            Global number of cells when sharded (defaults to the sum over ranks).
    match_scipy_order
            Emit rows in the (descending) column order scipy's SpGEMM produces instead of
            canonical sorted CSR.
    keep_on_device
            Keep the device copy attached to the result so that ``lsi`` skips the upload.
    reuse_host
            Opt-in (default off; ``None`` reads ``MUON_AMD_REUSE_HOST=1``): when ``adata.X`` is rebound and NOTHING else
            holds a Python reference to the matrix it replaces or to its arrays, the result adopts that matrix's index
            arrays and value buffer instead of allocating 12 bytes per stored entry.  The reference never touches the
            old matrix (preproc.py:121-127) and a raw-pointer holder is invisible to reference counts: hence opt-in.
    """
    adata = modality(data, "atac")

    if log_tfidf and (log_tf or log_idf):
        raise AttributeError(
            "When returning log(TF*IDF), \
            applying neither log(TF) nor log(IDF) is possible."
        )

    if copy and not inplace:
        raise ValueError("`copy=True` cannot be used with `inplace=False`.")

    if to_layer is not None and not inplace:
        raise ValueError(f"`to_layer='{str(to_layer)}'` cannot be used with `inplace=False`.")

    if copy:
        adata = adata.copy()

    view_to_actual(adata)

    counts = adata.X if from_layer is None else adata.layers[from_layer]

    # Check before the computation
    if to_layer is not None and to_layer in adata.layers:
        warn(f"Existing layer '{str(to_layer)}' will be overwritten")

    backend = backend_or_default(backend)  # raises without a GPU: there is no CPU fallback
    comm = default_comm(comm)

    X = resident(counts, backend)  # left on the device by binarize(): no second upload
    if X is not None:
        host = counts
    elif _is_canonical_csc(counts):
        # column-compressed input (.h5ad / .h5mu files may store X that way): its arrays are the CSR
        # of the transpose, which the device turns into the CSR of X instead of a
        # single-threaded scipy tocsr() on the host
        n_r, n_c = counts.shape
        Xc = backend.upload_csr(counts.indptr, counts.indices, counts.data, (n_c, n_r))
        # f32: the tile-staged transposition of csrc/tpack4.hip (3x the rate of the general kernel)
        X = transposed_csr(backend, Xc)
        host = None
    else:
        host, X = upload_canonical(backend, counts)
    if n_obs is None:
        n_obs = comm.sum_scalar(adata.shape[0])
    flags = _flags(log_tf, log_idf, log_tfidf)
    # (the result's row stream - lsi's operand - is only worth its 8 bytes per entry when the device copy stays attached)
    R = tfidf_device(backend, X, n_obs, flags, _effective_scale(scale_factor), comm=comm,
                     emit_stream=keep_on_device and not (match_scipy_order and log_tf and not log_tfidf))

    shares = host is not None and R.indices is X.indices
    # the matrix this call replaces, when nothing else can see it (or a canonicalised temporary of this call): the
    # result takes its index arrays and is downloaded into its value array - see _dies_with_rebinding
    if shares and host is not counts:  # a canonicalised temporary (canonical_csr copies before it sorts / sums / widens)
        own = not any(np.may_share_memory(getattr(host, k), getattr(counts, k)) for k in ("data", "indices", "indptr")
                      if isinstance(getattr(counts, k, None), np.ndarray))
    else:
        own = (shares and inplace and to_layer is None and from_layer is None and not copy
               and _reuse_host_enabled(reuse_host) and _dies_with_rebinding(counts, 2))
    if own:
        want = np.dtype(np.float32) if R.values.element_size() == 4 else np.dtype(np.float64)
        buf = host.data if host.data.dtype == want else (host.data.view(want) if host.data.dtype.itemsize == want.itemsize
                                                         else None)
        vals = backend.to_host(R.values, out=buf) if buf is not None and buf.shape == (int(R.values.numel()),) else \
            backend.to_host(R.values)
        res = csr_matrix((vals, host.indices, host.indptr), shape=host.shape, copy=False)
        if host is counts:
            # the fingerprint of the device copy attached to the old matrix describes values that are gone
            try:
                delattr(counts, DEVICE_ATTR)
            except Exception:  # noqa: BLE001
                pass
    elif shares:
        vals = backend.to_host(R.values)
        res = csr_matrix((vals, _copy_array(host.indices), host.indptr.copy()), shape=host.shape)
    else:  # explicit zeros were dropped on the device, or the CSR only ever existed there
        vals = backend.to_host(R.values)
        ip = backend.to_host(R.indptr)
        if host is not None:
            ip = ip.astype(host.indptr.dtype)
        elif ip[-1] < 2**31:
            ip = ip.astype(np.int32)  # what scipy would have chosen
        res = csr_matrix((vals, backend.to_host(R.indices), ip), shape=tuple(counts.shape))
    res.has_sorted_indices = True
    if match_scipy_order and log_tf and not log_tfidf:
        res = _reverse_rows(res)
    if keep_on_device and not (match_scipy_order and log_tf and not log_tfidf):
        attach_device(res, R, backend)

    # res = np.nan_to_num(tf_idf, nan=0.0) is a no-op on sparse matrices (preproc.py:119)
    if not inplace:
        return res

    if to_layer is not None:
        adata.layers[to_layer] = res
    else:
        adata.X = res

    if copy:
        return adata


def binarize(data, *, backend=None):
    """
    Transform peak counts to the binary matrix (all the non-zero values become 1).
    Mirrors preproc.py:132-152: sparse X has its stored values set to 1 in place.
    """
    adata = modality(data, "atac")

    backend = backend_or_default(backend)
    if issparse(adata.X):
        # Sparse matrix: stored values that are non-zero become 1, in place (:148-150)
        data = adata.X.data
        if data.dtype not in (np.float32, np.float64):
            data[data != 0] = 1  # integer counts: no floating-point kernel involved
            return
        m = adata.X
        if _is_canonical(m):
            # upload the whole CSR once and leave it resident for the tfidf() that follows
            Xd = backend.upload_csr(m.indptr, m.indices, data, m.shape)
            backend.binarize_values(Xd.values)
            data[...] = backend.to_host(Xd.values)
            attach_device(m, Xd, backend)
        else:
            vals = backend.to_device(data)
            backend.binarize_values(vals)
            data[...] = backend.to_host(vals)
    else:
        # dense input is a toy-size branch in the reference too (:151-152)
        adata.X[adata.X != 0] = 1


from .scopen import scopen  # noqa: E402,F401  (atac.pp.scopen resolves here, like the reference's)
