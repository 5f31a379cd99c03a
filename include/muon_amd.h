/*
 * muon_amd.h - C-ABI of libmuon_amd.so: the MI355X (gfx950) kernels behind
 *   muon.atac.pp.tfidf   (/root/reference/muon/_atac/preproc.py:16-129)
 *   muon.atac.tl.lsi     (/root/reference/muon/_atac/tools.py:29-71)
 *   muon.tl.mofa         (/root/reference/muon/_core/tools.py:290-708)
 *
 * The reference is pure Python and has no FFI of its own; the boundary a
 * maintainer binds is therefore "the scipy / mofapy2 calls those three functions
 * make".  Every entry point below names the reference statement it replaces.
 * INTEGRATION.md shows the ctypes stub that would sit in the reference.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.
 *   - every function returns 0 on success and a negative mu_status otherwise;
 *     mu_last_error() returns a thread-local description of the last failure.
 *   - pointers named d_* are DEVICE pointers (hipMalloc'd by the caller - e.g.
 *     torch tensors' data_ptr() - or obtained from mu_malloc); h_* are host.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  All
 *     kernels are launched asynchronously on it; nothing synchronises unless the
 *     comment says so.  The library keeps no global state except the error string.
 *   - CSR layout: indptr int64[n_rows+1], indices int32[nnz], values f32|f64[nnz];
 *     column indices sorted ascending inside each row where stated.
 *   - dense blocks are row-major with a fixed leading dimension ld == B columns,
 *     B in {16, 32, 64}.
 */
#ifndef MUON_AMD_H
#define MUON_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  MU_OK = 0,
  MU_ERR_ARG = -1,     /* bad argument (null pointer, unsupported B, ...) */
  MU_ERR_HIP = -2,     /* a HIP runtime call or kernel launch failed      */
  MU_ERR_NO_DEVICE = -3,
  MU_ERR_UNSUPPORTED = -4
} mu_status;

#define MU_DTYPE_F32 0
#define MU_DTYPE_F64 1

/* tfidf flag bits: the booleans of preproc.py:18-20 */
#define MU_TFIDF_LOG_TF 1
#define MU_TFIDF_LOG_IDF 2
#define MU_TFIDF_LOG_TFIDF 4

/* ---- runtime plumbing ------------------------------------------------------ */
int mu_version(void);
const char* mu_last_error(void);
int mu_device_count(int* count);
int mu_set_device(int device);
/* name (<= len-1 chars), #CUs and bytes of device memory of `device` */
int mu_device_info(int device, char* name, int len, int* n_cu, size_t* total_mem);
int mu_malloc(void** d_ptr, size_t bytes);
int mu_free(void* d_ptr);
int mu_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes, void* stream);
int mu_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes, void* stream);
int mu_memset(void* d_dst, int value, size_t bytes, void* stream);
int mu_stream_sync(void* stream);
/* 64-bit change-detecting digest of a HOST byte range on n_threads cores (16 MiB chunks, XXH64-style lanes, chunk
 * digests folded in order): the fingerprint of the API path's resident-copy check (the matrices `adata.X` that
 * /root/reference/muon/_atac/preproc.py:81-129 and tools.py:50-53 read), which a Python-level hash computes on one core. */
int mu_host_hash64(const void* h_ptr, size_t n_bytes, int n_threads, uint64_t seed, uint64_t* h_out); /* blocks the host */

/* ---- TF-IDF (preproc.py:92-119) ------------------------------------------- */
/* Bytes of scratch mu_csr_row_col_sums needs for this shape (d_work). */
size_t mu_csr_row_col_sums_worksize(int64_t n_rows, int64_t n_cols);

/* rowsum[i] = sum_j c_ij  (preproc.py:93  counts.sum(axis=1))
 * colsum[j] = sum_i c_ij  (preproc.py:106 counts.sum(axis=0))
 * One pass over (indices, values): LDS-staged per-column partial sums swept slab by
 * slab over sorted rows, wave shuffle reductions for the row sums, fixed-order final
 * reduction (bit-reproducible).  Requires sorted column indices.  Both outputs f64. */
int mu_csr_row_col_sums(int dtype, int64_t n_rows, int64_t n_cols, const int64_t* d_indptr,
                        const int32_t* d_indices, const void* d_values, double* d_rowsum,
                        double* d_colsum, void* d_work, size_t work_bytes, void* stream);

/* idf[j] = n_obs / colsum[j]; log1p if MU_TFIDF_LOG_IDF  (preproc.py:106-108), computed
 * and stored in `dtype` (f32 counts give an f32 idf in the reference).
 * n_obs is adata.shape[0] - the GLOBAL cell count when rows are sharded. */
int mu_tfidf_idf(int dtype, int64_t n_cols, double n_obs, const double* d_colsum, int flags,
                 void* d_idf, void* stream);

/* out_ij = f(c_ij) following preproc.py:93-117 in the reference's operation order:
 *   t = (1/rowsum_i)*c_ij ; t *= scale (skipped when scale is 0 or 1) ; log1p if LOG_TF ;
 *   t *= idf_j ; log1p if LOG_TFIDF.
 * Replaces the two diag x CSR SpGEMMs (scipy csr_matmat) and the sparse log1p with one
 * fused pass; arithmetic is done in the dtype of the values like the reference does.
 * d_out may alias d_values.  d_zero_count (may be NULL) receives the number of outputs
 * that are exactly 0 - entries scipy's SpGEMM would have dropped. */
int mu_tfidf_scale(int dtype, int64_t n_rows, const int64_t* d_indptr, const int32_t* d_indices,
                   const void* d_values, const double* d_rowsum, const void* d_idf, double scale,
                   int flags, void* d_out, unsigned long long* d_zero_count, void* stream);

/* The same pass walked slab by slab with the slab of idf in LDS (the per-lane idf gather of
 * mu_tfidf_scale is what bounds it); results are bit-identical.  d_work: a buffer of
 * mu_csr_row_col_sums_worksize bytes; have_slab_ptr != 0 says it is the one a preceding
 * mu_csr_row_col_sums filled for this very (d_indptr, d_indices), whose row/slab pointers are
 * then reused instead of being searched again. */
int mu_tfidf_scale_sweep(int dtype, int64_t n_rows, int64_t n_cols, const int64_t* d_indptr,
                         const int32_t* d_indices, const void* d_values, const double* d_rowsum,
                         const void* d_idf, double scale, int flags, void* d_out,
                         unsigned long long* d_zero_count, void* d_work, size_t work_bytes,
                         int have_slab_ptr, void* stream);

/* Drop stored entries whose value is exactly 0 (what csr_matmat does to explicit zeros).
 * Step 1 writes the surviving count of every row; the caller scans it into the new
 * indptr (mu_exclusive_scan_i64); step 2 compacts. */
int mu_csr_count_nonzero(int dtype, int64_t n_rows, const int64_t* d_indptr, const void* d_values,
                         int64_t* d_row_nnz, void* stream);
int mu_csr_compact_nonzero(int dtype, int64_t n_rows, const int64_t* d_indptr,
                           const int32_t* d_indices, const void* d_values,
                           const int64_t* d_new_indptr, int32_t* d_new_indices, void* d_new_values,
                           void* stream);
/* out[0]=0, out[i+1]=out[i]+in[i], i<n.  d_in and d_out must not overlap (n >= 65536 runs as a
 * three-pass chunked scan that parks the chunk sums in d_out). */
int mu_exclusive_scan_i64(int64_t n, const int64_t* d_in, int64_t* d_out, void* stream);

/* binarize (preproc.py:148-150): X.data[X.data != 0] = 1, in place (NaN != 0, so NaN -> 1;
 * explicit stored zeros stay 0). */
int mu_binarize_values(int dtype, int64_t nnz, void* d_values, void* stream);

/* ---- QC metrics and in-place filtering (muon/_core/preproc.py:675-881) ------ */
/* One sweep for the columns mu.pp.filter_var / filter_obs key on (the tutorials' `n_cells_by_counts`,
 * `n_genes_by_counts`, `total_counts` of scanpy's calculate_qc_metrics, which _filter_attr reads at
 * preproc.py:729 `subset = func(df[key].values)`):
 *   row_nnz[i] = #{j : x_ij stored and != 0}, rowsum[i] = sum_j x_ij   (int64 / f64)
 *   col_nnz[j], colsum[j]: the same per column.
 * NaN counts as non-zero, an explicitly stored zero does not.  The sweep is mu_csr_row_col_sums' (same slabs, same
 * order of additions, column partials of the workgroups reduced in fixed order, no global atomics): the sums are
 * bit-identical to that entry point's on the same matrix.  Sorted column indices inside each row, like there;
 * d_slab_ptr: mu_csr_slab_ptr's table of these index arrays, or NULL (searched into d_work).
 * d_work: mu_csr_qc_worksize(n_rows, n_cols) bytes. */
size_t mu_csr_qc_worksize(int64_t n_rows, int64_t n_cols);
int mu_csr_qc(int dtype, int64_t n_rows, int64_t n_cols, const int64_t* d_indptr, const int32_t* d_indices,
              const void* d_values, int64_t* d_row_nnz, double* d_rowsum, int64_t* d_col_nnz, double* d_colsum,
              void* d_work, size_t work_bytes, const int64_t* d_slab_ptr, void* stream);

/* The submatrix _filter_attr takes (preproc.py:782-784 `X[subset, :]` / `X[:, subset]`), both axes in one pass:
 * d_rows int64[n_keep], ascending: new row -> old row; d_col_table int32[n_cols]: old column -> new column, -1 dropped.
 *   1. mu_csr_submatrix_count: new_row_nnz[i] = surviving entries of row d_rows[i]
 *   2. the caller scans it into new_indptr (mu_exclusive_scan_i64) and allocates new_indices / new_values
 *   3. mu_csr_submatrix_fill writes them.
 * Entries keep their STORED order inside a row (nothing is sorted), explicitly stored zeros survive and values are copied
 * bit for bit - what scipy's slicing does.  Offsets are 64-bit throughout. */
int mu_csr_submatrix_count(int64_t n_rows, int64_t n_cols, int64_t n_keep, const int64_t* d_indptr,
                           const int32_t* d_indices, const int64_t* d_rows, const int32_t* d_col_table,
                           int64_t* d_new_row_nnz, void* stream);
int mu_csr_submatrix_fill(int dtype, int64_t n_rows, int64_t n_cols, int64_t n_keep, const int64_t* d_indptr,
                          const int32_t* d_indices, const void* d_values, const int64_t* d_rows,
                          const int32_t* d_col_table, const int64_t* d_new_indptr, int32_t* d_new_indices,
                          void* d_new_values, void* stream);

/* ---- fragment tools (muon/_atac/tools.py:746-1201) --------------------------- */
/* The loops of count_fragments_features (:859-878), _tss_pileup (:1044-1059) and nucleosome_signal (:1170-1180) over a
 * fragment table in device memory: five int32 columns of equal length in file order - chrom (code), start, end (BED,
 * half-open), barcode (code), score - grouped by contig and non-decreasing in start inside a contig;
 * d_chrom_ptr int64[n_contigs + 1] bounds the contigs' segments and max_len = max(end - start).
 * d_cell_of int32[n_barcodes]: barcode code -> row of the caller's object, -1 = not in it (the KeyError the
 * reference swallows).  Everything is integer arithmetic; results do not depend on the order of execution.
 *
 * mu_frag_ranges: per window (d_wchrom code, -1 = a contig the table lacks; [d_wlo, d_whi), lo < 0 read as 0) the
 * candidates start > lo - max_len && start < hi of the contig's segment, by two binary searches: rng_lo (index of the
 * first one) and rng_len.  Every fragment that tabix's fetch would yield for the window is among them. */
int mu_frag_chunk(void); /* candidates per work item of the passes below (256) */
int mu_frag_ranges(int64_t n_win, int64_t n_contigs, const int32_t* d_wchrom, const int32_t* d_wlo,
                   const int32_t* d_whi, const int64_t* d_chrom_ptr, const int32_t* d_start, int64_t max_len,
                   int64_t* d_rng_lo, int64_t* d_rng_len, void* stream);
/* The work item of the next three passes is a chunk of mu_frag_chunk() candidates of one window:
 * d_chunk_ptr int64[n_win + 1] = exclusive scan of ceil(rng_len / chunk), n_chunks its last element.  A candidate
 * passes when end > max(lo, 0) && start < hi (tabix's overlap rule) and its barcode is a cell of the caller.
 *   1. mu_frag_overlap_count: chunk_cnt[c] = passing candidates of chunk c
 *   2. the caller scans it into chunk_off int64[n_chunks + 1] (mu_exclusive_scan_i64) and allocates keys / vals
 *   3. mu_frag_overlap_emit: keys = cell * n_features + window (int64), vals = score (d_score NULL: 1), in window order
 *      and file order inside a window (wave ballot + popcount: the order is a function of the input). */
int mu_frag_overlap_count(int64_t n_win, int64_t n_chunks, const int64_t* d_chunk_ptr, const int64_t* d_rng_lo,
                          const int64_t* d_rng_len, const int32_t* d_wlo, const int32_t* d_whi, const int32_t* d_start,
                          const int32_t* d_end, const int32_t* d_barcode, const int32_t* d_cell_of, int64_t n_barcodes,
                          int64_t n_obs, int64_t* d_chunk_cnt, void* stream);
int mu_frag_overlap_emit(int64_t n_win, int64_t n_chunks, const int64_t* d_chunk_ptr, const int64_t* d_rng_lo,
                         const int64_t* d_rng_len, const int32_t* d_wlo, const int32_t* d_whi, const int32_t* d_start,
                         const int32_t* d_end, const int32_t* d_barcode, const int32_t* d_score,
                         const int32_t* d_cell_of, int64_t n_barcodes, int64_t n_obs, int64_t n_features,
                         const int64_t* d_chunk_off, int64_t* d_keys, int32_t* d_vals, void* stream);
/* tools.py:1055-1057 `mx[rowind, colind_start:colind_end] += score` as two adds into the ZEROED difference array
 * d_diff int32[n_obs, width + 1]: +score at max(start - lo, 0), -score at min(end - lo, width) (lo NOT clamped here:
 * it is the region's first position).  int32 atomics; the caller checks that n_win * max(score) fits. */
int mu_frag_pileup(int64_t n_win, int64_t n_chunks, const int64_t* d_chunk_ptr, const int64_t* d_rng_lo,
                   const int64_t* d_rng_len, const int32_t* d_wlo, const int32_t* d_whi, const int32_t* d_start,
                   const int32_t* d_end, const int32_t* d_barcode, const int32_t* d_score, const int32_t* d_cell_of,
                   int64_t n_barcodes, int64_t n_obs, int64_t width, int32_t* d_diff, void* stream);
/* Row-wise inclusive scan of the first `width` columns of d_diff in place (the pileup; column `width` is left as it
 * is) and, in the same pass, tools.py:1095-1104: d_sums int64[n_obs, 2] = (sum of the first and last flank_size columns,
 * sum of the columns center_dist .. width - center_dist). */
int mu_frag_pileup_scan(int64_t n_obs, int64_t width, int64_t flank_size, int64_t center_dist, int32_t* d_diff,
                        int64_t* d_sums, void* stream);
/* tools.py:1173-1178 over the first n_take fragments in file order into the ZEROED d_classes int32[n_obs, 2]:
 * column 0 counts end - start < free_bound, column 1 the others with end - start < mono_bound. */
int mu_frag_length_classes(int64_t n_take, const int32_t* d_start, const int32_t* d_end, const int32_t* d_barcode,
                           const int32_t* d_cell_of, int64_t n_barcodes, int64_t n_obs, int free_bound, int mono_bound,
                           int32_t* d_classes, void* stream);

/* ---- CSR transpose (device CSC copy used for X^T * Y) ----------------------- */
size_t mu_csr_transpose_worksize(int64_t n_rows, int64_t n_cols, int64_t nnz);
/* Builds the CSR of X^T: t_indptr int64[n_cols+1], t_indices int32[nnz] (row ids of X,
 * ascending inside each output row), t_values.  Stable => bit-reproducible. */
int mu_csr_transpose(int dtype, int64_t n_rows, int64_t n_cols, int64_t nnz,
                     const int64_t* d_indptr, const int32_t* d_indices, const void* d_values,
                     int64_t* d_t_indptr, int32_t* d_t_indices, void* d_t_values, void* d_work,
                     size_t work_bytes, void* stream);

/* ---- LSI building blocks (tools.py:53: the ARPACK operator of scipy svds) ---- */
/* Y[n_rows x B] = X * Q, X CSR f32, Q dense [n_cols x B] f32 row-major (ld=B).
 * The SpMM that replaces the csr_matvec / csr_matvecs calls inside svds.
 * accumulate != 0 adds into Y instead of overwriting. */
int mu_spmm_f32(int64_t n_rows, int64_t n_cols, const int64_t* d_indptr, const int32_t* d_indices,
                const float* d_values, const float* d_Q, int B, float* d_Y, int accumulate,
                void* stream);

/* X^T straight from X, cell ids ascending inside every output row - what Z = X^T Y of the iteration streams; no
 * intermediate copy: mu_tpack4_* below (csrc/tpack4.hip; r06 removed the third generation, mu_csr_tpack_*):
 *   1. mu_tpack4_count: col_nnz[c] = stored entries of column c (and keeps its per-row-block column prefixes in d_work)
 *   2. caller lays the output rows out and scans their lengths into row pointers
 *   3. mu_tpack4_fill_stream (row stream) or mu_tpack4_fill_csr with the SAME d_work
 * nnz = stored entries of X (it sizes the row blocks and tiles; pass the same value everywhere).
 * d_slab_ptr (may be NULL): the slab pointers of the SAME index arrays (mu_csr_slab_ptr) if the caller holds them.
 * Stable and free of global atomics => bit-reproducible.  Shapes mu_tpack4_supported refuses (2^31 rows, a row block
 * of 2^29 entries) take mu_csr_transpose + mu_csr_stream_fill (stable as well, slower). */

/* ---- the SpMM of the LSI iteration and its operand, the ROW STREAM (r02) --------------------------
 * Y[perm[p]][0..B-1] = row perm[p] of X times Q for every position p < n_pos (B = 16, 32 or 64): the
 * operator of scipy svds (tools.py:53; _svds.py:441-466 matvec / rmatvec) for a block of B vectors.
 *
 * Row stream: the (column int32, value f32) pairs of the matrix, 8 bytes each, row after row in
 * LAUNCH ORDER without padding - position p holds row perm[p] (perm[p] < 0: no row; perm == NULL: the
 * identity, n_pos = n_rows) at ent[sptr[p] .. sptr[p+1]), sptr int64[n_pos + 1].  The kernel gives 4
 * consecutive positions to the four 16-lane groups of a wave, K such row-sets to a wave, 16 waves
 * to a workgroup (K = mu_spmm_stream_k(n_rows)); the host sorts the rows by length and deals the
 * row-sets round robin to workgroups and waves (muon_amd/_backend.py spmm_layout), so that rows that
 * advance in lock step have similar lengths and every workgroup gets the same mix.  The 64 K rows of
 * one workgroup must span less than 4 GiB of the stream (cursors are 32-bit byte offsets).
 *   1. mu_csr_stream_len: len[p] = stored entries of row perm[p] (0 for an empty position)
 *   2. caller scans len into sptr (mu_exclusive_scan_i64) and allocates ent: 8 bytes x sptr[n_pos]
 *   3. mu_csr_stream_fill (a streaming copy), or - for X^T straight from X -
 *      mu_tpack4_count, the layout of the output rows from col_nnz, and mu_tpack4_fill_stream
 *      (inv int32[n_cols]: output row -> position) with the SAME d_work
 * Requires canonical CSR (sorted column indices, no duplicates).  The entries of a row are
 * accumulated in column order with one fmaf chain per dense column, whatever the layout =>
 * bit-reproducible and layout-independent. */
int mu_spmm_stream_k(int64_t n_rows);

/* ---- r05: the row stream of the TF-IDF result from the scale sweep, and the transposition that reads it ------------
 * mu_tfidf_scale_sweep_stream = mu_tfidf_scale_sweep for f32 values that ALSO writes the row stream of its result:
 * pair i of row r - (column int32, value f32), 8 bytes - goes to d_ent[d_row_dst[r] + i], i.e. the caller lays the
 * rows out in the launch order of mu_spmm_stream_f32 beforehand (row lengths are known before the values are) and
 * the streaming copy mu_csr_stream_fill is not needed (replaces, with the values array it still writes,
 * /root/reference/muon/_atac/preproc.py:96-117; the stream is the matvec operand of scipy svds, _svds.py:441-466).
 *
 * mu_tpack4_*: X^T as a row stream (or CSR) straight from X, fourth generation (csrc/tpack4.hip) - the bytes of
 * scipy's csr.T.tocsr() with sorted indices.  Source: the row stream of X when d_x_ent != NULL (d_x_row_dst[r] = pair index of
 * row r's first pair; d_indptr gives the row lengths) - rows are read as contiguous pairs - else the CSR arrays.
 * Row blocks are fixed row ranges (mu_tpack4_geometry: 16 waves x <= 32 rows), d_work is shared by _count and _fill,
 * d_slab_ptr: see above.  mu_tpack4_supported: 0 for shapes that take the general transposition (2^31 rows, a
 * row block of 2^29 entries).  mu_tpack4_status reads the fill's error word (0 = fine; synchronises: tests). */
int mu_tfidf_scale_sweep_stream(int64_t n_rows, int64_t n_cols, const int64_t* d_indptr, const int32_t* d_indices,
                                const float* d_values, const double* d_rowsum, const float* d_idf, double scale,
                                int flags, float* d_out, unsigned long long* d_zero_count, void* d_work,
                                size_t work_bytes, int have_slab_ptr, const int64_t* d_slab_ptr,
                                const int64_t* d_row_dst, void* d_ent, void* stream);
/* The slab pointers of a CSR (first entry of every row at or behind every 8192-column boundary; int64[n_rows *
 * (ceil(n_cols / 8192) + 1)]) depend on the index arrays alone, which do not change between ingest, binarize, tfidf
 * and lsi: built ONCE where the device CSR is made (upload, 10x ingest) instead of searched by every tfidf call (26
 * binary searches per row at 200 000 columns: 3.0 ms of a 1e6-cell step).  The _sp entries take the table
 * (mu_tfidf_scale_sweep_stream and mu_tpack4_count have a d_slab_ptr argument of their own);
 * NULL = search as before.  Replaces nothing in the reference by itself: bookkeeping of preproc.py:92-117's kernels. */
int mu_csr_slab_ptr(int64_t n_rows, int64_t n_cols, const int64_t* d_indptr, const int32_t* d_indices, int64_t* d_sp,
                    void* stream);
/* ... for slabs of `width` columns (int64[n_rows * (ceil(n_cols / width) + 1)]): entries per (row, slab) of the sliced-ELL
 * operand of MOFA's sparse views (mu_spmm_ell16_*; 1024 / 512 columns) without a histogram over every entry */
int mu_csr_slab_ptr_width(int64_t n_rows, int64_t n_cols, int64_t width, const int64_t* d_indptr,
                          const int32_t* d_indices, int64_t* d_sp, void* stream);
int mu_csr_row_col_sums_sp(int dtype, int64_t n_rows, int64_t n_cols, const int64_t* d_indptr,
                           const int32_t* d_indices, const void* d_values, double* d_rowsum, double* d_colsum,
                           void* d_work, size_t work_bytes, const int64_t* d_slab_ptr, void* stream);
int mu_tfidf_scale_sweep_sp(int dtype, int64_t n_rows, int64_t n_cols, const int64_t* d_indptr,
                            const int32_t* d_indices, const void* d_values, const double* d_rowsum, const void* d_idf,
                            double scale, int flags, void* d_out, unsigned long long* d_zero_count,
                            const int64_t* d_slab_ptr, void* stream);
int mu_tpack4_supported(int64_t n_rows, int64_t n_cols, int64_t nnz);
int mu_tpack4_geometry(int64_t n_rows, int64_t n_cols, int64_t nnz, int64_t* rows_per_block, int* n_blocks,
                       int* tile_cols);
size_t mu_tpack4_worksize(int64_t n_rows, int64_t n_cols, int64_t nnz);
int mu_tpack4_count(int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t* d_indptr, const int32_t* d_indices,
                    int64_t* d_col_nnz, void* d_work, size_t work_bytes, const int64_t* d_slab_ptr, void* stream);
int mu_tpack4_fill_stream(int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t* d_indptr,
                          const int32_t* d_indices, const float* d_values, const int64_t* d_x_row_dst,
                          const void* d_x_ent, const int64_t* d_sptr, const int32_t* d_inv, void* d_ent, void* d_work,
                          size_t work_bytes, void* stream);
int mu_tpack4_fill_csr(int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t* d_indptr, const int32_t* d_indices,
                       const float* d_values, const int64_t* d_x_row_dst, const void* d_x_ent,
                       const int64_t* d_t_indptr, int32_t* d_t_indices, float* d_t_values, void* d_work,
                       size_t work_bytes, void* stream);
int mu_tpack4_status(const void* d_work, int64_t n_rows, int64_t n_cols, int64_t nnz, int* h_err);
/* byte offset of that error word (an int32) inside d_work, for callers that read it with a fetch of their own instead of
 * synchronising (lsi reads it with its first Gram fetch and raises if the transposition tripped an invariant) */
size_t mu_tpack4_err_offset(int64_t n_rows, int64_t n_cols, int64_t nnz);
/* byte offset inside d_work of the count pass' prefix table uint32 cnt[n_blocks + 1][n_cols] (cnt[g][c] = entries of column
 * c in the row blocks before g; mu_tpack4_geometry gives the rows per block): where the cells of a row-block range begin
 * inside every row of X^T - the table of mu_spmm_stream_ranges_f32 for the warm start's X_S^T Y_S */
size_t mu_tpack4_cnt_offset(int64_t n_rows, int64_t n_cols, int64_t nnz);
int mu_tpack4_phase_cycles(unsigned long long* h_out6, int reset);
/* The table-driven fill of lsi's hot path (csrc/tperm.hip): X^T's row stream from the row stream of X, the same bytes as
 * mu_tpack4_fill_stream writes, with every entry's staging slot and every row block's tile schedule taken from a plan
 * that depends on the index arrays alone (tune "tperm_off" = 1 in the Python layer: the old fill).
 *   The CSR must be canonical: column indices strictly increasing inside every row (mu_tpack4_* assume the same).
 *   mu_tperm_plan, count pass (d_tile_off = NULL): d_ntile[n_blocks] <- tiles of every row block (n_blocks from
 *     mu_tpack4_geometry; tile_cols = widest tile, 16 .. 512).  The caller scans them: d_tile_off[n_blocks + 1], [0] = 0.
 *   mu_tperm_plan, record pass (d_tile_off given, same tile_cols): d_tiles[T + n_blocks] (T = d_tile_off[n_blocks]; block
 *     g's tile boundaries at d_tile_off[g] + g, closed by n_cols), d_cont[16 T] (per tile and wave: the rows with a
 *     continuation window), d_slots[nnz] (per pair of X's row stream - d_x_row_dst[r] = first pair of row r - its
 *     slot in the staging buffer of its tile, < mu_tperm_stage_pairs()).
 *   mu_tperm_fill: d_cdst[c] = first pair of column c's row in the target stream, d_cnt = the count pass' prefix table
 *     (mu_tpack4_cnt_offset inside the work buffer of mu_tpack4_count); d_x_ent 256-byte aligned. */
int mu_tperm_stage_pairs(void);
int mu_tperm_plan(int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t* d_indptr, const int32_t* d_indices,
                  const int64_t* d_x_row_dst, int tile_cols, const int64_t* d_tile_off, int32_t* d_ntile,
                  int32_t* d_tiles, uint32_t* d_cont, uint16_t* d_slots, void* stream);
int mu_tperm_fill(int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t* d_indptr, const int64_t* d_x_row_dst,
                  const void* d_x_ent, const int64_t* d_cdst, const void* d_cnt, const int64_t* d_tile_off,
                  const int32_t* d_tiles, const uint32_t* d_cont, const uint16_t* d_slots, void* d_ent, void* stream);
/* mu_tperm_fill through the PHASE ACCOUNTING instance of its kernel (probes: scripts/probes/tperm_phases.py): the same
 * bytes in d_ent, and d_phases[16 n_blocks][8] <- per (row block, wave) the shader cycles spent in the six phases of a
 * tile, summed over the block's tiles - [0] top wait, [1] header scan, [2] staging, [3] retire + window issue,
 * [4] barrier, [5] write-out - then [6] the block's tiles and [7] 0.  The stamps cost cycles of their own. */
int mu_tperm_fill_phases(int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t* d_indptr,
                         const int64_t* d_x_row_dst, const void* d_x_ent, const int64_t* d_cdst, const void* d_cnt,
                         const int64_t* d_tile_off, const int32_t* d_tiles, const uint32_t* d_cont,
                         const uint16_t* d_slots, void* d_ent, unsigned long long* d_phases, void* stream);
/* The same fill with a FLAT READ-IN (csrc/tflat.hip; tune "tperm_flat" = 1 in the Python layer): the plan also records how
 * many pairs of every row fall into every tile, and lane i of a wave reads the wave's pair i of the tile - no windows.
 * Same bytes in d_ent as mu_tperm_fill and mu_tpack4_fill_stream.  Its tile rule is its own: a tile ends at the widest
 * column bound (<= tile_cols) at which every wave's pairs are <= 64 mu_tflat_rounds() and the block's pairs are
 * <= mu_tperm_stage_pairs(); otherwise the width is halved (a multiple of 16, at least 16).
 *   mu_tflat_plan: the two passes of mu_tperm_plan.  The record pass writes d_counts[512 T] instead of d_cont -
 *     d_counts[(tile * 16 + wave) * 32 + l] = pairs of row l of the wave in the tile, uint16 - and d_slots[nnz] for ITS
 *     tiles.  d_err (int32[1], zeroed by the caller) is set to 1 by either pass if a row is not canonical (a count
 *     past the tile's width): the plan must then be dropped.
 *     d_slots is laid out in the order the fill READS it, not by stream position: a wave's rows are consecutive CSR
 *     rows, and the CSR range [d_indptr[first row of the wave], ...) holds the wave's slots tile after tile; inside a
 *     tile, slot number P_r + k belongs to pair k of row r's pairs in the tile (P_r: the exclusive prefix of the
 *     tile's counts over the wave's rows), so lane l reads slot 64 u + l in round u.  The slot VALUES are those of
 *     mu_tperm_plan's.  d_x_row_dst is not read by either pass (it may be NULL); the fill needs it and d_indptr.
 *   mu_tflat_fill / mu_tflat_fill_phases: as mu_tperm_fill / mu_tperm_fill_phases with d_counts for d_cont; d_x_ent needs
 *     no alignment beyond its pairs'.  Phase [3] is the scan of the counts, the row search and the issue of the loads. */
int mu_tflat_rounds(void);
int mu_tflat_plan(int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t* d_indptr, const int32_t* d_indices,
                  const int64_t* d_x_row_dst, int tile_cols, const int64_t* d_tile_off, int32_t* d_ntile,
                  int32_t* d_tiles, uint16_t* d_counts, uint16_t* d_slots, int* d_err, void* stream);
int mu_tflat_fill(int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t* d_indptr, const int64_t* d_x_row_dst,
                  const void* d_x_ent, const int64_t* d_cdst, const void* d_cnt, const int64_t* d_tile_off,
                  const int32_t* d_tiles, const uint16_t* d_counts, const uint16_t* d_slots, void* d_ent, void* stream);
int mu_tflat_fill_phases(int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t* d_indptr,
                         const int64_t* d_x_row_dst, const void* d_x_ent, const int64_t* d_cdst, const void* d_cnt,
                         const int64_t* d_tile_off, const int32_t* d_tiles, const uint16_t* d_counts,
                         const uint16_t* d_slots, void* d_ent, unsigned long long* d_phases, void* stream);
int mu_csr_stream_len(int64_t n_pos, const int32_t* d_perm, const int64_t* d_indptr, int64_t* d_len,
                      void* stream);
int mu_csr_stream_fill(int64_t n_pos, const int32_t* d_perm, const int64_t* d_indptr,
                       const int32_t* d_indices, const float* d_values, const int64_t* d_sptr,
                       void* d_ent, void* stream);
/* B = 64 / 32: k_spmm_win (csrc/spmm_win.hip).  B = 16: k_spmm_narrow (csrc/spmm_narrow.hip: 16 stored entries x 4
 * columns per wave step) - the DEFAULT kernel of every 16-column product on a row stream: lsi with n_comps <= 2, the
 * neighbourhood means of mu.pp.neighbors on embeddings of <= 16 dimensions, MOFA f32 views whose operand is not laid
 * out as sliced ELL (tests/test_gpu_kernels.py runs it against scipy at B = 16).  MOFA's default for <= 16 stacked
 * factor columns is mu_spmm_ell16_* below. */
int mu_spmm_stream_f32(int64_t n_pos, int64_t n_cols, const int64_t* d_sptr, const void* d_ent,
                       const int32_t* d_perm, int k_layout, const float* d_Q, int B, float* d_Y,
                       void* stream);
/* The same row stream (f32 stored values) against an f64 dense block, f64 accumulation and product,
 * B = 16 / 32: mofapy2's default precision (tools.py:308 use_float32=False).  accumulate != 0 adds to
 * d_Y - an f64-valued matrix is the sum of two f32-valued ones (v = fl32(v) + fl32(v - fl32(v)), exact
 * to 2^-48), i.e. two streams and two launches; data that is exact in f32 (counts) needs one. */
/* r06 - the products of lsi's SUBSAMPLED WARM START (muon_amd/_atac/tools.py; the reference has no counterpart: its
 * ARPACK run, /root/reference/muon/_atac/tools.py:53, starts from a random vector) without operands of their own:
 * mu_spmm_stream_ranges_f32 is mu_spmm_stream_f32 (B = 64) restricted to a list of <= 32 column ranges (narrower
 * blocks, B = 16 / 32, are zero-padded to 64 columns by the callers: HipBackend.spmm_slice / spmm_slice_t).  h_ranges5 holds
 * {col0, col1, q_off, ta, tb} per range: the entries of position p's row in columns [col0, col1)
 * are pairs d_sptr[p] + d_tbl[ta * tbl_stride + row] .. d_sptr[p] + d_tbl[tb * tbl_stride + row] (row = d_perm[p], or p),
 * column c multiplies row c - col0 + q_off of d_Q (q_rows x 64).  Workgroup (x, y) walks ranges [y per_wg, (y + 1) per_wg)
 * and writes its partial product to d_Y + y * y_stride (elements): the caller sums the ceil(n_ranges / per_wg) partials in
 * fixed order.  X_S^T Y_S: the row stream of X^T as it is, d_tbl = the transposition's count prefixes
 * (mu_tpack4_cnt_offset), one range per run of row blocks, per_wg = n_ranges.  X_S Q: mu_csr_slice_stream's compact
 * stream of the slice's rows, ranges = 8192-column super-slabs, per_wg = 1 .. (the column slabs split over the chip).
 * mu_csr_slice_stream: the (column, value) pairs of <= 32 ranges of consecutive rows of a CSR, range after range, rows in
 * their own order (h_row0 / h_rows: the ranges; h_lo / h_hi: d_indptr at their ends, known to the host), d_sptr
 * int64[n_s + 1], d_rel uint32[(ceil(n_cols / 8192) + 1) * n_s] from the CSR's slab pointers (mu_csr_slab_ptr). */
int mu_csr_slice_stream(int n_ranges, const int64_t* h_row0, const int64_t* h_rows, const int64_t* h_lo,
                        const int64_t* h_hi, int64_t n_cols, const int64_t* d_indptr, const int32_t* d_indices,
                        const float* d_values, const int64_t* d_slab_ptr, int64_t* d_sptr, void* d_ent, uint32_t* d_rel,
                        void* stream);
int mu_spmm_stream_ranges_f32(int64_t n_pos, const int64_t* d_sptr, const void* d_ent, const int32_t* d_perm,
                              int k_layout, const float* d_Q, int64_t q_rows, float* d_Y, int64_t y_stride,
                              const uint32_t* d_tbl, int64_t tbl_stride, int n_ranges, const int32_t* h_ranges5,
                              int per_wg, void* stream);
int mu_spmm_stream_f64(int64_t n_pos, int64_t n_cols, const int64_t* d_sptr, const void* d_ent,
                       const int32_t* d_perm, int k_layout, const double* d_Q, int B, double* d_Y,
                       int accumulate, void* stream);
/* r08 - the width of the Q slabs as an argument.  mu_spmm_stream_f32 / mu_spmm_stream_ranges_f32 sweep the columns in
 * slabs of 256 (2 x 64 KiB of LDS at B = 64); the B = 64 kernels for K >= 6 row-sets per wave also exist with slabs of
 * 320 columns (2 x 80 KiB: all of a gfx950 CU's LDS), which pays the per-pass costs of a (row-set, slab) 20 % less often.
 * A row's entries are accumulated in column order whatever the width: the products are bit-identical.
 * slab_cols = 256: the entries above.  slab_cols = 320: an error unless B = 64 and the K in effect (k_layout, or the
 * tune key "spmm_k") is 6, 7 or 8.  Any other width is an error.  mu_spmm_stream_slab_ok: 1 if (B, K, slab_cols) has an
 * instance, else 0.  The host decides (HipBackend.spmm_slab; tune key "spmm_slab": 0 decide, 256 / 320 force). */
int mu_spmm_stream_slab_ok(int B, int K, int slab_cols);
int mu_spmm_stream_slab_f32(int64_t n_pos, int64_t n_cols, const int64_t* d_sptr, const void* d_ent,
                            const int32_t* d_perm, int k_layout, const float* d_Q, int B, float* d_Y,
                            int slab_cols, void* stream);
int mu_spmm_stream_ranges_slab_f32(int64_t n_pos, const int64_t* d_sptr, const void* d_ent, const int32_t* d_perm,
                                   int k_layout, const float* d_Q, int64_t q_rows, float* d_Y, int64_t y_stride,
                                   const uint32_t* d_tbl, int64_t tbl_stride, int n_ranges, const int32_t* h_ranges5,
                                   int per_wg, int slab_cols, void* stream);


/* ---- narrow-block SpMM on a sliced-ELL operand (r04; csrc/spmm_ell.hip) -------------------------------------
 * Y[n, 16] = X Q for the <= 16-column factor blocks of MOFA's sparse views (A = Y (tau o W), B = Y^T Z: the Z / W node
 * updates of mofapy2's ent.run(), /root/reference/muon/_core/tools.py:583-585), on an operand laid out once per fit:
 * positions in launch order (d_perm[p] = row at position p, -1 none), 16 positions = a group = the rows of one wave,
 * columns in slabs of 1024.  The entries of (group, slab) are steps - one entry of each of the 16 rows, padded to the
 * longest row - stored as windows of 4 steps (384 bytes: value[64] f32, then offset[64] u16; slot 4 r + j = row r's
 * step 4 w + j, offset = byte offset of the Q row inside the slab = column % 1024 * 64; padding = (0.0, 0)).
 * A group's windows are contiguous from d_wave_base[group], slab after slab; d_hdr[group][slab] is the number of
 * windows.  d_ent needs eight windows of slack (the kernel reads that far ahead).  A workgroup = `waves` (1 .. 15)
 * consecutive groups plus one wave that copies the Q slabs; mu_spmm_ell16_waves picks it for a row count so that
 * full rounds of workgroups cover the chip - it is a launch parameter, not part of the layout. */
int mu_spmm_ell16_waves(int64_t n_rows);
int mu_spmm_ell16_f32(int waves, int64_t n_pos, int64_t n_cols, const int32_t* d_hdr, const int64_t* d_wave_base,
                      const void* d_ent, const int32_t* d_perm, const float* d_Q, float* d_Y, void* stream);
/* The same operand format against an f64 block (f64 products and sums; mofapy2's default precision): Q rows are 128
 * bytes, so the slabs are 512 columns and offset = column % 512 * 128.  Stored values stay f32 - an f64-valued matrix
 * is two operands, hi = fl32(v) and lo = fl32(v - hi), and two launches, the second with accumulate != 0. */
int mu_spmm_ell16_f64(int waves, int64_t n_pos, int64_t n_cols, const int32_t* d_hdr, const int64_t* d_wave_base,
                      const void* d_ent, const int32_t* d_perm, const double* d_Q, double* d_Y, int accumulate,
                      void* stream);
/* r06: the same two products with the column slabs split into `parts` over blockIdx.y - part y writes its partial product
 * to d_Y + y * y_stride (elements), the caller sums the partials in order - for operands of a few thousand rows (one rank's
 * shard of a sharded mu.tl.mofa fit, /root/reference/muon/_core/tools.py:583-585): every workgroup otherwise pulls all of Q
 * through its LDS.  mu_spmm_ell16_parts: the (waves, parts) to launch with (parts = 1: the plain entries). */
int mu_spmm_ell16_parts(int64_t n_rows, int64_t n_cols, int wide, int* waves, int* parts);
int mu_spmm_ell16_parts_f32(int waves, int parts, int64_t n_pos, int64_t n_cols, const int32_t* d_hdr,
                            const int64_t* d_wave_base, const void* d_ent, const int32_t* d_perm, const float* d_Q,
                            float* d_Y, int64_t y_stride, void* stream);
int mu_spmm_ell16_parts_f64(int waves, int parts, int64_t n_pos, int64_t n_cols, const int32_t* d_hdr,
                            const int64_t* d_wave_base, const void* d_ent, const int32_t* d_perm, const double* d_Q,
                            double* d_Y, int64_t y_stride, void* stream);

/* The layout itself: the windows of a canonical f32 CSR from its slab pointers of the operand's width
 * (mu_csr_slab_ptr_width(slab_cols): d_slab_ptr[row][0 .. S]).  d_perm / d_hdr / d_win_base[group][slab] (first window
 * of every (group, slab): the exclusive scan of d_hdr) as the product reads them, made by the caller from the slab
 * pointers (rows by descending length, the longest row of a group per slab).  Writes every slot of every window
 * (padding included); the eight windows of slack behind them are the caller's to zero. */
int mu_ell16_fill(int64_t n_groups, int64_t n_cols, int64_t nnz, int slab_cols, const int32_t* d_indices, const float* d_values,
                  const int64_t* d_slab_ptr, const int32_t* d_perm, const int32_t* d_hdr, const int64_t* d_win_base,
                  void* d_ent, void* stream);


/* Tune keys (tests, probes and bench only; process-global; every default is what ships).  The keys, their defaults, largest
 * accepted values and meanings are declared once, in csrc/common.hpp (MU_TUNE_KEYS); INTEGRATION.md lists them.
 * mu_tune_set fails on a NULL or unknown key ("unknown key"), a negative value and a value above the key's largest;
 * mu_tune_get of a NULL or unknown key returns -1.  mu_tune_count / mu_tune_name(i) / mu_tune_default(i) list the table
 * (host only; i out of range: NULL / -1). */
int mu_tune_set(const char* key, int value);
int mu_tune_get(const char* key);
int mu_tune_count(void);
const char* mu_tune_name(int i);
int mu_tune_default(int i);

/* Same product in f64 (MOFA runs in float64 unless use_float32=True, tools.py:308). */
int mu_spmm_f64(int64_t n_rows, int64_t n_cols, const int64_t* d_indptr, const int32_t* d_indices,
                const double* d_values, const double* d_Q, int B, double* d_Y, int accumulate,
                void* stream);

size_t mu_gram_worksize(int64_t n_rows, int B);
/* G[B x B] (f64) = A^T A and colsum[B] (f64) = 1^T A for A [n_rows x B] f32 (ld=B).
 * f64 MFMA (v_mfma_f64_16x16x4_f64), fixed-order reduction. Replaces the dense QR of
 * svds (_svds.py:513) together with mu_dense_apply_f32 (CholeskyQR). */
int mu_gram_f32(int64_t n_rows, int B, const float* d_A, double* d_G, double* d_colsum,
                void* d_work, size_t work_bytes, void* stream);

/* C[B x B] (f64) = A^T Bm for A, Bm [n_rows x B] f32 (ld = B); same work buffer size as mu_gram_f32.
 * Feeds the stopping rule of lsi (angle between the Ritz subspaces of consecutive iterations). */
int mu_gram_cross_f32(int64_t n_rows, int B, const float* d_A, const float* d_Bm, double* d_C,
                      void* d_work, size_t work_bytes, void* stream);

/* Out[n_rows x B] = A[n_rows x B] * M[B x B] + bias[B] (bias may be NULL); f32 MFMA
 * (v_mfma_f32_16x16x4_f32).  Out may alias A. */
int mu_dense_apply_f32(int64_t n_rows, int B, const float* d_A, const float* d_M,
                       const float* d_bias, float* d_Out, void* stream);
/* Z[n_rows x B] -= A[n_rows x B] * C[B x B] with C in f64 as mu_gram_cross_f32 leaves it (rounded to
 * f32 for the MFMA): one block of the Gram-Schmidt projection that keeps a new Krylov block
 * orthogonal to the basis (the reorthogonalisation inside ARPACK's dsaupd, tools.py:53). */
int mu_dense_project_out_f32(int64_t n_rows, int B, const float* d_A, const double* d_C, float* d_Z,
                             void* stream);

/* M[B x B] (f32) = R^-1, upper triangular, zero outside the leading w x w block, for G = R^T R (f64,
 * B x B, B <= 64): the small step of CholeskyQR on the device (one wave, LDS resident) instead of two
 * host round trips.  A pivot that is not safely positive sets *d_flag to 1 (never cleared here) and is
 * clamped: the output stays finite, the caller redoes the step on the host. */
int mu_chol_rinv_f64(int B, int w, const double* d_G, float* d_M, int* d_flag, void* stream);

/* standard normal fill, counter based (seed, element index) -> reproducible */
int mu_randn_f32(int64_t count, uint64_t seed, float* d_out, void* stream);

/* ---- MOFA+: the two passes over a DENSE view per iteration (tall-skinny products on the matrix cores)
 * Y [n_rows x D] row-major with leading dimension ldY (a row range of the view); the factor blocks are
 * zero padded to 16 columns.  Replace the library GEMMs of the dense views (tools.py:583-585 ->
 * mofapy2's Y W / Y^T Z products); both stream Y exactly once.
 *   nn: out[n_rows x 16] = Y * T,  T [D x 16]            (Z update:  A = Y (tau o <W>))
 *   tn: C[D x 16] = Y^T * Z,       Z [n_rows x 16]       (W / tau / ELBO:  B = Y^T <Z>) */
size_t mu_skinny_tn_worksize(int dtype, int64_t n_rows, int64_t D);
int mu_skinny_nn(int dtype, int64_t n_rows, int64_t D, int64_t ldY, const void* d_Y, const void* d_T,
                 void* d_out, void* stream);
int mu_skinny_tn(int dtype, int64_t n_rows, int64_t D, int64_t ldY, const void* d_Y, const void* d_Z,
                 void* d_C, void* d_work, size_t work_bytes, void* stream);
/* The same two products in f64 with Y STORED in f32 (r04): a dense view whose values are exact in f32 - AnnData's
 * default dtype, tools.py:308 converts to float64 for the default use_float32=False - streams half the bytes and is
 * widened in registers; every product and sum is the f64 one.  (work: mu_skinny_tn_worksize(MU_DTYPE_F64, ..).) */
int mu_skinny_nn_f64_f32(int64_t n_rows, int64_t D, int64_t ldY, const float* d_Y, const double* d_T, double* d_out,
                         void* stream);
int mu_skinny_tn_f64_f32(int64_t n_rows, int64_t D, int64_t ldY, const float* d_Y, const double* d_Z, double* d_C,
                         void* d_work, size_t work_bytes, void* stream);

/* ---- MOFA+ coordinate updates (tools.py:585 ent.run(): mofapy2's W and Z node updates) ---- */
/* Spike-and-slab + ARD update of the weights of ONE view, one thread per feature, Gauss-Seidel
 * over the K factors.  Inputs are the sufficient statistics of the current factors:
 *   B[G][D][K] = Y_g^T <Z_g>, tau[G][D], Gz[G][K][K] = <Z_g>^T <Z_g>, Z2[G][K] = sum_n <z_nk^2>,
 *   alpha[K] = <alpha_k>, lth[K] = <ln theta_k>, l1mth[K] = <ln(1-theta_k)>.
 * In/out EW[D][K]; out EW2 = <w^2>, gamma = q(s=1), EWh2 = <w_hat^2>, sig2 = slab variance. */
int mu_mofa_update_w(int dtype, int64_t D, int K, int G, const void* d_B, const void* d_tau,
                     const void* d_Gz, const void* d_Z2, const void* d_alpha, const void* d_lth,
                     const void* d_l1mth, int spikeslab, void* d_EW, void* d_EW2, void* d_gamma,
                     void* d_EWh2, void* d_sig2, void* stream);
/* Update of the factors, one thread per sample.  A[M][N][K] = Y_m (tau_g o <W_m>) (row n uses its
 * own group's tau), pres[M][N] in {0,1} (sample observed in view m), grp[N] group id,
 * Gw[M][G][K][K] = <W>^T diag(tau_g) <W>, dw2[M][G][K] = sum_d tau_gd <w_dk^2>, alphaz[G][K],
 * corr[M][G][K] (nullable): subtracted from A per (view, group) - mu_g^T (tau_g o <W>), the implicit
 * centring of a sparse view.  In/out EZ[N][K]; out EZ2 = <z^2>, sig2 = posterior variance. */
int mu_mofa_update_z(int dtype, int64_t N, int K, int M, int G, const void* d_A, const void* d_pres,
                     const int32_t* d_grp, const void* d_Gw, const void* d_dw2, const void* d_alphaz,
                     const void* d_corr, void* d_EZ, void* d_EZ2, void* d_sig2, void* stream);

/* The K x K statistics of a factor / weight block E[R][K] (second moments E2) in one pass over rows
 * r0 .. r1-1 (csrc/mofa_stats.hip; mofapy2 recomputes the same moments inside its node updates,
 * tools.py:585): with a row weight w (nullable = 1) and an auxiliary row weight a (nullable = 1), both
 * indexed by the absolute row,
 *   pad[r][col0 + k] = (scale_out ? w_r : 1) E[r][k]   (leading dimension ld; nullable; the other columns
 *                      are the caller's - zero padding is written once by the caller)
 *   out_t[k][r]      = the same value, transposed with leading dimension ld_t (nullable)
 *   gram[i][j] = sum_r w_r E[r][i] E[r][j],  s2[k] = sum_r w_r E2[r][k],  s1[k] = sum_r a_r w_r E[r][k]
 * (each nullable).  W side: w = tau_g, a = the feature means of a sparse view -> tau o <W>, Gw, dw2 and the
 * centring correction; Z side: w = the presence mask -> <Z>, Gz, sum <z^2>, sum <z>.  f64 accumulation,
 * fixed-order reduction.  d_work: mu_mofa_rowstats_work_doubles(K) doubles. */
size_t mu_mofa_rowstats_work_doubles(int K);
int mu_mofa_rowstats(int dtype, int64_t r0, int64_t r1, int K, const void* d_E, const void* d_E2,
                     const void* d_wgt, const void* d_aux, int scale_out, void* d_out_pad, int ld, int col0,
                     void* d_out_t, int64_t ld_t, void* d_gram, void* d_s2, void* d_s1, double* d_work,
                     void* stream);

/* Per-feature moments of rows r0 .. r1-1 of a dense row-major view Y[.][D] (f32 / f64 storage, f64 sums) in one pass:
 * partial[chunk][0][j] = sum y_rj, partial[chunk][1][j] = sum y_rj^2 over the chunk's rows, `chunks`
 * (mu_dense_col_moments_chunks(rows, D); <= 65535) chunks of consecutive rows, folded by the caller in a fixed order.
 * The group means mofapy2 centres a view by before training (kept as the intercepts,
 * /root/reference/muon/_core/tools.py:283-286) and the sum of squares behind the noise update. */
int mu_dense_col_moments_chunks(int64_t n_rows, int64_t D);
int mu_dense_col_moments(int dtype, int64_t r0, int64_t r1, int64_t D, const void* d_Y, int chunks,
                         double* d_partial, void* stream);

/* ---- exhaustive nearest-neighbour search, the filter pass (replaces the n x n distance panels + radix top-k
 * of the tensor formulation behind muon.pp.neighbors, /root/reference/muon/_core/preproc.py:366-373,453-461,
 * 525-533, where the reference calls UMAP's approximate NN-descent).  For every query q < n_q and every
 * candidate position c in [c_lo, c_hi) with |x_q - y_c|^2 = sqq[q] + sqc[c] - 2 x_q . y_c < thr[q] and
 * c != self_pos[q]: append (c, that squared distance) to the query's buffer, rows of `cap` entries; cnt[q] =
 * number of candidates that passed (may exceed cap: the caller then redoes the query).  Xq [n_q x p_pad],
 * Xc [>= c_hi x p_pad] row-major f64, zero-padded to p_pad (a multiple of 4) columns. */
int mu_knn_filter_f64(int64_t n_q, int64_t c_lo, int64_t c_hi, int p_pad, const double* d_Xq, const double* d_Xc,
                      const double* d_sqq, const double* d_sqc, const double* d_thr, const int32_t* d_self_pos,
                      int cap, int32_t* d_buf_pos, double* d_buf_d, int32_t* d_cnt, void* stream);
/* The merge after a filter pass (r04): for every query the kc smallest (distance, position) pairs of its list [kc] and
 * the first min(cnt, cap) buffer entries, ascending, ties by position, and d_thr = the kc-th distance - what the
 * reference's NN-descent keeps per point as its heap (pynndescent behind /root/reference/muon/_core/preproc.py:366-373,
 * 517-523).  kc + cap <= 1024; not in place.  A row with cnt > cap is the caller's to redo. */
int mu_knn_merge_f64(int64_t n_q, int kc, int cap, const double* d_cur_d, const int64_t* d_cur_p, const double* d_buf_d,
                     const int32_t* d_buf_pos, const int32_t* d_cnt, double* d_out_d, int64_t* d_out_p, double* d_thr,
                     void* stream);

/* ---- kernel bandwidths of muon.pp.neighbors (/root/reference/muon/_core/preproc.py:400-472): csigma[i] = mean
 * Euclidean distance from cell i to the n_bw cells whose neighbour sets overlap its own least (but do), ties
 * towards the larger distance, i.e. the n_bw smallest keys N (1 - jaccard distance) + (bbox - euclid) / bbox
 * (:53-77), ties by cell number.  g_*: the kNN graph (CSR pattern, int64 row pointers, int32 columns), r_*: its
 * transpose; X [n x p] f64 row-major, p <= 256.  NaN for a cell without candidates; *d_overflow = 1 when a
 * cell's candidate list exceeds 8192 entries (repetitions included) - the caller then uses its tensor formulation;
 * n_bw <= 64. */
int mu_wnn_bandwidth_f64(int64_t n, int p, const double* d_X, const int64_t* d_g_indptr, const int32_t* d_g_indices,
                         const int64_t* d_r_indptr, const int32_t* d_r_indices, int n_bw, double bbox,
                         double* d_csigma, int32_t* d_overflow, void* stream);

/* ---- MOFA+ with element-wise precisions (non-gaussian likelihoods, NaN entries): one Gauss-Seidel sweep over
 * the K factors of every row r with the row's own statistics T[r] (K x K) and b[r] (K), tools.py:585 -> mofapy2's
 * W / Z node updates:  t = b_k - sum_{j != k} E_j T_kj,  prec = T_kk + prior_k,  sigma2 = 1 / prec,  mu = t sigma2,
 * gamma = sigmoid(lth_k - l1mth_k + (ln prior_k - ln prec + t^2 sigma2) / 2) (1 without spike-and-slab),
 * E_k = gamma mu,  E2_k = gamma (mu^2 + sigma2),  Eh2_k = E2_k + (1 - gamma) / prior_k.  d_gamma / d_Eh2 nullable
 * (sample rows).  f64 arithmetic, storage type `dtype`. */
int mu_mofa_gs_update(int dtype, int64_t n, int K, const void* d_T, const void* d_b, const double* d_prior,
                      const double* d_lth, const double* d_l1mth, int spikeslab, void* d_E, void* d_E2,
                      void* d_gamma, void* d_Eh2, void* d_sig2, void* stream);

/* ---- UMAP connectivities of a fixed-degree neighbour table (scanpy's `umap` method behind sc.pp.neighbors /
 * mu.pp.neighbors, preproc.py:615-622): per row rho (first positive distance), sigma by 64 bisection steps towards
 * sum_{j >= 1} exp(-max(d_j - rho, 0) / sigma) = target (= log2 n_neighbors), floors, then val[r][j] = 0 for the row
 * itself, 1 where d <= rho, exp(-(d - rho) / sigma) elsewhere.  dist [n x k] f64 (rounded to f32 inside, as umap),
 * idx [n x k] int64, mean_all = the table's mean distance. */
int mu_umap_strengths_f64(int64_t n, int k, const double* d_dist, const int64_t* d_idx, double target, double mean_all,
                          double* d_val, void* stream);

/* Rows [r0, r1) of a CSR (int64 row pointers, int32 columns, values of `dtype`) as a dense row-major chunk
 * d_out [(r1 - r0) x D]: zero fill and scatter in one pass (the chunk walks of the element-wise-precision MOFA
 * engine: zeros are data for a count likelihood, tools.py:117-141 densifies whole modalities on the host). */
int mu_csr_densify_rows(int dtype, int64_t r0, int64_t r1, int64_t D, const int64_t* d_indptr,
                        const int32_t* d_indices, const void* d_values, void* d_out, void* stream);

/* Bernoulli pseudo-data precision of a dense chunk (mofapy2's Bernoulli node, Jaakkola bound): out = 2 lambda(xi) =
 * tanh(xi / 2) / (2 xi) with xi^2 = max(zeta^2 + a - b, 0), xi >= 1e-8; n elements, arithmetic in the storage type. */
int mu_mofa_jaakkola(int dtype, int64_t n, const void* d_zeta, const void* d_a, const void* d_b, void* d_out,
                     void* stream);

/* Poisson pseudo-data of a dense chunk of predictions zeta [n_rows x D] (mofapy2's Poisson node, Seeger bound):
 * rate = softplus(zeta) clamped away from 0;  mode 0: out = kappa_d zeta - sigmoid(zeta) (1 - y / rate);
 * mode 1: out = y ln(rate) - rate.  Element-wise, arithmetic in the storage type `dtype`; d_out may alias d_zeta. */
int mu_mofa_poisson_pseudo(int dtype, int64_t n_rows, int64_t D, int mode, const void* d_zeta, const void* d_Y,
                           const void* d_kappa, void* d_out, void* stream);

/* A poisson view WITHOUT anything of size N x D (r04, csrc/mofa_poisson.hip): for y = 0 an element of the pseudo-data
 * depends on (z_n, w_d) only, so a pass = a dense sweep over all (n, d) that reads just the two K-column blocks, plus a
 * correction over the stored entries.  mode 0: own = samples, other = features, out[n][k] = sum_d R[n, d] w_dk (the Z
 * update's a = R <W>);  mode 1: own = features, other = samples, out[d][k] = sum_n R[n, d] z_nk (the W update's b = R^T
 * <Z>), kappa indexed by own;  mode 2: out[n] = sum_d y ln(rate) - rate (the likelihood term);  mode 3 (r05): mode 1 and
 * the likelihood term in one sweep, rows of K + 1 values: out[d][0 .. K-1] as mode 1, out[d][K] = sum_n y ln(rate) - rate
 * (d_part [..][n_own][K + 1]) - the ELBO pass of an iteration and the W update of the next read the same factors.  R, rate as in
 * mu_mofa_poisson_pseudo.  E_own [n_own x KP], E_other [n_other x KP] row-major with the K <= 32 columns PADDED with zeros
 * to KP = 4 / 8 / 12 / 16 / 32 (the smallest of these >= K; 16-byte aligned rows); outputs have K columns.
 * mu_mofa_poisson_dense writes PARTIAL results for column blocks of `other_block` rows of the other block
 * (mu_mofa_poisson_blocks_for(dtype, mode, K, n_own, n_other) picks it - r06: from the occupancy of the kernel those
 * arguments select, so that the workgroups fill whole rounds; mu_mofa_poisson_blocks is r04's kernel-blind rule, kept
 * for callers of that release; any multiple of 128 is valid): d_part [ceil(n_other / other_block)][n_own][K] (mode 2: [..][n_own]),
 * to be added in block order; mu_mofa_poisson_sparse ADDS the stored entries' terms to the summed result: (indptr,
 * indices, values) = CSR of the view for modes 0 / 2, of its transpose for mode 1. */
int64_t mu_mofa_poisson_blocks(int64_t n_own, int64_t n_other);
int64_t mu_mofa_poisson_blocks_for(int dtype, int mode, int K, int64_t n_own, int64_t n_other);
int mu_mofa_poisson_dense(int dtype, int mode, int64_t n_own, int64_t n_other, int K, int64_t other_block,
                          const void* d_E_own, const void* d_E_other, const void* d_kappa, void* d_part, void* stream);
int mu_mofa_poisson_sparse(int dtype, int mode, int64_t n_own, int K, const int64_t* d_indptr, const int32_t* d_indices,
                           const void* d_values, const void* d_E_own, const void* d_E_other, void* d_out, void* stream);
/* r06: the same two with an explicit row stride `ld` (in elements) of BOTH factor blocks: a multiple of 4, at least the
 * padded width above; columns K .. ld - 1 zero.  With 9 <= K <= 16 and ld = 16 (64-byte rows of f32) the stored-entry pass
 * reads a row with ONE cache-line look-up - four lanes per entry, k_pois_sparse_quad - instead of three (the look-up rate
 * of the gathers is what bounds it), while the dense sweep still runs its KP = 12 instance for K <= 12. */
int mu_mofa_poisson_dense_ld(int dtype, int mode, int64_t n_own, int64_t n_other, int K, int ld, int64_t other_block,
                             const void* d_E_own, const void* d_E_other, const void* d_kappa, void* d_part,
                             void* stream);
int mu_mofa_poisson_sparse_ld(int dtype, int mode, int64_t n_own, int K, int ld, const int64_t* d_indptr,
                              const int32_t* d_indices, const void* d_values, const void* d_E_own, const void* d_E_other,
                              void* d_out, void* stream);

/* A bernoulli view WITHOUT anything of size N x D (r06, csrc/mofa_bernoulli.hip; mofapy2's Bernoulli node with the Jaakkola
 * bound, reached from /root/reference/muon/_core/tools.py:583-585): the data enter through R = y - 1/2 and the likelihood
 * only (sparse products and the poisson likelihood sweep, mode 2 above), the precision Omega_nd = tanh(xi / 2) / (2 xi),
 * xi^2 = zeta^2 + sum_k (<z_k^2><w_k^2> - <z_k>^2 <w_k>^2), depends on the two factor blocks alone.  The sweep:
 *   out[own][c] = sum_other Omega(own, other) M_other[c],   c over the pc = K (K + 1) / 2 distinct entries of <m m^T>
 * (own = features, other = samples, M = packed <z z^T>: the W update's T;  own = samples, other = features, M = packed
 * <w w^T>: the Z update's S).  E / E2 [rows x K] row-major (first / second moments, stride K), M_other [n_other x ldm] from
 * mu_mofa_pack_moments (k <= l row-major, the diagonal = second moments, zero padded; ldm = mu_mofa_jaakkola_cols(K)),
 * 1 <= K <= 16.  Partial results for column blocks of `other_block` rows (mu_mofa_jaakkola_blocks picks it):
 * d_part [ceil(n_other / other_block)][n_own][pc], to be added in block order.  f32 and f64 on the matrix cores. */
int mu_mofa_jaakkola_cols(int K);
int mu_mofa_pack_moments(int dtype, int64_t n, int K, int ldm, const void* d_E, const void* d_E2, void* d_M,
                         void* stream);
int64_t mu_mofa_jaakkola_blocks(int dtype, int K, int64_t n_own, int64_t n_other);
int mu_mofa_jaakkola_sweep(int dtype, int64_t n_own, int64_t n_other, int K, int64_t other_block, const void* d_E_own,
                           const void* d_E2_own, const void* d_E_other, const void* d_E2_other, const void* d_M_other,
                           int ldm, void* d_part, void* stream);

/* ---- MOFA+ small nodes and the ELBO, fused (tools.py:585 ent.run(): mofapy2's Tau, AlphaW, ThetaW,
 * AlphaZ node updates and calculateELBO()).  Arithmetic in f64 for both storage types; every entry
 * ADDS its ELBO terms to the device scalar *d_elbo.  d_work: mu_mofa_elbo_work_doubles(K) doubles. */
size_t mu_mofa_elbo_work_doubles(int K);
/* tau node of one view and the likelihood term.  yy[G][D] = sum_n (y - mean)^2 over the observed
 * samples of the group, Ngm[G] their number, EW / EW2[D][K], B[G][D][K], Gz[G][K][K], Z2[G][K] as
 * in mu_mofa_update_w.  Out tau[G][D] = <tau>, ltau[G][D] = <ln tau>. */
int mu_mofa_tau_elbo(int dtype, int64_t D, int K, int G, const void* d_yy, const void* d_Ngm,
                     const void* d_EW, const void* d_EW2, const void* d_B, const void* d_Gz,
                     const void* d_Z2, double a0, double b0, void* d_tau, void* d_ltau, double* d_elbo,
                     double* d_work, void* stream);
/* r06, for views whose statistics are per FEATURE (a dense gaussian view with missing entries in the general engine): the
 * expected squared residual S[d] = yy[d] - 2 <w_d> . B[d] + sum_kl Q[d][k, l] <w w^T>_d[k, l] (Q [q_rows x K^2], q_rows = D
 * or 1 = the same block for every feature; <w w^T>[k, k] = <w_k^2>) in f64, and the node's finish for n = G x D (group,
 * feature) pairs with their own f64 counts: a = a0 + N / 2, b = b0 + S / 2, tau = a / b, <ln tau> = psi(a) - ln b, the
 * likelihood and tau-node terms ADDED to *d_elbo (work: mu_mofa_elbo_work_doubles).  Between the two the caller sums S and
 * N over the ranks. */
int mu_mofa_stats_resid(int dtype, int64_t D, int K, int64_t q_rows, const double* d_yy, const void* d_EW,
                        const void* d_EW2, const void* d_B, const void* d_Q, double* d_S, void* stream);
int mu_mofa_tau_finish(int dtype, int64_t n, const double* d_S, const double* d_Ngd, double a0, double b0, void* d_tau,
                       void* d_ltau, double* d_elbo, double* d_work, void* stream);
/* ARD precision (ard != 0: alpha[K], lalpha[K] = <ln alpha>) and sparsity level (spikeslab != 0:
 * lth[K] = <ln theta>, l1mth[K] = <ln(1 - theta)>) of one view's weights from EWh2, gamma, sig2
 * [D][K] (outputs of mu_mofa_update_w), and the ELBO terms of the W, alpha_w and theta nodes.
 * a_alpha = a0 + D / 2; (th_a0, th_b0): the Beta prior of theta. */
int mu_mofa_w_elbo(int dtype, int64_t D, int K, int ard, int spikeslab, const void* d_EWh2,
                   const void* d_gamma, const void* d_sig2, double a_alpha, double a0, double b0,
                   double th_a0, double th_b0, void* d_alpha, void* d_lalpha, void* d_lth, void* d_l1mth,
                   double* d_elbo, double* d_work, void* stream);
/* d_out[0][K] = sum_n <z_nk^2>, d_out[1][K] = sum_n ln sig2_nk over the rows [n0, n1) (one group's
 * samples on this rank; the caller adds the ranks up), then with zs[G][2][K] and the group sizes
 * Ng[G] (f64): the ARD precision of the factors (ard != 0: alpha_z, lalpha_z [G][K]) and the ELBO
 * terms of the Z and alpha_z nodes. */
int mu_mofa_z_sums(int dtype, int64_t n0, int64_t n1, int K, const void* d_EZ2, const void* d_sig2,
                   double* d_out, double* d_work, void* stream);
int mu_mofa_z_elbo(int dtype, int K, int G, int ard, const double* d_zs, const double* d_Ng, double a0,
                   double b0, void* d_alpha_z, void* d_lalpha_z, double* d_elbo, void* stream);

/* ---- muon.prot.pp.dsb (/root/reference/muon/_prot/preproc.py:161-198; csrc/prot.hip, C-ABI v700) ---------------------
 * mu_prot_max_proteins(): the widest panel the CSR moments kernel and the fit kernel take (1024: 16 values per lane).
 *
 * Log-moments of the empty droplets: d_mean[j], d_std[j] (ddof = 1) of log(x + pseudocount) over the n rows, f64, from
 * the CSR as it is (canonical rows: sorted, no duplicates) or from a dense row-major matrix.  Zeros are accounted for in
 * closed form, the sums are centred on log(pseudocount) (> 0 required; 0 is the caller's dense two-pass expression).
 * dtype f32: the logarithm is rounded to f32 first, as numpy does for a float32 matrix.  d_work: mu_prot_moments_worksize
 * bytes (partial sums of fixed row ranges, added in order: two runs agree bit for bit). */
int mu_prot_max_proteins(void);
size_t mu_prot_moments_worksize(int64_t n, int64_t d);
int mu_prot_log_moments_csr(int dtype, int64_t n, int64_t d, const int64_t* d_indptr, const int32_t* d_indices,
                            const void* d_values, double pseudocount, double* d_mean, double* d_std, void* d_work,
                            size_t work_bytes, void* stream);
int mu_prot_log_moments_dense(int dtype, int64_t n, int64_t d, const void* d_X, double pseudocount, double* d_mean,
                              double* d_std, void* d_work, size_t work_bytes, void* stream);
/* The per-cell fit, one wave per cell: the row (d_X dense [n x d], or d_X = NULL and a CSR) becomes
 * (log(x + pseudocount) - mean_j) / std_j (d_std NULL: no division; dtype f32: rounded to f32 where numpy does), is
 * written to d_scaled [n x d] f64, and gets scikit-learn's 2-component GaussianMixture EM (init_params "random", tol 1e-3,
 * reg_covar 1e-6, max_iter 100) for covariance_type "tied" and "full" in f64.  d_resp: the uniform draws [d x 2] of the
 * initial responsibilities of cell c and model m (0 tied, 1 full) at d_resp + c * resp_cell_stride + m * resp_model_stride
 * (doubles; both 0: one matrix for every fit, what an integer random_state means).  Out: d_bgmean [n] = the smaller
 * component mean of the model with the lower BIC, d_bic [n x 2], d_niter [n x 2] (n_iter_).  1 <= d <= 1024. */
int mu_prot_dsb_fit(int dtype, int64_t n, int64_t d, const void* d_X, const int64_t* d_indptr, const int32_t* d_indices,
                    const void* d_values, double pseudocount, const double* d_mean, const double* d_std,
                    const double* d_resp, int64_t resp_cell_stride, int64_t resp_model_stride, double* d_scaled,
                    double* d_bgmean, double* d_bic, int32_t* d_niter, void* stream);

/* ---- muon.tl.ica: one fixed-point sweep of parallel FastICA (/root/reference/muon/_core/tools.py:1365-1386 hands the
 * arithmetic to scikit-learn's FastICA; csrc/ica.hip, C-ABI v801) --------------------------------------------------------
 * d_Z [n x ldz] row-major f64: the whitened data, k components in columns 0 .. k - 1 (ldz >= kp = k rounded up to a
 * multiple of 16, ldz even, d_Z 16-byte aligned; columns k .. ldz - 1 are read and ignored, whatever they hold).
 * d_W [k x k] row-major.  With y_ij = sum_c Z[i][c] W[j][c]  (i < n; j, c < k):
 *     d_A[j][c] = sum_i g(y_ij) Z[i][c]        [k x k] row-major
 *     d_gp[j]   = sum_i g'(y_ij)               [k]
 *   fun 0 (logcosh): t = tanh(alpha y), g = t, g' = alpha (1 - t^2)
 *   fun 1 (exp):     e = exp(-y^2 / 2), g = y e, g' = (1 - y^2) e
 *   fun 2 (cube):    g = y^3, g' = 3 y^2
 * all in f64 on the matrix cores, Z read once.  No float atomics: every workgroup leaves its partial sums in its slot of
 * d_work (mu_ica_worksize bytes) and a second kernel adds the slots in order - two calls agree bit for bit.  The grid is
 * min(ceil(n / 64), max_blocks) workgroups (max_blocks 0: 512).  1 <= k <= mu_ica_max_components() = 64; n = 0 gives zeros. */
int mu_ica_max_components(void);
size_t mu_ica_worksize(int64_t n, int k, int max_blocks);
int mu_ica_sweep_f64(int64_t n, int k, int64_t ldz, const double* d_Z, const double* d_W, int fun, double alpha,
                     double* d_A, double* d_gp, void* d_work, size_t work_bytes, int max_blocks, void* stream);

/* ---- muon.atac.tl.rank_peaks_groups: per-group statistics of every peak (scanpy's rank_genes_groups under
 * /root/reference/muon/_atac/tools.py:337-373; csrc/rank.hip, C-ABI v802) ------------------------------------------------
 * Both take X^T as a CSR (d rows = peaks, d_cells = the cell of every entry, n_cells columns) and d_labels [n_cells]:
 * 0 .. n_buckets - 1 is the cell's bucket, -1 leaves the cell out entirely.  1 <= n_buckets <= mu_group_moments_max_groups()
 * = 64.  Outputs are [d x n_buckets] row-major, written once; no atomics: two calls agree bit for bit.  A row longer than
 * mu_rank_row_cap() entries is split over the four waves of its workgroup and the pieces are joined in piece order.
 * n_cells < 2^31, and no row may hold 2^31 entries or more (a canonical CSR has at most n_cells per row): positions and
 * counts inside a row are 32-bit, ranks and sums are formed in f64 from them.
 *   mu_group_moments: d_sum / d_sumsq (f64 whatever the value type) and d_nnz = number of stored values != 0 (NaN counts,
 *     an explicitly stored zero does not) of the entries of bucket b in row j.
 *   mu_rank_sums: every row's entries must be sorted ascending by value (d_cells permuted alike).  Ranks are those of the
 *     row over the n_kept labelled cells, ties averaged, the implicit and the explicitly stored zeros forming one tie block
 *     between the negative and the positive values.  d_ranksum[j][b]: sum of the ranks of the stored non-zero entries of
 *     bucket b; d_zero_rank[j]: the rank of the zero block; d_tie[j]: sum over the tie blocks of t^3 - t, the zero block
 *     included.  The caller adds (n_b - nnz[j][b]) * zero_rank[j].  n_kept: the number of labels >= 0. */
int mu_group_moments_max_groups(void);
int mu_rank_row_cap(void);
int mu_group_moments(int dtype, int64_t d, int64_t n_cells, int64_t nnz, int n_buckets, const int64_t* d_indptr,
                     const int32_t* d_cells, const void* d_values, const int32_t* d_labels, double* d_sum,
                     double* d_sumsq, int64_t* d_nnz, void* stream);
int mu_rank_sums(int dtype, int64_t d, int64_t n_cells, int64_t nnz, int n_buckets, int64_t n_kept,
                 const int64_t* d_indptr, const int32_t* d_cells, const void* d_values, const int32_t* d_labels,
                 double* d_ranksum, double* d_zero_rank, double* d_tie, void* stream);

/* ---- muon.tl.snf: similarity network fusion (/root/reference/muon/_core/tools.py:716-920; csrc/snf.hip, C-ABI v804) ----
 * Every matrix is n x n row-major f64 with a leading dimension >= n; what lies past column n of a row is never read into
 * a result.  No atomics: two calls agree bit for bit.  Arguments are checked before any HIP call.
 *   mu_snf_affinity_f64: d_W = _affinity_matrix(d_D, k, sigma): D <- (D + D^T) / 2 with a zero diagonal, means_i = mean of
 *     the finite values among the 2nd .. (k+1)-th smallest of row i, + eps (d_means [n], written), sig = (means_i +
 *     means_j) / 3 + D / 3 + eps, W = N(0, sigma sig).pdf(D).  d_W may be d_D.  1 <= k <= mu_snf_affinity_max_k() = 127,
 *     n <= 65535.
 *   mu_snf_normalize_f64: r_i = sum_j x_ij - x_ii, 1 where that is 0 (d_r [n], written); out_ij = (x_ij / (2 r_i) +
 *     x_ji / (2 r_j)) / 2, diagonal 0.5: symmetric bit for bit.  d_out may be d_X (one read, one write of the matrix).
 *   mu_snf_topk_f64: the k largest of every row with their columns, descending: d_idx / d_val [n x k].
 *     1 <= k <= mu_snf_max_k() = 64, k <= n.  Equal values: in no promised order.
 *   mu_snf_p_scale_f64: on the CSR of z (n rows): d_rowsum[i] = sum of row i in stored order (compensated), then every
 *     entry (i, j) is divided by d_rowsum[j], in place - the reference's `z / z.sum(axis=1)`.
 *   mu_snf_diffuse_f64: Y = (P X)^T, P the CSR (d_indptr int64, d_cols int32, d_vals), X = (X_0 + .. + X_{nmat-1}) / nmat
 *     formed while it is read (h_X: HOST array of nmat device pointers, all with the leading dimension ldx, added in this
 *     order), the entries of a row of P added in stored order.  1 <= nmat <= mu_snf_max_terms() = 8; d_Y is none of the
 *     terms.  Twice in a row it gives P S P^T for a symmetric S. */
int mu_snf_max_k(void);
int mu_snf_affinity_max_k(void);
int mu_snf_max_terms(void);
int mu_snf_affinity_f64(int64_t n, int k, int64_t ldd, const double* d_D, int64_t ldw, double* d_W, double sigma,
                        double eps, double* d_means, void* stream);
int mu_snf_normalize_f64(int64_t n, int64_t ldx, const double* d_X, int64_t ldo, double* d_out, double* d_r, void* stream);
int mu_snf_topk_f64(int64_t n, int k, int64_t ldw, const double* d_W, int32_t* d_idx, double* d_val, void* stream);
int mu_snf_p_scale_f64(int64_t n, int64_t nnz, const int64_t* d_indptr, const int32_t* d_cols, double* d_vals,
                       double* d_rowsum, void* stream);
int mu_snf_diffuse_f64(int64_t n, int nmat, const void* const* h_X, int64_t ldx, const int64_t* d_indptr,
                       const int32_t* d_cols, const double* d_vals, int64_t ldy, double* d_Y, void* stream);

/* ---- muon.atac.tl.scan_sequences: position weight matrices against every window of every sequence (csrc/motif.hip,
 * C-ABI v805; the arithmetic is stated in DESIGN.md 9.10) -------------------------------------------------------------
 * The sequences are one stream d_codes [total] (uint8: 0..3 = A C G T, 4 = invalid) with d_offsets [n_seq + 1] (int64,
 * offsets[0] = 0, ascending, offsets[n_seq] = total).  The bank is sorted by length and cut into n_mtiles tiles of
 * mu_motif_group() = 16 motifs: d_bank [n_mtiles][mu_motif_max_len() = 32][4][16] f64 (tile, column, base, motif; zero
 * past a motif's length), d_tile_len [n_mtiles] the longest motif of a tile, d_mlen / d_thr / d_orig [16 n_mtiles] every
 * motif's length (a padding slot: 255), threshold (padding: +inf) and index in the caller's order.  Every value of the
 * bank must be finite.
 *   mu_motif_room: d_room[p] = number of valid codes from p to the next invalid one or the end of p's sequence, capped
 *     at mu_motif_max_len().
 *   mu_motif_count: d_counts [n_mtiles][ceil(total / mu_motif_tile())] = hits of every (motif tile, position tile).  A
 *     window is a hit iff room >= length and the j-ascending f64 sum of M[code[p + j], j] is >= the threshold.
 *   mu_motif_write: with d_base = the exclusive scan of d_counts (int64) and n_hits its total, every hit goes to its own
 *     slot of d_seq / d_motif / d_pos (int32) / d_score (f64): no atomics, two calls agree byte for byte.  Slots are in
 *     (motif tile, position tile) order; the caller orders the rows. */
int mu_motif_max_len(void);
int mu_motif_tile(void);
int mu_motif_group(void);
int mu_motif_room(int64_t total, int64_t n_seq, const uint8_t* d_codes, const int64_t* d_offsets, uint8_t* d_room,
                  void* stream);
int mu_motif_count(int64_t total, int64_t n_seq, int n_mtiles, const uint8_t* d_codes, const uint8_t* d_room,
                   const double* d_bank, const int32_t* d_tile_len, const int32_t* d_mlen, const double* d_thr,
                   int32_t* d_counts, void* stream);
int mu_motif_write(int64_t total, int64_t n_seq, int n_mtiles, const uint8_t* d_codes, const uint8_t* d_room,
                   const int64_t* d_offsets, const double* d_bank, const int32_t* d_tile_len, const int32_t* d_mlen,
                   const double* d_thr, const int32_t* d_orig, const int32_t* d_counts, const int64_t* d_base,
                   int64_t n_hits, int32_t* d_seq, int32_t* d_motif, int32_t* d_pos, double* d_score, void* stream);

/* ---- muon.tl.leiden / muon.tl.louvain: multiplex clustering (/root/reference/muon/_core/tools.py:928-1206; csrc/cluster.hip,
 * C-ABI v806; the optimiser is stated in muon_amd/_core/cluster.py and DESIGN.md 9.11) -----------------------------------
 * All arithmetic f64, labels int32, offsets int64.  No atomics: two calls agree bit for bit.  Arguments are checked
 * before any HIP call.
 *   mu_cluster_move_f64: one sub-round.  S without its diagonal is the CSR (d_indptr [nv + 1], d_cols, d_vals [nnz]);
 *     d_labels [nv] the snapshot, d_size [nv] the members per community id, d_P / d_K [nv][2 n_layers] the strengths
 *     (kout^1, kin^1, ...) of the vertices / their totals per community id, h_coef (HOST) the n_layers coefficients.
 *     For each of the nverts vertices v of d_verts: the candidates are labels[v] = a and the labels of v's neighbours
 *     (with d_bound, nullable: of the neighbours u with bound[u] == bound[v]); score(C) = w(v, C) - sum_l coef_l
 *     (kout_v Kin_C + kin_v Kout_C), P[v] taken out of K[a]; when size[a] == 1 a candidate C != a with size[C] == 1
 *     and C > a is none; the best is the largest score, ties to the smallest id; d_prop[v] = the best if it is not a and
 *     scores above a strictly, else a; d_score[v] = the score of d_prop[v].  only_single: a vertex with size[a] != 1
 *     gets d_prop[v] = a, d_score[v] = 0.  A vertex with more than mu_cluster_max_table() = 512 candidates stores 1 to
 *     *d_overflow (never 0: the caller clears it), d_prop[v] = a, d_score[v] = 0.  Entries of vertices not in d_verts are
 *     not written.  1 <= n_layers <= mu_cluster_max_layers() = 4.
 *   mu_cluster_segsum_f64: d_out[s][:] = sum of the rows d_ptr[s] .. d_ptr[s + 1] of d_vals [n][w]; lane j of a wave
 *     adds rows j, j + 64, ... in order, then the xor butterfly. */
int mu_cluster_max_table(void);
int mu_cluster_max_layers(void);
int mu_cluster_move_f64(int64_t nverts, const int32_t* d_verts, int64_t nv, int64_t nnz, const int64_t* d_indptr,
                        const int32_t* d_cols, const double* d_vals, const int32_t* d_labels, const int32_t* d_bound,
                        const int32_t* d_size, int n_layers, const double* d_P, const double* d_K, const double* h_coef,
                        int only_single, int32_t* d_prop, double* d_score, int32_t* d_overflow, void* stream);
int mu_cluster_segsum_f64(int64_t n, int64_t nseg, int w, const double* d_vals, const int64_t* d_ptr, double* d_out,
                          void* stream);

/* ---- muon.tl.umap: the layout optimiser of the multimodal UMAP (/root/reference/muon/_core/tools.py:1209-1362; csrc/umap.hip,
 * C-ABI v807; the optimiser is stated in muon_amd/_core/umap.py and DESIGN.md 9.12) -----------------------------------------
 * All arithmetic f64, columns int32, offsets and periods int64.  No atomics: two calls agree bit for bit.  Arguments are
 * checked before any HIP call.
 *   mu_umap_epoch_f64: epoch `epoch` (1 .. n_epochs <= 2^20) as one Jacobi step, d_Y_out = d_Y_in + alpha_e F(d_Y_in), both
 *     [n][n_components] row-major and two different buffers; n_components is 2 or 3 (mu_umap_max_components() = 3).  The
 *     graph is the CSR (d_indptr [n + 1], d_cols [nnz]) with d_E [nnz] the entries' periods in units of 2^-16 epochs
 *     (E >= 2^16; a smaller one is never active).  With t = epoch 2^16 and c = floor(t / E), entry j of row v is active iff
 *     t mod E < 2^16; it then adds to F_v clip(-2ab d2^(b-1) / (1 + a d2^b) (y_v - y_u)) (u its column, d2 = |y_v - y_u|^2,
 *     nothing when d2 == 0, clip to +-4 per coordinate), and for s = 0 .. floor(t rate / E) - floor(p 2^16 rate / E) - 1 with
 *     p = ceil((c - 1) E / 2^16): clip(2 gamma b / ((0.001 + d2)(1 + a d2^b)) (y_v - y_k)), k = ((h >> 32) n) >> 32 of h =
 *     splitmix64(splitmix64(splitmix64(seed + epoch) ^ j) + s), nothing when k == v or d2 == 0.  0 <= rate <= 1024.  d2^b is
 *     one pow; a group of 16 lanes per vertex, lane g adds the entries g, g + 16, ... in order (an entry: its attraction,
 *     then its negatives in order), then the xor butterfly over offsets 8, 4, 2, 1.  One launch, no synchronisation. */
int mu_umap_max_components(void);
int mu_umap_epoch_f64(int64_t n, int64_t nnz, const int64_t* d_indptr, const int32_t* d_cols, const int64_t* d_E,
                      int n_components, int epoch, int n_epochs, int rate, double a, double b, double gamma,
                      double alpha_e, uint64_t seed, const double* d_Y_in, double* d_Y_out, void* stream);

/* ---- muon.atac.pp.scopen: one coordinate-descent sweep of bounded NMF over the rows of a factor
 * (/root/reference/muon/_atac/preproc.py:155-236 hands the arithmetic to scOpen's MF module, scikit-learn's
 * _update_cdnmf_fast; csrc/nmf.hip, C-ABI v810) -------------------------------------------------------------
 * All f64, row-major.  Per row i, for t = 0 .. k-1 in order:  b = d_B[i,t] (* d_bscale[i]) (- l1 when l1 != 0);
 * grad = -b, then grad = grad + d_G[t,r] * W[i,r] for r = 0 .. k-1 ascending (product and sum two roundings, the row's
 * already-updated entries);  pg = W[i,t] == 0 ? min(0, grad) : grad;  v_i += |pg|;  if d_G[t,t] != 0:
 * W[i,t] = max(W[i,t] - grad / d_G[t,t], 0).  The updated d_W is bit-equal to that statement.
 *   d_W [rows x ldw] in / out and d_B [rows x ldb]: columns >= k are neither read nor written.  d_G [k x k] (an l2 term
 *   already on its diagonal).  d_Wout (optional) [rows x ldo]: d_oscale[i] * Wnew[i,t] (d_oscale NULL: a copy), columns
 *   k .. ldo-1 written as zero.  d_gram [k x k] = Wnew^T Wnew, d_viol [1] = sum of the v_i.
 * No float atomics: every workgroup (one wave, 64-row tiles walked grid-stride) leaves its partial sums in its slot of
 * d_work (mu_nmf_cd_worksize bytes) and a second kernel adds the slots in slot order - two calls agree bit for bit.  The
 * grid is min(ceil(rows / 64), max_blocks) workgroups (max_blocks 0: 512).  1 <= k <= mu_nmf_max_components() = 64;
 * rows = 0 gives zeros.  Arguments are checked before any HIP call. */
int mu_nmf_max_components(void);
size_t mu_nmf_cd_worksize(int64_t rows, int k, int max_blocks);
int mu_nmf_cd_sweep_f64(int64_t rows, int k, double* d_W, int64_t ldw, const double* d_B, int64_t ldb,
                        const double* d_bscale, const double* d_G, double l1, const double* d_oscale, double* d_Wout,
                        int64_t ldo, double* d_gram, double* d_viol, void* d_work, size_t work_bytes, int max_blocks,
                        void* stream);

/* ---- muon_amd.rna.pp / muon_amd.tl.pca: the RNA branch on the device CSR (scanpy's normalize_total, log1p,
 * highly_variable_genes and pca, the steps with which /root/reference/docs/source/omics opens every RNA modality;
 * csrc/rna.hip, C-ABI v811) ------------------------------------------------------------------------------
 *   mu_gene_moments: X^T as a CSR (d rows = genes; only d_indptr and d_values [nnz] are read).  d_sums [4 x d] f64:
 *     row 0 sum x, row 1 sum x^2, row 2 sum e, row 3 sum e^2 with e = expm1(x * c) (rows 2 and 3 are zero when with_e
 *     is 0); d_nnz [d]: stored values != 0 (NaN counts, a stored zero does not).  Values are widened to f64 first.  A
 *     wave per gene, walked grid-stride; lane l adds the entries lo + l, lo + l + 64, ... in that order (squares by fma)
 *     and the lane sums are combined by a tree over the lane offsets 32, 16, .. 1: no atomics, two calls agree bit for
 *     bit.  The grid is min(ceil(d / 4), max_blocks) workgroups (max_blocks 0: mu_gene_moments_max_blocks()).
 *   mu_rna_value_sweep: v = x (/ d_div[row] when d_div is given) (-> log1p(v) when log_flag, then / log_div when
 *     log_div != 0: log_div = ln(base)), computed in f64 and rounded once to the storage type.  d_out may be d_in.
 *   mu_shift_cols_f32: Y[i, j] -= (float)d_m[j] for a row-major n x B block, B in {16, 32, 64}: the f32 subtraction
 *     of the once-rounded mean, bit for bit.  A column with d_m[j] = 0 comes back as it was.
 *   mu_scale_rows_f32: d_out[i, j] = d_s[i] * d_Q[i, j] (one f32 product) for a row-major d x B block; d_out may be d_Q.
 * Arguments are checked before any HIP call. */
int mu_gene_moments_max_blocks(void);
int mu_gene_moments(int dtype, int64_t d, int64_t nnz, const int64_t* d_indptr, const void* d_values, double c,
                    int with_e, double* d_sums, int64_t* d_nnz, int max_blocks, void* stream);
int mu_rna_value_sweep(int dtype, int64_t n, int64_t nnz, const int64_t* d_indptr, const void* d_in, void* d_out,
                       const double* d_div, int log_flag, double log_div, void* stream);
int mu_shift_cols_f32(int64_t n, int B, float* d_Y, const double* d_m, void* stream);
int mu_scale_rows_f32(int64_t d, int B, const float* d_s, const float* d_Q, float* d_out, void* stream);

/* ---- muon.tl.mofa with smooth_covariate (MEFISTO): the eigen route's two passes over the eigenvectors of a factor's
 * prior covariance (csrc/gp.hip, C-ABI v813) -----------------------------------------------------------------
 * d_V [n x n] f64 row-major with leading dimension ldv >= n; every vector f64 [n]; 1 <= n <= 2^22 (n = 0: nothing is done).
 *   mu_gp_project_f64:   d_u = V^T d_r.  Panels of 256 rows write partial sums to d_work [ceil(n / 256) x n]
 *     (mu_gp_project_worksize bytes): within a panel a column's products are added in four chains (row mod 4), then
 *     ((c0 + c1) + c2) + c3; a second kernel adds the panels in panel order.
 *   mu_gp_posterior_f64: d_m[i] = sum_j V[i,j] d_g[j] d_u[j] and d_dc[i] = sum_j V[i,j]^2 d_g[j] from ONE read of row i.
 *     A wave per row: lane l adds the terms j = l, l + 64, ... in four chains (j / 64 mod 4), added as above, and the lane
 *     sums are combined by a tree over the lane offsets 32, 16, .. 1.
 * No atomics; two calls agree bit for bit.  Arguments are checked before any HIP call. */
size_t mu_gp_project_worksize(int64_t n);
int mu_gp_project_f64(int64_t n, const double* d_V, int64_t ldv, const double* d_r, double* d_u, void* d_work,
                      size_t work_bytes, void* stream);
int mu_gp_posterior_f64(int64_t n, const double* d_V, int64_t ldv, const double* d_g, const double* d_u, double* d_m,
                        double* d_dc, void* stream);

/* ---- muon_amd.rna.pp.scale: clipped z-scores of a device CSR as a sparse matrix plus one row (scanpy's scale;
 * csrc/scale.hip, C-ABI v814) ------------------------------------------------------------------------------
 * Row-major CSR: d_indptr int64 [n + 1], d_indices int32 [nnz], values f32 / f64 [nnz].  d_mean, d_std, d_z: f64 [d];
 * lo <= hi are the clip range (-inf / +inf for a side that is not clipped).  One statement, all f64, no contraction:
 * t = (x - d_mean[c]) / d_std[c];  t < lo -> lo, t > hi -> hi by comparisons (a NaN stays NaN, as with np.clip); one
 * rounding to the storage type.
 *   mu_scale_values: d_out[p] = T(t - d_z[c]) for every stored entry p (the kernel needs no d_indptr: an entry's result
 *     depends on its value and its column alone).  d_out may be d_in.  A column outside [0, d) gives NaN.  With d_mean =
 *     d_z = 0 and lo = -inf it is the scaling without centring; with d_z = clip((0 - mean) / std) it is S = C - 1 z^T.
 *   mu_scale_dense_rows: rows [row_lo, row_hi) of the dense C into the row-major block d_out [(row_hi - row_lo) x d]:
 *     T(d_z[j]) where nothing is stored, T(t) - computed from x, rounded once - where an entry is stored (a stored
 *     zero gives the value of an implicit one when d_z = clip((0 - mean) / std)).  A wave per row, walked
 *     grid-stride; fill and stored values meet in the wave's own LDS tile, in that order, and a whole segment of the
 *     row is written out once, coalesced.  Rows are sorted by column (an unsorted row loses the entries behind a
 *     larger column).  d_indptr is clamped to [0, nnz] and a column outside [0, d) is skipped.
 * No atomics, every output element is written once: two calls agree byte for byte.  Arguments are checked before any
 * HIP call. */
int mu_scale_values(int dtype, int64_t nnz, int64_t d, const int32_t* d_indices, const void* d_in, void* d_out,
                    const double* d_mean, const double* d_std, const double* d_z, double lo, double hi, void* stream);
int mu_scale_dense_rows(int dtype, int64_t n, int64_t d, int64_t nnz, int64_t row_lo, int64_t row_hi,
                        const int64_t* d_indptr, const int32_t* d_indices, const void* d_values, const double* d_mean,
                        const double* d_std, const double* d_z, double lo, double hi, void* d_out, void* stream);

/* ---- muon_amd.pp.qc_metrics(qc_vars=, percent_top=): per-row sums of a device CSR (scanpy's calculate_qc_metrics;
 * csrc/qc.hip, C-ABI v815) ---------------------------------------------------------------------------------
 * Row-major CSR: d_indptr int64 [n_rows + 1], d_indices int32 [nnz], values f32 / f64 [nnz]; d_indptr is clamped to
 * [0, nnz].  A wave per row, walked grid-stride; results are f64; no float atomics and a fixed order of every sum: two
 * calls agree byte for byte.  Arguments are checked before any HIP call.
 *   mu_csr_row_masked_sums: d_flags uint32 [n_cols], bit q set when the column belongs to mask q; 1 <= n_masks <= 32;
 *     d_out[i * n_masks + q] = sum of row i's stored values whose column has bit q set (bit 31 is an ordinary bit; a
 *     column outside [0, n_cols) belongs to no mask).  One read of the row serves every mask.
 *   mu_csr_row_top_sums: h_ns is a HOST array of n_tops values, 1 <= n_tops <= 8, strictly ascending, each in
 *     1 .. n_cols; d_out[i * n_tops + j] = sum of the min(h_ns[j], len_i) largest stored values of row i (only stored
 *     entries are looked at: rows shorter than n are padded with zeros).  A radix select over order-preserving integer
 *     keys finds the n-th largest value t for every n in the same passes, then sum(v > t) + (n - count(v > t)) * t; no
 *     limit on the row length.  A row that stores a NaN terminates and writes something. */
int mu_csr_row_masked_sums(int dtype, int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t* d_indptr,
                           const int32_t* d_indices, const void* d_values, const uint32_t* d_flags, int n_masks,
                           double* d_out, void* stream);
int mu_csr_row_top_sums(int dtype, int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t* d_indptr,
                        const void* d_values, int n_tops, const int64_t* h_ns, double* d_out, void* stream);

/* ---- muon_amd.pp.harmony_integrate: the cell-long steps of Harmony's k-means rounds (csrc/harmony.hip, C-ABI v816;
 * the statement is muon_amd/_core/harmony.py and DESIGN.md 9.17) ---------------------------------------------------------
 * All arithmetic f64 on the matrix cores.  1 <= K <= mu_harmony_max_clusters() = 128, 1 <= d <= mu_harmony_max_dims() =
 * 64, 1 <= B, n_seg <= mu_harmony_max_levels() = 64; kp and dp are K and d rounded up to a multiple of 16.  d_idx is an
 * optional int64 list of row numbers (NULL: the rows are 0, 1, ...); a row number outside [0, n) contributes nothing and
 * is not written, a level code outside [0, B) is clamped: no address leaves the operands whatever the arrays hold.  No
 * float atomics: two calls agree byte for byte.  Arguments are checked before any HIP call.
 *   mu_harmony_gram_f64: d_out[s] = R_s^T Z_s, row-major [n_seg][kp][dp], over the rows d_idx[h_seg_ptr[s]] ..
 *     d_idx[h_seg_ptr[s + 1] - 1] (without d_idx: the rows h_seg_ptr[s] .. h_seg_ptr[s + 1] - 1) of d_R [n][ldr >= K]
 *     and d_Z [n][ldz >= d].  h_seg_ptr is a HOST array of n_seg + 1 offsets into the m entries of the list, ascending
 *     within [0, m]; an empty segment gives zeros.  Columns of R at or past K and of Z at or past d are masked by index
 *     (NaN there does no harm); the padding of d_out is zero.  Partial sums go to ceil(rows / 64) slots per segment, at
 *     most 512 / n_seg, in d_work (mu_harmony_gram_worksize bytes); a second kernel adds them in slot order.
 *   mu_harmony_assign_f64: for the nb cells c = d_idx[0 .. nb) with g = d_codes[c]:
 *       D_k = 2 (1 - Zc_c . Y_k);  t_k = -D_k / sigma_k;  w_k = exp(t_k - max_k t_k) * F[k][g];  R[c][k] = w_k / sum_k w_k
 *     for k < K and R[c][k] = 0 for K <= k < kp (ldr >= kp); no contraction.  d_Zc [n][ldz >= d], d_Y [K][d], d_sigma
 *     [K], d_F [K][B] row-major, d_codes int32 [n].  Rows of d_R that the list does not name are not touched.
 *   mu_harmony_objective_f64: d_out[0 .. 2] = the three terms of the objective over all n cells c and k < K, with r =
 *     R[c][k], D as above and g = d_codes[c]:  sum r D,  sum sigma_k r log r (0 log 0 := 0),  sum sigma_k r G[k][g]; d_G
 *     [K][B] row-major, d_R [n][ldr >= K] (columns at or past K are masked by index), one read of R.  Every workgroup
 *     (min(ceil(n / 64), 512): a function of n) leaves three partial sums in d_work (mu_harmony_objective_worksize
 *     bytes), a second kernel adds them in order; no contraction.
 *   mu_harmony_correct_f64: the cells are sorted by level, level g owns the rows h_seg_ptr[g] .. h_seg_ptr[g + 1] - 1
 *     (a HOST array of B + 1 ascending offsets from 0 to n).  d_Zcorr[c] = d_Z[c] - R[c][:K] W[g] with d_W [B][K][d]
 *     row-major, and d_Zc[c] = d_Zcorr[c] / |d_Zcorr[c]|_2, in one pass; both outputs [n][ldo >= d], columns at or past d
 *     are not written. */
int mu_harmony_max_clusters(void);
int mu_harmony_max_dims(void);
int mu_harmony_max_levels(void);
size_t mu_harmony_gram_worksize(int64_t m, int n_seg, int K, int d);
int mu_harmony_gram_f64(int64_t n, int64_t m, int K, int d, const double* d_R, int64_t ldr, const double* d_Z,
                        int64_t ldz, const int64_t* d_idx, int n_seg, const int64_t* h_seg_ptr, double* d_out,
                        void* d_work, size_t work_bytes, void* stream);
int mu_harmony_assign_f64(int64_t n, int K, int d, int B, int64_t nb, const double* d_Zc, int64_t ldz,
                          const double* d_Y, const double* d_sigma, const double* d_F, const int32_t* d_codes,
                          const int64_t* d_idx, double* d_R, int64_t ldr, void* stream);
size_t mu_harmony_objective_worksize(int64_t n);
int mu_harmony_objective_f64(int64_t n, int K, int d, int B, const double* d_Zc, int64_t ldz, const double* d_Y,
                             const double* d_R, int64_t ldr, const double* d_sigma, const double* d_G,
                             const int32_t* d_codes, double* d_out, void* d_work, size_t work_bytes, void* stream);
int mu_harmony_correct_f64(int64_t n, int K, int d, int B, const double* d_Z, int64_t ldz, const double* d_R,
                           int64_t ldr, const double* d_W, const int64_t* h_seg_ptr, double* d_Zcorr, double* d_Zc,
                           int64_t ldo, void* stream);

/* ---- muon_amd.pp.scrublet: synthetic doublets and the merge of a search with a large k (csrc/scrublet.hip, C-ABI v817;
 * the statement is muon_amd/_core/scrublet.py and DESIGN.md 9.18) ----------------------------------------------------------
 * Simulated row s is the sum of the rows d_parents[2 s] and d_parents[2 s + 1] (int64 [n_sim][2]) of a CANONICAL CSR
 * (columns ascending, no duplicates; int64 row pointers, f32 values, indices of index_bytes = 4 or 8 bytes): every
 * column stored in either parent is a stored entry of the result (explicit zeros included, nothing pruned), columns
 * ascending, a column stored in both carries the f32 sum, every other entry its value bit for bit; a pair (a, a) gives
 * the row doubled.  A parent outside [0, n_rows) gives an empty row.
 *   1. mu_csr_pair_rows_count: d_new_row_nnz[s] = len(a) + len(b) - (columns stored in both)
 *   2. the caller scans it into new_indptr (mu_exclusive_scan_i64) and allocates new_indices / new_values
 *   3. mu_csr_pair_rows_fill: the entries, each at a slot computed in closed form; a row never writes outside
 *      new_indptr[s] .. new_indptr[s + 1].  One wave per simulated row, no atomics, no row-length limit: two calls agree
 *      byte for byte. */
int mu_csr_pair_rows_count(int index_bytes, int64_t n_rows, int64_t n_sim, const int64_t* d_indptr,
                           const void* d_indices, const int64_t* d_parents, int64_t* d_new_row_nnz, void* stream);
int mu_csr_pair_rows_fill(int index_bytes, int64_t n_rows, int64_t n_sim, const int64_t* d_indptr, const void* d_indices,
                          const float* d_values, const int64_t* d_parents, const int64_t* d_new_indptr,
                          void* d_new_indices, float* d_new_values, void* stream);
/* mu_knn_merge_f64's contract for kc + cap <= mu_knn_merge_wide_max() = 8192 (callable below 1024 too): one workgroup
 * per query, the pairs sorted in LDS by (distance, position) - the same total order, so both merges return identical
 * arrays at every shape both accept.  cnt[q] is clamped to [0, cap] and not written; not in place. */
int mu_knn_merge_wide_max(void);
int mu_knn_merge_wide_f64(int64_t n_q, int kc, int cap, const double* d_cur_d, const int64_t* d_cur_p,
                          const double* d_buf_d, const int32_t* d_buf_pos, const int32_t* d_cnt, double* d_out_d,
                          int64_t* d_out_p, double* d_thr, void* stream);

/* ---- synthetic planted-topic counts (bench / tests only) ------ */
/* Pass 1: nnz of every row for rows [row0, row0+n_rows) of the global matrix.
 * Pass 2 (after scanning the counts into indptr): fills indices / values (f32 counts).*/
int mu_synth_row_nnz(int64_t row0, int64_t n_rows, int64_t n_cols, int n_topics, double density,
                     uint64_t seed, int64_t* d_row_nnz, void* stream);
int mu_synth_fill(int64_t row0, int64_t n_rows, int64_t n_cols, int n_topics, double density,
                  uint64_t seed, const int64_t* d_indptr, int32_t* d_indices, float* d_values,
                  void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MUON_AMD_H */
