// QC sweep and row / column selection on the device CSR: what muon.pp.filter_obs / filter_var
// (muon/_core/preproc.py:675-881) and scanpy's calculate_qc_metrics need from a matrix that is resident in HBM, so that
// the filtering step between ingest and tfidf does not send the matrix over PCIe a second time.
//
//  * k_csr_qc: the slab sweep of k_row_col_sums (tfidf.hip) with the counts of the non-zero values carried next to the
//    sums: per row and per column, one pass, 8 B/entry (f32).  Same walk, same per-lane order, same wave reduction and the
//    same fixed-order reduction of the per-workgroup column partials: sums are bit-identical to mu_csr_row_col_sums
//    wherever that sweep is reproducible (sums that are exact in f64: counts, binarised values); counts are integers.
//  * k_submatrix_count / k_submatrix_fill: a wave per kept row walks the source row 256 entries at a time, looks every
//    column up in the old -> new table, ballots the survivors and stores them in stored order at the row's running
//    offset.  8 B/entry read, 8 B/kept entry written (f32); the table (4 B/column) stays in L2.
#include "sweep.hpp"

// ---------------------------------------------------------------------------------
// QC sweep
// ---------------------------------------------------------------------------------
// 96 KiB of LDS (f64 sums + int32 counts of one 8192-column slab): one 1024-thread workgroup per CU.
// Entries of a workgroup's row block are addressed by 32-bit offsets from the block's first entry, like the sum sweep.
template <typename T>
__global__ __launch_bounds__(kSweepThreads, 4) void k_csr_qc(
    int64_t n_rows, int64_t n_cols, int64_t S, const int64_t* __restrict__ indptr,
    const int32_t* __restrict__ indices, const T* __restrict__ values, const int64_t* __restrict__ sp,
    int64_t* __restrict__ row_nnz, double* __restrict__ rowsum, double* __restrict__ partial,
    int32_t* __restrict__ partial_cnt) {
  __shared__ double bins[kSlab];
  __shared__ int32_t cnts[kSlab];
  __shared__ int64_t s_r[2];
  const int g = blockIdx.x, G = gridDim.x;
  if (threadIdx.x == 0) sweep_row_range(indptr, n_rows, g, G, s_r[0], s_r[1]);
  __syncthreads();
  const int64_t r0 = s_r[0], r1 = s_r[1];
  const int wave = uniform32(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int64_t wg_base = uniform64(indptr[r0 < n_rows ? r0 : n_rows]);
  const int32_t* __restrict__ ib = indices + wg_base;
  const T* __restrict__ vb = values + wg_base;
  for (int64_t s = 0; s < S; ++s) {
    for (int t = threadIdx.x; t < kSlab; t += kSweepThreads) {
      bins[t] = 0.0;
      cnts[t] = 0;
    }
    __syncthreads();
    const int32_t cbase = (int32_t)(s * kSlab);
    for (int64_t strip = r0 + wave; strip < r1; strip += (int64_t)kSweepWaves * 64) {
      const int64_t myrow = strip + (int64_t)kSweepWaves * lane;
      int lo_l = 0, hi_l = 0;
      if (myrow < r1) {
        lo_l = (int)(sp[myrow * (S + 1) + s] - wg_base);
        hi_l = (int)(sp[myrow * (S + 1) + s + 1] - wg_base);
      }
      const int64_t left = (r1 - strip + kSweepWaves - 1) / kSweepWaves;
      const int nrow = left < 64 ? (int)left : 64;  // wave-uniform
      double racc = 0.0;
      int cacc = 0;
      for (int l = 0; l < nrow; ++l) {
        const int lo = __builtin_amdgcn_readlane(lo_l, l), hi = __builtin_amdgcn_readlane(hi_l, l);
        double rs = 0.0;
        int rc = 0;
        for (int p = lo + lane; p < hi; p += 256) {
          int32_t c[4];
          T v[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int q = p + 64 * u;
            const bool ok = q < hi;
            c[u] = ok ? ib[q] : -1;
            v[u] = ok ? vb[q] : (T)0;
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            // (a column outside the slab - rows that are not sorted - must not leave the bins)
            const unsigned b = (unsigned)(c[u] - cbase);
            if (c[u] >= 0 && b < (unsigned)kSlab) {
              atomicAdd(&bins[b], (double)v[u]);
              rs += (double)v[u];
              if (v[u] != (T)0) {  // NaN counts; an explicitly stored zero does not
                atomicAdd(&cnts[b], 1);
                ++rc;
              }
            }
          }
        }
        rs = wave_sum(rs);  // (lane 0)
        rc = wave_sum(rc);
        const double tot = __shfl(rs, 0, 64);
        const int ctot = __shfl(rc, 0, 64);
        if (lane == l) {
          racc = tot;
          cacc = ctot;
        }
      }
      if (myrow < r1) {
        if (s == 0) {
          rowsum[myrow] = racc;
          row_nnz[myrow] = cacc;
        } else {
          rowsum[myrow] += racc;
          row_nnz[myrow] += cacc;
        }
      }
    }
    __syncthreads();
    const int64_t ncol_here = (n_cols - (int64_t)cbase) < kSlab ? (n_cols - (int64_t)cbase) : kSlab;
    double* dst = partial + (int64_t)g * n_cols + cbase;
    int32_t* dstc = partial_cnt + (int64_t)g * n_cols + cbase;
    for (int t = threadIdx.x; t < ncol_here; t += kSweepThreads) {
      dst[t] = bins[t];
      dstc[t] = cnts[t];
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_qc_reduce_partials(int64_t n_cols, int G, const double* __restrict__ partial,
                                                            const int32_t* __restrict__ partial_cnt,
                                                            double* __restrict__ colsum, int64_t* __restrict__ col_nnz) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_cols) return;
  double acc = 0.0;
  int64_t cnt = 0;
  for (int g = 0; g < G; ++g) {  // fixed order
    acc += partial[(int64_t)g * n_cols + j];
    cnt += partial_cnt[(int64_t)g * n_cols + j];
  }
  colsum[j] = acc;
  col_nnz[j] = cnt;
}

// ---------------------------------------------------------------------------------
// submatrix: kept rows (ascending list) x column table (old -> new, -1 dropped)
// ---------------------------------------------------------------------------------
constexpr int kSubUnroll = 4;  // 64-entry chunks a wave has in flight per step

// new column of the entry at p (-1: past the row's end, dropped, or a column outside the table)
__device__ __forceinline__ int32_t sub_lookup(const int32_t* __restrict__ indices, const int32_t* __restrict__ table,
                                              int64_t n_cols, int64_t p, int64_t hi) {
  if (p >= hi) return -1;
  const int32_t c = indices[p];
  return ((uint32_t)c < (uint64_t)n_cols) ? table[c] : -1;
}

__global__ __launch_bounds__(256) void k_submatrix_count(int64_t n_rows, int64_t n_cols, int64_t n_keep,
                                                         const int64_t* __restrict__ indptr,
                                                         const int32_t* __restrict__ indices,
                                                         const int64_t* __restrict__ rows,
                                                         const int32_t* __restrict__ table,
                                                         int64_t* __restrict__ new_row_nnz) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t i = wave0; i < n_keep; i += n_waves) {
    const int64_t row = rows[i];
    int64_t cnt = 0;
    if (row >= 0 && row < n_rows) {
      const int64_t lo = indptr[row], hi = indptr[row + 1];
      for (int64_t p0 = lo; p0 < hi; p0 += 64 * kSubUnroll) {
        int32_t nc[kSubUnroll];
#pragma unroll
        for (int u = 0; u < kSubUnroll; ++u) nc[u] = sub_lookup(indices, table, n_cols, p0 + 64 * u + lane, hi);
#pragma unroll
        for (int u = 0; u < kSubUnroll; ++u) cnt += __popcll(__ballot(nc[u] >= 0));
      }
    }
    if (lane == 0) new_row_nnz[i] = cnt;
  }
}

// V: an unsigned integer of the value's width - values are moved, never computed with (NaN payloads survive)
template <typename V>
__global__ __launch_bounds__(256) void k_submatrix_fill(int64_t n_rows, int64_t n_cols, int64_t n_keep,
                                                        const int64_t* __restrict__ indptr,
                                                        const int32_t* __restrict__ indices,
                                                        const V* __restrict__ values,
                                                        const int64_t* __restrict__ rows,
                                                        const int32_t* __restrict__ table,
                                                        const int64_t* __restrict__ new_indptr,
                                                        int32_t* __restrict__ new_indices, V* __restrict__ new_values) {
  const int lane = threadIdx.x & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t i = wave0; i < n_keep; i += n_waves) {
    const int64_t row = rows[i];
    if (row < 0 || row >= n_rows) continue;
    const int64_t lo = indptr[row], hi = indptr[row + 1];
    int64_t dst = uniform64(new_indptr[i]);
    const int64_t end = uniform64(new_indptr[i + 1]);  // (a row never writes past its own slots)
    for (int64_t p0 = lo; p0 < hi; p0 += 64 * kSubUnroll) {
      int32_t nc[kSubUnroll];
      V v[kSubUnroll];
#pragma unroll
      for (int u = 0; u < kSubUnroll; ++u) {
        const int64_t p = p0 + 64 * u + lane;
        nc[u] = sub_lookup(indices, table, n_cols, p, hi);
        v[u] = p < hi ? values[p] : (V)0;
      }
#pragma unroll
      for (int u = 0; u < kSubUnroll; ++u) {
        const unsigned long long m = __ballot(nc[u] >= 0);
        const int64_t at = dst + __popcll(m & below);
        if (nc[u] >= 0 && at < end) {
          new_indices[at] = nc[u];
          new_values[at] = v[u];
        }
        dst += __popcll(m);
      }
    }
  }
}

extern "C" {

size_t mu_csr_qc_worksize(int64_t n_rows, int64_t n_cols) {
  if (n_rows < 0 || n_cols < 0) return 0;
  const int64_t S = num_slabs(n_cols);
  const size_t G = (size_t)mu_num_cus();
  return align256((size_t)(n_rows * (S + 1)) * sizeof(int64_t)) + align256(G * (size_t)n_cols * sizeof(double)) +
         align256(G * (size_t)n_cols * sizeof(int32_t)) + 256;
}

int mu_csr_qc(int dtype, int64_t n_rows, int64_t n_cols, const int64_t* d_indptr, const int32_t* d_indices,
              const void* d_values, int64_t* d_row_nnz, double* d_rowsum, int64_t* d_col_nnz, double* d_colsum,
              void* d_work, size_t work_bytes, const int64_t* d_slab_ptr, void* stream) {
  MU_REQUIRE(n_rows >= 0 && n_cols >= 0, "negative shape");
  MU_REQUIRE(n_cols < (int64_t)1 << 31, "column indices are int32");
  MU_REQUIRE(dtype == MU_DTYPE_F32 || dtype == MU_DTYPE_F64, "dtype must be f32 or f64");
  MU_REQUIRE(d_indptr, "null pointer");
  MU_REQUIRE(n_rows == 0 || (d_row_nnz && d_rowsum), "null pointer");
  MU_REQUIRE(n_cols == 0 || (d_col_nnz && d_colsum), "null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (n_cols == 0 || n_rows == 0) {
    if (n_cols) {
      MU_CHECK_HIP(hipMemsetAsync(d_colsum, 0, sizeof(double) * n_cols, st));
      MU_CHECK_HIP(hipMemsetAsync(d_col_nnz, 0, sizeof(int64_t) * n_cols, st));
    }
    if (n_rows) {
      MU_CHECK_HIP(hipMemsetAsync(d_rowsum, 0, sizeof(double) * n_rows, st));
      MU_CHECK_HIP(hipMemsetAsync(d_row_nnz, 0, sizeof(int64_t) * n_rows, st));
    }
    return MU_OK;
  }
  MU_REQUIRE(d_work && work_bytes >= mu_csr_qc_worksize(n_rows, n_cols), "work buffer too small");
  const int64_t S = num_slabs(n_cols);
  const int G = mu_num_cus();
  const int64_t* sp = d_slab_ptr ? d_slab_ptr : (const int64_t*)d_work;
  size_t off = align256((size_t)(n_rows * (S + 1)) * sizeof(int64_t));
  double* partial = (double*)((char*)d_work + off);
  off += align256((size_t)G * (size_t)n_cols * sizeof(double));
  int32_t* partial_cnt = (int32_t*)((char*)d_work + off);
  if (!d_slab_ptr) {
    int rc = launch_slab_ptr(n_rows, n_cols, d_indptr, d_indices, (int64_t*)d_work, st);
    if (rc) return rc;
  }
  by_dtype(dtype, [&](auto t) {
    hipLaunchKernelGGL(k_csr_qc<decltype(t)>, dim3(G), dim3(kSweepThreads), 0, st, n_rows, n_cols, S, d_indptr, d_indices,
                       (const decltype(t)*)d_values, sp, d_row_nnz, d_rowsum, partial, partial_cnt);
  });
  MU_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_qc_reduce_partials, dim3((unsigned)((n_cols + 255) / 256)), dim3(256), 0, st, n_cols, G, partial,
                     partial_cnt, d_colsum, d_col_nnz);
  MU_CHECK_LAUNCH();
  return MU_OK;
}

int mu_csr_submatrix_count(int64_t n_rows, int64_t n_cols, int64_t n_keep, const int64_t* d_indptr,
                           const int32_t* d_indices, const int64_t* d_rows, const int32_t* d_col_table,
                           int64_t* d_new_row_nnz, void* stream) {
  MU_REQUIRE(n_rows >= 0 && n_cols >= 0 && n_keep >= 0, "negative shape");
  MU_REQUIRE(n_keep <= n_rows, "more kept rows than rows");
  MU_REQUIRE(n_cols < (int64_t)1 << 31, "column indices are int32");
  if (n_keep == 0) return MU_OK;
  MU_REQUIRE(d_indptr && d_rows && d_new_row_nnz, "null pointer");
  MU_REQUIRE(n_cols == 0 || d_col_table, "null pointer");
  hipLaunchKernelGGL(k_submatrix_count, dim3(wave_grid(n_keep, 4, 16)), dim3(256), 0, (hipStream_t)stream, n_rows, n_cols,
                     n_keep, d_indptr, d_indices, d_rows, d_col_table, d_new_row_nnz);
  MU_CHECK_LAUNCH();
  return MU_OK;
}

int mu_csr_submatrix_fill(int dtype, int64_t n_rows, int64_t n_cols, int64_t n_keep, const int64_t* d_indptr,
                          const int32_t* d_indices, const void* d_values, const int64_t* d_rows,
                          const int32_t* d_col_table, const int64_t* d_new_indptr, int32_t* d_new_indices,
                          void* d_new_values, void* stream) {
  MU_REQUIRE(n_rows >= 0 && n_cols >= 0 && n_keep >= 0, "negative shape");
  MU_REQUIRE(n_keep <= n_rows, "more kept rows than rows");
  MU_REQUIRE(n_cols < (int64_t)1 << 31, "column indices are int32");
  MU_REQUIRE(dtype == MU_DTYPE_F32 || dtype == MU_DTYPE_F64, "dtype must be f32 or f64");
  if (n_keep == 0) return MU_OK;
  MU_REQUIRE(d_indptr && d_rows && d_new_indptr, "null pointer");
  MU_REQUIRE(n_cols == 0 || d_col_table, "null pointer");
  const unsigned grid = wave_grid(n_keep, 4, 16);
  by_dtype(dtype, [&](auto t) {
    using U = std::conditional_t<sizeof(t) == 4, uint32_t, uint64_t>;  // values move as bits
    hipLaunchKernelGGL(k_submatrix_fill<U>, dim3(grid), dim3(256), 0, (hipStream_t)stream, n_rows, n_cols, n_keep,
                       d_indptr, d_indices, (const U*)d_values, d_rows, d_col_table, d_new_indptr, d_new_indices,
                       (U*)d_new_values);
  });
  MU_CHECK_LAUNCH();
  return MU_OK;
}

}  // extern "C"
