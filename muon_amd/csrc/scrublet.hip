// muon_amd.pp.scrublet: the two pieces doublet detection needs that nothing else here offers.
//
//  * k_pair_count / k_pair_fill: a simulated doublet is the sum of two raw count rows, E_sim[s] = E[a] + E[b].  One wave
//    per simulated row over two CANONICAL parent rows (columns ascending, no duplicates).  The count pass finds the
//    columns both rows store - every entry of a is looked up in b by a binary search, 64 entries per step - and the row's
//    length is len(a) + len(b) - matches.  The host scans the lengths (mu_exclusive_scan_i64); the fill pass then knows
//    every entry's slot in closed form:
//        a_i                goes to  i + lower_bound_b(col a_i) - (matches among a_0 .. a_{i-1})
//        b_j (no match)     goes to  j + lower_bound_a(col b_j) - (matches among b_0 .. b_{j-1})
//    (the entries before a_i in the union are the i entries of a before it and the entries of b with a smaller column,
//    and a column stored in both was counted twice).  "Matches before" is a prefix count inside the 64-entry step plus a
//    count carried across the steps.  A match stores the f32 sum, every other entry its own value, bit for bit: every
//    column stored in either parent stays a stored entry, explicit zeros included.  No atomics, no row-length limit, the
//    same bytes on every run.  A pair (a, a) gives the row doubled.
//  * k_knn_merge_wide: mu_knn_merge_f64's contract (csrc/knn.hip) past its 1024 pairs: list [kc] ++ buffer [min(cnt, cap)]
//    -> the kc smallest (distance, position) pairs ascending, ties by position, and the new threshold, for kc + cap <=
//    8192.  One workgroup of 256 threads per query, the pairs in LDS (12 bytes each: 96 KiB of the 160 KiB at 8192), a
//    workgroup-wide bitonic sort over the next power of two of the query's own count (padding = (+inf, INT_MAX): the
//    usual buffer holds about kc candidates, a quarter of its capacity).  The same total order as the
//    wave-wide kernel, so the two return identical arrays at every shape both accept.
#include "common.hpp"

namespace {

// first index in [0, n) of the ascending a[.] with a[i] >= key
template <typename I>
__device__ __forceinline__ int64_t pair_lower_bound(const I* __restrict__ a, int64_t n, int64_t key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if ((int64_t)a[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the two parent rows of simulated row s as (first entry, length); false: a parent outside the matrix (an empty row)
__device__ __forceinline__ bool pair_rows(const int64_t* __restrict__ indptr, const int64_t* __restrict__ parents,
                                          int64_t n_rows, int64_t s, int64_t& a0, int64_t& an, int64_t& b0,
                                          int64_t& bn) {
  const int64_t ra = parents[2 * s], rb = parents[2 * s + 1];
  if (ra < 0 || ra >= n_rows || rb < 0 || rb >= n_rows) return false;
  a0 = uniform64(indptr[ra]);
  an = uniform64(indptr[ra + 1]) - a0;
  b0 = uniform64(indptr[rb]);
  bn = uniform64(indptr[rb + 1]) - b0;
  return an >= 0 && bn >= 0;
}

template <typename I>
__global__ __launch_bounds__(256) void k_pair_count(int64_t n_rows, int64_t n_sim, const int64_t* __restrict__ indptr,
                                                    const I* __restrict__ indices,
                                                    const int64_t* __restrict__ parents,
                                                    int64_t* __restrict__ new_row_nnz) {
  const int lane = lane_id();
  const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t s = wave0; s < n_sim; s += n_waves) {
    int64_t a0, an, b0, bn, cnt = 0;
    if (pair_rows(indptr, parents, n_rows, s, a0, an, b0, bn)) {
      const I* __restrict__ A = indices + a0;
      const I* __restrict__ B = indices + b0;
      int64_t matches = 0;
      for (int64_t i0 = 0; i0 < an; i0 += 64) {
        const int64_t i = i0 + lane;
        bool hit = false;
        if (i < an) {
          const int64_t col = (int64_t)A[i];
          const int64_t lb = pair_lower_bound(B, bn, col);
          hit = lb < bn && (int64_t)B[lb] == col;
        }
        matches += __popcll(__ballot(hit));
      }
      cnt = an + bn - matches;
    }
    if (lane == 0) new_row_nnz[s] = cnt;
  }
}

// one side of the fill: the entries of `own` (n_own of them) into the union with `other`; the side that stores the
// matches (kSum) adds the other row's value, the other side skips them
template <bool kSum, typename I>
__device__ __forceinline__ void pair_fill_side(const I* __restrict__ own, const float* __restrict__ own_v, int64_t n_own,
                                               const I* __restrict__ other, const float* __restrict__ other_v,
                                               int64_t n_other, int64_t dst, int64_t end, I* __restrict__ out_i,
                                               float* __restrict__ out_v, int lane) {
  const unsigned long long below = (1ull << lane) - 1ull;
  int64_t carried = 0;  // matches in the steps before this one (wave-uniform)
  for (int64_t i0 = 0; i0 < n_own; i0 += 64) {
    const int64_t i = i0 + lane;
    bool hit = false;
    int64_t lb = 0;
    I col = 0;
    if (i < n_own) {
      col = own[i];
      lb = pair_lower_bound(other, n_other, (int64_t)col);
      hit = lb < n_other && (int64_t)other[lb] == (int64_t)col;
    }
    const unsigned long long m = __ballot(hit);
    if (i < n_own && (kSum || !hit)) {
      const int64_t at = dst + i + lb - (carried + __popcll(m & below));
      if (at >= dst && at < end) {  // (a row never writes outside its own slots)
        out_i[at] = col;
        out_v[at] = (kSum && hit) ? own_v[i] + other_v[lb] : own_v[i];
      }
    }
    carried += __popcll(m);
  }
}

template <typename I>
__global__ __launch_bounds__(256) void k_pair_fill(int64_t n_rows, int64_t n_sim, const int64_t* __restrict__ indptr,
                                                   const I* __restrict__ indices, const float* __restrict__ values,
                                                   const int64_t* __restrict__ parents,
                                                   const int64_t* __restrict__ new_indptr, I* __restrict__ new_indices,
                                                   float* __restrict__ new_values) {
  const int lane = lane_id();
  const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t s = wave0; s < n_sim; s += n_waves) {
    int64_t a0, an, b0, bn;
    if (!pair_rows(indptr, parents, n_rows, s, a0, an, b0, bn)) continue;
    const int64_t dst = uniform64(new_indptr[s]), end = uniform64(new_indptr[s + 1]);
    pair_fill_side<true>(indices + a0, values + a0, an, indices + b0, values + b0, bn, dst, end, new_indices,
                         new_values, lane);
    pair_fill_side<false>(indices + b0, values + b0, bn, indices + a0, values + a0, an, dst, end, new_indices,
                          new_values, lane);
  }
}

// ---- the wide merge -----------------------------------------------------------------------------------------------
constexpr int kWideThreads = 256;
constexpr int kWideMax = 8192;  // kc + cap must fit: 8192 pairs x 12 bytes = 96 KiB of LDS

__global__ __launch_bounds__(kWideThreads) void k_knn_merge_wide(int64_t n_q, int kc, int cap, int P,
                                                                 const double* __restrict__ cur_d,
                                                                 const int64_t* __restrict__ cur_p,
                                                                 const double* __restrict__ buf_d,
                                                                 const int32_t* __restrict__ buf_pos,
                                                                 const int32_t* __restrict__ cnt,
                                                                 double* __restrict__ out_d, int64_t* __restrict__ out_p,
                                                                 double* __restrict__ thr) {
  extern __shared__ double wide_smem[];
  double* K = wide_smem;                        // [P]
  int* V = reinterpret_cast<int*>(K + P);       // [P]
  const int tid = threadIdx.x;
  for (int64_t q = blockIdx.x; q < n_q; q += gridDim.x) {
    int c = cnt[q];
    c = c < 0 ? 0 : (c < cap ? c : cap);  // (an overflowed row is redone by the caller)
    const int m = kc + c;
    // this query's power of two: the filter appends about kc candidates per panel, a quarter of what the buffer holds
    int Pq = 64;
    while (Pq < m) Pq <<= 1;  // (<= P: m <= kc + cap)
    for (int t = tid; t < Pq; t += kWideThreads) {
      double d = __builtin_inf();
      int v = 0x7fffffff;
      if (t < kc) {
        d = cur_d[q * kc + t];
        v = (int)cur_p[q * kc + t];
      } else if (t < m) {
        d = buf_d[q * cap + (t - kc)];
        v = buf_pos[q * cap + (t - kc)];
      }
      K[t] = d;
      V[t] = v;
    }
    __syncthreads();
    // the pairs (t, t | j) of a step: P / 2 of them, pair i has t = i with a zero bit inserted at j
    for (int k = 2; k <= Pq; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int i = tid; i < (Pq >> 1); i += kWideThreads) {
          const int t = ((i & ~(j - 1)) << 1) | (i & (j - 1));
          const int u = t | j;
          const double a = K[t], b = K[u];
          const int va = V[t], vb = V[u];
          const bool gt = a > b || (a == b && va > vb);  // (no NaN: distances are finite or +inf)
          const bool up = (t & k) == 0;
          if (gt == up) {
            K[t] = b;
            K[u] = a;
            V[t] = vb;
            V[u] = va;
          }
        }
        __syncthreads();
      }
    }
    for (int t = tid; t < kc; t += kWideThreads) {
      out_d[q * kc + t] = K[t];
      out_p[q * kc + t] = (int64_t)V[t];
    }
    if (tid == 0) thr[q] = K[kc - 1];
    __syncthreads();  // the next query overwrites the pairs
  }
}

template <typename I>
int pair_count(int64_t n_rows, int64_t n_sim, const int64_t* indptr, const void* indices, const int64_t* parents,
               int64_t* row_nnz, hipStream_t st) {
  hipLaunchKernelGGL(k_pair_count<I>, dim3(wave_grid(n_sim, 4, 16)), dim3(256), 0, st, n_rows, n_sim, indptr,
                     (const I*)indices, parents, row_nnz);
  MU_CHECK_LAUNCH();
  return MU_OK;
}

template <typename I>
int pair_fill(int64_t n_rows, int64_t n_sim, const int64_t* indptr, const void* indices, const float* values,
              const int64_t* parents, const int64_t* new_indptr, void* new_indices, float* new_values, hipStream_t st) {
  hipLaunchKernelGGL(k_pair_fill<I>, dim3(wave_grid(n_sim, 4, 16)), dim3(256), 0, st, n_rows, n_sim, indptr,
                     (const I*)indices, values, parents, new_indptr, (I*)new_indices, new_values);
  MU_CHECK_LAUNCH();
  return MU_OK;
}

}  // namespace

extern "C" {

int mu_csr_pair_rows_count(int index_bytes, int64_t n_rows, int64_t n_sim, const int64_t* d_indptr,
                           const void* d_indices, const int64_t* d_parents, int64_t* d_new_row_nnz, void* stream) {
  MU_REQUIRE(n_rows >= 0 && n_sim >= 0, "negative shape");
  MU_REQUIRE(index_bytes == 4 || index_bytes == 8, "index_bytes must be 4 or 8");
  if (n_sim == 0) return MU_OK;
  MU_REQUIRE(d_indptr && d_parents && d_new_row_nnz, "null pointer");
  return by_index<2>(index_bytes == 8, [&](auto wide) {
    using I = std::conditional_t<decltype(wide)::value == 1, int64_t, int32_t>;
    return pair_count<I>(n_rows, n_sim, d_indptr, d_indices, d_parents, d_new_row_nnz, (hipStream_t)stream);
  });
}

int mu_csr_pair_rows_fill(int index_bytes, int64_t n_rows, int64_t n_sim, const int64_t* d_indptr, const void* d_indices,
                          const float* d_values, const int64_t* d_parents, const int64_t* d_new_indptr,
                          void* d_new_indices, float* d_new_values, void* stream) {
  MU_REQUIRE(n_rows >= 0 && n_sim >= 0, "negative shape");
  MU_REQUIRE(index_bytes == 4 || index_bytes == 8, "index_bytes must be 4 or 8");
  if (n_sim == 0) return MU_OK;
  MU_REQUIRE(d_indptr && d_parents && d_new_indptr, "null pointer");
  return by_index<2>(index_bytes == 8, [&](auto wide) {
    using I = std::conditional_t<decltype(wide)::value == 1, int64_t, int32_t>;
    return pair_fill<I>(n_rows, n_sim, d_indptr, d_indices, d_values, d_parents, d_new_indptr, d_new_indices,
                        d_new_values, (hipStream_t)stream);
  });
}

int mu_knn_merge_wide_max(void) { return kWideMax; }

int mu_knn_merge_wide_f64(int64_t n_q, int kc, int cap, const double* d_cur_d, const int64_t* d_cur_p,
                          const double* d_buf_d, const int32_t* d_buf_pos, const int32_t* d_cnt, double* d_out_d,
                          int64_t* d_out_p, double* d_thr, void* stream) {
  MU_REQUIRE(n_q >= 0 && kc >= 1 && cap >= 1 && (int64_t)kc + cap <= kWideMax, "kc + cap must be <= 8192");
  if (n_q == 0) return MU_OK;
  MU_REQUIRE(d_cur_d && d_cur_p && d_buf_d && d_buf_pos && d_cnt && d_out_d && d_out_p && d_thr, "null pointer");
  MU_REQUIRE(d_out_d != d_cur_d && d_out_p != d_cur_p, "the merge is not in place");
  int P = 64;
  while (P < kc + cap) P <<= 1;
  const size_t lds = (size_t)P * (sizeof(double) + sizeof(int));
  if (lds > 64 * 1024)
    MU_CHECK_HIP(hipFuncSetAttribute((const void*)k_knn_merge_wide, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  // as many workgroups as the LDS lets a CU hold, the queries walked grid-stride
  const int per_cu = (int)((160 * 1024) / lds) < 8 ? (int)((160 * 1024) / lds) : 8;
  int64_t wgs = (int64_t)mu_num_cus() * (per_cu < 1 ? 1 : per_cu);
  if (wgs > n_q) wgs = n_q;
  hipLaunchKernelGGL(k_knn_merge_wide, dim3((unsigned)wgs), dim3(kWideThreads), lds, (hipStream_t)stream, n_q, kc, cap, P,
                     d_cur_d, d_cur_p, d_buf_d, d_buf_pos, d_cnt, d_out_d, d_out_p, d_thr);
  MU_CHECK_LAUNCH();
  return MU_OK;
}

}  // extern "C"
