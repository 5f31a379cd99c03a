// Per-row QC sums on the device CSR: what scanpy's calculate_qc_metrics adds for `qc_vars` and `percent_top`
// (pct_counts_mt, pct_counts_in_top_50_genes: the columns the RNA tutorials filter on) from a matrix that is resident
// in HBM.  A wave per row, walked grid-stride; every result is f64; no float atomics, every sum in a fixed order (a
// lane adds its entries in stored order, the lanes meet in the shuffle tree of wave_sum): two calls agree byte for byte.
//
//  * k_row_masked_sums: out[i * M + q] = sum of row i's stored values whose column has bit q of the per-column flag
//    word set.  One read of the row (8 B/entry f32, 12 f64) serves all M <= 32 masks; the flag table (4 B/column) stays
//    in L2, like the column table of k_submatrix_*.
//  * k_row_top_sums: out[i * L + j] = sum of the min(ns[j], len_i) largest stored values of row i, for L <= 8 ascending
//    ns at once.  Select, then sum: a radix select over order-preserving integer keys (8 bits per pass, most
//    significant first: 4 passes for f32, 8 for f64) finds the key t_j of the m_j-th largest value for every j in the
//    same passes - histograms of 256 bins in LDS, private to the wave, one per j, shared between the j whose digits
//    so far agree - and one more pass forms  sum(v : key(v) > t_j) + (m_j - #{key(v) > t_j}) * t_j.  Ties at the m-th
//    value and explicit zeros do not change that sum.  No row-length limit: the row is read again from L2 per pass
//    (values only, the columns are never needed).  The pass count is fixed, so a row that stores a NaN terminates like
//    any other (its result is outside the contract).
#include "common.hpp"

// ---------------------------------------------------------------------------------
// masked sums
// ---------------------------------------------------------------------------------
constexpr int kQcUnroll = 4;  // 64-entry chunks a wave has in flight per step

template <typename T, int MW>
__global__ __launch_bounds__(256) void k_row_masked_sums(int64_t n_rows, int64_t n_cols, int64_t nnz, int M,
                                                         const int64_t* __restrict__ indptr,
                                                         const int32_t* __restrict__ indices,
                                                         const T* __restrict__ values,
                                                         const uint32_t* __restrict__ flags, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t i = wave0; i < n_rows; i += n_waves) {
    int64_t lo = uniform64(indptr[i]), hi = uniform64(indptr[i + 1]);
    lo = lo < 0 ? 0 : (lo > nnz ? nnz : lo);  // (a row never reads outside the entry arrays)
    hi = hi < lo ? lo : (hi > nnz ? nnz : hi);
    double acc[MW];
#pragma unroll
    for (int q = 0; q < MW; ++q) acc[q] = 0.0;
    for (int64_t p0 = lo; p0 < hi; p0 += 64 * kQcUnroll) {
      uint32_t f[kQcUnroll];
      double v[kQcUnroll];
#pragma unroll
      for (int u = 0; u < kQcUnroll; ++u) {
        const int64_t p = p0 + 64 * u + lane;
        const bool ok = p < hi;
        const int32_t c = ok ? indices[p] : -1;
        v[u] = ok ? (double)values[p] : 0.0;
        f[u] = ((uint32_t)c < (uint64_t)n_cols) ? flags[c] : 0u;  // (a column outside the table belongs to no mask)
      }
#pragma unroll
      for (int u = 0; u < kQcUnroll; ++u) {
#pragma unroll
        for (int q = 0; q < MW; ++q)
          if ((f[u] >> q) & 1u) acc[q] += v[u];
      }
    }
    double mine = 0.0;
#pragma unroll
    for (int q = 0; q < MW; ++q) {
      const double r = wave_sum_all(acc[q]);
      if (lane == q) mine = r;
    }
    if (lane < M) out[i * M + lane] = mine;
  }
}

// ---------------------------------------------------------------------------------
// top-n sums
// ---------------------------------------------------------------------------------
constexpr int kTopMaxL = 8;
constexpr int kTopWaves = 4;  // waves of a workgroup: each owns LW histograms of 256 bins (LW KiB)
struct TopNs {
  int64_t n[kTopMaxL];
};

// order-preserving keys: a < b as values  <=>  key(a) < key(b) as unsigned integers (-0 sorts below +0)
__device__ __forceinline__ uint32_t top_key(float v) {
  const uint32_t u = __builtin_bit_cast(uint32_t, v);
  return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ uint64_t top_key(double v) {
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double top_value(uint32_t k) {
  return (double)__builtin_bit_cast(float, (k >> 31) ? (k ^ 0x80000000u) : ~k);
}
__device__ __forceinline__ double top_value(uint64_t k) {
  return __builtin_bit_cast(double, (k >> 63) ? (k ^ 0x8000000000000000ull) : ~k);
}

// hist[digit] += 1 for every lane with `take` (called by the whole wave).  Count data puts most lanes of a step into
// one bin: then one lane adds the count instead of 64 adds to one address queuing up.
__device__ __forceinline__ void top_hist_add(uint32_t* hist, int digit, bool take, int lane) {
  const unsigned long long act = __ballot(take);
  if (act == 0) return;
  const int first = __ffsll(act) - 1;
  const int d0 = __builtin_amdgcn_readlane(digit, first);
  if (__ballot(take && digit == d0) == act) {
    if (lane == first) atomicAdd(&hist[d0], (uint32_t)__popcll(act));
  } else if (take) {
    atomicAdd(&hist[digit], 1u);
  }
}

template <typename T, int LW>
__global__ __launch_bounds__(64 * kTopWaves) void k_row_top_sums(int64_t n_rows, int64_t nnz, int L, TopNs ns,
                                                                  const int64_t* __restrict__ indptr,
                                                                  const T* __restrict__ values,
                                                                  double* __restrict__ out) {
  using K = decltype(top_key(T{}));
  constexpr int kDigits = (int)sizeof(K);
  __shared__ uint32_t s_hist[kTopWaves][LW][256];
  const int lane = threadIdx.x & 63, wave = uniform32(threadIdx.x >> 6);
  uint32_t(*hist)[256] = s_hist[wave];
  const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t i = wave0; i < n_rows; i += n_waves) {
    int64_t lo = uniform64(indptr[i]), hi = uniform64(indptr[i + 1]);
    lo = lo < 0 ? 0 : (lo > nnz ? nnz : lo);
    hi = hi < lo ? lo : (hi > nnz ? nnz : hi);
    if (hi - lo > 0x7fffffff) hi = lo + 0x7fffffff;  // (ranks and bin counts are 32-bit)
    const int len = (int)(hi - lo);
    if (len == 0) {
      if (lane < L) out[i * L + lane] = 0.0;
      continue;
    }
    // m[j]: how many of the row's values sum j takes; rem[j]: the rank of the wanted key among the entries that share
    // prefix[j]'s digits so far (1 = the largest).  1 <= rem[j] <= number of those entries, pass after pass.
    K prefix[LW];
    int m[LW], rem[LW];
#pragma unroll
    for (int j = 0; j < LW; ++j) {
      const int64_t n = ns.n[j];
      m[j] = rem[j] = n < (int64_t)len ? (int)n : len;
      prefix[j] = 0;
    }
    for (int dg = kDigits - 1; dg >= 0; --dg) {
      const int shift = 8 * dg;
      const K himask = dg == kDigits - 1 ? (K)0 : (K)(~(K)0 << (shift + 8));  // the digits already fixed
      // src[j]: the histogram j reads - its predecessor's where the digits so far agree (the same entries match)
      int src[LW];
      src[0] = 0;
#pragma unroll
      for (int j = 1; j < LW; ++j) src[j] = prefix[j] == prefix[j - 1] ? src[j - 1] : j;
#pragma unroll
      for (int j = 0; j < LW; ++j) {
        if (src[j] == j) {
#pragma unroll
          for (int u = 0; u < 4; ++u) hist[j][lane + 64 * u] = 0;
        }
      }
      wave_lds_sync();
      // (wave-uniform trip counts: the ballots below see the whole wave; four chunks' loads are in flight together)
      for (int64_t p0 = lo; p0 < hi; p0 += 64 * kQcUnroll) {
        K key[kQcUnroll];
#pragma unroll
        for (int u = 0; u < kQcUnroll; ++u) {
          const int64_t p = p0 + 64 * u + lane;
          key[u] = p < hi ? top_key(values[p]) : (K)0;
        }
#pragma unroll
        for (int u = 0; u < kQcUnroll; ++u) {
          if (p0 + 64 * u >= hi) break;
          const bool ok = p0 + 64 * u + lane < hi;
          const int digit = (int)((key[u] >> shift) & 0xff);
#pragma unroll
          for (int j = 0; j < LW; ++j) {
            if (src[j] == j) top_hist_add(hist[j], digit, ok && ((key[u] ^ prefix[j]) & himask) == 0, lane);
          }
        }
      }
      wave_lds_sync();
#pragma unroll
      for (int j = 0; j < LW; ++j) {
        // lane l holds bins 4 l .. 4 l + 3; above = entries in larger bins than the lane's own
        const uint32_t* h = hist[src[j]];
        int b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) b[u] = (int)h[4 * lane + u];
        const int own = b[0] + b[1] + b[2] + b[3];
        int inc = own;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const int t = __shfl_down(inc, off, 64);
          if (lane + off < 64) inc += t;
        }
        int above = inc - own, found = -1, left = 0;
#pragma unroll
        for (int u = 3; u >= 0; --u) {
          if (found < 0 && above < rem[j] && rem[j] <= above + b[u]) {
            found = 4 * lane + u;
            left = rem[j] - above;
          }
          above += b[u];
        }
        const unsigned long long who = __ballot(found >= 0);
        if (who != 0) {  // (always: the rank lies inside the matching entries)
          const int fl = __ffsll(who) - 1;
          prefix[j] |= (K)(unsigned)__builtin_amdgcn_readlane(found, fl) << shift;
          rem[j] = __builtin_amdgcn_readlane(left, fl);
        }
      }
      wave_lds_sync();  // (the next pass zeroes the bins this one read)
    }
    // prefix[j] is the key of the m[j]-th largest value: everything above it, plus the ties that fill the count
    double s[LW];
    int c[LW];
#pragma unroll
    for (int j = 0; j < LW; ++j) {
      s[j] = 0.0;
      c[j] = 0;
    }
    for (int64_t p0 = lo; p0 < hi; p0 += 64 * kQcUnroll) {
      T x[kQcUnroll];
      bool ok[kQcUnroll];
#pragma unroll
      for (int u = 0; u < kQcUnroll; ++u) {
        const int64_t p = p0 + 64 * u + lane;
        ok[u] = p < hi;
        x[u] = ok[u] ? values[p] : (T)0;
      }
#pragma unroll
      for (int u = 0; u < kQcUnroll; ++u) {
        const K key = top_key(x[u]);
#pragma unroll
        for (int j = 0; j < LW; ++j) {
          if (ok[u] && key > prefix[j]) {
            s[j] += (double)x[u];
            ++c[j];
          }
        }
      }
    }
    double mine = 0.0;
#pragma unroll
    for (int j = 0; j < LW; ++j) {
      const double sj = wave_sum_all(s[j]);
      const int cj = wave_sum_all(c[j]);
      if (lane == j) mine = sj + (double)(m[j] - cj) * top_value(prefix[j]);
    }
    if (lane < L) out[i * L + lane] = mine;
  }
}

extern "C" {

int mu_csr_row_masked_sums(int dtype, int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t* d_indptr,
                           const int32_t* d_indices, const void* d_values, const uint32_t* d_flags, int n_masks,
                           double* d_out, void* stream) {
  MU_REQUIRE(n_rows >= 0 && n_cols >= 0 && nnz >= 0, "negative shape");
  MU_REQUIRE(n_cols < (int64_t)1 << 31, "column indices are int32");
  MU_REQUIRE(dtype == MU_DTYPE_F32 || dtype == MU_DTYPE_F64, "dtype must be f32 or f64");
  MU_REQUIRE(n_masks >= 1 && n_masks <= 32, "1 to 32 masks per launch");
  if (n_rows == 0) return MU_OK;
  MU_REQUIRE(d_indptr && d_out, "null pointer");
  MU_REQUIRE(nnz == 0 || (d_indices && d_values), "null pointer");
  MU_REQUIRE(n_cols == 0 || d_flags, "null pointer");
  const unsigned grid = wave_grid(n_rows, 4, 16);
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    by_width<1, 8, 32>(n_masks, [&](auto mw) {
      hipLaunchKernelGGL((k_row_masked_sums<T, decltype(mw)::value>), dim3(grid), dim3(256), 0, (hipStream_t)stream, n_rows, n_cols, nnz,
                         n_masks, d_indptr, d_indices, (const T*)d_values, d_flags, d_out);
    });
  });
  MU_CHECK_LAUNCH();
  return MU_OK;
}

int mu_csr_row_top_sums(int dtype, int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t* d_indptr,
                        const void* d_values, int n_tops, const int64_t* h_ns, double* d_out, void* stream) {
  MU_REQUIRE(n_rows >= 0 && n_cols >= 0 && nnz >= 0, "negative shape");
  MU_REQUIRE(dtype == MU_DTYPE_F32 || dtype == MU_DTYPE_F64, "dtype must be f32 or f64");
  MU_REQUIRE(n_tops >= 1 && n_tops <= kTopMaxL, "1 to 8 values of n per launch");
  MU_REQUIRE(h_ns, "null pointer");
  TopNs ns;
  for (int j = 0; j < kTopMaxL; ++j) {
    ns.n[j] = h_ns[j < n_tops ? j : n_tops - 1];  // (the instance's spare slots repeat the last n; they are not stored)
    MU_REQUIRE(ns.n[j] >= 1 && ns.n[j] <= n_cols, "every n must lie in 1 .. n_cols");
    MU_REQUIRE(j == 0 || j >= n_tops || ns.n[j] > ns.n[j - 1], "the values of n must be strictly ascending");
  }
  if (n_rows == 0) return MU_OK;
  MU_REQUIRE(d_indptr && d_out, "null pointer");
  MU_REQUIRE(nnz == 0 || d_values, "null pointer");
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    by_width<1, 2, 4, 8>(n_tops, [&](auto lw) {
      // LW KiB of histograms per wave: 8 workgroups per CU at LW = 4 (the 32-wave cap), 5 at LW = 8 (160 KiB of LDS)
      hipLaunchKernelGGL((k_row_top_sums<T, decltype(lw)::value>), dim3(wave_grid(n_rows, kTopWaves, 8)), dim3(64 * kTopWaves), 0,
                         (hipStream_t)stream, n_rows, nnz, n_tops, ns, d_indptr, (const T*)d_values, d_out);
    });
  });
  MU_CHECK_LAUNCH();
  return MU_OK;
}

}  // extern "C"
