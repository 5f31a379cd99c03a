// The RNA branch on the device CSR (muon_amd.rna.pp, muon_amd.tl.pca): per-gene moments, the value
// sweep of normalize_total / log1p, and the two block operators with which lsi's block Lanczos process works on the
// centred (and scaled) matrix without ever forming it.
//
//  * k_gene_moments: X^T as a CSR, one row per gene.  A wave takes a gene and grid-strides over the genes; lane l adds
//    the entries lo + l, lo + l + 64, ... in that order (four loads in flight, the additions in order), and the 64 lane
//    sums are combined by wave_sum's tree (offsets 32, 16, .. 1): the order of every addition is a function of the
//    row's length alone - no atomics, two calls agree bit for bit.  Values are widened to f64 first; expm1 and all sums
//    are f64.
//  * k_value_sweep: a wave per row, x -> x / div[row] (-> log1p (-> / log_div)), the arithmetic in f64 and one rounding
//    to the storage type; every entry is read and written by the same lane, so it may run in place.
//  * k_shift_cols / k_scale_rows: one f32 operation per element of a row-major block, four elements per lane.
//
// rank.hip's moments walk stages every entry in LDS for its lane-per-bucket readers; a gene's plain sums need no
// staging, so nothing of it is shared here beyond common.hpp.
#include "common.hpp"

constexpr int kRnaThreads = 256;
constexpr int kRnaWaves = kRnaThreads / 64;
constexpr int kRnaBlocksPerCu = 8;

template <typename T>
__global__ __launch_bounds__(kRnaThreads) void k_gene_moments(int64_t d, int64_t nnz, const int64_t* __restrict__ indptr,
                                                              const T* __restrict__ values, double c, int with_e,
                                                              double* __restrict__ sums, int64_t* __restrict__ cnt) {
  const int wave = uniform32(threadIdx.x >> 6), lane = lane_id();
  for (int64_t g = (int64_t)blockIdx.x * kRnaWaves + wave; g < d; g += (int64_t)gridDim.x * kRnaWaves) {
    int64_t lo = uniform64(indptr[g]), hi = uniform64(indptr[g + 1]);
    if (lo < 0) lo = 0;  // (a row never reaches outside the value array, whatever indptr holds)
    if (hi > nnz) hi = nnz;
    double s1 = 0.0, s2 = 0.0, e1 = 0.0, e2 = 0.0;
    int64_t nz = 0;
    auto add = [&](double x) {
      s1 += x;
      s2 = fma(x, x, s2);
      nz += (x != 0.0) ? 1 : 0;  // NaN counts; an explicitly stored zero does not
      if (with_e) {
        const double e = expm1(x * c);
        e1 += e;
        e2 = fma(e, e, e2);
      }
    };
    int64_t p = lo + lane;
    for (; p + 192 < hi; p += 256) {  // four loads in flight; the additions keep the lane's ascending order
      const T x0 = values[p], x1 = values[p + 64], x2 = values[p + 128], x3 = values[p + 192];
      add((double)x0);
      add((double)x1);
      add((double)x2);
      add((double)x3);
    }
    for (; p < hi; p += 64) add((double)values[p]);
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    nz = wave_sum(nz);
    if (with_e) {
      e1 = wave_sum(e1);
      e2 = wave_sum(e2);
    }
    if (lane == 0) {
      sums[g] = s1;
      sums[d + g] = s2;
      sums[2 * d + g] = e1;
      sums[3 * d + g] = e2;
      cnt[g] = nz;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kRnaThreads) void k_value_sweep(int64_t n, int64_t nnz, const int64_t* __restrict__ indptr,
                                                             const T* vin, T* vout, const double* __restrict__ div,
                                                             int log_flag, double log_div) {
  const int wave = uniform32(threadIdx.x >> 6), lane = lane_id();
  for (int64_t r = (int64_t)blockIdx.x * kRnaWaves + wave; r < n; r += (int64_t)gridDim.x * kRnaWaves) {
    int64_t lo = uniform64(indptr[r]), hi = uniform64(indptr[r + 1]);
    if (lo < 0) lo = 0;
    if (hi > nnz) hi = nnz;
    const double dv = div ? div[r] : 1.0;
    for (int64_t p = lo + lane; p < hi; p += 64) {
      double v = (double)vin[p];
      if (div) v = v / dv;
      if (log_flag) {
        v = log1p(v);
        if (log_div != 0.0) v = v / log_div;
      }
      vout[p] = (T)v;
    }
  }
}

// Y[i, j] -= (float)m[j]; B in {16, 32, 64}.  A lane's four columns are the same in every round: the stride of the
// grid, 4 * kRnaThreads * gridDim.x elements, is a multiple of B.
__global__ __launch_bounds__(kRnaThreads) void k_shift_cols(int64_t quads, int B, float* __restrict__ Y,
                                                            const double* __restrict__ m) {
  const int64_t t0 = (int64_t)blockIdx.x * kRnaThreads + threadIdx.x;
  const int j0 = (int)((t0 * 4) & (int64_t)(B - 1));
  const float m0 = (float)m[j0], m1 = (float)m[j0 + 1], m2 = (float)m[j0 + 2], m3 = (float)m[j0 + 3];
  float4* Y4 = reinterpret_cast<float4*>(Y);
  for (int64_t t = t0; t < quads; t += (int64_t)gridDim.x * kRnaThreads) {
    float4 y = Y4[t];
    y.x -= m0;
    y.y -= m1;
    y.z -= m2;
    y.w -= m3;
    Y4[t] = y;
  }
}

// out[i, j] = s[i] * Q[i, j]; out may be Q
__global__ __launch_bounds__(kRnaThreads) void k_scale_rows(int64_t quads, int shift, const float* __restrict__ s,
                                                            const float* Q, float* out) {
  const float4* Q4 = reinterpret_cast<const float4*>(Q);
  float4* O4 = reinterpret_cast<float4*>(out);
  for (int64_t t = (int64_t)blockIdx.x * kRnaThreads + threadIdx.x; t < quads; t += (int64_t)gridDim.x * kRnaThreads) {
    const float f = s[t >> shift];  // (B / 4 quads per row: shift = log2(B) - 2)
    float4 q = Q4[t];
    q.x *= f;
    q.y *= f;
    q.z *= f;
    q.w *= f;
    O4[t] = q;
  }
}

static inline int block_shift(int B) { return B == 16 ? 2 : B == 32 ? 3 : B == 64 ? 4 : -1; }

extern "C" {

int mu_gene_moments_max_blocks(void) { return mu_num_cus() * kRnaBlocksPerCu; }

int mu_gene_moments(int dtype, int64_t d, int64_t nnz, const int64_t* d_indptr, const void* d_values, double c,
                    int with_e, double* d_sums, int64_t* d_nnz, int max_blocks, void* stream) {
  MU_REQUIRE(d >= 0 && nnz >= 0 && max_blocks >= 0, "negative shape");
  MU_REQUIRE(dtype == MU_DTYPE_F32 || dtype == MU_DTYPE_F64, "dtype must be f32 or f64");
  if (d == 0) return MU_OK;
  MU_REQUIRE(d_indptr && d_sums && d_nnz && (nnz == 0 || d_values), "null pointer");
  unsigned grid = wave_grid(d, kRnaWaves, kRnaBlocksPerCu);
  if (max_blocks > 0 && grid > (unsigned)max_blocks) grid = (unsigned)max_blocks;
  hipStream_t st = (hipStream_t)stream;
  by_dtype(dtype, [&](auto t) {
    hipLaunchKernelGGL(k_gene_moments<decltype(t)>, dim3(grid), dim3(kRnaThreads), 0, st, d, nnz, d_indptr,
                       (const decltype(t)*)d_values, c, with_e, d_sums, d_nnz);
  });
  MU_CHECK_LAUNCH();
  return MU_OK;
}

int mu_rna_value_sweep(int dtype, int64_t n, int64_t nnz, const int64_t* d_indptr, const void* d_in, void* d_out,
                       const double* d_div, int log_flag, double log_div, void* stream) {
  MU_REQUIRE(n >= 0 && nnz >= 0, "negative shape");
  MU_REQUIRE(dtype == MU_DTYPE_F32 || dtype == MU_DTYPE_F64, "dtype must be f32 or f64");
  MU_REQUIRE(log_div >= 0.0, "log_div is ln(base) > 0, or 0 for the natural logarithm");
  if (n == 0 || nnz == 0) return MU_OK;
  MU_REQUIRE(d_indptr && d_in && d_out, "null pointer");
  const unsigned grid = wave_grid(n, kRnaWaves, kRnaBlocksPerCu);
  hipStream_t st = (hipStream_t)stream;
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_value_sweep<T>, dim3(grid), dim3(kRnaThreads), 0, st, n, nnz, d_indptr, (const T*)d_in,
                       (T*)d_out, d_div, log_flag, log_div);
  });
  MU_CHECK_LAUNCH();
  return MU_OK;
}

int mu_shift_cols_f32(int64_t n, int B, float* d_Y, const double* d_m, void* stream) {
  MU_REQUIRE(n >= 0, "negative shape");
  MU_REQUIRE(block_shift(B) >= 0, "B must be 16, 32 or 64");
  if (n == 0) return MU_OK;
  MU_REQUIRE(d_Y && d_m, "null pointer");
  const int64_t quads = n * (B / 4);
  hipLaunchKernelGGL(k_shift_cols, dim3(wave_grid(quads, kRnaThreads, kRnaBlocksPerCu)), dim3(kRnaThreads), 0,
                     (hipStream_t)stream, quads, B, d_Y, d_m);
  MU_CHECK_LAUNCH();
  return MU_OK;
}

int mu_scale_rows_f32(int64_t d, int B, const float* d_s, const float* d_Q, float* d_out, void* stream) {
  MU_REQUIRE(d >= 0, "negative shape");
  MU_REQUIRE(block_shift(B) >= 0, "B must be 16, 32 or 64");
  if (d == 0) return MU_OK;
  MU_REQUIRE(d_s && d_Q && d_out, "null pointer");
  const int64_t quads = d * (B / 4);
  hipLaunchKernelGGL(k_scale_rows, dim3(wave_grid(quads, kRnaThreads, kRnaBlocksPerCu)), dim3(kRnaThreads), 0,
                     (hipStream_t)stream, quads, block_shift(B), d_s, d_Q, d_out);
  MU_CHECK_LAUNCH();
  return MU_OK;
}

}  // extern "C"
