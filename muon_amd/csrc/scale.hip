// muon_amd.rna.pp.scale on the device CSR: clipped z-scores as a sparse matrix plus one row.
//
// With per-gene tables mean, std, z = clip((0 - mean) / std, lo, hi) every implicit zero of gene j maps to z[j], so the
// clipped scaled matrix is C = S + 1 z^T with S on the stored entries of X alone.  Both kernels share one statement, all
// of it f64 (the file is built with -ffp-contract=off: subtraction, division and the final rounding stay apart):
//     t = (x - mean[c]) / std[c];   t < lo -> lo,  t > hi -> hi  (comparisons: a NaN fails both and stays NaN).
//
//  * k_scale_values: out[p] = T(t - z[c]) for every stored entry p.  One lane per entry over the flat value array,
//    grid-stride: an entry's result depends on its value and its column alone, so the kernel reads no indptr.  The lane
//    that reads entry p writes entry p, so out may be the values themselves.  A column outside [0, d) reads no table
//    and gives NaN.
//  * k_scale_dense_rows: rows [row_lo, row_hi) of the dense C.  A WAVE takes a row (grid-stride) and walks it in
//    segments of kSegCols columns through an LDS tile of its own; nothing is shared between waves, so there is no
//    workgroup barrier anywhere and a CU's waves are at different phases of different rows:
//        (1) tile[j] = T(z[c0 + j]) for the whole segment
//        (2) tile[c - c0] = T(t) for the row's stored entries with c0 <= c < c0 + w.  The rows of a device CSR are
//            sorted: the wave keeps one position p in the row, reads 64 entries from it, writes those inside the segment
//            and advances p to the first entry that belongs to a later segment - every entry is read once (twice when a
//            batch straddles a segment's end), not once per segment
//        (3) out[row, c0 + j] = tile[j], consecutive lanes consecutive columns (16 bytes per lane when every row of the
//            block starts on a 16-byte boundary)
//    Why no element can end up with the fill value over the stored one: the fill (1) and the stored values (2) meet in
//    LDS only, written by the SAME wave in program order - a wave's LDS accesses complete in the order they issue, and
//    wave_lds_sync() keeps the compiler from reordering them - so every write of (2) lands after every write of (1);
//    global memory sees an element once, in (3), read back from the tile after (2).  There is no second pass over the
//    output in which a fill could overtake a stored value, and nothing is ordered by launch or by memory-system luck.
//    T(t) is computed from x, not as S + z: every element is rounded once.  A stored zero gives T(clip((0 - mean) /
//    std)), which is T(z[j]) by z's definition.  Two entries of one row in the same column (no canonical CSR has them)
//    leave one of the two values, never the fill.  A row that is NOT sorted loses the entries that lie behind a larger
//    column (they come out as implicit zeros); it still reaches nothing outside the arrays.
//
// Neither kernel uses atomics and every output element is written exactly once: two calls agree byte for byte.  indptr
// is clamped to [0, nnz] as in rank.hip's rank_row_range, and a column outside the segment - so any column outside
// [0, d) - is never used as an index: nothing reaches outside the arrays, whatever the CSR holds.
#include "common.hpp"

namespace {

constexpr int kScaleThreads = 256;
constexpr int kScaleBlocksPerCu = 8;
constexpr int kScaleWaves = kScaleThreads / 64;
constexpr int kSegCols = 1024;  // per wave: 16 KiB (f32) / 32 KiB (f64) of LDS per workgroup, five workgroups and more per CU

__device__ __forceinline__ double scale_clip(double x, double mean, double sd, double lo, double hi) {
  double t = (x - mean) / sd;
  if (t < lo) t = lo;
  if (t > hi) t = hi;
  return t;
}

template <typename T>
__global__ __launch_bounds__(kScaleThreads) void k_scale_values(int64_t nnz, int64_t d, const int32_t* __restrict__ indices,
                                                                const T* vin, T* vout, const double* __restrict__ mean,
                                                                const double* __restrict__ sd,
                                                                const double* __restrict__ z, double lo, double hi) {
  const int64_t stride = (int64_t)gridDim.x * kScaleThreads;
  for (int64_t p = (int64_t)blockIdx.x * kScaleThreads + threadIdx.x; p < nnz; p += stride) {
    const int64_t c = indices[p];
    double r = __builtin_nan("");
    if (c >= 0 && c < d) r = scale_clip((double)vin[p], mean[c], sd[c], lo, hi) - z[c];
    vout[p] = (T)r;
  }
}

// VEC: the write-out stores 16 bytes per lane (the host asks for it when every row of the block starts on a 16-byte
// boundary); otherwise one element per lane
template <typename T, bool VEC>
__global__ __launch_bounds__(kScaleThreads) void k_scale_dense_rows(int64_t row_lo, int64_t row_hi, int64_t d, int64_t nnz,
                                                                    const int64_t* __restrict__ indptr,
                                                                    const int32_t* __restrict__ indices,
                                                                    const T* __restrict__ values,
                                                                    const double* __restrict__ mean,
                                                                    const double* __restrict__ sd,
                                                                    const double* __restrict__ z, double lo, double hi,
                                                                    T* __restrict__ out) {
  constexpr int kV = 16 / (int)sizeof(T);
  typedef T V16 __attribute__((ext_vector_type(kV)));
  __shared__ __attribute__((aligned(16))) T tiles[kScaleWaves][kSegCols];
  const int wave = uniform32(threadIdx.x >> 6), lane = lane_id();
  T* tile = tiles[wave];
  for (int64_t row = row_lo + (int64_t)blockIdx.x * kScaleWaves + wave; row < row_hi;
       row += (int64_t)gridDim.x * kScaleWaves) {
    int64_t p = uniform64(indptr[row]), b = uniform64(indptr[row + 1]);
    if (p < 0) p = 0;  // (a row never reaches outside the entry arrays, whatever indptr holds)
    if (b > nnz) b = nnz;
    T* o = out + (row - row_lo) * d;
    for (int64_t c0 = 0; c0 < d; c0 += kSegCols) {
      const int w = (int)(d - c0 < kSegCols ? d - c0 : kSegCols);
      for (int j = lane; j < w; j += 64) tile[j] = (T)z[c0 + j];
      wave_lds_sync();
      while (p < b) {  // (p, b wave-uniform)
        const int64_t q = p + lane;
        int64_t j = kSegCols;  // a lane past the row's end counts as "behind this segment"
        if (q < b) j = (int64_t)indices[q] - c0;
        if (j >= 0 && j < w) tile[j] = (T)scale_clip((double)values[q], mean[c0 + j], sd[c0 + j], lo, hi);
        const unsigned long long behind = __ballot(j >= w);
        if (behind) {  // the first entry of a later segment (or the row's end): the next segment starts there
          p += __builtin_ctzll(behind);
          break;
        }
        p += 64;
      }
      wave_lds_sync();
      if constexpr (VEC) {  // (every row starts on a 16-byte boundary and d is a multiple of kV: so is w)
        const V16* t16 = reinterpret_cast<const V16*>(tile);
        V16* o16 = reinterpret_cast<V16*>(o + c0);
        for (int j = lane; j < w / kV; j += 64) o16[j] = t16[j];
      } else {
        for (int j = lane; j < w; j += 64) o[c0 + j] = tile[j];
      }
      wave_lds_sync();  // (the next segment's fill stays behind these reads)
    }
  }
}

}  // namespace

extern "C" {

int mu_scale_values(int dtype, int64_t nnz, int64_t d, const int32_t* d_indices, const void* d_in, void* d_out,
                    const double* d_mean, const double* d_std, const double* d_z, double lo, double hi, void* stream) {
  MU_REQUIRE(nnz >= 0 && d >= 0, "negative shape");
  MU_REQUIRE(dtype == MU_DTYPE_F32 || dtype == MU_DTYPE_F64, "dtype must be f32 or f64");
  MU_REQUIRE(lo <= hi, "lo <= hi (the infinities for a side that is not clipped)");
  if (nnz == 0) return MU_OK;
  MU_REQUIRE(d_indices && d_in && d_out && (d == 0 || (d_mean && d_std && d_z)), "null pointer");
  const unsigned grid = wave_grid(nnz, kScaleThreads, kScaleBlocksPerCu);
  hipStream_t st = (hipStream_t)stream;
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_scale_values<T>, dim3(grid), dim3(kScaleThreads), 0, st, nnz, d, d_indices, (const T*)d_in,
                       (T*)d_out, d_mean, d_std, d_z, lo, hi);
  });
  MU_CHECK_LAUNCH();
  return MU_OK;
}

int mu_scale_dense_rows(int dtype, int64_t n, int64_t d, int64_t nnz, int64_t row_lo, int64_t row_hi,
                        const int64_t* d_indptr, const int32_t* d_indices, const void* d_values, const double* d_mean,
                        const double* d_std, const double* d_z, double lo, double hi, void* d_out, void* stream) {
  MU_REQUIRE(n >= 0 && d >= 0 && nnz >= 0, "negative shape");
  MU_REQUIRE(dtype == MU_DTYPE_F32 || dtype == MU_DTYPE_F64, "dtype must be f32 or f64");
  MU_REQUIRE(row_lo >= 0 && row_lo <= row_hi && row_hi <= n, "0 <= row_lo <= row_hi <= n");
  MU_REQUIRE(lo <= hi, "lo <= hi (the infinities for a side that is not clipped)");
  if (row_hi == row_lo || d == 0) return MU_OK;
  MU_REQUIRE(d_indptr && d_mean && d_std && d_z && d_out && (nnz == 0 || (d_indices && d_values)), "null pointer");
  const unsigned grid = wave_grid(row_hi - row_lo, kScaleWaves, kScaleBlocksPerCu);
  hipStream_t st = (hipStream_t)stream;
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    const bool vec = (uintptr_t)d_out % 16 == 0 && (d * (int64_t)sizeof(T)) % 16 == 0;
    by_index<2>(vec, [&](auto v) {
      hipLaunchKernelGGL((k_scale_dense_rows<T, (v() != 0)>), dim3(grid), dim3(kScaleThreads), 0, st, row_lo, row_hi, d,
                         nnz, d_indptr, d_indices, (const T*)d_values, d_mean, d_std, d_z, lo, hi, (T*)d_out);
    });
  });
  MU_CHECK_LAUNCH();
  return MU_OK;
}

}  // extern "C"
