// The cell-long steps of muon_amd.pp.harmony_integrate (the statement is the package's own,
// muon_amd/_core/harmony.py), f64 on the matrix cores: k_har_gram and k_har_assign, the inner loop of the k-means
// rounds, described here; k_har_objective and k_har_correct, described where they stand.  v_mfma_f64_16x16x4_f64, operand maps as in
// common.hpp:  A operand lane l = A[i = l & 15][k = l >> 4],  B operand lane l = B[k = l >> 4][j = l & 15],  C/D reg r
// of lane l = C[row = (l >> 4) + 4 r][col = l & 15].
//
// k_har_gram: out[s] = R[rows of segment s]^T Z[rows of segment s], [kp x dp] per segment (kp, dp: K and d rounded up
//   to 16).  The rows of segment s are seg[s] .. seg[s + 1] - 1, or idx[seg[s]] .. idx[seg[s + 1] - 1] with an index
//   list.  The segment offsets travel BY VALUE in the kernel's arguments (at most 64 segments): the host has checked
//   them, the grid is a function of the shapes.  Workgroup (p, s) = four waves walks the 64-row tiles p, p + P, ... of
//   segment s.  i = cluster, j = column of Z, k = row: the A operand, R[row 4 u + (l >> 4)][cluster 16 b + (l & 15)],
//   is used by one wave only (wave w owns the cluster blocks w and w + 4) and goes from global memory straight to a
//   register, 128 contiguous bytes per row; the B operand is the staged tile of Z, which all four waves share (row
//   stride dp * 8 + 16 bytes: the two rows a half wave reads lie 16 bytes apart modulo the bank row).  Rows past the
//   segment's end, clusters at or past K, columns at or past d and rows whose index is outside [0, n) are ZEROED BY
//   INDEX (a select on a clamped address: NaN in the padding of an operand does no harm, and no address leaves the
//   operands).  Every workgroup leaves its partial [kp x dp] in its slot; k_har_reduce adds the P slots of a segment
//   in slot order.  No float atomics: two calls agree byte for byte.
//
// k_har_assign: for the cells idx[0 .. nb) (or 0 .. nb - 1), cell c with level code g:
//     D_k = 2 (1 - Zc_c . Y_k)    t_k = -D_k / sigma_k    s_k = exp(t_k - max_k t_k)    w_k = s_k F[k][g]
//     R[c][k] = w_k / sum_k w_k   (k < K),    R[c][k] = 0   (K <= k < kp)
//   A wave owns 16 cells and ALL cluster blocks, so a cell's maximum and sum never leave the wave: i = cell, j =
//   cluster, k = column.  The C/D map leaves cell (l >> 4) + 4 r x cluster 16 b + (l & 15) in register r of block b:
//   a cell's clusters lie in the KB registers of 16 consecutive lanes (four xor steps), and a row of R is written as
//   128-byte pieces.  Y [K x d] is staged once per workgroup (row stride dp * 8 + 16: 16 clusters x one f64 on 16
//   distinct 4-bank groups), masked by index; the A operand, one f64 per lane of the cell's row of Zc, comes straight
//   from global memory.  Built with -ffp-contract=off: the exponent is -D / sigma - max as the statement writes it, a
//   true division and no fused product, so that with exact distances the weights are those of the NumPy statement up
//   to libm's exp.  Every cell's row is written by one wave, once: no atomics, two calls agree byte for byte.
#include "common.hpp"

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int kHarMaxK = 128;    // clusters
constexpr int kHarMaxD = 64;     // columns of the basis
constexpr int kHarMaxB = 64;     // levels of the key = segments of a gram
constexpr int kHarTile = 64;     // rows per tile of the gram
constexpr int kHarSlots = 512;   // partial slots of one gram, all segments together

struct HarSegs {
  int64_t p[kHarMaxB + 1];
};

__device__ __forceinline__ int64_t clamp_row(int64_t i, int64_t n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

template <int KW, int DB>
__global__ __launch_bounds__(256) void k_har_gram(HarSegs segs, int64_t n, int K, int kp, int d,
                                                  const double* __restrict__ R, int64_t ldr,
                                                  const double* __restrict__ Z, int64_t ldz,
                                                  const int64_t* __restrict__ idx, double* __restrict__ work) {
  constexpr int DP = 16 * DB;
  constexpr int RS = DP * 8 + 16;  // LDS row stride in bytes
  __shared__ __attribute__((aligned(16))) char zs[kHarTile * RS];
  const int lane = threadIdx.x & 63;
  const int wave = uniform32(threadIdx.x >> 6);
  const int lr = lane >> 4, lc = lane & 15;
  const int s = blockIdx.y;
  const int64_t lo = segs.p[s], hi = segs.p[s + 1];
  const int64_t n_tiles = (hi - lo + kHarTile - 1) / kHarTile;

  d4 acc[KW][DB];
#pragma unroll
  for (int w = 0; w < KW; ++w)
#pragma unroll
    for (int c = 0; c < DB; ++c) acc[w][c] = d4{0, 0, 0, 0};

  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t r0 = lo + tile * kHarTile;
    __syncthreads();  // the previous tile has been read
    for (int e = threadIdx.x; e < kHarTile * DP; e += 256) {
      const int row = e / DP, col = e % DP;
      const int64_t j = r0 + row;
      const int64_t jj = j < hi ? j : hi - 1;  // (hi > lo >= 0 here: in bounds)
      const int64_t i = idx ? idx[jj] : jj;
      const bool ok = j < hi && col < d && i >= 0 && i < n;
      const double v = Z[clamp_row(i, n) * ldz + (col < d ? col : d - 1)];
      *reinterpret_cast<double*>(&zs[row * RS + col * 8]) = ok ? v : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < KW; ++w) {
      const int b = wave + 4 * w;
      if (16 * b >= kp) continue;  // (wave-uniform)
      const int comp = 16 * b + lc;
      const int cc = comp < K ? comp : K - 1;
#pragma unroll 4
      for (int u = 0; u < kHarTile / 4; ++u) {
        const int64_t j = r0 + 4 * u + lr;
        const int64_t jj = j < hi ? j : hi - 1;
        const int64_t i = idx ? idx[jj] : jj;
        const bool ok = j < hi && comp < K && i >= 0 && i < n;
        const double v = R[clamp_row(i, n) * ldr + cc];
        const double a = ok ? v : 0.0;
#pragma unroll
        for (int c = 0; c < DB; ++c) {
          const double z = *reinterpret_cast<const double*>(&zs[(4 * u + lr) * RS + (16 * c + lc) * 8]);
          acc[w][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, z, acc[w][c], 0, 0, 0);
        }
      }
    }
  }

  double* slot = work + ((int64_t)s * gridDim.x + blockIdx.x) * ((int64_t)kp * DP);
#pragma unroll
  for (int w = 0; w < KW; ++w) {
    const int b = wave + 4 * w;
    if (16 * b >= kp) continue;
#pragma unroll
    for (int c = 0; c < DB; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) slot[(16 * b + lr + 4 * r) * DP + 16 * c + lc] = acc[w][c][r];
  }
}

// out[s][e] = the sum of segment s's P slots, in slot order; one thread per element
__global__ __launch_bounds__(256) void k_har_reduce(int64_t per, int P, const double* __restrict__ work,
                                                    double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= per) return;
  const double* src = work + (int64_t)blockIdx.y * P * per + e;
  double acc = 0.0;
  for (int p = 0; p < P; ++p) acc += src[(int64_t)p * per];
  out[(int64_t)blockIdx.y * per + e] = acc;
}

// rows [K x d] of a small matrix into LDS, row stride DP * 8 + 16 bytes, rows at or past K and columns at or past d zero
template <int ROWS, int DB>
__device__ __forceinline__ void har_stage(char* lds, const double* __restrict__ M, int K, int d) {
  constexpr int DP = 16 * DB;
  constexpr int RS = DP * 8 + 16;
  for (int e = threadIdx.x; e < ROWS * DP; e += 256) {
    const int k = e / DP, col = e % DP;
    const bool ok = k < K && col < d;
    const double v = M[(int64_t)(k < K ? k : K - 1) * d + (col < d ? col : d - 1)];
    *reinterpret_cast<double*>(&lds[k * RS + col * 8]) = ok ? v : 0.0;
  }
}

// acc[b] = Zc[16 cells of the tile] . Y[cluster block b]^T from the staged Y: register r of block b is cell lr + 4 r
// of the tile x cluster 16 b + lc.  The A operand: cell lc of the tile, column 4 u + lr of its row.
template <int KB, int DB>
__device__ __forceinline__ void har_dots(const char* ys, int64_t tile, int64_t nb, int64_t n, int kp, int d,
                                         const double* __restrict__ Zc, int64_t ldz, const int64_t* __restrict__ idx,
                                         d4 (&acc)[KB]) {
  constexpr int DP = 16 * DB;
  constexpr int RS = DP * 8 + 16;
  const int lane = threadIdx.x & 63;
  const int lr = lane >> 4, lc = lane & 15;
  const int64_t ja = tile * 16 + lc;
  const int64_t jja = ja < nb ? ja : nb - 1;
  const int64_t ia = idx ? idx[jja] : jja;
  const bool oka = ja < nb && ia >= 0 && ia < n;
  const double* zrow = Zc + clamp_row(ia, n) * ldz;
#pragma unroll
  for (int b = 0; b < KB; ++b) acc[b] = d4{0, 0, 0, 0};
#pragma unroll
  for (int u = 0; u < DP / 4; ++u) {
    const int col = 4 * u + lr;
    const double v = zrow[col < d ? col : d - 1];
    const double a = (oka && col < d) ? v : 0.0;
#pragma unroll
    for (int b = 0; b < KB; ++b) {
      if (16 * b >= kp) continue;  // (uniform)
      const double y = *reinterpret_cast<const double*>(&ys[(16 * b + lc) * RS + col * 8]);
      acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, y, acc[b], 0, 0, 0);
    }
  }
}

template <int KB, int DB>
__global__ __launch_bounds__(256) void k_har_assign(int64_t n, int K, int kp, int d, int B, int64_t nb,
                                                    const double* __restrict__ Zc, int64_t ldz,
                                                    const double* __restrict__ Y, const double* __restrict__ sigma,
                                                    const double* __restrict__ F, const int32_t* __restrict__ codes,
                                                    const int64_t* __restrict__ idx, double* __restrict__ R,
                                                    int64_t ldr) {
  constexpr int DP = 16 * DB;
  constexpr int KP = 16 * KB;
  constexpr int RS = DP * 8 + 16;  // LDS row stride in bytes
  __shared__ __attribute__((aligned(16))) char ys[KP * RS];
  const int lane = threadIdx.x & 63;
  const int wave = uniform32(threadIdx.x >> 6);
  const int lr = lane >> 4, lc = lane & 15;

  har_stage<KP, DB>(ys, Y, K, d);
  __syncthreads();

  double sig[KB];
#pragma unroll
  for (int b = 0; b < KB; ++b) {
    const int k = 16 * b + lc;
    sig[b] = sigma[k < K ? k : K - 1];
  }

  const int64_t n_tiles = (nb + 15) / 16;
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < n_tiles; tile += (int64_t)gridDim.x * 4) {
    d4 acc[KB];
    har_dots<KB, DB>(ys, tile, nb, n, kp, d, Zc, ldz, idx, acc);
    // register r of block b: cell lr + 4 r of the tile, cluster 16 b + lc
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t j = tile * 16 + lr + 4 * r;
      const int64_t jj = j < nb ? j : nb - 1;
      const int64_t i = idx ? idx[jj] : jj;
      const bool okc = j < nb && i >= 0 && i < n;
      const int64_t ic = clamp_row(i, n);
      int g = codes[ic];
      g = g < 0 ? 0 : (g >= B ? B - 1 : g);
      double t[KB];
      double m = -INFINITY;
#pragma unroll
      for (int b = 0; b < KB; ++b) {
        const bool valid = 16 * b + lc < K;
        const double dist = 2.0 * (1.0 - acc[b][r]);
        t[b] = valid ? -dist / sig[b] : -INFINITY;
        m = fmax(m, t[b]);
      }
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) m = fmax(m, __shfl_xor(m, off, 64));
      double sum = 0.0;
#pragma unroll
      for (int b = 0; b < KB; ++b) {
        const int k = 16 * b + lc;
        const bool valid = k < K;
        const double f = F[(int64_t)(valid ? k : K - 1) * B + g];
        const double w = exp(t[b] - m) * f;
        t[b] = valid ? w : 0.0;
        sum += t[b];
      }
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) sum += __shfl_xor(sum, off, 64);
      if (okc) {
#pragma unroll
        for (int b = 0; b < KB; ++b) {
          if (16 * b >= kp) continue;
          const bool valid = 16 * b + lc < K;
          R[ic * ldr + 16 * b + lc] = valid ? t[b] / sum : 0.0;
        }
      }
    }
  }
}

// The three terms of the objective from one read of R: per cell c (all n, in order) and cluster k < K, with r =
// R[c][k], D as in k_har_assign and g the cell's level:  r D,  sigma_k r log r (0 log 0 := 0),  sigma_k r G[k][g].
// A lane adds its own terms over its tiles, the wave's lanes are added by the xor butterfly, the four waves in order;
// the workgroup's three sums go to its slot, k_har_objective_reduce adds the slots in order.
template <int KB, int DB>
__global__ __launch_bounds__(256) void k_har_objective(int64_t n, int K, int kp, int d, int B,
                                                       const double* __restrict__ Zc, int64_t ldz,
                                                       const double* __restrict__ Y, const double* __restrict__ R,
                                                       int64_t ldr, const double* __restrict__ sigma,
                                                       const double* __restrict__ G, const int32_t* __restrict__ codes,
                                                       double* __restrict__ work) {
  constexpr int DP = 16 * DB;
  constexpr int KP = 16 * KB;
  constexpr int RS = DP * 8 + 16;
  __shared__ __attribute__((aligned(16))) char ys[KP * RS + 4 * 3 * 8];
  double* red = reinterpret_cast<double*>(&ys[KP * RS]);
  const int lane = threadIdx.x & 63;
  const int wave = uniform32(threadIdx.x >> 6);
  const int lr = lane >> 4, lc = lane & 15;

  har_stage<KP, DB>(ys, Y, K, d);
  __syncthreads();

  double sig[KB];
#pragma unroll
  for (int b = 0; b < KB; ++b) {
    const int k = 16 * b + lc;
    sig[b] = sigma[k < K ? k : K - 1];
  }
  double t1 = 0.0, t2 = 0.0, t3 = 0.0;
  const int64_t n_tiles = (n + 15) / 16;
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < n_tiles; tile += (int64_t)gridDim.x * 4) {
    d4 acc[KB];
    har_dots<KB, DB>(ys, tile, n, n, kp, d, Zc, ldz, nullptr, acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t j = tile * 16 + lr + 4 * r;
      const int64_t ic = j < n ? j : n - 1;
      int g = codes[ic];
      g = g < 0 ? 0 : (g >= B ? B - 1 : g);
#pragma unroll
      for (int b = 0; b < KB; ++b) {
        if (16 * b >= kp) continue;
        const int k = 16 * b + lc;
        const bool valid = k < K && j < n;
        const int kc = k < K ? k : K - 1;
        const double rv = R[ic * ldr + kc];
        const double rr = valid ? rv : 0.0;
        const double dist = 2.0 * (1.0 - acc[b][r]);
        const double lg = rr > 0.0 ? rr * log(rr) : 0.0;
        const double gg = G[(int64_t)kc * B + g];
        t1 += valid ? rr * dist : 0.0;
        t2 += valid ? sig[b] * lg : 0.0;
        t3 += valid ? sig[b] * (rr * gg) : 0.0;
      }
    }
  }
  t1 = wave_sum_all(t1);
  t2 = wave_sum_all(t2);
  t3 = wave_sum_all(t3);
  if (lane == 0) {
    red[wave * 3 + 0] = t1;
    red[wave * 3 + 1] = t2;
    red[wave * 3 + 2] = t3;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int t = threadIdx.x;
    work[(int64_t)blockIdx.x * 3 + t] = ((red[t] + red[3 + t]) + red[6 + t]) + red[9 + t];
  }
}

__global__ __launch_bounds__(64) void k_har_objective_reduce(int slots, const double* __restrict__ work,
                                                             double* __restrict__ out) {
  if (threadIdx.x >= 3) return;
  double acc = 0.0;
  for (int s = 0; s < slots; ++s) acc += work[(int64_t)s * 3 + threadIdx.x];
  out[threadIdx.x] = acc;
}

// Zcorr[c] = Z[c] - R[c][:K] W[g] and Zc[c] = Zcorr[c] / |Zcorr[c]| for the cells of level g = blockIdx.y, the rows
// segs.p[g] .. segs.p[g + 1] - 1 (the cells are sorted by level).  i = cell, j = column, k = cluster: the B operand,
// W[g] [K x d], is staged once per workgroup; the A operand R[cell lc][cluster 4 u + lr] comes straight from global
// memory.  A cell's squared norm is added over the DB registers of 16 consecutive lanes (four xor steps).
template <int KB, int DB>
__global__ __launch_bounds__(256) void k_har_correct(HarSegs segs, int K, int d, const double* __restrict__ Z,
                                                     int64_t ldz, const double* __restrict__ R, int64_t ldr,
                                                     const double* __restrict__ W, double* __restrict__ Zcorr,
                                                     double* __restrict__ Zcn, int64_t ldo) {
  constexpr int DP = 16 * DB;
  constexpr int KP = 16 * KB;
  constexpr int RS = DP * 8 + 16;
  __shared__ __attribute__((aligned(16))) char ws[KP * RS];
  const int lane = threadIdx.x & 63;
  const int wave = uniform32(threadIdx.x >> 6);
  const int lr = lane >> 4, lc = lane & 15;
  const int g = blockIdx.y;
  const int64_t lo = segs.p[g], hi = segs.p[g + 1];
  if (hi <= lo) return;  // (the whole workgroup)
  har_stage<KP, DB>(ws, W + (int64_t)g * K * d, K, d);
  __syncthreads();
  const int64_t n_tiles = (hi - lo + 15) / 16;
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < n_tiles; tile += (int64_t)gridDim.x * 4) {
    const int64_t ja = lo + tile * 16 + lc;
    const bool oka = ja < hi;
    const double* rrow = R + (oka ? ja : hi - 1) * ldr;
    d4 acc[DB];
#pragma unroll
    for (int c = 0; c < DB; ++c) acc[c] = d4{0, 0, 0, 0};
#pragma unroll 4
    for (int u = 0; u < KP / 4; ++u) {
      const int k = 4 * u + lr;
      const double v = rrow[k < K ? k : K - 1];
      const double a = (oka && k < K) ? v : 0.0;
#pragma unroll
      for (int c = 0; c < DB; ++c) {
        const double w = *reinterpret_cast<const double*>(&ws[k * RS + (16 * c + lc) * 8]);
        acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, w, acc[c], 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t j = lo + tile * 16 + lr + 4 * r;
      const bool okc = j < hi;
      const int64_t jc = okc ? j : hi - 1;
      double o[DB];
      double ss = 0.0;
#pragma unroll
      for (int c = 0; c < DB; ++c) {
        const int col = 16 * c + lc;
        const double z = Z[jc * ldz + (col < d ? col : d - 1)];
        o[c] = col < d ? z - acc[c][r] : 0.0;
        ss += o[c] * o[c];
      }
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) ss += __shfl_xor(ss, off, 64);
      const double nrm = sqrt(ss);
      if (okc) {
#pragma unroll
        for (int c = 0; c < DB; ++c) {
          const int col = 16 * c + lc;
          if (col < d) {
            Zcorr[jc * ldo + col] = o[c];
            Zcn[jc * ldo + col] = o[c] / nrm;
          }
        }
      }
    }
  }
}

inline int har_pad(int k) { return (k + 15) / 16 * 16; }

// slots per segment: a function of (rows, segments) alone
inline int har_slots(int64_t m, int n_seg) {
  int64_t p = (m + kHarTile - 1) / kHarTile;
  const int64_t cap = kHarSlots / n_seg > 1 ? kHarSlots / n_seg : 1;
  if (p > cap) p = cap;
  return (int)(p < 1 ? 1 : p);
}

}  // namespace

extern "C" {

int mu_harmony_max_clusters(void) { return kHarMaxK; }
int mu_harmony_max_dims(void) { return kHarMaxD; }
int mu_harmony_max_levels(void) { return kHarMaxB; }

size_t mu_harmony_gram_worksize(int64_t m, int n_seg, int K, int d) {
  if (m < 0 || n_seg < 1 || n_seg > kHarMaxB || K < 1 || K > kHarMaxK || d < 1 || d > kHarMaxD) return 0;
  return (size_t)n_seg * har_slots(m, n_seg) * har_pad(K) * har_pad(d) * sizeof(double);
}

int mu_harmony_gram_f64(int64_t n, int64_t m, int K, int d, const double* d_R, int64_t ldr, const double* d_Z,
                        int64_t ldz, const int64_t* d_idx, int n_seg, const int64_t* h_seg_ptr, double* d_out,
                        void* d_work, size_t work_bytes, void* stream) {
  MU_REQUIRE(n >= 0 && m >= 0, "negative shape");
  MU_REQUIRE(K >= 1 && K <= kHarMaxK, "K must be 1..128");
  MU_REQUIRE(d >= 1 && d <= kHarMaxD, "d must be 1..64");
  MU_REQUIRE(n_seg >= 1 && n_seg <= kHarMaxB, "the number of segments must be 1..64");
  MU_REQUIRE(h_seg_ptr && d_out && (m == 0 || (d_R && d_Z)), "null pointer");
  MU_REQUIRE(d_idx || m <= n, "without an index list the rows are 0 .. m - 1: m must not exceed n");
  MU_REQUIRE(ldr >= K && ldz >= d, "ldr must cover K and ldz must cover d");
  HarSegs segs;
  for (int s = 0; s <= kHarMaxB; ++s) segs.p[s] = 0;
  MU_REQUIRE(h_seg_ptr[0] >= 0 && h_seg_ptr[n_seg] <= m, "seg_ptr must lie in [0, m]");
  for (int s = 0; s < n_seg; ++s)
    MU_REQUIRE(h_seg_ptr[s] <= h_seg_ptr[s + 1], "seg_ptr must not descend");
  for (int s = 0; s <= n_seg; ++s) segs.p[s] = h_seg_ptr[s];
  hipStream_t st = (hipStream_t)stream;
  const int kp = har_pad(K), dp = har_pad(d);
  const int64_t per = (int64_t)kp * dp;
  if (m == 0 || n == 0) {
    MU_CHECK_HIP(hipMemsetAsync(d_out, 0, (size_t)n_seg * per * sizeof(double), st));
    return MU_OK;
  }
  MU_REQUIRE(d_work && work_bytes >= mu_harmony_gram_worksize(m, n_seg, K, d), "work buffer too small");
  const int P = har_slots(m, n_seg);
  double* work = (double*)d_work;
  by_width<64, 128>(K, [&](auto kw) {
    by_width<16, 32, 48, 64>(d, [&](auto dw) {
      hipLaunchKernelGGL((k_har_gram<decltype(kw)::value / 64, decltype(dw)::value / 16>), dim3(P, n_seg), dim3(256), 0,
                         st, segs, n, K, kp, d, d_R, ldr, d_Z, ldz, d_idx, work);
    });
  });
  MU_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_har_reduce, dim3((unsigned)((per + 255) / 256), n_seg), dim3(256), 0, st, per, P,
                     (const double*)work, d_out);
  MU_CHECK_LAUNCH();
  return MU_OK;
}

int mu_harmony_assign_f64(int64_t n, int K, int d, int B, int64_t nb, const double* d_Zc, int64_t ldz,
                          const double* d_Y, const double* d_sigma, const double* d_F, const int32_t* d_codes,
                          const int64_t* d_idx, double* d_R, int64_t ldr, void* stream) {
  MU_REQUIRE(n >= 0 && nb >= 0, "negative shape");
  MU_REQUIRE(K >= 1 && K <= kHarMaxK, "K must be 1..128");
  MU_REQUIRE(d >= 1 && d <= kHarMaxD, "d must be 1..64");
  MU_REQUIRE(B >= 1 && B <= kHarMaxB, "B must be 1..64");
  MU_REQUIRE(d_idx || nb <= n, "without an index list the cells are 0 .. nb - 1: nb must not exceed n");
  MU_REQUIRE(d_Zc && d_Y && d_sigma && d_F && d_codes && d_R, "null pointer");
  if (nb == 0 || n == 0) return MU_OK;
  const int kp = har_pad(K);
  MU_REQUIRE(ldr >= kp && ldz >= d, "ldr must cover K rounded up to a multiple of 16 and ldz must cover d");
  hipStream_t st = (hipStream_t)stream;
  const unsigned blocks = wave_grid((nb + 15) / 16, 4, 2);
  by_width<16, 32, 64, 128>(K, [&](auto kw) {
    by_width<16, 32, 48, 64>(d, [&](auto dw) {
      hipLaunchKernelGGL((k_har_assign<decltype(kw)::value / 16, decltype(dw)::value / 16>), dim3(blocks), dim3(256), 0,
                         st, n, K, kp, d, B, nb, d_Zc, ldz, d_Y, d_sigma, d_F, d_codes, d_idx, d_R, ldr);
    });
  });
  MU_CHECK_LAUNCH();
  return MU_OK;
}

size_t mu_harmony_objective_worksize(int64_t n) {
  if (n < 0) return 0;
  int64_t blocks = (n + 63) / 64;
  if (blocks > kHarSlots) blocks = kHarSlots;
  if (blocks < 1) blocks = 1;
  return (size_t)blocks * 3 * sizeof(double);
}

int mu_harmony_objective_f64(int64_t n, int K, int d, int B, const double* d_Zc, int64_t ldz, const double* d_Y,
                             const double* d_R, int64_t ldr, const double* d_sigma, const double* d_G,
                             const int32_t* d_codes, double* d_out, void* d_work, size_t work_bytes, void* stream) {
  MU_REQUIRE(n >= 0, "negative shape");
  MU_REQUIRE(K >= 1 && K <= kHarMaxK, "K must be 1..128");
  MU_REQUIRE(d >= 1 && d <= kHarMaxD, "d must be 1..64");
  MU_REQUIRE(B >= 1 && B <= kHarMaxB, "B must be 1..64");
  MU_REQUIRE(d_Zc && d_Y && d_R && d_sigma && d_G && d_codes && d_out, "null pointer");
  MU_REQUIRE(ldr >= K && ldz >= d, "ldr must cover K and ldz must cover d");
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {
    MU_CHECK_HIP(hipMemsetAsync(d_out, 0, 3 * sizeof(double), st));
    return MU_OK;
  }
  MU_REQUIRE(d_work && work_bytes >= mu_harmony_objective_worksize(n), "work buffer too small");
  const int blocks = (int)(mu_harmony_objective_worksize(n) / (3 * sizeof(double)));  // a function of n alone
  const int kp = har_pad(K);
  double* work = (double*)d_work;
  by_width<16, 32, 64, 128>(K, [&](auto kw) {
    by_width<16, 32, 48, 64>(d, [&](auto dw) {
      hipLaunchKernelGGL((k_har_objective<decltype(kw)::value / 16, decltype(dw)::value / 16>), dim3(blocks), dim3(256),
                         0, st, n, K, kp, d, B, d_Zc, ldz, d_Y, d_R, ldr, d_sigma, d_G, d_codes, work);
    });
  });
  MU_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_har_objective_reduce, dim3(1), dim3(64), 0, st, blocks, (const double*)work, d_out);
  MU_CHECK_LAUNCH();
  return MU_OK;
}

int mu_harmony_correct_f64(int64_t n, int K, int d, int B, const double* d_Z, int64_t ldz, const double* d_R,
                           int64_t ldr, const double* d_W, const int64_t* h_seg_ptr, double* d_Zcorr, double* d_Zc,
                           int64_t ldo, void* stream) {
  MU_REQUIRE(n >= 0, "negative shape");
  MU_REQUIRE(K >= 1 && K <= kHarMaxK, "K must be 1..128");
  MU_REQUIRE(d >= 1 && d <= kHarMaxD, "d must be 1..64");
  MU_REQUIRE(B >= 1 && B <= kHarMaxB, "B must be 1..64");
  MU_REQUIRE(h_seg_ptr && d_Z && d_R && d_W && d_Zcorr && d_Zc, "null pointer");
  MU_REQUIRE(ldr >= K && ldz >= d && ldo >= d, "ldr must cover K, ldz and ldo must cover d");
  HarSegs segs;
  for (int s = 0; s <= kHarMaxB; ++s) segs.p[s] = 0;
  MU_REQUIRE(h_seg_ptr[0] == 0 && h_seg_ptr[B] == n, "seg_ptr must run from 0 to n");
  for (int s = 0; s < B; ++s) MU_REQUIRE(h_seg_ptr[s] <= h_seg_ptr[s + 1], "seg_ptr must not descend");
  for (int s = 0; s <= B; ++s) segs.p[s] = h_seg_ptr[s];
  if (n == 0) return MU_OK;
  hipStream_t st = (hipStream_t)stream;
  int64_t P = (n + 63) / 64;
  const int64_t cap = 1024 / B > 1 ? 1024 / B : 1;
  if (P > cap) P = cap;
  by_width<16, 32, 64, 128>(K, [&](auto kw) {
    by_width<16, 32, 48, 64>(d, [&](auto dw) {
      hipLaunchKernelGGL((k_har_correct<decltype(kw)::value / 16, decltype(dw)::value / 16>), dim3((unsigned)P, B),
                         dim3(256), 0, st, segs, K, d, d_Z, ldz, d_R, ldr, d_W, d_Zcorr, d_Zc, ldo);
    });
  });
  MU_CHECK_LAUNCH();
  return MU_OK;
}

}  // extern "C"
