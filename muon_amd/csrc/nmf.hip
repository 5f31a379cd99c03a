// One coordinate-descent sweep of bounded NMF over the rows of a factor W [rows x k] (row-major f64, leading dimension
// ldw), fused (the reference, /root/reference/muon/_atac/preproc.py:155-236, hands the arithmetic to
// scOpen's MF module, which is scikit-learn's coordinate-descent solver: _cdnmf_fast.pyx::_update_cdnmf_fast).
//
// Per row i, for t = 0 .. k-1 in order:
//   b    = B[i,t] (* bscale[i]) (- l1 when l1 != 0)
//   grad = -b;  grad = grad + G[t,r] * W[i,r]  for r = 0 .. k-1 ascending, product and sum TWO roundings (the file is
//          built with -ffp-contract=off), on the row's already-updated entries
//   pg   = W[i,t] == 0 ? min(0, grad) : grad;   v_i += |pg|
//   if G[t,t] != 0:  W[i,t] = max(W[i,t] - grad / G[t,t], 0)
// That is scikit-learn's loop nest turned inside out (rows are independent): the updated factor is bit-equal to a
// NumPy restatement in this order.
//
// Map: a workgroup is ONE wave and walks 64-row tiles grid-stride; lane l owns row l of the tile and keeps its KP
// (= k rounded up to 16 / 32 / 64) values in registers for the whole sweep, as KP / 16 vectors of 16: the coordinate t
// is a wave-uniform loop counter, so reading and writing W[i,t] is a register-indexed move, not a select chain.  G
// lies in LDS, padded to KP x KP with zeros BY INDEX, and is read at wave-uniform addresses (broadcast).  One LDS tile
// [64 x KP, row stride KP + 1 doubles: a lane per row reads conflict free] is used four times per tile of rows:
//   1. W comes in with coalesced 8-byte loads (rows >= `rows` and columns >= k are zero BY INDEX: NaN in the padding of
//      W or B reaches nothing), each lane takes its row;   2. B comes in the same way, the sweep reads b from it;
//   3. the updated rows go back: the Gram matrix of the tile is accumulated from it on the matrix cores
//      (v_mfma_f64_16x16x4_f64, operand maps in common.hpp: both operands are tile[row = 4 s + (l >> 4)][16 a + (l & 15)]
//      - the blocks on and above the diagonal only) and W is written out coalesced (columns < k only);
//   4. oscale[i] * Wnew[i,:] goes through it to Wout (columns k .. ldo-1 written as zero).
// The wave's LDS accesses issue in order: wave_lds_sync, no workgroup barrier.
//
// No float atomics: a workgroup writes its Gram blocks and its violation (per lane: v_i added tile after tile in walk
// order; then wave_sum's tree) to its slot of the workspace, k_nmf_reduce adds the slots in slot order (four fixed
// quarters, then their sum in order) and mirrors the blocks below the diagonal.  The grid is min(ceil(rows / 64),
// max_blocks or 512): a function of (rows, max_blocks) alone, so two calls agree bit for bit.
#include "common.hpp"

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d16 __attribute__((ext_vector_type(16)));

constexpr int kNmfMaxK = 64;
constexpr int kNmfTile = 64;     // rows per tile: a lane each
constexpr int kNmfBlocks = 512;  // default cap of the grid

template <int KP>
__global__ __launch_bounds__(64) void k_nmf_sweep(int64_t rows, int k, double* __restrict__ W, int64_t ldw,
                                                  const double* __restrict__ B, int64_t ldb,
                                                  const double* __restrict__ bscale, const double* __restrict__ G,
                                                  double l1, const double* __restrict__ oscale,
                                                  double* __restrict__ Wout, int64_t ldo, double* __restrict__ work) {
  constexpr int NB = KP / 16;
  constexpr int RS = KP + 1;  // LDS row stride in doubles
  __shared__ double tile[kNmfTile * RS];
  __shared__ double gs[KP * KP];
  const int lane = threadIdx.x;
  const int lr = lane >> 4, lc = lane & 15;

#pragma unroll 4
  for (int e = lane; e < KP * KP; e += 64) {
    const int r = e / KP, c = e % KP;
    gs[e] = (r < k && c < k) ? G[r * k + c] : 0.0;
  }

  d4 acc[NB * (NB + 1) / 2];
#pragma unroll
  for (int u = 0; u < NB * (NB + 1) / 2; ++u) acc[u] = d4{0, 0, 0, 0};
  double viol = 0.0;

  // a [64 x KP] piece of a row-major matrix <-> the tile, 64 consecutive doubles per instruction
  auto stage = [&](const double* __restrict__ src, int64_t ld, int64_t row0) {
#pragma unroll 8
    for (int i = 0; i < KP; ++i) {
      const int e = lane + 64 * i;
      const int r = e / KP, c = e % KP;
      const bool in = row0 + r < rows && c < k;
      tile[r * RS + c] = in ? src[(row0 + r) * ld + c] : 0.0;
    }
  };

  const int64_t n_tiles = (rows + kNmfTile - 1) / kNmfTile;
  for (int64_t ti = blockIdx.x; ti < n_tiles; ti += gridDim.x) {
    const int64_t row0 = ti * kNmfTile;
    const int64_t row = row0 + lane;
    const bool live = row < rows;

    wave_lds_sync();  // (first tile: G is in LDS; later: the previous tile has been read)
    stage(W, ldw, row0);
    wave_lds_sync();
    d16 w[NB];
#pragma unroll
    for (int c = 0; c < KP; ++c) w[c / 16][c % 16] = tile[lane * RS + c];
    wave_lds_sync();
    stage(B, ldb, row0);
    wave_lds_sync();

    const double bs = (bscale != nullptr && live) ? bscale[row] : 1.0;
    double vi = 0.0;
#pragma unroll
    for (int tb = 0; tb < NB; ++tb) {
      const int tn = k - 16 * tb < 16 ? k - 16 * tb : 16;  // (wave-uniform)
      for (int tt = 0; tt < tn; ++tt) {
        const int t = 16 * tb + tt;
        double b = tile[lane * RS + t];
        if (bscale != nullptr) b = b * bs;
        if (l1 != 0.0) b = b - l1;
        const double* g = gs + t * KP;
        double grad = -b;
#pragma unroll
        for (int r = 0; r < KP; ++r) grad = grad + g[r] * w[r / 16][r % 16];
        const double wt = w[tb][tt];
        const double pg = wt == 0.0 ? fmin(0.0, grad) : grad;
        vi += fabs(pg);
        const double hess = g[t];
        if (hess != 0.0) w[tb][tt] = fmax(wt - grad / hess, 0.0);
      }
    }
    viol += live ? vi : 0.0;

    wave_lds_sync();  // every lane has read its b
#pragma unroll
    for (int c = 0; c < KP; ++c) tile[lane * RS + c] = live ? w[c / 16][c % 16] : 0.0;
    wave_lds_sync();

#pragma unroll 4
    for (int s = 0; s < kNmfTile / 4; ++s) {
      double val[NB];
#pragma unroll
      for (int a = 0; a < NB; ++a) val[a] = tile[(4 * s + lr) * RS + 16 * a + lc];
      int u = 0;
#pragma unroll
      for (int a = 0; a < NB; ++a)
#pragma unroll
        for (int b = a; b < NB; ++b, ++u) acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(val[a], val[b], acc[u], 0, 0, 0);
    }
#pragma unroll 8
    for (int i = 0; i < KP; ++i) {
      const int e = lane + 64 * i;
      const int r = e / KP, c = e % KP;
      if (row0 + r < rows && c < k) W[(row0 + r) * ldw + c] = tile[r * RS + c];
    }

    if (Wout != nullptr) {
      if (oscale != nullptr) {
        const double os = live ? oscale[row] : 0.0;
        wave_lds_sync();  // the Gram and the write-out have read the tile
#pragma unroll
        for (int c = 0; c < KP; ++c) tile[lane * RS + c] = live ? os * w[c / 16][c % 16] : 0.0;
        wave_lds_sync();
      }
      if (ldo == KP) {
#pragma unroll 8
        for (int i = 0; i < KP; ++i) {
          const int e = lane + 64 * i;
          const int r = e / KP, c = e % KP;
          if (row0 + r < rows) Wout[(row0 + r) * ldo + c] = tile[r * RS + c];  // (columns k .. KP-1 of the tile are zero)
        }
      } else {
        const int64_t nr = rows - row0 < kNmfTile ? rows - row0 : kNmfTile;
        for (int64_t e = lane; e < nr * ldo; e += 64) {
          const int64_t r = e / ldo, c = e % ldo;
          Wout[row0 * ldo + e] = c < k ? tile[r * RS + c] : 0.0;
        }
      }
    }
  }

  double* slot = work + (int64_t)blockIdx.x * (KP * KP + 1);
  int u = 0;
#pragma unroll
  for (int a = 0; a < NB; ++a)
#pragma unroll
    for (int b = a; b < NB; ++b, ++u)
#pragma unroll
      for (int r = 0; r < 4; ++r) slot[(16 * a + lr + 4 * r) * KP + 16 * b + lc] = acc[u][r];
  viol = wave_sum(viol);
  if (lane == 0) slot[KP * KP] = viol;
}

// gram[k x k] and viol[1] from the slots, in slot order: thread (e, part) adds the part-th quarter of the slots for
// output element e, the four quarters are added in order.  An element below the diagonal blocks is its mirror image.
__global__ __launch_bounds__(256) void k_nmf_reduce(int k, int kp, int slots, const double* __restrict__ work,
                                                    double* __restrict__ gram, double* __restrict__ viol) {
  __shared__ double red[256];
  const int total = k * k + 1;
  const int e = blockIdx.x * 64 + (threadIdx.x & 63);
  const int part = threadIdx.x >> 6;
  double acc = 0.0;
  if (e < total) {
    int src = kp * kp;
    if (e < k * k) {
      const int i = e / k, j = e % k;
      src = i / 16 > j / 16 ? j * kp + i : i * kp + j;
    }
    const int64_t stride = (int64_t)kp * kp + 1;
    const int s0 = slots * part / 4, s1 = slots * (part + 1) / 4;
#pragma unroll 8
    for (int s = s0; s < s1; ++s) acc += work[s * stride + src];
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  if (part == 0 && e < total) {
    const double v = ((red[threadIdx.x] + red[threadIdx.x + 64]) + red[threadIdx.x + 128]) + red[threadIdx.x + 192];
    if (e < k * k) gram[e] = v; else viol[0] = v;
  }
}

inline int nmf_kp(int k) { return k <= 16 ? 16 : (k <= 32 ? 32 : 64); }

inline int64_t nmf_blocks(int64_t rows, int max_blocks) {
  int64_t b = (rows + kNmfTile - 1) / kNmfTile;
  const int64_t cap = max_blocks > 0 ? max_blocks : kNmfBlocks;
  if (b > cap) b = cap;
  return b < 1 ? 1 : b;
}

}  // namespace

extern "C" {

int mu_nmf_max_components(void) { return kNmfMaxK; }

size_t mu_nmf_cd_worksize(int64_t rows, int k, int max_blocks) {
  if (rows < 0 || k < 1 || k > kNmfMaxK) return 0;
  const size_t kp = (size_t)nmf_kp(k);
  return (size_t)nmf_blocks(rows, max_blocks) * (kp * kp + 1) * sizeof(double);
}

int mu_nmf_cd_sweep_f64(int64_t rows, int k, double* d_W, int64_t ldw, const double* d_B, int64_t ldb,
                        const double* d_bscale, const double* d_G, double l1, const double* d_oscale, double* d_Wout,
                        int64_t ldo, double* d_gram, double* d_viol, void* d_work, size_t work_bytes, int max_blocks,
                        void* stream) {
  MU_REQUIRE(k >= 1 && k <= kNmfMaxK, "k must be 1..64");
  MU_REQUIRE(rows >= 0, "bad shape");
  MU_REQUIRE(max_blocks >= 0, "negative max_blocks");
  MU_REQUIRE(ldw >= k, "ldw must cover k");
  MU_REQUIRE(ldb >= k, "ldb must cover k");
  MU_REQUIRE(d_Wout == nullptr || ldo >= k, "ldo must cover k");
  MU_REQUIRE(d_gram && d_viol, "null pointer");
  MU_REQUIRE(rows == 0 || (d_W && d_B && d_G), "null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (rows == 0) {
    MU_CHECK_HIP(hipMemsetAsync(d_gram, 0, (size_t)k * k * sizeof(double), st));
    MU_CHECK_HIP(hipMemsetAsync(d_viol, 0, sizeof(double), st));
    return MU_OK;
  }
  MU_REQUIRE(d_work && work_bytes >= mu_nmf_cd_worksize(rows, k, max_blocks), "work buffer too small");
  const unsigned blocks = (unsigned)nmf_blocks(rows, max_blocks);
  const int kp = nmf_kp(k);
  double* work = (double*)d_work;
  by_width<16, 32, 64>(k, [&](auto w) {
    hipLaunchKernelGGL((k_nmf_sweep<decltype(w)::value>), dim3(blocks), dim3(64), 0, st, rows, k, d_W, ldw, d_B, ldb,
                       d_bscale, d_G, l1, d_oscale, d_Wout, ldo, work);
  });
  MU_CHECK_LAUNCH();
  const int total = k * k + 1;
  hipLaunchKernelGGL(k_nmf_reduce, dim3((unsigned)((total + 63) / 64)), dim3(256), 0, st, k, kp, (int)blocks,
                     (const double*)work, d_gram, d_viol);
  MU_CHECK_LAUNCH();
  return MU_OK;
}

}  // extern "C"
