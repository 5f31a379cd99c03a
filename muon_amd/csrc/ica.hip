// One fixed-point sweep of parallel FastICA over the whitened data Z [n x kp] (row-major f64, leading dimension ldz),
// fused (the reference hands the arithmetic to scikit-learn through
// /root/reference/muon/_core/tools.py:1365-1386):
//
//   y = Z W^T   [n x k]          A  = g(y)^T Z     [k x k]          gp[j] = sum_i g'(y_ij)
//
// The library formulation is three passes over n x k data with an n x k temporary (W Z, the tanh pass with its mean,
// g(W Z) Z^T); here a workgroup reads a 64-row tile of Z once and leaves k x k + k numbers.  v_mfma_f64_16x16x4_f64,
// operand maps as at the top of skinny.hip:  A operand lane l = A[i = l & 15][k = l >> 4],  B operand lane l =
// B[k = l >> 4][j = l & 15],  C/D reg r of lane l = C[row = (l >> 4) + 4 r][col = l & 15].
//
// Workgroup = four waves; wave w owns component block w (components 16 w .. 16 w + 15) and idles - it still loads
// and stages its share of every tile - where k leaves its block empty (k <= 48).  Per tile a wave
//   1. Y[64 x 16] = Z_tile W[block w, :]^T : i = row, j = component, k = column of Z.  The A operand comes from the
//      staged tile (row stride kp * 8 + 16 bytes: 16 rows x one f64 land on 16 distinct 4-bank groups, conflict free);
//      the B operand, this wave's 16 x kp block of W, lives in kp / 4 registers for the whole kernel (W is not
//      staged in LDS: no wave ever needs another wave's block);
//   2. applies g and g' to its 16 accumulator values, masked by row (< n) and component (< k) INDEX - g'(0) = 1 for
//      logcosh and exp, so a padded row or component that is merely zero would be counted -, and adds g' into a
//      per-lane partial column sum;
//   3. A[block w, :] += G^T Z_tile : i = component, j = column of Z, k = row.  Register r of accumulator q IS the A
//      operand of the step over rows 16 q + 4 r .. + 3 (the f64 C/D map puts row (l >> 4) + 4 r on lane l, the A
//      operand map wants k = l >> 4 there): g(Y) never leaves the registers.  The B operand is the staged tile again
//      (two rows x 16 consecutive f64 per half wave: two-way conflicts on part of the banks, behind 32-cycle MFMAs).
// The tile is staged with coalesced 16-byte loads, one tile ahead in registers; rows at or past n and columns at or
// past k are ZEROED ON THE WAY INTO LDS by index (a select, so NaN in the padding of Z does no harm).
//
// No float atomics: each workgroup writes its partial [kp x kp + kp] to its slot of the workspace and a second kernel
// adds the slots in slot order (four fixed quarters, then their sum in order): two runs agree bit for bit.  The grid is
// min(tiles, max_blocks or 512): a function of (n, max_blocks) alone.
#include "common.hpp"

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

constexpr int kIcaMaxK = 64;
constexpr int kIcaTile = 64;      // rows of Z per tile
constexpr int kIcaBlocks = 512;   // default cap of the grid
enum { kFunLogcosh = 0, kFunExp = 1, kFunCube = 2 };

template <int FUN>
__device__ __forceinline__ void ica_g(double y, double alpha, double& g, double& gp) {
  if constexpr (FUN == kFunLogcosh) {
    const double t = tanh(alpha * y);
    g = t;
    gp = alpha * (1.0 - t * t);
  } else if constexpr (FUN == kFunExp) {
    const double y2 = y * y;
    const double e = exp(-y2 / 2);
    g = y * e;
    gp = (1.0 - y2) * e;
  } else {
    const double y2 = y * y;
    g = y2 * y;
    gp = 3.0 * y2;
  }
}

template <int FUN, int NB>
__global__ __launch_bounds__(256) void k_ica_sweep(int64_t n, int k, int64_t ldz, const double* __restrict__ Z,
                                                   const double* __restrict__ W, double alpha,
                                                   double* __restrict__ work) {
  constexpr int KP = 16 * NB;
  constexpr int RS = KP * 8 + 16;  // LDS row stride in bytes
  constexpr int PPR = KP / 2;      // 16-byte pieces per row
  constexpr int NP = 2 * NB;       // pieces per thread and tile: 64 * PPR / 256
  __shared__ __attribute__((aligned(16))) char zs[kIcaTile * RS];
  const int lane = threadIdx.x & 63;
  const int wave = uniform32(threadIdx.x >> 6);
  const int lr = lane >> 4, lc = lane & 15;
  const bool active = wave < NB;
  const int comp = 16 * wave + lc;
  const int64_t n_tiles = (n + kIcaTile - 1) / kIcaTile;

  double wreg[KP / 4];
#pragma unroll
  for (int u = 0; u < KP / 4; ++u) {
    const int c = 4 * u + lr;
    wreg[u] = (comp < k && c < k) ? W[(int64_t)comp * k + c] : 0.0;
  }

  d2 pre[NP];
  auto gload = [&](int64_t tile) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int p = threadIdx.x + 256 * i;
      const int64_t row = tile * kIcaTile + p / PPR;
      const int64_t rc = row < n ? row : n - 1;  // (in bounds; zeroed by index in stage())
      pre[i] = *reinterpret_cast<const d2*>(Z + rc * ldz + 2 * (p % PPR));
    }
  };
  auto stage = [&](int64_t tile) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int p = threadIdx.x + 256 * i;
      const bool rk = tile * kIcaTile + p / PPR < n;
      const int c0 = 2 * (p % PPR);
      d2 v = pre[i];
      v.x = (rk && c0 < k) ? v.x : 0.0;
      v.y = (rk && c0 + 1 < k) ? v.y : 0.0;
      *reinterpret_cast<d2*>(&zs[(p / PPR) * RS + (p % PPR) * 16]) = v;
    }
  };

  d4 accA[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) accA[b] = d4{0, 0, 0, 0};
  double gps = 0.0;

  int64_t tile = blockIdx.x;
  if (tile < n_tiles) gload(tile);
  for (; tile < n_tiles; tile += gridDim.x) {
    __syncthreads();  // the previous tile has been read
    stage(tile);
    __syncthreads();
    const int64_t next = tile + gridDim.x;
    if (next < n_tiles) gload(next);  // in flight under this tile's products
    if (active) {
      d4 y[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        y[q] = d4{0, 0, 0, 0};
#pragma unroll
        for (int u = 0; u < KP / 4; ++u) {
          const double a = *reinterpret_cast<const double*>(&zs[(16 * q + lc) * RS + (4 * u + lr) * 8]);
          y[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, wreg[u], y[q], 0, 0, 0);
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool ok = (tile * kIcaTile + 16 * q + lr + 4 * r < n) && comp < k;
          double g, gp;
          ica_g<FUN>(y[q][r], alpha, g, gp);
          y[q][r] = ok ? g : 0.0;
          gps += ok ? gp : 0.0;
        }
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int b = 0; b < NB; ++b) {
            const double z = *reinterpret_cast<const double*>(&zs[(16 * q + 4 * r + lr) * RS + (16 * b + lc) * 8]);
            accA[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(y[q][r], z, accA[b], 0, 0, 0);
          }
    }
  }

  if (active) {
    double* slot = work + (int64_t)blockIdx.x * (KP * KP + KP);
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) slot[(16 * wave + lr + 4 * r) * KP + 16 * b + lc] = accA[b][r];
    gps += __shfl_xor(gps, 16, 64);
    gps += __shfl_xor(gps, 32, 64);
    if (lr == 0) slot[KP * KP + comp] = gps;
  }
}

// A[k x k] and gp[k] from the slots, in slot order: thread (e, part) adds the part-th quarter of the slots for output
// element e, the four quarters are added in order.
__global__ __launch_bounds__(256) void k_ica_reduce(int k, int kp, int slots, const double* __restrict__ work,
                                                    double* __restrict__ A, double* __restrict__ gp) {
  __shared__ double red[256];
  const int total = k * k + k;
  const int e = blockIdx.x * 64 + (threadIdx.x & 63);
  const int part = threadIdx.x >> 6;
  double acc = 0.0;
  if (e < total) {
    const int src = e < k * k ? (e / k) * kp + e % k : kp * kp + (e - k * k);
    const int64_t stride = (int64_t)kp * kp + kp;
    const int s0 = slots * part / 4, s1 = slots * (part + 1) / 4;
#pragma unroll 8
    for (int s = s0; s < s1; ++s) acc += work[s * stride + src];
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  if (part == 0 && e < total) {
    const double v = ((red[threadIdx.x] + red[threadIdx.x + 64]) + red[threadIdx.x + 128]) + red[threadIdx.x + 192];
    if (e < k * k) A[e] = v; else gp[e - k * k] = v;
  }
}

inline int ica_kp(int k) { return (k + 15) / 16 * 16; }

inline int64_t ica_blocks(int64_t n, int max_blocks) {
  int64_t b = (n + kIcaTile - 1) / kIcaTile;
  const int64_t cap = max_blocks > 0 ? max_blocks : kIcaBlocks;
  if (b > cap) b = cap;
  return b < 1 ? 1 : b;
}

}  // namespace

extern "C" {

int mu_ica_max_components(void) { return kIcaMaxK; }

size_t mu_ica_worksize(int64_t n, int k, int max_blocks) {
  if (n < 0 || k < 1 || k > kIcaMaxK) return 0;
  const size_t kp = (size_t)ica_kp(k);
  return (size_t)ica_blocks(n, max_blocks) * (kp * kp + kp) * sizeof(double);
}

int mu_ica_sweep_f64(int64_t n, int k, int64_t ldz, const double* d_Z, const double* d_W, int fun, double alpha,
                     double* d_A, double* d_gp, void* d_work, size_t work_bytes, int max_blocks, void* stream) {
  MU_REQUIRE(k >= 1 && k <= kIcaMaxK, "k must be 1..64");
  MU_REQUIRE(n >= 0, "bad shape");
  MU_REQUIRE(fun >= kFunLogcosh && fun <= kFunCube, "fun must be 0 (logcosh), 1 (exp) or 2 (cube)");
  MU_REQUIRE(max_blocks >= 0, "negative max_blocks");
  const int kp = ica_kp(k);
  MU_REQUIRE(ldz >= kp, "ldz must cover k rounded up to a multiple of 16");
  MU_REQUIRE(ldz % 2 == 0 && (reinterpret_cast<uintptr_t>(d_Z) % 16) == 0, "Z must be 16-byte aligned with an even ldz");
  MU_REQUIRE(d_A && d_gp && d_W && (n == 0 || d_Z), "null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {
    MU_CHECK_HIP(hipMemsetAsync(d_A, 0, (size_t)k * k * sizeof(double), st));
    MU_CHECK_HIP(hipMemsetAsync(d_gp, 0, (size_t)k * sizeof(double), st));
    return MU_OK;
  }
  MU_REQUIRE(d_work && work_bytes >= mu_ica_worksize(n, k, max_blocks), "work buffer too small");
  const unsigned blocks = (unsigned)ica_blocks(n, max_blocks);
  double* work = (double*)d_work;
  by_index<3>(fun, [&](auto f) {  // kFunLogcosh, kFunExp, kFunCube
    by_width<16, 32, 48, 64>(k, [&](auto w) {  // NB = kp / 16
      hipLaunchKernelGGL((k_ica_sweep<decltype(f)::value, decltype(w)::value / 16>), dim3(blocks), dim3(256), 0, st, n, k,
                         ldz, d_Z, d_W, alpha, work);
    });
  });
  MU_CHECK_LAUNCH();
  const int total = k * k + k;
  hipLaunchKernelGGL(k_ica_reduce, dim3((unsigned)((total + 63) / 64)), dim3(256), 0, st, k, kp, (int)blocks,
                     (const double*)work, d_A, d_gp);
  MU_CHECK_LAUNCH();
  return MU_OK;
}

}  // extern "C"
