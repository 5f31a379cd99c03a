// muon.tl.snf: similarity network fusion (/root/reference/muon/_core/tools.py:716-920), all f64.
//
// Every matrix is N x N row-major with a leading dimension >= N; whatever lies past column N of a row is never read
// into a result (masked by INDEX: it may hold NaN).  Nothing is read or written by columns from global memory: the
// transposed accesses go through 64 x 64 LDS tiles with a row stride of 65 doubles (130 dwords), so that the
// transposed read tile[lane][r] puts lanes 0..31 of a ds_read_b64 on 32 distinct bank pairs (2 lane mod 64) instead
// of one.
//
//   k_snf_pair<SYM>    out = (X + X^T) / 2, diagonal 0                     a workgroup owns the tile PAIR (I, J), (J, I),
//   k_snf_pair<NORM>   out = (x_ij / (2 r_i) + x_ji / (2 r_j)) / 2,        I <= J: both tiles are staged, then both are
//                      diagonal 0.5                                        written - one read and one write of the
//                      matrix, in place if wanted, and the result is symmetric bit for bit (a + b == b + a)
//   k_snf_rowsum       r_i = sum_j x_ij - x_ii, 1 where that is 0          a wave per row, lanes stride the row, then
//                                                                          the xor butterfly: a fixed order
//   k_snf_means        the k + 1 smallest of a row, mean of the finite     a wave per row, the running list lives one
//                      ones among the 2nd .. (k+1)-th, + eps               value per lane (two registers: 128 ranks)
//   k_snf_pdf          W = N(0, sigma sig).pdf(D), sig = (m_i + m_j) / 3 + D / 3 + eps.  Element-wise: D is symmetric
//                      bit for bit after k_snf_pair<SYM> and m_i + m_j == m_j + m_i, so dens is symmetric bit for bit
//                      and the reference's (dens + dens^T) / 2 returns dens itself
//   k_snf_topk         the k largest of a row with their columns           a wave per row, the same list (one register)
//   k_snf_p_rowsum / k_snf_p_div   P[i][j] = z[i][j] / rowsum_z[j] on the CSR of z, sums in stored order (compensated)
//   k_snf_diffuse      Y = (P X)^T, X = (X_0 + X_1 + ...) / nmat formed on read
//
// k_snf_diffuse: a workgroup owns 64 rows of P x one 64-column strip of X; a wave takes 16 of the rows in turn, lane =
// column, so every gathered row of X is one contiguous 512-byte read per term and the entries of a row of P (wave
// uniform) are added in stored order.  The 64 x 64 result goes through the LDS tile and leaves transposed, again in
// 512-byte rows.  Workgroups are numbered strip-major: all row tiles of a strip run before the next strip starts, so the
// strip of X (N x 512 bytes per term) that they gather from stays in L2 / Infinity Cache while they consume it.
// No atomics anywhere: two runs agree bit for bit.
#include "common.hpp"

#include <math.h>

namespace {

constexpr int kSnfMaxK = 64;         // k_snf_topk: one list register
constexpr int kSnfAffinityMaxK = 127;  // k_snf_means: k + 1 ranks in two list registers
constexpr int kSnfMaxTerms = 8;
constexpr int kT = 64;   // tile edge
constexpr int kTS = 65;  // LDS row stride, doubles

struct SnfTerms {
  const double* p[kSnfMaxTerms];
};

enum { kPairSym = 0, kPairNorm = 1 };

template <int MODE>
__device__ __forceinline__ double pair_value(double a, double b, double ra, double rb, bool diag) {
  if constexpr (MODE == kPairSym) {
    return diag ? 0.0 : (a + b) / 2;
  } else {
    return diag ? 0.5 : (a / (2 * ra) + b / (2 * rb)) / 2;
  }
}

// X and out may be the same matrix: a workgroup stages both of its tiles before it writes either, and no other
// workgroup touches them.
template <int MODE>
__global__ __launch_bounds__(256) void k_snf_pair(int64_t n, int64_t ldx, const double* X, const double* __restrict__ r,
                                                  int64_t ldo, double* out) {
  const int I = blockIdx.y, J = blockIdx.x;
  if (I > J) return;
  __shared__ double A[kT * kTS];  // A[a][b] = X[i0 + a][j0 + b]
  __shared__ double B[kT * kTS];  // B[a][b] = X[j0 + a][i0 + b]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t i0 = (int64_t)I * kT, j0 = (int64_t)J * kT;
  for (int a = wave; a < kT; a += 4) {
    const bool oka = i0 + a < n && j0 + lane < n;
    A[a * kTS + lane] = oka ? X[(i0 + a) * ldx + j0 + lane] : 0.0;
    const bool okb = j0 + a < n && i0 + lane < n;
    B[a * kTS + lane] = okb ? X[(j0 + a) * ldx + i0 + lane] : 0.0;
  }
  __syncthreads();
  double rl_i = 1.0, rl_j = 1.0;  // r of this lane's column in tile (J, I) / tile (I, J)
  if constexpr (MODE == kPairNorm) {
    rl_i = i0 + lane < n ? r[i0 + lane] : 1.0;
    rl_j = j0 + lane < n ? r[j0 + lane] : 1.0;
  }
  for (int a = wave; a < kT; a += 4) {
    // element (i0 + a, j0 + lane)
    if (i0 + a < n && j0 + lane < n) {
      const double ri = MODE == kPairNorm ? r[i0 + a] : 1.0;
      out[(i0 + a) * ldo + j0 + lane] =
          pair_value<MODE>(A[a * kTS + lane], B[lane * kTS + a], ri, rl_j, i0 + a == j0 + lane);
    }
    // element (j0 + a, i0 + lane): the same two operands, the other way round
    if (I != J && j0 + a < n && i0 + lane < n) {
      const double rj = MODE == kPairNorm ? r[j0 + a] : 1.0;
      out[(j0 + a) * ldo + i0 + lane] = pair_value<MODE>(B[a * kTS + lane], A[lane * kTS + a], rj, rl_i, false);
    }
  }
}

__global__ __launch_bounds__(256) void k_snf_rowsum(int64_t n, int64_t ldx, const double* __restrict__ X,
                                                    double* __restrict__ r) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + uniform32(threadIdx.x >> 6);
  if (i >= n) return;
  const double* row = X + i * ldx;
  double acc = 0.0;
  for (int64_t c = lane; c < n; c += 64) acc += row[c];
  acc = wave_sum_all(acc);
  double v = acc - row[i];
  if (v == 0) v = 1.0;
  if (lane == 0) r[i] = v;
}

// ---- the running list of a wave: ascending, rank = lane, +inf where nothing has been put yet --------------------------
// Puts the wave-uniform (v, vi) where it belongs (after the elements equal to it) and hands back what falls off the end.
// A v that is not below the last element changes nothing.
__device__ __forceinline__ void list_insert(double& held, int& hidx, double v, int vi, double& ev, int& evi) {
  const int lane = threadIdx.x & 63;
  const int pos = __popcll(__ballot(held <= v));  // the list ascends: these lanes are a prefix
  ev = __shfl(held, 63, 64);
  evi = __shfl(hidx, 63, 64);
  const double up = __shfl_up(held, 1, 64);
  const int upi = __shfl_up(hidx, 1, 64);
  if (lane == pos) {
    held = v;
    hidx = vi;
  } else if (lane > pos) {
    held = up;
    hidx = upi;
  }
}

// The `want` smallest keys of key(c), c < n, of one wave's row: ranks 0..63 in (lo, loi), 64..127 in (hi, hii) if TWO.
template <bool TWO, typename KeyFn>
__device__ __forceinline__ void wave_smallest(int64_t n, int want, KeyFn key, double& lo, int& loi, double& hi, int& hii) {
  const int lane = threadIdx.x & 63;
  const double inf = __builtin_huge_val();
  lo = inf, hi = inf, loi = -1, hii = -1;
  double thr = inf;  // the key at rank want - 1: a candidate has to be below it
  const int tl = (want - 1) & 63;
  const bool thi = TWO && want > 64;
  for (int64_t c0 = 0; c0 < n; c0 += 64) {
    const int64_t c = c0 + lane;
    const double v = c < n ? key(c) : inf;
    uint64_t mask = __ballot(v < thr);
    while (mask) {
      const int src = __builtin_ctzll(mask);
      mask &= mask - 1;
      const double cv = __shfl(v, src, 64);
      if (!(cv < thr)) continue;  // (the bar has come down since the ballot)
      const int ci = (int)(c0 + src);
      double ev, ev2;
      int evi, evi2;
      const double last = __shfl(lo, 63, 64);
      if (cv < last) {
        list_insert(lo, loi, cv, ci, ev, evi);
        if (TWO) list_insert(hi, hii, ev, evi, ev2, evi2);
      } else if (TWO) {
        list_insert(hi, hii, cv, ci, ev2, evi2);
      }
      thr = thi ? __shfl(hi, tl, 64) : __shfl(lo, tl, 64);
    }
  }
}

__global__ __launch_bounds__(256) void k_snf_means(int64_t n, int k, int64_t ldd, const double* __restrict__ D, double eps,
                                                   double* __restrict__ means) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + uniform32(threadIdx.x >> 6);
  if (i >= n) return;
  const double* row = D + i * ldd;
  double lo, hi;
  int loi, hii;
  wave_smallest<true>(n, k + 1, [&](int64_t c) { return row[c]; }, lo, loi, hi, hii);
  // ranks 1 .. k, the finite ones (the fill of a short row is +inf: not finite either)
  const bool use_lo = lane >= 1 && lane <= k && isfinite(lo);
  const bool use_hi = lane + 64 <= k && isfinite(hi);
  const double s = wave_sum_all(use_lo ? lo : 0.0) + wave_sum_all(use_hi ? hi : 0.0);
  const int cnt = __popcll(__ballot(use_lo)) + __popcll(__ballot(use_hi));
  if (lane == 0) means[i] = s / (double)cnt + eps;
}

__global__ __launch_bounds__(256) void k_snf_pdf(int64_t n, int64_t ldw, double* __restrict__ W,
                                                 const double* __restrict__ means, double sigma, double eps) {
  const int64_t i = blockIdx.y;
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const double d = W[i * ldw + j];
  const double sig = (means[i] + means[j]) / 3 + d / 3 + eps;
  const double scale = sigma * sig;
  const double y = d / scale;
  // scipy.stats.norm(0, scale).pdf(d): exp(-y**2 / 2.0) / sqrt(2 pi) / scale
  W[i * ldw + j] = exp(-(y * y) / 2.0) / 2.5066282746310002 / scale;
}

__global__ __launch_bounds__(256) void k_snf_topk(int64_t n, int k, int64_t ldw, const double* __restrict__ W,
                                                  int32_t* __restrict__ idx, double* __restrict__ val) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + uniform32(threadIdx.x >> 6);
  if (i >= n) return;
  const double* row = W + i * ldw;
  double lo, hi;
  int loi, hii;
  wave_smallest<false>(n, k, [&](int64_t c) { return -row[c]; }, lo, loi, hi, hii);  // the largest: the smallest of -w
  if (lane < k) {
    idx[i * k + lane] = loi;
    val[i * k + lane] = -lo;
  }
}

// Row sums of the CSR of z in stored order, compensated (Neumaier): the sum of a row does not depend on how many
// entries it has to within an ulp.
__global__ __launch_bounds__(256) void k_snf_p_rowsum(int64_t n, const int64_t* __restrict__ indptr,
                                                      const double* __restrict__ vals, double* __restrict__ rowsum) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double s = 0.0, comp = 0.0;
  for (int64_t e = indptr[i]; e < indptr[i + 1]; ++e) {
    const double v = vals[e];
    const double t = s + v;
    comp += fabs(s) >= fabs(v) ? (s - t) + v : (v - t) + s;
    s = t;
  }
  rowsum[i] = s + comp;
}

__global__ __launch_bounds__(256) void k_snf_p_div(int64_t nnz, const int32_t* __restrict__ cols, double* __restrict__ vals,
                                                   const double* __restrict__ rowsum) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < nnz) vals[e] = vals[e] / rowsum[cols[e]];
}

// POW2: nmat is a power of two, the division is a multiplication by its exact reciprocal.
template <bool POW2>
__global__ __launch_bounds__(256) void k_snf_diffuse(int64_t n, int nmat, SnfTerms X, int64_t ldx,
                                                     const int64_t* __restrict__ indptr, const int32_t* __restrict__ cols,
                                                     const double* __restrict__ vals, int64_t ldy, double* __restrict__ Y,
                                                     int64_t row_tiles) {
  __shared__ double tile[kT * kTS];
  const int lane = threadIdx.x & 63, wave = uniform32(threadIdx.x >> 6);
  const int64_t strip = blockIdx.x / row_tiles, rt = blockIdx.x % row_tiles;
  const int64_t c = strip * kT + lane;
  const bool cok = c < n;
  const int64_t cc = cok ? c : 0;  // (in bounds; masked below)
  const double div = (double)nmat, inv = 1.0 / (double)nmat;
  for (int q = 0; q < 16; ++q) {
    const int rl = wave * 16 + q;
    const int64_t i = rt * kT + rl;
    double acc = 0.0;
    if (i < n) {
      const int64_t e0 = uniform64(indptr[i]), e1 = uniform64(indptr[i + 1]);
#pragma unroll 4
      for (int64_t e = e0; e < e1; ++e) {
        const int64_t off = (int64_t)cols[e] * ldx + cc;
        double x = X.p[0][off];
        for (int m = 1; m < nmat; ++m) x += X.p[m][off];
        x = POW2 ? x * inv : x / div;
        acc += vals[e] * (cok ? x : 0.0);
      }
    }
    tile[rl * kTS + lane] = acc;
  }
  __syncthreads();
  const int64_t i = rt * kT + lane;
  for (int a = wave; a < kT; a += 4) {
    const int64_t col = strip * kT + a;
    if (col < n && i < n) Y[col * ldy + i] = tile[lane * kTS + a];
  }
}

inline unsigned tiles_of(int64_t n) { return (unsigned)((n + kT - 1) / kT); }

// the grids index with 32-bit tile counts and a y dimension of at most 65535
constexpr int64_t kSnfMaxN = (int64_t)65535 * kT;

}  // namespace

extern "C" {

int mu_snf_max_k(void) { return kSnfMaxK; }
int mu_snf_affinity_max_k(void) { return kSnfAffinityMaxK; }
int mu_snf_max_terms(void) { return kSnfMaxTerms; }

int mu_snf_affinity_f64(int64_t n, int k, int64_t ldd, const double* d_D, int64_t ldw, double* d_W, double sigma,
                        double eps, double* d_means, void* stream) {
  MU_REQUIRE(n >= 0 && n <= 65535, "n must be 0..65535");
  MU_REQUIRE(k >= 1 && k <= kSnfAffinityMaxK, "k must be 1..127");
  MU_REQUIRE(ldd >= n && ldw >= n, "leading dimension below n");
  MU_REQUIRE(n == 0 || (d_D && d_W && d_means), "null pointer");
  if (n == 0) return MU_OK;
  hipStream_t st = (hipStream_t)stream;
  const unsigned t = tiles_of(n);
  hipLaunchKernelGGL((k_snf_pair<kPairSym>), dim3(t, t), dim3(256), 0, st, n, ldd, d_D, (const double*)nullptr, ldw, d_W);
  MU_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_snf_means, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, n, k, ldw, (const double*)d_W, eps,
                     d_means);
  MU_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_snf_pdf, dim3((unsigned)((n + 255) / 256), (unsigned)n), dim3(256), 0, st, n, ldw, d_W,
                     (const double*)d_means, sigma, eps);
  MU_CHECK_LAUNCH();
  return MU_OK;
}

int mu_snf_normalize_f64(int64_t n, int64_t ldx, const double* d_X, int64_t ldo, double* d_out, double* d_r, void* stream) {
  MU_REQUIRE(n >= 0 && n <= kSnfMaxN, "bad n");
  MU_REQUIRE(ldx >= n && ldo >= n, "leading dimension below n");
  MU_REQUIRE(n == 0 || (d_X && d_out && d_r), "null pointer");
  if (n == 0) return MU_OK;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_snf_rowsum, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, n, ldx, d_X, d_r);
  MU_CHECK_LAUNCH();
  const unsigned t = tiles_of(n);
  hipLaunchKernelGGL((k_snf_pair<kPairNorm>), dim3(t, t), dim3(256), 0, st, n, ldx, d_X, (const double*)d_r, ldo, d_out);
  MU_CHECK_LAUNCH();
  return MU_OK;
}

int mu_snf_topk_f64(int64_t n, int k, int64_t ldw, const double* d_W, int32_t* d_idx, double* d_val, void* stream) {
  MU_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "bad n");
  MU_REQUIRE(k >= 1 && k <= kSnfMaxK, "k must be 1..64");
  MU_REQUIRE(n == 0 || k <= n, "k above n");
  MU_REQUIRE(ldw >= n, "leading dimension below n");
  MU_REQUIRE(n == 0 || (d_W && d_idx && d_val), "null pointer");
  if (n == 0) return MU_OK;
  hipLaunchKernelGGL(k_snf_topk, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, n, k, ldw, d_W, d_idx,
                     d_val);
  MU_CHECK_LAUNCH();
  return MU_OK;
}

int mu_snf_p_scale_f64(int64_t n, int64_t nnz, const int64_t* d_indptr, const int32_t* d_cols, double* d_vals,
                       double* d_rowsum, void* stream) {
  MU_REQUIRE(n >= 0 && n < ((int64_t)1 << 31) && nnz >= 0, "bad shape");
  MU_REQUIRE(d_indptr && (n == 0 || d_rowsum) && (nnz == 0 || (d_cols && d_vals)), "null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (n > 0) {
    hipLaunchKernelGGL(k_snf_p_rowsum, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, d_indptr,
                       (const double*)d_vals, d_rowsum);
    MU_CHECK_LAUNCH();
  }
  if (nnz > 0) {
    hipLaunchKernelGGL(k_snf_p_div, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, st, nnz, d_cols, d_vals,
                       (const double*)d_rowsum);
    MU_CHECK_LAUNCH();
  }
  return MU_OK;
}

int mu_snf_diffuse_f64(int64_t n, int nmat, const void* const* h_X, int64_t ldx, const int64_t* d_indptr,
                       const int32_t* d_cols, const double* d_vals, int64_t ldy, double* d_Y, void* stream) {
  MU_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "bad n");
  MU_REQUIRE(nmat >= 1 && nmat <= kSnfMaxTerms, "nmat must be 1..8");
  MU_REQUIRE(ldx >= n && ldy >= n, "leading dimension below n");
  MU_REQUIRE(h_X && d_indptr && (n == 0 || (d_cols && d_vals && d_Y)), "null pointer");
  SnfTerms terms;
  for (int m = 0; m < kSnfMaxTerms; ++m) {
    terms.p[m] = m < nmat ? (const double*)h_X[m] : nullptr;
    MU_REQUIRE(m >= nmat || n == 0 || terms.p[m], "null term");
    MU_REQUIRE(m >= nmat || n == 0 || terms.p[m] != d_Y, "Y must not be one of the terms");
  }
  if (n == 0) return MU_OK;
  const int64_t t = tiles_of(n);
  MU_REQUIRE(t * t < ((int64_t)1 << 31), "n too large for one launch");
  hipStream_t st = (hipStream_t)stream;
  if ((nmat & (nmat - 1)) == 0)
    hipLaunchKernelGGL((k_snf_diffuse<true>), dim3((unsigned)(t * t)), dim3(256), 0, st, n, nmat, terms, ldx, d_indptr,
                       d_cols, d_vals, ldy, d_Y, t);
  else
    hipLaunchKernelGGL((k_snf_diffuse<false>), dim3((unsigned)(t * t)), dim3(256), 0, st, n, nmat, terms, ldx, d_indptr,
                       d_cols, d_vals, ldy, d_Y, t);
  MU_CHECK_LAUNCH();
  return MU_OK;
}

}  // extern "C"
