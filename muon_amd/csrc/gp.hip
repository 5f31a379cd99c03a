// The two matrix-vector passes of MEFISTO's eigen route (muon_amd/_core/mefisto.py): the posterior of one
// factor under a Gaussian-process prior whose covariance has the eigenvectors V [n x n, row-major f64, leading
// dimension ldv] when the likelihood's precision is one number for every sample,
//     u = V^T r,      m = V (g o u),      diag C = (V o V) g.
// As tensor operations that is three passes over V per factor and iteration; the factors cannot be batched (the sweep
// over them is Gauss-Seidel), and V is the fit's whole memory traffic.  Here it is two:
//
//   k_gp_project   u = V^T r.  A workgroup takes a panel of kGpPanel rows and a tile of 256 columns, a thread one
//                  column: every row is read with consecutive 8-byte loads, eight rows in flight per thread.  Thread i
//                  adds the products of rows 0, 4, 8, ... of its panel in one chain, rows 1, 5, 9, ... in a second, and so
//                  on (four chains), then ((c0 + c1) + c2) + c3, and writes the partial sum to work[panel][i];
//                  k_gp_project_finish adds the panels in panel order.
//   k_gp_posterior one read of row n of V gives both m_n = sum_i V_ni g_i u_i and (diag C)_n = sum_i V_ni^2 g_i.  A wave
//                  takes a row: lane l adds the terms i = l, l + 64, l + 128, ... - four chains (i / 64 mod 4), added as
//                  above - and the 64 lane sums go through wave_sum's tree.
//
// No atomics, every sum in the order stated above: a function of n alone, so two calls agree bit for bit.  Every index is
// checked against n; a thread past the matrix reads nothing.
#include "common.hpp"

namespace {

constexpr int kGpPanel = 256;  // rows per partial sum of the projection
constexpr int kGpCols = 256;   // columns per workgroup of the projection: a thread each
constexpr int kGpRows = 4;     // rows per workgroup of the posterior: a wave each

__global__ __launch_bounds__(kGpCols) void k_gp_project(int64_t n, const double* __restrict__ V, int64_t ldv,
                                                        const double* __restrict__ r, double* __restrict__ work) {
  const int64_t col = (int64_t)blockIdx.x * kGpCols + threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.y * kGpPanel;
  const int64_t row1 = row0 + kGpPanel < n ? row0 + kGpPanel : n;
  if (col >= n) return;
  const double* __restrict__ p = V + col;
  double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;
  int64_t i = row0;
  for (; i + 8 <= row1; i += 8) {
    double v[8], x[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) v[t] = p[(i + t) * ldv];
#pragma unroll
    for (int t = 0; t < 8; ++t) x[t] = r[i + t];
    c0 += v[0] * x[0]; c1 += v[1] * x[1]; c2 += v[2] * x[2]; c3 += v[3] * x[3];
    c0 += v[4] * x[4]; c1 += v[5] * x[5]; c2 += v[6] * x[6]; c3 += v[7] * x[7];
  }
  // (the panel starts at a multiple of 4 and i - row0 is a multiple of 8: row i + t belongs to chain t mod 4)
  for (int t = 0; i < row1; ++i, ++t) {
    const double y = p[i * ldv] * r[i];
    if ((t & 3) == 0) c0 += y; else if ((t & 3) == 1) c1 += y; else if ((t & 3) == 2) c2 += y; else c3 += y;
  }
  work[(int64_t)blockIdx.y * n + col] = ((c0 + c1) + c2) + c3;
}

__global__ __launch_bounds__(256) void k_gp_project_finish(int64_t n, int panels, const double* __restrict__ work,
                                                           double* __restrict__ u) {
  const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (col >= n) return;
  double acc = 0.0;
  for (int p = 0; p < panels; ++p) acc += work[(int64_t)p * n + col];
  u[col] = acc;
}

__global__ __launch_bounds__(64 * kGpRows) void k_gp_posterior(int64_t n, const double* __restrict__ V, int64_t ldv,
                                                               const double* __restrict__ g,
                                                               const double* __restrict__ u, double* __restrict__ m,
                                                               double* __restrict__ dc) {
  const int lane = lane_id();
  const int64_t row = (int64_t)blockIdx.x * kGpRows + uniform32(threadIdx.x >> 6);
  if (row >= n) return;  // (wave-uniform)
  const double* __restrict__ p = V + row * ldv;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;  // m_n
  double b0 = 0.0, b1 = 0.0, b2 = 0.0, b3 = 0.0;  // (diag C)_n
  int64_t i = lane;
  for (; i + 192 < n; i += 256) {
    const double v0 = p[i], v1 = p[i + 64], v2 = p[i + 128], v3 = p[i + 192];
    const double g0 = g[i], g1 = g[i + 64], g2 = g[i + 128], g3 = g[i + 192];
    const double u0 = u[i], u1 = u[i + 64], u2 = u[i + 128], u3 = u[i + 192];
    const double w0 = v0 * g0, w1 = v1 * g1, w2 = v2 * g2, w3 = v3 * g3;
    a0 += w0 * u0; a1 += w1 * u1; a2 += w2 * u2; a3 += w3 * u3;
    b0 += w0 * v0; b1 += w1 * v1; b2 += w2 * v2; b3 += w3 * v3;
  }
  // (i - lane is a multiple of 256: the term i + 64 t belongs to chain t)
  for (int t = 0; i < n; i += 64, ++t) {
    const double v = p[i];
    const double w = v * g[i];
    const double ya = w * u[i], yb = w * v;
    if (t == 0) { a0 += ya; b0 += yb; } else if (t == 1) { a1 += ya; b1 += yb; } else { a2 += ya; b2 += yb; }
  }
  const double sa = wave_sum(((a0 + a1) + a2) + a3);
  const double sb = wave_sum(((b0 + b1) + b2) + b3);
  if (lane == 0) {
    m[row] = sa;
    dc[row] = sb;
  }
}

inline int64_t gp_panels(int64_t n) { return (n + kGpPanel - 1) / kGpPanel; }

}  // namespace

extern "C" {

size_t mu_gp_project_worksize(int64_t n) {
  if (n < 1) return 0;
  return (size_t)gp_panels(n) * (size_t)n * sizeof(double);
}

int mu_gp_project_f64(int64_t n, const double* d_V, int64_t ldv, const double* d_r, double* d_u, void* d_work,
                      size_t work_bytes, void* stream) {
  MU_REQUIRE(n >= 0, "bad shape");
  if (n == 0) return MU_OK;
  MU_REQUIRE(ldv >= n, "ldv must cover n");
  MU_REQUIRE(n <= ((int64_t)1 << 22), "n must be at most 2^22");
  MU_REQUIRE(d_V && d_r && d_u, "null pointer");
  MU_REQUIRE(d_work && work_bytes >= mu_gp_project_worksize(n), "work buffer too small");
  hipStream_t st = (hipStream_t)stream;
  const int64_t panels = gp_panels(n);
  const unsigned tiles = (unsigned)((n + kGpCols - 1) / kGpCols);
  hipLaunchKernelGGL(k_gp_project, dim3(tiles, (unsigned)panels), dim3(kGpCols), 0, st, n, d_V, ldv, d_r, (double*)d_work);
  MU_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_gp_project_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, (int)panels,
                     (const double*)d_work, d_u);
  MU_CHECK_LAUNCH();
  return MU_OK;
}

int mu_gp_posterior_f64(int64_t n, const double* d_V, int64_t ldv, const double* d_g, const double* d_u, double* d_m,
                        double* d_dc, void* stream) {
  MU_REQUIRE(n >= 0, "bad shape");
  if (n == 0) return MU_OK;
  MU_REQUIRE(ldv >= n, "ldv must cover n");
  MU_REQUIRE(n <= ((int64_t)1 << 22), "n must be at most 2^22");
  MU_REQUIRE(d_V && d_g && d_u && d_m && d_dc, "null pointer");
  hipLaunchKernelGGL(k_gp_posterior, dim3((unsigned)((n + kGpRows - 1) / kGpRows)), dim3(64 * kGpRows), 0,
                     (hipStream_t)stream, n, d_V, ldv, d_g, d_u, d_m, d_dc);
  MU_CHECK_LAUNCH();
  return MU_OK;
}

}  // extern "C"
