// muon.tl.umap: one epoch of the layout optimiser as a Jacobi step (muon_amd/_core/umap.py states the
// optimiser).  All arithmetic f64, columns int32, offsets and periods int64.
//
//   k_umap_epoch<DIM>   a group of kUmapGroup = 16 lanes per vertex v, four vertices per wave, sixteen per workgroup.  Lane
//                       j of the group takes the entries j, j + 16, ... of v's row, in order.  For each entry it evaluates
//                       the integer schedule (active at epoch e iff (e 2^16) mod E < 2^16), then, for an active entry,
//                       the attraction towards the entry's column and after it the entry's negatives s = 0, 1, ... in
//                       sample order, every force from the snapshot Y_in, into a private accumulator.  The group adds the
//                       sixteen accumulators with the xor butterfly (offsets 8, 4, 2, 1) and lane 0 writes Y_out[v] =
//                       Y_in[v] + alpha_e F.  A vertex without entries, or without an active one, adds F = 0.  Long rows
//                       loop: one row, one group, one summation order.  No atomics, no LDS, nothing shared between
//                       groups: two launches on equal arguments write equal bytes.
//
// d2^b is one pow(d2, b); d2^(b - 1) is that value divided by d2.
#include "common.hpp"

#include <math.h>

namespace {

constexpr int kUmapGroup = 16;
constexpr int kUmapMaxComponents = 3;
constexpr int64_t kUmapOne = (int64_t)1 << 16;  // the schedule's fixed point: E = round(period 2^16)
constexpr int kUmapMaxEpochs = 1 << 20;         // with the rate's bound: e 2^16 rate < 2^46, (c - 1) E < 2^56
constexpr int kUmapMaxRate = 1 << 10;

__device__ __forceinline__ double clip4(double x) { return fmin(4.0, fmax(-4.0, x)); }

template <int DIM>
__global__ __launch_bounds__(256) void k_umap_epoch(int n, int64_t nnz, const int64_t* __restrict__ indptr,
                                                    const int32_t* __restrict__ cols, const int64_t* __restrict__ E,
                                                    int64_t e, int64_t rate, double a, double b, double gamma,
                                                    double alpha_e, uint64_t key, const double* __restrict__ Yin,
                                                    double* __restrict__ Yout) {
  const int g = threadIdx.x & (kUmapGroup - 1);
  const int64_t v = (int64_t)blockIdx.x * (256 / kUmapGroup) + (threadIdx.x / kUmapGroup);
  const bool valid = v < n;  // (no lane leaves before the butterfly)
  int64_t rb = 0, re = 0;
  double yv[DIM], acc[DIM];
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    yv[d] = 0.0;
    acc[d] = 0.0;
  }
  if (valid) {
    rb = indptr[v];
    re = indptr[v + 1];
    if (rb < 0) rb = 0;
    if (re > nnz) re = nnz;
#pragma unroll
    for (int d = 0; d < DIM; ++d) yv[d] = Yin[v * DIM + d];
  }
  const int64_t t = e * kUmapOne;
  for (int64_t j = rb + g; j < re; j += kUmapGroup) {
    const int64_t Ej = E[j];
    if (Ej < kUmapOne) continue;  // (no period below one epoch: nothing to divide by)
    const int64_t c = t / Ej;
    if (t - c * Ej >= kUmapOne) continue;  // c(e) == c(e - 1): not active
    const int u = cols[j];
    if ((unsigned)u >= (unsigned)n) continue;
    double diff[DIM], d2 = 0.0;
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
      diff[d] = yv[d] - Yin[(int64_t)u * DIM + d];
      d2 = d2 + diff[d] * diff[d];
    }
    if (d2 > 0.0) {
      const double pw = pow(d2, b);
      const double coef = (-2.0 * a * b * (pw / d2)) / (1.0 + a * pw);
#pragma unroll
      for (int d = 0; d < DIM; ++d) acc[d] = acc[d] + clip4(coef * diff[d]);
    }
    const int64_t p = ((c - 1) * Ej + (kUmapOne - 1)) / kUmapOne;  // the previous activation (0: none)
    const int64_t nneg = (t * rate) / Ej - (p * kUmapOne * rate) / Ej;
    const uint64_t hj = splitmix64(key ^ (uint64_t)j);
    for (int64_t s = 0; s < nneg; ++s) {
      const uint64_t h = splitmix64(hj + (uint64_t)s);
      const int64_t k = (int64_t)(((h >> 32) * (uint64_t)n) >> 32);  // < n
      if (k == v) continue;
      d2 = 0.0;
#pragma unroll
      for (int d = 0; d < DIM; ++d) {
        diff[d] = yv[d] - Yin[k * DIM + d];
        d2 = d2 + diff[d] * diff[d];
      }
      if (d2 > 0.0) {
        const double pw = pow(d2, b);
        const double coef = (2.0 * gamma * b) / ((0.001 + d2) * (1.0 + a * pw));
#pragma unroll
        for (int d = 0; d < DIM; ++d) acc[d] = acc[d] + clip4(coef * diff[d]);
      }
    }
  }
#pragma unroll
  for (int off = kUmapGroup / 2; off > 0; off >>= 1) {
#pragma unroll
    for (int d = 0; d < DIM; ++d) acc[d] = acc[d] + __shfl_xor(acc[d], off, 64);
  }
  if (valid && g == 0) {
#pragma unroll
    for (int d = 0; d < DIM; ++d) Yout[v * DIM + d] = yv[d] + alpha_e * acc[d];
  }
}

}  // namespace

extern "C" {

int mu_umap_max_components(void) { return kUmapMaxComponents; }

int mu_umap_epoch_f64(int64_t n, int64_t nnz, const int64_t* d_indptr, const int32_t* d_cols, const int64_t* d_E,
                      int n_components, int epoch, int n_epochs, int rate, double a, double b, double gamma,
                      double alpha_e, uint64_t seed, const double* d_Y_in, double* d_Y_out, void* stream) {
  MU_REQUIRE(n >= 0 && n < ((int64_t)1 << 31) && nnz >= 0, "bad shape");
  MU_REQUIRE(n_components >= 2 && n_components <= kUmapMaxComponents, "n_components must be 2 or 3");
  MU_REQUIRE(n_epochs >= 1 && n_epochs <= kUmapMaxEpochs, "n_epochs must be 1..2^20");
  MU_REQUIRE(epoch >= 1 && epoch <= n_epochs, "epoch must be 1..n_epochs");
  MU_REQUIRE(rate >= 0 && rate <= kUmapMaxRate, "rate must be 0..1024");
  MU_REQUIRE(a > 0.0 && b > 0.0 && gamma == gamma && alpha_e == alpha_e, "a and b must be positive, gamma and alpha_e numbers");
  MU_REQUIRE(n == 0 || (d_indptr && d_Y_in && d_Y_out), "null pointer");
  MU_REQUIRE(nnz == 0 || (d_cols && d_E), "null pointer");
  MU_REQUIRE(n == 0 || d_Y_in != d_Y_out, "Y_in and Y_out must be two buffers");
  if (n == 0) return MU_OK;
  const int64_t blocks = (n + (256 / kUmapGroup) - 1) / (256 / kUmapGroup);  // < 2^27: one grid dimension
  const uint64_t key = splitmix64(seed + (uint64_t)epoch);
  hipStream_t st = (hipStream_t)stream;
#define MU_UMAP_EPOCH(DD)                                                                                             \
  hipLaunchKernelGGL(k_umap_epoch<DD>, dim3((unsigned)blocks), dim3(256), 0, st, (int)n, nnz, d_indptr, d_cols, d_E,  \
                     (int64_t)epoch, (int64_t)rate, a, b, gamma, alpha_e, key, d_Y_in, d_Y_out)
  if (n_components == 2) {
    MU_UMAP_EPOCH(2);
  } else {
    MU_UMAP_EPOCH(3);
  }
#undef MU_UMAP_EPOCH
  MU_CHECK_LAUNCH();
  return MU_OK;
}

}  // extern "C"
