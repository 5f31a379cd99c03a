// muon.prot.pp.dsb on the device (/root/reference/muon/_prot/preproc.py:161-198): the log-moments of the empty
// droplets and the per-cell two-component Gaussian mixtures.
//
// 1. Moments.  mean_j and std_j (ddof = 1) of log(x + pc) over the n empty droplets.  With t = log(x + pc) - log(pc)
//    a zero contributes nothing, so the sums S1_j = sum t, S2_j = sum t^2 run over the STORED entries of the CSR only:
//    mean = log(pc) + S1 / n,  var = (S2 - S1^2 / n) / (n - 1).  t >= 0 and mostly 0: S1^2 / n is a small part of S2
//    (no cancellation; centred on the matrix-wide mean of log(x + pc) it would be).  A wave owns a fixed range of rows
//    and walks them in order, its per-column accumulators in LDS (columns are unique inside a canonical row: no two
//    lanes meet); the partial sums of the waves are then added in wave order.  The partition depends on n alone: two
//    runs add the same numbers in the same order.
//
// 2. Fit.  A wave owns a cell.  Its d <= 1024 values live in registers, NPL = 1 / 2 / 4 / 8 / 16 per lane (value j in
//    lane j % 64, slot j / 64), with the responsibilities of both components next to them.  It runs scikit-learn's EM
//    (sklearn/mixture/_base.py fit_predict, _gaussian_mixture.py _estimate_gaussian_parameters / _estimate_log_gaussian_prob
//    for one feature) for covariance_type "tied" and then "full", statement by statement in f64; every sum is a lane-local
//    sum over the slots in order followed by the xor butterfly (the same tree in every lane, so all lanes hold the same
//    bits and the stopping rule is wave-uniform).  No contraction into fused multiply-adds: the host formulation
//    (muon_amd/_prot/preproc.py _em_torch) is the same statements as tensor operations.
#include "common.hpp"

#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int kProtMaxD = 1024;   // values per cell the fit kernel holds (16 per lane)
constexpr int kMomWaves = 2;      // waves per workgroup of the CSR moments kernel: 2 x 2 x d doubles of LDS (32 KiB at d = 1024)
constexpr int kMomMaxParts = 2048;
constexpr int kFitWaves = 4;

// log(v + pc); F32: what numpy computes for a float32 matrix (the sum and the logarithm rounded to f32)
template <typename T>
__device__ __forceinline__ double prot_log(T v, double pc) {
  if (sizeof(T) == 4) {
    const float s = (float)v + (float)pc;
    return (double)(float)log((double)s);
  }
  return log((double)v + pc);
}

__host__ __device__ inline int64_t mom_rows_per_part(int64_t n) {
  int64_t rpp = (n + kMomMaxParts - 1) / kMomMaxParts;
  return rpp < 16 ? 16 : rpp;
}

template <typename T>
__global__ __launch_bounds__(64 * kMomWaves) void k_prot_moments_csr(int64_t n, int d, const int64_t* __restrict__ indptr,
                                                                     const int32_t* __restrict__ indices,
                                                                     const T* __restrict__ values, double pc, double logpc,
                                                                     int64_t rpp, double* __restrict__ part) {
  extern __shared__ double mom_lds[];  // [kMomWaves][2][d]
  const int lane = threadIdx.x & 63, wave = uniform32(threadIdx.x >> 6);
  const int64_t g = (int64_t)blockIdx.x * kMomWaves + wave;
  const int64_t r0 = g * rpp;
  if (r0 >= n) return;  // (wave-uniform; no workgroup barrier below)
  const int64_t r1 = r0 + rpp < n ? r0 + rpp : n;
  double* a1 = mom_lds + (size_t)wave * 2 * d;
  double* a2 = a1 + d;
  for (int c = lane; c < d; c += 64) a1[c] = 0.0, a2[c] = 0.0;
  wave_lds_sync();
  for (int64_t r = r0; r < r1; ++r) {
    const int64_t e0 = uniform64(indptr[r]), e1 = uniform64(indptr[r + 1]);
    for (int64_t e = e0 + lane; e < e1; e += 64) {
      const int c = indices[e];
      if (c >= 0 && c < d) {
        const double t = prot_log<T>(values[e], pc) - logpc;
        a1[c] += t;
        a2[c] += t * t;
      }
    }
    wave_lds_sync();  // (rows longer than 64 entries and the next row come after this row's updates)
  }
  double* out = part + (size_t)g * 2 * d;
  for (int c = lane; c < d; c += 64) out[c] = a1[c], out[d + c] = a2[c];
}

template <typename T>
__global__ __launch_bounds__(256) void k_prot_moments_dense(int64_t n, int64_t d, const T* __restrict__ X, double pc,
                                                            double logpc, int64_t rpp, double* __restrict__ part) {
  const int64_t c = (int64_t)blockIdx.y * 256 + threadIdx.x;
  const int64_t g = blockIdx.x;
  const int64_t r0 = g * rpp, r1 = r0 + rpp < n ? r0 + rpp : n;
  if (c >= d) return;
  double s1 = 0.0, s2 = 0.0;
  for (int64_t r = r0; r < r1; ++r) {
    const double t = prot_log<T>(X[r * d + c], pc) - logpc;
    s1 += t;
    s2 += t * t;
  }
  part[(size_t)g * 2 * d + c] = s1;
  part[(size_t)g * 2 * d + d + c] = s2;
}

__global__ __launch_bounds__(256) void k_prot_moments_finish(int64_t n, int64_t d, int64_t parts, double logpc,
                                                             const double* __restrict__ part, double* __restrict__ mean,
                                                             double* __restrict__ sd) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= d) return;
  double s1 = 0.0, s2 = 0.0;
  for (int64_t g = 0; g < parts; ++g) {
    s1 += part[(size_t)g * 2 * d + c];
    s2 += part[(size_t)g * 2 * d + d + c];
  }
  const double nn = (double)n;
  mean[c] = logpc + s1 / nn;
  double num = s2 - s1 * s1 / nn;
  if (n > 1 && num < 0.0) num = 0.0;
  sd[c] = sqrt(num / (nn - 1.0));  // (n = 1: 0 / 0, numpy's nan)
}

// ---- the per-cell fit -------------------------------------------------------------------------------------------------
template <int K>
__device__ __forceinline__ void wave_sum_all_k(double (&v)[K]) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] += __shfl_xor(v[k], off, 64);
  }
}

struct GmmPar {
  double w0, w1, m0, m1, p0, p1;  // weights, means, precisions_cholesky (p0 == p1 when tied)
};

constexpr double kLog2Pi = 1.8378770664093453;  // np.log(2 * np.pi)
constexpr double kLn2 = 0.6931471805599453;
constexpr double kRegCovar = 1e-6;
constexpr double kNkEps = 10.0 * 2.220446049250313e-16;
constexpr double kTol = 1e-3;
constexpr int kMaxIter = 100;

// _estimate_log_prob_resp for one value: log p(x) and, when asked, the responsibilities exp(log_resp)
__device__ __forceinline__ double gmm_point(double x, const GmmPar& P, double ld0, double ld1, double lw0, double lw1,
                                            bool want_resp, double& r0, double& r1) {
  const double y0 = x * P.p0 - P.m0 * P.p0, y1 = x * P.p1 - P.m1 * P.p1;
  const double a0 = (-0.5 * (kLog2Pi + y0 * y0) + ld0) + lw0;
  const double a1 = (-0.5 * (kLog2Pi + y1 * y1) + ld1) + lw1;
  // scipy.special.logsumexp over two entries: the maxima leave the sum, log1p(rest / m) + log(m) + max
  double lpn;
  if (a0 == a1) {
    lpn = kLn2 + a0;
  } else {
    const double mx = a0 > a1 ? a0 : a1, mn = a0 > a1 ? a1 : a0;
    lpn = log1p(exp(mn - mx)) + mx;
  }
  if (want_resp) {
    r0 = exp(a0 - lpn);
    r1 = exp(a1 - lpn);
  }
  return lpn;
}

template <typename T, int NPL>
__global__ __launch_bounds__(64 * kFitWaves) void k_prot_dsb_fit(
    int64_t n, int d, const T* __restrict__ Xd, const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const T* __restrict__ values, double pc, const double* __restrict__ mean, const double* __restrict__ sd,
    const double* __restrict__ resp, int64_t resp_cell_stride, int64_t resp_model_stride, double* __restrict__ scaled,
    double* __restrict__ bg, double* __restrict__ bic, int32_t* __restrict__ niter) {
  __shared__ double rowbuf[kFitWaves][NPL * 64];
  const int lane = threadIdx.x & 63, wave = uniform32(threadIdx.x >> 6);
  const int64_t cell = (int64_t)blockIdx.x * kFitWaves + wave;
  if (cell >= n) return;  // (wave-uniform; only wave-level synchronisation below)
  constexpr bool kF32 = sizeof(T) == 4;
  double x[NPL];
  if (Xd != nullptr) {
#pragma unroll
    for (int s = 0; s < NPL; ++s) {
      const int j = s * 64 + lane;
      x[s] = j < d ? prot_log<T>(Xd[cell * (int64_t)d + j], pc) : 0.0;
    }
  } else {
    // a CSR row scattered over zeros (stored as the counts: the logarithm is taken once per value below)
    double* row = rowbuf[wave];
#pragma unroll
    for (int s = 0; s < NPL; ++s) row[s * 64 + lane] = 0.0;
    wave_lds_sync();
    const int64_t e0 = uniform64(indptr[cell]), e1 = uniform64(indptr[cell + 1]);
    for (int64_t e = e0 + lane; e < e1; e += 64) {
      const int c = indices[e];
      if (c >= 0 && c < d) row[c] = (double)values[e];
    }
    wave_lds_sync();
#pragma unroll
    for (int s = 0; s < NPL; ++s) {
      const int j = s * 64 + lane;
      x[s] = j < d ? prot_log<T>((T)row[s * 64 + lane], pc) : 0.0;
    }
  }
  // (log(x + pc) - mean_j) / std_j, the reference's statements in its order (:173-177)
  double x2 = 0.0;
#pragma unroll
  for (int s = 0; s < NPL; ++s) {
    const int j = s * 64 + lane;
    if (j < d) {
      double z = x[s] - mean[j];
      if (sd != nullptr) z = z / sd[j];
      if (kF32) z = (double)(float)z;
      x[s] = z;
      scaled[cell * (int64_t)d + j] = z;
      x2 += z * z;
    }
  }
  {
    double v[1] = {x2};
    wave_sum_all_k<1>(v);
    x2 = v[0];
  }
  const double nd = (double)d;
  double bics[2], mins[2];
  for (int model = 0; model < 2; ++model) {  // 0: tied, 1: full
    const bool full = model == 1;
    const double* R = resp + cell * resp_cell_stride + model * resp_model_stride;
    double r0[NPL], r1[NPL];
#pragma unroll
    for (int s = 0; s < NPL; ++s) {
      const int j = s * 64 + lane;
      r0[s] = 0.0, r1[s] = 0.0;
      if (j < d) {
        const double u0 = R[2 * j], u1 = R[2 * j + 1], su = u0 + u1;
        r0[s] = u0 / su;
        r1[s] = u1 / su;
      }
    }
    GmmPar P;
    double lower = -__builtin_inf();
    int it = 0;
    bool init = true;
    for (;;) {
      double lb = 0.0;
      if (!init) {
        // E step with the current parameters
        const double ld0 = log(P.p0), ld1 = log(P.p1), lw0 = log(P.w0), lw1 = log(P.w1);
#pragma unroll
        for (int s = 0; s < NPL; ++s) {
          const int j = s * 64 + lane;
          double q0, q1;
          const double lpn = gmm_point(x[s], P, ld0, ld1, lw0, lw1, true, q0, q1);
          const bool ok = j < d;
          r0[s] = ok ? q0 : 0.0;
          r1[s] = ok ? q1 : 0.0;
          lb += ok ? lpn : 0.0;
        }
      }
      // M step (_estimate_gaussian_parameters): nk, means, covariances, precisions_cholesky
      double v[5] = {0.0, 0.0, 0.0, 0.0, lb};
#pragma unroll
      for (int s = 0; s < NPL; ++s) {
        v[0] += r0[s];
        v[1] += r1[s];
        v[2] += r0[s] * x[s];
        v[3] += r1[s] * x[s];
      }
      wave_sum_all_k<5>(v);
      const double nk0 = v[0] + kNkEps, nk1 = v[1] + kNkEps;
      P.m0 = v[2] / nk0;
      P.m1 = v[3] / nk1;
      double c0, c1;
      if (full) {
        double cv[2] = {0.0, 0.0};
#pragma unroll
        for (int s = 0; s < NPL; ++s) {
          const double d0 = x[s] - P.m0, d1 = x[s] - P.m1;
          cv[0] += (r0[s] * d0) * d0;
          cv[1] += (r1[s] * d1) * d1;
        }
        wave_sum_all_k<2>(cv);
        c0 = cv[0] / nk0 + kRegCovar;
        c1 = cv[1] / nk1 + kRegCovar;
      } else {
        const double m2 = (nk0 * P.m0) * P.m0 + (nk1 * P.m1) * P.m1;
        c0 = c1 = (x2 - m2) / (nk0 + nk1) + kRegCovar;
      }
      P.p0 = 1.0 / sqrt(c0);
      P.p1 = 1.0 / sqrt(c1);
      if (init) {
        P.w0 = nk0 / nd;  // (_initialize: weights / n_samples, not renormalised)
        P.w1 = nk1 / nd;
        init = false;
        continue;
      }
      const double ws = nk0 + nk1;
      P.w0 = nk0 / ws;
      P.w1 = nk1 / ws;
      ++it;
      const double prev = lower;
      lower = v[4] / nd;
      const double change = lower - prev;
      const int stop = (fabs(change) < kTol) || it >= kMaxIter;
      if (__builtin_amdgcn_readfirstlane(stop)) break;
    }
    // score with the final parameters -> BIC
    const double ld0 = log(P.p0), ld1 = log(P.p1), lw0 = log(P.w0), lw1 = log(P.w1);
    double sc[1] = {0.0};
#pragma unroll
    for (int s = 0; s < NPL; ++s) {
      const int j = s * 64 + lane;
      double q0, q1;
      const double lpn = gmm_point(x[s], P, ld0, ld1, lw0, lw1, false, q0, q1);
      sc[0] += j < d ? lpn : 0.0;
    }
    wave_sum_all_k<1>(sc);
    const double score = sc[0] / nd;
    bics[model] = -2.0 * score * nd + (full ? 5.0 : 4.0) * log(nd);
    mins[model] = P.m0 < P.m1 ? P.m0 : P.m1;  // np.min
    if (P.m0 != P.m0 || P.m1 != P.m1) mins[model] = __builtin_nan("");
    if (lane == 0) {
      bic[cell * 2 + model] = bics[model];
      niter[cell * 2 + model] = it;
    }
  }
  if (lane == 0) {
    double b = bics[0] < bics[1] ? mins[0] : mins[1];
    if (kF32) b = (double)(float)b;
    bg[cell] = b;
  }
}

// what numpy's float32 arithmetic makes of the pseudocount and its logarithm
void prot_pc(int dtype, double pc, double* pc_out, double* logpc) {
  if (dtype == MU_DTYPE_F32) {
    const float p = (float)pc;
    *pc_out = (double)p;
    *logpc = (double)(float)log((double)p);
  } else {
    *pc_out = pc;
    *logpc = log(pc);
  }
}

}  // namespace

extern "C" {

int mu_prot_max_proteins(void) { return kProtMaxD; }

size_t mu_prot_moments_worksize(int64_t n, int64_t d) {
  if (n <= 0 || d <= 0) return 0;
  const int64_t rpp = mom_rows_per_part(n);
  const int64_t parts = (n + rpp - 1) / rpp;
  return (size_t)parts * 2 * (size_t)d * sizeof(double);
}

int mu_prot_log_moments_csr(int dtype, int64_t n, int64_t d, const int64_t* d_indptr, const int32_t* d_indices,
                            const void* d_values, double pseudocount, double* d_mean, double* d_std, void* d_work,
                            size_t work_bytes, void* stream) {
  MU_REQUIRE(dtype == MU_DTYPE_F32 || dtype == MU_DTYPE_F64, "dtype must be f32 or f64");
  MU_REQUIRE(n >= 1 && d >= 1 && d <= kProtMaxD, "shape out of range (1 <= d <= 1024, n >= 1)");
  MU_REQUIRE(pseudocount > 0.0, "pseudocount must be positive (zero: the dense formulation)");
  MU_REQUIRE(d_indptr && d_mean && d_std && d_work, "null pointer");
  MU_REQUIRE(work_bytes >= mu_prot_moments_worksize(n, d), "work buffer too small");
  double pc, logpc;
  prot_pc(dtype, pseudocount, &pc, &logpc);
  const int64_t rpp = mom_rows_per_part(n), parts = (n + rpp - 1) / rpp;
  const dim3 grid((unsigned)((parts + kMomWaves - 1) / kMomWaves)), block(64 * kMomWaves);
  const size_t lds = (size_t)kMomWaves * 2 * (size_t)d * sizeof(double);
  hipStream_t st = (hipStream_t)stream;
  by_dtype(dtype, [&](auto t) {
    hipLaunchKernelGGL(k_prot_moments_csr<decltype(t)>, grid, block, lds, st, n, (int)d, d_indptr, d_indices,
                       (const decltype(t)*)d_values, pc, logpc, rpp, (double*)d_work);
  });
  MU_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_prot_moments_finish, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, st, n, d, parts, logpc,
                     (const double*)d_work, d_mean, d_std);
  MU_CHECK_LAUNCH();
  return MU_OK;
}

int mu_prot_log_moments_dense(int dtype, int64_t n, int64_t d, const void* d_X, double pseudocount, double* d_mean,
                              double* d_std, void* d_work, size_t work_bytes, void* stream) {
  MU_REQUIRE(dtype == MU_DTYPE_F32 || dtype == MU_DTYPE_F64, "dtype must be f32 or f64");
  MU_REQUIRE(n >= 1 && d >= 1 && d < ((int64_t)1 << 31), "shape out of range");
  MU_REQUIRE(pseudocount > 0.0, "pseudocount must be positive");
  MU_REQUIRE(d_X && d_mean && d_std && d_work, "null pointer");
  MU_REQUIRE(work_bytes >= mu_prot_moments_worksize(n, d), "work buffer too small");
  double pc, logpc;
  prot_pc(dtype, pseudocount, &pc, &logpc);
  const int64_t rpp = mom_rows_per_part(n), parts = (n + rpp - 1) / rpp;
  const dim3 grid((unsigned)parts, (unsigned)((d + 255) / 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  by_dtype(dtype, [&](auto t) {
    hipLaunchKernelGGL(k_prot_moments_dense<decltype(t)>, grid, block, 0, st, n, d, (const decltype(t)*)d_X, pc, logpc,
                       rpp, (double*)d_work);
  });
  MU_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_prot_moments_finish, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, st, n, d, parts, logpc,
                     (const double*)d_work, d_mean, d_std);
  MU_CHECK_LAUNCH();
  return MU_OK;
}

int mu_prot_dsb_fit(int dtype, int64_t n, int64_t d, const void* d_X, const int64_t* d_indptr, const int32_t* d_indices,
                    const void* d_values, double pseudocount, const double* d_mean, const double* d_std,
                    const double* d_resp, int64_t resp_cell_stride, int64_t resp_model_stride, double* d_scaled,
                    double* d_bgmean, double* d_bic, int32_t* d_niter, void* stream) {
  MU_REQUIRE(dtype == MU_DTYPE_F32 || dtype == MU_DTYPE_F64, "dtype must be f32 or f64");
  MU_REQUIRE(n >= 0 && n < ((int64_t)1 << 33) && d >= 1 && d <= kProtMaxD, "shape out of range (1 <= d <= 1024)");
  MU_REQUIRE(pseudocount >= 0.0, "pseudocount cannot be negative");
  MU_REQUIRE(resp_cell_stride >= 0 && resp_model_stride >= 0, "negative stride");
  if (n == 0) return MU_OK;
  MU_REQUIRE(d_X || (d_indptr && (d_indices || !d_values)), "neither a dense matrix nor a CSR");
  MU_REQUIRE(d_mean && d_resp && d_scaled && d_bgmean && d_bic && d_niter, "null pointer");
  double pc, logpc;
  prot_pc(dtype, pseudocount, &pc, &logpc);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((n + kFitWaves - 1) / kFitWaves)), block(64 * kFitWaves);
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    by_width<64, 128, 256, 512, 1024>((int)d, [&](auto w) {  // NPL: proteins per lane
      hipLaunchKernelGGL((k_prot_dsb_fit<T, decltype(w)::value / 64>), grid, block, 0, st, n, (int)d, (const T*)d_X,
                         d_indptr, d_indices, (const T*)d_values, pc, d_mean, d_std, d_resp, resp_cell_stride,
                         resp_model_stride, d_scaled, d_bgmean, d_bic, d_niter);
    });
  });
  MU_CHECK_LAUNCH();
  return MU_OK;
}

}  // extern "C"
