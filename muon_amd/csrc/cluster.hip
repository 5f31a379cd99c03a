// muon.tl.leiden / muon.tl.louvain: the sub-round of the multiplex local moving and the fixed-order segmented sum
// (muon_amd/_core/cluster.py states the optimiser).  All arithmetic f64, labels int32, offsets int64.
//
//   k_cluster_move<L>   one WAVE per deciding vertex v.  The row of S (a CSR without its diagonal) is read 64 entries
//                       at a time; each lane gathers its neighbour's label (in refinement: only where the neighbour's
//                       bound equals v's).  Grouping by community inside the chunk takes no atomics: while lanes remain,
//                       the first remaining lane's community is broadcast, the lanes holding it are balloted, their
//                       weights are added by the xor butterfly (the others contribute 0.0: a fixed order), and lane 0
//                       adds the sum into the wave's own LDS table.  The table is addressed by the community id when the
//                       level has at most kClusterTable vertices, else by linear probing from a multiplicative hash; the
//                       probe runs wave-uniformly (every lane reads the same slot: a broadcast) and only lane 0 writes,
//                       so there is nothing to race.  Chunks go in order: every w(v, C) has one summation order.
//                       Then a lane per table entry computes score(C) = w - sum_l c_l (kout_v Kin_C + kin_v Kout_C) from
//                       K (P[v] taken out of the own community), applies the swap guard, and the wave takes the arg-max
//                       (largest score, ties to the smallest id - a total order, so the butterfly's order is immaterial).
//                       More distinct communities than the table holds: the wave stores 1 to *overflow and leaves its
//                       vertex where it is; the caller then runs the level's tensor formulation.
//   k_cluster_segsum    out[s] = sum of the f64 rows ptr[s] .. ptr[s + 1]: a wave per segment, lane j adds rows
//                       j, j + 64, ... in order, then the xor butterfly.
//
// Compiled with -ffp-contract=off: a score is the same roundings as the tensor formulation's.
#include "common.hpp"

#include <limits.h>

namespace {

constexpr int kClusterMaxLayers = 4;
constexpr int kClusterTable = 512;  // entries of a wave's table: 4 waves x (4 + 8 + 2) x 512 B = 28 KiB per workgroup,
                                    // five workgroups (20 waves) share the 160 KiB of a CU
constexpr int kClusterTableBits = 9;
constexpr int kWaves = 4;

struct ClusterCoef {
  double c[kClusterMaxLayers];
};

template <int L>
__global__ __launch_bounds__(256) void k_cluster_move(int64_t nverts, const int32_t* __restrict__ verts, int nv, int64_t nnz,
                                                      const int64_t* __restrict__ indptr, const int32_t* __restrict__ cols,
                                                      const double* __restrict__ vals, const int32_t* __restrict__ lab,
                                                      const int32_t* __restrict__ bound, const int32_t* __restrict__ size,
                                                      const double* __restrict__ P, const double* __restrict__ K,
                                                      ClusterCoef coef, int only_single, int direct,
                                                      int32_t* __restrict__ prop, double* __restrict__ score,
                                                      int32_t* __restrict__ overflow) {
  __shared__ int32_t s_key[kWaves][kClusterTable];
  __shared__ double s_val[kWaves][kClusterTable];
  __shared__ uint16_t s_list[kWaves][kClusterTable];
  const int lane = threadIdx.x & 63, wave = uniform32(threadIdx.x >> 6);
  const int64_t i = (int64_t)blockIdx.x * kWaves + wave;
  if (i >= nverts) return;  // (no workgroup barrier below: a wave may leave)
  const int v = uniform32(verts[i]);
  if ((unsigned)v >= (unsigned)nv) return;
  const int a = uniform32(lab[v]);
  if ((unsigned)a >= (unsigned)nv) return;
  const int sa = uniform32(size[a]);
  if (only_single && sa != 1) {
    if (lane == 0) {
      prop[v] = a;
      score[v] = 0.0;
    }
    return;
  }
  int32_t* key = s_key[wave];
  double* val = s_val[wave];
  uint16_t* list = s_list[wave];
  for (int s = lane; s < kClusterTable; s += 64) {
    key[s] = -1;
    val[s] = 0.0;
  }
  wave_lds_sync();
  int cnt = 0;
  bool full = false;
  // adds `sum` to community c's entry (wave-uniform arguments); sets `full` when c needs an entry and none is left.
  // No wave_lds_sync() between two calls: every key[] value the probe acts on comes out of uniform32(), that is from
  // lane 0's own load, and lane 0 is the only lane that stores to key[], val[] and list[] - one thread reading what it
  // wrote itself, in program order (the compiler may not move a may-alias load over the store, and a wave's LDS
  // accesses issue in order).  What the OTHER lanes read of the table (list[], key[], val[] in the score phase) they
  // read after the wave_lds_sync() that follows the last call.
  auto add = [&](int c, double sum) {
    unsigned slot = direct ? (unsigned)c : ((unsigned)c * 2654435761u) >> (32 - kClusterTableBits);
    int k = uniform32(key[slot]);
    if (!direct) {
      for (int probe = 1; k != c && k != -1 && probe < kClusterTable; ++probe) {
        slot = (slot + 1) & (kClusterTable - 1);
        k = uniform32(key[slot]);
      }
      if (k != c && k != -1) {
        full = true;
        return;
      }
    }
    if (k == -1) {
      if (lane == 0) {
        key[slot] = c;
        list[cnt] = (uint16_t)slot;
      }
      ++cnt;
    }
    if (lane == 0) val[slot] += sum;
  };
  add(a, 0.0);  // the own community is entry 0
  int64_t b = uniform64(indptr[v]), e = uniform64(indptr[v + 1]);
  if (b < 0) b = 0;
  if (e > nnz) e = nnz;
  const int bv = bound ? uniform32(bound[v]) : 0;
  for (int64_t j0 = b; j0 < e && !full; j0 += 64) {
    const int64_t j = j0 + lane;
    int c = -1;
    double w = 0.0;
    if (j < e) {
      const int u = cols[j];
      if ((unsigned)u < (unsigned)nv && (!bound || bound[u] == bv)) {
        c = lab[u];
        w = vals[j];
        if ((unsigned)c >= (unsigned)nv) c = -1;
      }
    }
    uint64_t act = __ballot(c >= 0);
    while (act && !full) {
      const int first = __ffsll((unsigned long long)act) - 1;
      const int cf = uniform32(__shfl(c, first, 64));
      const bool same = c == cf;
      const uint64_t m = __ballot(same);
      const double s = wave_sum_all(same ? w : 0.0);
      add(cf, s);
      act &= ~m;
    }
  }
  if (full) {
    if (lane == 0) {
      *overflow = 1;
      prop[v] = a;
      score[v] = 0.0;
    }
    return;
  }
  wave_lds_sync();
  double pv[2 * L];
#pragma unroll
  for (int t = 0; t < 2 * L; ++t) pv[t] = P[(int64_t)v * (2 * L) + t];
  const double ninf = -__builtin_huge_val();
  double best_s = ninf, own_s = 0.0;
  int best_c = INT_MAX;
  for (int t0 = 0; t0 < cnt; t0 += 64) {
    const int t = t0 + lane;
    double s = ninf;
    int c = INT_MAX;
    if (t < cnt) {
      const int slot = list[t];
      c = key[slot];
      const double w = val[slot];
      const double* Kc = K + (int64_t)c * (2 * L);
      double pen = 0.0;
#pragma unroll
      for (int l = 0; l < L; ++l) {
        double kout_c = Kc[2 * l], kin_c = Kc[2 * l + 1];
        if (c == a) {
          kout_c -= pv[2 * l];
          kin_c -= pv[2 * l + 1];
        }
        pen = pen + coef.c[l] * (pv[2 * l] * kin_c + pv[2 * l + 1] * kout_c);
      }
      s = w - pen;
      if (c != a && sa == 1 && size[c] == 1 && c > a) {  // the swap guard: no candidate
        s = ninf;
        c = INT_MAX;
      }
    }
    if (t0 == 0) own_s = __shfl(s, 0, 64);
    if (s > best_s || (s == best_s && c < best_c)) {
      best_s = s;
      best_c = c;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double os = __shfl_xor(best_s, off, 64);
    const int oc = __shfl_xor(best_c, off, 64);
    if (os > best_s || (os == best_s && oc < best_c)) {
      best_s = os;
      best_c = oc;
    }
  }
  if (lane == 0) {
    const bool move = best_c != a && best_s > own_s;
    prop[v] = move ? best_c : a;
    score[v] = move ? best_s : own_s;
  }
}

__global__ __launch_bounds__(256) void k_cluster_segsum(int64_t n, int64_t nseg, int w, const double* __restrict__ vals,
                                                        const int64_t* __restrict__ ptr, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t seg = (int64_t)blockIdx.x * kWaves + uniform32(threadIdx.x >> 6);
  if (seg >= nseg) return;
  int64_t b = uniform64(ptr[seg]), e = uniform64(ptr[seg + 1]);
  if (b < 0) b = 0;
  if (e > n) e = n;
  for (int col = 0; col < w; ++col) {
    double acc = 0.0;
    for (int64_t r = b + lane; r < e; r += 64) acc += vals[r * w + col];
    acc = wave_sum_all(acc);
    if (lane == 0) out[seg * w + col] = acc;
  }
}

}  // namespace

extern "C" {

int mu_cluster_max_table(void) { return kClusterTable; }
int mu_cluster_max_layers(void) { return kClusterMaxLayers; }

int mu_cluster_move_f64(int64_t nverts, const int32_t* d_verts, int64_t nv, int64_t nnz, const int64_t* d_indptr,
                        const int32_t* d_cols, const double* d_vals, const int32_t* d_labels, const int32_t* d_bound,
                        const int32_t* d_size, int n_layers, const double* d_P, const double* d_K, const double* h_coef,
                        int only_single, int32_t* d_prop, double* d_score, int32_t* d_overflow, void* stream) {
  MU_REQUIRE(nv >= 0 && nv < ((int64_t)1 << 31) && nnz >= 0, "bad shape");
  MU_REQUIRE(nverts >= 0 && nverts <= nv, "nverts must be 0..nv");
  MU_REQUIRE(n_layers >= 1 && n_layers <= kClusterMaxLayers, "n_layers must be 1..4");
  MU_REQUIRE(h_coef, "null coefficients");
  MU_REQUIRE(nverts == 0 || (d_verts && d_indptr && d_labels && d_size && d_P && d_K && d_prop && d_score && d_overflow),
             "null pointer");
  MU_REQUIRE(nnz == 0 || (d_cols && d_vals), "null pointer");
  if (nverts == 0) return MU_OK;
  const int64_t blocks = (nverts + kWaves - 1) / kWaves;
  ClusterCoef coef;
  for (int l = 0; l < kClusterMaxLayers; ++l) coef.c[l] = l < n_layers ? h_coef[l] : 0.0;
  const int direct = nv <= kClusterTable ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
#define MU_CLUSTER_MOVE(LL)                                                                                            \
  hipLaunchKernelGGL(k_cluster_move<LL>, dim3((unsigned)blocks), dim3(256), 0, st, nverts, d_verts, (int)nv, nnz,      \
                     d_indptr, d_cols, d_vals, d_labels, d_bound, d_size, d_P, d_K, coef, only_single ? 1 : 0, direct, \
                     d_prop, d_score, d_overflow)
  switch (n_layers) {
    case 1: MU_CLUSTER_MOVE(1); break;
    case 2: MU_CLUSTER_MOVE(2); break;
    case 3: MU_CLUSTER_MOVE(3); break;
    default: MU_CLUSTER_MOVE(4); break;
  }
#undef MU_CLUSTER_MOVE
  MU_CHECK_LAUNCH();
  return MU_OK;
}

int mu_cluster_segsum_f64(int64_t n, int64_t nseg, int w, const double* d_vals, const int64_t* d_ptr, double* d_out,
                          void* stream) {
  MU_REQUIRE(n >= 0 && nseg >= 0 && w >= 1, "bad shape");
  MU_REQUIRE((nseg + kWaves - 1) / kWaves < ((int64_t)1 << 31), "too many segments for one launch");
  MU_REQUIRE(d_ptr, "null pointer");
  MU_REQUIRE(nseg == 0 || d_out, "null pointer");
  MU_REQUIRE(n == 0 || d_vals, "null pointer");
  if (nseg == 0) return MU_OK;
  hipLaunchKernelGGL(k_cluster_segsum, dim3((unsigned)((nseg + kWaves - 1) / kWaves)), dim3(256), 0, (hipStream_t)stream,
                     n, nseg, w, d_vals, d_ptr, d_out);
  MU_CHECK_LAUNCH();
  return MU_OK;
}

}  // extern "C"
