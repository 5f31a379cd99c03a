// Per-group peak statistics on the device CSR of X^T: what scanpy's rank_genes_groups (the call under
// muon.atac.tl.rank_peaks_groups, muon/_atac/tools.py:337-373) needs from a matrix that is resident in HBM.
//
// Both kernels walk X^T as a CSR (rows: peaks; indices: cells) next to a per-cell int32 label table (0 .. B-1: the
// cell's bucket, -1: the cell does not take part; 4 B/cell, it stays in L2).  A workgroup of four waves takes four
// consecutive rows at a time.  A row of at most kRankCap entries belongs to one wave; a longer one is cut into four
// contiguous pieces, one per wave, and wave 0 combines the pieces in piece order.  Inside a piece a wave stages 64
// entries in LDS and lane l, the owner of bucket l, walks the staged entries in stored order: no atomics, every output
// written once, and the order of every addition is a function of the row's length alone - two calls agree bit for bit.
//
//  * k_group_moments: sum, sum of squares (f64) and the count of non-zero values per (peak, bucket).
//    8 B/entry (f32) or 12 B/entry (f64) read plus the label gather.
//  * k_rank_sums: the rows come sorted by value.  Tie-averaged ranks over all labelled cells, the implicit and the
//    explicitly stored zeros as ONE tie block between the negative and the positive values.  The walk keeps the open
//    run of equal values (value, first position, per-bucket count) and settles a run when the value changes; a piece
//    hands its first and its last run on unsettled, so a run that crosses a piece boundary is joined by the combiner.
//
// Limit: positions and counts inside one row are `int`, so a row of X^T holds fewer than 2^31 entries.  The entry
// points ask for n_cells < 2^31, which bounds the rows of a canonical CSR (one entry per cell at most); ranks and their
// sums are formed in double from those counts.
#include "common.hpp"

constexpr int kRankThreads = 256;
constexpr int kRankWaves = kRankThreads / 64;
constexpr int kRankCap = 256;        // a longer row is split over the workgroup's waves
constexpr int kRankMaxGroups = 64;   // one lane per bucket

struct RankStage {  // one staged entry, read by every lane at once (an LDS broadcast)
  double v;
  int32_t lab;
  int32_t nz;  // value != 0: the moments' count (the rank walk stages non-zero entries only and leaves it alone)
};

// entries [lo, hi) of a row cut into kRankWaves contiguous pieces of a multiple of 64 entries
__device__ __forceinline__ void rank_piece(int64_t lo, int64_t hi, int w, int64_t& plo, int64_t& phi) {
  const int64_t len = hi - lo;
  const int64_t pl = ((len + kRankWaves - 1) / kRankWaves + 63) & ~(int64_t)63;
  plo = lo + (int64_t)w * pl;
  phi = plo + pl;
  if (plo > hi) plo = hi;
  if (phi > hi) phi = hi;
}

__device__ __forceinline__ void rank_row_range(const int64_t* __restrict__ indptr, int64_t row, int64_t nnz, int64_t& lo,
                                               int64_t& hi) {
  lo = uniform64(indptr[row]);
  hi = uniform64(indptr[row + 1]);
  if (lo < 0) lo = 0;  // (a row never reaches outside the entry arrays, whatever indptr holds)
  if (hi > nnz) hi = nnz;
  if (hi < lo) hi = lo;
}

// ---------------------------------------------------------------------------------
// moments
// ---------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void moments_piece(int64_t lo, int64_t hi, int64_t n_cells, const int32_t* __restrict__ cells,
                                              const T* __restrict__ values, const int32_t* __restrict__ labels,
                                              RankStage* __restrict__ st, int lane, double& s, double& ss, int& c) {
  for (int64_t p0 = lo; p0 < hi; p0 += 64) {
    const int64_t p = p0 + lane;
    int32_t lab = -1;
    double v = 0.0;
    if (p < hi) {
      const int32_t cell = cells[p];
      if ((uint32_t)cell < (uint64_t)n_cells) lab = labels[cell];
      v = (double)values[p];
    }
    st[lane].v = v;
    st[lane].lab = lab;
    st[lane].nz = (v != 0.0) ? 1 : 0;  // NaN counts; an explicitly stored zero does not
    wave_lds_sync();
    const int cnt = (hi - p0) < 64 ? (int)(hi - p0) : 64;  // wave-uniform
    for (int i = 0; i < cnt; ++i) {
      const RankStage e = st[i];
      const bool mine = e.lab == lane;
      const double x = mine ? e.v : 0.0;
      s += x;
      ss = fma(x, x, ss);
      c += mine ? e.nz : 0;
    }
    wave_lds_sync();
  }
}

template <typename T>
__global__ __launch_bounds__(kRankThreads) void k_group_moments(int64_t d, int64_t n_cells, int64_t nnz, int B,
                                                                const int64_t* __restrict__ indptr,
                                                                const int32_t* __restrict__ cells,
                                                                const T* __restrict__ values,
                                                                const int32_t* __restrict__ labels,
                                                                double* __restrict__ out_sum,
                                                                double* __restrict__ out_sumsq,
                                                                int64_t* __restrict__ out_nnz) {
  __shared__ RankStage stage[kRankWaves][64];
  __shared__ double p_s[kRankWaves][64], p_ss[kRankWaves][64];
  __shared__ int p_c[kRankWaves][64];
  const int wave = uniform32(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int64_t n_quads = (d + kRankWaves - 1) / kRankWaves;
  for (int64_t q = blockIdx.x; q < n_quads; q += gridDim.x) {
    // rows that one wave takes whole
    {
      const int64_t row = q * kRankWaves + wave;
      if (row < d) {
        int64_t lo, hi;
        rank_row_range(indptr, row, nnz, lo, hi);
        if (hi - lo <= kRankCap) {
          double s = 0.0, ss = 0.0;
          int c = 0;
          moments_piece<T>(lo, hi, n_cells, cells, values, labels, stage[wave], lane, s, ss, c);
          if (lane < B) {
            out_sum[row * B + lane] = s;
            out_sumsq[row * B + lane] = ss;
            out_nnz[row * B + lane] = c;
          }
        }
      }
    }
    // long rows: four pieces, combined in piece order
    for (int r = 0; r < kRankWaves; ++r) {
      const int64_t row = q * kRankWaves + r;
      if (row >= d) break;  // (uniform over the workgroup)
      int64_t lo, hi;
      rank_row_range(indptr, row, nnz, lo, hi);
      if (hi - lo <= kRankCap) continue;  // (uniform over the workgroup)
      int64_t plo, phi;
      rank_piece(lo, hi, wave, plo, phi);
      double s = 0.0, ss = 0.0;
      int c = 0;
      moments_piece<T>(plo, phi, n_cells, cells, values, labels, stage[wave], lane, s, ss, c);
      p_s[wave][lane] = s;
      p_ss[wave][lane] = ss;
      p_c[wave][lane] = c;
      __syncthreads();
      if (wave == 0 && lane < B) {
        double ts = p_s[0][lane], tss = p_ss[0][lane];
        int64_t tc = p_c[0][lane];
        for (int w = 1; w < kRankWaves; ++w) {
          ts += p_s[w][lane];
          tss += p_ss[w][lane];
          tc += p_c[w][lane];
        }
        out_sum[row * B + lane] = ts;
        out_sumsq[row * B + lane] = tss;
        out_nnz[row * B + lane] = tc;
      }
      __syncthreads();
    }
  }
}

// ---------------------------------------------------------------------------------
// rank sums
// ---------------------------------------------------------------------------------
// What a wave knows of its piece.  Positions count the piece's labelled non-zero entries from 0.  The first run, and
// the last one if the piece holds more than one, are handed on as they are; the runs in between are settled with
// piece-local positions (rs: sum of local rank x count; closed: entries settled; posc: of those, not negative).
struct RankPiece {
  double rs[64];
  int closed[64], posc[64], firstc[64], lastc[64];
  double tie, fv, lv;
  int K, neg, flen, llen;  // labelled non-zero entries; negative ones; lengths of the first / last run (llen 0: one run)
};

struct RankRun {  // the open run of the walk; `cnt` is the lane's own bucket, the rest is the same in every lane
  double cur;
  int s, pos, cnt;
  bool have;
};

template <typename T>
__device__ __forceinline__ void ranks_piece(int64_t lo, int64_t hi, int64_t n_cells, const int32_t* __restrict__ cells,
                                            const T* __restrict__ values, const int32_t* __restrict__ labels,
                                            RankStage* __restrict__ st, RankPiece* __restrict__ out, int lane) {
  const unsigned long long below = (1ull << lane) - 1ull;
  RankRun run = {0.0, 0, 0, 0, false};
  bool first = true;  // the open run is the piece's first
  double rs = 0.0, tie = 0.0, fv = 0.0;
  int closed = 0, posc = 0, firstc = 0, flen = 0, neg = 0;
  for (int64_t p0 = lo; p0 < hi; p0 += 64) {
    const int64_t p = p0 + lane;
    int32_t lab = -1;
    double v = 0.0;
    if (p < hi) {
      const int32_t cell = cells[p];
      if ((uint32_t)cell < (uint64_t)n_cells) lab = labels[cell];
      v = (double)values[p];
    }
    // only the labelled non-zero entries are staged, in stored order (zeros, stored or not, are one block)
    const bool keep = lab >= 0 && v != 0.0;
    const unsigned long long m = __ballot(keep);
    neg += __popcll(__ballot(keep && v < 0.0));
    if (keep) {
      const int at = __popcll(m & below);
      st[at].v = v;
      st[at].lab = lab;
    }
    wave_lds_sync();
    const int cnt = __popcll(m);  // wave-uniform
    for (int i = 0; i < cnt; ++i) {
      const double ev = st[i].v;
      const int32_t el = st[i].lab;
      if (!run.have || !(ev == run.cur)) {
        if (run.have) {
          if (first) {
            fv = run.cur;
            flen = run.pos;
            firstc = run.cnt;
            first = false;
          } else {
            const double t = (double)(run.pos - run.s);
            rs += 0.5 * ((double)run.s + (double)run.pos + 1.0) * (double)run.cnt;  // ranks s+1 .. pos, averaged
            closed += run.cnt;
            if (!(run.cur < 0.0)) posc += run.cnt;
            tie += t * t * t - t;
          }
        }
        run.cur = ev;
        run.s = run.pos;
        run.cnt = 0;
        run.have = true;
      }
      run.cnt += (el == lane) ? 1 : 0;
      ++run.pos;
    }
    wave_lds_sync();
  }
  out->rs[lane] = rs;
  out->closed[lane] = closed;
  out->posc[lane] = posc;
  if (first) {  // no run, or one
    out->firstc[lane] = run.cnt;
    out->lastc[lane] = 0;
  } else {
    out->firstc[lane] = firstc;
    out->lastc[lane] = run.cnt;
  }
  if (lane == 0) {
    out->tie = tie;
    out->K = run.pos;
    out->neg = neg;
    if (first) {
      out->fv = run.cur;
      out->flen = run.pos;
      out->lv = 0.0;
      out->llen = 0;
    } else {
      out->fv = fv;
      out->flen = flen;
      out->lv = run.cur;
      out->llen = run.pos - run.s;
    }
  }
}

// settle the open run at global positions [s, pos)
__device__ __forceinline__ void rank_settle(RankRun& run, double& rs, int& posc, double& tie) {
  if (run.have) {
    const double t = (double)(run.pos - run.s);
    rs += 0.5 * ((double)run.s + (double)run.pos + 1.0) * (double)run.cnt;
    if (!(run.cur < 0.0)) posc += run.cnt;
    tie += t * t * t - t;
  }
  run.cnt = 0;
  run.have = false;
}

// one wave (lane = bucket) joins `n_pieces` pieces in order and writes the row's outputs
__device__ __forceinline__ void ranks_combine(const RankPiece* __restrict__ pieces, int n_pieces, int64_t n_kept,
                                              int64_t row, int B, int lane, double* __restrict__ out_ranksum,
                                              double* __restrict__ out_zero_rank, double* __restrict__ out_tie) {
  RankRun run = {0.0, 0, 0, 0, false};
  double rs = 0.0, tie = 0.0;
  int posc = 0, neg = 0;
  for (int w = 0; w < n_pieces; ++w) {
    const RankPiece* pc = pieces + w;
    const int K = pc->K;
    if (K == 0) continue;
    neg += pc->neg;
    const int P = run.pos;  // global position of the piece's first entry
    const double fv = pc->fv;
    if (!(run.have && fv == run.cur)) {
      rank_settle(run, rs, posc, tie);
      run.cur = fv;
      run.s = run.pos;
      run.have = true;
    }
    run.cnt += pc->firstc[lane];
    run.pos += pc->flen;
    if (pc->llen > 0) {
      rank_settle(run, rs, posc, tie);
      rs += pc->rs[lane] + (double)P * (double)pc->closed[lane];
      posc += pc->posc[lane];
      tie += pc->tie;
      run.cur = pc->lv;
      run.s = P + K - pc->llen;
      run.pos = P + K;
      run.cnt = pc->lastc[lane];
      run.have = true;
    }
  }
  rank_settle(run, rs, posc, tie);
  const double z = (double)(n_kept - (int64_t)run.pos);  // the zero block: implicit and explicitly stored zeros
  if (lane < B) out_ranksum[row * B + lane] = rs + z * (double)posc;
  if (lane == 0) {
    out_zero_rank[row] = (double)neg + 0.5 * (z + 1.0);
    out_tie[row] = tie + (z * z * z - z);
  }
}

template <typename T>
__global__ __launch_bounds__(kRankThreads) void k_rank_sums(int64_t d, int64_t n_cells, int64_t nnz, int B,
                                                            int64_t n_kept, const int64_t* __restrict__ indptr,
                                                            const int32_t* __restrict__ cells,
                                                            const T* __restrict__ values,
                                                            const int32_t* __restrict__ labels,
                                                            double* __restrict__ out_ranksum,
                                                            double* __restrict__ out_zero_rank,
                                                            double* __restrict__ out_tie) {
  __shared__ RankStage stage[kRankWaves][64];
  __shared__ RankPiece pieces[kRankWaves];
  const int wave = uniform32(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int64_t n_quads = (d + kRankWaves - 1) / kRankWaves;
  for (int64_t q = blockIdx.x; q < n_quads; q += gridDim.x) {
    {
      const int64_t row = q * kRankWaves + wave;
      if (row < d) {
        int64_t lo, hi;
        rank_row_range(indptr, row, nnz, lo, hi);
        if (hi - lo <= kRankCap) {
          ranks_piece<T>(lo, hi, n_cells, cells, values, labels, stage[wave], &pieces[wave], lane);
          wave_lds_sync();
          ranks_combine(&pieces[wave], 1, n_kept, row, B, lane, out_ranksum, out_zero_rank, out_tie);
        }
      }
    }
    __syncthreads();
    for (int r = 0; r < kRankWaves; ++r) {
      const int64_t row = q * kRankWaves + r;
      if (row >= d) break;  // (uniform over the workgroup)
      int64_t lo, hi;
      rank_row_range(indptr, row, nnz, lo, hi);
      if (hi - lo <= kRankCap) continue;  // (uniform over the workgroup)
      int64_t plo, phi;
      rank_piece(lo, hi, wave, plo, phi);
      ranks_piece<T>(plo, phi, n_cells, cells, values, labels, stage[wave], &pieces[wave], lane);
      __syncthreads();
      if (wave == 0) ranks_combine(pieces, kRankWaves, n_kept, row, B, lane, out_ranksum, out_zero_rank, out_tie);
      __syncthreads();
    }
  }
}

extern "C" {

int mu_group_moments_max_groups(void) { return kRankMaxGroups; }
int mu_rank_row_cap(void) { return kRankCap; }

static int rank_check(int dtype, int64_t d, int64_t n_cells, int64_t nnz, int n_buckets, const void* indptr,
                      const void* cells, const void* values, const void* labels) {
  MU_REQUIRE(d >= 0 && n_cells >= 0 && nnz >= 0, "negative shape");
  MU_REQUIRE(n_cells < (int64_t)1 << 31, "cell indices are int32");
  MU_REQUIRE(dtype == MU_DTYPE_F32 || dtype == MU_DTYPE_F64, "dtype must be f32 or f64");
  MU_REQUIRE(n_buckets >= 1 && n_buckets <= kRankMaxGroups, "1 <= n_buckets <= mu_group_moments_max_groups()");
  MU_REQUIRE(indptr, "null pointer");
  MU_REQUIRE(nnz == 0 || (cells && values), "null pointer");
  MU_REQUIRE(n_cells == 0 || labels, "null pointer");
  return MU_OK;
}

int mu_group_moments(int dtype, int64_t d, int64_t n_cells, int64_t nnz, int n_buckets, const int64_t* d_indptr,
                     const int32_t* d_cells, const void* d_values, const int32_t* d_labels, double* d_sum,
                     double* d_sumsq, int64_t* d_nnz, void* stream) {
  int rc = rank_check(dtype, d, n_cells, nnz, n_buckets, d_indptr, d_cells, d_values, d_labels);
  if (rc) return rc;
  if (d == 0) return MU_OK;
  MU_REQUIRE(d_sum && d_sumsq && d_nnz, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  by_dtype(dtype, [&](auto t) {
    hipLaunchKernelGGL(k_group_moments<decltype(t)>, dim3(wave_grid(d, kRankWaves, 8)), dim3(kRankThreads), 0, st, d,
                       n_cells, nnz, n_buckets, d_indptr, d_cells, (const decltype(t)*)d_values, d_labels, d_sum, d_sumsq,
                       d_nnz);
  });
  MU_CHECK_LAUNCH();
  return MU_OK;
}

int mu_rank_sums(int dtype, int64_t d, int64_t n_cells, int64_t nnz, int n_buckets, int64_t n_kept,
                 const int64_t* d_indptr, const int32_t* d_cells, const void* d_values, const int32_t* d_labels,
                 double* d_ranksum, double* d_zero_rank, double* d_tie, void* stream) {
  int rc = rank_check(dtype, d, n_cells, nnz, n_buckets, d_indptr, d_cells, d_values, d_labels);
  if (rc) return rc;
  MU_REQUIRE(n_kept >= 0 && n_kept <= n_cells, "0 <= n_kept <= n_cells");
  if (d == 0) return MU_OK;
  MU_REQUIRE(d_ranksum && d_zero_rank && d_tie, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  by_dtype(dtype, [&](auto t) {
    hipLaunchKernelGGL(k_rank_sums<decltype(t)>, dim3(wave_grid(d, kRankWaves, 8)), dim3(kRankThreads), 0, st, d, n_cells,
                       nnz, n_buckets, n_kept, d_indptr, d_cells, (const decltype(t)*)d_values, d_labels, d_ranksum,
                       d_zero_rank, d_tie);
  });
  MU_CHECK_LAUNCH();
  return MU_OK;
}

}  // extern "C"
