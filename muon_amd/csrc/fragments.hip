// Fragment tools on the device: the loops of muon.atac.tl.count_fragments_features, tss_enrichment and nucleosome_signal
// (muon/_atac/tools.py:746-1201) over a fragment table that is resident in HBM (five int32 columns in file order, grouped
// by contig and sorted by start inside a contig, as every tabix-indexed file is).
//
//  * k_frag_ranges: one thread per window (contig, lo, hi): two binary searches in the contig's segment of `start` give
//    the candidates start > lo - max_len && start < hi.  No fragment is longer than max_len, so every fragment that
//    overlaps [lo, hi) is a candidate.
//  * k_frag_overlap_count / _emit: the work item is a chunk of 256 candidates of one window, a wave per chunk in four
//    steps of 64 lanes.  A lane tests tabix's overlap rule end > lo && start < hi and looks its barcode up in the table of
//    the caller's cells.  The count pass writes the passing pairs per chunk; after a prefix sum the emit pass stores
//    (cell * n_features + window, score | 1) at the slot a wave ballot and a popcount give: the output order is a function
//    of the input alone.  20 B per candidate (start, end, barcode, score, the table entry) per pass.
//  * k_frag_pileup: the same chunks over the TSS windows; a passing fragment adds +score at its first column and -score
//    behind its last one in a cells x (W + 1) difference array: two int32 atomics per fragment, order-independent.
//  * k_frag_pileup_scan: a wave per cell turns its row of differences into the pileup in place, 64 columns a step with a
//    carry, and sums the flanks and the centre as int64 on the way: the pileup is read once.
//  * k_frag_length_classes: a thread per fragment, an int32 atomic into cells x 2.
// All arithmetic is integer.
#include "common.hpp"

constexpr int kFragChunk = 256;  // candidates per work item
constexpr int kFragSteps = kFragChunk / 64;

// first index i in [lo, hi) with a[i] >= key (a ascending)
__device__ __forceinline__ int64_t lower_bound_i32(const int32_t* __restrict__ a, int64_t lo, int64_t hi, int64_t key) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if ((int64_t)a[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void k_frag_ranges(int64_t n_win, int64_t n_contigs, const int32_t* __restrict__ wchrom,
                                                     const int32_t* __restrict__ wlo, const int32_t* __restrict__ whi,
                                                     const int64_t* __restrict__ chrom_ptr,
                                                     const int32_t* __restrict__ start, int64_t max_len,
                                                     int64_t* __restrict__ rng_lo, int64_t* __restrict__ rng_len) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n_win) return;
  const int32_t c = wchrom[w];
  int64_t a = 0, b = 0;
  if (c >= 0 && (int64_t)c < n_contigs) {  // (a contig the table lacks: an empty range)
    const int64_t s0 = chrom_ptr[c], s1 = chrom_ptr[c + 1];
    int64_t lo = wlo[w];
    const int64_t hi = whi[w];
    if (lo < 0) lo = 0;  // no fragment has a negative coordinate
    a = lower_bound_i32(start, s0, s1, lo - max_len + 1);
    b = lower_bound_i32(start, a, s1, hi);
    if (b < a) b = a;
  }
  rng_lo[w] = a;
  rng_len[w] = b - a;
}

// the window of chunk c: the last w with chunk_ptr[w] <= c
__device__ __forceinline__ int64_t chunk_window(const int64_t* __restrict__ chunk_ptr, int64_t n_win, int64_t c) {
  return lower_bound_i64(chunk_ptr, 0, n_win + 1, c + 1) - 1;
}

struct FragCand {
  int32_t cell;   // row of the caller's object, -1: no overlap / unknown barcode / past the chunk's end
  int32_t start, end;
};

__device__ __forceinline__ FragCand frag_test(int64_t p, int64_t p_end, int32_t lo, int32_t hi,
                                              const int32_t* __restrict__ start, const int32_t* __restrict__ end,
                                              const int32_t* __restrict__ barcode, const int32_t* __restrict__ cell_of,
                                              int64_t n_barcodes, int64_t n_obs) {
  FragCand r{-1, 0, 0};
  if (p >= p_end) return r;
  r.start = start[p];
  r.end = end[p];
  if (r.end > lo && r.start < hi) {
    const int32_t b = barcode[p];
    if ((uint32_t)b < (uint64_t)n_barcodes) {
      const int32_t cell = cell_of[b];
      if (cell >= 0 && (int64_t)cell < n_obs) r.cell = cell;
    }
  }
  return r;
}

__global__ __launch_bounds__(256) void k_frag_overlap_count(
    int64_t n_win, int64_t n_chunks, const int64_t* __restrict__ chunk_ptr, const int64_t* __restrict__ rng_lo,
    const int64_t* __restrict__ rng_len, const int32_t* __restrict__ wlo, const int32_t* __restrict__ whi,
    const int32_t* __restrict__ start, const int32_t* __restrict__ end, const int32_t* __restrict__ barcode,
    const int32_t* __restrict__ cell_of, int64_t n_barcodes, int64_t n_obs, int64_t* __restrict__ chunk_cnt) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t c = wave0; c < n_chunks; c += n_waves) {
    const int64_t w = chunk_window(chunk_ptr, n_win, c);
    const int64_t p0 = rng_lo[w] + (c - chunk_ptr[w]) * kFragChunk, p_end = rng_lo[w] + rng_len[w];
    const int32_t lo = wlo[w] < 0 ? 0 : wlo[w], hi = whi[w];
    int cnt = 0;
#pragma unroll
    for (int u = 0; u < kFragSteps; ++u) {
      const FragCand f = frag_test(p0 + 64 * u + lane, p_end, lo, hi, start, end, barcode, cell_of, n_barcodes, n_obs);
      cnt += __popcll(__ballot(f.cell >= 0));
    }
    if (lane == 0) chunk_cnt[c] = cnt;
  }
}

__global__ __launch_bounds__(256) void k_frag_overlap_emit(
    int64_t n_win, int64_t n_chunks, const int64_t* __restrict__ chunk_ptr, const int64_t* __restrict__ rng_lo,
    const int64_t* __restrict__ rng_len, const int32_t* __restrict__ wlo, const int32_t* __restrict__ whi,
    const int32_t* __restrict__ start, const int32_t* __restrict__ end, const int32_t* __restrict__ barcode,
    const int32_t* __restrict__ score, const int32_t* __restrict__ cell_of, int64_t n_barcodes, int64_t n_obs,
    int64_t n_features, const int64_t* __restrict__ chunk_off, int64_t* __restrict__ keys, int32_t* __restrict__ vals) {
  const int lane = threadIdx.x & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t c = wave0; c < n_chunks; c += n_waves) {
    const int64_t w = chunk_window(chunk_ptr, n_win, c);
    const int64_t p0 = rng_lo[w] + (c - chunk_ptr[w]) * kFragChunk, p_end = rng_lo[w] + rng_len[w];
    const int32_t lo = wlo[w] < 0 ? 0 : wlo[w], hi = whi[w];
    int64_t dst = uniform64(chunk_off[c]);
    const int64_t dst_end = uniform64(chunk_off[c + 1]);  // (a chunk never writes past its own slots)
#pragma unroll
    for (int u = 0; u < kFragSteps; ++u) {
      const int64_t p = p0 + 64 * u + lane;
      const FragCand f = frag_test(p, p_end, lo, hi, start, end, barcode, cell_of, n_barcodes, n_obs);
      const unsigned long long m = __ballot(f.cell >= 0);
      const int64_t at = dst + __popcll(m & below);
      if (f.cell >= 0 && at < dst_end) {
        keys[at] = (int64_t)f.cell * n_features + w;
        vals[at] = score ? score[p] : 1;
      }
      dst += __popcll(m);
    }
  }
}

__global__ __launch_bounds__(256) void k_frag_pileup(
    int64_t n_win, int64_t n_chunks, const int64_t* __restrict__ chunk_ptr, const int64_t* __restrict__ rng_lo,
    const int64_t* __restrict__ rng_len, const int32_t* __restrict__ wlo, const int32_t* __restrict__ whi,
    const int32_t* __restrict__ start, const int32_t* __restrict__ end, const int32_t* __restrict__ barcode,
    const int32_t* __restrict__ score, const int32_t* __restrict__ cell_of, int64_t n_barcodes, int64_t n_obs, int W,
    int32_t* __restrict__ diff) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t c = wave0; c < n_chunks; c += n_waves) {
    const int64_t w = chunk_window(chunk_ptr, n_win, c);
    const int64_t p0 = rng_lo[w] + (c - chunk_ptr[w]) * kFragChunk, p_end = rng_lo[w] + rng_len[w];
    const int64_t tss = wlo[w];  // first position of the region: columns count from it, also where it is negative
    const int32_t lo = wlo[w] < 0 ? 0 : wlo[w], hi = whi[w];
#pragma unroll
    for (int u = 0; u < kFragSteps; ++u) {
      const int64_t p = p0 + 64 * u + lane;
      const FragCand f = frag_test(p, p_end, lo, hi, start, end, barcode, cell_of, n_barcodes, n_obs);
      if (f.cell < 0) continue;
      int64_t c0 = (int64_t)f.start - tss, c1 = (int64_t)f.end - tss;
      if (c0 < 0) c0 = 0;
      if (c1 > W) c1 = W;
      if (c0 >= c1) continue;  // (an empty slice adds nothing)
      const int32_t s = score ? score[p] : 1;
      int32_t* row = diff + (int64_t)f.cell * (W + 1);
      atomicAdd(row + c0, s);
      atomicAdd(row + c1, -s);
    }
  }
}

// inclusive prefix sum over the wave (valid in every lane)
__device__ __forceinline__ int32_t wave_scan_i32(int32_t v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int32_t t = __shfl_up(v, off, 64);
    if (lane >= off) v += t;
  }
  return v;
}

// flank columns: [0, f0) and [f1, W); centre columns: [c0, c1)
__global__ __launch_bounds__(256) void k_frag_pileup_scan(int64_t n_obs, int W, int f0, int f1, int c0, int c1,
                                                          int32_t* __restrict__ diff, int64_t* __restrict__ sums) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t i = wave0; i < n_obs; i += n_waves) {
    int32_t* row = diff + i * (W + 1);
    int32_t carry = 0;
    int64_t flank = 0, centre = 0;
    for (int j0 = 0; j0 < W; j0 += 64) {
      const int j = j0 + lane;
      const int32_t d = j < W ? row[j] : 0;
      const int32_t v = carry + wave_scan_i32(d, lane);
      if (j < W) {
        row[j] = v;
        if (j < f0 || j >= f1) flank += v;
        if (j >= c0 && j < c1) centre += v;
      }
      carry = __shfl(v, 63, 64);
    }
    flank = wave_sum(flank);
    centre = wave_sum(centre);
    if (lane == 0) {
      sums[2 * i] = flank;
      sums[2 * i + 1] = centre;
    }
  }
}

__global__ __launch_bounds__(256) void k_frag_length_classes(int64_t n_take, const int32_t* __restrict__ start,
                                                             const int32_t* __restrict__ end,
                                                             const int32_t* __restrict__ barcode,
                                                             const int32_t* __restrict__ cell_of, int64_t n_barcodes,
                                                             int64_t n_obs, int free_bound, int mono_bound,
                                                             int32_t* __restrict__ classes) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_take; p += stride) {
    const int32_t b = barcode[p];
    if ((uint32_t)b >= (uint64_t)n_barcodes) continue;
    const int32_t cell = cell_of[b];
    if (cell < 0 || (int64_t)cell >= n_obs) continue;  // (a fragment of an unknown barcode uses up its turn)
    const int64_t len = (int64_t)end[p] - (int64_t)start[p];
    if (len < free_bound)
      atomicAdd(classes + 2 * (int64_t)cell, 1);
    else if (len < mono_bound)
      atomicAdd(classes + 2 * (int64_t)cell + 1, 1);
  }
}

extern "C" {

int mu_frag_chunk(void) { return kFragChunk; }

int mu_frag_ranges(int64_t n_win, int64_t n_contigs, const int32_t* d_wchrom, const int32_t* d_wlo,
                   const int32_t* d_whi, const int64_t* d_chrom_ptr, const int32_t* d_start, int64_t max_len,
                   int64_t* d_rng_lo, int64_t* d_rng_len, void* stream) {
  MU_REQUIRE(n_win >= 0 && n_contigs >= 0 && max_len >= 0, "negative size");
  if (n_win == 0) return MU_OK;
  MU_REQUIRE(d_wchrom && d_wlo && d_whi && d_chrom_ptr && d_rng_lo && d_rng_len, "null pointer");
  hipLaunchKernelGGL(k_frag_ranges, dim3((unsigned)((n_win + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n_win,
                     n_contigs, d_wchrom, d_wlo, d_whi, d_chrom_ptr, d_start, max_len, d_rng_lo, d_rng_len);
  MU_CHECK_LAUNCH();
  return MU_OK;
}

int mu_frag_overlap_count(int64_t n_win, int64_t n_chunks, const int64_t* d_chunk_ptr, const int64_t* d_rng_lo,
                          const int64_t* d_rng_len, const int32_t* d_wlo, const int32_t* d_whi, const int32_t* d_start,
                          const int32_t* d_end, const int32_t* d_barcode, const int32_t* d_cell_of, int64_t n_barcodes,
                          int64_t n_obs, int64_t* d_chunk_cnt, void* stream) {
  MU_REQUIRE(n_win >= 0 && n_chunks >= 0 && n_barcodes >= 0 && n_obs >= 0, "negative size");
  if (n_chunks == 0) return MU_OK;
  MU_REQUIRE(d_chunk_ptr && d_rng_lo && d_rng_len && d_wlo && d_whi && d_start && d_end && d_barcode && d_cell_of &&
                 d_chunk_cnt, "null pointer");
  hipLaunchKernelGGL(k_frag_overlap_count, dim3(wave_grid(n_chunks, 4, 16)), dim3(256), 0, (hipStream_t)stream, n_win,
                     n_chunks, d_chunk_ptr, d_rng_lo, d_rng_len, d_wlo, d_whi, d_start, d_end, d_barcode, d_cell_of,
                     n_barcodes, n_obs, d_chunk_cnt);
  MU_CHECK_LAUNCH();
  return MU_OK;
}

int mu_frag_overlap_emit(int64_t n_win, int64_t n_chunks, const int64_t* d_chunk_ptr, const int64_t* d_rng_lo,
                         const int64_t* d_rng_len, const int32_t* d_wlo, const int32_t* d_whi, const int32_t* d_start,
                         const int32_t* d_end, const int32_t* d_barcode, const int32_t* d_score,
                         const int32_t* d_cell_of, int64_t n_barcodes, int64_t n_obs, int64_t n_features,
                         const int64_t* d_chunk_off, int64_t* d_keys, int32_t* d_vals, void* stream) {
  MU_REQUIRE(n_win >= 0 && n_chunks >= 0 && n_barcodes >= 0 && n_obs >= 0, "negative size");
  MU_REQUIRE(n_features >= n_win, "fewer features than windows");
  if (n_chunks == 0) return MU_OK;
  MU_REQUIRE(d_chunk_ptr && d_rng_lo && d_rng_len && d_wlo && d_whi && d_start && d_end && d_barcode && d_cell_of &&
                 d_chunk_off, "null pointer");
  hipLaunchKernelGGL(k_frag_overlap_emit, dim3(wave_grid(n_chunks, 4, 16)), dim3(256), 0, (hipStream_t)stream, n_win,
                     n_chunks, d_chunk_ptr, d_rng_lo, d_rng_len, d_wlo, d_whi, d_start, d_end, d_barcode, d_score,
                     d_cell_of, n_barcodes, n_obs, n_features, d_chunk_off, d_keys, d_vals);
  MU_CHECK_LAUNCH();
  return MU_OK;
}

int mu_frag_pileup(int64_t n_win, int64_t n_chunks, const int64_t* d_chunk_ptr, const int64_t* d_rng_lo,
                   const int64_t* d_rng_len, const int32_t* d_wlo, const int32_t* d_whi, const int32_t* d_start,
                   const int32_t* d_end, const int32_t* d_barcode, const int32_t* d_score, const int32_t* d_cell_of,
                   int64_t n_barcodes, int64_t n_obs, int64_t width, int32_t* d_diff, void* stream) {
  MU_REQUIRE(n_win >= 0 && n_chunks >= 0 && n_barcodes >= 0 && n_obs >= 0, "negative size");
  MU_REQUIRE(width >= 1 && width < ((int64_t)1 << 30), "region width out of range");
  if (n_chunks == 0 || n_obs == 0) return MU_OK;
  MU_REQUIRE(d_chunk_ptr && d_rng_lo && d_rng_len && d_wlo && d_whi && d_start && d_end && d_barcode && d_cell_of &&
                 d_diff, "null pointer");
  hipLaunchKernelGGL(k_frag_pileup, dim3(wave_grid(n_chunks, 4, 16)), dim3(256), 0, (hipStream_t)stream, n_win, n_chunks,
                     d_chunk_ptr, d_rng_lo, d_rng_len, d_wlo, d_whi, d_start, d_end, d_barcode, d_score, d_cell_of,
                     n_barcodes, n_obs, (int)width, d_diff);
  MU_CHECK_LAUNCH();
  return MU_OK;
}

int mu_frag_pileup_scan(int64_t n_obs, int64_t width, int64_t flank_size, int64_t center_dist, int32_t* d_diff,
                        int64_t* d_sums, void* stream) {
  MU_REQUIRE(n_obs >= 0, "negative size");
  MU_REQUIRE(width >= 1 && width < ((int64_t)1 << 30), "region width out of range");
  MU_REQUIRE(flank_size >= 0 && 2 * flank_size <= width, "flanks overlap");
  MU_REQUIRE(center_dist >= 0 && 2 * center_dist <= width, "centre is empty");
  if (n_obs == 0) return MU_OK;
  MU_REQUIRE(d_diff && d_sums, "null pointer");
  hipLaunchKernelGGL(k_frag_pileup_scan, dim3(wave_grid(n_obs, 4, 16)), dim3(256), 0, (hipStream_t)stream, n_obs,
                     (int)width, (int)flank_size, (int)(width - flank_size), (int)center_dist,
                     (int)(width - center_dist), d_diff, d_sums);
  MU_CHECK_LAUNCH();
  return MU_OK;
}

int mu_frag_length_classes(int64_t n_take, const int32_t* d_start, const int32_t* d_end, const int32_t* d_barcode,
                           const int32_t* d_cell_of, int64_t n_barcodes, int64_t n_obs, int free_bound, int mono_bound,
                           int32_t* d_classes, void* stream) {
  MU_REQUIRE(n_take >= 0 && n_barcodes >= 0 && n_obs >= 0, "negative size");
  if (n_take == 0 || n_obs == 0) return MU_OK;
  MU_REQUIRE(d_start && d_end && d_barcode && d_cell_of && d_classes, "null pointer");
  int64_t blocks = (n_take + 255) / 256;
  const int64_t cap = (int64_t)mu_num_cus() * 16;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(k_frag_length_classes, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, n_take, d_start,
                     d_end, d_barcode, d_cell_of, n_barcodes, n_obs, free_bound, mono_bound, d_classes);
  MU_CHECK_LAUNCH();
  return MU_OK;
}

}  // extern "C"
