// Motif scanning on the device: every window of every sequence scored against every position weight matrix
// (muon.atac.tl.scan_sequences, muon/_atac/tools.py:446-517; the arithmetic is stated in DESIGN.md 9.10).
//
// Sequences arrive as ONE stream of codes (0..3 = A C G T, 4 = anything else) with int64 offsets.  k_motif_room gives
// every stream position its "room": the number of valid bases from there to the next invalid code or to the end of
// its sequence, capped at kMotifCap.  A window of motif m at position p is admissible iff room[p] >= L_m.
//
// k_motif_scan: the bank comes sorted by length in tiles of 16 motifs; blockIdx.y is the motif tile, and a wave keeps
// the tile's matrix in registers for its whole life: column j as ONE B operand of v_mfma_f64_16x16x4_f64
// (lane (k, n) holds M_n[k, j]: the instruction's inner dimension is exactly the four bases).  The workgroup then
// walks position tiles of kMotifTile stream positions (grid-stride over blockIdx.x): codes (+ a halo of kMotifCap)
// and room go to LDS, every wave takes 64 positions as four 16-row sub-tiles, and for column j the A operand is the
// one-hot of code[p + j] (lane (k, i): code == k).  One term of every inner product is M[base, j], the other three are
// exact zeros, so the accumulator is the j-ascending f64 sum of the statement, rounding for rounding; columns past a
// shorter motif's end are zero columns.  Scores are compared in registers with the threshold and the room.
//
// Hits leave without atomics and without any dependence on the order of the workgroups: pass 1 (kWrite = false)
// writes the number of hits of every (motif tile, position tile); the caller takes an exclusive scan; pass 2
// (kWrite = true) skips the pairs without a hit, recomputes the others and writes every hit to its own slot (prefix
// over the lanes of a wave, then over the waves).  The caller orders the rows (sequence, motif, position).
#include "common.hpp"

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int kMotifCap = 32;       // longest motif the kernel takes (columns held in registers)
constexpr int kMotifTile = 256;     // stream positions per workgroup step
constexpr int kMotifThreads = 256;
constexpr int kMotifGroup = 16;     // motifs per tile: the N of the MFMA

// the sequence that holds stream position p: the last s with offsets[s] <= p (empty sequences own nothing)
__device__ __forceinline__ int64_t motif_seq_of(const int64_t* __restrict__ offsets, int64_t n_seq, int64_t p) {
  int64_t lo = 0, hi = n_seq;  // first s in [0, n_seq] with offsets[s] > p
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (offsets[mid] > p) hi = mid; else lo = mid + 1;
  }
  int64_t s = lo - 1;
  if (s < 0) s = 0;
  if (s > n_seq - 1) s = n_seq - 1;
  return s;
}

__global__ __launch_bounds__(256) void k_motif_room(int64_t total, int64_t n_seq, const uint8_t* __restrict__ codes,
                                                    const int64_t* __restrict__ offsets, uint8_t* __restrict__ room) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += step) {
    const int64_t s = motif_seq_of(offsets, n_seq, p);
    int64_t end = offsets[s + 1];
    if (end > total) end = total;  // (never past the stream, whatever the offsets hold)
    if (end > p + kMotifCap) end = p + kMotifCap;
    int r = 0;
    while (p + r < end && codes[p + r] < 4) ++r;
    room[p] = (uint8_t)r;
  }
}

template <bool kWrite>
__global__ __launch_bounds__(kMotifThreads) void k_motif_scan(
    int64_t total, int64_t n_seq, int64_t n_ptiles, const uint8_t* __restrict__ codes, const uint8_t* __restrict__ room,
    const int64_t* __restrict__ offsets, const double* __restrict__ bank, const int32_t* __restrict__ tile_len,
    const int32_t* __restrict__ mlen, const double* __restrict__ thr, const int32_t* __restrict__ orig,
    int32_t* __restrict__ counts, const int64_t* __restrict__ base, int64_t n_hits, int32_t* __restrict__ out_seq,
    int32_t* __restrict__ out_motif, int32_t* __restrict__ out_pos, double* __restrict__ out_score) {
  __shared__ uint8_t s_code[kMotifTile + kMotifCap];
  __shared__ uint8_t s_room[kMotifTile];
  __shared__ int s_wcnt[kMotifThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = uniform32(tid >> 6);
  const int lr = lane >> 4, lc = lane & 15;  // A: row lc, inner lr;  B: inner lr, column lc;  D[r]: row lr + 4 r, column lc
  const int t = blockIdx.y;
  int L = uniform32(tile_len[t]);
  if (L > kMotifCap) L = kMotifCap;

  // the tile's matrix: bank[t][j][k][n], column j as the B operand of step j
  double b[kMotifCap];
  {
    const double* bt = bank + (int64_t)t * kMotifCap * 64 + lane;
#pragma unroll
    for (int j = 0; j < kMotifCap; ++j) b[j] = (j < L) ? bt[j * 64] : 0.0;
  }
  const int m = t * kMotifGroup + lc;  // this lane's motif (sorted order)
  const double th = thr[m];
  const int ml = mlen[m];              // padding motifs: longer than any room

  for (int64_t pt = blockIdx.x; pt < n_ptiles; pt += gridDim.x) {
    const int64_t cidx = (int64_t)t * n_ptiles + pt;
    if (kWrite) {
      if (uniform32(counts[cidx]) == 0) continue;  // (uniform over the workgroup)
    }
    const int64_t g0 = pt * kMotifTile;
    __syncthreads();  // the previous tile is consumed
    for (int i = tid; i < kMotifTile + kMotifCap; i += kMotifThreads) {
      const int64_t g = g0 + i;
      s_code[i] = g < total ? codes[g] : (uint8_t)4;
    }
    {
      const int64_t g = g0 + tid;
      s_room[tid] = g < total ? room[g] : (uint8_t)0;  // (no room past the stream: nothing there is a hit)
    }
    __syncthreads();

    d4 acc[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) acc[s] = d4{0.0, 0.0, 0.0, 0.0};
    const uint8_t* cw = s_code + wave * 64 + lc;
#pragma unroll
    for (int j = 0; j < kMotifCap; ++j) {
      if (j < L) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const double a = ((int)cw[16 * s + j] == lr) ? 1.0 : 0.0;
          acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[j], acc[s], 0, 0, 0);
        }
      }
    }
    // acc[s][r]: the score of motif lc at tile position 64 wave + 16 s + lr + 4 r
    unsigned mask = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int p = wave * 64 + 16 * s + lr + 4 * r;
        const bool hit = acc[s][r] >= th && (int)s_room[p] >= ml;
        mask |= (hit ? 1u : 0u) << (4 * s + r);
      }
    }
    const int n = __popc(mask);
    // inclusive prefix of n over the lanes of the wave
    int incl = n;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    if (lane == 63) s_wcnt[wave] = incl;
    __syncthreads();
    if (!kWrite) {
      if (tid == 0) counts[cidx] = s_wcnt[0] + s_wcnt[1] + s_wcnt[2] + s_wcnt[3];
    } else if (n > 0) {
      int64_t o = base[cidx] + (incl - n);
      for (int w = 0; w < wave; ++w) o += s_wcnt[w];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (mask & (1u << (4 * s + r))) {
            const int64_t g = g0 + wave * 64 + 16 * s + lr + 4 * r;
            const int64_t sq = motif_seq_of(offsets, n_seq, g);
            if (o >= 0 && o < n_hits) {  // (a slot outside the arrays is never written, whatever `base` holds)
              out_seq[o] = (int32_t)sq;
              out_motif[o] = orig[m];
              out_pos[o] = (int32_t)(g - offsets[sq]);
              out_score[o] = acc[s][r];
            }
            ++o;
          }
        }
      }
    }
  }
}

extern "C" {

int mu_motif_max_len(void) { return kMotifCap; }
int mu_motif_tile(void) { return kMotifTile; }
int mu_motif_group(void) { return kMotifGroup; }

static int motif_check(int64_t total, int64_t n_seq, int n_mtiles) {
  MU_REQUIRE(total >= 0 && n_seq >= 1, "total >= 0 and n_seq >= 1");
  MU_REQUIRE(n_seq < (int64_t)1 << 31, "sequence indices are int32");
  MU_REQUIRE(n_mtiles >= 1 && n_mtiles <= 65535, "1 <= motif tiles <= 65535");
  return MU_OK;
}

static inline unsigned motif_grid_x(int64_t n_ptiles, int n_mtiles) {
  // enough workgroups to fill the chip eight deep, however few motif tiles there are
  int64_t want = ((int64_t)mu_num_cus() * 8 + n_mtiles - 1) / n_mtiles;
  if (want > n_ptiles) want = n_ptiles;
  if (want < 1) want = 1;
  return (unsigned)want;
}

int mu_motif_room(int64_t total, int64_t n_seq, const uint8_t* d_codes, const int64_t* d_offsets, uint8_t* d_room,
                  void* stream) {
  MU_REQUIRE(total >= 0 && n_seq >= 1, "total >= 0 and n_seq >= 1");
  if (total == 0) return MU_OK;
  MU_REQUIRE(d_codes && d_offsets && d_room, "null pointer");
  int64_t blocks = (total + 255) / 256;
  const int64_t cap = (int64_t)mu_num_cus() * 16;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(k_motif_room, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, total, n_seq, d_codes,
                     d_offsets, d_room);
  MU_CHECK_LAUNCH();
  return MU_OK;
}

int mu_motif_count(int64_t total, int64_t n_seq, int n_mtiles, const uint8_t* d_codes, const uint8_t* d_room,
                   const double* d_bank, const int32_t* d_tile_len, const int32_t* d_mlen, const double* d_thr,
                   int32_t* d_counts, void* stream) {
  int rc = motif_check(total, n_seq, n_mtiles);
  if (rc) return rc;
  if (total == 0) return MU_OK;
  MU_REQUIRE(d_codes && d_room && d_bank && d_tile_len && d_mlen && d_thr && d_counts, "null pointer");
  const int64_t n_ptiles = (total + kMotifTile - 1) / kMotifTile;
  hipLaunchKernelGGL(k_motif_scan<false>, dim3(motif_grid_x(n_ptiles, n_mtiles), (unsigned)n_mtiles),
                     dim3(kMotifThreads), 0, (hipStream_t)stream, total, n_seq, n_ptiles, d_codes, d_room,
                     (const int64_t*)nullptr, d_bank, d_tile_len, d_mlen, d_thr, (const int32_t*)nullptr, d_counts,
                     (const int64_t*)nullptr, (int64_t)0, (int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr,
                     (double*)nullptr);
  MU_CHECK_LAUNCH();
  return MU_OK;
}

int mu_motif_write(int64_t total, int64_t n_seq, int n_mtiles, const uint8_t* d_codes, const uint8_t* d_room,
                   const int64_t* d_offsets, const double* d_bank, const int32_t* d_tile_len, const int32_t* d_mlen,
                   const double* d_thr, const int32_t* d_orig, const int32_t* d_counts, const int64_t* d_base,
                   int64_t n_hits, int32_t* d_seq, int32_t* d_motif, int32_t* d_pos, double* d_score, void* stream) {
  int rc = motif_check(total, n_seq, n_mtiles);
  if (rc) return rc;
  MU_REQUIRE(n_hits >= 0, "negative hit count");
  if (total == 0 || n_hits == 0) return MU_OK;
  MU_REQUIRE(d_codes && d_room && d_offsets && d_bank && d_tile_len && d_mlen && d_thr && d_orig && d_counts && d_base,
             "null pointer");
  MU_REQUIRE(d_seq && d_motif && d_pos && d_score, "null pointer");
  const int64_t n_ptiles = (total + kMotifTile - 1) / kMotifTile;
  hipLaunchKernelGGL(k_motif_scan<true>, dim3(motif_grid_x(n_ptiles, n_mtiles), (unsigned)n_mtiles),
                     dim3(kMotifThreads), 0, (hipStream_t)stream, total, n_seq, n_ptiles, d_codes, d_room, d_offsets,
                     d_bank, d_tile_len, d_mlen, d_thr, d_orig, const_cast<int32_t*>(d_counts), d_base, n_hits, d_seq,
                     d_motif, d_pos, d_score);
  MU_CHECK_LAUNCH();
  return MU_OK;
}

}  // extern "C"
