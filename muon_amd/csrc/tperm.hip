// X^T as a row stream from the row stream of X, TABLE DRIVEN: the per-step fill of lsi's hot path.
//
// csrc/tpack4.hip ranks every tile on every call - a bitmap per (wave, column), a prefix over the waves, a lookup per
// entry - although the staging slot of an entry depends on the index arrays alone.  Here that work is done ONCE per
// matrix (`mu_tperm_plan`, made with the first fill and kept with the transposition plan):
//   * the exact TILE SCHEDULE of every row block: variable-width tiles chosen so that a tile always fits the staging
//     buffer, at most two rows of a wave have more than 32 entries in it and none more than 64 - nothing is ever retried;
//   * per (tile, wave) the (up to two) rows that need a CONTINUATION window;
//   * per stored entry, in the order of X's row stream, its 16-bit STAGING SLOT inside its (row block, tile).
// The per-step kernel `k_tperm_move` only moves data: windows of (column, value) pairs as in tpack4 (circular: pair p of
// the stream lives in lane p % 32 of its row's half) plus the same entries' slots, `stage[slot] = (where, value)` with
// where = cell | column << 16 inside the (row block, tile), ONE barrier per tile (the staging buffer and the run tables
// are double buffered in the LDS the bitmap no longer needs), then the FLAT write-out: the staged pairs lie in (column, cell) order, lane i takes pair i of the tile and finds its run
// through the column the staged word names - no loop over columns, every lane stores.  Same bytes out as `k_t4_fill`
// (which keeps the write-out by column and is the independent reference): same tiles of work per (row block, column),
// runs sorted by (column, cell).
#include <type_traits>
#include <utility>

#include "common.hpp"
#pragma clang diagnostic ignored "-Winline-asm"

namespace {

constexpr int kT = 1024, kNW = 16;  // threads / waves of a workgroup
constexpr int kMaxC = 512;          // widest tile (columns)
constexpr int kCap = 9216;          // staged pairs of ONE of the two staging buffers: 2 x 72 KiB
constexpr int kH0 = 72;             // asm-owned v[72..75]: the header of the tile after the next
constexpr int kW0 = 76;             // asm-owned window slot j: v[kW0 + 2j] column, + 1 value bits (an aligned pair) ...
constexpr int kS0 = 110;            // ... and v[kS0 + j] the same pairs' staging slots
constexpr int kSlotP = 16;          // the continuation window (slot 16 of both)
constexpr int kNone = 0xff;         // "no row" in a continuation word

#define MU_TP_CLOB                                                                                                      \
  "v72", "v73", "v74", "v75", "v76", "v77", "v78", "v79", "v80", "v81", "v82", "v83", "v84", "v85", "v86", "v87", "v88", \
      "v89", "v90", "v91", "v92", "v93", "v94", "v95", "v96", "v97", "v98", "v99", "v100", "v101", "v102", "v103",       \
      "v104", "v105", "v106", "v107", "v108", "v109", "v110", "v111", "v112", "v113", "v114", "v115", "v116", "v117",    \
      "v118", "v119", "v120", "v121", "v122", "v123", "v124", "v125", "v126", "v127"

__device__ __forceinline__ int tp_wave_min(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int t = __shfl_xor(v, off, 64);
    v = t < v ? t : v;
  }
  return v;
}

// ---- plan: tile schedule, continuation rows, staging slots (once per matrix: simple, exact, a thread per row) ----------
// ROWS MUST BE CANONICAL (column indices strictly increasing inside a row, as everywhere in this library: tpack4 assumes
// the same): a tile advances because a row's 33rd next entry lies at least 32 columns on, and one bit per (row, column)
// ranks an entry - duplicate columns would stall the schedule or give two entries one slot.
// REC = false: counts the tiles of every row block (ntile); REC = true: the same schedule again, written down together
// with the slots.  A wave owns the same rw rows as in the fill (lane l < 32 = row l of the wave).
template <bool REC>
__global__ __launch_bounds__(kT) void k_tperm_plan(int64_t n_rows, int64_t n_cols, int Cmax, int rw,
                                                   const int64_t* __restrict__ indptr,
                                                   const int32_t* __restrict__ indices,
                                                   const int64_t* __restrict__ row_dst,
                                                   const int64_t* __restrict__ toff, int32_t* __restrict__ ntile,
                                                   int32_t* __restrict__ tiles, uint32_t* __restrict__ cont,
                                                   uint16_t* __restrict__ slots) {
  __shared__ uint32_t bm[REC ? kNW : 1][kMaxC];  // (wave, column): bitmap of the wave's rows with that column
  __shared__ uint32_t fs[REC ? kNW : 1][kMaxC];  // (wave, column): first staging slot of the wave's entries
  __shared__ uint32_t wsum[kNW];
  __shared__ int s_lim;
  __shared__ unsigned s_tot;
  const int g = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, sub = lane & 31;
  const int64_t rpb = (int64_t)kNW * rw;
  const int64_t r0 = (int64_t)g * rpb;
  const int64_t r1 = (r0 + rpb) < n_rows ? (r0 + rpb) : n_rows;
  const int64_t row = r0 + (int64_t)wave * rw + sub;
  const bool active = lane < 32 && sub < rw && row < r1;
  int64_t cur = active ? indptr[row] : 0;
  const int64_t end = active ? indptr[row + 1] : 0;
  const int64_t dst0 = (REC && active) ? row_dst[row] - cur : 0;  // slot index of CSR position q: dst0 + q
  if (REC)
    for (int t = tid; t < kNW * kMaxC; t += kT) (&bm[0][0])[t] = 0u;
  const int64_t tb = REC ? toff[g] + g : 0, tc = REC ? toff[g] : 0;
  int t = 0;
  for (int64_t cb = 0; cb < n_cols; ++t) {
    if (tid == 0) {
      s_lim = (int)((cb + Cmax) < n_cols ? (cb + Cmax) : n_cols);
      s_tot = 0u;
    }
    __syncthreads();
    // the tile ends before the 33rd entry of the wave's third fullest row and before anybody's 65th
    const int64_t left = end - cur;
    int x = left > 32 ? indices[cur + 32] : 0x7fffffff;
    int lim = tp_wave_min(left > 64 ? indices[cur + 64] : 0x7fffffff);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int m = tp_wave_min(x);
      const unsigned long long b = __ballot(x == m);
      if (lane == (int)__builtin_ctzll(b)) x = 0x7fffffff;
    }
    const int m3 = tp_wave_min(x);
    lim = m3 < lim ? m3 : lim;
    if (lane == 0 && lim != 0x7fffffff) atomicMin(&s_lim, lim);
    __syncthreads();
    int cend = s_lim;
    int n;
    unsigned total;
    for (;;) {
      int lo = 0, hi = (int)(left < 64 ? left : 64);  // entries of this row in the tile: a prefix of its next 64
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (indices[cur + mid] < cend) lo = mid + 1; else hi = mid;
      }
      n = lo;
      const int ws = wave_sum_all(n);
      if (lane == 0 && ws) atomicAdd(&s_tot, (unsigned)ws);
      __syncthreads();
      total = s_tot;
      __syncthreads();
      if (total <= (unsigned)kCap) break;
      // (a block denser than the staging buffer: half the width; 16 columns x 512 rows always fit)
      if (tid == 0) s_tot = 0u;
      int w = ((int)(cend - cb) / 2 / 16) * 16;
      w = w < 16 ? 16 : w;
      cend = (int)cb + w;
      __syncthreads();
    }
    if (REC) {
      if (tid == 0) tiles[tb + t] = (int32_t)cb;
      const unsigned over = (unsigned)__ballot(n > 32);  // (at most two bits, by the choice of the tile's end)
      if (lane == 0) {
        int pa = kNone, pb = kNone;
        if (over) {
          pa = __builtin_ctz(over);
          const unsigned o2 = over & (over - 1u);
          if (o2) pb = __builtin_ctz(o2);
        }
        cont[(tc + t) * kNW + wave] = (uint32_t)(pa | (pb << 8));
      }
      if (total > 0u) {
        const int W = cend - (int)cb;
        for (int k = 0; k < n; ++k) atomicOr(&bm[wave][indices[cur + k] - (int)cb], 1u << sub);
        __syncthreads();
        uint32_t mine = 0;
        if (tid < W)
          for (int w = 0; w < kNW; ++w) mine += (uint32_t)__popc(bm[w][tid]);
        uint32_t incl = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const uint32_t u = __shfl_up(incl, off, 64);
          if (lane >= off) incl += u;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        uint32_t run = incl - mine;
        for (int w = 0; w < wave; ++w) run += wsum[w];
        if (tid < W)
          for (int w = 0; w < kNW; ++w) {
            fs[w][tid] = run;
            run += (uint32_t)__popc(bm[w][tid]);
          }
        __syncthreads();
        for (int k = 0; k < n; ++k) {
          const int c = indices[cur + k] - (int)cb;
          slots[dst0 + cur + k] = (uint16_t)(fs[wave][c] + (uint32_t)__popc(bm[wave][c] & ((1u << sub) - 1u)));
        }
        __syncthreads();
        if (tid < W)
          for (int w = 0; w < kNW; ++w) bm[w][tid] = 0u;
      }
    }
    cur += n;
    cb = cend;
  }
  if (tid == 0) {
    if (REC) tiles[tb + t] = (int32_t)n_cols;
    else ntile[g] = t;
  }
}

// ---- the window registers ------------------------------------------------------------------------------------------
// Circular windows as in tpack4 (t4_issue_circ), with the staging slots of the same pairs: b = address of the 256-byte
// block of the stream the first new pair lies in, tb = address of that block's 32 slots, s = the first new pair's lane,
// m = the lanes to load; a lane before s belongs to the NEXT block.
template <int J>
__device__ __forceinline__ void tp_issue_circ(uint64_t b0, uint64_t b1, uint64_t tb0, uint64_t tb1, unsigned s0, unsigned s1,
                                              unsigned m0, unsigned m1, unsigned sub, unsigned sub8, unsigned sub8w,
                                              unsigned sub2, unsigned sub2w) {
  unsigned long long save;
  unsigned p0, p1, q0, q1;
  asm volatile(
      "s_mov_b64 %[save], exec\n\t"
      "v_cmp_gt_u32 vcc, %[s0], %[sub]\n\t"
      "v_cndmask_b32 %[p0], %[sub8], %[sub8w], vcc\n\t"
      "v_cndmask_b32 %[q0], %[sub2], %[sub2w], vcc\n\t"
      "v_cmp_gt_u32 vcc, %[s1], %[sub]\n\t"
      "v_cndmask_b32 %[p1], %[sub8], %[sub8w], vcc\n\t"
      "v_cndmask_b32 %[q1], %[sub2], %[sub2w], vcc\n\t"
      "s_mov_b32 exec_lo, %[m0]\n\t"
      "s_mov_b32 exec_hi, 0\n\t"
      "global_load_dwordx2 v[%c[C]:%c[V]], %[p0], %[b0]\n\t"
      "global_load_ushort v%c[S], %[q0], %[tb0]\n\t"
      "s_mov_b32 exec_lo, 0\n\t"
      "s_mov_b32 exec_hi, %[m1]\n\t"
      "global_load_dwordx2 v[%c[C]:%c[V]], %[p1], %[b1]\n\t"
      "global_load_ushort v%c[S], %[q1], %[tb1]\n\t"
      "s_mov_b64 exec, %[save]"
      : [save] "=&s"(save), [p0] "=&v"(p0), [p1] "=&v"(p1), [q0] "=&v"(q0), [q1] "=&v"(q1)
      : [sub] "v"(sub), [sub8] "v"(sub8), [sub8w] "v"(sub8w), [sub2] "v"(sub2), [sub2w] "v"(sub2w), [b0] "s"(b0),
        [b1] "s"(b1), [tb0] "s"(tb0), [tb1] "s"(tb1), [s0] "s"(s0), [s1] "s"(s1), [m0] "s"(m0), [m1] "s"(m1),
        [C] "i"(kW0 + 2 * J), [V] "i"(kW0 + 2 * J + 1), [S] "i"(kS0 + J)
      : MU_TP_CLOB, "vcc", "memory");
}
// the continuation window: the 32 pairs behind the circular window of two rows (a0 / a1: their address, t0 / t1: of
// their slots, n0 / n1 in 0 .. 32: how many the row has there), lane = pair
__device__ __forceinline__ void tp_issue_cont(uint64_t a0, uint64_t a1, uint64_t t0, uint64_t t1, int n0, int n1,
                                              unsigned sub8, unsigned sub2) {
  unsigned long long save, m0, m1;
  asm volatile(
      "s_bfm_b64 %[m0], %[n0], 0\n\t"
      "s_bfm_b64 %[m1], %[n1], 32\n\t"
      "s_mov_b64 %[save], exec\n\t"
      "v_mov_b32 v%c[C], 0x7fffffff\n\t"
      "s_mov_b64 exec, %[m0]\n\t"
      "global_load_dwordx2 v[%c[C]:%c[V]], %[o8], %[a0]\n\t"
      "global_load_ushort v%c[S], %[o2], %[t0]\n\t"
      "s_mov_b64 exec, %[m1]\n\t"
      "global_load_dwordx2 v[%c[C]:%c[V]], %[o8], %[a1]\n\t"
      "global_load_ushort v%c[S], %[o2], %[t1]\n\t"
      "s_mov_b64 exec, %[save]"
      : [save] "=&s"(save), [m0] "=&s"(m0), [m1] "=&s"(m1)
      : [o8] "v"(sub8), [o2] "v"(sub2), [a0] "s"(a0), [a1] "s"(a1), [t0] "s"(t0), [t1] "s"(t1), [n0] "s"(n0), [n1] "s"(n1),
        [C] "i"(kW0 + 2 * kSlotP), [V] "i"(kW0 + 2 * kSlotP + 1), [S] "i"(kS0 + kSlotP)
      : MU_TP_CLOB, "memory");
}
template <int J>
__device__ __forceinline__ void tp_pad_slot() {
  asm volatile("v_mov_b32 v%c0, 0x7fffffff" ::"i"(kW0 + 2 * J) : MU_TP_CLOB);
}
// the pairs of slot J that the tile took (column < cend) become padding
template <int J>
__device__ __forceinline__ void tp_retire_slot(int cend, int pad) {
  asm volatile(
      "v_cmp_le_i32 vcc, %0, v%c1\n\t"
      "v_cndmask_b32 v%c1, %2, v%c1, vcc" ::"s"(cend),
      "i"(kW0 + 2 * J), "v"(pad)
      : MU_TP_CLOB, "vcc");
}
__device__ __forceinline__ void tp_wait_all() { asm volatile("s_waitcnt vmcnt(0)" ::: MU_TP_CLOB, "memory"); }
template <int R>
__device__ __forceinline__ unsigned tp_reg() {
  unsigned v;
  asm volatile("v_mov_b32 %0, v%c1" : "=v"(v) : "i"(R) : MU_TP_CLOB);
  return v;
}
// a tile's header (this block's count prefix of its columns, the next block's, where the columns' runs start): three
// loads by every thread, clamped inside the arrays, into v[kH0 .. kH0 + 3]
__device__ __forceinline__ void tp_issue_header(const uint32_t* bg, const uint32_t* bn, const int64_t* cd, unsigned off4) {
  asm volatile(
      "global_load_dword v%c4, %0, %1\n\t"
      "global_load_dword v%c5, %0, %2\n\t"
      "v_lshlrev_b32 v%c6, 1, %0\n\t"
      "global_load_dwordx2 v[%c6:%c7], v%c6, %3"
      :
      : "v"(off4), "s"(bg), "s"(bn), "s"(cd), "i"(kH0), "i"(kH0 + 1), "i"(kH0 + 2), "i"(kH0 + 3)
      : MU_TP_CLOB, "memory");
}

// ---- the per-step fill ---------------------------------------------------------------------------------------------
// Tile t of a block: [top] wait for everything in flight (windows of t, header of t + 1, the write-out's stores) - the
// header of t + 1 is scanned (per-wave sums into wsum) - every entry of t goes to stage[t & 1][slot] - the windows of
// t + 1 and the header of t + 2 are requested - BARRIER - the run table of t + 1 is finished from wsum - write-out of t.
// Everything shared has two sets, indexed by the tile's parity: what tile t + 2 overwrites was last read before the
// barrier of t + 1.
// (amdgpu_num_vgpr counts in the units this hipcc allocates in for a 1024-thread workgroup - TWO registers: 36 keeps the
//  compiler below v72 = kH0, exactly as tpack4's 44 keeps it below v88.  Without it hipcc parks temporaries in the
//  asm-owned registers between two asm statements; tests/test_tperm_isa.py audits the result.)
//
// ACCT = true is the PHASE ACCOUNTING instance (`k_tperm_phases`, mu_tperm_fill_phases): the same tile loop with an
// s_memtime stamp at every phase boundary, summed per wave in scalar registers and written to `acct` at the end.  Every
// stamp sits behind `if constexpr (ACCT)`: the production kernel holds none of it.
constexpr int kPhases = 6;  // top wait, header scan, staging, retire + window issue, barrier, write-out
template <bool ACCT>
__device__ __forceinline__ void tperm_move_body(
    int64_t n_rows, int64_t n_cols, int rw, int G, const int64_t* __restrict__ indptr,
    const int64_t* __restrict__ row_dst, const unsigned long long* __restrict__ xent,
    const int64_t* __restrict__ cdst, const uint32_t* __restrict__ base, const int64_t* __restrict__ toff,
    const int32_t* __restrict__ tiles, const uint32_t* __restrict__ cont, const uint16_t* __restrict__ slots,
    unsigned long long* __restrict__ out, unsigned long long* __restrict__ acct) {
  __shared__ unsigned long long stage[2][kCap];  // 144 KiB
  __shared__ int64_t dcol[2][kMaxC];             // per column of a tile: where its run goes - its first staging slot
  __shared__ __attribute__((aligned(16))) uint32_t wsum[2][kNW];
  int g = blockIdx.x;
  if (G > 0) {  // XCD-aware order (see k_t4_fill)
    const int per = (G + 7) / 8;
    g = (g % 8) * per + (g / 8);
    if (g >= G) return;
  } else {
    G = -G;
  }
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = uniform32(tid >> 6);
  const int half = lane >> 5, sub = lane & 31;
  const int64_t rpb = (int64_t)kNW * rw;
  const int64_t r0 = (int64_t)g * rpb;
  const int64_t r1 = (r0 + rpb) < n_rows ? (r0 + rpb) : n_rows;
  const int64_t wr0 = r0 + (int64_t)wave * rw;

  // lane l < 32: the state of row wr0 + l - address of its next pair and the pairs it has left
  uint64_t A = 0;
  int rem = 0, ld = 0;
  {
    const int64_t row = wr0 + sub;
    const bool ok = sub < rw && row < r1;
    const int64_t p0 = ok ? indptr[row] : 0;
    rem = ok ? (int)(indptr[row + 1] - p0) : 0;
    A = (uint64_t)xent + 8ull * (uint64_t)(ok ? row_dst[row] : 0);
  }
  const int64_t tb = uniform64(toff[g]) + g;              // this block's tile boundaries: tiles[tb .. tb + nt]
  const int nt = (int)(uniform64(toff[g + 1]) - uniform64(toff[g]));
  const uint32_t* cw = cont + (tb - g) * kNW + wave;     // this wave's continuation word of tile t: cw[t * kNW]
  const unsigned subo = (unsigned)sub * 8u, sub2 = (unsigned)sub * 2u;
  static_for<16>([&](auto jc) { tp_pad_slot<decltype(jc)::value>(); });

  // windows of tile `t` (the cursors stand at its first pairs)
  auto cont_of = [&](int t) { return t < nt ? uniform32((int)cw[(int64_t)t * kNW]) : (kNone | (kNone << 8)); };
  auto issue_all = [&](int pw) {
    const int remc = rem < 32 ? rem : 32;
    const int nn = remc - ld;                               // new pairs of the row (>= 0) ...
    const uint64_t st = A + 8ull * (uint64_t)(unsigned)ld;  // ... from this address on
    const unsigned s5 = (unsigned)(st >> 3) & 31u;
    const unsigned rot = __builtin_rotateleft32((unsigned)((1ull << nn) - 1ull), s5);
    const uint64_t b256 = st & ~255ull;
    const uint64_t tb64 = (uint64_t)slots + ((b256 - (uint64_t)xent) >> 2);
    ld = remc;
    static_for<16>([&](auto jc) {
      constexpr int J = decltype(jc)::value;
      tp_issue_circ<J>(readlane_u64(b256, 2 * J), readlane_u64(b256, 2 * J + 1), readlane_u64(tb64, 2 * J),
                       readlane_u64(tb64, 2 * J + 1), (unsigned)__builtin_amdgcn_readlane((int)s5, 2 * J),
                       (unsigned)__builtin_amdgcn_readlane((int)s5, 2 * J + 1),
                       (unsigned)__builtin_amdgcn_readlane((int)rot, 2 * J),
                       (unsigned)__builtin_amdgcn_readlane((int)rot, 2 * J + 1), (unsigned)sub, subo, subo + 256u, sub2,
                       sub2 + 64u);
    });
    const int pa = pw & 0xff, pb = pw >> 8;
    if (pa != kNone) {
      const int lb = pb != kNone ? pb : pa;
      int na = __builtin_amdgcn_readlane(rem, pa) - 32, nb = pb != kNone ? __builtin_amdgcn_readlane(rem, pb) - 32 : 0;
      na = __builtin_amdgcn_readfirstlane(na < 0 ? 0 : (na > 32 ? 32 : na));
      nb = __builtin_amdgcn_readfirstlane(nb < 0 ? 0 : (nb > 32 ? 32 : nb));
      const uint64_t a0 = readlane_u64(A, pa) + 256u, a1 = readlane_u64(A, lb) + 256u;
      tp_issue_cont(a0, a1, (uint64_t)slots + ((a0 - (uint64_t)xent) >> 2), (uint64_t)slots + ((a1 - (uint64_t)xent) >> 2),
                    na, nb, subo, sub2);
    }
  };
  const uint32_t* base_g = base + (int64_t)g * n_cols;
  const uint32_t* base_n = base + (int64_t)(g + 1) * n_cols;
  auto issue_header = [&](int64_t cb) {
    int64_t ofs = n_cols - 1 - cb;
    if (ofs < 0) {
      ofs = 0;
      cb = n_cols - 1;
    }
    const unsigned o4 = (unsigned)((int64_t)tid < ofs ? (int64_t)tid : ofs) * 4u;
    tp_issue_header(base_g + cb, base_n + cb, cdst + cb, o4);
  };
  // the header in v[kH0 ..] belongs to a tile of `W` columns: this thread's column count, where its run goes, and the
  // inclusive scan of the counts over the wave (its total to wsum[set])
  uint32_t mine = 0, incl = 0;
  int64_t gd = 0;
  auto take_header = [&](int W, int set) {
    const uint32_t b0 = tp_reg<kH0>(), b1 = tp_reg<kH0 + 1>();
    const unsigned lo = tp_reg<kH0 + 2>(), hi = tp_reg<kH0 + 3>();
    mine = tid < W ? b1 - b0 : 0u;
    gd = (int64_t)(((unsigned long long)hi << 32) | lo) + (int64_t)b0;
    incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t u = __shfl_up(incl, off, 64);
      if (lane >= off) incl += u;
    }
    if (lane == 63) wsum[set][wave] = incl;
  };
  // (behind a barrier: every wave's sum is there)  The staging buffer holds a tile's pairs in (column, cell) order, a
  // column's first slot is the prefix of the counts: pair i of the tile goes to out[dcol[column] + i].  Returns the
  // tile's pairs.
  auto finish_header = [&](int W, int set) {
    const uint4* ws4 = reinterpret_cast<const uint4*>(wsum[set]);
    uint32_t wpre = 0, total = 0;
#pragma unroll
    for (int q = 0; q < kNW / 4; ++q) {
      const uint4 u4 = ws4[q];
      const uint32_t u[4] = {u4.x, u4.y, u4.z, u4.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        total += u[k];
        wpre += u[k] & (uint32_t)-(int)(4 * q + k < wave);  // (a mask, not a branch per wave)
      }
    }
    if (tid < W) dcol[set][tid] = gd - (int64_t)(wpre + incl - mine);
    return uniform32((int)total);
  };
  // write-out, FLAT: one staged pair per lane whatever column it belongs to, every lane busy up to the tile's last
  // pair; the staged low word names the pair's column and cell inside the tile (see the staging below)
  auto write_out = [&](int set, int total) {
    const unsigned long long* stg = stage[set];
    const int64_t* dc = dcol[set];
    // N whole rounds of the workgroup from pair i on: the reads of all N, then their stores
    auto rounds = [&](auto nc, int i) {
      constexpr int N = decltype(nc)::value;
      unsigned long long e[N];
      int64_t q[N];
#pragma unroll
      for (int u = 0; u < N; ++u) e[u] = stg[i + u * kT];
#pragma unroll
      for (int u = 0; u < N; ++u) q[u] = dc[((unsigned)e[u] >> 16) & (unsigned)(kMaxC - 1)];
#pragma unroll
      for (int u = 0; u < N; ++u)
        out[q[u] + (i + u * kT)] =
            (e[u] & 0xffffffff00000000ull) | (unsigned long long)((unsigned)r0 + ((unsigned)e[u] & 0xffffu));
    };
    const int whole = total / kT;  // (uniform: the rounds in which every thread has a pair)
    int r = 0;
    for (; r + 4 <= whole; r += 4) rounds(std::integral_constant<int, 4>{}, tid + r * kT);
    if ((whole - r) & 2) {
      rounds(std::integral_constant<int, 2>{}, tid + r * kT);
      r += 2;
    }
    if ((whole - r) & 1) {
      rounds(std::integral_constant<int, 1>{}, tid + r * kT);
      r += 1;
    }
    if (tid + r * kT < total) rounds(std::integral_constant<int, 1>{}, tid + r * kT);
  };

  auto tile_at = [&](int t) { return uniform32(tiles[tb + (t < nt ? t : nt)]); };
  int c0 = tile_at(0), c1 = tile_at(1), c2 = tile_at(2);
  issue_header(c0);
  tp_wait_all();
  take_header(c1 - c0, 0);
  int pw = cont_of(0);
  issue_all(pw);
  issue_header(c1);
  __syncthreads();
  int tot = finish_header(c1 - c0, 0);  // pairs of tile t

  // (ACCT) cycles of this wave per phase: a stamp closes the phase named by its index
  unsigned long long ph[kPhases] = {}, t_prev = 0;
  if constexpr (ACCT) t_prev = __builtin_amdgcn_s_memtime();
  auto stamp = [&](auto kc) {
    if constexpr (ACCT) {
      const unsigned long long now = __builtin_amdgcn_s_memtime();
      ph[decltype(kc)::value] += now - t_prev;
      t_prev = now;
    }
  };
  using std::integral_constant;

  for (int t = 0; t < nt; ++t) {
    const int set = t & 1;
    const int cend = c1;
    int hf = half;
    asm volatile("" : "+v"(hf));  // (per-slot constants made from `half` are recomputed, not kept in registers)
    const int pw_next = cont_of(t + 1);
    tp_wait_all();
    stamp(integral_constant<int, 0>{});
    take_header(c2 - c1, set ^ 1);
    stamp(integral_constant<int, 1>{});
    // every entry of the tile to its slot, straight from the window registers.  The staged low word is
    // cell_local | col_local << 16: the row inside the block (wave * rw + row of the wave, <= 511) and the column
    // inside the tile (c - c0, <= 511) - what the flat write-out needs to find the pair's run and to rebuild its cell.
    // (c << 16 wraps; the difference to c0 << 16 does not)
    unsigned long long* stg = stage[set];
    const unsigned wbase = (unsigned)(wave * rw) - ((unsigned)c0 << 16);
    int cntv = 0;  // lane r < 32: pairs of row r consumed by this tile
    static_for<16>([&](auto jc) {
      constexpr int J = decltype(jc)::value;
      const int c = (int)tp_reg<kW0 + 2 * J>();
      const unsigned v = tp_reg<kW0 + 2 * J + 1>(), s = tp_reg<kS0 + J>();
      const bool valid = c < cend;  // sorted rows: a run of each half; padding lanes hold INT_MAX
      const unsigned long long m = __ballot(valid);
      if (valid) stg[s] = (unsigned long long)(((unsigned)c << 16) + (wbase + 2 * J + hf)) | ((unsigned long long)v << 32);
      cntv = writelane_c<2 * J>(cntv, __popc((unsigned)m));
      cntv = writelane_c<2 * J + 1>(cntv, __popc((unsigned)(m >> 32)));
    });
    const int pa = pw & 0xff, pb = pw >> 8;
    if (pa != kNone) {  // the rows the plan gave a continuation window
      const int lb = pb != kNone ? pb : pa;
      const int c = (int)tp_reg<kW0 + 2 * kSlotP>();
      const unsigned v = tp_reg<kW0 + 2 * kSlotP + 1>(), s = tp_reg<kS0 + kSlotP>();
      const bool valid = c < cend;
      const unsigned long long m = __ballot(valid);
      if (valid) stg[s] = (unsigned long long)(((unsigned)c << 16) + (wbase + (hf ? lb : pa))) | ((unsigned long long)v << 32);
      cntv = writelane_s(cntv, __builtin_amdgcn_readlane(cntv, pa) + __popc((unsigned)m), pa);
      if (pb != kNone) cntv = writelane_s(cntv, __builtin_amdgcn_readlane(cntv, pb) + __popc((unsigned)(m >> 32)), pb);
    }
    stamp(integral_constant<int, 2>{});
    // the cursors move on, the consumed lanes are free, the next windows are requested
    {
      int padv = 0x7fffffff;
      asm volatile("" : "+v"(padv));
      static_for<16>([&](auto jc) { tp_retire_slot<decltype(jc)::value>(cend, padv); });
    }
    if (half == 0) {
      A += (uint64_t)(unsigned)cntv * 8u;
      rem -= cntv;
      ld = ld > cntv ? ld - cntv : 0;  // (a row that went into its continuation has nothing left in the window)
    }
    pw = pw_next;
    issue_all(pw);
    issue_header(c2);
    const int c3 = tile_at(t + 3);
    stamp(integral_constant<int, 3>{});
    __syncthreads();
    stamp(integral_constant<int, 4>{});
    const int tot_next = finish_header(c2 - c1, set ^ 1);
    write_out(set, tot);
    tot = tot_next;
    stamp(integral_constant<int, 5>{});
    c0 = c1;
    c1 = c2;
    c2 = c3;
  }
  tp_wait_all();  // (windows and a header requested for a tile that does not exist)
  if constexpr (ACCT) {
    // row (block, wave) of acct: the six phase sums, the block's tiles, 0
    if (lane == 0) {
      unsigned long long* row = acct + ((int64_t)g * kNW + wave) * (kPhases + 2);
#pragma unroll
      for (int k = 0; k < kPhases; ++k) row[k] = ph[k];
      row[kPhases] = (unsigned long long)nt;
      row[kPhases + 1] = 0ull;
    }
  }
}

__global__ __launch_bounds__(kT) __attribute__((amdgpu_num_vgpr(36))) void k_tperm_move(
    int64_t n_rows, int64_t n_cols, int rw, int G, const int64_t* __restrict__ indptr,
    const int64_t* __restrict__ row_dst, const unsigned long long* __restrict__ xent,
    const int64_t* __restrict__ cdst, const uint32_t* __restrict__ base, const int64_t* __restrict__ toff,
    const int32_t* __restrict__ tiles, const uint32_t* __restrict__ cont, const uint16_t* __restrict__ slots,
    unsigned long long* __restrict__ out) {
  tperm_move_body<false>(n_rows, n_cols, rw, G, indptr, row_dst, xent, cdst, base, toff, tiles, cont, slots, out, nullptr);
}
__global__ __launch_bounds__(kT) __attribute__((amdgpu_num_vgpr(36))) void k_tperm_phases(
    int64_t n_rows, int64_t n_cols, int rw, int G, const int64_t* __restrict__ indptr,
    const int64_t* __restrict__ row_dst, const unsigned long long* __restrict__ xent,
    const int64_t* __restrict__ cdst, const uint32_t* __restrict__ base, const int64_t* __restrict__ toff,
    const int32_t* __restrict__ tiles, const uint32_t* __restrict__ cont, const uint16_t* __restrict__ slots,
    unsigned long long* __restrict__ out, unsigned long long* __restrict__ acct) {
  tperm_move_body<true>(n_rows, n_cols, rw, G, indptr, row_dst, xent, cdst, base, toff, tiles, cont, slots, out, acct);
}

}  // namespace

extern "C" {

int mu_tperm_stage_pairs(void) { return kCap; }

int mu_tperm_plan(int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t* d_indptr, const int32_t* d_indices,
                  const int64_t* d_x_row_dst, int tile_cols, const int64_t* d_tile_off, int32_t* d_ntile,
                  int32_t* d_tiles, uint32_t* d_cont, uint16_t* d_slots, void* stream) {
  MU_REQUIRE(mu_tpack4_supported(n_rows, n_cols, nnz), "shape out of range (mu_tpack4_supported)");
  MU_REQUIRE(d_indptr && d_indices, "null pointer");
  MU_REQUIRE(tile_cols >= 16 && tile_cols <= kMaxC, "tile_cols out of range (16 .. 512)");
  MU_REQUIRE(d_tile_off ? (d_x_row_dst && d_tiles && d_cont && d_slots) : d_ntile != nullptr,
             "count pass: d_ntile; record pass: d_x_row_dst, d_tile_off, d_tiles, d_cont, d_slots");
  int64_t rpb = 0;
  int G = 0;
  mu_tpack4_geometry(n_rows, n_cols, nnz, &rpb, &G, nullptr);
  const int rw = (int)(rpb / kNW);
  hipStream_t st = (hipStream_t)stream;
  if (d_tile_off)
    hipLaunchKernelGGL((k_tperm_plan<true>), dim3(G), dim3(kT), 0, st, n_rows, n_cols, tile_cols, rw, d_indptr, d_indices,
                       d_x_row_dst, d_tile_off, d_ntile, d_tiles, d_cont, d_slots);
  else
    hipLaunchKernelGGL((k_tperm_plan<false>), dim3(G), dim3(kT), 0, st, n_rows, n_cols, tile_cols, rw, d_indptr,
                       d_indices, d_x_row_dst, d_tile_off, d_ntile, d_tiles, d_cont, d_slots);
  MU_CHECK_LAUNCH();
  return MU_OK;
}

// d_phases = nullptr: the production kernel; given: the accounting instance
static int tperm_fill(int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t* d_indptr, const int64_t* d_x_row_dst,
                      const void* d_x_ent, const int64_t* d_cdst, const void* d_cnt, const int64_t* d_tile_off,
                      const int32_t* d_tiles, const uint32_t* d_cont, const uint16_t* d_slots, void* d_ent,
                      unsigned long long* d_phases, void* stream) {
  MU_REQUIRE(mu_tpack4_supported(n_rows, n_cols, nnz), "shape out of range (mu_tpack4_supported)");
  MU_REQUIRE(d_indptr && d_x_row_dst && d_x_ent && d_cdst && d_cnt && d_tile_off && d_tiles && d_cont && d_slots && d_ent,
             "null pointer");
  MU_REQUIRE((reinterpret_cast<uintptr_t>(d_x_ent) & 255) == 0, "the row stream of X must be 256-byte aligned");
  int64_t rpb = 0;
  int G = 0;
  mu_tpack4_geometry(n_rows, n_cols, nnz, &rpb, &G, nullptr);
  const int rw = (int)(rpb / kNW);
  const bool xcd = tune(kTune_tpack4_plain) != 1;
  const unsigned grid = xcd ? (unsigned)(8 * ((G + 7) / 8)) : (unsigned)G;
  if (d_phases)
    hipLaunchKernelGGL(k_tperm_phases, dim3(grid), dim3(kT), 0, (hipStream_t)stream, n_rows, n_cols, rw, xcd ? G : -G,
                       d_indptr, d_x_row_dst, (const unsigned long long*)d_x_ent, d_cdst, (const uint32_t*)d_cnt,
                       d_tile_off, d_tiles, d_cont, d_slots, (unsigned long long*)d_ent, d_phases);
  else
    hipLaunchKernelGGL(k_tperm_move, dim3(grid), dim3(kT), 0, (hipStream_t)stream, n_rows, n_cols, rw, xcd ? G : -G,
                       d_indptr, d_x_row_dst, (const unsigned long long*)d_x_ent, d_cdst, (const uint32_t*)d_cnt,
                       d_tile_off, d_tiles, d_cont, d_slots, (unsigned long long*)d_ent);
  MU_CHECK_LAUNCH();
  return MU_OK;
}

int mu_tperm_fill(int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t* d_indptr, const int64_t* d_x_row_dst,
                  const void* d_x_ent, const int64_t* d_cdst, const void* d_cnt, const int64_t* d_tile_off,
                  const int32_t* d_tiles, const uint32_t* d_cont, const uint16_t* d_slots, void* d_ent, void* stream) {
  return tperm_fill(n_rows, n_cols, nnz, d_indptr, d_x_row_dst, d_x_ent, d_cdst, d_cnt, d_tile_off, d_tiles, d_cont,
                    d_slots, d_ent, nullptr, stream);
}

int mu_tperm_fill_phases(int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t* d_indptr,
                         const int64_t* d_x_row_dst, const void* d_x_ent, const int64_t* d_cdst, const void* d_cnt,
                         const int64_t* d_tile_off, const int32_t* d_tiles, const uint32_t* d_cont,
                         const uint16_t* d_slots, void* d_ent, unsigned long long* d_phases, void* stream) {
  MU_REQUIRE(d_phases, "null pointer");
  return tperm_fill(n_rows, n_cols, nnz, d_indptr, d_x_row_dst, d_x_ent, d_cdst, d_cnt, d_tile_off, d_tiles, d_cont,
                    d_slots, d_ent, d_phases, stream);
}

}  // extern "C"
