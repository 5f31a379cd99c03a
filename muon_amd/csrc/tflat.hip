// X^T as a row stream from the row stream of X, table driven, with a FLAT READ-IN: a sibling of
// csrc/tperm.hip, which stays as the fallback and as the reference.
//
// `k_tperm_move` reads a tile through 17 window slots per wave - a window of 32 pairs per row under a half-wave EXEC mask -
// because it finds out from the data how many pairs of a row fall into the tile.  That number depends on the index arrays
// alone, so here the PLAN (`k_tflat_plan`, once per matrix) writes it down: counts[tile][wave][row of the wave], 16 bits
// each.  The per-step kernel `k_tflat_move` then reads a tile as the write-out writes it: lanes 0 .. 31 of a wave hold
// their row's cursor and its count, a scan gives the prefixes P_r and the wave's total T, and in round u lane l takes
// the wave's pair i = 64 u + l < T - the pair i - P_r of row r, r the last row with P_r <= i (five steps through a
// 32-word table in the LDS) - with ONE full-wave load of the pair and one of its staging slot.  The slots lie in that
// read order: a wave's rows are consecutive CSR rows, the CSR range of its entries holds its slots tile after tile, and
// slot i of a tile is pair i's - a round's slot load is 64 consecutive 16-bit words from a wave-uniform pointer, it
// needs no row search, and no line of the table is read in two tiles.  Everything else is
// `k_tperm_move`'s: the row blocks, the tile schedule array, the two staging buffers, dcol / wsum, the header a tile ahead,
// one barrier per tile, the flat write-out, the same bytes out.
//
// The tile rule is this kernel's own (the per-row limits of the windows are gone): a tile ends at the widest column
// bound (<= tile_cols) at which every wave's total is <= 64 kR and the block's total fits a staging buffer; otherwise the
// width is halved.  16 columns x 32 rows = 512 <= 64 kR pairs per wave always pass.  tests/test_tflat_plan_host.py restates
// the rule in numpy.
#include <type_traits>
#include <utility>

#include "common.hpp"

namespace {

constexpr int kT = 1024, kNW = 16;  // threads / waves of a workgroup
constexpr int kRows = 32;           // rows of a wave (lanes 0 .. 31 hold their state)
constexpr int kMaxC = 512;          // widest tile (columns)
constexpr int kCap = 9216;          // staged pairs of ONE of the two staging buffers: 2 x 72 KiB
constexpr int kR = 12;              // rounds of 64 pairs a wave can read per tile (>= 8: the 16-column tile)
constexpr int kWaveCap = 64 * kR;
constexpr int kGrp = 4;             // rounds whose row searches run side by side
static_assert(kR % kGrp == 0, "whole groups of rounds");
static_assert(kR >= 8&& 16 * kRows <= kWaveCap && 16 * kNW * kRows <= kCap, "the 16-column tile must be admissible");

// ---- plan: tile schedule, counts per (tile, row), staging slots (once per matrix: simple, exact, a thread per row) -----
// ROWS MUST BE CANONICAL (column indices strictly increasing inside a row, as for csrc/tperm.hip): a row then has at
// most one pair per column of a tile, <= kMaxC.  A row that breaks this is caught here - err[0] <- 1 - and the caller
// drops the plan; the step kernel checks nothing.
// REC = false: counts the tiles of every row block (ntile); REC = true: the same schedule again, written down together
// with the counts and the slots.  A wave owns the same rw rows as in the fill (lane l < 32 = row l of the wave).
// A slot's VALUE is the pair's place in the staging buffer, the tile's pairs in (column, cell) order; its PLACE in
// `slots` is indptr[first row of the wave] + the wave's pairs in the block's earlier tiles + P_r + k for the k-th pair
// of row r in the tile (tests/test_tflat_slots_host.py restates both in numpy and fills with them).
template <bool REC>
__global__ __launch_bounds__(kT) void k_tflat_plan(int64_t n_rows, int64_t n_cols, int Cmax, int rw,
                                                   const int64_t* __restrict__ indptr,
                                                   const int32_t* __restrict__ indices,
                                                   const int64_t* __restrict__ toff, int32_t* __restrict__ ntile,
                                                   int32_t* __restrict__ tiles, uint16_t* __restrict__ counts,
                                                   uint16_t* __restrict__ slots, int* __restrict__ err) {
  __shared__ uint32_t bm[REC ? kNW : 1][kMaxC];  // (wave, column): bitmap of the wave's rows with that column
  __shared__ uint32_t fs[REC ? kNW : 1][kMaxC];  // (wave, column): first staging slot of the wave's entries
  __shared__ uint32_t wsum[kNW];
  __shared__ unsigned s_tot, s_wmax;
  const int g = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, sub = lane & 31;
  const int64_t rpb = (int64_t)kNW * rw;
  const int64_t r0 = (int64_t)g * rpb;
  const int64_t r1 = (r0 + rpb) < n_rows ? (r0 + rpb) : n_rows;
  const int64_t row = r0 + (int64_t)wave * rw + sub;
  const bool active = lane < 32 && sub < rw && row < r1;
  int64_t cur = active ? indptr[row] : 0;
  const int64_t end = active ? indptr[row + 1] : 0;
  // where the wave's slots of the next tile start: its rows are consecutive CSR rows, so its entries are one CSR range,
  // and the slots lie in it tile after tile in the order the fill's lanes read them (a wave without rows never has one)
  const int64_t wrow = r0 + (int64_t)wave * rw;
  int64_t sl = REC ? indptr[wrow < r1 ? wrow : r1] : 0;
  if (REC)
    for (int t = tid; t < kNW * kMaxC; t += kT) (&bm[0][0])[t] = 0u;
  const int64_t tb = REC ? toff[g] + g : 0, tc = REC ? toff[g] : 0;
  int t = 0;
  for (int64_t cb = 0; cb < n_cols; ++t) {
    int cend = (int)((cb + Cmax) < n_cols ? (cb + Cmax) : n_cols);
    if (tid == 0) s_tot = s_wmax = 0u;
    __syncthreads();
    const int64_t left = end - cur;
    int n;
    unsigned total;
    for (;;) {
      // entries of this row in the tile: a prefix of its next kMaxC + 1 (one more than a canonical row can have)
      int lo = 0, hi = (int)(left < kMaxC + 1 ? left : kMaxC + 1);
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (indices[cur + mid] < cend) lo = mid + 1; else hi = mid;
      }
      n = lo;
      const int ws = wave_sum_all(n);
      if (lane == 0 && ws) {
        atomicAdd(&s_tot, (unsigned)ws);
        atomicMax(&s_wmax, (unsigned)ws);
      }
      __syncthreads();
      total = s_tot;
      const unsigned wmax = s_wmax;
      __syncthreads();
      if (total <= (unsigned)kCap && wmax <= (unsigned)kWaveCap) break;
      // (a wave or the block has more than it can take: half the width; 16 columns always fit)
      if (cend - (int)cb <= 16) {  // ... unless a row has a column twice
        if (tid == 0) atomicOr(err, 1);
        break;
      }
      if (tid == 0) s_tot = s_wmax = 0u;
      int w = ((int)(cend - cb) / 2 / 16) * 16;
      w = w < 16 ? 16 : w;
      cend = (int)cb + w;
      __syncthreads();
    }
    if (n > cend - (int)cb) {  // (the range check of the 16-bit counts and of the slots: a canonical row passes)
      atomicOr(err, 1);
      n = cend - (int)cb;
    }
    if (REC) {
      if (tid == 0) tiles[tb + t] = (int32_t)cb;
      if (lane < 32) counts[((tc + t) * kNW + wave) * kRows + sub] = (uint16_t)n;
      // the wave's pair P_r + k of the tile is the k-th of row r's: the prefix the fill's `prepare` makes of the counts
      int pin = n;  // (a lane >= 32 has no row and no count)
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_up(pin, off, 64);
        if (lane >= off) pin += v;
      }
      const int64_t sl_r = sl + (pin - n);
      sl += __builtin_amdgcn_readlane(pin, 63);
      if (total > 0u && total <= (unsigned)kCap) {
        const int W = cend - (int)cb;
        for (int k = 0; k < n; ++k) {
          const int c = indices[cur + k] - (int)cb;
          if (c >= 0 && c < W) atomicOr(&bm[wave][c], 1u << sub);
        }
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
          if (c >= 0 && c < W)
            slots[sl_r + k] = (uint16_t)(fs[wave][c] + (uint32_t)__popc(bm[wave][c] & ((1u << sub) - 1u)));
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

// ---- the per-step fill ---------------------------------------------------------------------------------------------
// Tile t of a block: [top] wait for everything in flight (pairs and slots of t, header of t + 1, counts of t + 2, the
// write-out's stores) - a group of kGrp rounds at a time: the pairs of t in those registers go to stage[t & 1][slot],
// then the same rounds of t + 1 are requested (row search, full-wave loads of pairs and of slots: the first loads leave
// after kGrp rounds of staging, not after the whole tile's) - the header of t + 1 is scanned (per-wave sums into wsum),
// the header of t + 2 and the counts of t + 3 are requested - BARRIER - the run table of t + 1 is finished from wsum -
// write-out of t - the search table of t + 2 is made from its counts (a scan over the wave's 32 rows), while the stores
// drain and the loads fly: between the wait and the first load there is nothing but kGrp rounds of staging and a search.
// Everything shared by the workgroup has two sets, indexed by the tile's parity; the search table is a wave's own and is
// written only behind the wave's last read of the one before.
//
// ACCT = true is the PHASE ACCOUNTING instance (`k_tflat_phases`, mu_tflat_fill_phases): the same six phases as
// `k_tperm_phases`, an s_memtime stamp at every boundary, every stamp behind `if constexpr (ACCT)`.
constexpr int kPhases = 6;  // top wait, header scan, staging, scan + search + issue, barrier, write-out
template <bool ACCT>
__device__ __forceinline__ void tflat_move_body(
    int64_t n_rows, int64_t n_cols, int rw, int G, const int64_t* __restrict__ indptr,
    const int64_t* __restrict__ row_dst, const unsigned long long* __restrict__ xent,
    const int64_t* __restrict__ cdst, const uint32_t* __restrict__ base, const int64_t* __restrict__ toff,
    const int32_t* __restrict__ tiles, const uint16_t* __restrict__ counts, const uint16_t* __restrict__ slots,
    unsigned long long* __restrict__ out, unsigned long long* __restrict__ acct) {
  __shared__ unsigned long long stage[2][kCap];  // 144 KiB
  __shared__ int64_t dcol[2][kMaxC];             // per column of a tile: where its run goes - its first staging slot
  __shared__ __attribute__((aligned(16))) uint32_t wsum[2][kNW];
  __shared__ int64_t rbase[kNW][kRows];  // per wave and row: stream index of the row's next pair - its prefix
  __shared__ uint32_t rpre[kNW][kRows];  // per wave and row: pairs of the wave's rows before it in the tile
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
  const int sub = lane & 31;
  const int64_t rpb = (int64_t)kNW * rw;
  const int64_t r0 = (int64_t)g * rpb;
  const int64_t r1 = (r0 + rpb) < n_rows ? (r0 + rpb) : n_rows;
  const int64_t wr0 = r0 + (int64_t)wave * rw;

  // lane l < 32: stream index of the next pair of row wr0 + l (a lane without a row never has a count)
  int64_t pos = 0;
  {
    const int64_t row = wr0 + sub;
    const bool ok = lane < 32 && sub < rw && row < r1;
    pos = ok ? row_dst[row] : 0;
  }
  const int64_t tc = uniform64(toff[g]);
  const int64_t tb = tc + g;  // this block's tile boundaries: tiles[tb .. tb + nt]
  const int nt = (int)(uniform64(toff[g + 1]) - tc);
  const uint16_t* cnt_w = counts + (tc * kNW + wave) * kRows + sub;  // this lane's count of tile t: cnt_w[t * 512]
  // the slots of the wave's pairs of the next tile to request, in the order its lanes take them: wave-uniform, moved on
  // by the wave's total with every tile (the plan laid them out so, inside the CSR range of the wave's rows)
  const uint16_t* sl_w = slots + uniform64(indptr[wr0 < r1 ? wr0 : r1]);

  // the pairs of a tile in flight: round u, lane l = pair 64 u + l of the wave
  unsigned long long e[kR];  // (column, value bits)
  uint16_t s[kR];            // staging slot (16 bits as loaded: widened where it is used, behind the wait)
  unsigned rr[kR];           // row of the wave
#pragma unroll
  for (int u = 0; u < kR; ++u) e[u] = 0ull, s[u] = 0, rr[u] = 0u;

  // the search table of the tile the cursors stand at; `n`: this lane's count of it.  Returns the wave's total.
  auto prepare = [&](int n) {
    int incl = lane < 32 ? n : 0;
#pragma unroll
    for (int off = 1; off < 32; off <<= 1) {
      const int v = __shfl_up(incl, off, 64);
      if (sub >= off) incl += v;
    }
    const int T = __builtin_amdgcn_readlane(incl, 31);
    if (T > 0) {
      if (lane < 32) {
        const int excl = incl - n;
        rpre[wave][sub] = (unsigned)excl;
        rbase[wave][sub] = pos - excl;
      }
      wave_lds_sync();
    }
    return T;
  };
  // requests the `T` pairs of that tile and moves the cursors on (`n` as above).  `before_group(u0)` runs before the
  // rounds u0 .. u0 + kGrp - 1 are requested: the caller stages the pairs those registers still hold, so the first
  // loads leave before the whole tile is staged.
  auto issue_all = [&](int T, int n, auto&& before_group) {
    const uint32_t* pre = rpre[wave];
    const int64_t* bas = rbase[wave];
    // (rounds in groups of kGrp: the searches of a group are independent chains of LDS reads, walked side by side)
    static_for<kR / kGrp>([&](auto gc) {
      constexpr int u0 = decltype(gc)::value * kGrp;
      before_group(gc);
      if (64 * u0 < T) {  // (wave-uniform, as every guard here)
        unsigned i[kGrp], r[kGrp];
        int64_t p[kGrp];
#pragma unroll
        for (int k = 0; k < kGrp; ++k) {
          i[k] = (unsigned)(64 * (u0 + k) + lane);
          i[k] = i[k] < (unsigned)T ? i[k] : (unsigned)T - 1u;  // (idle lanes repeat the wave's last pair)
          r[k] = 0;
        }
        // (the slots do not wait for the search: a scalar base and the lane's pair number as a 32-bit byte offset, one or
        //  two lines a round)
#pragma unroll
        for (int k = 0; k < kGrp; ++k)
          if (64 * (u0 + k) < T)
            s[u0 + k] = *reinterpret_cast<const uint16_t*>(reinterpret_cast<const char*>(sl_w) + 2u * i[k]);
#pragma unroll
        for (int st = 16; st > 0; st >>= 1)
#pragma unroll
          for (int k = 0; k < kGrp; ++k) r[k] += pre[r[k] + st] <= i[k] ? (unsigned)st : 0u;
#pragma unroll
        for (int k = 0; k < kGrp; ++k) p[k] = bas[r[k]] + (int64_t)i[k];
#pragma unroll
        for (int k = 0; k < kGrp; ++k)
          if (64 * (u0 + k) < T) {
            e[u0 + k] = xent[p[k]];
            rr[u0 + k] = r[k];
          }
      }
    });
    wave_lds_sync();
    pos += n;
    sl_w += T;
  };
  auto count_of = [&](int t) { return (t < nt && lane < 32) ? (int)cnt_w[(int64_t)t * (kNW * kRows)] : 0; };

  const uint32_t* base_g = base + (int64_t)g * n_cols;
  const uint32_t* base_n = base + (int64_t)(g + 1) * n_cols;
  // a tile's header (this block's count prefix of its columns, the next block's, where the columns' runs start): three
  // loads by every thread, clamped inside the arrays
  uint32_t hb0 = 0, hb1 = 0;
  int64_t hcd = 0;
  auto issue_header = [&](int64_t cb) {
    int64_t ofs = n_cols - 1 - cb;
    if (ofs < 0) {
      ofs = 0;
      cb = n_cols - 1;
    }
    const int64_t o = (int64_t)tid < ofs ? (int64_t)tid : ofs;
    hb0 = base_g[cb + o];
    hb1 = base_n[cb + o];
    hcd = cdst[cb + o];
  };
  // the loaded header belongs to a tile of `W` columns: this thread's column count, where its run goes, and the
  // inclusive scan of the counts over the wave (its total to wsum[set])
  uint32_t mine = 0, incl = 0;
  int64_t gd = 0;
  auto take_header = [&](int W, int set) {
    mine = tid < W ? hb1 - hb0 : 0u;
    gd = hcd + (int64_t)hb0;
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
  // write-out, FLAT: one staged pair per lane whatever column it belongs to (see k_tperm_move)
  auto write_out = [&](int set, int total) {
    const unsigned long long* stg = stage[set];
    const int64_t* dc = dcol[set];
    auto rounds = [&](auto nc, int i) {
      constexpr int N = decltype(nc)::value;
      unsigned long long w[N];
      int64_t q[N];
#pragma unroll
      for (int u = 0; u < N; ++u) w[u] = stg[i + u * kT];
#pragma unroll
      for (int u = 0; u < N; ++u) q[u] = dc[((unsigned)w[u] >> 16) & (unsigned)(kMaxC - 1)];
#pragma unroll
      for (int u = 0; u < N; ++u)
        out[q[u] + (i + u * kT)] =
            (w[u] & 0xffffffff00000000ull) | (unsigned long long)((unsigned)r0 + ((unsigned)w[u] & 0xffffu));
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
  auto wait_all = [] { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };

  auto tile_at = [&](int t) { return uniform32(tiles[tb + (t < nt ? t : nt)]); };
  int c0 = tile_at(0), c1 = tile_at(1), c2 = tile_at(2);
  issue_header(c0);
  int cn = count_of(0);
  take_header(c1 - c0, 0);
  int Tw = prepare(cn);  // pairs of this wave in tile t
  issue_all(Tw, cn, [](auto) {});
  issue_header(c1);
  // the counts run two tiles ahead, so that a tile's search table is made at the END of the tile before it - behind the
  // write-out, while its stores drain and the loads are in flight - not between the wait and the first load
  int cnext = count_of(1);      // counts of tile t + 1 ...
  int Tnext = prepare(cnext);   // ... and its search table
  cn = count_of(2);             // counts of t + 2: in flight
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
    wait_all();
    const int cnext2 = cn;  // (counts of t + 2, here: the register is loaded again below)
    stamp(integral_constant<int, 0>{});
    // every pair of the tile to its slot, a group of rounds at a time, each group's registers refilled at once with the
    // next tile's pairs (the cursors move on).  The staged low word is cell_local | col_local << 16: the row inside the
    // block (wave * rw + row of the wave, <= 511) and the column inside the tile (c - c0, <= 511) - what the flat
    // write-out needs to find the pair's run and to rebuild its cell.  (c << 16 wraps; the difference to c0 << 16 does not)
    unsigned long long* stg = stage[set];
    const unsigned wbase = (unsigned)(wave * rw) - ((unsigned)c0 << 16);
    const int Tcur = Tw;
    issue_all(Tnext, cnext, [&](auto gc) {
      stamp(integral_constant<int, 3>{});
#pragma unroll
      for (int k = 0; k < kGrp; ++k) {
        constexpr int u0 = decltype(gc)::value * kGrp;
        const int u = u0 + k;
        if (64 * u < Tcur) {  // (wave-uniform)
          if (64 * u + lane < Tcur)
            stg[s[u]] = (unsigned long long)(((unsigned)e[u] << 16) + (wbase + rr[u])) | (e[u] & 0xffffffff00000000ull);
        }
      }
      stamp(integral_constant<int, 2>{});
    });
    stamp(integral_constant<int, 3>{});
    // the header of t + 1 is scanned (needed behind the barrier only), then the header and the counts of t + 2 requested
    take_header(c2 - c1, set ^ 1);
    stamp(integral_constant<int, 1>{});
    Tw = Tnext;
    issue_header(c2);
    cn = count_of(t + 3);
    const int c3 = tile_at(t + 3);
    stamp(integral_constant<int, 3>{});
    __syncthreads();
    stamp(integral_constant<int, 4>{});
    const int tot_next = finish_header(c2 - c1, set ^ 1);
    write_out(set, tot);
    tot = tot_next;
    stamp(integral_constant<int, 5>{});
    cnext = cnext2;
    Tnext = prepare(cnext);  // (the cursors stand behind t + 1: the table of t + 2)
    stamp(integral_constant<int, 3>{});
    c0 = c1;
    c1 = c2;
    c2 = c3;
  }
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

__global__ __launch_bounds__(kT) void k_tflat_move(
    int64_t n_rows, int64_t n_cols, int rw, int G, const int64_t* __restrict__ indptr,
    const int64_t* __restrict__ row_dst, const unsigned long long* __restrict__ xent,
    const int64_t* __restrict__ cdst, const uint32_t* __restrict__ base, const int64_t* __restrict__ toff,
    const int32_t* __restrict__ tiles, const uint16_t* __restrict__ counts, const uint16_t* __restrict__ slots,
    unsigned long long* __restrict__ out) {
  tflat_move_body<false>(n_rows, n_cols, rw, G, indptr, row_dst, xent, cdst, base, toff, tiles, counts, slots, out, nullptr);
}
__global__ __launch_bounds__(kT) void k_tflat_phases(
    int64_t n_rows, int64_t n_cols, int rw, int G, const int64_t* __restrict__ indptr,
    const int64_t* __restrict__ row_dst, const unsigned long long* __restrict__ xent,
    const int64_t* __restrict__ cdst, const uint32_t* __restrict__ base, const int64_t* __restrict__ toff,
    const int32_t* __restrict__ tiles, const uint16_t* __restrict__ counts, const uint16_t* __restrict__ slots,
    unsigned long long* __restrict__ out, unsigned long long* __restrict__ acct) {
  tflat_move_body<true>(n_rows, n_cols, rw, G, indptr, row_dst, xent, cdst, base, toff, tiles, counts, slots, out, acct);
}

}  // namespace

extern "C" {

int mu_tflat_rounds(void) { return kR; }

int mu_tflat_plan(int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t* d_indptr, const int32_t* d_indices,
                  const int64_t* d_x_row_dst, int tile_cols, const int64_t* d_tile_off, int32_t* d_ntile,
                  int32_t* d_tiles, uint16_t* d_counts, uint16_t* d_slots, int* d_err, void* stream) {
  MU_REQUIRE(mu_tpack4_supported(n_rows, n_cols, nnz), "shape out of range (mu_tpack4_supported)");
  MU_REQUIRE(d_indptr && d_indices && d_err, "null pointer");
  MU_REQUIRE(tile_cols >= 16 && tile_cols <= kMaxC, "tile_cols out of range (16 .. 512)");
  MU_REQUIRE(d_tile_off ? (d_tiles && d_counts && d_slots) : d_ntile != nullptr,
             "count pass: d_ntile; record pass: d_tile_off, d_tiles, d_counts, d_slots");
  (void)d_x_row_dst;  // (the slots lie in the waves' CSR ranges: no pass reads the stream's layout)
  int64_t rpb = 0;
  int G = 0;
  mu_tpack4_geometry(n_rows, n_cols, nnz, &rpb, &G, nullptr);
  const int rw = (int)(rpb / kNW);
  hipStream_t st = (hipStream_t)stream;
  if (d_tile_off)
    hipLaunchKernelGGL((k_tflat_plan<true>), dim3(G), dim3(kT), 0, st, n_rows, n_cols, tile_cols, rw, d_indptr, d_indices,
                       d_tile_off, d_ntile, d_tiles, d_counts, d_slots, d_err);
  else
    hipLaunchKernelGGL((k_tflat_plan<false>), dim3(G), dim3(kT), 0, st, n_rows, n_cols, tile_cols, rw, d_indptr,
                       d_indices, d_tile_off, d_ntile, d_tiles, d_counts, d_slots, d_err);
  MU_CHECK_LAUNCH();
  return MU_OK;
}

// d_phases = nullptr: the production kernel; given: the accounting instance
static int tflat_fill(int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t* d_indptr, const int64_t* d_x_row_dst,
                      const void* d_x_ent, const int64_t* d_cdst, const void* d_cnt, const int64_t* d_tile_off,
                      const int32_t* d_tiles, const uint16_t* d_counts, const uint16_t* d_slots, void* d_ent,
                      unsigned long long* d_phases, void* stream) {
  MU_REQUIRE(mu_tpack4_supported(n_rows, n_cols, nnz), "shape out of range (mu_tpack4_supported)");
  MU_REQUIRE(d_indptr && d_x_row_dst && d_x_ent && d_cdst && d_cnt && d_tile_off && d_tiles && d_counts && d_slots && d_ent,
             "null pointer");
  int64_t rpb = 0;
  int G = 0;
  mu_tpack4_geometry(n_rows, n_cols, nnz, &rpb, &G, nullptr);
  const int rw = (int)(rpb / kNW);
  const bool xcd = tune(kTune_tpack4_plain) != 1;
  const unsigned grid = xcd ? (unsigned)(8 * ((G + 7) / 8)) : (unsigned)G;
  if (d_phases)
    hipLaunchKernelGGL(k_tflat_phases, dim3(grid), dim3(kT), 0, (hipStream_t)stream, n_rows, n_cols, rw, xcd ? G : -G,
                       d_indptr, d_x_row_dst, (const unsigned long long*)d_x_ent, d_cdst, (const uint32_t*)d_cnt,
                       d_tile_off, d_tiles, d_counts, d_slots, (unsigned long long*)d_ent, d_phases);
  else
    hipLaunchKernelGGL(k_tflat_move, dim3(grid), dim3(kT), 0, (hipStream_t)stream, n_rows, n_cols, rw, xcd ? G : -G,
                       d_indptr, d_x_row_dst, (const unsigned long long*)d_x_ent, d_cdst, (const uint32_t*)d_cnt,
                       d_tile_off, d_tiles, d_counts, d_slots, (unsigned long long*)d_ent);
  MU_CHECK_LAUNCH();
  return MU_OK;
}

int mu_tflat_fill(int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t* d_indptr, const int64_t* d_x_row_dst,
                  const void* d_x_ent, const int64_t* d_cdst, const void* d_cnt, const int64_t* d_tile_off,
                  const int32_t* d_tiles, const uint16_t* d_counts, const uint16_t* d_slots, void* d_ent, void* stream) {
  return tflat_fill(n_rows, n_cols, nnz, d_indptr, d_x_row_dst, d_x_ent, d_cdst, d_cnt, d_tile_off, d_tiles, d_counts,
                    d_slots, d_ent, nullptr, stream);
}

int mu_tflat_fill_phases(int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t* d_indptr,
                         const int64_t* d_x_row_dst, const void* d_x_ent, const int64_t* d_cdst, const void* d_cnt,
                         const int64_t* d_tile_off, const int32_t* d_tiles, const uint16_t* d_counts,
                         const uint16_t* d_slots, void* d_ent, unsigned long long* d_phases, void* stream) {
  MU_REQUIRE(d_phases, "null pointer");
  return tflat_fill(n_rows, n_cols, nnz, d_indptr, d_x_row_dst, d_x_ent, d_cdst, d_cnt, d_tile_off, d_tiles, d_counts,
                    d_slots, d_ent, d_phases, stream);
}

}  // extern "C"
