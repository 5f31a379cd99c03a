// Shared helpers for libmuon_amd.so (gfx950 only; wave = 64 lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>
#include <utility>

#include "muon_amd.h"

void mu_set_error(const char* fmt, ...);

#define MU_CHECK_HIP(expr)                                                              \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess) {                                                             \
      mu_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__,     \
                   __LINE__);                                                           \
      return MU_ERR_HIP;                                                                \
    }                                                                                   \
  } while (0)

#define MU_CHECK_LAUNCH() MU_CHECK_HIP(hipGetLastError())

#define MU_REQUIRE(cond, msg)                        \
  do {                                               \
    if (!(cond)) {                                   \
      mu_set_error("%s: %s", __func__, msg);         \
      return MU_ERR_ARG;                             \
    }                                                \
  } while (0)

constexpr int kWave = 64;

// ---- tune keys: THE table (tests, probes and bench only; every default is what ships) -----------------------------
// X(name, default, largest accepted value, description).  csrc reads a key as tune(kTune_<name>): a key that is not
// here does not compile.  mu_tune_set / mu_tune_get (csrc/runtime.hip) look the name up in the same table and refuse
// anything else; INTEGRATION.md lists it, tests/test_tune_keys.py holds the three together.
constexpr int kTuneAny = 0x7fffffff;
#define MU_TUNE_KEYS(X)                                                                                              \
  X(spmm_k, 0, 16, "row-sets per wave of the row-stream SpMM: 0 = the layout's / automatic, 1..8 force")             \
  X(spmm_mode, 0, kTuneAny, "64: cycle accounting of the row-stream SpMM (K = 8), 6: of the narrow kernel; any other non-zero value has no instance") \
  X(spmm_slab, 0, 320, "Q slab width the host asks for: 0 = the host's rule, 256 / 320 force (320 where an instance exists)") \
  X(spmm_narrow_off, 0, 1, "1: B = 16 runs the NB = 1 instance of spmm_win.hip instead of the narrow kernel")        \
  X(gram_wg, 0, kTuneAny, "workgroups per CU of the Gram kernels: 0 = 2")                                            \
  X(pack_wg, 0, kTuneAny, "workgroups per CU of the row-stream copy: 0 = 32")                                        \
  X(stream_pipe, 0, 1, "1: the row-stream copy's plain loop instead of the software-pipelined one")                  \
  X(tfidf_pipe, 0, 1, "1: the TF-IDF sweeps of r03 (the tests' reference) instead of the software-pipelined ones")   \
  X(tfidf_sum_m, 0, 2, "f32 sum sweep: 0 = by size, 1: always 8192-column bins, 2: always 16 384-column bins")      \
  X(nn_interleave, 0, 1, "1: every wave of k_skinny_nn takes a contiguous quarter of the columns (only probes set it)") \
  X(tpack_dbg, 0, 1, "1: the transposition fills run their phase-accounting instances")                              \
  X(tpack4_c, 0, kTuneAny, "columns per tile of the transposition: 0 = from the geometry")                           \
  X(tpack4_plain, 0, 1, "1: workgroup = row block instead of the XCD-aware order (only probes set it)")              \
  X(tpack4_circ, 0, 2, "2: the stream-source fill without its circular windows")                                     \
  X(tpack4_off, 0, 1, "1: the host takes mu_csr_transpose + mu_csr_stream_fill instead of the fused transposition")  \
  X(tperm_off, 0, 1, "1: the fill of tpack4.hip instead of the table-driven one")                                    \
  X(tperm_flat, 1, 1, "1: the flat read-in of tflat.hip, 0: k_tperm_move")                                           \
  X(pois_valu, 0, 1, "1: the Poisson sweep on the vector ALU instead of the matrix cores")                           \
  X(pois_lane, 0, 1, "1: one lane per entry in the sparse Poisson sweep instead of four")
enum TuneKey {
#define MU_TUNE_ENUM(name, def, max, doc) kTune_##name,
  MU_TUNE_KEYS(MU_TUNE_ENUM)
#undef MU_TUNE_ENUM
  kTuneCount
};
int tune(TuneKey key);  // the key's current value (csrc/runtime.hip)

// number of CUs of the current device (cached per device id)
int mu_num_cus();

// grid of a kernel that gives every item (a row, a chunk) one wave: `waves_per_block` items per block, capped at
// `blocks_per_cu` blocks per CU - the kernel walks the rest grid-stride - and never empty
static inline unsigned wave_grid(int64_t items, int waves_per_block, int blocks_per_cu) {
  int64_t blocks = (items + waves_per_block - 1) / waves_per_block;
  const int64_t cap = (int64_t)mu_num_cus() * blocks_per_cu;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  return (unsigned)blocks;
}

// carving a work buffer: every piece starts on a 256-byte boundary
static inline size_t align256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

// tell the compiler a value is wave-uniform (it cannot see that threadIdx.x >> 6 is)
__device__ __forceinline__ int uniform32(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ int64_t uniform64(int64_t x) {
  const int lo = __builtin_amdgcn_readfirstlane((int)(x & 0xffffffffll));
  const int hi = __builtin_amdgcn_readfirstlane((int)(x >> 32));
  return ((int64_t)hi << 32) | (int64_t)(uint32_t)lo;
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;  // valid in lane 0
}

template <typename T>
__device__ __forceinline__ T wave_sum_all(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;  // valid in every lane
}

// LDS written by one lane and read by another of the SAME wave: the wave's LDS accesses issue in order, so no
// workgroup barrier is needed - but the compiler has to be told.  The fence scope is exactly "wavefront": it emits no
// instruction and only keeps the compiler from moving LDS accesses across it; a wider scope adds waits for the
// memory operations in flight, and without the fence the barrier alone orders nothing.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): a loop whose index is a template argument of
// what the body calls (a register number in an asm statement, a counted wait)
template <int... I, class F>
__device__ __forceinline__ void static_for_impl(std::integer_sequence<int, I...>, F&& f) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  static_for_impl(std::make_integer_sequence<int, N>{}, static_cast<F&&>(f));
}

// ---- host-side dispatch: a run-time value picks the template instance, every ladder spelt once -------------------
// Each returns what f returns (every branch the same type).  MU_REQUIRE / MU_CHECK_* inside f return from f: either f
// returns the int status and the entry point returns the helper's, or f only launches and MU_CHECK_LAUNCH() follows
// the helper call.  The entry point's MU_REQUIRE lines have refused every value the ladders do not name.
// f(float{}) for MU_DTYPE_F32, f(double{}) otherwise
template <class F>
inline constexpr auto by_dtype(int dtype, F&& f) {
  if (dtype == MU_DTYPE_F32) return f(float{});
  return f(double{});
}
// f(integral_constant<int, Wi>) for the first Wi with k <= Wi; the last entry takes everything larger
template <int W0, int... Ws, class F>
inline constexpr auto by_width(int k, F&& f) {
  if constexpr (sizeof...(Ws) == 0) {
    return f(std::integral_constant<int, W0>{});
  } else {
    if (k <= W0) return f(std::integral_constant<int, W0>{});
    return by_width<Ws...>(k, f);
  }
}
// f(integral_constant<int, i>) for i in 0 .. N - 2, f(<N - 1>) for anything else (a bool goes through by_index<2>)
template <int N, int I = 0, class F>
inline constexpr auto by_index(int i, F&& f) {
  if constexpr (I == N - 1) {
    return f(std::integral_constant<int, I>{});
  } else {
    if (i == I) return f(std::integral_constant<int, I>{});
    return by_index<N, I + 1>(i, f);
  }
}

namespace dispatch_check {  // both sides of every edge of every width list the library uses
constexpr auto self = [](auto w) { return (int)w(); };
constexpr auto size = [](auto t) { return (int)sizeof(t); };
static_assert(by_dtype(MU_DTYPE_F32, size) == 4 && by_dtype(MU_DTYPE_F64, size) == 8);
static_assert(by_width<16, 32>(-1, self) == 16 && by_width<16, 32>(1, self) == 16 && by_width<16, 32>(16, self) == 16 &&
              by_width<16, 32>(17, self) == 32 && by_width<16, 32>(32, self) == 32 && by_width<16, 32>(33, self) == 32);
static_assert(by_width<16, 32, 64>(0, self) == 16 && by_width<16, 32, 64>(16, self) == 16 &&
              by_width<16, 32, 64>(17, self) == 32 && by_width<16, 32, 64>(32, self) == 32 &&
              by_width<16, 32, 64>(33, self) == 64 && by_width<16, 32, 64>(64, self) == 64 &&
              by_width<16, 32, 64>(65, self) == 64);
static_assert(by_width<16, 32, 48, 64>(0, self) == 16 && by_width<16, 32, 48, 64>(16, self) == 16 &&
              by_width<16, 32, 48, 64>(17, self) == 32 && by_width<16, 32, 48, 64>(32, self) == 32 &&
              by_width<16, 32, 48, 64>(33, self) == 48 && by_width<16, 32, 48, 64>(48, self) == 48 &&
              by_width<16, 32, 48, 64>(49, self) == 64 && by_width<16, 32, 48, 64>(64, self) == 64 &&
              by_width<16, 32, 48, 64>(65, self) == 64);
static_assert(by_width<4, 8, 12, 16>(0, self) == 4 && by_width<4, 8, 12, 16>(4, self) == 4 &&
              by_width<4, 8, 12, 16>(5, self) == 8 && by_width<4, 8, 12, 16>(8, self) == 8 &&
              by_width<4, 8, 12, 16>(9, self) == 12 && by_width<4, 8, 12, 16>(12, self) == 12 &&
              by_width<4, 8, 12, 16>(13, self) == 16 && by_width<4, 8, 12, 16>(16, self) == 16 &&
              by_width<4, 8, 12, 16>(17, self) == 16);
static_assert(by_width<4, 8, 12, 16, 32>(0, self) == 4 && by_width<4, 8, 12, 16, 32>(4, self) == 4 &&
              by_width<4, 8, 12, 16, 32>(5, self) == 8 && by_width<4, 8, 12, 16, 32>(8, self) == 8 &&
              by_width<4, 8, 12, 16, 32>(9, self) == 12 && by_width<4, 8, 12, 16, 32>(12, self) == 12 &&
              by_width<4, 8, 12, 16, 32>(13, self) == 16 && by_width<4, 8, 12, 16, 32>(16, self) == 16 &&
              by_width<4, 8, 12, 16, 32>(17, self) == 32 && by_width<4, 8, 12, 16, 32>(32, self) == 32 &&
              by_width<4, 8, 12, 16, 32>(33, self) == 32);
static_assert(by_width<64, 128, 256, 512, 1024>(0, self) == 64 && by_width<64, 128, 256, 512, 1024>(64, self) == 64 &&
              by_width<64, 128, 256, 512, 1024>(65, self) == 128 && by_width<64, 128, 256, 512, 1024>(128, self) == 128 &&
              by_width<64, 128, 256, 512, 1024>(129, self) == 256 && by_width<64, 128, 256, 512, 1024>(256, self) == 256 &&
              by_width<64, 128, 256, 512, 1024>(257, self) == 512 && by_width<64, 128, 256, 512, 1024>(512, self) == 512 &&
              by_width<64, 128, 256, 512, 1024>(513, self) == 1024 && by_width<64, 128, 256, 512, 1024>(1024, self) == 1024 &&
              by_width<64, 128, 256, 512, 1024>(1025, self) == 1024);
static_assert(by_width<1, 8, 32>(0, self) == 1 && by_width<1, 8, 32>(1, self) == 1 && by_width<1, 8, 32>(2, self) == 8 &&
              by_width<1, 8, 32>(8, self) == 8 && by_width<1, 8, 32>(9, self) == 32 && by_width<1, 8, 32>(32, self) == 32 &&
              by_width<1, 8, 32>(33, self) == 32);
static_assert(by_width<1, 2, 4, 8>(0, self) == 1 && by_width<1, 2, 4, 8>(1, self) == 1 && by_width<1, 2, 4, 8>(2, self) == 2 &&
              by_width<1, 2, 4, 8>(3, self) == 4 && by_width<1, 2, 4, 8>(4, self) == 4 && by_width<1, 2, 4, 8>(5, self) == 8 &&
              by_width<1, 2, 4, 8>(8, self) == 8 && by_width<1, 2, 4, 8>(9, self) == 8);
static_assert(by_index<2>(false, self) == 0 && by_index<2>(true, self) == 1 && by_index<2>(-1, self) == 1 &&
              by_index<2>(7, self) == 1);
static_assert(by_index<3>(0, self) == 0 && by_index<3>(1, self) == 1 && by_index<3>(2, self) == 2 &&
              by_index<3>(3, self) == 2 && by_index<3>(-1, self) == 2);
static_assert(by_index<4>(0, self) == 0 && by_index<4>(1, self) == 1 && by_index<4>(2, self) == 2 &&
              by_index<4>(3, self) == 3 && by_index<4>(4, self) == 3 && by_index<4>(-1, self) == 3);
}  // namespace dispatch_check

// lane `l` of a 64-bit value, as two 32-bit readlanes (l wave-uniform)
__device__ __forceinline__ uint64_t readlane_u64(uint64_t v, int l) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ double readlane_f64(double v, int l) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), l);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// lane `L` of v <- the wave-uniform x (this clang has no writelane builtin)
template <int L>
__device__ __forceinline__ int writelane_c(int v, int x) {
  asm("v_writelane_b32 %0, %1, %2" : "+v"(v) : "s"(x), "n"(L));
  return v;
}
// the same with a wave-uniform lane number.  The lane select goes through M0 (one SGPR operand per instruction) and M0
// is CLOBBERED: nothing that keeps a value in M0 (dma_piece's LDS address, an LDS-direct load) may span a call.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"  // ("clobber list contains reserved registers: m0": meant)
__device__ __forceinline__ int writelane_s(int v, int x, int l) {
  asm("s_mov_b32 m0, %2\n\tv_writelane_b32 %0, %1, m0" : "+v"(v) : "s"(x), "s"(l) : "m0");
  return v;
}
#pragma clang diagnostic pop

// One LDS-DMA piece: 64 lanes x 16 B land contiguously at the wave-uniform LDS byte address `lds_dst`; the source is
// base (scalar) + a 32-bit byte offset per lane (64-bit per-lane addresses cost four registers and a 64-bit clamp per
// piece; callers keep the operand under 4 GiB and check it on the host).  The destination travels in M0, which the
// compiler also uses: it is saved and restored inside the one asm statement (early-clobber `keep`), and the s_nop
// covers the hazard between the write of M0 and the load that reads it.
__device__ __forceinline__ void dma_piece(const void* base, unsigned byte_off, unsigned lds_dst) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %3\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, %2\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(byte_off), "s"(base), "s"(lds_dst)
      : "memory");
}

// The (column, value) pair at ib + off / vb + off (byte offset), issued from asm and NOT waited for: the caller's
// counted wait (pipe_wait, sf_wait: each file's own, it names the registers of its own pipeline) takes c and v as
// read-write operands, so every use is ordered behind it.  Early-clobber outputs: the second load still reads `off`
// after the first has been given its destination.
__device__ __forceinline__ void load_pair(const int32_t* ib, const float* vb, unsigned off, int32_t& c, float& v) {
  asm volatile("global_load_dword %0, %2, %3\n\tglobal_load_dword %1, %2, %4"
               : "=&v"(c), "=&v"(v)
               : "v"(off), "s"(ib), "s"(vb)
               : "memory");
}

// The pieces of a wave's strip of rows walked as ONE flat sequence of iterations: row l's piece is [lo_l, hi_l) of
// lane l, `step` entries at a time, then the next row's.  Start with {-1, 0, 0, rows, step}.
struct FlatWalk {
  int l, pb, hi, nrow, step;
  // the next iteration: false when the strip is through (wave-uniform: every member lives in scalar registers)
  __device__ __forceinline__ bool advance(int lo_l, int hi_l) {
    pb += step;
    while (pb >= hi) {
      if (++l >= nrow) return false;
      pb = __builtin_amdgcn_readlane(lo_l, l);
      hi = __builtin_amdgcn_readlane(hi_l, l);
    }
    return true;
  }
};

// v_mfma_{f32,f64}_16x16x4: A operand lane l = A[i = l & 15][k = l >> 4], B operand lane l = B[k = l >> 4][j = l & 15],
// C/D register r of lane l = C[row(l >> 4, r)][col = l & 15] - the one place where the two instructions differ.
template <typename T> struct Mfma16x16x4;
template <> struct Mfma16x16x4<float> {
  typedef float acc_t __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ acc_t mfma(float a, float b, acc_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int row(int q, int r) { return 4 * q + r; }
};
template <> struct Mfma16x16x4<double> {
  typedef double acc_t __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ acc_t mfma(double a, double b, acc_t c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int row(int q, int r) { return q + 4 * r; }
};

// transcendentals in the storage type: the hardware's exp / log for an f32 model, libm's for f64 (and for log1p)
__device__ __forceinline__ float mu_exp(float x) { return __expf(x); }
__device__ __forceinline__ double mu_exp(double x) { return exp(x); }
__device__ __forceinline__ float mu_log(float x) { return __logf(x); }
__device__ __forceinline__ double mu_log(double x) { return log(x); }
__device__ __forceinline__ float mu_log1p(float x) { return log1pf(x); }
__device__ __forceinline__ double mu_log1p(double x) { return log1p(x); }

// first index i in [lo, hi) with a[i] >= key (a ascending)
__device__ __forceinline__ int64_t lower_bound_i64(const int64_t* a, int64_t lo, int64_t hi,
                                                   int64_t key) {
  while (lo < hi) {
    int64_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// splitmix64: counter-based hashing for reproducible device-side random numbers
__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// uniform in (0,1) from the top 24 bits
__host__ __device__ __forceinline__ float u01(uint64_t h) {
  return ((float)(h >> 40) + 0.5f) * (1.0f / 16777216.0f);
}
