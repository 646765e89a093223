// K32: the Mann-Kendall statistics and the Theil-Sen slopes of every row of a row block -- the rank-based trend of an
// index series (K27 / K29: one value per year and grid point), where least squares (K21) is not what is reported.
// Y is n <= 128 columns (time points) of m floats; a point is valid iff it is finite (K20's test of the bits).
//
// Arithmetic (the contract of tests/mk_ref.py, held bit for bit): S, E and the tie term G are integers formed from IEEE
// comparisons of the valid points.  A slope is fp32(fp64(y_b - y_a) / (t_b - t_a)): one rounded subtraction each, one
// correctly rounded division, one rounding to fp32, nothing fused (contraction is off for the whole file), nothing
// flushed.  The N = v (v - 1) / 2 slopes are ordered by K25's key of the bit pattern and the order statistic of a
// rank passes with its bits unchanged.
//
// One wave takes one row at a time.  It compacts the valid points with a ballot prefix into its LDS slice; the N pairs
// are spread evenly over the lanes (pair p = lane + 64 k, decoded to (a, b)), every lane forms the keys of its pairs once
// into the wave's slice, and the wave bisects the key most significant bit first for the four ranks at once
// (cquant.hip's selection: the largest x with count(key < x) <= rank IS the order statistic).  Counts are integers summed
// through the lanes: the bits depend on the operands alone.  No atomics, no workspace, no barrier: a wave shares its
// slice with nobody.
//
// The slice holds the 8128 keys of 128 points whatever n is: 32 KB per wave, one workgroup per CU.  A slice sized by n
// would put more rows of short series in flight; whether that pays has not been measured, so it is not here.
#include "time_rows.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRowsPerWg = 32;                     // consecutive rows: the waves of a workgroup share the lines of Y
constexpr int kMaxN = DMDX_MK_MAX_N;
constexpr int kMaxRanks = DMDX_SEN_MAX_RANKS;
constexpr int kCap = 8192;                         // keys of a wave's slice: N <= 8128, rounded up to 256
constexpr uint32_t kPadKey = 0xFFFFFFFFu;          // above every key that is not a NaN's, and no slope is a NaN
static_assert(kMaxN * (kMaxN - 1) / 2 <= kCap && kCap % 256 == 0, "the slice holds the pairs of kMaxN points");

struct TimeAxis { double t[kMaxN]; };              // travels by value, padded with its last entry

__device__ __forceinline__ uint32_t key_of(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ uint32_t bits_of(uint32_t k) { return (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k; }

template <int CTRL>
__device__ __forceinline__ uint32_t dpp(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
}

// v of every lane -> the sum over the 64 lanes, in every lane (cquant.hip's lanes_reduce; every lane active)
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  v += dpp<0xB1>(v);
  v += dpp<0x4E>(v);
  v += dpp<0x141>(v);
  v += dpp<0x140>(v);
  v += (uint32_t)__shfl_xor((int)v, 16);
  v += (uint32_t)__shfl_xor((int)v, 32);
  return v;
}

// what a lane wrote to the wave's slice is there for the other lanes: the wave's LDS operations run in order, this
// keeps the compiler from moving them
__device__ __forceinline__ void slice_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); }

// The valid points of row i in ascending time -> ys[0 .. v) (and their coordinates -> ts[0 .. v) where ts is given);
// lane l looks at the points l and l + 64.  Returns v, the same in every lane.
template <bool TIMES>
__device__ __forceinline__ int compact_row(const float* __restrict__ Y, int64_t i, int n, int64_t ldy, const TimeAxis* tc,
                                           float* ys, double* ts, int lane) {
  const float* p = Y + i;
  float x0 = 0.f, x1 = 0.f;
  bool ok0 = false, ok1 = false;
  if (lane < n) {
    x0 = p[(int64_t)lane * ldy];
    ok0 = finite_bits(x0);
  }
  if (lane + 64 < n) {
    x1 = p[(int64_t)(lane + 64) * ldy];
    ok1 = finite_bits(x1);
  }
  const uint64_t m0 = __ballot(ok0), m1 = __ballot(ok1), below = (1ull << lane) - 1ull;
  const int c0 = __popcll(m0);
  if (ok0) {
    const int k = __popcll(m0 & below);
    ys[k] = x0;
    if (TIMES) ts[k] = tc->t[lane];
  }
  if (ok1) {
    const int k = c0 + __popcll(m1 & below);
    ys[k] = x1;
    if (TIMES) ts[k] = tc->t[lane + 64];
  }
  return c0 + __popcll(m1);
}

// ---- the integer planes: v, S, E, G.  Lane l holds the points a = l and l + 64 and walks all points b once.
__global__ __launch_bounds__(kThreads) void mk_stats_kernel(const float* __restrict__ Y, int64_t m, int n, int64_t ldy,
                                                            int32_t* __restrict__ out, int64_t ldo) {
  __shared__ float ys_all[kWaves][kMaxN];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* ys = ys_all[wave];
  const int64_t r0 = (int64_t)blockIdx.x * kRowsPerWg;
  for (int r = wave; r < kRowsPerWg; r += kWaves) {
    const int64_t i = r0 + r;
    if (i >= m) break;                                          // (the same in every lane)
    slice_fence();                                              // the row before is done with
    const int v = compact_row<false>(Y, i, n, ldy, nullptr, ys, nullptr, lane);
    slice_fence();
    const int a0 = lane, a1 = lane + 64;
    const bool in0 = a0 < v, in1 = a1 < v;
    const float y0 = in0 ? ys[a0] : 0.f, y1 = in1 ? ys[a1] : 0.f;
    int s = 0, e = 0, c0 = 0, c1 = 0;
    for (int b = 0; b < v; ++b) {
      const float yb = ys[b];                                   // (one address: a broadcast)
      const int eq0 = yb == y0 ? 1 : 0, eq1 = yb == y1 ? 1 : 0;
      c0 += eq0;
      c1 += eq1;
      if (in0 && b > a0) {
        s += (yb > y0 ? 1 : 0) - (yb < y0 ? 1 : 0);
        e += eq0;
      }
      if (in1 && b > a1) {
        s += (yb > y1 ? 1 : 0) - (yb < y1 ? 1 : 0);
        e += eq1;
      }
    }
    const int g = (in0 ? (c0 - 1) * (2 * c0 + 5) : 0) + (in1 ? (c1 - 1) * (2 * c1 + 5) : 0);
    const uint32_t S = wave_sum((uint32_t)s), E = wave_sum((uint32_t)e), G = wave_sum((uint32_t)g);
    if (lane < DMDX_MK_NQ)
      out[(int64_t)lane * ldo + i] = (int32_t)(lane == 0 ? (uint32_t)v : lane == 1 ? S : lane == 2 ? E : G);
  }
}

// the first pair of point a among the pairs (a, b), a < b < v, counted row by row: a (2 v - a - 1) / 2
__device__ __forceinline__ int pair_base(int a, int v) { return a * (2 * v - a - 1) / 2; }

// ---- the slopes: the order statistics rank[j, i] of the N slope keys of row i
__global__ __launch_bounds__(kThreads) void sen_kernel(const float* __restrict__ Y, int64_t m, int n, int64_t ldy, TimeAxis tc,
                                                       const int32_t* __restrict__ rank, int64_t ldr, int J,
                                                       float* __restrict__ out, int64_t ldo) {
  __shared__ uint4 keys_all[kWaves][kCap / 4];
  __shared__ double ts_all[kWaves][kMaxN];
  __shared__ float ys_all[kWaves][kMaxN];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint4* keys4 = keys_all[wave];
  uint32_t* keys = reinterpret_cast<uint32_t*>(keys_all[wave]);
  double* ts = ts_all[wave];
  float* ys = ys_all[wave];
  const int64_t r0 = (int64_t)blockIdx.x * kRowsPerWg;
  for (int r = wave; r < kRowsPerWg; r += kWaves) {
    const int64_t i = r0 + r;
    if (i >= m) break;                                          // (the same in every lane)
    slice_fence();                                              // the row before is done with
    const int v = compact_row<true>(Y, i, n, ldy, &tc, ys, ts, lane);
    slice_fence();
    const int N = v * (v - 1) / 2, Npad = (N + 255) & ~255;     // Npad <= kCap

    // pair p -> (a, b): a from the root of base(a) = p in fp32 (all integers here are below 2^17: exact), then stepped
    // to the row that holds p whatever the rounding of the root was
    const int w = 2 * v - 1;
    for (int p = lane; p < N; p += 64) {
      int a = (int)(((float)w - sqrtf((float)(w * w - 8 * p))) * 0.5f);
      a = a < 0 ? 0 : (a > v - 2 ? v - 2 : a);
      while (pair_base(a, v) > p) --a;
      while (pair_base(a + 1, v) <= p) ++a;                     // (base(v - 1) = N > p: a stays <= v - 2)
      const int b = a + 1 + (p - pair_base(a, v));
      const double d = (double)ys[b] - (double)ys[a];
      const double h = ts[b] - ts[a];
      const double s = d / h;
      keys[p] = key_of(__builtin_bit_cast(uint32_t, (float)s));
    }
    for (int p = N + lane; p < Npad; p += 64) keys[p] = kPadKey;
    slice_fence();

    uint32_t rk[kMaxRanks], x[kMaxRanks];
    bool has[kMaxRanks];
#pragma unroll
    for (int j = 0; j < kMaxRanks; ++j) {
      const int32_t q = rank[(int64_t)(j < J ? j : J - 1) * ldr + i];
      has[j] = q >= 0 && q < N;
      rk[j] = has[j] ? (uint32_t)q : 0u;
      x[j] = 0u;
    }
    const int quads = Npad / 256;                               // 16-byte reads of a lane per step
#pragma unroll 1
    for (int bit = 31; bit >= 0 && N > 0; --bit) {
      uint32_t cand[kMaxRanks], cnt[kMaxRanks];
#pragma unroll
      for (int j = 0; j < kMaxRanks; ++j) {
        cand[j] = x[j] | (1u << bit);
        cnt[j] = 0u;
      }
      for (int k = 0; k < quads; ++k) {
        const uint4 q = keys4[lane + 64 * k];
        const uint32_t key[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < kMaxRanks; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) cnt[j] += key[e] < cand[j] ? 1u : 0u;
      }
      // counts <= N <= 8128 < 2^16: two ranks share a register on the way through the lanes
      static_assert(kMaxRanks == 4, "the counts of four ranks travel in two registers");
      const uint32_t s01 = wave_sum(cnt[0] | (cnt[1] << 16)), s23 = wave_sum(cnt[2] | (cnt[3] << 16));
      cnt[0] = s01 & 0xFFFFu, cnt[1] = s01 >> 16, cnt[2] = s23 & 0xFFFFu, cnt[3] = s23 >> 16;
#pragma unroll
      for (int j = 0; j < kMaxRanks; ++j) x[j] = cnt[j] <= rk[j] ? cand[j] : x[j];
    }
#pragma unroll
    for (int j = 0; j < kMaxRanks; ++j)
      if (lane == j && j < J)
        out[(int64_t)j * ldo + i] = __builtin_bit_cast(float, has[j] ? bits_of(x[j]) : kQuietNaN);
  }
}

unsigned grid_of(int64_t m) { return (unsigned)((m + kRowsPerWg - 1) / kRowsPerWg); }

}  // namespace

extern "C" int dmdx_mk_max_n(void) { return kMaxN; }
extern "C" int dmdx_sen_max_ranks(void) { return kMaxRanks; }

extern "C" int dmdx_mk_stats_f32(const float* Y, int64_t m, int64_t n, int64_t ldy, int32_t* out, int64_t ldo, void* stream) {
  DMDX_CHECK_ARG(Y && out, "mk_stats: null pointer");
  DMDX_CHECK_ARG(n >= 1 && n <= kMaxN, "mk_stats: n=%lld outside 1..%d", (long long)n, kMaxN);
  if (int rc = check_block("mk_stats", m, n, {{"ldy", ldy}, {"ldo", ldo}}, {Y, out})) return rc;
  if (int rc = check_ranges("mk_stats", Y, n, ldy, (const float*)out, DMDX_MK_NQ, ldo, m, false)) return rc;
  if (m == 0) return 0;
  hipLaunchKernelGGL(mk_stats_kernel, dim3(grid_of(m)), dim3(kThreads), 0, (hipStream_t)stream, Y, m, (int)n, ldy, out, ldo);
  DMDX_LAUNCH_CHECK();
  return 0;
}

extern "C" int dmdx_sen_slopes_f32(const float* Y, int64_t m, int64_t n, int64_t ldy, const double* tc, const int32_t* rank,
                                   int64_t ldr, int J, float* out, int64_t ldo, void* stream) {
  DMDX_CHECK_ARG(Y && out && tc && rank, "sen_slopes: null pointer");
  DMDX_CHECK_ARG(n >= 1 && n <= kMaxN, "sen_slopes: n=%lld outside 1..%d", (long long)n, kMaxN);
  DMDX_CHECK_ARG(J >= 1 && J <= kMaxRanks, "sen_slopes: J=%d outside 1..%d", J, kMaxRanks);
  if (int rc = check_block("sen_slopes", m, n, {{"ldy", ldy}, {"ldo", ldo}, {"ldr", ldr}}, {Y, out, rank}, {tc})) return rc;
  TimeAxis ax;
  for (int t = 0; t < kMaxN; ++t) {
    const double c = tc[t < n ? t : n - 1];
    if (t < n)
      DMDX_CHECK_ARG(c - c == 0.0 && (t == 0 || c > ax.t[t - 1]),
                     "sen_slopes: tc[%d]=%g is not finite or does not ascend strictly", t, c);
    ax.t[t] = c;
  }
  if (int rc = check_ranges("sen_slopes", Y, n, ldy, out, J, ldo, m, false)) return rc;
  if (int rc = check_ranges("sen_slopes", (const float*)rank, J, ldr, out, J, ldo, m, false)) return rc;
  if (m == 0) return 0;
  const dim3 grid(grid_of(m)), block(kThreads);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sen_kernel, grid, block, 0, st, Y, m, (int)n, ldy, ax, rank, ldr, J, out, ldo);
  DMDX_LAUNCH_CHECK();
  return 0;
}
