// K25: empirical quantiles of the snapshots of one row block per calendar slot, on the device -- the thresholds K24
// scores against when the climate is not normal (ETCCDI percentiles, terciles).  The lists are K18's (clim.hip): slot s
// owns order[start[s] .. start[s + 1]), start clamped to [0, n_order], an entry outside [0, T) skipped and not counted.
//
// Arithmetic (the contract of tests/quant_ref.py, held bit for bit): the n_s counted members of (slot, row) are
// ordered by the order-preserving key of their bit pattern (key_of: a total order, -0.0 before +0.0, the infinities
// and denormals ordinary values); h = q (n_s - 1) in fp64 picks x_(lo) and, for the linear method with a fractional
// h, x_(lo + 1), and r = a + (b - a) g runs in fp64, every step rounded, one rounding to fp32.  An order statistic
// passes with its bits unchanged.  Contraction is off for the whole file.
//
// Selection is a bisection on the key, most significant bit first: the largest v with count(key < v) <= lo IS x_(lo).
// A step counts, for every row and J candidates at once, the keys below the candidates; one last pass yields
// count(key <= x_(lo)) and min(key > x_(lo)), hence x_(lo + 1).  No sort, no workspace, no atomics: the counts are
// integers, so the bits depend on the operands alone, not on which body ran or how the members were split over lanes.
//
// A workgroup takes a slot and 64 consecutive rows, and chooses per slot, by the length of the (clamped) list:
//   staged    <= kCap64 entries: the keys of 64 rows go to LDS once; <= 2 kCap64: 32 rows at a time, two passes;
//             <= 4 kCap64 = dmdx_clim_quantile_max_staged(): 16 rows at a time, four passes.  One read of X.
//   streamed  longer lists (or streamed != 0): the same bisection with the members re-read from global memory in
//             every step.  Slow and correct; no limit on the list.
// A skipped entry keeps its place in the staged tile as the key 0xFFFFFFFF, above every value that is not a NaN:
// the ranks below n_s never reach it.  A NaN member is seen while staging (or in the streamed body's first pass).
#include "time_rows.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kTileRows = 64;                      // rows of a workgroup
constexpr int kCap64 = 208;                        // list entries of a 64-row tile: 52 KB, three workgroups per CU
constexpr int kMaxStaged = 4 * kCap64;
constexpr int kTileDwords = kCap64 * kTileRows;
constexpr uint32_t kSkipped = 0xFFFFFFFFu;
constexpr int kFly = 4;                            // loads of a lane issued before their keys are used (streamed)
constexpr int kStageFly = 16;                      // ... while staging: 48 KB in flight per CU with three workgroups

struct QList { double q[DMDX_CLIM_QUANTILE_MAX_Q]; };

__device__ __forceinline__ uint32_t key_of(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ uint32_t bits_of(uint32_t k) { return (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k; }
__device__ __forceinline__ bool nan_bits(uint32_t u) { return (u & 0x7FFFFFFFu) > 0x7F800000u; }

template <int CTRL>
__device__ __forceinline__ uint32_t dpp(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
}

enum Op { kAdd, kMin, kOr, kAnd };
template <int OP>
__device__ __forceinline__ uint32_t op2(uint32_t a, uint32_t b) {
  return OP == kAdd ? a + b : OP == kMin ? (a < b ? a : b) : OP == kOr ? (a | b) : (a & b);
}

// v of every lane -> op over the G consecutive lanes the lane belongs to (G = 16, 32, 64; every lane active):
// quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror inside the 16-lane row, bpermute beyond.
template <int G, int OP>
__device__ __forceinline__ uint32_t lanes_reduce(uint32_t v) {
  auto op = [](uint32_t a, uint32_t b) { return op2<OP>(a, b); };
  v = op(v, dpp<0xB1>(v));
  v = op(v, dpp<0x4E>(v));
  v = op(v, dpp<0x141>(v));
  v = op(v, dpp<0x140>(v));
  if (G >= 32) v = op(v, (uint32_t)__shfl_xor((int)v, 16));
  if (G >= 64) v = op(v, (uint32_t)__shfl_xor((int)v, 32));
  return v;
}

// The ranks of a slot with n counted members (the same in every lane): x_(lo[j]), and with lerp[j] the fp64
// interpolation towards x_(lo[j] + 1) by g[j].
template <int JT>
struct Rank {
  uint32_t lo[JT];
  double g[JT];
  bool any_lerp;
};

template <int JT>
__device__ __forceinline__ Rank<JT> rank_of(const QList& ql, int method, int64_t n) {
  Rank<JT> rk;
  rk.any_lerp = false;
#pragma unroll
  for (int j = 0; j < JT; ++j) {
    const double q = ql.q[j];                                   // (the host repeats the last one beyond J)
    const double h = q * (double)(n > 0 ? n - 1 : 0);           // one rounding
    const double fl = floor(h);
    double g = h - fl;
    double pos = fl;
    if (method == 1) g = 0.0;
    if (method == 2) { pos = ceil(h); g = 0.0; }
    rk.lo[j] = (uint32_t)pos;
    rk.g[j] = g;
    rk.any_lerp = rk.any_lerp || g != 0.0;
  }
  return rk;
}

// The bisection over the members a source presents.  Src: count_below(cand, cnt) -- per (j, row) the members whose key
// lies below cand, over the whole list --, above(x, cnt_le, mn) -- per row count(key <= x) and min(key > x) --, spread(or, and)
// -- the OR and the AND of the row's keys, skipped entries left out.
// A bit that all keys of a row share is that bit of every order statistic of the row, and the step would find just
// that: the shared bits are set beforehand, and a step no row of the wave needs is not taken (ERA5 temperatures share
// the sign and most of the exponent).  Shared ones below the bit of a step change no count: every key carries them.
template <int V, int JT, class Src>
__device__ __forceinline__ void select_rows(Src& src, const Rank<JT>& rk, uint32_t (&xlo)[JT][V], uint32_t (&xhi)[JT][V]) {
  uint32_t orv[V], andv[V], differ = 0u;
  src.spread(orv, andv);
#pragma unroll
  for (int e = 0; e < V; ++e) differ |= (orv[e] == 0u && andv[e] == 0xFFFFFFFFu) ? 0u : orv[e] ^ andv[e];   // (no key at all)
  // the bits in which the keys of some row of the wave differ (the waves that meet at a barrier hold the same rows)
  uint32_t steps = __builtin_amdgcn_readfirstlane(lanes_reduce<64, kOr>(differ));
#pragma unroll
  for (int j = 0; j < JT; ++j)
#pragma unroll
    for (int e = 0; e < V; ++e) xlo[j][e] = andv[e] & ~steps;
  while (steps != 0u) {
    const int bit = 31 - __builtin_clz(steps);
    steps &= ~(1u << bit);
    uint32_t cand[JT][V], cnt[JT][V];
#pragma unroll
    for (int j = 0; j < JT; ++j)
#pragma unroll
      for (int e = 0; e < V; ++e) {
        cand[j][e] = xlo[j][e] | (1u << bit);
        cnt[j][e] = 0u;
      }
    src.count_below(cand, cnt);
#pragma unroll
    for (int j = 0; j < JT; ++j)
#pragma unroll
      for (int e = 0; e < V; ++e) xlo[j][e] = cnt[j][e] <= rk.lo[j] ? cand[j][e] : xlo[j][e];
  }
#pragma unroll
  for (int j = 0; j < JT; ++j) {                                // one pass per interpolated quantile: few registers
    uint32_t cnt[V], mn[V];
    if (rk.g[j] != 0.0) src.above(xlo[j], cnt, mn);             // (the same in every lane)
#pragma unroll
    for (int e = 0; e < V; ++e)
      xhi[j][e] = (rk.g[j] != 0.0 && cnt[e] <= rk.lo[j] + 1u) ? mn[e] : xlo[j][e];   // ties: x_(lo + 1) = x_(lo)
  }
}

// The value of (j, row) from its two order statistics, as bits.
__device__ __forceinline__ uint32_t value_bits(uint32_t klo, uint32_t khi, double g) {
  const uint32_t ulo = bits_of(klo);
  if (g == 0.0) return ulo;
  const double a = (double)__builtin_bit_cast(float, ulo), b = (double)__builtin_bit_cast(float, bits_of(khi));
  const double d = b - a;
  const double p = d * g;
  const double r = a + p;
  return __builtin_bit_cast(uint32_t, (float)r);
}

// rows r .. r + V - 1 of slot s, written by the lane whose `writer` equals j: plane j of out
template <int V, int JT>
__device__ __forceinline__ void write_rows(float* __restrict__ out, int64_t ldo, int64_t S, int64_t s, int64_t m, int64_t r,
                                           int J, int writer, int64_t n, const Rank<JT>& rk, const bool (&isnan)[V],
                                           const uint32_t (&xlo)[JT][V], const uint32_t (&xhi)[JT][V]) {
#pragma unroll
  for (int j = 0; j < JT; ++j) {
    if (writer != j || j >= J) continue;
    float* o = out + ((int64_t)j * S + s) * ldo + r;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      if (r + e >= m) continue;
      const uint32_t bits = (n == 0 || isnan[e]) ? kQuietNaN : value_bits(xlo[j][e], xhi[j][e], rk.g[j]);
      o[e] = __builtin_bit_cast(float, bits);
    }
  }
}

// ---- staged: the keys of R rows x len list entries in LDS, entry-major, 16 bytes (4 rows) per lane and read.
// Entry e holds its R / 4 quads at quad (rq ^ sw(e)), sw(e) = (e >> SH) & (Q - 1): the 16 lanes a ds_read_b128 serves in
// one cycle then hit 16 different 16-byte slots of the 256-byte bank row in all three tiers.  Wave w owns the quads
// w QW .. w QW + QW - 1, its 64 lanes = QW quads x G entries: lane (rql, g) walks the entries g, g + G, ...
template <int R>
struct Tier {
  static constexpr int Q = R / 4, SUBS = kThreads / R, SH = R == 64 ? 0 : (R == 32 ? 1 : 2), QW = R / 16, G = 64 / QW;
};

template <int R, int JT>
struct StagedSrc {
  typedef Tier<R> Tr;
  const uint4* p;       // the lane's quad of its first entry
  int g, len;

  __device__ __forceinline__ void count_below(const uint32_t (&cand)[JT][4], uint32_t (&cnt)[JT][4]) {
    const uint4* q = p;
#pragma unroll 1
    for (int k = g; k < len; k += Tr::G, q += Tr::G * Tr::Q) {
      const uint4 v = *q;
      const uint32_t key[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < JT; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) cnt[j][e] += key[e] < cand[j][e] ? 1u : 0u;
    }
    // counts <= len <= 832 < 2^16: two rows share a register on the way through the lanes
#pragma unroll
    for (int j = 0; j < JT; ++j)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const uint32_t s = lanes_reduce<Tr::G, kAdd>(cnt[j][e] | (cnt[j][e + 2] << 16));
        cnt[j][e] = s & 0xFFFFu;
        cnt[j][e + 2] = s >> 16;
      }
  }

  __device__ __forceinline__ void above(const uint32_t (&x)[4], uint32_t (&cnt)[4], uint32_t (&mn)[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      cnt[e] = 0u;
      mn[e] = kSkipped;
    }
    const uint4* q = p;
    for (int k = g; k < len; k += Tr::G, q += Tr::G * Tr::Q) {
      const uint4 v = *q;
      const uint32_t key[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool le = key[e] <= x[e];
        cnt[e] += le ? 1u : 0u;
        mn[e] = (!le && key[e] < mn[e]) ? key[e] : mn[e];
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      cnt[e] = lanes_reduce<Tr::G, kAdd>(cnt[e]);
      mn[e] = lanes_reduce<Tr::G, kMin>(mn[e]);
    }
  }

  __device__ __forceinline__ void spread(uint32_t (&orv)[4], uint32_t (&andv)[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      orv[e] = 0u;
      andv[e] = 0xFFFFFFFFu;
    }
    const uint4* q = p;
    for (int k = g; k < len; k += Tr::G, q += Tr::G * Tr::Q) {
      const uint4 v = *q;
      const uint32_t key[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        orv[e] |= key[e] == kSkipped ? 0u : key[e];
        andv[e] &= key[e];
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      orv[e] = lanes_reduce<Tr::G, kOr>(orv[e]);
      andv[e] = lanes_reduce<Tr::G, kAnd>(andv[e]);
    }
  }
};

template <int R, int JT>
__device__ __forceinline__ void staged_pass(uint4* tile4, int* nanrow, int* cntv, const float* __restrict__ X, int64_t m,
                                            int64_t T, int64_t ldx, const int32_t* __restrict__ ord, int len,
                                            const QList& ql, int J, int method, int64_t rbase, int64_t S, int64_t s,
                                            float* __restrict__ out, int64_t ldo) {
  typedef Tier<R> Tr;
  const int tid = threadIdx.x;
  uint32_t* tile = reinterpret_cast<uint32_t*>(tile4);
  __syncthreads();                                              // the tile and the flags of the pass before are done with
  if (tid < kTileRows) nanrow[tid] = 0;
  __syncthreads();

  {
    const int sub = tid / R, row = tid % R;
    const bool rowok = rbase + row < m;
    const float* xp = X + rbase + row;
    const int qd = row >> 2, el = row & 3;
    int nv = 0;
    bool sawnan = false;
    for (int e0 = sub; e0 < len; e0 += Tr::SUBS * kStageFly) {
      uint32_t u[kStageFly];
      bool in[kStageFly], ok[kStageFly];
#pragma unroll
      for (int f = 0; f < kStageFly; ++f) {
        const int e = e0 + f * Tr::SUBS;
        in[f] = e < len;
        const int32_t t = ord[in[f] ? e : e0];
        const bool counted = in[f] && t >= 0 && (int64_t)t < T;
        nv += counted ? 1 : 0;
        ok[f] = counted && rowok;
        u[f] = 0u;
        if (ok[f]) u[f] = __builtin_bit_cast(uint32_t, xp[(int64_t)t * ldx]);
      }
#pragma unroll
      for (int f = 0; f < kStageFly; ++f) {
        const int e = e0 + f * Tr::SUBS;
        sawnan = sawnan || (ok[f] && nan_bits(u[f]));
        if (in[f]) tile[e * R + (((qd ^ ((e >> Tr::SH) & (Tr::Q - 1))) << 2) | el)] = ok[f] ? key_of(u[f]) : kSkipped;
      }
    }
    if (sawnan) nanrow[row] = 1;
    if (row == 0) cntv[sub] = nv;
  }
  __syncthreads();

  int64_t n = 0;
#pragma unroll
  for (int i = 0; i < Tr::SUBS; ++i) n += cntv[i];
  const Rank<JT> rk = rank_of<JT>(ql, method, n);

  const int lane = tid & 63, wave = tid >> 6;
  const int g = lane % Tr::G, rq = wave * Tr::QW + lane / Tr::G;
  StagedSrc<R, JT> src;
  src.g = g;
  src.len = len;
  src.p = tile4 + (g * Tr::Q + (rq ^ ((g >> Tr::SH) & (Tr::Q - 1))));
  uint32_t xlo[JT][4], xhi[JT][4];
  if (n > 0) {                                                  // (the same in every lane)
    select_rows<4, JT>(src, rk, xlo, xhi);
  } else {
#pragma unroll
    for (int j = 0; j < JT; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) xlo[j][e] = xhi[j][e] = 0u;
  }
  bool isnan[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) isnan[e] = nanrow[4 * rq + e] != 0;
  write_rows<4, JT>(out, ldo, S, s, m, rbase + 4 * rq, J, g, n, rk, isnan, xlo, xhi);
}

// ---- streamed: thread (sub, row) = (tid / 64, tid % 64) reads row `row` of the entries sub, sub + 4, ...; the four
// partial results of a row meet in LDS (the tile, idle here), two barriers per step.
template <int JT>
struct StreamedSrc {
  const float* xp;      // row `row` of snapshot 0; not dereferenced when !rowok
  const int32_t* ord;
  uint32_t* part;       // [4][2 JT][64]
  int64_t len, T, ldx;
  int sub, row;
  bool rowok;
  uint32_t or_keys, and_keys;   // of the row, set by first_pass

  template <int N, int OP>
  __device__ __forceinline__ void meet(uint32_t (&v)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) part[(sub * N + i) * kTileRows + row] = v[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) {
      uint32_t r = part[i * kTileRows + row];
#pragma unroll
      for (int w = 1; w < 4; ++w) {
        const uint32_t o = part[(w * N + i) * kTileRows + row];
        r = op2<OP>(r, o);
      }
      v[i] = r;
    }
    __syncthreads();
  }

  // f(key, counted, isnan) over the lane's entries, kFly loads in flight
  template <class F>
  __device__ __forceinline__ void walk(F f) {
    for (int64_t e0 = sub; e0 < len; e0 += 4 * kFly) {
      uint32_t u[kFly];
      bool counted[kFly], ok[kFly];
#pragma unroll
      for (int i = 0; i < kFly; ++i) {
        const int64_t e = e0 + 4 * i;
        const bool in = e < len;
        const int32_t t = ord[in ? e : e0];
        counted[i] = in && t >= 0 && (int64_t)t < T;
        ok[i] = counted[i] && rowok;
        u[i] = 0u;
        if (ok[i]) u[i] = __builtin_bit_cast(uint32_t, xp[(int64_t)t * ldx]);
      }
#pragma unroll
      for (int i = 0; i < kFly; ++i) f(ok[i] ? key_of(u[i]) : kSkipped, counted[i], ok[i] && nan_bits(u[i]));
    }
  }

  // -> the counted members of the slot; sets isnan
  __device__ __forceinline__ int64_t first_pass(bool& isnan) {
    uint32_t st[2] = {0u, 0u}, o[1] = {0u}, a[1] = {0xFFFFFFFFu};
    walk([&](uint32_t key, bool counted, bool nan) {
      st[0] += counted ? 1u : 0u;
      st[1] |= nan ? 1u : 0u;
      o[0] |= key == kSkipped ? 0u : key;
      a[0] &= key;
    });
    meet<2, kAdd>(st);
    meet<1, kOr>(o);
    meet<1, kAnd>(a);
    or_keys = o[0];
    and_keys = a[0];
    isnan = st[1] != 0u;
    return (int64_t)st[0];
  }

  __device__ __forceinline__ void spread(uint32_t (&orv)[1], uint32_t (&andv)[1]) {
    orv[0] = or_keys;
    andv[0] = and_keys;
  }

  __device__ __forceinline__ void count_below(const uint32_t (&cand)[JT][1], uint32_t (&cnt)[JT][1]) {
    uint32_t c[JT];
#pragma unroll
    for (int j = 0; j < JT; ++j) c[j] = 0u;
    walk([&](uint32_t key, bool, bool) {
#pragma unroll
      for (int j = 0; j < JT; ++j) c[j] += key < cand[j][0] ? 1u : 0u;
    });
    meet<JT, kAdd>(c);
#pragma unroll
    for (int j = 0; j < JT; ++j) cnt[j][0] = c[j];
  }

  __device__ __forceinline__ void above(const uint32_t (&x)[1], uint32_t (&cnt)[1], uint32_t (&mn)[1]) {
    cnt[0] = 0u;
    mn[0] = kSkipped;
    walk([&](uint32_t key, bool, bool) {
      const bool le = key <= x[0];
      cnt[0] += le ? 1u : 0u;
      mn[0] = (!le && key < mn[0]) ? key : mn[0];
    });
    meet<1, kAdd>(cnt);
    meet<1, kMin>(mn);
  }
};

template <int JT>
__device__ __forceinline__ void streamed_pass(uint4* tile4, const float* __restrict__ X, int64_t m, int64_t T, int64_t ldx,
                                              const int32_t* __restrict__ ord, int64_t len, const QList& ql, int J,
                                              int method, int64_t r0, int64_t S, int64_t s, float* __restrict__ out,
                                              int64_t ldo) {
  StreamedSrc<JT> src;
  src.sub = threadIdx.x >> 6;
  src.row = threadIdx.x & 63;
  src.rowok = r0 + src.row < m;
  src.xp = X + r0 + src.row;
  src.ord = ord;
  src.part = reinterpret_cast<uint32_t*>(tile4);
  src.len = len;
  src.T = T;
  src.ldx = ldx;
  __syncthreads();                                              // the tile of a staged slot before is done with
  bool isnan[1];
  const int64_t n = src.first_pass(isnan[0]);
  const Rank<JT> rk = rank_of<JT>(ql, method, n);
  uint32_t xlo[JT][1], xhi[JT][1];
  if (n > 0) {
    select_rows<1, JT>(src, rk, xlo, xhi);
  } else {
#pragma unroll
    for (int j = 0; j < JT; ++j) xlo[j][0] = xhi[j][0] = 0u;
  }
  write_rows<1, JT>(out, ldo, S, s, m, r0 + src.row, J, src.sub, n, rk, isnan, xlo, xhi);
}

// grid.x: tiles of 64 rows, grid.y: slots (strided when S > gridDim.y).  No lane leaves early: the reductions through
// the lanes and the barriers take all 256.  Three workgroups per CU by LDS, and the registers are held to that
// (launch bound 3: 168 VGPRs; `make resource-usage` must show no scratch).
template <int JT>
__global__ __launch_bounds__(kThreads, 3) void cquant_kernel(const float* __restrict__ X, int64_t m, int64_t T, int64_t ldx,
                                                          const int32_t* __restrict__ order, int64_t n_order,
                                                          const int32_t* __restrict__ start, int64_t S, QList ql, int J,
                                                          int method, int streamed, float* __restrict__ out,
                                                          int64_t ldo) {
  __shared__ uint4 tile4[kTileDwords / 4];
  __shared__ int nanrow[kTileRows];
  __shared__ int cntv[16];
  const int64_t r0 = (int64_t)blockIdx.x * kTileRows;
  for (int64_t s = blockIdx.y; s < S; s += gridDim.y) {
    int64_t a = start[s], b = start[s + 1];
    a = a < 0 ? 0 : (a > n_order ? n_order : a);
    b = b < a ? a : (b > n_order ? n_order : b);
    const int64_t len = T == 0 ? 0 : b - a;
    const int32_t* ord = order + a;
    if (streamed || len > kMaxStaged) {
      streamed_pass<JT>(tile4, X, m, T, ldx, ord, len, ql, J, method, r0, S, s, out, ldo);
    } else if (len <= kCap64) {
      staged_pass<64, JT>(tile4, nanrow, cntv, X, m, T, ldx, ord, (int)len, ql, J, method, r0, S, s, out, ldo);
    } else if (len <= 2 * kCap64) {
      for (int p = 0; p < 2; ++p)
        if (r0 + 32 * p < m)
          staged_pass<32, JT>(tile4, nanrow, cntv, X, m, T, ldx, ord, (int)len, ql, J, method, r0 + 32 * p, S, s, out, ldo);
    } else {
      for (int p = 0; p < 4; ++p)
        if (r0 + 16 * p < m)
          staged_pass<16, JT>(tile4, nanrow, cntv, X, m, T, ldx, ord, (int)len, ql, J, method, r0 + 16 * p, S, s, out, ldo);
    }
  }
}

}  // namespace

extern "C" int dmdx_clim_quantile_max_q(void) { return DMDX_CLIM_QUANTILE_MAX_Q; }
extern "C" int dmdx_clim_quantile_max_staged(void) { return kMaxStaged; }

extern "C" int dmdx_clim_quantile_f32(const float* X, int64_t m, int64_t T, int64_t ldx, const int32_t* order, int64_t n_order,
                                      const int32_t* start, int64_t S, const double* q, int64_t J, int method, int streamed,
                                      float* out, int64_t ldo, void* stream) {
  DMDX_CHECK_ARG(X && order && start && q && out, "clim_quantile: null pointer");
  DMDX_CHECK_ARG(n_order >= 0 && n_order < kMaxSize, "clim_quantile: n_order=%lld outside 0..2^31-1", (long long)n_order);
  DMDX_CHECK_ARG(S >= 1 && S < kMaxSize, "clim_quantile: S=%lld outside 1..2^31-1", (long long)S);
  DMDX_CHECK_ARG(J >= 1 && J <= DMDX_CLIM_QUANTILE_MAX_Q, "clim_quantile: J=%lld outside 1..%d", (long long)J,
                 DMDX_CLIM_QUANTILE_MAX_Q);
  DMDX_CHECK_ARG(J * S < kMaxSize, "clim_quantile: J S=%lld >= 2^31", (long long)(J * S));
  DMDX_CHECK_ARG(method >= 0 && method <= 2, "clim_quantile: method=%d outside 0..2", method);
  QList ql;
  for (int j = 0; j < DMDX_CLIM_QUANTILE_MAX_Q; ++j) {
    const double v = q[j < J ? j : J - 1];
    DMDX_CHECK_ARG(v >= 0.0 && v <= 1.0, "clim_quantile: q[%d]=%g is not inside [0, 1]", j, v);
    ql.q[j] = v;
  }
  if (int rc = check_block("clim_quantile", m, T, {{"ldx", ldx}, {"ldo", ldo}}, {X, out, order, start})) return rc;
  if (m == 0) return 0;
  const dim3 grid((unsigned)((m + kTileRows - 1) / kTileRows), grid_rows(S));
  if (J == 1)
    hipLaunchKernelGGL(cquant_kernel<1>, grid, dim3(kThreads), 0, (hipStream_t)stream, X, m, T, ldx, order, n_order, start,
                       S, ql, (int)J, method, streamed, out, ldo);
  else
    hipLaunchKernelGGL(cquant_kernel<4>, grid, dim3(kThreads), 0, (hipStream_t)stream, X, m, T, ldx, order, n_order, start,
                       S, ql, (int)J, method, streamed, out, ldo);
  DMDX_LAUNCH_CHECK();
  return 0;
}
