// K13: coefficients of raw snapshots in the basis U, C = U^T xt with xt = (X - mu) / sigma formed on the fly, and
// the energy sum_i xt^2 of every snapshot.  U: m x k (m huge, k <= 256), X: m x T, C: k x T fp64.  K12's twin: the
// same operands and layouts, the other direction.
//
// Shape.  K3's: D = OpA^T OpB with both operands contiguous along the contraction (the space index i), A = U,
// B = xt.  A unit is (a range of at most DMDX_PROJECT_FP32_ROWS rows, a tile of 128 snapshots).  Its workgroup
// (4 waves) puts the waves side by side along T: wave w owns snapshots 32 w .. 32 w + 31 of the tile and ALL of
// k, as KB = ceil(k / 32) blocks of v_mfma_f32_32x32x2_f32 accumulators (k = 256: 128 registers), so one pass
// over X serves every k.  The rows run in chunks of 32 through LDS images [column][32 rows] (128 B per column,
// K3's XOR swizzle of the 16-byte row piece with (column >> 1) & 7: conflict-free ds_read_b128 fragments).
//
// Staging.  Both operands go through registers: a lane loads 16 bytes = 4 rows of one column (8 lanes = one
// 128-byte line of a column).  X cannot go by LDS-DMA, it is transformed in flight: the lane's mu / sigma quad is
// loaded with it, xt = fl(fl(x - mu) / sigma) is exactly what K5 leaves in place (one subtraction, one correctly
// rounded division), xt^2 goes to a per-lane fp32 energy accumulator and xt to LDS.  A wave stages the columns it
// consumes itself.  The chunk c + 1 is loaded from global memory before the MFMAs of chunk c and stored behind
// them: into the other stage up to k = 128 (one barrier per chunk), into the same stage beyond (two barriers,
// half the LDS: two to three workgroups per CU hide each other's staging).
//
// Zeros.  Rows past the unit's range or past m, snapshots past T and columns of U past k are exact zeros on
// BOTH sides (0 * 0, never a clamped duplicate): an Inf meets no pad.  For such rows mu = 0 and sigma = 1.
//
// Sums.  One fp32 MFMA chain per unit and element of C (at most DMDX_PROJECT_FP32_ROWS rows), stored as it is
// into the unit's slot part[row range][k][T]; the energy of a snapshot is the fp32 sum of the 8 lanes that
// staged it, slot epart[row range][T].  A second kernel adds the row ranges in fp64, in order.  No atomics:
// the order of every sum depends on (m, k, T) only.
#include "dmdx_common.h"

namespace {

constexpr int TT = 128;     // snapshots per unit (4 waves x 32)
constexpr int BK = 32;      // rows per chunk
constexpr int MAXK = 256;
constexpr int RMAX = DMDX_PROJECT_FP32_ROWS;
constexpr int RMIN = 256;   // shortest row range of the fill rule
constexpr int FILL = 1024;  // units a launch should have at least (4 per CU)
static_assert(RMAX % BK == 0 && RMIN % BK == 0 && RMAX <= 4096, "row ranges are whole chunks; K1's fp32 bound");

__device__ __forceinline__ int swz(int col) { return (col >> 1) & 7; }

// rows i .. i + 3 of one column (p points at row i); rows >= iend are exact zeros and never addressed
__device__ __forceinline__ f32x4 load_quad(const float* p, int64_t i, int64_t iend, int vec) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (vec && i + 4 <= iend) {
    v = *reinterpret_cast<const f32x4*>(p);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (i + e < iend) v[e] = p[e];
  }
  return v;
}

template <int KB>
__global__ __launch_bounds__(256) void project_kernel(const float* __restrict__ U, int64_t m, int k, int64_t ldu,
                                                      const float* __restrict__ X, int64_t ldx, int64_t T,
                                                      const float* __restrict__ mu, const float* __restrict__ sigma,
                                                      int64_t rpu, int64_t ntiles, int uvec, int xvec, int mvec, int svec,
                                                      float* __restrict__ part, float* __restrict__ epart,
                                                      unsigned long long* clk) {
  constexpr int KP = 32 * KB;               // padded k
  constexpr int NST = KB <= 4 ? 2 : 1;      // LDS stages
  constexpr int STG = (KP + TT) * BK;       // floats per stage: U image [KP][32], then X image [128][32]
  __shared__ __attribute__((aligned(16))) float lds[NST * STG];

  unsigned long long pc0 = 0, pr0 = 0;   // measurement aid (dmdx_set_clock_probe; null on the product path)
  if (clk != nullptr) {
    pc0 = __builtin_amdgcn_s_memtime();
    pr0 = __builtin_amdgcn_s_memrealtime();
  }

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, h = lane >> 5;
  // units are numbered T-tile-fastest: the workgroups that share a U panel run together
  const int64_t tile = (int64_t)blockIdx.x % ntiles, rr = (int64_t)blockIdx.x / ntiles;
  const int64_t t0 = tile * TT, r0 = rr * rpu;
  const int64_t r1 = r0 + rpu < m ? r0 + rpu : m;
  const int nchunks = (int)((r1 - r0 + BK - 1) / BK);

  // staging: piece sp (rows 4 sp .. 4 sp + 3 of the chunk) of X columns 32 wave + 8 pass + (lane >> 3) and of
  // U columns 32 pass + (tid >> 3)
  const int sp = lane & 7;
  const int xc0 = 32 * wave + (lane >> 3), uc0 = tid >> 3;
  const float* xp[4];
  bool xok[4];
#pragma unroll
  for (int ps = 0; ps < 4; ++ps) {
    const int64_t t = t0 + xc0 + 8 * ps;
    xok[ps] = t < T;
    xp[ps] = X + (xok[ps] ? t : 0) * ldx;
  }

  f32x4 xr[4], ur[KB], mq, sq;
  auto gload = [&](int c) {
    const int64_t i = r0 + (int64_t)c * BK + 4 * sp;
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      xr[ps] = xok[ps] ? load_quad(xp[ps] + i, i, r1, xvec) : z;
    }
#pragma unroll
    for (int ps = 0; ps < KB; ++ps) {
      const int j = uc0 + 32 * ps;
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      ur[ps] = j < k ? load_quad(U + (int64_t)j * ldu + i, i, r1, uvec) : z;
    }
    if (mu != nullptr) mq = load_quad(mu + i, i, r1, mvec);
    if (sigma != nullptr) {
      sq = load_quad(sigma + i, i, r1, svec);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (i + e >= r1) sq[e] = 1.f;
    }
  };

  float eacc[4] = {0.f, 0.f, 0.f, 0.f};
  auto lstore = [&](int st) {
    float* us = lds + st * STG;
    float* xs = us + KP * BK;
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
      f32x4 v = xr[ps];
      if (mu != nullptr) v = v - mq;
      if (sigma != nullptr) v = v / sq;
      if (!xok[ps]) v = f32x4{0.f, 0.f, 0.f, 0.f};
      eacc[ps] += ((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + v[3] * v[3];
      const int c = xc0 + 8 * ps;
      *reinterpret_cast<f32x4*>(xs + c * BK + 4 * (sp ^ swz(c))) = v;
    }
#pragma unroll
    for (int ps = 0; ps < KB; ++ps) {
      const int c = uc0 + 32 * ps;
      *reinterpret_cast<f32x4*>(us + c * BK + 4 * (sp ^ swz(c))) = ur[ps];
    }
  };

  f32x16 acc[KB];
#pragma unroll
  for (int b = 0; b < KB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;

  gload(0);
  lstore(0);
  __syncthreads();
  int cur = 0;
  for (int c = 0; c < nchunks; ++c) {
    const bool has_next = c + 1 < nchunks;
    if (has_next) gload(c + 1);

    // MFMA step 4 q + e of lane half h contracts row 8 q + 4 h + e of the chunk: piece 2 q + h of the lane's
    // column, one 16-byte read per operand; A = U (j on the registers of D), B = xt (t on its lanes)
    const float* us = lds + cur * STG;
    const float* xs = us + KP * BK + (32 * wave + li) * BK;
    const int sw = swz(li);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int po = 4 * ((2 * q + h) ^ sw);
      const f32x4 b = *reinterpret_cast<const f32x4*>(xs + po);
#pragma unroll
      for (int jb = 0; jb < KB; ++jb) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(us + (32 * jb + li) * BK + po);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[jb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], b[e], acc[jb], 0, 0, 0);
      }
    }

    if (NST == 1) __syncthreads();   // every wave is done with the one stage
    if (has_next) lstore(NST == 1 ? 0 : cur ^ 1);
    __syncthreads();
    if (NST == 2) cur ^= 1;
  }

  // the unit's slots: part[rr][j][t], epart[rr][t]
  {
    const int64_t t = t0 + 32 * wave + li;
    if (t < T) {
#pragma unroll
      for (int jb = 0; jb < KB; ++jb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int j = 32 * jb + (r & 3) + 8 * (r >> 2) + 4 * h;
          if (j < k) part[(rr * k + j) * T + t] = acc[jb][r];
        }
    }
  }
  if (epart != nullptr) {
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
      float s = eacc[ps];
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      s += __shfl_xor(s, 4, 64);
      if (sp == 0 && xok[ps]) epart[rr * T + t0 + xc0 + 8 * ps] = s;
    }
  }
  if (clk != nullptr) {
    const unsigned long long pc1 = __builtin_amdgcn_s_memtime(), pr1 = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0) {
      atomicAdd(&clk[0], pc1 - pc0);
      atomicAdd(&clk[1], pr1 - pr0);
      atomicAdd(&clk[2], 1ull);
    }
  }
}

// C[j, t] (+)= sum over the row ranges of part[rr][j][t], energy[t] (+)= sum of epart[rr][t], in fp64 and in
// order.  Workgroup (x, y): snapshots 32 x .., y < jblocks: columns 8 y .. 8 y + 7 of U, one element per thread
// (read t-fastest, turned in LDS, written j-fastest); y == jblocks: the energy.
__global__ __launch_bounds__(256) void project_reduce_kernel(const float* __restrict__ part, const float* __restrict__ epart,
                                                             int64_t nsplit, int k, int64_t T, int jblocks,
                                                             double* __restrict__ C, int64_t ldc, double* __restrict__ energy,
                                                             int accumulate) {
  __shared__ double tile[8][33];
  const int a = threadIdx.x & 31, b = threadIdx.x >> 5;
  const int64_t t0 = (int64_t)blockIdx.x * 32;
  if ((int)blockIdx.y == jblocks) {
    const int64_t t = t0 + a;
    if (b != 0 || t >= T) return;
    double s = 0.0;
#pragma unroll 8
    for (int64_t rr = 0; rr < nsplit; ++rr) s += (double)epart[rr * T + t];
    energy[t] = accumulate ? energy[t] + s : s;
    return;
  }
  const int j0 = 8 * (int)blockIdx.y;
  {
    const int j = j0 + b;
    const int64_t t = t0 + a;
    double s = 0.0;
    if (j < k && t < T) {
      const float* p = part + (int64_t)j * T + t;
      const int64_t step = (int64_t)k * T;
#pragma unroll 8
      for (int64_t rr = 0; rr < nsplit; ++rr) s += (double)p[rr * step];
    }
    tile[b][a] = s;
  }
  __syncthreads();
  {
    const int j = j0 + (threadIdx.x & 7);
    const int64_t t = t0 + (threadIdx.x >> 3);
    if (j < k && t < T) {
      double* c = C + t * ldc + j;
      const double s = tile[threadIdx.x & 7][threadIdx.x >> 3];
      *c = accumulate ? *c + s : s;
    }
  }
}

// the row range is shortened until the launch has ~FILL units; a function of the shapes only, so that the
// partial sums -- and with them the results -- do not depend on the device
struct Plan {
  int64_t ntiles, rpu, nsplit;
};
Plan plan_for(int64_t m, int64_t T) {
  Plan p;
  p.ntiles = (T + TT - 1) / TT;
  const int64_t want = p.ntiles >= FILL ? 1 : (FILL + p.ntiles - 1) / p.ntiles;
  int64_t rpu = ((m + want - 1) / want + BK - 1) / BK * BK;
  if (rpu < RMIN) rpu = RMIN;
  if (rpu > RMAX) rpu = RMAX;
  p.rpu = rpu;
  p.nsplit = (m + rpu - 1) / rpu;
  return p;
}

constexpr int64_t DIM_LIMIT = int64_t(1) << 31;
constexpr int64_t UNIT_LIMIT = int64_t(1) << 24;   // 256 threads each: the launch stays below 2^32 threads

inline size_t align16(size_t n) { return (n + 15) & ~size_t(15); }

}  // namespace

extern "C" int dmdx_project_max_k(void) { return MAXK; }

// [<= 15 bytes to a 16-byte boundary][part: row ranges x k x T fp32][epart: row ranges x T fp32]
extern "C" size_t dmdx_project_workspace_bytes(int64_t m, int64_t k, int64_t T) {
  if (m < 1 || T < 1 || k < 1) return 16;
  const Plan p = plan_for(m, T);
  return 16 + align16((size_t)p.nsplit * (size_t)k * (size_t)T * sizeof(float)) + (size_t)p.nsplit * (size_t)T * sizeof(float);
}

extern "C" int dmdx_project_f32(const float* U, int64_t m, int64_t k, int64_t ldu, const float* X, int64_t ldx, int64_t T,
                                const float* mu, const float* sigma, double* C, int64_t ldc, double* energy, int accumulate,
                                void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "dmdx_project_f32";
  DMDX_CHECK_ARG(U != nullptr && X != nullptr && C != nullptr, "%s: U, X and C must not be null", who);
  DMDX_CHECK_ARG(m >= 1 && T >= 1, "%s: m = %lld, T = %lld must be >= 1", who, (long long)m, (long long)T);
  DMDX_CHECK_ARG(k >= 1 && k <= MAXK, "%s: k = %lld outside 1 .. %d", who, (long long)k, MAXK);
  DMDX_CHECK_ARG(ldu >= m && ldc >= k && ldx >= 1, "%s: ldu = %lld < m = %lld, ldc = %lld < k = %lld or ldx = %lld < 1", who,
                 (long long)ldu, (long long)m, (long long)ldc, (long long)k, (long long)ldx);
  DMDX_CHECK_ARG(m < DIM_LIMIT && T < DIM_LIMIT && ldu < DIM_LIMIT && ldx < DIM_LIMIT && ldc < DIM_LIMIT,
                 "%s: m, T, ldu, ldx, ldc must be < 2^31", who);
  const Plan p = plan_for(m, T);
  if (p.nsplit * p.ntiles >= UNIT_LIMIT) {
    dmdx_set_error("%s: project of %lld x %lld needs %lld units, at most %lld per call: pass row blocks", who, (long long)m,
                   (long long)T, (long long)(p.nsplit * p.ntiles), (long long)UNIT_LIMIT - 1);
    return DMDX_E_UNSUPPORTED;
  }
  const size_t need = dmdx_project_workspace_bytes(m, k, T);
  if (workspace == nullptr || workspace_bytes < need) {
    dmdx_set_error("%s: project workspace of %zu bytes, %zu needed", who, workspace == nullptr ? (size_t)0 : workspace_bytes, need);
    return DMDX_E_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  char* base = reinterpret_cast<char*>(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
  float* part = reinterpret_cast<float*>(base);
  float* epart = reinterpret_cast<float*>(base + align16((size_t)p.nsplit * (size_t)k * (size_t)T * sizeof(float)));
  const int uvec = dmdx_aligned16(U) && ldu % 4 == 0, xvec = dmdx_aligned16(X) && ldx % 4 == 0;
  const int mvec = dmdx_aligned16(mu), svec = dmdx_aligned16(sigma);
  const dim3 grid((unsigned)(p.nsplit * p.ntiles));
  switch ((k + 31) / 32) {
#define DMDX_CASE(KB)                                                                                                  \
  case KB:                                                                                                             \
    hipLaunchKernelGGL((project_kernel<KB>), grid, dim3(256), 0, st, U, m, (int)k, ldu, X, ldx, T, mu, sigma, p.rpu,     \
                       p.ntiles, uvec, xvec, mvec, svec, part, energy != nullptr ? epart : nullptr, dmdx_clock_probe_ptr); \
    break
    DMDX_CASE(1); DMDX_CASE(2); DMDX_CASE(3); DMDX_CASE(4); DMDX_CASE(5); DMDX_CASE(6); DMDX_CASE(7); DMDX_CASE(8);
#undef DMDX_CASE
    default:
      dmdx_set_error("%s: project: unsupported k %lld", who, (long long)k);
      return DMDX_E_INVALID;
  }
  DMDX_LAUNCH_CHECK();
  const int jblocks = (int)((k + 7) / 8);
  hipLaunchKernelGGL(project_reduce_kernel, dim3((unsigned)((T + 31) / 32), (unsigned)(jblocks + (energy != nullptr ? 1 : 0))),
                     dim3(256), 0, st, part, epart, p.nsplit, (int)k, T, jblocks, C, ldc, energy, accumulate);
  DMDX_LAUNCH_CHECK();
  return 0;
}
