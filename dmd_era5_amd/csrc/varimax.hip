// K30: one step of the orthomax (varimax) iteration over the leading k modes, and the row norms of Kaiser's
// normalisation.  U: m x k (m huge, k <= 64), R: k x k.  With a = U (or fl(U w), w one weight per row) and L = a R,
//
//     G = a^T (L o L o L),   q = colsum(L o L),   f = colsum(L o L o L o L)
//
// in ONE read of U; L is never stored.  The host turns G and q into the next rotation (rotation.py).
//
// Shape.  A unit is a range of at most DMDX_VARIMAX_FP32_ROWS rows; its workgroup (4 waves) deals the 32-row chunks
// of the range round robin, chunk c to wave c % 4, and every wave does both products of its chunks on its own:
//   1. the wave stages its chunk as K13's swizzled LDS image [column][32 rows] (a lane loads 16 bytes = 4 rows of one
//      column and multiplies them by w);
//   2. L = a R as KB = ceil(k / 32) accumulator blocks of v_mfma_f32_32x32x2_f32: A = the image read across its columns
//      (one dword per step, j = 2 s + h in step s of lane half h: j ascending along the chain), B = R, which the lane
//      holds in registers for the whole unit (16 KB^2 of them);
//   3. L is cubed in the accumulator registers: L2 = fl(L L), L3 = fl(L2 L), L4 = fl(L2 L2); L2 and L4 go to per-lane
//      fp32 sums (q, f), L3 to a second LDS image of the same layout -- an accumulator holds 4 consecutive rows of a
//      column per register quad, which is one 16-byte piece of that image;
//   4. G += a^T L3 as KB^2 accumulator blocks, both operands read as K13 reads them (one 16-byte piece per 4 steps).
// The images are private to a wave (16 KB at k > 32, 64 KB per workgroup).  At k > 32 the registers (R 64, G 64, L 32,
// the prefetched chunk 32) leave one wave per SIMD; at k <= 32 three.
//
// Zeros.  Rows past the range or past m and columns past k are exact zeros in a AND in R (w is applied to the columns
// below k only: 0 * Inf in a pad column would put a NaN into every column of L), and L is set to zero for
// the rows past the range before it is cubed: a non-finite R[j, c] meets no pad row and reaches column c alone.
//
// Sums.  fp32 inside a unit: per lane over its chunks, then the lane halves, then the four waves in order; stored
// into the unit's slot [k k (G, column-major) | k (q) | k (f)].  A second kernel adds the slots in fp64, in a fixed order.
// No atomics: the order of every sum depends on (m, k) only.
#include "dmdx_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int BK = 32;      // rows per chunk
constexpr int MAXK = 64;
constexpr int RMAX = DMDX_VARIMAX_FP32_ROWS;
constexpr int RMIN = 256;   // shortest row range of the fill rule
constexpr int FILL = 512;   // units a launch should have at least (2 per CU; 1024 measured 3 to 12 % slower)
static_assert(RMAX % (4 * BK) == 0 && RMIN % (4 * BK) == 0 && RMAX <= 4096, "row ranges are whole rounds of chunks");

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
__global__ __launch_bounds__(256) void varimax_kernel(const float* __restrict__ U, int64_t m, int k, int64_t ldu,
                                                      const float* __restrict__ R, int64_t ldr,
                                                      const float* __restrict__ w, int64_t rpu, int uvec, int wvec,
                                                      float* __restrict__ slots) {
  constexpr int KP = 32 * KB;            // padded k
  constexpr int IMG = KP * BK;           // floats of one image
  constexpr int NP = KP / 8;             // staging passes: 8 columns of the chunk per pass
  static_assert(KP * KP <= 2 * IMG, "a wave's G fits its two images");
  __shared__ __attribute__((aligned(16))) float lds[4 * 2 * IMG];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, h = lane >> 5;
  const int64_t rr = blockIdx.x;
  const int64_t r0 = rr * rpu;
  const int64_t r1 = r0 + rpu < m ? r0 + rpu : m;
  const int nchunks = (int)((r1 - r0 + BK - 1) / BK);
  const int nit = (nchunks + 3) / 4;      // the same for the four waves: their barriers meet
  float* aimg = lds + wave * (2 * IMG);
  float* limg = aimg + IMG;

  // R in B-operand layout: step s of block cb needs R[2 s + h, 32 cb + li]; zero outside k x k, never addressed there
  float rreg[KB][16 * KB];
#pragma unroll
  for (int cb = 0; cb < KB; ++cb)
#pragma unroll
    for (int s = 0; s < 16 * KB; ++s) {
      const int j = 2 * s + h, c = 32 * cb + li;
      rreg[cb][s] = (j < k && c < k) ? R[(int64_t)c * ldr + j] : 0.f;
    }

  // staging: piece sp (rows 4 sp .. 4 sp + 3 of the chunk) of columns 8 pass + (lane >> 3)
  const int sp = lane & 7, sc0 = lane >> 3;
  f32x4 ur[NP], wq;
  auto gload = [&](int it) {
    const int64_t i = r0 + ((int64_t)(4 * it + wave)) * BK + 4 * sp;
#pragma unroll
    for (int ps = 0; ps < NP; ++ps) {
      const int j = sc0 + 8 * ps;
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      ur[ps] = j < k ? load_quad(U + (int64_t)j * ldu + i, i, r1, uvec) : z;
    }
    if (w != nullptr) wq = load_quad(w + i, i, r1, wvec);
  };
  auto lstore = [&]() {
#pragma unroll
    for (int ps = 0; ps < NP; ++ps) {
      f32x4 v = ur[ps];
      const int c = sc0 + 8 * ps;
      if (w != nullptr && c < k) v = v * wq;   // the pad columns stay exact zeros: 0 * Inf would be a NaN in every L
      *reinterpret_cast<f32x4*>(aimg + c * BK + 4 * (sp ^ swz(c))) = v;
    }
  };

  f32x16 gacc[KB][KB];
  float qacc[KB], facc[KB];
#pragma unroll
  for (int jb = 0; jb < KB; ++jb)
#pragma unroll
    for (int cb = 0; cb < KB; ++cb)
#pragma unroll
      for (int r = 0; r < 16; ++r) gacc[jb][cb][r] = 0.f;
#pragma unroll
  for (int cb = 0; cb < KB; ++cb) qacc[cb] = facc[cb] = 0.f;

  // The barriers of the loop are workgroup barriers, stronger than needed: both images are private to a wave, so
  // ordering within the wave would do.  They keep the four waves in step, which is why every wave runs nit rounds
  // and a round past the range stages zeros.
  if (nit > 0) gload(0);
  for (int it = 0; it < nit; ++it) {
    lstore();
    if (it + 1 < nit) gload(it + 1);
    __syncthreads();

    // L = a R: step s of lane half h contracts column j = 2 s + h; A = a[row li, j], B = R[j, column li of the block]
    f32x16 lacc[KB];
#pragma unroll
    for (int cb = 0; cb < KB; ++cb)
#pragma unroll
      for (int r = 0; r < 16; ++r) lacc[cb][r] = 0.f;
#pragma unroll
    for (int s = 0; s < 16 * KB; ++s) {
      const int j = 2 * s + h;
      const float av = aimg[j * BK + 4 * ((li >> 2) ^ swz(j)) + (li & 3)];
#pragma unroll
      for (int cb = 0; cb < KB; ++cb) lacc[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, rreg[cb][s], lacc[cb], 0, 0, 0);
    }

    // register r = 4 g + e of a lane holds row 8 g + 4 h + e of column 32 cb + li: piece 2 g + h of that column
    const int64_t left = r1 - (r0 + ((int64_t)(4 * it + wave)) * BK);
    const int nvalid = left < 0 ? 0 : (left > BK ? BK : (int)left);
#pragma unroll
    for (int cb = 0; cb < KB; ++cb) {
      const int c = 32 * cb + li;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 l3;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float l = (8 * g + 4 * h + e) < nvalid ? lacc[cb][4 * g + e] : 0.f;
          const float l2 = l * l;
          l3[e] = l2 * l;
          qacc[cb] = qacc[cb] + l2;
          facc[cb] = facc[cb] + l2 * l2;
        }
        *reinterpret_cast<f32x4*>(limg + c * BK + 4 * ((2 * g + h) ^ swz(c))) = l3;
      }
    }
    __syncthreads();

    // G += a^T L3: MFMA step 4 p + e of lane half h contracts row 8 p + 4 h + e of the chunk, piece 2 p + h of the
    // lane's column in both images; A = a (j on the registers of D), B = L3 (c on its lanes)
    const int sw = swz(li);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int po = 4 * ((2 * p + h) ^ sw);
      f32x4 b[KB];
#pragma unroll
      for (int cb = 0; cb < KB; ++cb) b[cb] = *reinterpret_cast<const f32x4*>(limg + (32 * cb + li) * BK + po);
#pragma unroll
      for (int jb = 0; jb < KB; ++jb) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(aimg + (32 * jb + li) * BK + po);
#pragma unroll
        for (int cb = 0; cb < KB; ++cb)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            gacc[jb][cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], b[cb][e], gacc[jb][cb], 0, 0, 0);
      }
    }
    __syncthreads();   // the images are free for the next chunk
  }

  // the four waves meet in LDS: every wave lays its G down as [j][c ^ (j & 31)] over its own images, then the
  // workgroup adds wave 0 .. 3 in order and stores the unit's slot
  float* slot = slots + rr * ((int64_t)k * k + 2 * k);
  {
    float* gd = lds + wave * (2 * IMG);
#pragma unroll
    for (int jb = 0; jb < KB; ++jb)
#pragma unroll
      for (int cb = 0; cb < KB; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int j = 32 * jb + (r & 3) + 8 * (r >> 2) + 4 * h;
          gd[j * KP + 32 * cb + (li ^ (j & 31))] = gacc[jb][cb][r];
        }
  }
  __syncthreads();
  for (int e = tid; e < k * k; e += 256) {
    const int c = e / k, j = e - c * k;
    const int at = j * KP + (c & 32) + ((c & 31) ^ (j & 31));
    float s = lds[at];
#pragma unroll
    for (int v = 1; v < 4; ++v) s = s + lds[v * (2 * IMG) + at];
    slot[e] = s;
  }
  __syncthreads();
#pragma unroll
  for (int cb = 0; cb < KB; ++cb) {
    const float qs = qacc[cb] + __shfl_xor(qacc[cb], 32, 64);
    const float fs = facc[cb] + __shfl_xor(facc[cb], 32, 64);
    if (h == 0) {
      lds[wave * (2 * KP) + 32 * cb + li] = qs;
      lds[wave * (2 * KP) + KP + 32 * cb + li] = fs;
    }
  }
  __syncthreads();
  if (tid < 2 * KP) {
    const int c = tid & (KP - 1), which = tid / KP;   // 0: q, 1: f
    float s = lds[tid];
#pragma unroll
    for (int v = 1; v < 4; ++v) s = s + lds[v * (2 * KP) + tid];
    if (c < k) slot[(int64_t)k * k + which * k + c] = s;
  }
}

// G[j, c] (+)= sum over the units of their slots, q and f alike, in fp64 and in a fixed order: a workgroup owns 32
// elements, its 8 half waves take 8 consecutive runs of units (each added in order, 16 loads in flight: a single
// lane walking all units waits for memory ~nsplit / 8 times), and the runs are added in order
constexpr int RSEG = 8;
__global__ __launch_bounds__(256) void varimax_reduce_kernel(const float* __restrict__ slots, int64_t nsplit, int k,
                                                             double* __restrict__ G, int64_t ldg, double* __restrict__ q,
                                                             double* __restrict__ f, int accumulate) {
  __shared__ double part[RSEG][32];
  const int per = k * k + 2 * k;
  const int el = threadIdx.x & 31, seg = threadIdx.x >> 5;
  const int e = blockIdx.x * 32 + el;
  const int64_t len = (nsplit + RSEG - 1) / RSEG;
  const int64_t a = seg * len, b = a + len < nsplit ? a + len : nsplit;
  double s = 0.0;
  if (e < per) {
    const float* p = slots + e;
#pragma unroll 16
    for (int64_t rr = a; rr < b; ++rr) s += (double)p[rr * per];
  }
  part[seg][el] = s;
  __syncthreads();
  if (seg != 0 || e >= per) return;
#pragma unroll
  for (int v = 1; v < RSEG; ++v) s += part[v][el];
  double* dst;
  if (e < k * k) {
    const int c = e / k, j = e - c * k;
    dst = G + (int64_t)c * ldg + j;
  } else if (e < k * k + k) {
    dst = q + (e - k * k);
  } else {
    if (f == nullptr) return;
    dst = f + (e - k * k - k);
  }
  *dst = accumulate ? *dst + s : s;
}

// h[i] = fp32(sqrt(sum_j fp64(fl(U[i, j] cscale[j]))^2)), j ascending, squares rounded before they are added; a lane
// per row (R = 4: a quad of rows, 16-byte loads)
template <int R>
__global__ __launch_bounds__(256) void row_norms_kernel(const float* __restrict__ U, int64_t m, int k, int64_t ldu,
                                                        const float* __restrict__ cscale, float* __restrict__ hout) {
  typedef float vec __attribute__((ext_vector_type(R)));
  const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * R;
  if (i0 >= m) return;
  const int nr = (m - i0) < R ? (int)(m - i0) : R;
  double acc[R];
#pragma unroll
  for (int e = 0; e < R; ++e) acc[e] = 0.0;
  if (nr == R) {
#pragma unroll 4
    for (int j = 0; j < k; ++j) {
      const vec v = *reinterpret_cast<const vec*>(U + (int64_t)j * ldu + i0);
      const float cs = cscale != nullptr ? cscale[j] : 1.f;
#pragma unroll
      for (int e = 0; e < R; ++e) {
        const double d = (double)(cscale != nullptr ? v[e] * cs : v[e]);
        const double d2 = d * d;
        acc[e] = acc[e] + d2;
      }
    }
  } else {
    for (int j = 0; j < k; ++j) {
      const float cs = cscale != nullptr ? cscale[j] : 1.f;
      for (int e = 0; e < nr; ++e) {
        const float x = U[(int64_t)j * ldu + i0 + e];
        const double d = (double)(cscale != nullptr ? x * cs : x);
        const double d2 = d * d;
        acc[e] = acc[e] + d2;
      }
    }
  }
  for (int e = 0; e < nr; ++e) hout[i0 + e] = (float)__builtin_sqrt(acc[e]);
}

// the row range is shortened until the launch has ~FILL units; a function of m only, so that the partial sums --
// and with them the results -- do not depend on the device
struct Plan {
  int64_t rpu, nsplit;
};
Plan plan_for(int64_t m) {
  Plan p;
  int64_t rpu = ((m + FILL - 1) / FILL + 4 * BK - 1) / (4 * BK) * (4 * BK);
  if (rpu < RMIN) rpu = RMIN;
  if (rpu > RMAX) rpu = RMAX;
  p.rpu = rpu;
  p.nsplit = (m + rpu - 1) / rpu;
  return p;
}
// the units of any m' <= m never outnumber this: non-decreasing in m, where plan_for(m).nsplit steps down whenever
// the range grows by a round of chunks
int64_t max_units(int64_t m) {
  if (m <= (int64_t)FILL * RMIN) return (m + RMIN - 1) / RMIN;
  const int64_t long_ranges = (m + RMAX - 1) / RMAX;
  return long_ranges > FILL ? long_ranges : FILL;
}

inline size_t align16(size_t n) { return (n + 15) & ~size_t(15); }

}  // namespace

extern "C" int dmdx_varimax_max_k(void) { return MAXK; }

// [<= 15 bytes to a 16-byte boundary][slots: units x (k k + 2 k) fp32]
extern "C" size_t dmdx_varimax_workspace_bytes(int64_t m, int64_t k) {
  if (m < 1 || k < 1 || k > MAXK || m >= kMaxSize) return 16;
  return 16 + align16((size_t)max_units(m) * (size_t)(k * k + 2 * k) * sizeof(float));
}

extern "C" int dmdx_varimax_step_f32(const float* U, int64_t m, int64_t k, int64_t ldu, const float* R, int64_t ldr,
                                     const float* w, double* G, int64_t ldg, double* q, double* f, int accumulate,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "dmdx_varimax_step_f32";
  DMDX_CHECK_ARG(U != nullptr && R != nullptr && G != nullptr && q != nullptr, "%s: U, R, G and q must not be null", who);
  DMDX_CHECK_ARG(m >= 1, "%s: m = %lld must be >= 1", who, (long long)m);
  DMDX_CHECK_ARG(k >= 1 && k <= MAXK, "%s: k = %lld outside 1 .. %d", who, (long long)k, MAXK);
  DMDX_CHECK_ARG(ldu >= m && ldr >= k && ldg >= k, "%s: ldu = %lld < m = %lld, ldr = %lld or ldg = %lld < k = %lld", who,
                 (long long)ldu, (long long)m, (long long)ldr, (long long)ldg, (long long)k);
  DMDX_CHECK_ARG(m < kMaxSize && ldu < kMaxSize && ldr < kMaxSize && ldg < kMaxSize, "%s: m, ldu, ldr, ldg must be < 2^31",
                 who);
  const Plan p = plan_for(m);
  const size_t need = dmdx_varimax_workspace_bytes(m, k);
  if (workspace == nullptr || workspace_bytes < need) {
    dmdx_set_error("%s: varimax workspace of %zu bytes, %zu needed", who, workspace == nullptr ? (size_t)0 : workspace_bytes,
                   need);
    return DMDX_E_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  float* slots = reinterpret_cast<float*>(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
  const int uvec = dmdx_aligned16(U) && ldu % 4 == 0, wvec = dmdx_aligned16(w);
  const dim3 grid((unsigned)p.nsplit);
  if (k <= 32)
    hipLaunchKernelGGL((varimax_kernel<1>), grid, dim3(256), 0, st, U, m, (int)k, ldu, R, ldr, w, p.rpu, uvec, wvec, slots);
  else
    hipLaunchKernelGGL((varimax_kernel<2>), grid, dim3(256), 0, st, U, m, (int)k, ldu, R, ldr, w, p.rpu, uvec, wvec, slots);
  DMDX_LAUNCH_CHECK();
  const int per = (int)(k * k + 2 * k);
  hipLaunchKernelGGL(varimax_reduce_kernel, dim3((unsigned)((per + 31) / 32)), dim3(256), 0, st, slots, p.nsplit, (int)k, G,
                     ldg, q, f, accumulate);
  DMDX_LAUNCH_CHECK();
  return 0;
}

extern "C" int dmdx_row_norms_f32(const float* U, int64_t m, int64_t k, int64_t ldu, const float* cscale, float* h,
                                  void* stream) {
  const char* who = "dmdx_row_norms_f32";
  DMDX_CHECK_ARG(U != nullptr && h != nullptr, "%s: U and h must not be null", who);
  DMDX_CHECK_ARG(m >= 1 && k >= 1, "%s: m = %lld, k = %lld must be >= 1", who, (long long)m, (long long)k);
  DMDX_CHECK_ARG(ldu >= m, "%s: ldu = %lld < m = %lld", who, (long long)ldu, (long long)m);
  DMDX_CHECK_ARG(m < kMaxSize && k < kMaxSize && ldu < kMaxSize, "%s: m, k, ldu must be < 2^31", who);
  hipStream_t st = (hipStream_t)stream;
  if (dmdx_aligned16(U) && ldu % 4 == 0 && dmdx_aligned16(h)) {
    hipLaunchKernelGGL((row_norms_kernel<4>), dim3((unsigned)((m + 1023) / 1024)), dim3(256), 0, st, U, m, (int)k, ldu, cscale, h);
  } else {
    hipLaunchKernelGGL((row_norms_kernel<1>), dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, U, m, (int)k, ldu, cscale, h);
  }
  DMDX_LAUNCH_CHECK();
  return 0;
}
