// K17: fields -> CF-packed int16 codes on the device, the inverse of K14 (unpack.hip), and the value range a
// packing is chosen from.  Two pairs of entry points:
//   dmdx_expand_range_f32 / dmdx_expand_pack_i16   Xhat = mu + sigma .* (U C) formed as K12 forms it and never stored:
//                                                  one more body on K12's shape (expand_tile.h, which see for the
//                                                  tile, the MFMA orientation and the k order; verify.hip is the
//                                                  sibling this one was written after)
//   dmdx_range_f32 / dmdx_pack_f32_i16             the same two epilogues on a field that exists: streaming kernels
//
// Arithmetic of a code (labeled.Packing.encode, tests/pack_ref.py):
//   non-finite x -> -32768 (the fill code), counted as filled
//   r = rint((fp64(x) - add_offset) / scale_factor)     an fp64 subtract, an IEEE fp64 divide, round half to even
//   r clamped to [-32767, 32767], an element that needed the clamp counted as saturated
// No reciprocal and no FMA: contraction is off for the file.  xhat is K12's bit for bit: the chain and the two
// operations of sigma * acc + mu are expand_tile.h's.
//
// Range.  min / max of the finite values and the number of non-finite ones: per lane over its tiles, over the wave by
// shuffles, over the workgroup through LDS, one slot per workgroup in the workspace, a one-workgroup reduce kernel.
// min and max do not round and an integer sum has no order: no atomics, the result depends on the values only.
// Counts of the pack kernels ACCUMULATE with one vector atomicAdd per workgroup and counter, as K14's fill count.
#include "expand_tile.h"

#pragma clang fp contract(off)

namespace {

constexpr int FILL = -32768;
constexpr int QMAX = 32767;
constexpr unsigned kPosInf = 0x7F800000u, kNegInf = 0xFF800000u;

__device__ __forceinline__ bool finite_f32(float v) { return (__builtin_bit_cast(unsigned, v) & kPosInf) != kPosInf; }

struct Tally {
  float mn, mx;          // range mode: of the finite values
  unsigned a, b;         // range mode: a = non-finite; pack mode: a = filled, b = saturated
};

__device__ __forceinline__ void tally_init(Tally& s) {
  s.mn = __builtin_bit_cast(float, kPosInf);
  s.mx = __builtin_bit_cast(float, kNegInf);
  s.a = 0u;
  s.b = 0u;
}

__device__ __forceinline__ void range_one(Tally& s, float v) {
  const bool fin = finite_f32(v);
  s.mn = (fin && v < s.mn) ? v : s.mn;
  s.mx = (fin && v > s.mx) ? v : s.mx;
  s.a += fin ? 0u : 1u;
}

__device__ __forceinline__ int16_t encode_one(Tally& s, float v, double sf, double ao) {
  const bool fin = finite_f32(v);
  const double d = (double)v - ao;
  const double q = d / sf;
  const double r = __builtin_rint(q);
  const bool lo = r < -(double)QMAX, hi = r > (double)QMAX;
  const double c = lo ? -(double)QMAX : hi ? (double)QMAX : r;
  s.a += fin ? 0u : 1u;
  s.b += (fin && (lo || hi)) ? 1u : 0u;
  return (int16_t)(fin ? (int)c : FILL);   // (c is finite: r is +-Inf at most, and clamped)
}

// the workgroup's tallies into lane 0 of wave 0: shuffles over the wave, 4 LDS slots over the waves
__device__ __forceinline__ void tally_workgroup(Tally& s, float* lds_f, unsigned* lds_u) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float omn = __shfl_xor(s.mn, off, 64), omx = __shfl_xor(s.mx, off, 64);
    s.mn = omn < s.mn ? omn : s.mn;
    s.mx = omx > s.mx ? omx : s.mx;
    s.a += __shfl_xor(s.a, off, 64);
    s.b += __shfl_xor(s.b, off, 64);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    lds_f[2 * wave] = s.mn;
    lds_f[2 * wave + 1] = s.mx;
    lds_u[2 * wave] = s.a;
    lds_u[2 * wave + 1] = s.b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      s.mn = lds_f[2 * w] < s.mn ? lds_f[2 * w] : s.mn;
      s.mx = lds_f[2 * w + 1] > s.mx ? lds_f[2 * w + 1] : s.mx;
      s.a += lds_u[2 * w];
      s.b += lds_u[2 * w + 1];
    }
  }
}

// the end of every kernel of the file (uniform: every lane gets here)
template <bool PACK>
__device__ __forceinline__ void finish(Tally& s, float* __restrict__ minmax, unsigned long long* __restrict__ nonfin,
                                       unsigned long long* __restrict__ counts) {
  __shared__ float lds_f[8];
  __shared__ unsigned lds_u[8];
  if (PACK && counts == nullptr) return;
  tally_workgroup(s, lds_f, lds_u);
  if (threadIdx.x != 0) return;
  if constexpr (PACK) {
    if (s.a) atomicAdd(&counts[0], (unsigned long long)s.a);
    if (s.b) atomicAdd(&counts[1], (unsigned long long)s.b);
  } else {
    const int64_t wg = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    minmax[2 * wg] = s.mn;
    minmax[2 * wg + 1] = s.mx;
    nonfin[wg] = s.a;
  }
}

// The second __launch_bounds__ argument is WAVES PER SIMD, as in expand.hip: 2 keeps the body within 256 registers
// per lane, i.e. two 4-wave workgroups per CU (MEASUREMENTS.md, K17, has the table per KG).
template <int KG, bool PACK>
__global__ __launch_bounds__(256, 2) void expand_pack_kernel(
    const float* __restrict__ U, int64_t m, int k, int64_t ldu, const float* __restrict__ C, int64_t ldc, int64_t T,
    const float* __restrict__ mu, const float* __restrict__ sigma, double sf, double ao, int16_t* __restrict__ Q,
    int64_t ldq, int64_t tiles_per_wg, int64_t ntiles, int cvec, float* __restrict__ minmax,
    unsigned long long* __restrict__ nonfin, unsigned long long* __restrict__ counts) {
  __shared__ __attribute__((aligned(16))) float ctile[2][Geom<KG>::STAGE];

  const Lane L = lane_of(m);
  float ureg[8 * KG];
  load_panel<KG>(ureg, U, ldu, k, L);
  const float mu_i = (mu != nullptr && L.rowok) ? mu[L.row] : 0.f;
  const float sg_i = (sigma != nullptr && L.rowok) ? sigma[L.row] : 1.f;

  const int64_t tile0 = (int64_t)blockIdx.y * tiles_per_wg;
  const int64_t tile1 = tile0 + tiles_per_wg < ntiles ? tile0 + tiles_per_wg : ntiles;
  Tally tally;
  tally_init(tally);

  Stager<KG> cs;
  cs.load(C, ldc, 0, tile0 * TT, T, k, cvec, L.tid);
  cs.store(ctile[0], L.tid);
  __syncthreads();
  int cur = 0;
  for (int64_t tile = tile0; tile < tile1; ++tile) {
    const int64_t t0 = tile * TT;
    const bool has_next = tile + 1 < tile1;
    if (has_next) cs.load(C, ldc, 0, t0 + TT, T, k, cvec, L.tid);

    const f32x16 acc = mfma_chain<KG>(ctile[cur], ureg, L);

#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t t = t0 + col_of(r, L.h);
      const float v = affine(acc[r], sigma != nullptr, sg_i, mu != nullptr, mu_i);
      if (L.rowok && t < T) {
        if constexpr (PACK) {
          Q[t * ldq + L.row] = encode_one(tally, v, sf, ao);
        } else {
          range_one(tally, v);
        }
      }
    }

    if (has_next) cs.store(ctile[cur ^ 1], L.tid);
    __syncthreads();
    cur ^= 1;
  }
  finish<PACK>(tally, minmax, nonfin, counts);
}

// A field that exists.  grid.x: 256 consecutive rows, grid.y: snapshots (strided when T > gridDim.y); one element per
// lane and step, 4-byte loads and 2-byte stores of exactly the logical elements, whatever X, Q and the leading
// dimensions are.
template <bool PACK>
__global__ __launch_bounds__(256) void field_pack_kernel(const float* __restrict__ X, int64_t m, int64_t T, int64_t ldx,
                                                         double sf, double ao, int16_t* __restrict__ Q, int64_t ldq,
                                                         float* __restrict__ minmax,
                                                         unsigned long long* __restrict__ nonfin,
                                                         unsigned long long* __restrict__ counts) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  Tally tally;
  tally_init(tally);
  if (row < m) {
    for (int64_t t = blockIdx.y; t < T; t += gridDim.y) {
      const float v = X[t * ldx + row];
      if constexpr (PACK) {
        Q[t * ldq + row] = encode_one(tally, v, sf, ao);
      } else {
        range_one(tally, v);
      }
    }
  }
  finish<PACK>(tally, minmax, nonfin, counts);
}

// range / count (merged with what they hold when accumulate != 0) from the n workgroup slots: one workgroup
__global__ __launch_bounds__(256) void range_reduce_kernel(const float* __restrict__ minmax,
                                                           const unsigned long long* __restrict__ nonfin, int64_t n,
                                                           float* __restrict__ range, unsigned long long* __restrict__ count,
                                                           int accumulate) {
  __shared__ float smn[256], smx[256];
  __shared__ unsigned long long scn[256];
  float mn = __builtin_bit_cast(float, kPosInf), mx = __builtin_bit_cast(float, kNegInf);
  unsigned long long cn = 0;
  for (int64_t i = threadIdx.x; i < n; i += 256) {
    const float a = minmax[2 * i], b = minmax[2 * i + 1];
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
    cn += nonfin[i];
  }
  smn[threadIdx.x] = mn;
  smx[threadIdx.x] = mx;
  scn[threadIdx.x] = cn;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) {
      const float a = smn[threadIdx.x + w], b = smx[threadIdx.x + w];
      smn[threadIdx.x] = a < smn[threadIdx.x] ? a : smn[threadIdx.x];
      smx[threadIdx.x] = b > smx[threadIdx.x] ? b : smx[threadIdx.x];
      scn[threadIdx.x] += scn[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  mn = smn[0];
  mx = smx[0];
  cn = scn[0];
  if (accumulate) {
    const float a = range[0], b = range[1];
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
    cn += count[0];
  }
  range[0] = mn;
  range[1] = mx;
  count[0] = cn;
}

// the streaming kernels: 256 rows per workgroup, snapshots over grid.y until the launch has ~4096 workgroups
struct FieldPlan {
  int64_t gx, gy;
};
FieldPlan field_plan_for(int64_t m, int64_t T) {
  FieldPlan p;
  p.gx = (m + 255) / 256;
  int64_t want = (4096 + p.gx - 1) / p.gx;
  p.gy = want < T ? want : T;
  if (p.gy > 65535) p.gy = 65535;
  if (p.gy < 1) p.gy = 1;
  return p;
}

// [<= 15 bytes to a 16-byte boundary][nonfin: n x uint64][minmax: n x 2 fp32]
inline size_t slots_bytes(int64_t n) { return 16 + (size_t)n * 16; }

int check_field(const float* X, int64_t m, int64_t T, int64_t ldx, const char* who) {
  DMDX_CHECK_ARG(X != nullptr, "%s: X must not be null", who);
  DMDX_CHECK_ARG(m >= 1 && T >= 1, "%s: m = %lld, T = %lld must be >= 1", who, (long long)m, (long long)T);
  DMDX_CHECK_ARG(m < DIM_LIMIT && T < DIM_LIMIT, "%s: m, T must be < 2^31", who);
  DMDX_CHECK_ARG(ldx >= 1 && ldx < DIM_LIMIT, "%s: ldx = %lld must be in 1 .. 2^31 - 1", who, (long long)ldx);
  return 0;
}

int check_packing(double sf, double ao, const int16_t* Q, int64_t ldq, int64_t m, const char* who) {
  DMDX_CHECK_ARG(Q != nullptr && ((uintptr_t)Q & 1u) == 0, "%s: Q must not be null and must be 2-byte aligned", who);
  DMDX_CHECK_ARG(ldq >= m && ldq < DIM_LIMIT, "%s: ldq = %lld must be in m = %lld .. 2^31 - 1", who, (long long)ldq,
                 (long long)m);
  DMDX_CHECK_ARG(sf == sf && sf - sf == 0.0 && sf != 0.0, "%s: scale_factor = %g must be finite and not 0", who, sf);
  DMDX_CHECK_ARG(ao - ao == 0.0, "%s: add_offset = %g must be finite", who, ao);
  return 0;
}

struct Slots {
  unsigned long long* nonfin;
  float* minmax;
};
int check_range(float* range, unsigned long long* count, void* workspace, size_t workspace_bytes, int64_t n, Slots* s,
                const char* who) {
  DMDX_CHECK_ARG(range != nullptr && count != nullptr, "%s: range and count must not be null", who);
  const size_t need = slots_bytes(n);
  if (workspace == nullptr || workspace_bytes < need) {
    dmdx_set_error("%s: workspace of %zu bytes, %zu needed", who, workspace == nullptr ? (size_t)0 : workspace_bytes, need);
    return DMDX_E_WORKSPACE;
  }
  char* base = reinterpret_cast<char*>(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
  s->nonfin = reinterpret_cast<unsigned long long*>(base);
  s->minmax = reinterpret_cast<float*>(base + (size_t)n * 8);
  return 0;
}

template <bool PACK>
int launch_expand(const float* U, int64_t m, int k, int64_t ldu, const float* C, int64_t ldc, int64_t T, const float* mu,
                  const float* sigma, double sf, double ao, int16_t* Q, int64_t ldq, float* minmax,
                  unsigned long long* nonfin, unsigned long long* counts, hipStream_t st, const char* who) {
  const Plan p = plan_for(m, T);
  const int cvec = cvec_of(C, ldc);
#define DMDX_LAUNCH(KG)                                                                                                     \
  hipLaunchKernelGGL((expand_pack_kernel<KG, PACK>), p.grid(), dim3(256), 0, st, U, m, k, ldu, C, ldc, T, mu, sigma, sf, ao, \
                     Q, ldq, p.tiles_per_wg, p.ntiles, cvec, minmax, nonfin, counts)
  DMDX_DISPATCH_KG(k, who, DMDX_LAUNCH)
#undef DMDX_LAUNCH
  DMDX_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int dmdx_pack_max_k(void) { return MAXK; }

extern "C" size_t dmdx_expand_range_workspace_bytes(int64_t m, int64_t k, int64_t T) {
  (void)k;
  if (m < 1 || T < 1 || m >= DIM_LIMIT || T >= DIM_LIMIT) return 16;
  const Plan p = plan_for(m, T);
  return slots_bytes(p.nrb * p.nsplit);
}

extern "C" int dmdx_expand_range_f32(const float* U, int64_t m, int64_t k, int64_t ldu, const float* C, int64_t ldc,
                                     int64_t T, const float* mu, const float* sigma, float* range,
                                     unsigned long long* count, int accumulate, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  const char* who = "dmdx_expand_range_f32";
  if (int rc = check_common(U, m, k, ldu, C, ldc, T, who)) return rc;
  const Plan p = plan_for(m, T);
  const int64_t n = p.nrb * p.nsplit;
  Slots s;
  if (int rc = check_range(range, count, workspace, workspace_bytes, n, &s, who)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = launch_expand<false>(U, m, (int)k, ldu, C, ldc, T, mu, sigma, 1.0, 0.0, nullptr, 0, s.minmax, s.nonfin,
                                    nullptr, st, who))
    return rc;
  hipLaunchKernelGGL(range_reduce_kernel, dim3(1), dim3(256), 0, st, s.minmax, s.nonfin, n, range, count, accumulate);
  DMDX_LAUNCH_CHECK();
  return 0;
}

extern "C" int dmdx_expand_pack_i16(const float* U, int64_t m, int64_t k, int64_t ldu, const float* C, int64_t ldc,
                                    int64_t T, const float* mu, const float* sigma, double scale_factor,
                                    double add_offset, int16_t* Q, int64_t ldq, unsigned long long* counts,
                                    void* stream) {
  const char* who = "dmdx_expand_pack_i16";
  if (int rc = check_common(U, m, k, ldu, C, ldc, T, who)) return rc;
  if (int rc = check_packing(scale_factor, add_offset, Q, ldq, m, who)) return rc;
  return launch_expand<true>(U, m, (int)k, ldu, C, ldc, T, mu, sigma, scale_factor, add_offset, Q, ldq, nullptr, nullptr,
                             counts, (hipStream_t)stream, who);
}

extern "C" size_t dmdx_range_workspace_bytes(int64_t m, int64_t T) {
  if (m < 1 || T < 1 || m >= DIM_LIMIT || T >= DIM_LIMIT) return 16;
  const FieldPlan p = field_plan_for(m, T);
  return slots_bytes(p.gx * p.gy);
}

extern "C" int dmdx_range_f32(const float* X, int64_t m, int64_t T, int64_t ldx, float* range, unsigned long long* count,
                              int accumulate, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "dmdx_range_f32";
  if (int rc = check_field(X, m, T, ldx, who)) return rc;
  const FieldPlan p = field_plan_for(m, T);
  const int64_t n = p.gx * p.gy;
  Slots s;
  if (int rc = check_range(range, count, workspace, workspace_bytes, n, &s, who)) return rc;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL((field_pack_kernel<false>), dim3((unsigned)p.gx, (unsigned)p.gy), dim3(256), 0, st, X, m, T, ldx, 1.0,
                     0.0, (int16_t*)nullptr, (int64_t)0, s.minmax, s.nonfin, (unsigned long long*)nullptr);
  DMDX_LAUNCH_CHECK();
  hipLaunchKernelGGL(range_reduce_kernel, dim3(1), dim3(256), 0, st, s.minmax, s.nonfin, n, range, count, accumulate);
  DMDX_LAUNCH_CHECK();
  return 0;
}

extern "C" int dmdx_pack_f32_i16(const float* X, int64_t m, int64_t T, int64_t ldx, double scale_factor, double add_offset,
                                 int16_t* Q, int64_t ldq, unsigned long long* counts, void* stream) {
  const char* who = "dmdx_pack_f32_i16";
  if (int rc = check_field(X, m, T, ldx, who)) return rc;
  if (int rc = check_packing(scale_factor, add_offset, Q, ldq, m, who)) return rc;
  const FieldPlan p = field_plan_for(m, T);
  hipLaunchKernelGGL((field_pack_kernel<true>), dim3((unsigned)p.gx, (unsigned)p.gy), dim3(256), 0, (hipStream_t)stream, X,
                     m, T, ldx, scale_factor, add_offset, Q, ldq, (float*)nullptr, (unsigned long long*)nullptr, counts);
  DMDX_LAUNCH_CHECK();
  return 0;
}
