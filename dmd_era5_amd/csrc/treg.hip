// K21: least-squares regression of every grid point of one row block on a small temporal design matrix (an intercept,
// a polynomial trend, annual and diurnal harmonics, user series), fitted and removed on the device.
//
// The host forms the design D (T x p, fp64) and W = (D^T D)^-1 D^T (p x T, fp64) once; both are data here.  Two HBM
// streams:
//   fit    one read of X:          coef[j, i] = fp32( sum over t of fp64(X[i, t]) * W[j, t] )      for all p at once
//   apply  one read + one write:   y = fp32( fp64(x) -+ sum over j of fp64(coef[j, i]) * D[t, j] )
//
// Arithmetic (the contract of tests/treg_ref.py, held bit for bit).  Time is cut into segments of `seg` snapshots,
// [0, seg), [seg, 2 seg), ...; a segment is one fp64 chain in ascending t that starts at +0.0 and adds one rounded
// product per snapshot, and the segment sums are added in ascending order to a total that starts at +0.0.  The
// partition is an argument, so the result does not depend on the launch geometry: with a workspace every segment is
// a workgroup row of its own and a second small kernel adds the partials in order; without one a lane walks its
// segments one after another.  Every multiply that meets an add is two roundings: contraction is switched off for
// the whole file.
//
// All p accumulators of a row live in one lane (p is a template argument: the accumulators are registers), so X is
// read once whatever p is.  W[., t] and D[t, .] are the same for every lane of a launch: wave-uniform loads.
#include "time_rows.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxP = 8;
constexpr int kInFlight = 8;       // snapshot loads issued before the 8 x p sequential adds
constexpr int kApplyChunk = 8;     // snapshots one lane of apply walks with its coefficients in registers

// One lane: R consecutive rows, P x R fp64 accumulators.  Segments s = blockIdx.y, blockIdx.y + gridDim.y, ...:
// SPLIT stores every segment sum to ws[(s P + j) m + row]; otherwise gridDim.y is 1 and the lane adds them up itself.
template <int P, int R, bool FULL, bool SPLIT>
__device__ __forceinline__ void treg_fit_rows(const float* __restrict__ xp, int nr, int64_t m, int64_t T, int64_t ldx,
                                              const double* __restrict__ W, int64_t ldw, int64_t seg, int64_t nseg,
                                              double* __restrict__ wsp, float* __restrict__ cp, int64_t ldc) {
  typedef float vec __attribute__((ext_vector_type(R)));
  auto ld = [&](int64_t t) -> vec {
    if (FULL) return *reinterpret_cast<const vec*>(xp + t * ldx);
    vec v;
#pragma unroll
    for (int e = 0; e < R; ++e) v[e] = e < nr ? xp[t * ldx + e] : 0.f;
    return v;
  };

  double tot[P][R];
#pragma unroll
  for (int j = 0; j < P; ++j)
#pragma unroll
    for (int e = 0; e < R; ++e) tot[j][e] = 0.0;

  for (int64_t s = blockIdx.y; s < nseg; s += gridDim.y) {
    const int64_t a = s * seg;
    const int64_t b = T - a < seg ? T : a + seg;
    double acc[P][R];
#pragma unroll
    for (int j = 0; j < P; ++j)
#pragma unroll
      for (int e = 0; e < R; ++e) acc[j][e] = 0.0;

    int64_t t = a;
    for (; t + kInFlight <= b; t += kInFlight) {
      vec v[kInFlight];
#pragma unroll
      for (int u = 0; u < kInFlight; ++u) v[u] = ld(t + u);
#pragma unroll
      for (int u = 0; u < kInFlight; ++u)
#pragma unroll
        for (int j = 0; j < P; ++j) {
          const double w = W[j * ldw + t + u];
#pragma unroll
          for (int e = 0; e < R; ++e) {
            const double q = (double)v[u][e] * w;              // a rounded product of its own
            acc[j][e] = acc[j][e] + q;
          }
        }
    }
    for (; t < b; ++t) {                                        // the ragged end of a segment
      const vec v = ld(t);
#pragma unroll
      for (int j = 0; j < P; ++j) {
        const double w = W[j * ldw + t];
#pragma unroll
        for (int e = 0; e < R; ++e) {
          const double q = (double)v[e] * w;
          acc[j][e] = acc[j][e] + q;
        }
      }
    }

    if (SPLIT) {
#pragma unroll
      for (int j = 0; j < P; ++j) {
        double* o = wsp + (s * P + j) * m;
#pragma unroll
        for (int e = 0; e < R; ++e)
          if (e < nr) o[e] = acc[j][e];
      }
    } else {
#pragma unroll
      for (int j = 0; j < P; ++j)
#pragma unroll
        for (int e = 0; e < R; ++e) tot[j][e] = tot[j][e] + acc[j][e];
    }
  }

  if (!SPLIT) {
#pragma unroll
    for (int j = 0; j < P; ++j) {
      float* o = cp + j * ldc;
      if (R > 1 && FULL && ((uintptr_t)o & 15u) == 0) {
        vec res;
#pragma unroll
        for (int e = 0; e < R; ++e) res[e] = (float)tot[j][e];
        *reinterpret_cast<vec*>(o) = res;
      } else {
#pragma unroll
        for (int e = 0; e < R; ++e)
          if (e < nr) o[e] = (float)tot[j][e];
      }
    }
  }
}

// grid.x: chunks of 256 R rows; grid.y: segments (SPLIT; strided when there are more than gridDim.y) or 1.  R = 4 is
// launched only for a 16-byte aligned X with ldx % 4 == 0: one 16-byte load per snapshot, the ragged last quad
// element by element in a loop of its own (no branch around a load); R = 1: one dword per lane.
template <int P, int R, bool SPLIT>
__global__ __launch_bounds__(256) void treg_fit_kernel(const float* __restrict__ X, int64_t m, int64_t T, int64_t ldx,
                                                       const double* __restrict__ W, int64_t ldw, int64_t seg,
                                                       int64_t nseg, double* __restrict__ ws,
                                                       float* __restrict__ coef, int64_t ldc) {
  const int64_t r0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * R;
  if (r0 >= m) return;
  const int nr = (m - r0) < R ? (int)(m - r0) : R;
  double* wsp = SPLIT ? ws + r0 : nullptr;
  if (nr == R)
    treg_fit_rows<P, R, true, SPLIT>(X + r0, nr, m, T, ldx, W, ldw, seg, nseg, wsp, coef + r0, ldc);
  else
    treg_fit_rows<P, R, false, SPLIT>(X + r0, nr, m, T, ldx, W, ldw, seg, nseg, wsp, coef + r0, ldc);
}

// The tail of the split form: one lane per (row, regressor) adds the segment sums in ascending order.
__global__ __launch_bounds__(256) void treg_combine_kernel(const double* __restrict__ ws, int64_t m, int p, int64_t nseg,
                                                           float* __restrict__ coef, int64_t ldc) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int j = blockIdx.y;
  if (i >= m) return;
  double tot = 0.0;
  for (int64_t s = 0; s < nseg; ++s) tot = tot + ws[(s * p + j) * m + i];
  coef[j * ldc + i] = (float)tot;
}

// grid.x: chunks of 4 consecutive rows per lane, grid.y: runs of kApplyChunk snapshots (strided when there are more
// than gridDim.y).  The chunks are head-shifted so that every full chunk of Y goes out as one aligned 16-byte store
// (quad_at, time_rows.h).  A lane keeps the p coefficients of its 4 rows in registers (as fp64) over the run and loads
// them again only when the head shift changes (never, when ldy % 4 == 0): coef is read T / kApplyChunk times, not T
// times.  X and Y carry no __restrict__: Y == X is in place (a lane reads its own elements before it writes them).
__global__ __launch_bounds__(256) void treg_apply_kernel(const float* X, int64_t m, int64_t T, int64_t ldx,
                                                         const double* __restrict__ D, int p, int64_t ldd,
                                                         const float* __restrict__ coef, int64_t ldc, int restore,
                                                         float* Y, int64_t ldy) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t nrun = (T + kApplyChunk - 1) / kApplyChunk;
  for (int64_t run = blockIdx.y; run < nrun; run += gridDim.y) {
    const int64_t t0 = run * kApplyChunk;
    const int64_t t1 = T - t0 < kApplyChunk ? T : t0 + kApplyChunk;
    double cd[kMaxP][4];
    int have = -1;                                              // the head shift cd was loaded for
    for (int64_t t = t0; t < t1; ++t) {
      float* yt = Y + t * ldy;
      const float* xt = X + t * ldx;
      Quad<4> q = quad_at<4>(yt, c);
      if (q.past(m)) continue;
      q.clip(m);
      const int64_t r = q.r;
      const bool full = q.full();
      if (q.head != have) {
        have = q.head;
#pragma unroll
        for (int j = 0; j < kMaxP; ++j) {
          if (j < p) {
            const float* cj = coef + j * ldc + r;
            if (full) {
              const f32x4 v = ldq_any(cj);
#pragma unroll
              for (int e = 0; e < 4; ++e) cd[j][e] = (double)v[e];
            } else {
#pragma unroll
              for (int e = 0; e < 4; ++e) cd[j][e] = (e >= q.lo && e < q.hi) ? (double)cj[e] : 0.0;
            }
          }
        }
      }
      double f[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int j = 0; j < kMaxP; ++j) {
        if (j < p) {
          const double d = D[t * ldd + j];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const double q = cd[j][e] * d;                      // product rounded, then the add
            f[e] = f[e] + q;
          }
        }
      }
      if (full) {
        f32x4 y = ldq_any(xt + r);
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = (float)(restore ? (double)y[e] + f[e] : (double)y[e] - f[e]);
        *reinterpret_cast<f32x4*>(yt + r) = y;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (e >= q.lo && e < q.hi) {
            const double x = (double)xt[r + e];
            yt[r + e] = (float)(restore ? x + f[e] : x - f[e]);
          }
      }
    }
  }
}

// nseg p m doubles (the factors are below 2^31, 2^4 and 2^31: the product is formed in 128 bits and saturates)
size_t fit_workspace_bytes(int64_t m, int64_t T, int64_t p, int64_t seg) {
  const int64_t nseg = (T + seg - 1) / seg;
  const unsigned __int128 n = (unsigned __int128)nseg * (unsigned)p * (uint64_t)m * sizeof(double);
  return n > (unsigned __int128)SIZE_MAX ? SIZE_MAX : (size_t)n;
}

template <int P>
int launch_fit(const float* X, int64_t m, int64_t T, int64_t ldx, const double* W, int64_t ldw, int64_t seg, int64_t nseg,
               double* ws, float* coef, int64_t ldc, hipStream_t st) {
  const bool quad = dmdx_aligned16(X) && ldx % 4 == 0;
  const int64_t rows_per_wg = quad ? 1024 : 256;
  const unsigned gx = (unsigned)((m + rows_per_wg - 1) / rows_per_wg);
  const dim3 grid(gx, ws ? grid_rows(nseg) : 1u);
  if (ws) {
    if (quad)
      hipLaunchKernelGGL((treg_fit_kernel<P, 4, true>), grid, dim3(256), 0, st, X, m, T, ldx, W, ldw, seg, nseg, ws, coef, ldc);
    else
      hipLaunchKernelGGL((treg_fit_kernel<P, 1, true>), grid, dim3(256), 0, st, X, m, T, ldx, W, ldw, seg, nseg, ws, coef, ldc);
    DMDX_LAUNCH_CHECK();
    hipLaunchKernelGGL(treg_combine_kernel, dim3((unsigned)((m + 255) / 256), (unsigned)P), dim3(256), 0, st, ws, m, P, nseg,
                       coef, ldc);
  } else {
    if (quad)
      hipLaunchKernelGGL((treg_fit_kernel<P, 4, false>), grid, dim3(256), 0, st, X, m, T, ldx, W, ldw, seg, nseg, ws, coef, ldc);
    else
      hipLaunchKernelGGL((treg_fit_kernel<P, 1, false>), grid, dim3(256), 0, st, X, m, T, ldx, W, ldw, seg, nseg, ws, coef, ldc);
  }
  DMDX_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int dmdx_treg_max_p(void) { return kMaxP; }

extern "C" size_t dmdx_treg_fit_workspace_bytes(int64_t m, int64_t T, int64_t p, int64_t seg) {
  if (m < 0 || T < 0 || p < 1 || p > kMaxP || seg < 1 || m >= kMaxSize || T >= kMaxSize || seg >= kMaxSize) return 0;
  return fit_workspace_bytes(m, T, p, seg);
}

extern "C" int dmdx_treg_fit_f32(const float* X, int64_t m, int64_t T, int64_t ldx, const double* W, int p, int64_t ldw,
                                 int64_t seg, float* coef, int64_t ldc, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  DMDX_CHECK_ARG(X && W && coef, "treg_fit: null pointer");
  DMDX_CHECK_ARG(p >= 1 && p <= kMaxP, "treg_fit: p=%d outside 1..%d", p, kMaxP);
  DMDX_CHECK_ARG(seg >= 1 && seg < kMaxSize, "treg_fit: seg=%lld outside 1..2^31-1", (long long)seg);
  if (int rc = check_block("treg_fit", m, T, {{"ldx", ldx}, {"ldc", ldc}}, {X, coef}, {W, workspace})) return rc;
  DMDX_CHECK_ARG(ldw >= T && ldw < kMaxSize, "treg_fit: ldw=%lld < T=%lld or >= 2^31", (long long)ldw, (long long)T);
  const size_t need = fit_workspace_bytes(m, T, p, seg);
  DMDX_CHECK_ARG(!workspace || (need != SIZE_MAX && workspace_bytes >= need), "treg_fit: workspace of %zu bytes, %zu needed",
                 workspace_bytes, need);
  if (m == 0 || T == 0) return 0;
  const int64_t nseg = (T + seg - 1) / seg;
  double* ws = (double*)workspace;
  hipStream_t st = (hipStream_t)stream;
  switch (p) {
    case 1: return launch_fit<1>(X, m, T, ldx, W, ldw, seg, nseg, ws, coef, ldc, st);
    case 2: return launch_fit<2>(X, m, T, ldx, W, ldw, seg, nseg, ws, coef, ldc, st);
    case 3: return launch_fit<3>(X, m, T, ldx, W, ldw, seg, nseg, ws, coef, ldc, st);
    case 4: return launch_fit<4>(X, m, T, ldx, W, ldw, seg, nseg, ws, coef, ldc, st);
    case 5: return launch_fit<5>(X, m, T, ldx, W, ldw, seg, nseg, ws, coef, ldc, st);
    case 6: return launch_fit<6>(X, m, T, ldx, W, ldw, seg, nseg, ws, coef, ldc, st);
    case 7: return launch_fit<7>(X, m, T, ldx, W, ldw, seg, nseg, ws, coef, ldc, st);
    default: return launch_fit<8>(X, m, T, ldx, W, ldw, seg, nseg, ws, coef, ldc, st);
  }
}

extern "C" int dmdx_treg_apply_f32(const float* X, int64_t m, int64_t T, int64_t ldx, const double* D, int p, int64_t ldd,
                                   const float* coef, int64_t ldc, int restore, float* Y, int64_t ldy, void* stream) {
  DMDX_CHECK_ARG(X && D && coef && Y, "treg_apply: null pointer");
  DMDX_CHECK_ARG(p >= 1 && p <= kMaxP, "treg_apply: p=%d outside 1..%d", p, kMaxP);
  if (int rc = check_block("treg_apply", m, T, {{"ldx", ldx}, {"ldc", ldc}, {"ldy", ldy}}, {X, Y, coef}, {D})) return rc;
  DMDX_CHECK_ARG(ldd >= p && ldd < kMaxSize, "treg_apply: ldd=%lld < p=%d or >= 2^31", (long long)ldd, p);
  if (int rc = check_ranges("treg_apply", X, T, ldx, Y, T, ldy, m, true)) return rc;
  if (m == 0 || T == 0) return 0;
  const int64_t nrun = (T + kApplyChunk - 1) / kApplyChunk;
  const dim3 grid((unsigned)((chunks_of<4>(m) + 255) / 256), grid_rows(nrun));
  hipLaunchKernelGGL(treg_apply_kernel, grid, dim3(256), 0, (hipStream_t)stream, X, m, T, ldx, D, p, ldd, coef, ldc, restore,
                     Y, ldy);
  DMDX_LAUNCH_CHECK();
  return 0;
}
