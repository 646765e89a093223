// K18: slot climatology of the snapshots of one row block, and the anomalies against it, on the device.
//
// A slot is a class of the calendar (an hour of the day, a (month, hour) pair, a day of the year).  The host hands
// the membership over as a CSR list -- slot s owns the snapshot indices order[start[s] .. start[s + 1]) -- and as a
// label per snapshot (slot[t], the climatology snapshot t takes).  Three HBM streams:
//   mean   one read of X:     mean[s, i] = fp32( sum over the list of fp64(X[i, t]) / n_s )
//   std    one more read:     sd[s, i]   = fp32( sqrt( sum of (fp64(X[i, t]) - fp64(mean[s, i]))^2 / (n_s - ddof) ) )
//   apply  one read + one write (+ S m 4 bytes of mean / sd that stay in L2 / Infinity Cache):
//          y = (x - mean) [/ sd]   or, restoring,   y = fl(fl(x * sd) + mean)
//
// Arithmetic (the contract of tests/clim_ref.py, held bit for bit): the sum of a slot runs in the order of its list,
// one fp64 add per entry, whatever the launch geometry -- so a slot is never split over workgroups or lanes, and the
// parallelism is rows x slots.  Every multiply that meets an add here is two roundings: contraction is switched off
// for the whole file (hipcc contracts a * b + c to an FMA by default, also across statements).
//
// The lists are data, not arguments the host has checked: start is clamped to [0, n_order], an entry of order outside
// [0, T) is skipped and not counted, a label outside [0, S) leaves its snapshot alone.  A wrong list gives wrong
// means; it never addresses anything outside X, mean or sd.
#include "time_rows.h"

#pragma clang fp contract(off)

namespace {

constexpr int kInFlight = 8;       // snapshot loads issued before the 8 sequential adds

// grid.x: chunks of 256 R rows, grid.y: slots (strided when S > gridDim.y).  A lane owns R consecutive rows and R
// fp64 accumulators.  R = 4 (launched only for a 16-byte aligned X with ldx % 4 == 0): one 16-byte load per listed
// snapshot, the ragged last quad element by element; R = 1: one dword per lane, for every other X and for launches
// that R = 4 would leave with too few workgroups.  The list entries are the same for every lane of the launch
// (wave-uniform loads); an entry that is skipped is replaced by snapshot 0, loaded and then selected away, so that the
// loop keeps kInFlight loads in flight without a branch.  Adding the +0.0 of a skipped entry changes no bit: the sum
// starts at +0.0 and x + y is -0.0 only for two -0.0, so the accumulator is never -0.0.
template <int R, bool STD, bool FULL>
__device__ __forceinline__ void clim_stat_rows(const float* __restrict__ xp, int nr, int64_t T, int64_t ldx,
                                               const int32_t* __restrict__ order, int64_t n_order,
                                               const int32_t* __restrict__ start, int64_t S,
                                               const float* __restrict__ mp, int64_t ldc, int ddof,
                                               float* __restrict__ op, int64_t ldo) {
  typedef float vec __attribute__((ext_vector_type(R)));
  auto ld = [&](int64_t t) -> vec {
    if (FULL) return *reinterpret_cast<const vec*>(xp + t * ldx);
    vec v;
#pragma unroll
    for (int e = 0; e < R; ++e) v[e] = e < nr ? xp[t * ldx + e] : 0.f;
    return v;
  };

  for (int64_t s = blockIdx.y; s < S; s += gridDim.y) {
    int64_t a = start[s], b = start[s + 1];
    a = a < 0 ? 0 : (a > n_order ? n_order : a);
    b = b < a ? a : (b > n_order ? n_order : b);
    if (T == 0) b = a;                                          // no snapshot 0 to stand in for a skipped entry

    double mu[R], acc[R];
#pragma unroll
    for (int e = 0; e < R; ++e) {
      acc[e] = 0.0;
      mu[e] = (STD && e < nr) ? (double)mp[s * ldc + e] : 0.0;
    }
    int64_t cnt = 0;
    for (int64_t j = a; j < b; j += kInFlight) {
      vec v[kInFlight];
      bool ok[kInFlight];
#pragma unroll
      for (int u = 0; u < kInFlight; ++u) {
        const bool in = j + u < b;
        const int32_t t = order[in ? j + u : a];
        ok[u] = in && t >= 0 && (int64_t)t < T;
        v[u] = ld(ok[u] ? (int64_t)t : 0);
      }
#pragma unroll
      for (int u = 0; u < kInFlight; ++u) {
        cnt += ok[u] ? 1 : 0;
#pragma unroll
        for (int e = 0; e < R; ++e) {
          double term = (double)v[u][e];
          if (STD) {
            const double d = term - mu[e];
            term = d * d;
          }
          acc[e] = acc[e] + (ok[u] ? term : 0.0);
        }
      }
    }

    const int64_t n = cnt - (STD ? ddof : 0);
    vec res;
#pragma unroll
    for (int e = 0; e < R; ++e) {
      const double q = acc[e] / (double)n;                      // IEEE fp64 divide, then one rounding to fp32
      res[e] = n > 0 ? (float)(STD ? __dsqrt_rn(q) : q) : __builtin_bit_cast(float, kQuietNaN);
    }
    float* o = op + s * ldo;
    if (R > 1 && FULL && ((uintptr_t)o & 15u) == 0) {
      *reinterpret_cast<vec*>(o) = res;
    } else {
#pragma unroll
      for (int e = 0; e < R; ++e)
        if (e < nr) o[e] = res[e];
    }
  }
}

template <int R, bool STD>
__global__ __launch_bounds__(256) void clim_stat_kernel(const float* __restrict__ X, int64_t m, int64_t T, int64_t ldx,
                                                        const int32_t* __restrict__ order, int64_t n_order,
                                                        const int32_t* __restrict__ start, int64_t S,
                                                        const float* __restrict__ mean, int64_t ldc, int ddof,
                                                        float* __restrict__ out, int64_t ldo) {
  const int64_t r0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * R;
  if (r0 >= m) return;
  const int nr = (m - r0) < R ? (int)(m - r0) : R;
  const float* mp = STD ? mean + r0 : nullptr;
  if (nr == R)     // (the one ragged quad at the end of the rows runs the loop of its own: no branch around a load)
    clim_stat_rows<R, STD, true>(X + r0, nr, T, ldx, order, n_order, start, S, mp, ldc, ddof, out + r0, ldo);
  else
    clim_stat_rows<R, STD, false>(X + r0, nr, T, ldx, order, n_order, start, S, mp, ldc, ddof, out + r0, ldo);
}

__device__ __forceinline__ float apply_one(float x, float mu, float sg, bool has_sd, bool restore) {
  if (restore) {
    const float y = has_sd ? x * sg : x;                        // two roundings: the file has no contraction
    return y + mu;
  }
  const float y = x - mu;
  return has_sd ? y / sg : y;                                   // correctly rounded fp32 divide (no fast-math), as K13
}

// grid.x: chunks of 4 consecutive rows per lane, head-shifted so that every full chunk of Y goes out as one aligned
// 16-byte store (quad_at, time_rows.h); grid.y: snapshots (strided when T > gridDim.y).  X, mean and sd are read
// with 16-byte loads where their address allows it and dword by dword otherwise; both routes apply apply_one to the
// same values.  X and Y carry no __restrict__: Y == X is in place (a lane reads its own elements before it writes them).
__global__ __launch_bounds__(256) void clim_apply_kernel(const float* X, int64_t m, int64_t T, int64_t ldx,
                                                         const int32_t* __restrict__ slot, int64_t S,
                                                         const float* __restrict__ mean, int64_t ldc,
                                                         const float* __restrict__ sd, int64_t lds, int restore,
                                                         float* Y, int64_t ldy) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool inplace = X == Y;
  const bool has_sd = sd != nullptr;
  for (int64_t t = blockIdx.y; t < T; t += gridDim.y) {
    const int32_t sl = slot[t];
    const bool has = sl >= 0 && (int64_t)sl < S;
    if (!has && inplace) continue;                              // a snapshot without a slot is not touched
    float* yt = Y + t * ldy;
    const float* xt = X + t * ldx;
    Quad<4> q = quad_at<4>(yt, c);
    if (q.past(m)) continue;
    q.clip(m);
    const int64_t r = q.r;
    const float* mp = mean + (has ? (int64_t)sl * ldc : 0);
    const float* sp = has_sd ? sd + (has ? (int64_t)sl * lds : 0) : nullptr;

    if (q.full()) {
      f32x4 y = ldq_any(xt + r);
      if (has) {
        const f32x4 mu = ldq_any(mp + r);
        f32x4 sg = {1.f, 1.f, 1.f, 1.f};
        if (has_sd) sg = ldq_any(sp + r);
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = apply_one(y[e], mu[e], sg[e], has_sd, restore != 0);
      }
      *reinterpret_cast<f32x4*>(yt + r) = y;
    } else {
      for (int e = q.lo; e < q.hi; ++e) {
        float y = xt[r + e];
        if (has) y = apply_one(y, mp[r + e], has_sd ? sp[r + e] : 1.f, has_sd, restore != 0);
        yt[r + e] = y;
      }
    }
  }
}

int check_stat(const char* who, const float* X, int64_t m, int64_t T, int64_t ldx, const int32_t* order, int64_t n_order,
               const int32_t* start, int64_t S, const float* mean, int64_t ldc) {
  DMDX_CHECK_ARG(X && order && start && mean, "%s: null pointer", who);
  DMDX_CHECK_ARG(n_order >= 0 && n_order < kMaxSize, "%s: n_order=%lld outside 0..2^31-1", who, (long long)n_order);
  DMDX_CHECK_ARG(S >= 1 && S < kMaxSize, "%s: S=%lld outside 1..2^31-1", who, (long long)S);
  return check_block(who, m, T, {{"ldx", ldx}, {"ldc", ldc}}, {X, mean, order, start});
}

// 4 rows per lane when X allows 16-byte loads and the launch still has about 1024 workgroups (4 per CU): K5's
// one-quad-per-lane kernel ran 127 workgroups on a 129 780-row block and left half of the chip idle.
template <bool STD>
int launch_stat(const float* X, int64_t m, int64_t T, int64_t ldx, const int32_t* order, int64_t n_order,
                const int32_t* start, int64_t S, const float* mean, int64_t ldc, int ddof, float* out, int64_t ldo,
                void* stream) {
  const bool quad = dmdx_aligned16(X) && ldx % 4 == 0 && S * ((m + 1023) / 1024) >= 1024;
  const int64_t rows_per_wg = quad ? 1024 : 256;
  const dim3 grid((unsigned)((m + rows_per_wg - 1) / rows_per_wg), grid_rows(S));
  if (quad)
    hipLaunchKernelGGL((clim_stat_kernel<4, STD>), grid, dim3(256), 0, (hipStream_t)stream, X, m, T, ldx, order, n_order,
                       start, S, mean, ldc, ddof, out, ldo);
  else
    hipLaunchKernelGGL((clim_stat_kernel<1, STD>), grid, dim3(256), 0, (hipStream_t)stream, X, m, T, ldx, order, n_order,
                       start, S, mean, ldc, ddof, out, ldo);
  DMDX_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int dmdx_clim_mean_f32(const float* X, int64_t m, int64_t T, int64_t ldx, const int32_t* order, int64_t n_order,
                                  const int32_t* start, int64_t S, float* mean, int64_t ldc, void* stream) {
  if (int rc = check_stat("clim_mean", X, m, T, ldx, order, n_order, start, S, mean, ldc)) return rc;
  if (m == 0) return 0;
  return launch_stat<false>(X, m, T, ldx, order, n_order, start, S, nullptr, ldc, 0, mean, ldc, stream);
}

extern "C" int dmdx_clim_std_f32(const float* X, int64_t m, int64_t T, int64_t ldx, const int32_t* order, int64_t n_order,
                                 const int32_t* start, int64_t S, const float* mean, int64_t ldc, int ddof, float* sd,
                                 int64_t lds, void* stream) {
  if (int rc = check_stat("clim_std", X, m, T, ldx, order, n_order, start, S, mean, ldc)) return rc;
  DMDX_CHECK_ARG(sd, "clim_std: null sd");
  DMDX_CHECK_ARG(ddof == 0 || ddof == 1, "clim_std: ddof=%d outside 0..1", ddof);
  if (int rc = check_block("clim_std", m, T, {{"lds", lds}}, {sd})) return rc;
  if (m == 0) return 0;
  return launch_stat<true>(X, m, T, ldx, order, n_order, start, S, mean, ldc, ddof, sd, lds, stream);
}

extern "C" int dmdx_clim_apply_f32(const float* X, int64_t m, int64_t T, int64_t ldx, const int32_t* slot, int64_t S,
                                   const float* mean, int64_t ldc, const float* sd, int64_t lds, int restore, float* Y,
                                   int64_t ldy, void* stream) {
  DMDX_CHECK_ARG(X && slot && mean && Y, "clim_apply: null pointer");
  DMDX_CHECK_ARG(S >= 1 && S < kMaxSize, "clim_apply: S=%lld outside 1..2^31-1", (long long)S);
  if (int rc = check_block("clim_apply", m, T, {{"ldx", ldx}, {"ldc", ldc}, {"ldy", ldy}, {"lds", sd ? lds : ldc}},
                           {X, Y, mean, sd, slot}))
    return rc;
  if (int rc = check_ranges("clim_apply", X, T, ldx, Y, T, ldy, m, true)) return rc;
  if (m == 0 || T == 0) return 0;
  const dim3 grid((unsigned)((chunks_of<4>(m) + 255) / 256), grid_rows(T));
  hipLaunchKernelGGL(clim_apply_kernel, grid, dim3(256), 0, (hipStream_t)stream, X, m, T, ldx, slot, S, mean, ldc, sd, lds,
                     restore, Y, ldy);
  DMDX_LAUNCH_CHECK();
  return 0;
}
