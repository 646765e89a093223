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
#include "dmdx_common.h"

#pragma clang fp contract(off)

namespace {

constexpr unsigned kQuietNaN = 0x7FC00000u;
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

__device__ __forceinline__ f32x4 load4(const float* p) {
  if (((uintptr_t)p & 15u) == 0) return *reinterpret_cast<const f32x4*>(p);
  f32x4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = p[e];
  return v;
}

__device__ __forceinline__ float apply_one(float x, float mu, float sg, bool has_sd, bool restore) {
  if (restore) {
    const float y = has_sd ? x * sg : x;                        // two roundings: the file has no contraction
    return y + mu;
  }
  const float y = x - mu;
  return has_sd ? y / sg : y;                                   // correctly rounded fp32 divide (no fast-math), as K13
}

// grid.x: chunks of 4 consecutive rows per lane, grid.y: snapshots (strided when T > gridDim.y), as K14's kernel: the
// chunks of snapshot t start `head` elements before row 0, so that every full chunk of Y goes out as one aligned
// 16-byte store whatever Y and ldy are.  X, mean and sd are read with 16-byte loads where their address allows it and
// dword by dword otherwise; both routes apply apply_one to the same values.  X and Y carry no __restrict__: Y == X is
// the in-place case (a lane reads its own elements before it writes them).
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
    const int head = (int)(((uintptr_t)yt >> 2) & 3u);         // elements of yt past a 16-byte boundary
    const int64_t r = c * 4 - head;                            // first row of this lane's chunk
    if (r >= m) continue;
    const int lo = r < 0 ? (int)(-r) : 0;
    const int hi = m - r < 4 ? (int)(m - r) : 4;
    const float* mp = mean + (has ? (int64_t)sl * ldc : 0);
    const float* sp = has_sd ? sd + (has ? (int64_t)sl * lds : 0) : nullptr;

    if (lo == 0 && hi == 4) {
      f32x4 y = load4(xt + r);
      if (has) {
        const f32x4 mu = load4(mp + r);
        f32x4 sg = {1.f, 1.f, 1.f, 1.f};
        if (has_sd) sg = load4(sp + r);
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = apply_one(y[e], mu[e], sg[e], has_sd, restore != 0);
      }
      *reinterpret_cast<f32x4*>(yt + r) = y;
    } else {
      for (int e = lo; e < hi; ++e) {
        float y = xt[r + e];
        if (has) y = apply_one(y, mp[r + e], has_sd ? sp[r + e] : 1.f, has_sd, restore != 0);
        yt[r + e] = y;
      }
    }
  }
}

constexpr int64_t kMaxSize = int64_t(1) << 31;

int check_stat(const char* who, const float* X, int64_t m, int64_t T, int64_t ldx, const int32_t* order, int64_t n_order,
               const int32_t* start, int64_t S, const float* mean, int64_t ldc) {
  DMDX_CHECK_ARG(X && order && start && mean, "%s: null pointer", who);
  DMDX_CHECK_ARG(m >= 0 && T >= 0 && n_order >= 0, "%s: negative size (m=%lld T=%lld n_order=%lld)", who, (long long)m,
                 (long long)T, (long long)n_order);
  DMDX_CHECK_ARG(S >= 1, "%s: S=%lld < 1", who, (long long)S);
  DMDX_CHECK_ARG(m < kMaxSize && T < kMaxSize && ldx < kMaxSize && ldc < kMaxSize && S < kMaxSize && n_order < kMaxSize,
                 "%s: a size >= 2^31 (m=%lld T=%lld ldx=%lld ldc=%lld S=%lld n_order=%lld)", who, (long long)m, (long long)T,
                 (long long)ldx, (long long)ldc, (long long)S, (long long)n_order);
  DMDX_CHECK_ARG(ldx >= m && ldc >= m, "%s: ldx=%lld or ldc=%lld < m=%lld", who, (long long)ldx, (long long)ldc, (long long)m);
  DMDX_CHECK_ARG(((uintptr_t)X & 3u) == 0 && ((uintptr_t)mean & 3u) == 0 && ((uintptr_t)order & 3u) == 0 &&
                     ((uintptr_t)start & 3u) == 0, "%s: a pointer is not aligned to its element", who);
  return 0;
}

// 4 rows per lane when X allows 16-byte loads and the launch still has about 1024 workgroups (4 per CU): K5's
// one-quad-per-lane kernel ran 127 workgroups on a 129 780-row block and left half of the chip idle.
template <bool STD>
int launch_stat(const float* X, int64_t m, int64_t T, int64_t ldx, const int32_t* order, int64_t n_order,
                const int32_t* start, int64_t S, const float* mean, int64_t ldc, int ddof, float* out, int64_t ldo,
                void* stream) {
  const bool quad = dmdx_aligned16(X) && ldx % 4 == 0 && S * ((m + 1023) / 1024) >= 1024;
  const int64_t rows_per_wg = quad ? 1024 : 256;
  const dim3 grid((unsigned)((m + rows_per_wg - 1) / rows_per_wg), (unsigned)(S < 65535 ? S : 65535));
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
  DMDX_CHECK_ARG(lds >= m && lds < kMaxSize, "clim_std: lds=%lld < m=%lld or >= 2^31", (long long)lds, (long long)m);
  DMDX_CHECK_ARG(((uintptr_t)sd & 3u) == 0, "clim_std: sd is not aligned to its element");
  if (m == 0) return 0;
  return launch_stat<true>(X, m, T, ldx, order, n_order, start, S, mean, ldc, ddof, sd, lds, stream);
}

extern "C" int dmdx_clim_apply_f32(const float* X, int64_t m, int64_t T, int64_t ldx, const int32_t* slot, int64_t S,
                                   const float* mean, int64_t ldc, const float* sd, int64_t lds, int restore, float* Y,
                                   int64_t ldy, void* stream) {
  DMDX_CHECK_ARG(X && slot && mean && Y, "clim_apply: null pointer");
  DMDX_CHECK_ARG(m >= 0 && T >= 0, "clim_apply: negative size (m=%lld T=%lld)", (long long)m, (long long)T);
  DMDX_CHECK_ARG(S >= 1, "clim_apply: S=%lld < 1", (long long)S);
  DMDX_CHECK_ARG(m < kMaxSize && T < kMaxSize && ldx < kMaxSize && ldc < kMaxSize && ldy < kMaxSize && S < kMaxSize &&
                     (!sd || lds < kMaxSize), "clim_apply: a size >= 2^31 (m=%lld T=%lld ldx=%lld ldc=%lld lds=%lld ldy=%lld S=%lld)",
                 (long long)m, (long long)T, (long long)ldx, (long long)ldc, (long long)lds, (long long)ldy, (long long)S);
  DMDX_CHECK_ARG(ldx >= m && ldc >= m && ldy >= m && (!sd || lds >= m),
                 "clim_apply: a leading dimension < m=%lld (ldx=%lld ldc=%lld lds=%lld ldy=%lld)", (long long)m,
                 (long long)ldx, (long long)ldc, (long long)lds, (long long)ldy);
  DMDX_CHECK_ARG(((uintptr_t)X & 3u) == 0 && ((uintptr_t)Y & 3u) == 0 && ((uintptr_t)mean & 3u) == 0 &&
                     ((uintptr_t)sd & 3u) == 0 && ((uintptr_t)slot & 3u) == 0, "clim_apply: a pointer is not aligned to its element");
  if (m == 0 || T == 0) return 0;
  if (!(Y == X && ldy == ldx)) {                                // anything but the in-place case: the ranges must be disjoint
    const uintptr_t x0 = (uintptr_t)X, x1 = x0 + 4 * (uintptr_t)((T - 1) * ldx + m);
    const uintptr_t y0 = (uintptr_t)Y, y1 = y0 + 4 * (uintptr_t)((T - 1) * ldy + m);
    DMDX_CHECK_ARG(x1 <= y0 || y1 <= x0, "clim_apply: X and Y overlap (only Y == X with ldy == ldx runs in place)");
  }
  const int64_t chunks = (m + 3 + 3) / 4;                       // + 3: the head shift of a column
  const dim3 grid((unsigned)((chunks + 255) / 256), (unsigned)(T < 65535 ? T : 65535));
  hipLaunchKernelGGL(clim_apply_kernel, grid, dim3(256), 0, (hipStream_t)stream, X, m, T, ldx, slot, S, mean, ldc, sd, lds,
                     restore, Y, ldy);
  DMDX_LAUNCH_CHECK();
  return 0;
}
