// K26: lagged second moments of every grid point of one row block: the sum of squares S, the lagged products P_l for up
// to 8 lags, and the squares at the two ends (H_l, E_l) that the pairs of a lag miss.  From them the host forms
// autocovariance and autocorrelation, the persistence / damped-persistence / climatology baselines of a forecast score
// and the effective sample size behind a trend map (dmd_era5_amd/baseline.py).
//
// Arithmetic (the contract of tests/lag_ref.py, held bit for bit).  d_t = fp64(x_t) - fp64(mu) (one rounded subtraction;
// no operation without mu), sq_t = d_t d_t, pr_u = d_{u - tau} d_u, indexed by the LATER snapshot u.  Time is cut into
// segments of `seg` snapshots as in K21 (treg.hip): a segment is one fp64 chain in ascending t that starts at +0.0, the
// segment sums are added in ascending order to a total that starts at +0.0.  The partition is an argument, so the bits do
// not depend on the launch: with a workspace every segment is a workgroup row of its own and a combine kernel adds the
// partials in order (split); without one a lane walks its segments (walk).  Contraction is off for the whole file.
//
// Main pass (S and P_l): a lane owns R consecutive rows and (1 + L) R fp64 accumulators (L is a template tier: the
// accumulators are registers).  The earlier member d_{u - tau} comes from one of two bodies with the same bits:
//   ring    tau <= kRing: every lane keeps its own last kRing loads in LDS, slot u mod kRing, one vector per slot.  A lane
//           reads only what it wrote itself: no barrier, no cross-lane hazard; consecutive lanes hold consecutive 16
//           bytes.  A segment starts by re-reading the largest near lag's worth of snapshots before it into the ring.
//   reload  tau > kRing, or flags bit 0: a second global load at u - tau, served by L2 / Infinity Cache.
// Lags are ascending, so the near lags are a prefix of the list: a mixed list uses each body per lag in one launch.
// Edge pass (H_l and E_l): one lane per row walks snapshots [0, tau_max) (blockIdx.y == 0) or [T - tau_max, T)
// (blockIdx.y == 1) with L chains under wave-uniform tests, in the same segment partition.
#include <type_traits>

#include "time_rows.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxL = 8;
#ifndef DMDX_LAG_RING
#define DMDX_LAG_RING 16           // 8 / 16 / 32 were measured (scripts/bench_lagstats.py --alt-lib, MEASUREMENTS.md K26)
#endif
constexpr int kRing = DMDX_LAG_RING;   // W: snapshots a lane keeps in LDS (16 B x 256 lanes x 16 = 64 KiB: two workgroups / CU)
static_assert(kRing >= 1 && kRing <= 32 && (kRing & (kRing - 1)) == 0, "the ring is a power of two of at most 32 slots");
constexpr int kInFlight = 4;       // snapshot loads issued before their (1 + L) sequential adds (tier of 8: 2, and 1 at R = 1)

// The product chains of a launch, by value.  A lag of 0 is no chain: its pairs are the squares and P_0 is S, chain for
// chain, so the host strips it (zero_first) and the sums of S are stored twice.  tau[0 .. n) are the other lags,
// ascending; the rest of a tier is filled with tau[n - 1] (computed, never stored; 0 when n == 0).  The first n_near
// entries are served from the ring (0: none, and no LDS is asked for).
struct Lags {
  int32_t tau[kMaxL];
  int32_t n;
  int32_t zero_first;
  int32_t n_near;
  int32_t pre;                     // the largest lag the ring serves (<= kRing): what a segment re-reads before its start
};

// One lane: R consecutive rows from row r0 of xb.  Segments s = blockIdx.y, blockIdx.y + gridDim.y, ...: SPLIT stores every
// segment sum to ws[(s np + plane) m + row], np = 1 + L; otherwise gridDim.y is 1 and the lane adds them up itself.
template <int LT, int R, bool FULL, bool SPLIT, bool MU>
__device__ __forceinline__ void lag_rows(const float* __restrict__ xb, int64_t r0, int nr, int64_t m, int64_t T, int64_t ldx,
                                         const float* __restrict__ mup, const Lags& lg, int64_t seg, int64_t nseg,
                                         double* __restrict__ wsp, double* __restrict__ op, int64_t ldo,
                                         typename VecOf<R>::type* ring) {
  typedef typename VecOf<R>::type vec;
  const float* xp = xb + r0;
  auto ld = [&](const float* p) { return ld_rows<R, FULL>(p, nr); };
  double mud[R];
#pragma unroll
  for (int e = 0; e < R; ++e) mud[e] = (MU && e < nr) ? (double)mup[e] : 0.0;

  const int n_near = lg.n_near;
  const int64_t tau_max = lg.tau[LT - 1];
  const int np = 1 + lg.zero_first + lg.n;

  double tot[1 + LT][R], acc[1 + LT][R];
#pragma unroll
  for (int j = 0; j <= LT; ++j)
#pragma unroll
    for (int e = 0; e < R; ++e) tot[j][e] = 0.0;
  int64_t pf[LT];

  // pf[l]: the offset of this lane's rows in snapshot u - tau_l from X, kept per lane (the row offset is part of it, so it
  // is a vector register pair: as scalars the eight of them drove the compiler to spill SGPRs) and moved on with every
  // step; dereferenced only where u >= tau_l.  Snapshot u with its load v: the square, one product per chain that has a
  // partner (CHECK: test u >= tau, wave-uniform), then the ring slot of u -- after the reads: slot (u - kRing) mod kRing
  // is the one u overwrites
  auto step = [&](auto check, int64_t u, vec v) {
    constexpr bool CHECK = decltype(check)::value;
    double d[R];
#pragma unroll
    for (int e = 0; e < R; ++e) {
      d[e] = MU ? (double)v[e] - mud[e] : (double)v[e];
      const double q = d[e] * d[e];
      acc[0][e] = acc[0][e] + q;
    }
    const int su = (int)u & (kRing - 1);
#pragma unroll
    for (int l = 0; l < LT; ++l) {
      const int tau = lg.tau[l];
      if (!CHECK || u >= tau) {
        const vec ev = l < n_near ? ring[((su - tau) & (kRing - 1)) * 256] : ld(xb + pf[l]);
#pragma unroll
        for (int e = 0; e < R; ++e) {
          const double de = MU ? (double)ev[e] - mud[e] : (double)ev[e];
          const double q = de * d[e];                           // a rounded product of its own
          acc[1 + l][e] = acc[1 + l][e] + q;
        }
      }
    }
    if (n_near) ring[su * 256] = v;
#pragma unroll
    for (int l = 0; l < LT; ++l) pf[l] += ldx;
  };

  // plane 0 is S; with zero_first plane 1 (P of lag 0) is S again; chain l goes to plane 1 + zero_first + l
  auto put = [&](const double (&val)[1 + LT][R], double* o, int64_t ldp) {
#pragma unroll
    for (int e = 0; e < R; ++e)
      if (e < nr) {
        o[e] = val[0][e];
        if (lg.zero_first) o[ldp + e] = val[0][e];
      }
    o += (1 + lg.zero_first) * ldp;
#pragma unroll
    for (int l = 0; l < LT; ++l)
      if (l < lg.n) {
#pragma unroll
        for (int e = 0; e < R; ++e)
          if (e < nr) o[l * ldp + e] = val[1 + l][e];
      }
  };

  for (int64_t s = blockIdx.y; s < nseg; s += gridDim.y) {
    const int64_t a = s * seg;
    const int64_t b = T - a < seg ? T : a + seg;
#pragma unroll
    for (int j = 0; j <= LT; ++j)
#pragma unroll
      for (int e = 0; e < R; ++e) acc[j][e] = 0.0;

    // the walk form (gridDim.y == 1) has just left these snapshots in the ring and reads them again all the same: one
    // start for both forms; it costs pre / seg of a read, and the wrapper splits whenever there is more than one segment
    for (int64_t t = a - lg.pre < 0 ? 0 : a - lg.pre; t < a; ++t) ring[((int)t & (kRing - 1)) * 256] = ld(xp + t * ldx);

    int64_t t = a;
    const float* px = xp + a * ldx;
#pragma unroll
    for (int l = 0; l < LT; ++l) pf[l] = (a - lg.tau[l]) * ldx + r0;
    const int64_t head = tau_max < b ? tau_max : b;             // before it a chain may lack its partner: tested steps
    for (; t < head; ++t, px += ldx) step(std::true_type(), t, ld(px));
    constexpr int G = LT < 8 ? kInFlight : R > 1 ? kInFlight / 2 : 1;
    for (; t + G <= b; t += G, px += G * ldx) {
      vec v[G];
#pragma unroll
      for (int u = 0; u < G; ++u) v[u] = ld(px + u * ldx);
#pragma unroll
      for (int u = 0; u < G; ++u) step(std::false_type(), t + u, v[u]);
    }
    for (; t < b; ++t, px += ldx) step(std::false_type(), t, ld(px));     // the ragged end of a segment

    if (SPLIT) {
      put(acc, wsp + s * np * m, m);
    } else {
#pragma unroll
      for (int j = 0; j <= LT; ++j)
#pragma unroll
        for (int e = 0; e < R; ++e) tot[j][e] = tot[j][e] + acc[j][e];
    }
  }
  if (!SPLIT) put(tot, op, ldo);
}

// grid.x: chunks of 256 R rows; grid.y: segments (SPLIT; strided when there are more than gridDim.y) or 1.  R = 4 is
// launched only for a 16-byte aligned X with ldx % 4 == 0, the ragged last quad in a loop of its own; R = 1: one dword
// per lane.  Dynamic LDS: kRing x 256 vectors when a lag is served from the ring, nothing otherwise.
template <int LT, int R, bool SPLIT, bool MU>
__global__ __launch_bounds__(256) void lag_main_kernel(const float* __restrict__ X, int64_t m, int64_t T, int64_t ldx,
                                                       const float* __restrict__ mu, Lags lg, int64_t seg,
                                                       int64_t nseg, double* __restrict__ ws, double* __restrict__ out,
                                                       int64_t ldo) {
  typedef typename VecOf<R>::type vec;
  extern __shared__ __attribute__((aligned(16))) unsigned char lag_lds[];
  vec* ring = reinterpret_cast<vec*>(lag_lds) + threadIdx.x;
  const int64_t r0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * R;
  if (r0 >= m) return;
  const int nr = (m - r0) < R ? (int)(m - r0) : R;
  double* wsp = SPLIT ? ws + r0 : nullptr;
  const float* mup = MU ? mu + r0 : nullptr;
  if (nr == R)
    lag_rows<LT, R, true, SPLIT, MU>(X, r0, nr, m, T, ldx, mup, lg, seg, nseg, wsp, out + r0, ldo, ring);
  else
    lag_rows<LT, R, false, SPLIT, MU>(X, r0, nr, m, T, ldx, mup, lg, seg, nseg, wsp, out + r0, ldo, ring);
}

// The tail of the split form: one lane per (row, plane) adds the segment sums in ascending order.
__global__ __launch_bounds__(256) void lag_combine_kernel(const double* __restrict__ ws, int64_t m, int np, int64_t nseg,
                                                          double* __restrict__ out, int64_t ldo) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int j = blockIdx.y;
  if (i >= m) return;
  double tot = 0.0;
  for (int64_t s = 0; s < nseg; ++s) tot = tot + ws[(s * np + j) * m + i];
  out[j * ldo + i] = tot;
}

// H_l = segsum(sq, [0, tau_l)) (blockIdx.y == 0) and E_l = segsum(sq, [T - tau_l, T)) (blockIdx.y == 1): one lane per
// row walks the tau_max snapshots of its end.  Chain l takes snapshot t when the index set of its lag holds it -- the
// same test for every lane.  At every segment boundary all chains are closed: the segments without an index add +0.0
// to a total that is never -0.0.
template <bool MU>
__global__ __launch_bounds__(256) void lag_edge_kernel(const float* __restrict__ X, int64_t m, int64_t T, int64_t ldx,
                                                       const float* __restrict__ mu, Lags lg, int L, int64_t seg,
                                                       double* __restrict__ out, int64_t ldo) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const bool tail = blockIdx.y != 0;
  const int64_t tau_max = lg.tau[kMaxL - 1];                    // (the tier is filled with the last lag)
  const int64_t t0 = tail ? T - tau_max : 0, t1 = tail ? T : tau_max;
  const double mud = MU ? (double)mu[i] : 0.0;
  double tot[kMaxL], acc[kMaxL];
#pragma unroll
  for (int l = 0; l < kMaxL; ++l) tot[l] = acc[l] = 0.0;
  for (int64_t t = t0; t < t1; ++t) {
    if (t > t0 && t % seg == 0) {
#pragma unroll
      for (int l = 0; l < kMaxL; ++l) {
        tot[l] = tot[l] + acc[l];
        acc[l] = 0.0;
      }
    }
    const double x = (double)X[t * ldx + i];
    const double d = MU ? x - mud : x;
    const double q = d * d;
#pragma unroll
    for (int l = 0; l < kMaxL; ++l) {
      const int64_t tau = lg.tau[l];
      if (tail ? t >= T - tau : t < tau) acc[l] = acc[l] + q;
    }
  }
  double* o = out + (int64_t)(1 + (tail ? 2 : 1) * L) * ldo + i;
#pragma unroll
  for (int l = 0; l < kMaxL; ++l)
    if (l < L) o[l * ldo] = tot[l] + acc[l];
}

// nseg (1 + L) m doubles
size_t lag_workspace_bytes(int64_t m, int64_t T, int64_t L, int64_t seg) {
  return saturating_bytes((T + seg - 1) / seg, 1 + L, m, sizeof(double));
}

template <int LT, int R, bool MU>
void launch_main_form(dim3 grid, size_t lds, hipStream_t st, const float* X, int64_t m, int64_t T, int64_t ldx,
                      const float* mu, const Lags& lg, int64_t seg, int64_t nseg, double* ws, double* out,
                      int64_t ldo) {
  if (lds > 64 * 1024) {                                        // (a ring of 32: more dynamic LDS than a launch gets unasked)
    const void* fn = ws ? (const void*)lag_main_kernel<LT, R, true, MU> : (const void*)lag_main_kernel<LT, R, false, MU>;
    (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  }
  if (ws)
    hipLaunchKernelGGL((lag_main_kernel<LT, R, true, MU>), grid, dim3(256), lds, st, X, m, T, ldx, mu, lg, seg, nseg, ws,
                       out, ldo);
  else
    hipLaunchKernelGGL((lag_main_kernel<LT, R, false, MU>), grid, dim3(256), lds, st, X, m, T, ldx, mu, lg, seg, nseg, ws,
                       out, ldo);
}

template <int LT>
int launch_main(const float* X, int64_t m, int64_t T, int64_t ldx, const float* mu, const Lags& lg, int L, int64_t seg,
                int64_t nseg, double* ws, double* out, int64_t ldo, hipStream_t st) {
  const RowLanes ln = row_lanes(X, ldx, m, nseg, ws != nullptr);
  const dim3 grid(ln.gx, ln.gy);
  const size_t lds = lg.n_near ? (size_t)kRing * 256 * (ln.quad ? 16 : 4) : 0;
  if (ln.quad) {
    if (mu) launch_main_form<LT, 4, true>(grid, lds, st, X, m, T, ldx, mu, lg, seg, nseg, ws, out, ldo);
    else launch_main_form<LT, 4, false>(grid, lds, st, X, m, T, ldx, mu, lg, seg, nseg, ws, out, ldo);
  } else {
    if (mu) launch_main_form<LT, 1, true>(grid, lds, st, X, m, T, ldx, mu, lg, seg, nseg, ws, out, ldo);
    else launch_main_form<LT, 1, false>(grid, lds, st, X, m, T, ldx, mu, lg, seg, nseg, ws, out, ldo);
  }
  DMDX_LAUNCH_CHECK();
  if (ws) {
    hipLaunchKernelGGL(lag_combine_kernel, dim3((unsigned)((m + 255) / 256), (unsigned)(1 + L)), dim3(256), 0, st, ws, m,
                       1 + L, nseg, out, ldo);
    DMDX_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace

extern "C" int dmdx_lag_moments_max_lags(void) { return kMaxL; }

extern "C" int dmdx_lag_moments_ring(void) { return kRing; }

extern "C" size_t dmdx_lag_moments_workspace_bytes(int64_t m, int64_t T, int64_t L, int64_t seg) {
  if (m < 0 || T < 0 || L < 1 || L > kMaxL || seg < 1 || m >= kMaxSize || T >= kMaxSize || seg >= kMaxSize) return 0;
  return lag_workspace_bytes(m, T, L, seg);
}

extern "C" int dmdx_lag_moments_f32(const float* X, int64_t m, int64_t T, int64_t ldx, const float* mu, const int32_t* lags,
                                    int L, int64_t seg, double* out, int64_t ldo, int flags, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  DMDX_CHECK_ARG(L >= 1 && L <= kMaxL, "lag_moments: L=%d outside 1..%d", L, kMaxL);
  DMDX_CHECK_ARG(lags, "lag_moments: null lags");
  DMDX_CHECK_ARG((flags & ~1) == 0, "lag_moments: flags=0x%x: only bit 0 (reload every lag) is defined", (unsigned)flags);
  DMDX_CHECK_ARG(seg >= 1 && seg < kMaxSize, "lag_moments: seg=%lld outside 1..2^31-1", (long long)seg);
  if (int rc = check_block("lag_moments", m, T, {{"ldx", ldx}, {"ldo", ldo}}, {X, mu}, {out, workspace})) return rc;
  for (int l = 0; l < L; ++l) {
    DMDX_CHECK_ARG(lags[l] >= 0 && (l == 0 || lags[l] > lags[l - 1]),
                   "lag_moments: lags must be >= 0 and strictly ascending (lags[%d]=%d)", l, (int)lags[l]);
    DMDX_CHECK_ARG(T == 0 || lags[l] < T, "lag_moments: lags[%d]=%d >= T=%lld", l, (int)lags[l], (long long)T);
  }
  DMDX_CHECK_ARG((X && out) || m == 0 || T == 0, "lag_moments: null X or out");
  // X against the (1 + 3L) planes of out, stated as a two-column fp32 matrix of the same extent: 2 ((1 + 3L - 1) ldo + m)
  // floats = (2 - 1) ldy + m with ldy = 6 L ldo + m
  if (int rc = check_ranges("lag_moments", X, T, ldx, (const float*)out, 2, 6 * (int64_t)L * ldo + m, m, false)) return rc;
  if (int rc = check_workspace("lag_moments", workspace, workspace_bytes, lag_workspace_bytes(m, T, L, seg))) return rc;
  if (m == 0 || T == 0) return 0;

  Lags all, lg;                                                 // every lag (the edge pass); the product chains
  all.n = L, all.zero_first = all.n_near = all.pre = 0;
  for (int l = 0; l < kMaxL; ++l) all.tau[l] = lags[l < L ? l : L - 1];
  lg.zero_first = lags[0] == 0;
  lg.n = L - lg.zero_first;
  const int LT = lg.n <= 1 ? 1 : lg.n == 2 ? 2 : lg.n <= 4 ? 4 : 8;
  lg.n_near = lg.pre = 0;
  for (int l = 0; l < kMaxL; ++l) {
    lg.tau[l] = lg.n ? lags[lg.zero_first + (l < lg.n ? l : lg.n - 1)] : 0;
    if (lg.n && l < LT && !(flags & 1) && lg.tau[l] <= kRing) lg.n_near = l + 1, lg.pre = lg.tau[l];
  }
  const int64_t nseg = (T + seg - 1) / seg;
  double* ws = (double*)workspace;
  hipStream_t st = (hipStream_t)stream;
  int rc;
  switch (LT) {
    case 1: rc = launch_main<1>(X, m, T, ldx, mu, lg, L, seg, nseg, ws, out, ldo, st); break;
    case 2: rc = launch_main<2>(X, m, T, ldx, mu, lg, L, seg, nseg, ws, out, ldo, st); break;
    case 4: rc = launch_main<4>(X, m, T, ldx, mu, lg, L, seg, nseg, ws, out, ldo, st); break;
    default: rc = launch_main<8>(X, m, T, ldx, mu, lg, L, seg, nseg, ws, out, ldo, st); break;
  }
  if (rc) return rc;
  const dim3 grid((unsigned)((m + 255) / 256), 2u);
  if (mu)
    hipLaunchKernelGGL(lag_edge_kernel<true>, grid, dim3(256), 0, st, X, m, T, ldx, mu, all, L, seg, out, ldo);
  else
    hipLaunchKernelGGL(lag_edge_kernel<false>, grid, dim3(256), 0, st, X, m, T, ldx, mu, all, L, seg, out, ldo);
  DMDX_LAUNCH_CHECK();
  return 0;
}
