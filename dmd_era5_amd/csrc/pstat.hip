// K29: per-period extremes and totals of a daily statistic of every grid point of one row block: the snapshots of a
// period are grouped into days of `group` snapshots, a day value is formed from the finite ones (sum, mean, max, min,
// range), a running sum over `window` valid days never crosses a period, and per period the count, the largest and the
// smallest running value with their day, the total, and the total and count beyond a per-row threshold come out (TXx,
// TNn, DTR, Rx1day, Rx5day, PRCPTOT, SDII, R95pTOT, degree days; dmd_era5_amd/extremes.py).
//
// The contract is tests/pstat_ref.py, a plain loop over time, held bit for bit.  The frame is time_rows.h's (DESIGN.md,
// "The period frame of K27 and K29"): pieces of `seg` DAYS, a record per piece, a combine kernel, a walk form.  A piece is
// scanned after the up to window - 1 days before it inside its period, which only fill the ring; its record, per row, is
// the eight planes of the piece alone, its partial sums from +0.0.  The merge, in ascending order: counts added, a strict
// compare for the extremes (the earlier piece wins a tie), tot = tot + acc.  The walk form closes a piece every seg days.
// Every running value is recomputed from the ring in one fixed order, so it does not depend on where a piece starts:
// both forms give the same bits.
//
// Per row: the day accumulators (s, hi, lo,
// c), a ring of the last W day values (W = window is a template parameter: the ring is rotated by moving registers once
// per day and never indexed at run time) with a bit mask of their validity, and the outer words.  kAhead snapshot loads
// are in flight ahead of their steps in a queue that is rotated the same way.  inner, the comparison and thr == NULL (a
// NaN threshold: no event) are wave-uniform run-time values: they are looked at once per day.  Only fp64 additions, one
// subtraction and one division: nothing a compiler could contract.  No atomics, no LDS, no barrier.
#include "time_rows.h"

namespace {

constexpr int kMaxWindow = DMDX_PSTAT_MAX_WINDOW;
constexpr int kNQ = DMDX_PSTAT_NQ;
constexpr int kAhead = 4;                   // snapshot loads in flight per lane

// The planes, and the words of a piece's record at ws[(piece kNQ + q) m + row].
enum { Q_N, Q_MAX, Q_ARGMAX, Q_MIN, Q_ARGMIN, Q_TOTAL, Q_ETOTAL, Q_ECOUNT };
static_assert(Q_ECOUNT + 1 == kNQ, "a record is DMDX_PSTAT_NQ doubles");

// What travels by value: the periods and their pieces (time_rows.h) and the scalars of the call.
struct Periods : PeriodCuts {
  int32_t group, inner, min_count;
  uint32_t flags;
};

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7FF8000000000000ll); }

// The outer words of one row: of a piece (split: a record), or of a period (walk: tot and etot collect the pieces).
struct Outer {
  double mx, mn, acc, eacc, tot, etot;
  int32_t n, amx, amn, ec;
  __device__ __forceinline__ void reset() { mx = mn = acc = eacc = tot = etot = 0.0, n = ec = 0, amx = amn = -1; }
  // the running value r of day k exists; ev: it is an event
  __device__ __forceinline__ void take(double r, int32_t k, bool ev) {
    const bool up = n == 0 || r > mx, dn = n == 0 || r < mn;
    mx = up ? r : mx, amx = up ? k : amx;
    mn = dn ? r : mn, amn = dn ? k : amn;
    n += 1;
    acc = acc + r;
    eacc = ev ? eacc + r : eacc;
    ec += ev ? 1 : 0;
  }
  __device__ __forceinline__ void close_piece() { tot = tot + acc, etot = etot + eacc, acc = 0.0, eacc = 0.0; }
};

// One lane: rows r0 .. r0 + nr - 1.  SPLIT: the pieces s = blockIdx.y, blockIdx.y + gridDim.y, ... of the call, a record
// each; otherwise the periods one after another, their planes stored as they end.
template <int W, int R, bool FULL, bool SPLIT>
__device__ __forceinline__ void pstat_rows(const float* __restrict__ X, int64_t r0, int nr, int64_t m, int64_t ldx,
                                           const float* __restrict__ thr, const Periods& pd, int64_t seg,
                                           double* __restrict__ ws, double* __restrict__ out, int64_t ldo) {
  typedef typename VecOf<R>::type vec;
  const float* xp = X + r0;
  auto ld = [&](const float* p) { return ld_rows<R, FULL>(p, nr); };

  const int32_t g = pd.group, inner = pd.inner, min_count = pd.min_count;
  const bool below = pd.flags & DMDX_PSTAT_BELOW, incl = pd.flags & DMDX_PSTAT_INCLUSIVE;
  constexpr uint32_t kAll = (1u << W) - 1u;

  double h[R];                              // the threshold of the row; NaN: no event
#pragma unroll
  for (int e = 0; e < R; ++e) h[e] = (thr && e < nr) ? (double)thr[r0 + e] : quiet_nan();

  double s[R], ring[W][R];
  float hi[R], lo[R];
  int32_t c[R];
  uint32_t vm[R];                           // bit u: the day u before the newest is valid
  Outer o[R];

  auto new_day = [&]() {
#pragma unroll
    for (int e = 0; e < R; ++e) s[e] = 0.0, hi[e] = lo[e] = 0.f, c[e] = 0;
  };

  auto step = [&](vec v) {
#pragma unroll
    for (int e = 0; e < R; ++e) {
      const float x = v[e];
      const bool fin = finite_bits(x);
      const bool first = c[e] == 0;
      s[e] = fin ? s[e] + (double)x : s[e];
      hi[e] = (fin && (first || x > hi[e])) ? x : hi[e];
      lo[e] = (fin && (first || x < lo[e])) ? x : lo[e];
      c[e] += fin ? 1 : 0;
    }
  };

  // day k of the period has ended; count: it belongs to the piece (and is not one of the days before it)
  auto day_end = [&](int32_t k, bool count) {
#pragma unroll
    for (int e = 0; e < R; ++e) {
      double d;
      switch (inner) {
        case DMDX_PSTAT_SUM: d = s[e]; break;
        case DMDX_PSTAT_MEAN: d = s[e] / (double)c[e]; break;
        case DMDX_PSTAT_MAX: d = (double)hi[e]; break;
        case DMDX_PSTAT_MIN: d = (double)lo[e]; break;
        default: d = (double)hi[e] - (double)lo[e]; break;
      }
#pragma unroll
      for (int u = 0; u + 1 < W; ++u) ring[u][e] = ring[u + 1][e];
      ring[W - 1][e] = d;
      vm[e] = ((vm[e] << 1) | (c[e] >= min_count ? 1u : 0u)) & kAll;
      double r = ring[0][e];
#pragma unroll
      for (int u = 1; u < W; ++u) r = r + ring[u][e];
      const bool exists = count && vm[e] == kAll;
      const double hh = h[e];
      const bool ev = below ? (incl ? r <= hh : r < hh) : (incl ? r >= hh : r > hh);
      if (exists) o[e].take(r, k, ev);
    }
    new_day();
  };

  // days [kfirst, k1) of the period that starts at snapshot b0 and ends before b1; the days before k0 only fill the ring
  auto scan = [&](int64_t b0, int64_t b1, int64_t kfirst, int64_t k0, int64_t k1) {
    const int64_t a = b0 + kfirst * g;
    const int64_t z = b1 - b0 <= k1 * g ? b1 : b0 + k1 * g;
#pragma unroll
    for (int e = 0; e < R; ++e) {
      vm[e] = 0;
#pragma unroll
      for (int u = 0; u < W; ++u) ring[u][e] = 0.0;
    }
    new_day();
    const float* px = xp + a * ldx;
    vec q[kAhead];
#pragma unroll
    for (int u = 0; u < kAhead; ++u) {
      if (a + u < z) q[u] = ld(px + u * ldx);
      else q[u] = vec(0.f);
    }
    int32_t j = 0, kin = 0;
    int64_t k = kfirst;
#pragma nounroll
    for (int64_t t = a; t < z; ++t, px += ldx) {
      const vec v = q[0];
#pragma unroll
      for (int u = 0; u + 1 < kAhead; ++u) q[u] = q[u + 1];
      if (t + kAhead < z) q[kAhead - 1] = ld(px + kAhead * ldx);
      step(v);
      if (++j == g || t + 1 == z) {
        day_end((int32_t)k, k >= k0);
        j = 0;
        ++k;
        if (!SPLIT && (++kin == seg || t + 1 == z)) {
          kin = 0;
#pragma unroll
          for (int e = 0; e < R; ++e) o[e].close_piece();
        }
      }
    }
  };

  // the eight words of row e at dst[q stride + e]
  auto emit = [&](double* dst, int64_t stride, double tot, double etot, int e) {
    const Outer& w = o[e];
    const bool any = w.n > 0;
    dst[Q_N * stride + e] = (double)w.n;
    dst[Q_MAX * stride + e] = any ? w.mx : quiet_nan();
    dst[Q_ARGMAX * stride + e] = (double)w.amx;
    dst[Q_MIN * stride + e] = any ? w.mn : quiet_nan();
    dst[Q_ARGMIN * stride + e] = (double)w.amn;
    dst[Q_TOTAL * stride + e] = tot;
    dst[Q_ETOTAL * stride + e] = etot;
    dst[Q_ECOUNT * stride + e] = (double)w.ec;
  };

  if (SPLIT) {
    const int64_t N = pd.piece0[pd.P];
    int p = 0;
    for (int64_t sx = blockIdx.y; sx < N; sx += gridDim.y) {
      p = pd.period_of(sx, p);
      const int64_t b0 = pd.bound[p], b1 = pd.bound[p + 1];
      const int64_t days = (b1 - b0 + g - 1) / g;
      const int64_t k0 = (sx - pd.piece0[p]) * seg;             // < days: the piece exists
      const int64_t k1 = days - k0 < seg ? days : k0 + seg;
      const int64_t kfirst = k0 < W - 1 ? 0 : k0 - (W - 1);
#pragma unroll
      for (int e = 0; e < R; ++e) o[e].reset();
      scan(b0, b1, kfirst, k0, k1);
      double* w = ws + sx * kNQ * m + r0;
#pragma unroll
      for (int e = 0; e < R; ++e)
        if (e < nr) emit(w, m, o[e].acc, o[e].eacc, e);
    }
  } else {
    for (int p = 0; p < pd.P; ++p) {
      const int64_t b0 = pd.bound[p], b1 = pd.bound[p + 1];
      const int64_t days = (b1 - b0 + g - 1) / g;
#pragma unroll
      for (int e = 0; e < R; ++e) o[e].reset();
      scan(b0, b1, 0, 0, days);
      double* w = out + (int64_t)p * ldo + r0;
#pragma unroll
      for (int e = 0; e < R; ++e)
        if (e < nr) emit(w, (int64_t)pd.P * ldo, o[e].tot, o[e].etot, e);
    }
  }
}

// grid.x: chunks of 256 R rows; grid.y: pieces (SPLIT; strided when there are more than gridDim.y) or 1.  R = 4 is
// launched only for a 16-byte aligned X with ldx % 4 == 0, the ragged last quad element by element.
template <int W, int R, bool SPLIT>
__global__ __launch_bounds__(256) void pstat_scan_kernel(const float* __restrict__ X, int64_t m, int64_t ldx,
                                                         const float* __restrict__ thr, Periods pd, int64_t seg,
                                                         double* __restrict__ ws, double* __restrict__ out, int64_t ldo) {
  const int64_t r0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * R;
  if (r0 >= m) return;
  const int nr = (m - r0) < R ? (int)(m - r0) : R;
  if (nr == R)
    pstat_rows<W, R, true, SPLIT>(X, r0, nr, m, ldx, thr, pd, seg, ws, out, ldo);
  else
    pstat_rows<W, R, false, SPLIT>(X, r0, nr, m, ldx, thr, pd, seg, ws, out, ldo);
}

// The tail of the split form: one lane per (row, period = blockIdx.y) merges the records in ascending order.
__global__ __launch_bounds__(256) void pstat_combine_kernel(const double* __restrict__ ws, int64_t m, Periods pd,
                                                            double* __restrict__ out, int64_t ldo) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int p = blockIdx.y;
  if (i >= m) return;
  double n = 0.0, mx = 0.0, amx = -1.0, mn = 0.0, amn = -1.0, tot = 0.0, etot = 0.0, ec = 0.0;
  for (int64_t sx = pd.piece0[p]; sx < pd.piece0[p + 1]; ++sx) {
    const double* w = ws + sx * kNQ * m + i;
    const double rn = w[Q_N * m];
    if (rn > 0.0) {
      const double rmx = w[Q_MAX * m], rmn = w[Q_MIN * m];
      const bool up = n == 0.0 || rmx > mx, dn = n == 0.0 || rmn < mn;
      mx = up ? rmx : mx, amx = up ? w[Q_ARGMAX * m] : amx;
      mn = dn ? rmn : mn, amn = dn ? w[Q_ARGMIN * m] : amn;
      n += rn;
    }
    tot = tot + w[Q_TOTAL * m];
    etot = etot + w[Q_ETOTAL * m];
    ec += w[Q_ECOUNT * m];
  }
  double* o = out + (int64_t)p * ldo + i;
  const int64_t pl = (int64_t)pd.P * ldo;
  o[Q_N * pl] = n;
  o[Q_MAX * pl] = n > 0.0 ? mx : quiet_nan();
  o[Q_ARGMAX * pl] = amx;
  o[Q_MIN * pl] = n > 0.0 ? mn : quiet_nan();
  o[Q_ARGMIN * pl] = amn;
  o[Q_TOTAL * pl] = tot;
  o[Q_ETOTAL * pl] = etot;
  o[Q_ECOUNT * pl] = ec;
}

// N kNQ m doubles
size_t pstat_workspace_bytes(int64_t m, int64_t N) { return saturating_bytes(N, kNQ, m, sizeof(double)); }

template <int W> struct Scan {
  template <int R, bool SPLIT> static constexpr auto kernel() { return pstat_scan_kernel<W, R, SPLIT>; }
};

}  // namespace

extern "C" int dmdx_period_stats_max_window(void) { return kMaxWindow; }

extern "C" int dmdx_period_stats_max_periods(void) { return kMaxPeriods; }

extern "C" size_t dmdx_period_stats_workspace_bytes(int64_t m, const int32_t* bounds, int P, int64_t group, int64_t seg) {
  if (m < 0 || m >= kMaxSize || group < 1 || group >= kMaxSize || seg < 1 || seg >= kMaxSize || !bounds_ok(bounds, P, -1))
    return 0;
  return pstat_workspace_bytes(m, count_pieces(bounds, P, group, seg, nullptr));
}

extern "C" int dmdx_period_stats_f32(const float* X, int64_t m, int64_t T, int64_t ldx, const int32_t* bounds, int P,
                                     int64_t group, int inner, int window, int64_t min_count, const float* thr, int64_t seg,
                                     double* out, int64_t ldo, unsigned flags, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  DMDX_CHECK_ARG(P >= 1 && P <= kMaxPeriods, "period_stats: P=%d outside 1..%d", P, kMaxPeriods);
  DMDX_CHECK_ARG(bounds, "period_stats: null bounds");
  DMDX_CHECK_ARG(group >= 1 && group < kMaxSize, "period_stats: group=%lld outside 1..2^31-1", (long long)group);
  DMDX_CHECK_ARG(inner >= DMDX_PSTAT_SUM && inner <= DMDX_PSTAT_RANGE, "period_stats: inner=%d outside 0..4", inner);
  DMDX_CHECK_ARG(window >= 1 && window <= kMaxWindow, "period_stats: window=%d outside 1..%d", window, kMaxWindow);
  DMDX_CHECK_ARG(min_count >= 1 && min_count <= group, "period_stats: min_count=%lld outside 1..group=%lld",
                 (long long)min_count, (long long)group);
  DMDX_CHECK_ARG(seg >= 1 && seg < kMaxSize, "period_stats: seg=%lld outside 1..2^31-1", (long long)seg);
  DMDX_CHECK_ARG((flags & ~(DMDX_PSTAT_BELOW | DMDX_PSTAT_INCLUSIVE)) == 0, "period_stats: flags=0x%x has an undefined bit",
                 flags);
  if (int rc = check_block("period_stats", m, T, {{"ldx", ldx}, {"ldo", ldo}}, {X, thr}, {out, workspace})) return rc;
  DMDX_CHECK_ARG(bounds_ok(bounds, P, T), "period_stats: bounds must be strictly ascending inside [0, T=%lld]", (long long)T);
  DMDX_CHECK_ARG((X && out) || m == 0, "period_stats: null X or out");
  // X and thr against the 8 P planes of out, stated as a two-column fp32 matrix of the same extent:
  // 2 ((8 P - 1) ldo + m) floats = (2 - 1) ldy + m with ldy = 2 (8 P - 1) ldo + m
  const int64_t ldy = 2 * ((int64_t)kNQ * P - 1) * ldo + m;
  if (int rc = check_ranges("period_stats", X, T, ldx, (const float*)out, 2, ldy, m, false)) return rc;
  if (thr)
    if (int rc = check_ranges("period_stats", thr, 1, m, (const float*)out, 2, ldy, m, false)) return rc;

  Periods pd;
  const int64_t N = fill_periods(pd, bounds, P, group, seg);
  if (int rc = check_workspace("period_stats", workspace, workspace_bytes, pstat_workspace_bytes(m, N))) return rc;
  if (m == 0) return 0;
  pd.group = (int32_t)group, pd.inner = inner, pd.min_count = (int32_t)min_count, pd.flags = flags;

  double* ws = (double*)workspace;
  hipStream_t st = (hipStream_t)stream;
  const RowLanes ln = row_lanes(X, ldx, m, N, ws != nullptr);
  switch (window) {
    case 1: launch_lanes<Scan<1>>(ln, ws, st, X, m, ldx, thr, pd, seg, ws, out, ldo); break;
    case 2: launch_lanes<Scan<2>>(ln, ws, st, X, m, ldx, thr, pd, seg, ws, out, ldo); break;
    case 3: launch_lanes<Scan<3>>(ln, ws, st, X, m, ldx, thr, pd, seg, ws, out, ldo); break;
    case 4: launch_lanes<Scan<4>>(ln, ws, st, X, m, ldx, thr, pd, seg, ws, out, ldo); break;
    case 5: launch_lanes<Scan<5>>(ln, ws, st, X, m, ldx, thr, pd, seg, ws, out, ldo); break;
    case 6: launch_lanes<Scan<6>>(ln, ws, st, X, m, ldx, thr, pd, seg, ws, out, ldo); break;
    case 7: launch_lanes<Scan<7>>(ln, ws, st, X, m, ldx, thr, pd, seg, ws, out, ldo); break;
    default: launch_lanes<Scan<8>>(ln, ws, st, X, m, ldx, thr, pd, seg, ws, out, ldo); break;
  }
  DMDX_LAUNCH_CHECK();
  if (ws) {
    hipLaunchKernelGGL(pstat_combine_kernel, dim3((unsigned)((m + 255) / 256), (unsigned)P), dim3(256), 0, st, ws, m, pd, out,
                       ldo);
    DMDX_LAUNCH_CHECK();
  }
  return 0;
}
