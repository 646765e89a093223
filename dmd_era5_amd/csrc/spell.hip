// K27: spell and exceedance-count indices of every grid point of one row block: per threshold j and period p the number
// of valid snapshots and of events, the number of qualifying runs of events and the snapshots in them, the longest run,
// and where the first qualifying run starts and the last one ends (TX90p, WSDI, CDD, onset and end of a season's heat
// waves, first and last frost; dmd_era5_amd/spells.py).
//
// The contract is tests/spell_ref.py, a plain loop over time, held element for element.  The state of the scan along
// time -- the open run -- is not a sum: K21 / K26 add the partials of their time split, here they are MERGED in order.
// The frame is time_rows.h's ("The period frame of K27 and K29"): pieces of `seg` snapshots, a record per
// piece, a combine kernel, a walk form.  The record of a piece, per (row, j): valid, events, the head run (from the
// piece's start to its first non-event), the tail run (from its last non-event to its end) and what the runs strictly
// inside closed to (count, snapshots, longest, first start, last end).  The merge, in ascending order:   all events: the
// piece extends the carry;   otherwise: carry + head is a run and is closed, the interior is added, the carry becomes
// the tail;   the carry is closed at the period's end.  All results are integers: both forms and every seg give the
// same ones.
//
// A lane keeps J R state machines in registers (J is a template tier).  The thresholds of a lane, h[j][e] = thr[(j S + slot[t]) ldthr + row], are loaded again only when
// slot[t] changes -- the same snapshot for every lane, so the test is wave-uniform.  No atomics, no LDS, no barrier.
#include "time_rows.h"

namespace {

constexpr int kMaxThr = DMDX_SPELL_MAX_THR;
constexpr int kNQ = DMDX_SPELL_NQ;
constexpr int kWords = DMDX_SPELL_WS_WORDS;

// The record of a piece, as word w of ws[((piece J + j) kWords + w) m + row].
enum { W_VALID, W_EVENT, W_HEAD, W_TAIL, W_NSPELL, W_INSPELL, W_LONGEST, W_FIRST, W_LAST };
static_assert(W_LAST + 1 == kWords, "a record is DMDX_SPELL_WS_WORDS words");

// What travels by value: the periods and their pieces (time_rows.h), the shortest qualifying run and the direction.
struct Periods : PeriodCuts {
  int32_t min_len[kMaxThr];
  uint32_t above;
};

// The seven results of one (row, j, period) and the open run.  close(len, end): a run of len >= 0 snapshots whose last
// one is `end` (relative to the period's start) has ended; len == 0 is no run and changes nothing (min_len >= 1).
struct Tally {
  int32_t nv, ne, ns, nin, longest, last, run;
  uint32_t first;                           // -1 is the largest value: the starts ascend, so the first one is the minimum
  __device__ __forceinline__ void reset() { nv = ne = ns = nin = longest = run = 0, last = -1, first = ~0u; }
  __device__ __forceinline__ void close(int32_t len, int32_t end, int32_t min_len) {
    longest = len > longest ? len : longest;
    const bool q = len >= min_len;
    ns += q ? 1 : 0;
    nin += q ? len : 0;
    const uint32_t start = (uint32_t)(end - len + 1);
    first = (q && start < first) ? start : first;
    last = q ? end : last;
  }
};

// One lane: rows r0 .. r0 + nr - 1.  SPLIT: the pieces s = blockIdx.y, blockIdx.y + gridDim.y, ... of the call, a record
// each; otherwise the periods one after another, their planes stored as they end.
template <int J, int R, bool FULL, bool SPLIT>
__device__ __forceinline__ void spell_rows(const float* __restrict__ X, int64_t r0, int nr, int64_t m, int64_t ldx,
                                           const float* __restrict__ thr, int64_t ldthr, int64_t S,
                                           const int32_t* __restrict__ slot, const Periods& pd, int64_t seg,
                                           int32_t* __restrict__ ws, int32_t* __restrict__ out, int64_t ldo) {
  typedef typename VecOf<R>::type vec;
  const float* xp = X + r0;
  auto ld = [&](const float* p) { return ld_rows<R, FULL>(p, nr); };

  Tally ty[J][R];
  int32_t head[J][R];                       // SPLIT: the head run, -1 until the piece's first non-event
  float h[J][R];
  int32_t cur = 0;
  bool have = false;                        // h holds the thresholds of slot `cur`

  // the thresholds of a snapshot in slot sl: the same snapshot for every lane
  auto thresholds = [&](int32_t sl) {
    if (have && sl == cur) return;
    cur = sl, have = true;
    const bool in = sl >= 0 && sl < S;      // no slot: nothing of thr is read, no snapshot of it is valid
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const float* tp = thr + ((int64_t)j * S + (in ? sl : 0)) * ldthr + r0;
#pragma unroll
      for (int e = 0; e < R; ++e) h[j][e] = (in && e < nr) ? tp[e] : __uint_as_float(kQuietNaN);
    }
  };

  // snapshot t of a period, `rel` snapshots after its start
  auto step = [&](int32_t rel, vec v) {
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const bool above = (pd.above >> j) & 1u;
      const int32_t ml = pd.min_len[j];
#pragma unroll
      for (int e = 0; e < R; ++e) {
        const float x = v[e], hh = h[j][e];
        const bool fin = finite_bits(x);
        const bool valid = fin && hh == hh;
        const bool ev = fin && (above ? x > hh : x < hh);
        Tally& s = ty[j][e];
        s.nv += valid ? 1 : 0;
        s.ne += ev ? 1 : 0;
        if (SPLIT) {
          const bool first_gap = !ev && head[j][e] < 0;
          head[j][e] = first_gap ? s.run : head[j][e];
          s.close((ev || first_gap) ? 0 : s.run, rel - 1, ml);
        } else {
          s.close(ev ? 0 : s.run, rel - 1, ml);
        }
        s.run = ev ? s.run + 1 : 0;
      }
    }
  };

  // snapshots [a, b) of X, the first of them `rel` after its period's start
  auto scan = [&](int64_t a, int64_t b, int32_t rel) {
    const float* px = xp + a * ldx;
    int64_t t = a;
    if (!slot) thresholds(0);
    for (; t + 4 <= b; t += 4, px += 4 * ldx, rel += 4) {
      vec v[4];
      int32_t sl[4];                        // the labels with the loads: no step waits for its own
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = ld(px + u * ldx);
#pragma unroll
      for (int u = 0; u < 4; ++u) sl[u] = slot ? slot[t + u] : 0;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (slot) thresholds(sl[u]);
        step(rel + u, v[u]);
      }
    }
    for (; t < b; ++t, px += ldx, ++rel) {
      if (slot) thresholds(slot[t]);
      step(rel, ld(px));
    }
  };

  if (SPLIT) {
    const int64_t N = pd.piece0[pd.P];
    int p = 0;
    for (int64_t s = blockIdx.y; s < N; s += gridDim.y) {
      p = pd.period_of(s, p);
      const int64_t off = (s - pd.piece0[p]) * seg;             // the piece's first snapshot, after the period's start
      const int64_t a = pd.bound[p] + off;
      const int64_t b = pd.bound[p + 1] - a < seg ? pd.bound[p + 1] : a + seg;
#pragma unroll
      for (int j = 0; j < J; ++j)
#pragma unroll
        for (int e = 0; e < R; ++e) ty[j][e].reset(), head[j][e] = -1;
      scan(a, b, (int32_t)off);
      int32_t* w = ws + s * J * kWords * m + r0;
#pragma unroll
      for (int j = 0; j < J; ++j, w += kWords * m)
#pragma unroll
        for (int e = 0; e < R; ++e)
          if (e < nr) {
            const Tally& q = ty[j][e];
            w[W_VALID * m + e] = q.nv, w[W_EVENT * m + e] = q.ne;
            w[W_HEAD * m + e] = head[j][e] < 0 ? q.run : head[j][e];      // all events: head = tail = the piece
            w[W_TAIL * m + e] = q.run;
            w[W_NSPELL * m + e] = q.ns, w[W_INSPELL * m + e] = q.nin, w[W_LONGEST * m + e] = q.longest;
            w[W_FIRST * m + e] = (int32_t)q.first, w[W_LAST * m + e] = q.last;
          }
    }
  } else {
    for (int p = 0; p < pd.P; ++p) {
      const int64_t a = pd.bound[p], b = pd.bound[p + 1];
#pragma unroll
      for (int j = 0; j < J; ++j)
#pragma unroll
        for (int e = 0; e < R; ++e) ty[j][e].reset();
      scan(a, b, 0);
#pragma unroll
      for (int j = 0; j < J; ++j) {
        int32_t* o = out + ((int64_t)j * kNQ * pd.P + p) * ldo + r0;
        const int64_t pl = (int64_t)pd.P * ldo;
#pragma unroll
        for (int e = 0; e < R; ++e)
          if (e < nr) {
            Tally& q = ty[j][e];
            q.close(q.run, (int32_t)(b - a) - 1, pd.min_len[j]);
            o[e] = q.nv, o[pl + e] = q.ne, o[2 * pl + e] = q.ns, o[3 * pl + e] = q.nin, o[4 * pl + e] = q.longest;
            o[5 * pl + e] = (int32_t)q.first, o[6 * pl + e] = q.last;
          }
      }
    }
  }
}

// grid.x: chunks of 256 R rows; grid.y: pieces (SPLIT; strided when there are more than gridDim.y) or 1.  R = 4 is
// launched only for a 16-byte aligned X with ldx % 4 == 0, the ragged last quad element by element.
template <int J, int R, bool SPLIT>
__global__ __launch_bounds__(256) void spell_scan_kernel(const float* __restrict__ X, int64_t m, int64_t ldx,
                                                         const float* __restrict__ thr, int64_t ldthr, int64_t S,
                                                         const int32_t* __restrict__ slot, Periods pd, int64_t seg,
                                                         int32_t* __restrict__ ws, int32_t* __restrict__ out,
                                                         int64_t ldo) {
  const int64_t r0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * R;
  if (r0 >= m) return;
  const int nr = (m - r0) < R ? (int)(m - r0) : R;
  if (nr == R)
    spell_rows<J, R, true, SPLIT>(X, r0, nr, m, ldx, thr, ldthr, S, slot, pd, seg, ws, out, ldo);
  else
    spell_rows<J, R, false, SPLIT>(X, r0, nr, m, ldx, thr, ldthr, S, slot, pd, seg, ws, out, ldo);
}

// The tail of the split form: one lane per (row, j = blockIdx.y, period = blockIdx.z) merges the records in order.
__global__ __launch_bounds__(256) void spell_combine_kernel(const int32_t* __restrict__ ws, int64_t m, int J, Periods pd,
                                                            int64_t seg, int32_t* __restrict__ out, int64_t ldo) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int j = blockIdx.y, p = blockIdx.z;
  if (i >= m) return;
  const int32_t ml = pd.min_len[j];
  const int64_t plen = (int64_t)pd.bound[p + 1] - pd.bound[p];
  Tally t;
  t.reset();                                                     // t.run is the carry: the run open at a piece's start
  int64_t off = 0;
  for (int64_t s = pd.piece0[p]; s < pd.piece0[p + 1]; ++s, off += seg) {
    const int32_t* w = ws + (s * J + j) * kWords * m + i;
    const int32_t len = (int32_t)(plen - off < seg ? plen - off : seg);
    const int32_t ne = w[W_EVENT * m];
    t.nv += w[W_VALID * m];
    t.ne += ne;
    if (ne == len) {
      t.run += len;
      continue;
    }
    const int32_t head = w[W_HEAD * m];
    t.close(t.run + head, (int32_t)off + head - 1, ml);
    const int32_t lg = w[W_LONGEST * m], l = w[W_LAST * m];
    const uint32_t f = (uint32_t)w[W_FIRST * m];
    t.ns += w[W_NSPELL * m];
    t.nin += w[W_INSPELL * m];
    t.longest = lg > t.longest ? lg : t.longest;
    t.first = f < t.first ? f : t.first;
    t.last = l >= 0 ? l : t.last;
    t.run = w[W_TAIL * m];
  }
  t.close(t.run, (int32_t)plen - 1, ml);
  int32_t* o = out + ((int64_t)j * kNQ * pd.P + p) * ldo + i;
  const int64_t pl = (int64_t)pd.P * ldo;
  o[0] = t.nv, o[pl] = t.ne, o[2 * pl] = t.ns, o[3 * pl] = t.nin, o[4 * pl] = t.longest, o[5 * pl] = (int32_t)t.first, o[6 * pl] = t.last;
}

// N J m kWords int32
size_t spell_workspace_bytes(int64_t m, int64_t N, int J) { return saturating_bytes(N, J, m, kWords * sizeof(int32_t)); }

template <int J> struct Scan {
  template <int R, bool SPLIT> static constexpr auto kernel() { return spell_scan_kernel<J, R, SPLIT>; }
};

}  // namespace

extern "C" int dmdx_spell_max_thresholds(void) { return kMaxThr; }

extern "C" int dmdx_spell_max_periods(void) { return kMaxPeriods; }

extern "C" size_t dmdx_spell_workspace_bytes(int64_t m, const int32_t* bounds, int P, int J, int64_t seg) {
  if (m < 0 || m >= kMaxSize || J < 1 || J > kMaxThr || seg < 1 || seg >= kMaxSize || !bounds_ok(bounds, P, -1)) return 0;
  return spell_workspace_bytes(m, count_pieces(bounds, P, 1, seg, nullptr), J);
}

extern "C" int dmdx_spell_f32(const float* X, int64_t m, int64_t T, int64_t ldx, const float* thr, int64_t ldthr, int J,
                              int64_t S, const int32_t* slot, unsigned above_mask, const int32_t* min_len,
                              const int32_t* bounds, int P, int64_t seg, int32_t* out, int64_t ldo, int flags,
                              void* workspace, size_t workspace_bytes, void* stream) {
  DMDX_CHECK_ARG(J >= 1 && J <= kMaxThr, "spell: J=%d outside 1..%d", J, kMaxThr);
  DMDX_CHECK_ARG(S >= 1 && S < kMaxSize && (int64_t)J * S < kMaxSize, "spell: S=%lld < 1, or S or J S >= 2^31", (long long)S);
  DMDX_CHECK_ARG(P >= 1 && P <= kMaxPeriods, "spell: P=%d outside 1..%d", P, kMaxPeriods);
  DMDX_CHECK_ARG(bounds && min_len, "spell: null bounds or min_len");
  DMDX_CHECK_ARG(flags == 0, "spell: flags=0x%x: no flag is defined", (unsigned)flags);
  DMDX_CHECK_ARG(seg >= 1 && seg < kMaxSize, "spell: seg=%lld outside 1..2^31-1", (long long)seg);
  DMDX_CHECK_ARG((above_mask >> J) == 0, "spell: above_mask=0x%x has a bit at or above J=%d", above_mask, J);
  for (int j = 0; j < J; ++j) DMDX_CHECK_ARG(min_len[j] >= 1, "spell: min_len[%d]=%d < 1", j, (int)min_len[j]);
  if (int rc = check_block("spell", m, T, {{"ldx", ldx}, {"ldthr", ldthr}, {"ldo", ldo}}, {X, thr, slot, out, workspace}))
    return rc;
  DMDX_CHECK_ARG(bounds_ok(bounds, P, T), "spell: bounds must be strictly ascending inside [0, T=%lld]", (long long)T);
  DMDX_CHECK_ARG((X && thr && out) || m == 0, "spell: null X, thr or out");
  // out is J 7 P rows of ldo int32, thr J S rows of ldthr floats: as fp32 matrices of m rows against X and each other
  const int64_t To = (int64_t)J * kNQ * P, Tt = (int64_t)J * S;
  if (int rc = check_ranges("spell", X, T, ldx, (const float*)out, To, ldo, m, false)) return rc;
  if (int rc = check_ranges("spell", thr, Tt, ldthr, (const float*)out, To, ldo, m, false)) return rc;

  Periods pd;
  const int64_t N = fill_periods(pd, bounds, P, 1, seg);
  if (int rc = check_workspace("spell", workspace, workspace_bytes, spell_workspace_bytes(m, N, J))) return rc;
  if (m == 0) return 0;
  for (int j = 0; j < kMaxThr; ++j) pd.min_len[j] = min_len[j < J ? j : J - 1];
  pd.above = above_mask;

  int32_t* ws = (int32_t*)workspace;
  hipStream_t st = (hipStream_t)stream;
  const RowLanes ln = row_lanes(X, ldx, m, N, ws != nullptr);
  switch (J) {
    case 1: launch_lanes<Scan<1>>(ln, ws, st, X, m, ldx, thr, ldthr, S, slot, pd, seg, ws, out, ldo); break;
    case 2: launch_lanes<Scan<2>>(ln, ws, st, X, m, ldx, thr, ldthr, S, slot, pd, seg, ws, out, ldo); break;
    case 3: launch_lanes<Scan<3>>(ln, ws, st, X, m, ldx, thr, ldthr, S, slot, pd, seg, ws, out, ldo); break;
    default: launch_lanes<Scan<4>>(ln, ws, st, X, m, ldx, thr, ldthr, S, slot, pd, seg, ws, out, ldo); break;
  }
  DMDX_LAUNCH_CHECK();
  if (ws) {
    hipLaunchKernelGGL(spell_combine_kernel, dim3((unsigned)((m + 255) / 256), (unsigned)J, (unsigned)P), dim3(256), 0, st, ws,
                       m, J, pd, seg, out, ldo);
    DMDX_LAUNCH_CHECK();
  }
  return 0;
}
