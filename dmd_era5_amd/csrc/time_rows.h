// What the kernels over (time, rows) blocks share -- unpack.hip (K14), clim.hip (K18), treg.hip (K21), tfilt.hip (K22),
// and the frame of the scans along time with a lane of R rows: lagmom.hip (K26), spell.hip (K27), pstat.hip (K29).
// Device: the head-shifted chunk of a lane, the quad load that looks at its address, the row lane and its loader, the
// periods of a launch.  Host (free of HIP: tests/host/check_ranges_main.cpp compiles it alone): checks, launch geometry,
// the pieces of the periods, workspace sizes.  What is not here: MEASUREMENTS.md, "time-axis" and "period frame".
#pragma once

#include <stddef.h>

#include <initializer_list>

#include "dmdx_check.h"

#ifdef __HIPCC__
#include "dmdx_common.h"
namespace {
// The head shift ("The head-shifted chunks of the time-axis kernels").  A kernel that writes a (time, rows)
// block gives each lane CHUNK consecutive rows of snapshot t, and the chunks start `head` elements before row 0, head =
// the elements of row 0 past a 16-byte boundary: every full chunk of the output is then 16-byte aligned, whatever base
// and leading dimension are.  The chunks at both ends of a snapshot are ragged: rows lo .. hi - 1 of the chunk exist.
template <int CHUNK>
struct Quad {
  int64_t r;        // the first row of the chunk; negative in the chunk that holds row 0 when head > 0
  int head, lo, hi; // lo, hi: set by clip()
  __device__ __forceinline__ bool past(int64_t m) const { return r >= m; }    // no row of the snapshot in this chunk
  __device__ __forceinline__ void clip(int64_t m) {
    lo = r < 0 ? (int)(-r) : 0;
    hi = m - r < CHUNK ? (int)(m - r) : CHUNK;
  }
  __device__ __forceinline__ bool full() const { return lo == 0 && hi == CHUNK; }
};

// chunk c of the snapshot with row 0 at `row`; then `if (q.past(m)) continue; q.clip(m);` (fewer steps compile otherwise)
template <int CHUNK>
__device__ __forceinline__ Quad<CHUNK> quad_at(const float* row, int64_t c) {
  Quad<CHUNK> q;
  q.head = (int)(((uintptr_t)row >> 2) & 3u);
  q.r = c * CHUNK - q.head;
  return q;
}

// 4 floats at p, all of them present: one 16-byte load where the address allows it, dword by dword otherwise
__device__ __forceinline__ f32x4 ldq_any(const float* p) {
  if (((uintptr_t)p & 15u) == 0) return *reinterpret_cast<const f32x4*>(p);
  f32x4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = p[e];
  return v;
}

// The row lane of lagmom.hip, spell.hip and pstat.hip: R consecutive rows (4 with 16-byte loads, 1 with dword loads),
// the snapshot of a lane one vector.  FULL: all R rows exist; otherwise the first nr, the rest read as 0.
template <int R> struct VecOf { typedef float type __attribute__((ext_vector_type(R))); };

template <int R, bool FULL>
__device__ __forceinline__ typename VecOf<R>::type ld_rows(const float* p, int nr) {
  typedef typename VecOf<R>::type vec;
  if (FULL) return *reinterpret_cast<const vec*>(p);
  vec v;
#pragma unroll
  for (int e = 0; e < R; ++e) v[e] = e < nr ? p[e] : 0.f;
  return v;
}
}  // namespace
#endif  // __HIPCC__

namespace {
// chunks of CHUNK rows that cover m rows under any head shift (+ 3: the shift itself)
template <int CHUNK> inline int64_t chunks_of(int64_t m) { return (m + 3 + CHUNK - 1) / CHUNK; }

// grid.y for n snapshots (or runs, slots, segments); the kernels stride over what is beyond
inline unsigned grid_rows(int64_t n) { return (unsigned)(n < 65535 ? n : 65535); }

// The row-lane launch ("The period frame"): grid.x chunks of 256 R rows, R = 4 only for a 16-byte aligned X
// with ldx % 4 == 0; grid.y the pieces of the time split, or 1 for the walk form.
struct RowLanes { bool quad; unsigned gx, gy; };
inline RowLanes row_lanes(const float* X, int64_t ldx, int64_t m, int64_t pieces, bool split) {
  const bool quad = ((uintptr_t)X & 15u) == 0 && ldx % 4 == 0;
  const int64_t rows_per_wg = quad ? 1024 : 256;
  return {quad, (unsigned)((m + rows_per_wg - 1) / rows_per_wg), split ? grid_rows(pieces) : 1u};
}

// a b c d bytes, every factor >= 0: the product is formed in 128 bits (factors below 2^31, 2^31, 2^31 and 2^7 as here
// cannot wrap it) and saturates to SIZE_MAX
inline size_t saturating_bytes(int64_t a, int64_t b, int64_t c, int64_t d) {
  const unsigned __int128 n = (unsigned __int128)(uint64_t)a * (uint64_t)b * (uint64_t)c * (uint64_t)d;
  return n > (unsigned __int128)SIZE_MAX ? SIZE_MAX : (size_t)n;
}

// a workspace, where one is given, holds what the split form needs (SIZE_MAX: more than any workspace holds)
inline int check_workspace(const char* who, const void* workspace, size_t workspace_bytes, size_t need) {
  DMDX_CHECK_ARG(!workspace || (need != SIZE_MAX && workspace_bytes >= need), "%s: workspace of %zu bytes, %zu needed", who,
                 workspace_bytes, need);
  return 0;
}

// The periods of a launch (spell.hip, pstat.hip): period p is the snapshots [bound[p], bound[p + 1]) and is cut from its
// own start into the pieces piece0[p] .. piece0[p + 1] - 1; piece0[P] = N.  They travel by value as the head of a
// kernel's own struct, padded to the maximum with their last entry.
constexpr int kMaxPeriods = 128;
static_assert(DMDX_SPELL_MAX_PERIODS == kMaxPeriods && DMDX_PSTAT_MAX_PERIODS == kMaxPeriods,
              "PeriodCuts is one struct for K27 and K29: both take the same number of periods per launch");
struct PeriodCuts {
  int32_t bound[kMaxPeriods + 1];
  int32_t piece0[kMaxPeriods + 1];
  int32_t P;
#ifdef __HIPCC__
  // the period of piece s, from the period p of an earlier piece (s ascends: p only moves forward)
  __device__ __forceinline__ int period_of(int64_t s, int p) const {
    while (piece0[p + 1] <= s) ++p;
    return p;
  }
#endif
};

// 0 <= b_0 < b_1 < ... < b_P (<= T when T >= 0 is given)
inline bool bounds_ok(const int32_t* bounds, int P, int64_t T) {
  if (!bounds || P < 1 || P > kMaxPeriods || bounds[0] < 0) return false;
  for (int p = 0; p < P; ++p)
    if (bounds[p + 1] <= bounds[p]) return false;
  return T < 0 || bounds[P] <= T;
}

// N = sum over the periods of ceil(days / seg), days = ceil(length / group): at most b_P - b_0 < 2^31
inline int64_t count_pieces(const int32_t* bounds, int P, int64_t group, int64_t seg, int32_t* piece0) {
  int64_t n = 0;
  for (int p = 0; p < P; ++p) {
    if (piece0) piece0[p] = (int32_t)n;
    const int64_t days = ((int64_t)bounds[p + 1] - bounds[p] + group - 1) / group;
    n += (days + seg - 1) / seg;
  }
  if (piece0) piece0[P] = (int32_t)n;
  return n;
}

// pd from checked bounds -> N
inline int64_t fill_periods(PeriodCuts& pd, const int32_t* bounds, int P, int64_t group, int64_t seg) {
  const int64_t N = count_pieces(bounds, P, group, seg, pd.piece0);
  for (int p = 0; p <= kMaxPeriods; ++p) {
    pd.bound[p] = bounds[p < P ? p : P];
    if (p > P) pd.piece0[p] = pd.piece0[P];
  }
  pd.P = P;
  return N;
}

struct NamedLd { const char* name; int64_t ld; };

// An m x T block and what is addressed with it: m and T in [0, 2^31), every leading dimension in [m, 2^31), the
// pointers to 4-byte (p4) and 8-byte (p8) elements aligned to them (null passes: presence is the caller's check).
inline int check_block(const char* who, int64_t m, int64_t T, std::initializer_list<NamedLd> lds,
                       std::initializer_list<const void*> p4, std::initializer_list<const void*> p8 = {}) {
  DMDX_CHECK_ARG(m >= 0 && T >= 0, "%s: negative size (m=%lld T=%lld)", who, (long long)m, (long long)T);
  DMDX_CHECK_ARG(m < kMaxSize && T < kMaxSize, "%s: a size >= 2^31 (m=%lld T=%lld)", who, (long long)m, (long long)T);
  for (const NamedLd& l : lds)
    DMDX_CHECK_ARG(l.ld >= m && l.ld < kMaxSize, "%s: %s=%lld < m=%lld or >= 2^31", who, l.name, (long long)l.ld,
                   (long long)m);
  for (const void* p : p4) DMDX_CHECK_ARG(((uintptr_t)p & 3u) == 0, "%s: a pointer is not aligned to its element", who);
  for (const void* p : p8) DMDX_CHECK_ARG(((uintptr_t)p & 7u) == 0, "%s: a pointer is not aligned to its element", who);
  return 0;
}

// The address ranges of X (m x T, ldx) and Y (m x T_y, ldy), fp32, every size inside check_block's limits.  First the
// extents as plain integers: (T - 1) ld + m can reach 2^62 elements and 4 times that wraps, so 2^60 elements or more
// are refused.  Then: the ranges are disjoint, or, where allowed, Y is X itself with the same leading dimension.
inline int check_ranges(const char* who, const float* X, int64_t T, int64_t ldx, const float* Y, int64_t T_y, int64_t ldy,
                        int64_t m, bool allow_in_place) {
  const int64_t nx = T < 1 ? 0 : (T - 1) * ldx + m, ny = T_y < 1 ? 0 : (T_y - 1) * ldy + m;
  DMDX_CHECK_ARG(nx < (int64_t(1) << 60) && ny < (int64_t(1) << 60),
                 "%s: (T - 1) ldx + m or (T_y - 1) ldy + m >= 2^60 elements: no address range holds that", who);
  if (m == 0 || T == 0 || T_y == 0) return 0;                  // an empty block overlaps nothing
  if (allow_in_place && Y == X && ldy == ldx) return 0;
  const uintptr_t x0 = (uintptr_t)X, y0 = (uintptr_t)Y;         // (differences: nothing wraps, whatever the pointers)
  DMDX_CHECK_ARG(y0 >= x0 ? y0 - x0 >= 4 * (uintptr_t)nx : x0 - y0 >= 4 * (uintptr_t)ny, "%s: X and Y overlap (%s)", who,
                 allow_in_place ? "only Y == X with ldy == ldx runs in place" : "there is no in-place form");
  return 0;
}

}  // namespace

#ifdef __HIPCC__
namespace {
// The scan kernel of a row-lane launch: K::kernel<R, SPLIT>() with R from the lanes and SPLIT where there is a workspace.
template <class K, class... Args>
void launch_lanes(const RowLanes& ln, bool split, hipStream_t st, Args... args) {
  const dim3 grid(ln.gx, ln.gy), block(256);
  if (ln.quad && split) hipLaunchKernelGGL((K::template kernel<4, true>()), grid, block, 0, st, args...);
  else if (ln.quad) hipLaunchKernelGGL((K::template kernel<4, false>()), grid, block, 0, st, args...);
  else if (split) hipLaunchKernelGGL((K::template kernel<1, true>()), grid, block, 0, st, args...);
  else hipLaunchKernelGGL((K::template kernel<1, false>()), grid, block, 0, st, args...);
}
}  // namespace
#endif  // __HIPCC__
