// What the kernels over (time, rows) blocks share -- unpack.hip (K14), clim.hip (K18), treg.hip (K21), tfilt.hip (K22).
// Device: the head-shifted chunk of a lane, the quad load that looks at its address.  Host (free of HIP: tests/host/
// check_ranges_main.cpp compiles it alone): checks and launch geometry.  What is not here: MEASUREMENTS.md, "time-axis".
#pragma once

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
}  // namespace
#endif  // __HIPCC__

namespace {
// chunks of CHUNK rows that cover m rows under any head shift (+ 3: the shift itself)
template <int CHUNK> inline int64_t chunks_of(int64_t m) { return (m + 3 + CHUNK - 1) / CHUNK; }

// grid.y for n snapshots (or runs, slots, segments); the kernels stride over what is beyond
inline unsigned grid_rows(int64_t n) { return (unsigned)(n < 65535 ? n : 65535); }
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
