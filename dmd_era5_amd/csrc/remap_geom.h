// The host half of K28 (remap.hip), free of HIP: remap_host.cpp compiles it alone into libdmdx_host.so, where
// tests/test_host_remap_checks.py calls it.  The argument checks of dmdx_remap_f32 on plain integers and the launch
// geometry.  What the checks cannot see is the content of the six tables, which live on the device: the kernel clamps
// what it reads from them (remap.hip, "Memory").
#pragma once

#include "coarsen_geom.h"

// lanes per workgroup: one target cell of a snapshot each
#define DMDX_REMAP_BLOCK 256

namespace {

constexpr int kRemapMaxSpan = 64;

// grid.x of K28: workgroups that cover the cells of one snapshot
inline int64_t remap_blocks(int64_t cells) { return (cells + DMDX_REMAP_BLOCK - 1) / DMDX_REMAP_BLOCK; }

// Every refusal of dmdx_remap_f32 (include/dmdx.h, K28), before any HIP call.  0: the call may run (or is empty).
inline int check_remap(const float* X, int64_t T, int64_t ldx, int64_t P, int64_t ldp, int64_t nlat, int64_t nlon,
                       const int32_t* iy0, const int32_t* ny, const double* wy, int64_t SY, const int32_t* jx0,
                       const int32_t* nx, const double* wx, int64_t SX, int64_t NLAT, int64_t NLON, double min_frac,
                       const float* Y, int64_t ldy, int64_t ldq) {
  const char* who = "remap";
  DMDX_CHECK_ARG(X && iy0 && ny && wy && jx0 && nx && wx && Y, "%s: null pointer", who);
  DMDX_CHECK_ARG(T >= 0 && P >= 0 && nlat >= 0 && nlon >= 0 && NLAT >= 0 && NLON >= 0 && ldx >= 0 && ldp >= 0 && ldy >= 0 &&
                     ldq >= 0,
                 "%s: negative size (T=%lld P=%lld nlat=%lld nlon=%lld NLAT=%lld NLON=%lld ldx=%lld ldp=%lld ldy=%lld ldq=%lld)",
                 who, (long long)T, (long long)P, (long long)nlat, (long long)nlon, (long long)NLAT, (long long)NLON,
                 (long long)ldx, (long long)ldp, (long long)ldy, (long long)ldq);
  DMDX_CHECK_ARG(T < kMaxSize && P < kMaxSize && nlat < kMaxSize && nlon < kMaxSize && NLAT < kMaxSize && NLON < kMaxSize &&
                     ldx < kMaxSize && ldp < kMaxSize && ldy < kMaxSize && ldq < kMaxSize,
                 "%s: a size or a leading dimension >= 2^31", who);
  DMDX_CHECK_ARG(SY >= 1 && SY <= kRemapMaxSpan && SX >= 1 && SX <= kRemapMaxSpan, "%s: SY=%lld or SX=%lld outside 1..%d", who,
                 (long long)SY, (long long)SX, kRemapMaxSpan);
  const int64_t plane = nlat * nlon, cells = NLAT * NLON;      // < 2^62
  // (a cell of an empty plane has nothing to read: the clamps of the kernel need one row and one column)
  DMDX_CHECK_ARG(cells == 0 || plane > 0, "%s: %lld x %lld cells of an empty plane (nlat=%lld nlon=%lld)", who, (long long)NLAT,
                 (long long)NLON, (long long)nlat, (long long)nlon);
  DMDX_CHECK_ARG(ldp >= plane, "%s: ldp=%lld < nlat nlon = %lld", who, (long long)ldp, (long long)plane);
  DMDX_CHECK_ARG(ldq >= cells, "%s: ldq=%lld < NLAT NLON = %lld", who, (long long)ldq, (long long)cells);
  const int64_t mx = P < 1 ? 0 : (P - 1) * ldp + plane, my = P < 1 ? 0 : (P - 1) * ldq + cells;   // < 2^63: ld, plane < 2^31
  DMDX_CHECK_ARG(ldx >= mx, "%s: ldx=%lld < (P - 1) ldp + nlat nlon = %lld", who, (long long)ldx, (long long)mx);
  DMDX_CHECK_ARG(ldy >= my, "%s: ldy=%lld < (P - 1) ldq + NLAT NLON = %lld", who, (long long)ldy, (long long)my);
  DMDX_CHECK_ARG(min_frac >= 0.0 && min_frac <= 1.0, "%s: min_frac=%g outside [0, 1]", who, min_frac);   // (a NaN fails both)
  DMDX_CHECK_ARG(((uintptr_t)X & 3u) == 0 && ((uintptr_t)Y & 3u) == 0 && ((uintptr_t)iy0 & 3u) == 0 && ((uintptr_t)ny & 3u) == 0 &&
                     ((uintptr_t)jx0 & 3u) == 0 && ((uintptr_t)nx & 3u) == 0 && ((uintptr_t)wy & 7u) == 0 && ((uintptr_t)wx & 7u) == 0,
                 "%s: a pointer is not aligned to its element", who);
  return check_ranges(who, X, T, ldx, mx, Y, cells == 0 ? 0 : T, ldy, my);   // no cells: Y is empty, whatever ldq is
}

}  // namespace
