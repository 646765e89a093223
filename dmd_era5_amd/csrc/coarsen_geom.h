// The host half of K23 (coarsen.hip), free of HIP: tests/host/coarsen_checks_main.cpp compiles it alone.  The argument
// checks of dmdx_coarsen_f32 on plain integers and the launch geometry.
#pragma once

#include "time_rows.h"

// lanes per workgroup: one output cell of a snapshot each, four at fx = 2 (tests/test_gpu_coarsen.py reads both numbers)
#define DMDX_COARSEN_BLOCK 256

namespace {

constexpr int kCoarsenMaxFactor = 64;

// The cells of a coarse row one lane forms, by the walk FX the launch takes (0: element by element; 2, 4, 8: fx itself):
// at fx = 2 the output is a quarter of the input, and four cells are one 16-byte store.  __host__ __device__ under
// hipcc, plain under a host compiler.
#ifdef __HIPCC__
__host__ __device__
#endif
constexpr int coarsen_cells_per_lane(int FX) { return FX == 2 ? 4 : 1; }

// lanes that cover the NLON cells of one coarse row (at fx = 2 the last lane of a row holds 1 .. 4 cells)
inline int64_t coarsen_lanes_per_row(int64_t NLON, int FX) {
  return (NLON + coarsen_cells_per_lane(FX) - 1) / coarsen_cells_per_lane(FX);
}

// grid.x of K23: workgroups that cover the lanes of one snapshot
inline int64_t coarsen_blocks(int64_t lanes) { return (lanes + DMDX_COARSEN_BLOCK - 1) / DMDX_COARSEN_BLOCK; }

// check_ranges (time_rows.h) for two blocks of different heights and no in-place form: X holds T snapshots of mx
// floats, Y holds T_y snapshots of my floats.  The same order: extents of 2^60 elements or more are refused first
// (4 times that wraps), then any overlap of the two address ranges.
inline int check_ranges(const char* who, const float* X, int64_t T, int64_t ldx, int64_t mx, const float* Y, int64_t T_y,
                        int64_t ldy, int64_t my) {
  const int64_t nx = (T < 1 || mx < 1) ? 0 : (T - 1) * ldx + mx, ny = (T_y < 1 || my < 1) ? 0 : (T_y - 1) * ldy + my;
  DMDX_CHECK_ARG(nx < (int64_t(1) << 60) && ny < (int64_t(1) << 60),
                 "%s: the extent of X or of Y is >= 2^60 elements: no address range holds that", who);
  if (nx == 0 || ny == 0) return 0;                             // an empty block overlaps nothing
  const uintptr_t x0 = (uintptr_t)X, y0 = (uintptr_t)Y;         // (differences: nothing wraps, whatever the pointers)
  DMDX_CHECK_ARG(y0 >= x0 ? y0 - x0 >= 4 * (uintptr_t)nx : x0 - y0 >= 4 * (uintptr_t)ny,
                 "%s: X and Y overlap (there is no in-place form)", who);
  return 0;
}

// Every refusal of dmdx_coarsen_f32 (include/dmdx.h, K23), before any HIP call.  0: the call may run (or is empty).
inline int check_coarsen(const float* X, int64_t T, int64_t ldx, int64_t P, int64_t ldp, int64_t nlat, int64_t nlon,
                         const double* w, int64_t fy, int64_t fx, int64_t lat0, int64_t lon0, int64_t NLAT, int64_t NLON,
                         double min_frac, const float* Y, int64_t ldy, int64_t ldq) {
  const char* who = "coarsen";
  DMDX_CHECK_ARG(X && w && Y, "%s: null pointer", who);
  DMDX_CHECK_ARG(T >= 0 && P >= 0 && nlat >= 0 && nlon >= 0 && NLAT >= 0 && NLON >= 0 && ldx >= 0 && ldp >= 0 && ldy >= 0 &&
                     ldq >= 0,
                 "%s: negative size (T=%lld P=%lld nlat=%lld nlon=%lld NLAT=%lld NLON=%lld ldx=%lld ldp=%lld ldy=%lld ldq=%lld)",
                 who, (long long)T, (long long)P, (long long)nlat, (long long)nlon, (long long)NLAT, (long long)NLON,
                 (long long)ldx, (long long)ldp, (long long)ldy, (long long)ldq);
  DMDX_CHECK_ARG(T < kMaxSize && P < kMaxSize && nlat < kMaxSize && nlon < kMaxSize && NLAT < kMaxSize && NLON < kMaxSize &&
                     ldx < kMaxSize && ldp < kMaxSize && ldy < kMaxSize && ldq < kMaxSize,
                 "%s: a size or a leading dimension >= 2^31", who);
  DMDX_CHECK_ARG(fy >= 1 && fy <= kCoarsenMaxFactor && fx >= 1 && fx <= kCoarsenMaxFactor, "%s: fy=%lld or fx=%lld outside 1..%d",
                 who, (long long)fy, (long long)fx, kCoarsenMaxFactor);
  DMDX_CHECK_ARG(lat0 >= 0 && lon0 >= 0, "%s: lat0=%lld or lon0=%lld negative", who, (long long)lat0, (long long)lon0);
  // (everything below 2^31, the factors at most 64: nothing here leaves 64 bits)
  DMDX_CHECK_ARG(lat0 <= nlat && NLAT * fy <= nlat - lat0, "%s: the cells end at latitude row lat0 + NLAT fy = %lld > nlat=%lld",
                 who, (long long)(lat0 + NLAT * fy), (long long)nlat);
  DMDX_CHECK_ARG(lon0 <= nlon && NLON * fx <= nlon - lon0, "%s: the cells end at longitude lon0 + NLON fx = %lld > nlon=%lld", who,
                 (long long)(lon0 + NLON * fx), (long long)nlon);
  const int64_t plane = nlat * nlon, cells = NLAT * NLON;      // < 2^62
  DMDX_CHECK_ARG(ldp >= plane, "%s: ldp=%lld < nlat nlon = %lld", who, (long long)ldp, (long long)plane);
  DMDX_CHECK_ARG(ldq >= cells, "%s: ldq=%lld < NLAT NLON = %lld", who, (long long)ldq, (long long)cells);
  const int64_t mx = P < 1 ? 0 : (P - 1) * ldp + plane, my = P < 1 ? 0 : (P - 1) * ldq + cells;   // < 2^63: ld, plane < 2^31
  DMDX_CHECK_ARG(ldx >= mx, "%s: ldx=%lld < (P - 1) ldp + nlat nlon = %lld", who, (long long)ldx, (long long)mx);
  DMDX_CHECK_ARG(ldy >= my, "%s: ldy=%lld < (P - 1) ldq + NLAT NLON = %lld", who, (long long)ldy, (long long)my);
  DMDX_CHECK_ARG(min_frac >= 0.0 && min_frac <= 1.0, "%s: min_frac=%g outside [0, 1]", who, min_frac);   // (a NaN fails both)
  DMDX_CHECK_ARG(((uintptr_t)X & 3u) == 0 && ((uintptr_t)Y & 3u) == 0 && ((uintptr_t)w & 7u) == 0,
                 "%s: a pointer is not aligned to its element", who);
  return check_ranges(who, X, T, ldx, mx, Y, cells == 0 ? 0 : T, ldy, my);   // no cells: Y is empty, whatever ldq is
}

}  // namespace
