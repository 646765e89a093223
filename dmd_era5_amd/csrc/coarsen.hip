// K23: the area-weighted block mean of the snapshots over fy x fx cells of the latitude / longitude grid, on the device.
//
// Layout.  X is a row block: snapshot t at X + t ldx.  A snapshot holds P planes (variable x level), plane p at p ldp,
// ldp >= nlat nlon (the slack is pad, never read); inside a plane latitude row i and longitude j sit at i nlon + j.  Y is
// laid out the same way: Y[t ldy + p ldq + I NLON + J], ldq >= NLAT NLON.  Output cell (I, J) covers the fine rows
// lat0 + I fy .. + fy - 1 and the longitudes lon0 + J fx .. + fx - 1: whole cells only, what lies outside them is not
// looked at.  w: one fp64 weight per fine latitude row of the plane.
//
// Arithmetic (the contract of tests/coarsen_ref.py, held bit for bit): all fp64, never an FMA (contraction is off for
// the whole file).  Per snapshot, plane and cell
//     num = den = full = +0.0
//     for a = 0 .. fy - 1 ascending, i = lat0 + I fy + a:
//         r = +0.0, c = 0;  for b = 0 .. fx - 1 ascending: x = X[t, p, i, lon0 + J fx + b];
//                           if (!skipna || finite(x)) { r = r + fp64(x); c = c + 1 }
//         num = num + w[i] * r;  den = den + w[i] * fp64(c);  full = full + w[i] * fp64(fx)      (products rounded)
//     Y = (den == 0 || den < min_frac * full) ? quiet NaN (0x7fc00000) : fp32(num / den)          (one rounding to fp32)
// finite(x) is K20's test of the bits (an exponent of all ones is not finite).
//
// Lanes.  One lane per output cell -- per four neighbouring cells of a coarse row at fx = 2, where the output is a
// quarter of the input and its stores count; grid.x over the lanes of a snapshot in the order of Y, grid.y over the
// snapshots (strided beyond 65535).  A wave holds 64 (256) consecutive J of a coarse row (where the row does not end
// inside the wave): for every fine row its loads cover 64 fx (512) contiguous floats and its store is 256 (1024)
// contiguous bytes.  A lane reads its floats of a fine row with one (fx = 4) or two (fx = 2, 8) 16-byte loads where the
// addresses allow it, and element by element otherwise and for every other fx; the four cells of fx = 2 leave as one
// 16-byte store where their address allows it, the last 1 .. 3 cells of a coarse row dword by dword: the same floats in
// the same order, the same bits.  No atomics, no workspace, no synchronisation: the launch geometry is not part of the
// result.  What was measured, and the lane shapes that were dropped: MEASUREMENTS.md, "K23".
//
// Memory: only elements of X inside some cell are read, only w[lat0 .. lat0 + NLAT fy), and only the logical
// P NLAT NLON x T elements of Y are written.  Refusals: check_coarsen, coarsen_geom.h.
#include "coarsen_geom.h"

#pragma clang fp contract(off)

namespace {

// DMDX_COARSEN_VEC=0 builds the element-by-element walk alone (the A/B of MEASUREMENTS.md "K23"); never the product
#ifndef DMDX_COARSEN_VEC
#define DMDX_COARSEN_VEC 1
#endif

constexpr int kBlock = DMDX_COARSEN_BLOCK;

// N values in ascending longitude -> r (their fp64 sum from +0.0) and c (how many were added)
template <int N, bool SKIPNA>
__device__ __forceinline__ void chain(const float* v, double& r, int& c) {
  r = 0.0;
  c = 0;
#pragma unroll
  for (int b = 0; b < N; ++b)
    if (!SKIPNA || finite_bits(v[b])) {
      r = r + (double)v[b];
      c += 1;
    }
}

// The floats of one fine row of the lane's cells, at p -> r[k], c[k] per cell.  FX = 4, 8: one cell of FX floats, one or
// two quads; FX = 2: CPL = 4 cells of 2 floats, two quads (nc < CPL: the last cells of a coarse row, dword by dword); a
// quad is one 16-byte load where its address allows it (ldq_any).  FX = 0: one cell of any fx, element by element.
template <int FX, int CPL, bool SKIPNA>
__device__ __forceinline__ void row_sums(const float* __restrict__ p, int fx, int nc, double (&r)[CPL], int (&c)[CPL]) {
  if constexpr (FX == 0) {
    r[0] = 0.0;
    c[0] = 0;
    for (int b = 0; b < fx; ++b) {
      const float x = p[b];
      if (!SKIPNA || finite_bits(x)) {
        r[0] = r[0] + (double)x;
        c[0] += 1;
      }
    }
  } else {
    constexpr int N = FX * CPL;                                  // floats of the lane in this row: 8, 4, 8
    float v[N];
    if (nc == CPL) {
#pragma unroll
      for (int k = 0; k < N / 4; ++k) {
        const f32x4 q = ldq_any(p + 4 * k);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * k + e] = q[e];
      }
    } else {
#pragma unroll
      for (int e = 0; e < N; ++e) v[e] = e < FX * nc ? p[e] : 0.f;   // (the cells that do not exist: zeros, never stored)
    }
#pragma unroll
    for (int k = 0; k < CPL; ++k) chain<FX, SKIPNA>(v + FX * k, r[k], c[k]);
  }
}

// lane q of a snapshot: plane p = q / per_plane, coarse row I and the CPL cells from J on of that row; per_row lanes cover
// a coarse row (NLON cells, the last lane of a row at fx = 2 holds 1 .. 4), per_plane = NLAT per_row, lanes = P per_plane
template <int FX, bool SKIPNA>
__global__ __launch_bounds__(kBlock) void coarsen_kernel(const float* __restrict__ X, int64_t T, int64_t ldx, int64_t ldp,
                                                         int64_t nlon, const double* __restrict__ w, int fy, int fx,
                                                         int64_t lat0, int64_t lon0, uint32_t NLON, uint32_t per_row,
                                                         uint32_t per_plane, uint32_t lanes, double min_frac,
                                                         float* __restrict__ Y, int64_t ldy, int64_t ldq) {
  constexpr int CPL = coarsen_cells_per_lane(FX);
  const int64_t q64 = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (q64 >= (int64_t)lanes) return;
  const uint32_t q = (uint32_t)q64;                              // lanes <= P NLAT NLON <= ldy < 2^31, host-checked
  const uint32_t p = q / per_plane, rem = q - p * per_plane;
  const uint32_t I = rem / per_row, J = CPL * (rem - I * per_row);
  const int nc = NLON - J < (uint32_t)CPL ? (int)(NLON - J) : CPL;   // cells of this lane: CPL, fewer at the end of a row
  const int64_t i0 = lat0 + (int64_t)I * fy;
  const float* x0 = X + (int64_t)p * ldp + i0 * nlon + lon0 + (int64_t)J * fx;
  float* y0 = Y + (int64_t)p * ldq + (int64_t)I * NLON + J;
  const double* wp = w + i0;
  const double dfx = (double)fx;

  for (int64_t t = blockIdx.y; t < T; t += gridDim.y) {
    const float* xp = x0 + t * ldx;
    double num[CPL], den[CPL], full = 0.0;
#pragma unroll
    for (int k = 0; k < CPL; ++k) num[k] = den[k] = 0.0;
#pragma unroll 4
    for (int a = 0; a < fy; ++a) {
      double r[CPL];
      int c[CPL];
      row_sums<FX, CPL, SKIPNA>(xp + a * nlon, fx, nc, r, c);
      const double wi = wp[a];
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        const double pn = wi * r[k], pd = wi * (double)c[k];      // rounded products of their own
        num[k] = num[k] + pn;
        den[k] = den[k] + pd;
      }
      const double pf = wi * dfx;
      full = full + pf;
    }
    const double least = min_frac * full;
    float y[CPL];
#pragma unroll
    for (int k = 0; k < CPL; ++k)
      y[k] = (den[k] == 0.0 || den[k] < least) ? __uint_as_float(kQuietNaN) : (float)(num[k] / den[k]);
    float* yp = y0 + t * ldy;
    if constexpr (CPL == 4) {
      if (nc == 4 && ((uintptr_t)yp & 15u) == 0) {
        const f32x4 quad = {y[0], y[1], y[2], y[3]};
        *reinterpret_cast<f32x4*>(yp) = quad;
        continue;
      }
    }
#pragma unroll
    for (int k = 0; k < CPL; ++k)
      if (k < nc) yp[k] = y[k];
  }
}

template <int FX>
void launch(bool skipna, dim3 grid, hipStream_t st, const float* X, int64_t T, int64_t ldx, int64_t ldp, int64_t nlon,
            const double* w, int fy, int fx, int64_t lat0, int64_t lon0, uint32_t NLON, uint32_t per_row, uint32_t per_plane,
            uint32_t lanes, double min_frac, float* Y, int64_t ldy, int64_t ldq) {
  if (skipna)
    hipLaunchKernelGGL((coarsen_kernel<FX, true>), grid, dim3(kBlock), 0, st, X, T, ldx, ldp, nlon, w, fy, fx, lat0, lon0, NLON,
                       per_row, per_plane, lanes, min_frac, Y, ldy, ldq);
  else
    hipLaunchKernelGGL((coarsen_kernel<FX, false>), grid, dim3(kBlock), 0, st, X, T, ldx, ldp, nlon, w, fy, fx, lat0, lon0, NLON,
                       per_row, per_plane, lanes, min_frac, Y, ldy, ldq);
}

}  // namespace

extern "C" int dmdx_coarsen_max_factor(void) { return kCoarsenMaxFactor; }

extern "C" int dmdx_coarsen_f32(const float* X, int64_t T, int64_t ldx, int64_t P, int64_t ldp, int64_t nlat, int64_t nlon,
                                const double* w, int fy, int fx, int64_t lat0, int64_t lon0, int64_t NLAT, int64_t NLON,
                                int skipna, double min_frac, float* Y, int64_t ldy, int64_t ldq, void* stream) {
  if (int rc = check_coarsen(X, T, ldx, P, ldp, nlat, nlon, w, fy, fx, lat0, lon0, NLAT, NLON, min_frac, Y, ldy, ldq)) return rc;
  if (T == 0 || P == 0 || NLAT == 0 || NLON == 0) return 0;
  const hipStream_t st = (hipStream_t)stream;
  const int FX = DMDX_COARSEN_VEC && (fx == 2 || fx == 4 || fx == 8) ? fx : 0;
  const int64_t per_row = coarsen_lanes_per_row(NLON, FX), per_plane = NLAT * per_row, lanes = P * per_plane;   // <= ldy < 2^31
  const dim3 grid((unsigned)coarsen_blocks(lanes), grid_rows(T));
#define DMDX_COARSEN_LAUNCH(F)                                                                                        \
  launch<F>(skipna != 0, grid, st, X, T, ldx, ldp, nlon, w, fy, fx, lat0, lon0, (uint32_t)NLON, (uint32_t)per_row,    \
            (uint32_t)per_plane, (uint32_t)lanes, min_frac, Y, ldy, ldq)
  switch (FX) {
    case 2: DMDX_COARSEN_LAUNCH(2); break;
    case 4: DMDX_COARSEN_LAUNCH(4); break;
    case 8: DMDX_COARSEN_LAUNCH(8); break;
    default: DMDX_COARSEN_LAUNCH(0); break;
  }
#undef DMDX_COARSEN_LAUNCH
  DMDX_LAUNCH_CHECK();
  return 0;
}
