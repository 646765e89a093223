// K28: first-order conservative remapping of the snapshots onto another regular latitude / longitude grid, separable in
// latitude and longitude, on the device.
//
// Layout.  X and Y are K23's: snapshot t at X + t ldx, plane p at p ldp (ldp >= nlat nlon, the slack is pad), latitude
// row i and longitude j of a plane at i nlon + j; Y[t ldy + p ldq + I NLON + J], ldq >= NLAT NLON.  Six device tables say
// what a target cell is made of.  Target row I overlaps the ny[I] source rows from iy0[I] on, with the fp64 weights
// wy[I SY + a]; target column J overlaps the nx[J] source columns (jx0[J] + b) mod nlon, with the weights wx[J SX + b].
// Entries of wy and wx beyond the count are never read.  regrid.Remap forms the tables on the host in fp64.
//
// Arithmetic (the contract of tests/remap_ref.py, held bit for bit): all fp64, never an FMA (contraction is off for the
// whole file).  Per snapshot, plane and cell
//     num = den = full = +0.0
//     for a = 0 .. ny[I] - 1 ascending, i = iy0[I] + a:
//         r = c = f = +0.0
//         for b = 0 .. nx[J] - 1 ascending, j = (jx0[J] + b) mod nlon, u = wx[J][b], x = X[t, p, i, j]:
//             if (!skipna || finite(x)) { r = r + u * fp64(x);  c = c + u; }
//             f = f + u
//         num = num + wy[I][a] * r;  den = den + wy[I][a] * c;  full = full + wy[I][a] * f     (products rounded)
//     Y = (den == 0 || den < min_frac * full) ? quiet NaN (0x7fc00000) : fp32(num / den)        (one rounding to fp32)
// finite(x) is K20's test of the bits.  Without skipna c is f and den is full, term for term: they are formed once.
//
// Lanes.  One lane per target cell; grid.x over the cells of a snapshot in the order of Y, grid.y over the snapshots
// (strided beyond 65535).  A wave holds 64 consecutive J of a target row (where the row does not end inside the wave):
// neighbouring lanes read neighbouring source runs, a wave's loads of one source row are one contiguous stretch, and
// its store is 256 contiguous bytes.  The tables are small (a 1 degree target: 181 x 5 and 360 x 5 doubles) and stay in
// the caches over T and P.  A lane whose table rows are at most kRegSpan wide keeps its wx row in registers for all
// of its source rows (the common case: 0.25 -> 1 degree spans 5); wider rows are read from the table element by
// element.  Such a lane also reads its run of a source row as the one to three aligned quads that cover it, 16 bytes a
// load, where the run does not wrap, the quads stay inside the row and the address of that row allows it (the test is
// per row, as K23's), and picks its floats out of them by jx0 mod 4; element by element otherwise.  Neighbouring lanes
// share quads, which the caches serve.  All routes put the same floats into the same chain in the same order: the same
// bits.  No atomics, no workspace, no synchronisation: the launch geometry is not part of the result.  What was
// measured: MEASUREMENTS.md, "K28".
//
// Memory.  The table contents cannot be checked by the entry point, so the kernel is safe for any contents: counts are
// clamped to 0 .. SY and 0 .. SX, row indices into [0, nlat), column indices are reduced modulo nlon (the entry point
// refuses cells of an empty plane).  A bad table gives a wrong number, never an access outside the planes of X.  Only
// the logical P NLAT NLON x T elements of Y are written.  Refusals: check_remap, remap_geom.h.
#include "remap_geom.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = DMDX_REMAP_BLOCK;
constexpr int kRegSpan = 8;                                      // wx rows up to this wide live in registers

template <bool REG, bool SKIPNA>
__global__ __launch_bounds__(kBlock) void remap_kernel(const float* __restrict__ X, int64_t T, int64_t ldx, int64_t ldp,
                                                       int64_t nlat, int64_t nlon, const int32_t* __restrict__ iy0,
                                                       const int32_t* __restrict__ ny, const double* __restrict__ wy, int SY,
                                                       const int32_t* __restrict__ jx0, const int32_t* __restrict__ nx,
                                                       const double* __restrict__ wx, int SX, uint32_t NLON, uint32_t per_plane,
                                                       uint32_t cells, double min_frac, float* __restrict__ Y, int64_t ldy,
                                                       int64_t ldq) {
  const int64_t q64 = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (q64 >= (int64_t)cells) return;
  const uint32_t q = (uint32_t)q64;                              // cells <= P NLAT NLON <= ldy < 2^31, host-checked
  const uint32_t p = q / per_plane, rem = q - p * per_plane;
  const uint32_t I = rem / NLON, J = rem - I * NLON;
  // what the tables say, made safe: counts in 0 .. S, the first row in [0, nlat), the first column in [0, nlon)
  int na = ny[I], nb = nx[J];
  na = na < 0 ? 0 : (na > SY ? SY : na);
  nb = nb < 0 ? 0 : (nb > SX ? SX : nb);
  int64_t i0 = iy0[I], j0 = (int64_t)jx0[J] % nlon;
  i0 = i0 < 0 ? 0 : (i0 > nlat - 1 ? nlat - 1 : i0);
  if (j0 < 0) j0 += nlon;
  const double* wyr = wy + (int64_t)I * SY;
  const double* wxr = wx + (int64_t)J * SX;
  const float* x0 = X + (int64_t)p * ldp;
  float* y0 = Y + (int64_t)p * ldq + (int64_t)I * NLON + J;

  double ureg[REG ? kRegSpan : 1];
  if constexpr (REG) {
#pragma unroll
    for (int b = 0; b < kRegSpan; ++b) ureg[b] = b < nb ? wxr[b] : 0.0;
  }
  // REG: the run j0 .. j0 + nb - 1 lies in the nq <= 3 quads from column jq = j0 - off on, where it neither wraps nor
  // leaves the row with them: 16-byte loads where the address of a row allows it, and a select by off
  const int off = (int)(j0 & 3), nq = (off + nb + 3) >> 2;
  const int64_t jq = j0 - off;
  const bool quads = REG && nb > 0 && j0 + nb <= nlon && jq + 4 * nq <= nlon;

  for (int64_t t = blockIdx.y; t < T; t += gridDim.y) {
    const float* xp = x0 + t * ldx;
    double num = 0.0, den = 0.0, full = 0.0;
    for (int a = 0; a < na; ++a) {
      const int64_t i = i0 + a > nlat - 1 ? nlat - 1 : i0 + a;
      const float* row = xp + i * nlon;
      double r = 0.0, c = 0.0, f = 0.0;
      int64_t j = j0;
      if (REG && quads && ((uintptr_t)(row + jq) & 15u) == 0) {
        float v[kRegSpan + 4];
#pragma unroll
        for (int k = 0; k < (kRegSpan + 4) / 4; ++k) {
          f32x4 q = {0.f, 0.f, 0.f, 0.f};
          if (k < nq) q = *reinterpret_cast<const f32x4*>(row + jq + 4 * k);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[4 * k + e] = q[e];
        }
#pragma unroll
        for (int b = 0; b < kRegSpan; ++b)
          if (b < nb) {
            const float x = off == 0 ? v[b] : (off == 1 ? v[b + 1] : (off == 2 ? v[b + 2] : v[b + 3]));
            const double u = ureg[b];
            if (!SKIPNA || finite_bits(x)) {
              const double ux = u * (double)x;
              r = r + ux;
              if (SKIPNA) c = c + u;
            }
            f = f + u;
          }
      } else if constexpr (REG) {
#pragma unroll
        for (int b = 0; b < kRegSpan; ++b)
          if (b < nb) {
            const float x = row[j];
            const double u = ureg[b];
            if (!SKIPNA || finite_bits(x)) {
              const double ux = u * (double)x;                   // a rounded product of its own
              r = r + ux;
              if (SKIPNA) c = c + u;
            }
            f = f + u;
            if (++j == nlon) j = 0;
          }
      } else {
        for (int b = 0; b < nb; ++b) {
          const float x = row[j];
          const double u = wxr[b];
          if (!SKIPNA || finite_bits(x)) {
            const double ux = u * (double)x;
            r = r + ux;
            if (SKIPNA) c = c + u;
          }
          f = f + u;
          if (++j == nlon) j = 0;
        }
      }
      const double wa = wyr[a];
      const double pn = wa * r, pf = wa * f;
      num = num + pn;
      full = full + pf;
      if (SKIPNA) {
        const double pd = wa * c;
        den = den + pd;
      }
    }
    if (!SKIPNA) den = full;                                     // c is f term for term: the same sums
    const double least = min_frac * full;
    y0[t * ldy] = (den == 0.0 || den < least) ? __uint_as_float(kQuietNaN) : (float)(num / den);
  }
}

template <bool REG>
void launch(bool skipna, dim3 grid, hipStream_t st, const float* X, int64_t T, int64_t ldx, int64_t ldp, int64_t nlat,
            int64_t nlon, const int32_t* iy0, const int32_t* ny, const double* wy, int SY, const int32_t* jx0, const int32_t* nx,
            const double* wx, int SX, uint32_t NLON, uint32_t per_plane, uint32_t cells, double min_frac, float* Y, int64_t ldy,
            int64_t ldq) {
  if (skipna)
    hipLaunchKernelGGL((remap_kernel<REG, true>), grid, dim3(kBlock), 0, st, X, T, ldx, ldp, nlat, nlon, iy0, ny, wy, SY, jx0, nx,
                       wx, SX, NLON, per_plane, cells, min_frac, Y, ldy, ldq);
  else
    hipLaunchKernelGGL((remap_kernel<REG, false>), grid, dim3(kBlock), 0, st, X, T, ldx, ldp, nlat, nlon, iy0, ny, wy, SY, jx0, nx,
                       wx, SX, NLON, per_plane, cells, min_frac, Y, ldy, ldq);
}

}  // namespace

extern "C" int dmdx_remap_max_span(void) { return kRemapMaxSpan; }

extern "C" int dmdx_remap_f32(const float* X, int64_t T, int64_t ldx, int64_t P, int64_t ldp, int64_t nlat, int64_t nlon,
                              const int32_t* iy0, const int32_t* ny, const double* wy, int SY, const int32_t* jx0,
                              const int32_t* nx, const double* wx, int SX, int64_t NLAT, int64_t NLON, int skipna,
                              double min_frac, float* Y, int64_t ldy, int64_t ldq, void* stream) {
  if (int rc = check_remap(X, T, ldx, P, ldp, nlat, nlon, iy0, ny, wy, SY, jx0, nx, wx, SX, NLAT, NLON, min_frac, Y, ldy, ldq))
    return rc;
  if (T == 0 || P == 0 || NLAT == 0 || NLON == 0) return 0;
  const hipStream_t st = (hipStream_t)stream;
  const int64_t per_plane = NLAT * NLON, cells = P * per_plane;   // <= ldy < 2^31
  const dim3 grid((unsigned)remap_blocks(cells), grid_rows(T));
  if (SX <= kRegSpan)
    launch<true>(skipna != 0, grid, st, X, T, ldx, ldp, nlat, nlon, iy0, ny, wy, SY, jx0, nx, wx, SX, (uint32_t)NLON,
                 (uint32_t)per_plane, (uint32_t)cells, min_frac, Y, ldy, ldq);
  else
    launch<false>(skipna != 0, grid, st, X, T, ldx, ldp, nlat, nlon, iy0, ny, wy, SY, jx0, nx, wx, SX, (uint32_t)NLON,
                  (uint32_t)per_plane, (uint32_t)cells, min_frac, Y, ldy, ldq);
  DMDX_LAUNCH_CHECK();
  return 0;
}
