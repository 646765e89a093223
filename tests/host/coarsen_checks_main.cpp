// The host half of K23 (csrc/coarsen_geom.h) on plain integers: no HIP, no device, no library.
// tests/test_host_coarsen_checks.py builds this with the host compiler under -fsanitize=address,undefined and runs it: a
// signed overflow in the extent arithmetic of the checks ends the program, a wrong verdict fails one of its cases.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "../../dmd_era5_amd/csrc/coarsen_geom.h"

static char g_err[512];

void dmdx_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

static int g_failed = 0;

static void expect(int line, int rc, int want, const char* in_message) {
  const bool ok = rc == want && (want == 0 || (strstr(g_err, in_message) != nullptr));
  if (!ok) {
    printf("line %d: rc = %d, expected %d with \"%s\" in the message; message: %s\n", line, rc, want, in_message, g_err);
    ++g_failed;
  }
  g_err[0] = 0;
}
#define REFUSED(call, text) expect(__LINE__, (call), DMDX_E_INVALID, text)
#define RUNS(call) expect(__LINE__, (call), 0, "")

static const float* at(uint64_t address) { return reinterpret_cast<const float*>(static_cast<uintptr_t>(address)); }
static const double* wat(uint64_t address) { return reinterpret_cast<const double*>(static_cast<uintptr_t>(address)); }

// the arguments of one call, in the order of check_coarsen
struct Args {
  const float* X;
  int64_t T, ldx, P, ldp, nlat, nlon;
  const double* w;
  int64_t fy, fx, lat0, lon0, NLAT, NLON;
  double min_frac;
  const float* Y;
  int64_t ldy, ldq;
};

static int check(const Args& a) {
  return check_coarsen(a.X, a.T, a.ldx, a.P, a.ldp, a.nlat, a.nlon, a.w, a.fy, a.fx, a.lat0, a.lon0, a.NLAT, a.NLON,
                       a.min_frac, a.Y, a.ldy, a.ldq);
}

int main() {
  const int64_t big = int64_t(1) << 31;
  const uint64_t x0 = 0x7f0000001000u, w0 = 0x7e0000000000u;
  // 3 planes of 9 x 14 with 2 floats of pad, 2 x 4 cells from (1, 2): 4 x 3 cells
  const int64_t T = 5, P = 3, nlat = 9, nlon = 14, ldp = nlat * nlon + 2, NLAT = 4, NLON = 3, ldq = NLAT * NLON + 1;
  const int64_t mx = (P - 1) * ldp + nlat * nlon, my = (P - 1) * ldq + NLAT * NLON, ldx = mx + 3, ldy = my + 2;
  const uint64_t xbytes = 4 * ((T - 1) * ldx + mx), ybytes = 4 * ((T - 1) * ldy + my);
  const Args good = {at(x0), T, ldx, P, ldp, nlat, nlon, wat(w0), 2, 4, 1, 2, NLAT, NLON, 0.5, at(x0 + (uint64_t(1) << 32)), ldy, ldq};
  RUNS(check(good));
  Args a;

  // ---- overlap with blocks of different heights: Y inside, across both ends, and directly before / behind X's range
  a = good, a.Y = good.X;                          REFUSED(check(a), "coarsen: X and Y overlap (there is no in-place form)");
  a = good, a.Y = at(x0 + 16);                     REFUSED(check(a), "overlap");
  a = good, a.Y = at(x0 - 8);                      REFUSED(check(a), "overlap");
  a = good, a.Y = at(x0 + xbytes - 4);             REFUSED(check(a), "overlap");
  a = good, a.Y = at(x0 - ybytes + 4);             REFUSED(check(a), "overlap");
  a = good, a.Y = at(x0 + xbytes);                 RUNS(check(a));
  a = good, a.Y = at(x0 - ybytes);                 RUNS(check(a));
  // the heights differ: a Y that ends where a block of X's height would still overlap is fine, and the other way round
  RUNS(check_ranges("coarsen", at(x0), T, ldx, mx, at(x0 - ybytes), T, ldy, my));
  REFUSED(check_ranges("coarsen", at(x0), T, ldx, mx, at(x0 - ybytes + 4), T, ldy, my), "overlap");
  REFUSED(check_ranges("coarsen", at(x0 - ybytes), T, ldy, my, at(x0 - 4), T, ldx, mx), "overlap");
  RUNS(check_ranges("coarsen", at(x0 - ybytes), T, ldy, my, at(x0), T, ldx, mx));
  // nothing wraps at the ends of the address space
  RUNS(check_ranges("coarsen", at(~uint64_t(0) - 4 * 64 + 1), 2, 32, 32, at(256), 2, 8, 8));
  REFUSED(check_ranges("coarsen", at(0), 2, 32, 32, at(252), 2, 8, 8), "overlap");
  RUNS(check_ranges("coarsen", at(64), 2, 32, 32, at(0), 2, 8, 8));                     // Y: 16 floats, ends at 64
  REFUSED(check_ranges("coarsen", at(60), 2, 32, 32, at(0), 2, 8, 8), "overlap");
  // empty blocks touch nothing
  RUNS(check_ranges("coarsen", at(x0), 0, ldx, mx, at(x0), T, ldy, my));
  RUNS(check_ranges("coarsen", at(x0), T, ldx, mx, at(x0), T, ldy, 0));
  a = good, a.Y = good.X, a.T = 0;                 RUNS(check(a));
  a = good, a.Y = good.X, a.P = 0;                 RUNS(check(a));
  a = good, a.Y = good.X, a.NLAT = 0;              RUNS(check(a));
  a = good, a.Y = good.X, a.NLON = 0;              RUNS(check(a));

  // ---- extents: every size below 2^31, the extent (T - 1) ld + rows at 2^60 and beyond
  a = good, a.T = big - 1, a.ldx = big - 1;        REFUSED(check(a), "2^60");
  a = good, a.T = big - 1, a.ldy = big - 1;        REFUSED(check(a), "2^60");
  a = good, a.T = big - 1, a.ldx = big - 1, a.ldy = big - 1, a.P = 1, a.ldp = big - 1, a.ldq = big - 1;
  REFUSED(check(a), "2^60");
  const int64_t g = int64_t(1) << 30;
  // the last extent below 2^60, 2^30 (2^30 - 1) + 2^30 - 1, and the first one at it, 2^30 2^30
  RUNS(check_ranges("coarsen", at(0), g + 1, g - 1, g - 1, at(uint64_t(1) << 63), 1, 8, 8));
  REFUSED(check_ranges("coarsen", at(0), g + 1, g, g, at(uint64_t(1) << 63), 1, 8, 8), "2^60");
  REFUSED(check_ranges("coarsen", at(0), 1, 8, 8, at(uint64_t(1) << 63), g + 1, g, g), "2^60");
  // 2^31 - 1 in every size at once: a plane of (2^31 - 1)^2 points cannot have ldp >= nlat nlon
  a = good, a.nlat = big - 1, a.nlon = big - 1, a.NLAT = 1, a.NLON = 1;   REFUSED(check(a), "ldp=");
  a = good, a.T = big - 1, a.P = big - 1;          REFUSED(check(a), "ldx=");             // (P - 1) ldp does not fit ldx
  a = good, a.T = big - 1;                         REFUSED(check(a), "overlap");          // 3.3 TB of X, Y 4 GB behind its start
  a = good, a.T = big - 1, a.Y = at(uint64_t(1) << 62);                                  RUNS(check(a));
  a = good, a.T = big, a.ldx = ldx;                REFUSED(check(a), ">= 2^31");
  a = good, a.nlon = big;                          REFUSED(check(a), ">= 2^31");
  a = good, a.ldq = big;                           REFUSED(check(a), ">= 2^31");

  // ---- ldx / ldp / ldy / ldq consistency
  a = good, a.ldp = nlat * nlon - 1;               REFUSED(check(a), "ldp=125 < nlat nlon = 126");
  a = good, a.ldp = nlat * nlon, a.ldx = (P - 1) * nlat * nlon + nlat * nlon;             RUNS(check(a));
  a = good, a.ldx = mx - 1;                        REFUSED(check(a), "ldx=");
  a = good, a.ldx = mx;                            RUNS(check(a));
  a = good, a.ldq = NLAT * NLON - 1;               REFUSED(check(a), "ldq=11 < NLAT NLON = 12");
  a = good, a.ldy = my - 1;                        REFUSED(check(a), "ldy=");
  a = good, a.ldy = my;                            RUNS(check(a));
  a = good, a.P = 1, a.ldx = nlat * nlon, a.ldy = NLAT * NLON;                             RUNS(check(a));
  a = good, a.P = 1, a.ldx = nlat * nlon - 1;      REFUSED(check(a), "ldx=");

  // ---- cells, factors, offsets, min_frac, pointers
  a = good, a.NLAT = 5;                            REFUSED(check(a), "lat0 + NLAT fy = 11 > nlat=9");
  a = good, a.NLON = 4;                            REFUSED(check(a), "lon0 + NLON fx = 18 > nlon=14");
  a = good, a.lat0 = nlat + 1, a.NLAT = 0;         REFUSED(check(a), "latitude");
  a = good, a.lat0 = -1;                           REFUSED(check(a), "negative");
  a = good, a.lon0 = -1;                           REFUSED(check(a), "negative");
  a = good, a.fy = 0;                              REFUSED(check(a), "outside 1..64");
  a = good, a.fx = 65;                             REFUSED(check(a), "outside 1..64");
  a = good, a.fy = 64, a.NLAT = 0;                 RUNS(check(a));
  a = good, a.fy = big, a.NLAT = big - 1;          REFUSED(check(a), "outside 1..64");
  a = good, a.min_frac = -1e-300;                  REFUSED(check(a), "min_frac");
  a = good, a.min_frac = 1.0 + 1e-15;              REFUSED(check(a), "min_frac");
  a = good, a.min_frac = NAN;                      REFUSED(check(a), "min_frac");
  a = good, a.min_frac = 0.0;                      RUNS(check(a));
  a = good, a.min_frac = 1.0;                      RUNS(check(a));
  a = good, a.X = nullptr;                         REFUSED(check(a), "null");
  a = good, a.w = nullptr;                         REFUSED(check(a), "null");
  a = good, a.Y = nullptr;                         REFUSED(check(a), "null");
  a = good, a.X = at(x0 + 2);                      REFUSED(check(a), "not aligned");
  a = good, a.w = wat(w0 + 4);                     REFUSED(check(a), "not aligned");
  a = good, a.T = -1;                              REFUSED(check(a), "negative size");
  a = good, a.ldq = -1;                            REFUSED(check(a), "negative size");

  // ---- launch geometry
  const bool geometry = coarsen_blocks(0) == 0 && coarsen_blocks(1) == 1 && coarsen_blocks(DMDX_COARSEN_BLOCK) == 1 &&
                        coarsen_blocks(DMDX_COARSEN_BLOCK + 1) == 2 &&
                        coarsen_blocks(big - 1) == (big - 1 + DMDX_COARSEN_BLOCK - 1) / DMDX_COARSEN_BLOCK && kCoarsenMaxFactor == 64 &&
                        coarsen_lanes_per_row(5, 2) == 2 && coarsen_lanes_per_row(4, 2) == 1 && coarsen_lanes_per_row(1, 2) == 1 &&
                        coarsen_lanes_per_row(5, 4) == 5 && coarsen_lanes_per_row(5, 8) == 5 && coarsen_lanes_per_row(5, 0) == 5 &&
                        coarsen_lanes_per_row(big - 1, 2) == big / 4;
  if (!geometry) {
    printf("coarsen_blocks / coarsen_lanes_per_row\n");
    ++g_failed;
  }
  printf("%d failed\n", g_failed);
  return g_failed ? 1 : 0;
}
