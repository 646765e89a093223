// The host half of K28 in libdmdx_host.so: the argument checks of dmdx_remap_f32 (remap_geom.h) behind a C entry point
// with the arguments of the kernel's, so that they run on the CPU without HIP and without libdmdx.so
// (tests/test_host_remap_checks.py).  Plain C++, no GPU code.  Only the three entry points below are exported.
#include <stdarg.h>
#include <stdio.h>

#pragma GCC visibility push(hidden)                            // dmdx_set_error stays inside this library
#include "remap_geom.h"

static thread_local char g_err[512];

void dmdx_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

#pragma GCC visibility pop

#define DMDX_HOST_API extern "C" __attribute__((visibility("default")))

DMDX_HOST_API const char* dmdx_host_last_error(void) { return g_err; }

DMDX_HOST_API int dmdx_host_remap_max_span(void) { return kRemapMaxSpan; }

// what dmdx_remap_f32 returns before its first HIP call: 0 (the call would run, or is empty) or DMDX_E_INVALID
DMDX_HOST_API int dmdx_host_remap_check(const float* X, int64_t T, int64_t ldx, int64_t P, int64_t ldp, int64_t nlat,
                                        int64_t nlon, const int32_t* iy0, const int32_t* ny, const double* wy, int SY,
                                        const int32_t* jx0, const int32_t* nx, const double* wx, int SX, int64_t NLAT,
                                        int64_t NLON, int skipna, double min_frac, const float* Y, int64_t ldy, int64_t ldq) {
  (void)skipna;
  g_err[0] = 0;
  return check_remap(X, T, ldx, P, ldp, nlat, nlon, iy0, ny, wy, SY, jx0, nx, wx, SX, NLAT, NLON, min_frac, Y, ldy, ldq);
}
