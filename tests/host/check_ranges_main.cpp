// The host half of csrc/time_rows.h on plain integers: no HIP, no device, no library.  tests/test_host_checks.py builds
// this with the host compiler under -fsanitize=undefined,address and runs it: a signed overflow in the extent
// arithmetic of check_ranges, the thing the 2^60 rule is there to prevent, ends the program.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "../../dmd_era5_amd/csrc/time_rows.h"

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

int main() {
  const int64_t big = int64_t(1) << 31, m = 12, T = 40, ld = 14;
  const uint64_t x0 = 0x7f0000001000u, xbytes = 4 * ((T - 1) * ld + m);
  const float *X = at(x0), *Y = at(x0 + (uint64_t(1) << 32));

  // ---- extents: every size below 2^31, (T - 1) ld + m beyond 2^60 -- 4 times that wraps 64 bits
  REFUSED(check_ranges("clim_apply", X, big - 1, big - 1, Y, big - 1, big - 1, m, true), "clim_apply: (T - 1) ldx + m");
  REFUSED(check_ranges("clim_apply", X, big - 1, big - 1, X, big - 1, big - 1, m, true), "2^60");   // in place
  REFUSED(check_ranges("treg_apply", X, big - 1, big - 1, Y, big - 1, ld, m, true), "treg_apply: (T - 1) ldx + m");
  REFUSED(check_ranges("treg_apply", X, big - 1, ld, Y, big - 1, big - 1, m, true), "2^60");
  REFUSED(check_ranges("tfilt", X, big - 1, big - 1, Y, 9, ld, m, false), "tfilt: (T - 1) ldx + m");
  REFUSED(check_ranges("tfilt", X, big - 1, ld, Y, big - 1, big - 1, m, false), "2^60");
  REFUSED(check_ranges("tfilt", X, big - 1, big - 1, Y, big - 1, big - 1, big - 1, false), "2^60");  // the largest of all
  REFUSED(check_ranges("tfilt", X, big - 1, big - 1, Y, 9, ld, 0, false), "2^60");                   // (as tfilt: before m == 0)
  RUNS(check_ranges("tfilt", X, big - 1, ld, at(x0 + (uint64_t(1) << 40)), big - 1, ld, m, false));   // 120 GB each
  REFUSED(check_ranges("tfilt", X, big - 1, ld, Y, big - 1, ld, m, false), "overlap");                 // ... 4 GB apart
  // the last extent below 2^60, 2^30 (2^30 - 1) + 2^30 - 1, and the first one at it, 2^30 2^30 + 0
  const int64_t g = int64_t(1) << 30;
  RUNS(check_ranges("tfilt", at(0), g + 1, g - 1, at(uint64_t(1) << 63), 1, g - 1, g - 1, false));
  REFUSED(check_ranges("tfilt", at(0), g + 1, g, at(uint64_t(1) << 63), 1, g, 0, false), "2^60");

  // ---- overlap: Y inside, across the front and across the end of X; directly behind and in front of it
  const uint64_t ybytes = 4 * ((9 - 1) * ld + m);
  REFUSED(check_ranges("tfilt", X, T, ld, X, 9, ld, m, false), "tfilt: X and Y overlap (there is no in-place form)");
  REFUSED(check_ranges("tfilt", X, T, ld, at(x0 + 16), 9, ld, m, false), "overlap");
  REFUSED(check_ranges("tfilt", X, T, ld, at(x0 - 8), 9, ld, m, false), "overlap");
  REFUSED(check_ranges("tfilt", X, T, ld, at(x0 + xbytes - 4), 9, ld, m, false), "overlap");
  REFUSED(check_ranges("tfilt", X, T, ld, at(x0 - ybytes + 4), 9, ld, m, false), "overlap");
  REFUSED(check_ranges("tfilt", X, T, ld, at(x0 + 4 * (T - 3) * ld), 9, ld, m, false), "overlap");
  RUNS(check_ranges("tfilt", X, T, ld, at(x0 + xbytes), 9, ld, m, false));
  RUNS(check_ranges("tfilt", X, T, ld, at(x0 - ybytes), 9, ld, m, false));
  REFUSED(check_ranges("clim_apply", X, T, ld, at(x0 + 16), T, ld, m, true), "only Y == X with ldy == ldx");
  REFUSED(check_ranges("clim_apply", X, T, ld, at(x0 - 8), T, ld, m, true), "overlap");
  REFUSED(check_ranges("clim_apply", X, T, ld, at(x0 + xbytes - 4), T, ld, m, true), "overlap");
  RUNS(check_ranges("clim_apply", X, T, ld, at(x0 + xbytes), T, ld, m, true));
  // in place: Y == X with the same leading dimension, where the entry point has an in-place form
  RUNS(check_ranges("treg_apply", X, T, ld, X, T, ld, m, true));
  REFUSED(check_ranges("treg_apply", X, T, ld, X, T, ld + 1, m, true), "treg_apply: X and Y overlap");
  REFUSED(check_ranges("treg_apply", X, T, ld, X, T, ld, m, false), "overlap");
  // nothing wraps at the ends of the address space either
  RUNS(check_ranges("tfilt", at(~uint64_t(0) - 4 * 64 + 1), 2, 32, at(256), 2, 32, 32, false));
  REFUSED(check_ranges("tfilt", at(0), 2, 32, at(252), 2, 32, 32, false), "overlap");
  // empty blocks touch nothing
  RUNS(check_ranges("clim_apply", X, 0, ld, X, 0, ld + 1, m, true));
  RUNS(check_ranges("tfilt", X, T, ld, X, 0, ld, m, false));
  RUNS(check_ranges("tfilt", X, T, ld, X, 9, ld, 0, false));

  // ---- check_block
  RUNS(check_block("who", m, T, {{"ldx", ld}, {"ldy", m}}, {X, Y, nullptr}, {at(x0 + 8)}));
  RUNS(check_block("who", 0, 0, {{"ldx", 0}}, {X}));
  REFUSED(check_block("clim_mean", -1, T, {{"ldx", ld}}, {X}), "clim_mean: negative size (m=-1 T=40)");
  REFUSED(check_block("who", m, -1, {{"ldx", ld}}, {X}), "negative size");
  REFUSED(check_block("who", big, T, {{"ldx", big}}, {X}), "a size >= 2^31");
  REFUSED(check_block("who", m, big, {{"ldx", ld}}, {X}), "a size >= 2^31");
  REFUSED(check_block("treg_fit", m, T, {{"ldx", ld}, {"ldc", m - 1}}, {X}), "treg_fit: ldc=11 < m=12");
  REFUSED(check_block("who", m, T, {{"ldx", big}, {"ldc", ld}}, {X}), "ldx=2147483648");
  REFUSED(check_block("who", m, T, {{"ldx", -1}}, {X}), "ldx=-1");
  REFUSED(check_block("who", m, T, {{"ldx", ld}}, {X, at(x0 + 2)}), "not aligned");
  REFUSED(check_block("who", m, T, {{"ldx", ld}}, {X}, {at(x0 + 4)}), "not aligned");

  // ---- launch geometry
  const bool geometry = chunks_of<4>(1) == 1 && chunks_of<4>(2) == 2 && chunks_of<4>(5) == 2 && chunks_of<4>(6) == 3 &&
                        chunks_of<8>(5) == 1 && chunks_of<8>(6) == 2 && chunks_of<4>(big - 1) == (big + 4) / 4 &&
                        grid_rows(0) == 0 && grid_rows(3) == 3 && grid_rows(65535) == 65535 && grid_rows(big - 1) == 65535;
  if (!geometry) {
    printf("chunks_of / grid_rows\n");
    ++g_failed;
  }
  printf("%d failed\n", g_failed);
  return g_failed ? 1 : 0;
}
