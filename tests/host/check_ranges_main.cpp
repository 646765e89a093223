// The host half of csrc/time_rows.h on plain integers: no HIP, no device, no library.  tests/test_host_checks.py builds
// this with the host compiler under -fsanitize=undefined,address and runs it: a signed overflow in the extent
// arithmetic of check_ranges, the thing the 2^60 rule is there to prevent, ends the program.  So does one in the
// piece counts of the period frame (bounds_ok, count_pieces, fill_periods) or a read past the bounds of a launch, and
// saturating_bytes is held to the last product that fits a size_t and the first that does not.
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
#define CHECK(cond) \
  do {              \
    if (!(cond)) printf("line %d: %s\n", __LINE__, #cond), ++g_failed; \
  } while (0)

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
  const RowLanes quad = row_lanes(at(x0), 16, 1025, 70000, true), dword = row_lanes(at(x0 + 4), 16, 1025, 9, false),
                 odd_ld = row_lanes(at(x0), 14, 256, 9, true);
  CHECK(quad.quad && quad.gx == 2 && quad.gy == 65535 && !dword.quad && dword.gx == 5 && dword.gy == 1);
  CHECK(!odd_ld.quad && odd_ld.gx == 1 && odd_ld.gy == 9);

  // ---- the periods of K27 / K29: bounds_ok
  int32_t ramp[kMaxPeriods + 2];
  for (int p = 0; p < kMaxPeriods + 2; ++p) ramp[p] = 3 * p;
  CHECK(!bounds_ok(ramp, 0, -1) && bounds_ok(ramp, 1, -1) && bounds_ok(ramp, 128, -1) && !bounds_ok(ramp, 129, -1));
  CHECK(!bounds_ok(nullptr, 1, -1) && !bounds_ok(ramp, -1, -1));
  CHECK(bounds_ok(ramp, 128, 384) && !bounds_ok(ramp, 128, 383) && bounds_ok(ramp, 4, 12) && bounds_ok(ramp, 4, 13));
  const int32_t equal[] = {0, 5, 5, 9}, down[] = {0, 7, 6, 9}, neg[] = {-1, 2, 6, 9}, from2[] = {2, 9, 10, 37, 58};
  CHECK(!bounds_ok(equal, 3, -1) && bounds_ok(equal, 1, -1) && !bounds_ok(down, 3, -1) && !bounds_ok(neg, 3, -1));
  CHECK(bounds_ok(from2, 4, 58) && !bounds_ok(from2, 4, 57) && bounds_ok(from2, 3, 57));     // bounds[P] at T and at T + 1

  // ---- count_pieces: the counts tests/test_spell_checks.py and tests/test_pstat_checks.py state by hand
  int32_t first[5];
  CHECK(count_pieces(from2, 4, 1, 1, nullptr) == 56 && count_pieces(from2, 4, 1, 100, nullptr) == 4);
  CHECK(count_pieces(from2, 4, 1, 4, first) == 2 + 1 + 7 + 6);                              // lengths 7, 1, 27, 21
  CHECK(first[0] == 0 && first[1] == 2 && first[2] == 3 && first[3] == 10 && first[4] == 16);
  CHECK(count_pieces(from2, 4, 1, 7, nullptr) == 1 + 1 + 4 + 3 && count_pieces(from2, 2, 1, 4, nullptr) == 2 + 1);
  const int32_t days[] = {2, 9, 10, 50, 93};                                                // lengths 7, 1, 40, 43
  CHECK(count_pieces(days, 4, 1, 1, nullptr) == 91 && count_pieces(days, 4, 3, 2, first) == 2 + 1 + 7 + 8);
  CHECK(first[0] == 0 && first[1] == 2 && first[2] == 3 && first[3] == 10 && first[4] == 18);
  CHECK(count_pieces(days, 4, 3, 4, nullptr) == 1 + 1 + 4 + 4 && count_pieces(days, 4, 24, 1, nullptr) == 1 + 1 + 2 + 2);
  CHECK(count_pieces(days, 4, 4, 7, nullptr) == 1 + 1 + 2 + 2 && count_pieces(days, 4, 100, 1, nullptr) == 4);
  // one period of 2^31 - 1 snapshots in pieces of 1: the last piece0 is the largest int32, nothing wraps
  const int32_t whole[] = {0, INT32_MAX};
  CHECK(bounds_ok(whole, 1, INT32_MAX) && !bounds_ok(whole, 1, INT32_MAX - 1));
  CHECK(count_pieces(whole, 1, 1, 1, first) == INT32_MAX && first[0] == 0 && first[1] == INT32_MAX);
  CHECK(count_pieces(whole, 1, big - 1, big - 1, nullptr) == 1 && count_pieces(whole, 1, 2, big - 1, nullptr) == 1);
  // by value: padded to the maximum with the last entry
  PeriodCuts pd;
  CHECK(fill_periods(pd, days, 4, 3, 2) == 18 && pd.P == 4 && pd.bound[0] == 2 && pd.bound[4] == 93 && pd.piece0[4] == 18);
  CHECK(pd.bound[5] == 93 && pd.bound[kMaxPeriods] == 93 && pd.piece0[5] == 18 && pd.piece0[kMaxPeriods] == 18);
  CHECK(fill_periods(pd, ramp, 128, 1, 2) == 256 && pd.bound[kMaxPeriods] == 384 && pd.piece0[kMaxPeriods] == 256);

  // ---- saturating_bytes: 2^64 - 2 and 2^64 - 1 are sizes, 2^64 and beyond are SIZE_MAX
  CHECK(saturating_bytes(56, 4, 1029, 36) == size_t(56) * 4 * 1029 * 36 && saturating_bytes(0, 4, big - 1, 64) == 0);
  CHECK(saturating_bytes(2, INT64_MAX, 1, 1) == SIZE_MAX - 1);
  CHECK(saturating_bytes(int64_t(0xFFFFFFFF), int64_t(0x100000001), 1, 1) == SIZE_MAX);    // (2^32 - 1)(2^32 + 1)
  CHECK(saturating_bytes(big * 2, big, 2, 1) == SIZE_MAX && saturating_bytes(big - 1, 8, big - 1, 64) == SIZE_MAX);
  CHECK(saturating_bytes(INT64_MAX, INT64_MAX, INT64_MAX, INT64_MAX) == SIZE_MAX);
  CHECK(saturating_bytes(big - 1, 4, big - 1, 1) == size_t(4) * (big - 1) * (big - 1));   // the last K27 / K29 size that fits
  RUNS(check_workspace("spell", nullptr, 0, SIZE_MAX));
  RUNS(check_workspace("spell", X, 144, 144));
  REFUSED(check_workspace("spell", X, 143, 144), "spell: workspace of 143 bytes, 144 needed");
  REFUSED(check_workspace("period_stats", X, SIZE_MAX, SIZE_MAX), "period_stats: workspace of");

  printf("%d failed\n", g_failed);
  return g_failed ? 1 : 0;
}
