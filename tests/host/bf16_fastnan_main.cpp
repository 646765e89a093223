// The premise of K1's unit-end verdict, on the host: no HIP, no device, no library.  tests/test_host_fastnan.py builds
// this with the host compiler under -fsanitize=undefined,address and runs it.  What it holds:
//   * for ALL 2^24 fp32 patterns with an all-ones exponent (every Inf and NaN, both signs) the fast split leaves a
//     bf16 NaN in the value's half of the packed l plane (and of the m plane), in either slot of the pair, so the
//     products l h' and h' l that K1 contracts for every pair carry NaN into every output the value feeds;
//   * the other half of the pair, a finite neighbour, keeps exactly the planes it has next to a finite value;
//   * alarm() fires on such a plane and on nothing finite;
//   * make_safe2 / sanitise2 on the fast planes of finite values are the identity (the rerun gives the planes of the
//     fast pass wherever the data is finite), over every normal binade with 8, 16 and 24 significant bits.
#include <stdint.h>
#include <stdio.h>

#include "../../dmd_era5_amd/csrc/bf16_split.h"

using namespace bf16split;

static long g_failed = 0;
#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      if (g_failed < 20) {                    \
        printf("line %d: ", __LINE__);        \
        printf(__VA_ARGS__);                  \
        printf("\n");                         \
      }                                       \
      ++g_failed;                             \
    }                                         \
  } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return (uint32_t)(g_rng >> 16);
}

static bool bf16_is_nan(uint32_t half) { return (half & 0x7F80u) == 0x7F80u && (half & 0x007Fu) != 0u; }

int main() {
  // finite neighbours, normal, both signs, and their planes next to a finite value
  const int NP = 8;
  float partner[NP];
  uint32_t Hp[NP], Mp[NP], Lp[NP];
  for (int i = 0; i < NP; ++i) {
    partner[i] = from_bits(((rnd() % 254u + 1u) << 23) | (rnd() & 0x807FFFFFu));
    split2_fast(partner[i], 1.0f, Hp[i], Mp[i], Lp[i]);   // partner in the low half
  }
  long patterns = 0;
  for (uint32_t sign = 0; sign < 2; ++sign)
    for (uint32_t mant = 0; mant < (1u << 23); ++mant) {
      const uint32_t u = (sign << 31) | 0x7F800000u | mant;
      const float x = from_bits(u);
      ++patterns;
      uint32_t h, m, l;
      split1(x, h, m, l);
      CHECK(bf16_is_nan(l >> 16), "%08x: the top half of l = %08x is no bf16 NaN", u, l);
      CHECK(bf16_is_nan(m >> 16), "%08x: m = %08x is no bf16 NaN", u, m);
      const int i = (int)(mant & (NP - 1));
      uint32_t H, M, L;
      split2_fast(x, partner[i], H, M, L);                  // the value in the low half
      CHECK(bf16_is_nan(L & 0xFFFFu) && bf16_is_nan(M & 0xFFFFu), "%08x, slot 0: L = %08x M = %08x", u, L, M);
      CHECK(alarm(from_bits(L << 16)) && !alarm(from_bits(L & TOP16)), "%08x, slot 0: alarm on L = %08x", u, L);
      CHECK((H >> 16) == (Hp[i] & 0xFFFFu) && (M >> 16) == (Mp[i] & 0xFFFFu) && (L >> 16) == (Lp[i] & 0xFFFFu),
            "%08x, slot 0: the finite neighbour %a changed: %08x %08x %08x", u, partner[i], H, M, L);
      split2_fast(partner[i], x, H, M, L);                  // the value in the high half
      CHECK(bf16_is_nan(L >> 16) && bf16_is_nan(M >> 16), "%08x, slot 1: L = %08x M = %08x", u, L, M);
      CHECK(alarm(from_bits(L & TOP16)) && !alarm(from_bits(L << 16)), "%08x, slot 1: alarm on L = %08x", u, L);
      CHECK((H & 0xFFFFu) == (Hp[i] & 0xFFFFu) && (M & 0xFFFFu) == (Mp[i] & 0xFFFFu) && (L & 0xFFFFu) == (Lp[i] & 0xFFFFu),
            "%08x, slot 1: the finite neighbour %a changed: %08x %08x %08x", u, partner[i], H, M, L);
    }
  // finite values: the class rule is the identity on the fast planes, and no plane raises the alarm
  long finite = 0;
  for (int e = 1; e <= 254; ++e)
    for (int t = 0; t < 400; ++t) {
      const uint32_t sign = (rnd() & 1u) << 31, mant = rnd() & 0x007FFFFFu;
      const uint32_t keep[3] = {0x007F0000u, 0x007FFF00u, 0x007FFFFFu};
      const float other = from_bits(((rnd() % 254u + 1u) << 23) | (rnd() & 0x807FFFFFu));
      for (int w = 0; w < 3; ++w) {
        const float x = from_bits(sign | ((uint32_t)e << 23) | (mant & keep[w]));
        uint32_t H, M, L;
        split2_fast(x, other, H, M, L);
        uint32_t H2 = H, M2 = M, L2 = L;
        make_safe2(x, other, H2, M2, L2);
        CHECK(H2 == H && M2 == M && L2 == L && sanitise2(H) == H, "make_safe2 / sanitise2 change the planes of finite (%a, %a)", x, other);
        CHECK(!alarm(from_bits(L << 16)) && !alarm(from_bits(L & TOP16)) && !alarm(from_bits(M << 16)) && !alarm(from_bits(H << 16)),
              "alarm on a plane of finite (%a, %a)", x, other);
        ++finite;
      }
    }
  printf("%ld non-finite patterns, %ld finite values\n%ld failed\n", patterns, finite, g_failed);
  return g_failed != 0;
}
