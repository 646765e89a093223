// csrc/bf16_split.h on the host: no HIP, no device, no library.  tests/test_host_split.py builds this with the host
// compiler under -fsanitize=undefined,address and runs it.  What it holds: the planes of a finite fp32 value sum back
// to it exactly and are bf16 values, the fast and the class-safe form agree on finite input, the class rule for
// Inf / NaN (every payload), the detector, 2^+-40 scaling, and -- emulated in fp32 on a small Gram -- that the six
// plane products with the sanitised copy h' give numpy-fp64's classes where the plain split does not.
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../dmd_era5_amd/csrc/bf16_split.h"

using namespace bf16split;

static int g_failed = 0;
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

static float lo_half(uint32_t P) { return from_bits(P << 16); }
static float hi_half(uint32_t P) { return from_bits(P & TOP16); }
static bool is_bf16(float x) { return (bits(x) & 0xFFFFu) == 0u; }
enum { FIN = 0, NAN_ = 1, PINF = 2, NINF = 3 };
static int cls(double x) { return x != x ? NAN_ : (x == INFINITY ? PINF : (x == -INFINITY ? NINF : FIN)); }

// one finite value next to a partner: everything the header promises for finite input
static void check_finite(float x, float partner) {
  uint32_t H, M, L, H2, HP, M2, L2;
  split2_fast(x, partner, H, M, L);
  const float h = lo_half(H), m = lo_half(M), l = lo_half(L);
  // exact while l stays a normal number (|x| >= 2^-103: l >= ulp(x) = 2^-23 |x|); below that the remainders are
  // subnormal, a bf16 plane keeps 7 of their bits and up to one bf16-subnormal quantum (2^-133) is lost
  if (x == 0.0f || fabsf(x) >= 0x1p-103f) {
    // the planes BEFORE packing (packing drops the low halves whatever they hold): h and m are masked, the last
    // remainder l is not, so that it fits bf16 is what makes the split exact
    uint32_t h1, m1, l1;
    split1(x, h1, m1, l1);
    CHECK(is_bf16(from_bits(h1)) && is_bf16(from_bits(m1)) && is_bf16(from_bits(l1)), "planes of %a are not bf16: %08x %08x %08x", x, h1, m1, l1);
    CHECK(bits(h) == h1 && bits(m) == m1 && bits(l) == l1, "packing changes the planes of %a", x);
    CHECK((h + m) + l == x && h + (m + l) == x, "planes of %a do not sum back: %a %a %a", x, h, m, l);
    CHECK((double)h + (double)m + (double)l == (double)x, "planes of %a do not sum back in fp64", x);
  } else {
    CHECK(fabs((double)h + (double)m + (double)l - (double)x) < 0x1p-132, "planes of %a: off by more than the subnormal quantum", x);
  }
  CHECK(fabsf(m) <= fabsf(h) * 0x1p-7f && fabsf(l) <= fabsf(h) * 0x1p-15f, "planes of %a do not shrink: %a %a %a", x, h, m, l);
  // the other slot of the pair holds the same planes
  uint32_t Hs, Ms, Ls;
  split2_fast(partner, x, Hs, Ms, Ls);
  CHECK(bits(hi_half(Hs)) == bits(h) && bits(hi_half(Ms)) == bits(m) && bits(hi_half(Ls)) == bits(l), "slot 1 differs for %a", x);
  split2_safe(x, partner, H2, HP, M2, L2);
  CHECK(H2 == H && M2 == M && L2 == L && HP == H, "fast and safe differ on finite (%a, %a)", x, partner);
  CHECK(sanitise2(H) == H, "sanitise2 changes finite planes of (%a, %a)", x, partner);
  CHECK(!fired(detect(x, detect(partner, 0.0f))), "detector fires on finite (%a, %a)", x, partner);
  // 2^+-40 commutes with the split while no plane turns subnormal
  for (int e = -40; e <= 40; e += 80) {
    const float s = ldexpf(1.0f, e), xs = x * s;
    if (!(fabsf(x) >= 0x1p-60f && fabsf(x) <= 0x1p60f)) continue;
    uint32_t He, Me, Le;
    split2_fast(xs, 0.0f, He, Me, Le);
    CHECK(lo_half(He) == h * s && lo_half(Me) == m * s && lo_half(Le) == l * s, "2^%d does not commute with the split of %a", e, x);
  }
}

static void check_non_finite(uint32_t u, float partner) {
  const float x = from_bits(u);
  const bool nan = (u & 0x007FFFFFu) != 0u;
  for (int slot = 0; slot < 2; ++slot) {
    uint32_t H, HP, M, L, Hf, Mf, Lf;
    if (slot == 0) split2_safe(x, partner, H, HP, M, L); else split2_safe(partner, x, H, HP, M, L);
    if (slot == 0) split2_fast(x, partner, Hf, Mf, Lf); else split2_fast(partner, x, Hf, Mf, Lf);
    const float h = slot ? hi_half(H) : lo_half(H), hp = slot ? hi_half(HP) : lo_half(HP);
    const float m = slot ? hi_half(M) : lo_half(M), l = slot ? hi_half(L) : lo_half(L);
    if (nan) CHECK(h != h && (bits(h) & 0x00400000u), "NaN %08x: h = %08x is no quiet NaN", u, bits(h));
    else CHECK(bits(h) == u, "Inf %08x: h = %08x", u, bits(h));
    CHECK(bits(hp) == 0u && bits(m) == 0u && bits(l) == 0u, "%08x: h' m l = %08x %08x %08x, expected zeros", u, bits(hp), bits(m), bits(l));
    // the finite partner keeps the planes of the fast form, and HP = sanitise2(H)
    const uint32_t keep = slot ? 0x0000FFFFu : 0xFFFF0000u;
    CHECK((H & keep) == (Hf & keep) && (M & keep) == (Mf & keep) && (L & keep) == (Lf & keep), "%08x changes its finite partner", u);
    CHECK(HP == sanitise2(H) && (HP & keep) == (H & keep), "%08x: HP is not the sanitised H", u);
    CHECK(fired(detect(partner, detect(x, 0.0f))) && fired(detect(x, detect(partner, 0.0f))), "detector silent on %08x", u);
  }
}

// fp32 emulation of the k-step: per output the six products in the kernel's order (rule = true: cross products on h'),
// or with the raw h everywhere and the fast planes (rule = false: what the value contract forbids)
static float dot6(const std::vector<float>& A, const std::vector<float>& B, int K, int n, int i, int j, bool rule) {
  float acc = 0.0f;
  for (int k = 0; k < K; ++k) {
    uint32_t Ha, Pa, Ma, La, Hb, Pb, Mb, Lb;
    if (rule) {
      split2_safe(A[(size_t)k * n + i], 0.0f, Ha, Pa, Ma, La);
      split2_safe(B[(size_t)k * n + j], 0.0f, Hb, Pb, Mb, Lb);
    } else {
      split2_fast(A[(size_t)k * n + i], 0.0f, Ha, Ma, La);
      split2_fast(B[(size_t)k * n + j], 0.0f, Hb, Mb, Lb);
      Pa = Ha;
      Pb = Hb;
    }
    const float ha = lo_half(Ha), pa = lo_half(Pa), ma = lo_half(Ma), la = lo_half(La);
    const float hb = lo_half(Hb), pb = lo_half(Pb), mb = lo_half(Mb), lb = lo_half(Lb);
    acc += ha * hb;
    acc += pa * lb;
    acc += la * pb;
    acc += pa * mb;
    acc += ma * pb;
    acc += ma * mb;
  }
  return acc;
}

static void check_gram_classes() {
  const int K = 64, n = 40;
  long wrong_rule = 0, wrong_plain = 0, outputs = 0;
  const uint32_t plants[6] = {0x7F800000u, 0xFF800000u, 0x7FC00000u, 0x7F800001u, 0xFF80FFFFu, 0x7FA00000u};
  for (int trial = 0; trial < 60; ++trial) {
    std::vector<float> X((size_t)K * n);
    for (int k = 0; k < K; ++k)
      for (int c = 0; c < n; ++c) {
        float v;
        if (c < 8) v = (float)((int)(rnd() % 19) - 9);                       // small integers, zeros among them: m = l = 0
        else if (c < 12) v = ldexpf(1.0f, (int)(rnd() % 9) - 4);             // powers of two
        else v = ((int)(rnd() % 2000001) - 1000000) * 1e-6f * 3.0f;          // 24 significant bits
        X[(size_t)k * n + c] = v;
      }
    if (trial % 3 == 0) X[(size_t)(rnd() % K) * n + 20] = 0.0f;              // planted zeros
    const int pk = (int)(rnd() % K), pc = (int)(rnd() % n);
    X[(size_t)pk * n + pc] = from_bits(plants[trial % 6]);
    if (trial % 4 == 0) X[(size_t)((pk + 7) % K) * n + pc] = from_bits(plants[(trial + 1) % 6]);   // a second one: Inf - Inf
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) {
        double ref = 0.0;
        for (int k = 0; k < K; ++k) ref += (double)X[(size_t)k * n + i] * (double)X[(size_t)k * n + j];
        ++outputs;
        if (cls(dot6(X, X, K, n, i, j, true)) != cls(ref)) ++wrong_rule;
        if (cls(dot6(X, X, K, n, i, j, false)) != cls(ref)) ++wrong_plain;
      }
  }
  printf("Gram classes against fp64: rule %ld wrong, plain split %ld wrong, of %ld outputs\n", wrong_rule, wrong_plain, outputs);
  CHECK(wrong_rule == 0, "the class rule gives %ld wrong classes", wrong_rule);
  CHECK(wrong_plain > 0, "the plain split was expected to break classes on this data (the test lost its teeth)");
}

// The three dropped products m l, l m, l l.  Truncation leaves m < 2^-7 and l < 2^-15 of the value's binade, so one
// product pair loses less than 2 * 2^-22 + 2^-30 of |a||b| (asserted); the remainders are uniform below those
// limits, a sum of many products loses a quarter of that on average: about 2^-23 sum |a||b| (asserted below 2^-22).
static void check_dropped_terms() {
  double worst = 0.0, lost = 0.0, total = 0.0;
  for (int t = 0; t < 200000; ++t) {
    const float a = 250.0f + (rnd() % 5000001) * 1e-5f, b = 250.0f + (rnd() % 5000001) * 1e-5f;
    uint32_t Ha, Ma, La, Hb, Mb, Lb;
    split2_fast(a, 0.0f, Ha, Ma, La);
    split2_fast(b, 0.0f, Hb, Mb, Lb);
    const double ha = lo_half(Ha), ma = lo_half(Ma), la = lo_half(La), hb = lo_half(Hb), mb = lo_half(Mb), lb = lo_half(Lb);
    const double six = ha * hb + ha * mb + ma * hb + ha * lb + ma * mb + la * hb;
    const double rel = fabs(six - (double)a * (double)b) / ((double)a * (double)b);
    if (rel > worst) worst = rel;
    lost += (double)a * (double)b - six;
    total += (double)a * (double)b;
  }
  printf("dropped products on [250, 300]: one product max %.3g of |a||b|, the sum %.3g of sum |a||b|\n", worst, lost / total);
  CHECK(worst <= 0x1p-21 + 0x1p-30, "the dropped products of one pair reach %.3g", worst);
  CHECK(fabs(lost / total) <= 0x1p-22, "the dropped products of the sum reach %.3g", lost / total);
}

int main() {
  long n = 0;
  // every normal binade, random mantissas, both signs; 8, 16 and 24 significant bits
  for (int e = 1; e <= 254; ++e)
    for (int t = 0; t < 4000; ++t) {
      const uint32_t sign = (rnd() & 1u) << 31, mant = rnd() & 0x007FFFFFu;
      const uint32_t keep[3] = {0x007F0000u, 0x007FFF00u, 0x007FFFFFu};
      const float partner = from_bits(((rnd() % 254u + 1u) << 23) | (rnd() & 0x007FFFFFu));
      for (int w = 0; w < 3; ++w) {
        check_finite(from_bits(sign | ((uint32_t)e << 23) | (mant & keep[w])), partner);
        ++n;
      }
    }
  check_finite(0.0f, 1.0f);
  check_finite(-0.0f, -3.5f);
  check_finite(1.0f, 0.0f);
  check_finite(from_bits(0x7F7FFFFFu), from_bits(0xFF7FFFFFu));   // +-FLT_MAX
  check_finite(from_bits(0x00800000u), 1.0f);                     // smallest normal: the planes below it are exact subnormals
  // non-finite: +-Inf, quiet / signalling / payload-low NaNs, both slots, random finite partners
  const uint32_t nf[10] = {0x7F800000u, 0xFF800000u, 0x7FC00000u, 0xFFC00000u, 0x7F800001u, 0xFF800001u,
                           0x7FA00000u, 0x7F80FFFFu, 0x7FFFFFFFu, 0xFF810000u};
  for (int i = 0; i < 10; ++i)
    for (int t = 0; t < 1000; ++t)
      check_non_finite(nf[i], from_bits(((rnd() % 254u + 1u) << 23) | (rnd() & 0x807FFFFFu)));
  for (int t = 0; t < 100000; ++t) check_non_finite(0x7F800000u | (rnd() & 0x807FFFFFu), 1.5f);
  check_gram_classes();
  check_dropped_terms();
  printf("%ld finite values\n%d failed\n", n, g_failed);
  return g_failed != 0;
}
