// An fp32 value as three bf16 planes, x = h + m + l exactly (truncation splits: each plane holds the top 8
// significant bits of what the planes before it leave), packed two values per dword for the bf16 MFMA.
// K1's 128 x 128 SYRK tiles (gemm_tn.hip, tn_unit) contract the six plane products h h, h' m, m h', h' l, m m,
// l h' on v_mfma_f32_32x32x16_bf16; the three dropped ones (m l, l m, l l) stay below 2^-21 |a b| per pair
// of values (truncation: m < 2^-7, l < 2^-15 of the binade) and come to about 2^-23 sum |a b| over a sum, one-signed
// on all-positive data.
//
// Two forms that give the SAME planes for every finite value.  K1 runs the fast one everywhere and asks once per work
// unit, on the unit's result, whether it was enough (alarm); only a unit that raised the alarm runs again, from its
// first chunk, on the class-safe form.
//   split2_fast  and / subtract / pack, nothing else in the loop.  A non-finite x leaves NaN in m and l (Inf - Inf,
//                NaN - Inf): the packed l plane of EVERY Inf and NaN is a bf16 NaN (all 2^24 patterns:
//                tests/host/bf16_fastnan_main.cpp).  The l plane is the carrier of the alarm: K1 contracts l h' and
//                h' l for every pair, so every output that a non-finite input feeds is NaN at the end of the unit,
//                whatever the partner holds (NaN * 0 is NaN), and an output that none feeds never sees such a plane.
//                No NaN in the unit's result: the fast planes were the right ones.
//   split2_safe  the rerun.  The class rule of the value contract: a non-finite x keeps its class in h (Inf stays Inf,
//                every NaN becomes a quiet bf16 NaN -- truncation alone would turn a NaN whose payload sits in
//                the low 16 bits into Inf), m = l = 0, and the copy h' for the four cross products holds 0 in
//                its place: Inf then meets only the h of its partner, which is non-zero exactly when the
//                (normal) partner is, where a zero m or l plane of a finite partner would give Inf * 0 = NaN.
//                The rule assumes NORMAL partners: a subnormal below 2^-133 truncates to h = 0 (and the bf16 matrix
//                core may flush the bf16 subnormals above it), so Inf times such a partner is NaN where numpy has
//                Inf.  The library's magnitude interval (dmdx.h: |x| in [2^-40, 2^40], zeros apart) excludes them.
// A power of two commutes with the split as long as no plane turns subnormal (|x| >= 2^-103: l >= 2^-23 |x|).
// Host + device: the header compiles alone with a host compiler (tests/host/bf16_split_main.cpp).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DMDX_SPLIT_HD __host__ __device__ inline
#else
#define DMDX_SPLIT_HD inline
#endif

namespace bf16split {

constexpr uint32_t TOP16 = 0xFFFF0000u;

DMDX_SPLIT_HD uint32_t bits(float x) {
  uint32_t u;
  __builtin_memcpy(&u, &x, 4);
  return u;
}
DMDX_SPLIT_HD float from_bits(uint32_t u) {
  float x;
  __builtin_memcpy(&x, &u, 4);
  return x;
}

// the bf16 patterns of two fp32 bit patterns whose low 16 bits do not matter: `a` in the low half
DMDX_SPLIT_HD uint32_t pack2(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(b, a, 0x07060302u);
#else
  return (b & TOP16) | (a >> 16);
#endif
}

// running detector: stays a (signed) zero over finite values, NaN from the first Inf or NaN on
// (the per-group detector of the first plane k-step; K1 no longer runs it -- the host checks still hold it to its word)
DMDX_SPLIT_HD float detect(float x, float s) { return __builtin_fmaf(x, 0.0f, s); }
DMDX_SPLIT_HD bool fired(float s) { return s != s; }

// the verdict on one value of a unit's result: a NaN there <= a non-finite input (or Inf - Inf after overflow) fed it
DMDX_SPLIT_HD bool alarm(float v) { return v != v; }

DMDX_SPLIT_HD bool non_finite(uint32_t u) { return (u & 0x7F800000u) == 0x7F800000u; }

// one value: h, m, l as fp32 bit patterns with zero low halves (finite x only)
DMDX_SPLIT_HD void split1(float x, uint32_t& h, uint32_t& m, uint32_t& l) {
  h = bits(x) & TOP16;
  const float r = x - from_bits(h);
  m = bits(r) & TOP16;
  l = bits(r - from_bits(m));
}

// two values -> the packed planes (x0 in the low half)
DMDX_SPLIT_HD void split2_fast(float x0, float x1, uint32_t& H, uint32_t& M, uint32_t& L) {
  uint32_t h0, m0, l0, h1, m1, l1;
  split1(x0, h0, m0, l0);
  split1(x1, h1, m1, l1);
  H = pack2(bits(x0), bits(x1));
  M = pack2(m0, m1);
  L = pack2(l0, l1);
}

#if defined(__HIPCC__)
// The fast form on a register pair, for the kernel: the same and / subtract / pack on both values at once (the two
// subtractions are one packed fp32 instruction each): the same planes as split2_fast, operation for operation.
// (detect_pair: the retired per-group detector on a pair, one packed fma; it stays (+-0, +-0) over finite values.)
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
DMDX_SPLIT_HD void split2_fast_pair(f32x2_t x, uint32_t& H, uint32_t& M, uint32_t& L) {
  const u32x2_t xb = __builtin_bit_cast(u32x2_t, x);
  const f32x2_t r = x - __builtin_bit_cast(f32x2_t, xb & TOP16);
  const u32x2_t mb = __builtin_bit_cast(u32x2_t, r) & TOP16;
  const u32x2_t lb = __builtin_bit_cast(u32x2_t, r - __builtin_bit_cast(f32x2_t, mb));
  H = pack2(xb[0], xb[1]);
  M = pack2(mb[0], mb[1]);
  L = pack2(lb[0], lb[1]);
}
DMDX_SPLIT_HD f32x2_t detect_pair(f32x2_t x, f32x2_t s) { return __builtin_elementwise_fma(x, (f32x2_t){0.0f, 0.0f}, s); }
#endif

// 0xFFFF in every half of a packed plane whose exponent is all ones (Inf, NaN), 0 in the others
DMDX_SPLIT_HD uint32_t non_finite_halves(uint32_t P) {
  const uint32_t t = ((P & 0x7F807F80u) + 0x00800080u) & 0x80008000u;   // bit 15 / 31 set where the half is non-finite
  return (t >> 15) * 0xFFFFu;
}

// The class rule, in place on the planes split2_fast made of (x0, x1): a NaN is quiet in H whatever its payload
// was, m = l = 0 for a non-finite value (the fast form leaves NaN there: Inf - Inf).  Finite values: no change.
DMDX_SPLIT_HD void make_safe2(float x0, float x1, uint32_t& H, uint32_t& M, uint32_t& L) {
  H |= (x0 != x0 ? 0x00000040u : 0u) | (x1 != x1 ? 0x00400000u : 0u);
  const uint32_t keep = ~non_finite_halves(H);
  M &= keep;
  L &= keep;
}

// HP from a packed H: the copy for the four cross products, 0 in place of a non-finite value
DMDX_SPLIT_HD uint32_t sanitise2(uint32_t H) { return H & ~non_finite_halves(H); }

// H: for the product h h alone; HP: the sanitised copy
DMDX_SPLIT_HD void split2_safe(float x0, float x1, uint32_t& H, uint32_t& HP, uint32_t& M, uint32_t& L) {
  split2_fast(x0, x1, H, M, L);
  make_safe2(x0, x1, H, M, L);
  HP = sanitise2(H);
}

}  // namespace bf16split
