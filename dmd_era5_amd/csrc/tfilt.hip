// K22: a FIR filter along time with an output stride -- the daily mean, the running mean, a Lanczos low-pass followed
// by decimation, a band-pass -- of the snapshots of one row block, on the device.
//
//   Y[i, u] = fp32( sum over j < L of fp64(X[i, u stride + j]) * h[j] )          u < T_out, "valid" windows only
//
// One HBM stream: X is read ((R - 1) stride + L) / R times per output from a lane's point of view (its neighbours in
// grid.y re-read the halo) and Y is written once.
//
// Arithmetic (the contract of tests/tfilt_ref.py, held bit for bit): per (row, output) one fp64 chain that starts at
// +0.0 and adds one rounded product per tap in ascending j, one rounding to fp32.  Every multiply that meets an add
// is two roundings: contraction is switched off for the whole file.  No symmetric-tap folding.
//
// A lane owns a quad of 4 consecutive rows and a run of kRun consecutive outputs.  Where the windows of a run overlap
// (stride < L) and the quad is the same for every output of the run (ldy % 4 == 0), the lane keeps kRun x 4 fp64
// accumulators in registers and walks the union window [u0 stride, (u0 + kRun - 1) stride + L) once in ascending t:
// every loaded snapshot is added to each output whose window holds it, so each output still sees its taps in
// ascending j.  Otherwise (block means: stride >= L, where every input feeds one output; or a Y whose rows change
// their 16-byte phase from output to output) the lane forms its outputs one after another.  The tap h[t - u stride]
// is the same for every lane of a launch: wave-uniform loads.
#include "time_rows.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxTaps = 2048;
#ifndef DMDX_TFILT_RUN
#define DMDX_TFILT_RUN 8
#endif
constexpr int kRun = DMDX_TFILT_RUN;     // outputs per lane: kRun x 4 fp64 accumulators (MEASUREMENTS.md K22)
constexpr int kInFlight = 4;             // snapshot loads issued before their adds (8 in the one-output walk)

// The quad of snapshot t: 4 floats at xp + t ldx.  VEC: one 16-byte load (the caller has checked the address);
// FULL: all 4 rows exist; otherwise rows lo .. hi - 1 only, element by element, the others 0 (never stored).
template <bool VEC, bool FULL>
__device__ __forceinline__ f32x4 ldq(const float* __restrict__ p, int lo, int hi) {
  if (VEC) return *reinterpret_cast<const f32x4*>(p);
  f32x4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = (FULL || (e >= lo && e < hi)) ? p[e] : 0.f;
  return v;
}

template <bool FULL>
__device__ __forceinline__ void stq(float* yp, const double (&acc)[4], int lo, int hi) {
  if (FULL) {                                                   // aligned by the head shift of the caller
    f32x4 y;
#pragma unroll
    for (int e = 0; e < 4; ++e) y[e] = (float)acc[e];
    *reinterpret_cast<f32x4*>(yp) = y;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e >= lo && e < hi) yp[e] = (float)acc[e];
  }
}

// One output: the L taps of the window that starts at xp (= X + u stride ldx + r), in ascending j.
template <bool VEC, bool FULL>
__device__ __forceinline__ void tfilt_one(const float* __restrict__ xp, int lo, int hi, int64_t ldx,
                                          const double* __restrict__ h, int L, float* yp) {
  constexpr int kFly = 2 * kInFlight;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  int j = 0;
  for (; j + kFly <= L; j += kFly) {
    f32x4 v[kFly];
#pragma unroll
    for (int q = 0; q < kFly; ++q) v[q] = ldq<VEC, FULL>(xp + (j + q) * ldx, lo, hi);
#pragma unroll
    for (int q = 0; q < kFly; ++q) {
      const double w = h[j + q];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double p = (double)v[q][e] * w;                   // a rounded product of its own
        acc[e] = acc[e] + p;
      }
    }
  }
  for (; j < L; ++j) {
    const f32x4 v = ldq<VEC, FULL>(xp + j * ldx, lo, hi);
    const double w = h[j];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double p = (double)v[e] * w;
      acc[e] = acc[e] + p;
    }
  }
  stq<FULL>(yp, acc, lo, hi);
}

// A run of nout <= kRun outputs whose windows overlap: one walk over the union window, that starts at xp
// (= X + u0 stride ldx + r).  Snapshot s of the walk is tap s - k stride of output k where that lies in [0, L).
// With all kRun outputs present and (kRun - 1) stride < L, the snapshots s in [(kRun - 1) stride, L) feed every
// output: that interior runs without a test; the ramps before and behind it test every (s, k).
template <bool VEC, bool FULL>
__device__ __forceinline__ void tfilt_run(const float* __restrict__ xp, int lo, int hi, int64_t ldx,
                                          const double* __restrict__ h, int L, int64_t stride, int nout, float* yp,
                                          int64_t ldy) {
  double acc[kRun][4];
#pragma unroll
  for (int k = 0; k < kRun; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[k][e] = 0.0;

  const int64_t W = (nout - 1) * stride + L;                    // snapshots of the union window
  const bool inner = nout == kRun && (kRun - 1) * stride < L;
  const int64_t a = inner ? (kRun - 1) * stride : W;            // [0, a) ramp up, [a, b) interior, [b, W) ramp down
  const int64_t b = inner ? L : W;

  auto ramp = [&](int64_t s0, int64_t s1) {
    for (int64_t s = s0; s < s1; ++s) {
      const f32x4 v = ldq<VEC, FULL>(xp + s * ldx, lo, hi);
      double x[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) x[e] = (double)v[e];
#pragma unroll
      for (int k = 0; k < kRun; ++k) {
        const int64_t j = s - k * stride;
        if (k < nout && j >= 0 && j < L) {
          const double w = h[j];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const double p = x[e] * w;
            acc[k][e] = acc[k][e] + p;
          }
        }
      }
    }
  };

  ramp(0, a);
  int64_t s = a;
  for (; s + kInFlight <= b; s += kInFlight) {
    f32x4 v[kInFlight];
#pragma unroll
    for (int q = 0; q < kInFlight; ++q) v[q] = ldq<VEC, FULL>(xp + (s + q) * ldx, lo, hi);
#pragma unroll
    for (int q = 0; q < kInFlight; ++q) {
      double x[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) x[e] = (double)v[q][e];
#pragma unroll
      for (int k = 0; k < kRun; ++k) {
        const double w = h[s + q - k * stride];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const double p = x[e] * w;
          acc[k][e] = acc[k][e] + p;
        }
      }
    }
  }
  for (; s < b; ++s) {
    const f32x4 v = ldq<VEC, FULL>(xp + s * ldx, lo, hi);
#pragma unroll
    for (int k = 0; k < kRun; ++k) {
      const double w = h[s - k * stride];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double p = (double)v[e] * w;
        acc[k][e] = acc[k][e] + p;
      }
    }
  }
  ramp(b, W);

#pragma unroll
  for (int k = 0; k < kRun; ++k)
    if (k < nout) stq<FULL>(yp + k * ldy, acc[k], lo, hi);
}

// grid.x: chunks of 4 consecutive rows per lane; grid.y: runs of kRun outputs (strided when there are more than
// gridDim.y).  The chunks are head-shifted so that every full chunk of Y goes out as one aligned 16-byte store
// (the geometry of Quad, time_rows.h).  X is read with 16-byte loads where ldx % 4 == 0 and the address of the
// lane's quad allows it (an aligned X under a Y of phase 0), element by element otherwise.  RUN: ldy % 4 == 0, so the
// head -- and with it the quad -- is the same for every output, and stride < L.
template <bool RUN>
__global__ __launch_bounds__(256) void tfilt_kernel(const float* __restrict__ X, int64_t m, int64_t ldx,
                                                    const double* __restrict__ h, int L, int64_t stride,
                                                    float* __restrict__ Y, int64_t T_out, int64_t ldy) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t nrun = (T_out + kRun - 1) / kRun;
  const bool ldx4 = ldx % 4 == 0;
  for (int64_t run = blockIdx.y; run < nrun; run += gridDim.y) {
    const int64_t u0 = run * kRun;
    const int nout = T_out - u0 < kRun ? (int)(T_out - u0) : kRun;
    for (int k = 0; k < (RUN ? 1 : nout); ++k) {
      float* yu = Y + (u0 + k) * ldy;
      const int head = (int)(((uintptr_t)yu >> 2) & 3u);       // Quad<4> of time_rows.h, spelled out: with quad_at
      const int64_t r = c * 4 - head;                            // the compiler swaps the operands of one s_and_b64
      if (r >= m) continue;
      const int lo = r < 0 ? (int)(-r) : 0;
      const int hi = m - r < 4 ? (int)(m - r) : 4;
      const bool full = lo == 0 && hi == 4;
      const float* xp = X + (u0 + k) * stride * ldx + r;
      const bool vec = full && ldx4 && ((uintptr_t)xp & 15u) == 0;
      if (RUN) {
        if (vec) tfilt_run<true, true>(xp, lo, hi, ldx, h, L, stride, nout, yu + r, ldy);
        else if (full) tfilt_run<false, true>(xp, lo, hi, ldx, h, L, stride, nout, yu + r, ldy);
        else tfilt_run<false, false>(xp, lo, hi, ldx, h, L, stride, nout, yu + r, ldy);
      } else {
        if (vec) tfilt_one<true, true>(xp, lo, hi, ldx, h, L, yu + r);
        else if (full) tfilt_one<false, true>(xp, lo, hi, ldx, h, L, yu + r);
        else tfilt_one<false, false>(xp, lo, hi, ldx, h, L, yu + r);
      }
    }
  }
}

}  // namespace

extern "C" int dmdx_tfilt_max_taps(void) { return kMaxTaps; }

extern "C" int dmdx_tfilt_f32(const float* X, int64_t m, int64_t T, int64_t ldx, const double* h, int64_t L, int64_t stride,
                              float* Y, int64_t T_out, int64_t ldy, void* stream) {
  DMDX_CHECK_ARG(X && h && Y, "tfilt: null pointer");
  DMDX_CHECK_ARG(L >= 1 && L <= kMaxTaps, "tfilt: L=%lld outside 1..%d", (long long)L, kMaxTaps);
  DMDX_CHECK_ARG(stride >= 1 && stride < kMaxSize, "tfilt: stride=%lld outside 1..2^31-1", (long long)stride);
  DMDX_CHECK_ARG(T_out >= 0 && T_out < kMaxSize, "tfilt: T_out=%lld outside 0..2^31-1", (long long)T_out);
  if (int rc = check_block("tfilt", m, T, {{"ldx", ldx}, {"ldy", ldy}}, {X, Y}, {h})) return rc;
  DMDX_CHECK_ARG((T_out - 1) * stride + L <= T, "tfilt: the last window ends at (T_out - 1) stride + L = %lld > T=%lld",
                 (long long)((T_out - 1) * stride + L), (long long)T);
  if (int rc = check_ranges("tfilt", X, T, ldx, Y, T_out, ldy, m, false)) return rc;   // (there is no in-place form)
  if (m == 0 || T_out == 0) return 0;
  const int64_t nrun = (T_out + kRun - 1) / kRun;
  const dim3 grid((unsigned)((chunks_of<4>(m) + 255) / 256), grid_rows(nrun));
  // every stride < L takes the union-window walk, also where the windows barely overlap ((kRun - 1) stride >= L: no
  // interior, every snapshot goes through the tested ramp); whether single outputs would be faster there is not measured
  if (stride < L && ldy % 4 == 0)
    hipLaunchKernelGGL(tfilt_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, X, m, ldx, h, (int)L, stride, Y, T_out,
                       ldy);
  else
    hipLaunchKernelGGL(tfilt_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, X, m, ldx, h, (int)L, stride, Y, T_out,
                       ldy);
  DMDX_LAUNCH_CHECK();
  return 0;
}
