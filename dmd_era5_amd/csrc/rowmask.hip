// K20: which rows (grid points) of a row block hold a missing value, and one value for all of those rows.
//
//   count   one read of X:   count[i] += number of snapshots j with X[j, i] not finite   (int32, accumulates)
//   apply   stores only:     X[j, i] = value for every j where count[i] != 0; other rows are neither read nor written
//
// X is the package's image of a row block: n snapshots of m floats, snapshot j at X + j ldx.  "Not finite" is a test
// of the bit pattern (exponent all ones), on integer registers: no floating-point option can fold it away.
//
// Launch: K5's aligned tile -- TX row lanes of one float4 each x TY time lanes, a wave reads 1 KiB of one snapshot per
// load -- and, new here, grid.y splits the snapshots, so that a narrow block with many snapshots still fills the chip.
// count: the time lanes of a workgroup meet in LDS; workgroups of different splits meet in integer atomics on count
// (integer adds commute: the result does not depend on their order).  R = 1 is the dword-per-lane route for an X whose
// base or leading dimension does not allow 16-byte accesses.  apply: see its kernel.
#include "dmdx_common.h"

namespace {

constexpr int kTX = 64, kTY = 4;                 // lanes of a workgroup: rows (x R) x time
constexpr int64_t kMinSplit = 64;                // a time split is never shorter than this many snapshots ...
constexpr int64_t kTargetWorkgroups = 2048;      // ... and splits stop once the launch has 8 workgroups per CU
constexpr int64_t kApplySplit = 64;               // snapshots per time split of apply (a multiple of kTY)

__device__ __forceinline__ int not_finite(uint32_t bits) { return (bits & 0x7F800000u) == 0x7F800000u ? 1 : 0; }

template <int R>
__global__ __launch_bounds__(kTX * kTY) void row_missing_count_kernel(const uint32_t* __restrict__ X, int64_t n,
                                                                      int64_t m, int64_t ldx, int64_t per_split,
                                                                      int32_t* __restrict__ count) {
  __shared__ int32_t red[kTY][kTX * R + 1];
  typedef uint32_t vec __attribute__((ext_vector_type(R)));
  const int tx = threadIdx.x & (kTX - 1), ty = threadIdx.x / kTX;
  const int64_t r0 = ((int64_t)blockIdx.x * kTX + tx) * R;
  const int nr = r0 < m ? ((m - r0) < R ? (int)(m - r0) : R) : 0;
  const int64_t j0 = (int64_t)blockIdx.y * per_split;
  const int64_t j1 = j0 + per_split < n ? j0 + per_split : n;
  const uint32_t* xp = X + (nr ? r0 : 0);

  int32_t c[R];
#pragma unroll
  for (int e = 0; e < R; ++e) c[e] = 0;
  if (nr == R) {
#pragma unroll 8
    for (int64_t j = j0 + ty; j < j1; j += kTY) {
      const vec v = *reinterpret_cast<const vec*>(xp + j * ldx);
#pragma unroll
      for (int e = 0; e < R; ++e) c[e] += not_finite(v[e]);
    }
  } else if (nr > 0) {                                           // the one ragged quad at the end of the rows
    for (int64_t j = j0 + ty; j < j1; j += kTY)
      for (int e = 0; e < nr; ++e) c[e] += not_finite(xp[j * ldx + e]);
  }
#pragma unroll
  for (int e = 0; e < R; ++e) red[ty][R * tx + e] = c[e];
  __syncthreads();
  if (ty != 0) return;
  for (int e = 0; e < nr; ++e) {
    int32_t t = 0;
#pragma unroll
    for (int k = 0; k < kTY; ++k) t += red[k][R * tx + e];
    if (t != 0) atomicAdd(count + r0 + e, t);
  }
}

// apply: a workgroup owns 256 consecutive rows and one time split; its four waves are four time lanes over the same
// rows (a quad of rows per lane), so every wave sees the same mask.
//   QUAD (a 16-byte aligned X with ldx % 4 == 0): a quad whose four rows are all masked goes out as one 16-byte store
//   per snapshot -- the runs of rows a land mask is made of.
//   Every other masked row (QUAD: the quads an edge of the mask or m cuts; otherwise all of them) must leave its
//   neighbours alone and is stored dword by dword.  Those rows are first compacted into a list in LDS, and the 256 lanes
//   walk the (snapshot, listed row) pairs in order: every lane of a store instruction is active and neighbouring lanes
//   hit neighbouring masked rows of one snapshot.  (One lane per row or per quad, with the unmasked lanes switched off,
//   issues 3.3 times the store instructions on a mask of single points.  It was no slower for that: such a mask is
//   bound by the partial lines it writes, MEASUREMENTS.md "K20"; the list keeps the instruction stream out of the way.)
template <bool QUAD>
__global__ __launch_bounds__(kTX * kTY) void row_mask_apply_kernel(float* __restrict__ X, int64_t n, int64_t m,
                                                                   int64_t ldx, int64_t per_split,
                                                                   const int32_t* __restrict__ count, float value) {
  static_assert(kTX == 64, "a wave is one time lane: the ballots below span the 256 rows");
  __shared__ int32_t listed[4 * kTX];
  const int tx = threadIdx.x & (kTX - 1), ty = threadIdx.x / kTX;
  const int64_t w0 = (int64_t)blockIdx.x * (4 * kTX);            // first row of the workgroup
  const int64_t r0 = w0 + 4 * tx;
  const int nr = r0 < m ? ((m - r0) < 4 ? (int)(m - r0) : 4) : 0;
  bool on[4];
  int masked = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    on[e] = e < nr && count[r0 + e] != 0;
    masked += on[e] ? 1 : 0;
  }
  const bool full = QUAD && masked == 4;
  // the list: the masked rows that are not part of a full quad, in row order (the same in every wave)
  const unsigned long long below = (1ull << tx) - 1ull;
  int n_listed = 0, pos = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const unsigned long long b = __ballot(on[e] && !full);
    n_listed += __popcll(b);
    pos += __popcll(b & below);
  }
  if (n_listed == 0 && __ballot(full) == 0) return;              // nothing of these 256 rows is masked (workgroup-uniform)
  if (ty == 0 && !full) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (on[e]) listed[pos++] = 4 * tx + e;
  }
  __syncthreads();
  const int64_t j0 = (int64_t)blockIdx.y * per_split;
  const int64_t len = (j0 + per_split < n ? j0 + per_split : n) - j0;

  if (full) {
    const f32x4 v = {value, value, value, value};
    float* xp = X + r0 + j0 * ldx;
#pragma unroll 8
    for (int64_t j = ty; j < len; j += kTY) *reinterpret_cast<f32x4*>(xp + j * ldx) = v;
  }
  if (n_listed == 0) return;
  // pair i = j * n_listed + r (snapshot j of the split, entry r of the list); a lane takes i = tid, tid + 256, ...
  const int step_j = (kTX * kTY) / n_listed, step_r = (kTX * kTY) % n_listed;
  int64_t j = threadIdx.x / n_listed;
  int r = threadIdx.x % n_listed;
  float* xp = X + w0 + j0 * ldx;
  while (j < len) {
    xp[j * ldx + listed[r]] = value;
    j += step_j;
    r += step_r;
    if (r >= n_listed) {
      r -= n_listed;
      ++j;
    }
  }
}

int check_shape(const char* who, const void* X, int64_t n, int64_t m, int64_t ldx, const void* count) {
  DMDX_CHECK_ARG(n >= 0 && m >= 0, "%s: negative size (n=%lld m=%lld)", who, (long long)n, (long long)m);
  DMDX_CHECK_ARG(n < kMaxSize && m < kMaxSize && ldx < kMaxSize, "%s: a size >= 2^31 (n=%lld m=%lld ldx=%lld)", who,
                 (long long)n, (long long)m, (long long)ldx);
  if (n == 0 || m == 0) return 0;
  DMDX_CHECK_ARG(X && count, "%s: null pointer", who);
  DMDX_CHECK_ARG(ldx >= m, "%s: ldx=%lld < m=%lld", who, (long long)ldx, (long long)m);
  DMDX_CHECK_ARG(((uintptr_t)X & 3u) == 0 && ((uintptr_t)count & 3u) == 0, "%s: a pointer is not aligned to its element",
                 who);
  return 0;
}

// grid.x: the row chunks of one workgroup, grid.y: the time splits.  -> snapshots per split (a multiple of kTY)
int64_t plan(int64_t n, int64_t m, int R, dim3* grid) {
  const int64_t gx = (m + kTX * R - 1) / (kTX * R);
  int64_t splits = (kTargetWorkgroups + gx - 1) / gx;
  const int64_t most = (n + kMinSplit - 1) / kMinSplit;
  if (splits > most) splits = most;
  if (splits < 1) splits = 1;
  int64_t per = (n + splits - 1) / splits;
  per = (per + kTY - 1) / kTY * kTY;
  splits = (n + per - 1) / per;
  *grid = dim3((unsigned)gx, (unsigned)splits);
  return per;
}

// apply: fixed, short time splits (measured on a cfg2 block: 16, 64, 256 and 1752 snapshots per split differ by 8 % at
// the most, the short ones ahead), so that the workgroups that hold masked rows are many whatever the mask is.
int64_t plan_apply(int64_t n, int64_t m, dim3* grid) {
  int64_t per = kApplySplit;
  if ((n + per - 1) / per > 65535) per = ((n + 65534) / 65535 + kTY - 1) / kTY * kTY;
  *grid = dim3((unsigned)((m + 4 * kTX - 1) / (4 * kTX)), (unsigned)((n + per - 1) / per));
  return per;
}

}  // namespace

extern "C" int dmdx_row_missing_count_f32(const float* X, int64_t n, int64_t m, int64_t ldx, int32_t* count,
                                          void* stream) {
  if (int rc = check_shape("row_missing_count", X, n, m, ldx, count)) return rc;
  if (n == 0 || m == 0) return 0;
  const uint32_t* bits = reinterpret_cast<const uint32_t*>(X);
  dim3 grid;
  if (ldx % 4 == 0 && dmdx_aligned16(X)) {
    const int64_t per = plan(n, m, 4, &grid);
    hipLaunchKernelGGL(row_missing_count_kernel<4>, grid, dim3(kTX * kTY), 0, (hipStream_t)stream, bits, n, m, ldx, per,
                       count);
  } else {
    const int64_t per = plan(n, m, 1, &grid);
    hipLaunchKernelGGL(row_missing_count_kernel<1>, grid, dim3(kTX * kTY), 0, (hipStream_t)stream, bits, n, m, ldx, per,
                       count);
  }
  DMDX_LAUNCH_CHECK();
  return 0;
}

extern "C" int dmdx_row_mask_apply_f32(float* X, int64_t n, int64_t m, int64_t ldx, const int32_t* count, float value,
                                       void* stream) {
  if (int rc = check_shape("row_mask_apply", X, n, m, ldx, count)) return rc;
  if (n == 0 || m == 0) return 0;
  dim3 grid;
  if (ldx % 4 == 0 && dmdx_aligned16(X)) {
    const int64_t per = plan_apply(n, m, &grid);
    hipLaunchKernelGGL(row_mask_apply_kernel<true>, grid, dim3(kTX * kTY), 0, (hipStream_t)stream, X, n, m, ldx, per, count,
                       value);
  } else {
    const int64_t per = plan_apply(n, m, &grid);
    hipLaunchKernelGGL(row_mask_apply_kernel<false>, grid, dim3(kTX * kTY), 0, (hipStream_t)stream, X, n, m, ldx, per, count,
                       value);
  }
  DMDX_LAUNCH_CHECK();
  return 0;
}
