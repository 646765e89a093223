// K14: CF-packed int16 codes -> fp32 snapshots of one row block, on the device.
//
// The ingest moves a packed variable as it sits in the file (2 bytes per value through the file
// system, the pinned staging and PCIe) and unpacks it in HBM: one streaming launch per row block
// reads 2 bytes and writes 4 per element, and replaces both the host cast and the strided device
// copy of the fp32 route.  The level selection and a shard's latitude band are one table of
// segment offsets (one segment per selected level), so the launch gathers while it unpacks.
//
// Arithmetic (the contract of the reader's host decode, tests/unpack_ref.py):
//   x = fp32( fp64(q) * scale_factor + add_offset )      fp64 multiply, fp64 add, one rounding to fp32
// The multiply and the add are two roundings: the helper below switches contraction off, because
// hipcc contracts a * b + c to an FMA by default (also through __dmul_rn / __dadd_rn, which are
// plain operators in this toolchain).
#include "time_rows.h"

namespace {

struct UnpackSegs {
  int64_t off[64];
};

constexpr int kChunk = 8;          // codes per lane: one 16-byte load, two 16-byte stores

__device__ __forceinline__ float unpack_value(int q, double sf, double ao) {
#pragma clang fp contract(off)
  const double prod = (double)q * sf;
  const double sum = prod + ao;
  return (float)sum;
}

// grid.x: chunks of 8 consecutive rows (256 lanes per workgroup), grid.y: snapshots (strided when
// T > gridDim.y).  The chunks are head-shifted (quad_at, time_rows.h), so that every full chunk is
// stored with two aligned 16-byte stores whatever X and ldx are; the ragged chunks at both
// ends of a column, the chunks that straddle two segments and the sources that are not 16-byte
// aligned go element by element.  Both routes apply unpack_value to the same codes.
__global__ __launch_bounds__(256) void unpack_i16_kernel(const int16_t* __restrict__ S, int64_t lds, int64_t T,
                                                         int64_t tstep, int64_t rows, uint32_t row0, uint32_t plane,
                                                         UnpackSegs segs, double sf, double ao, int nfill, int fill0,
                                                         int fill1, float* __restrict__ X, int64_t ldx,
                                                         unsigned long long* __restrict__ fill_count) {
  __shared__ unsigned wave_fills[4];
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  unsigned nf = 0;

  auto one = [&](int q) -> float {
    const bool isfill = (nfill > 0 && q == fill0) || (nfill > 1 && q == fill1);
    nf += isfill ? 1u : 0u;
    return isfill ? __builtin_bit_cast(float, kQuietNaN) : unpack_value(q, sf, ao);
  };

  for (int64_t j = blockIdx.y; j < T; j += gridDim.y) {
    float* xj = X + j * ldx;
    Quad<kChunk> q = quad_at<kChunk>(xj, c);
    if (q.past(rows)) continue;
    q.clip(rows);
    const int64_t r = q.r;
    const int16_t* sj = S + j * tstep * lds;
    const uint32_t g = row0 + (uint32_t)(r + q.lo);             // row inside the variable (< 2^31, host-checked)
    uint32_t sg = g / plane;
    uint32_t p = g - sg * plane;

    if (q.full() && p + kChunk <= plane) {
      const int16_t* sp = sj + segs.off[sg] + p;
      short q[kChunk];
      if (((uintptr_t)sp & 15u) == 0) {
        typedef short i16x8 __attribute__((ext_vector_type(8)));
        const i16x8 v = *reinterpret_cast<const i16x8*>(sp);
#pragma unroll
        for (int e = 0; e < kChunk; ++e) q[e] = v[e];
      } else {
#pragma unroll
        for (int e = 0; e < kChunk; ++e) q[e] = sp[e];
      }
      f32x4 a, b;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        a[e] = one(q[e]);
        b[e] = one(q[e + 4]);
      }
      *reinterpret_cast<f32x4*>(xj + r) = a;
      *reinterpret_cast<f32x4*>(xj + r + 4) = b;
    } else {
      for (int e = q.lo; e < q.hi; ++e) {
        while (p >= plane) {                                  // into the next segment(s)
          p -= plane;
          ++sg;
        }
        xj[r + e] = one(sj[segs.off[sg] + p]);
        ++p;
      }
    }
  }

  if (fill_count) {                                           // (uniform: every lane gets here)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) nf += __shfl_down(nf, off, 64);
    if ((threadIdx.x & 63) == 0) wave_fills[threadIdx.x >> 6] = nf;
    __syncthreads();
    if (threadIdx.x == 0) {
      const unsigned tot = wave_fills[0] + wave_fills[1] + wave_fills[2] + wave_fills[3];
      if (tot) atomicAdd(fill_count, (unsigned long long)tot);
    }
  }
}

}  // namespace

extern "C" int dmdx_unpack_i16_f32(const int16_t* S, int64_t lds, int64_t T, int64_t tstep, int64_t rows, int64_t row0,
                                   int64_t plane, int nseg, const int64_t* host_seg_offset, double scale_factor,
                                   double add_offset, int nfill, int fill0, int fill1, float* X, int64_t ldx,
                                   unsigned long long* fill_count, void* stream) {
  DMDX_CHECK_ARG(T >= 0 && rows >= 0 && row0 >= 0 && lds >= 0, "unpack_i16: negative size (T=%lld rows=%lld row0=%lld lds=%lld)",
                 (long long)T, (long long)rows, (long long)row0, (long long)lds);
  DMDX_CHECK_ARG(tstep >= 1, "unpack_i16: tstep=%lld < 1", (long long)tstep);
  DMDX_CHECK_ARG(nseg >= 1 && nseg <= 64, "unpack_i16: nseg=%d outside 1..64", nseg);
  DMDX_CHECK_ARG(nfill >= 0 && nfill <= 2, "unpack_i16: nfill=%d outside 0..2", nfill);
  DMDX_CHECK_ARG(ldx >= rows, "unpack_i16: ldx=%lld < rows=%lld", (long long)ldx, (long long)rows);
  DMDX_CHECK_ARG(plane >= 1 && (int64_t)nseg * plane < (int64_t(1) << 31),
                 "unpack_i16: plane=%lld with nseg=%d: need 1 <= plane and nseg * plane < 2^31", (long long)plane, nseg);
  DMDX_CHECK_ARG(row0 + rows <= (int64_t)nseg * plane, "unpack_i16: rows %lld..%lld leave the %d segments of %lld",
                 (long long)row0, (long long)(row0 + rows), nseg, (long long)plane);
  DMDX_CHECK_ARG(host_seg_offset, "unpack_i16: null segment table");
  UnpackSegs segs;
  for (int i = 0; i < 64; ++i) segs.off[i] = i < nseg ? host_seg_offset[i] : 0;
  for (int i = 0; i < nseg; ++i)
    DMDX_CHECK_ARG(segs.off[i] >= 0, "unpack_i16: seg_offset[%d]=%lld < 0", i, (long long)segs.off[i]);
  if (T == 0 || rows == 0) return 0;
  DMDX_CHECK_ARG(S && X, "unpack_i16: null pointer");
  DMDX_CHECK_ARG(((uintptr_t)X & 3u) == 0 && ((uintptr_t)S & 1u) == 0, "unpack_i16: S / X not aligned to their element");
  const dim3 grid((unsigned)((chunks_of<kChunk>(rows) + 255) / 256), grid_rows(T));
  hipLaunchKernelGGL(unpack_i16_kernel, grid, dim3(256), 0, (hipStream_t)stream, S, lds, T, tstep, rows, (uint32_t)row0,
                     (uint32_t)plane, segs, scale_factor, add_offset, nfill, fill0, fill1, X, ldx, fill_count);
  DMDX_LAUNCH_CHECK();
  return 0;
}
