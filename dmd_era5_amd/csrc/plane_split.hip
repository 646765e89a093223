// K1p: the bf16 planes of a row block, made once per call (plane_image.h has the layout; gemm_tn.hip streams them).
//
// One workgroup = one 128-column panel x 128 rows of K (four chunks of 32): it reads every column in one run of
// 512 bytes (a wave-instruction covers two columns), parks the 64 KB in LDS with a column stride of 528 bytes, and
// then every thread takes (column, 16-k group, lane half), reads its two 16-byte k-pieces from LDS (the padded stride
// spreads the 16 lanes of a ds_read_b128 pass over all 64 banks), splits the eight values with bf16split::split2_fast
// and stores one 16-byte piece per plane.  A wave's 64 pieces of a plane are 1 KiB contiguous in the image, so the
// four whole images leave as 1 KiB runs.  Columns past n and rows past K read as zero: the padding of the images holds
// zero planes.  A pure stream: 4 bytes in, 6 out per value.
#include "bf16_split.h"
#include "dmdx_common.h"
#include "plane_image.h"

namespace {

constexpr int PS_TH = 256;
constexpr int PS_ROWS = 128;              // rows of K per workgroup: four chunks, a 512-byte run per column
constexpr int PS_STRIDE = PS_ROWS + 4;    // floats per column in LDS (528 bytes)
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(PS_TH) void plane_split_kernel(const float* __restrict__ X, int64_t K, int64_t n, int64_t ldx,
                                                            int64_t chunks, unsigned runs, unsigned char* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float tile[plane_image::kCols * PS_STRIDE];
  const int tid = threadIdx.x;
  // (one flat grid, the runs of a panel next to each other: neither count fits grid.y at the sizes the entry takes)
  const int64_t pn = blockIdx.x / runs, run = blockIdx.x % runs;
  const int64_t k0 = run * PS_ROWS;
  // ---- 128 columns x 32 float4, 16 per thread: a wave reads two columns x 512 bytes per instruction
#pragma unroll 4
  for (int i = 0; i < 16; ++i) {
    const int idx = i * PS_TH + tid;
    const int col = idx >> 5, k4 = idx & 31;
    const int64_t c = pn * plane_image::kCols + col, k = k0 + 4 * k4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (c < n) {
      const float* p = X + c * ldx + k;
      if (k + 4 <= K) {
        v = *reinterpret_cast<const f32x4*>(p);   // (16-byte aligned: the entry point takes aligned blocks only)
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (k + e < K) v[e] = p[e];
      }
    }
    *reinterpret_cast<f32x4*>(tile + col * PS_STRIDE + 4 * k4) = v;
  }
  __syncthreads();
  // ---- thread -> (column block = wave, lane = h * 32 + column % 32), iteration -> 16-k group G of the 128 rows
  const int lane = tid & 63, cblk = tid >> 6;
  const int col = 32 * cblk + (lane & 31), h = lane >> 5;
#pragma unroll 2
  for (int G = 0; G < 8; ++G) {
    const int64_t chunk = run * 4 + (G >> 1);
    if (chunk >= chunks) break;
    const float* src = tile + col * PS_STRIDE + 16 * G + 4 * h;
    const f32x4 e = *reinterpret_cast<const f32x4*>(src), o = *reinterpret_cast<const f32x4*>(src + 8);
    uint32_t H[4], M[4], L[4];
    bf16split::split2_fast(e[0], e[1], H[0], M[0], L[0]);
    bf16split::split2_fast(e[2], e[3], H[1], M[1], L[1]);
    bf16split::split2_fast(o[0], o[1], H[2], M[2], L[2]);
    bf16split::split2_fast(o[2], o[3], H[3], M[3], L[3]);
    u32x4_t* img = reinterpret_cast<u32x4_t*>(out + (pn * chunks + chunk) * plane_image::kImageBytes);
    img[plane_image::piece_index(col, 0, G & 1, h)] = u32x4_t{H[0], H[1], H[2], H[3]};
    img[plane_image::piece_index(col, 1, G & 1, h)] = u32x4_t{M[0], M[1], M[2], M[3]};
    img[plane_image::piece_index(col, 2, G & 1, h)] = u32x4_t{L[0], L[1], L[2], L[3]};
  }
}

}  // namespace

// The images of one aligned K x n block (X 16-byte aligned, ldx % 4 == 0) into `out` (plane_image::block_bytes).
// Checks nothing: dmdx_syrk_blocks_planes_f32 has, before its first launch (dmdx_plane_split_fits among them).
bool dmdx_plane_split_fits(int64_t K, int64_t n) {
  return (plane_image::chunks_of(K) + 3) / 4 * plane_image::panels_of(n) < (int64_t(1) << 31);
}

int dmdx_plane_split_launch(const float* X, int64_t K, int64_t n, int64_t ldx, void* out, hipStream_t st) {
  const int64_t chunks = plane_image::chunks_of(K), panels = plane_image::panels_of(n);
  const unsigned runs = (unsigned)((chunks + 3) / 4);
  hipLaunchKernelGGL(plane_split_kernel, dim3((unsigned)(runs * panels)), dim3(PS_TH), 0, st, X, K, n, ldx, chunks, runs,
                     (unsigned char*)out);
  DMDX_LAUNCH_CHECK();
  return 0;
}
