// The bf16 plane images K1's plane-fed pass streams (gemm_tn.hip, tn_unit_planes) and the pre-split kernel writes
// (plane_split.hip).  Free of HIP: tests/host/plane_image_main.cpp compiles it alone.
//
// A row block X_j (K_j x n fp32, column-major) is split ONCE per call into its three bf16 planes (bf16_split.h,
// split2_fast) and stored as images of 128 columns x 32 k x 3 planes x 2 bytes = 24 576 bytes:
//   * images are ordered panel-major, chunk-minor: image (panel pn, chunk c) of a block is image pn * chunks + c, so a
//     work unit walking K on one 128-column panel reads one contiguous stream;
//   * n is padded to a multiple of 128 columns and K to a multiple of 32 rows; all padding holds zero planes;
//   * an image is 1536 pieces of 16 bytes.  A piece holds, for one column, one plane, one 16-k group g (0, 1) and one
//     lane half h (0, 1), the bf16 of k = 16 g + 4 h + e (e = 0 .. 3) in its low 8 bytes and of k = 16 g + 8 + 4 h + e
//     in its high 8 bytes: the four dwords the in-kernel split packs for the lane (column, h) and group g, i.e. one
//     v_mfma_f32_32x32x16_bf16 operand;
//   * piece index inside the image: g * 768 + (plane * 4 + column / 32) * 64 + h * 32 + column % 32.  The 64 pieces one
//     ds_read_b128 wave-instruction fetches (lane & 31 -> column of a 32-column block, lane >> 5 -> h) are 1024
//     contiguous bytes in lane order: free of bank conflicts with no swizzle on either side, and a 16-k group of a panel
//     (a "half image", 12 288 bytes) is contiguous, so LDS-DMA copies it with a constant lane offset.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace plane_image {

constexpr int kCols = 128;                 // columns of a panel
constexpr int kRows = 32;                  // k per image (one chunk of K1)
constexpr int kPlanes = 3;                 // h, m, l
constexpr int kPieceBytes = 16;
constexpr int kHalfPieces = kCols * kPlanes * 2;                 // 768: one 16-k group of a panel
constexpr int kImagePieces = 2 * kHalfPieces;                    // 1536
constexpr int64_t kHalfBytes = (int64_t)kHalfPieces * kPieceBytes;    // 12 288
constexpr int64_t kImageBytes = (int64_t)kImagePieces * kPieceBytes;  // 24 576
static_assert(kImageBytes == (int64_t)kCols * kRows * kPlanes * 2, "an image is 128 columns x 32 k x 3 planes of bf16");

// piece of (column 0 .. 127, plane 0 .. 2, group 0 .. 1, half 0 .. 1) inside its image
#if defined(__HIPCC__)
__host__ __device__
#endif
inline int piece_index(int column, int plane, int g, int h) {
  return g * kHalfPieces + (plane * 4 + (column >> 5)) * 64 + h * 32 + (column & 31);
}

// the k (inside the image's 32) of bf16 element e (0 .. 7) of a piece of group g, half h
inline int piece_k(int g, int h, int e) { return 16 * g + 4 * h + (e & 3) + 8 * (e >> 2); }

// (no n + 127: sizes up to 2^63 - 1 must not wrap)
inline int64_t panels_of(int64_t n) { return n / kCols + (n % kCols != 0); }
inline int64_t chunks_of(int64_t K) { return K / kRows + (K % kRows != 0); }

// a + b, saturating to SIZE_MAX
inline size_t saturating_add(size_t a, size_t b) { return a > SIZE_MAX - b ? SIZE_MAX : a + b; }

// bytes of the images of one K x n block (K, n >= 0); saturates to SIZE_MAX
inline size_t block_bytes(int64_t K, int64_t n) {
  const unsigned __int128 b = (unsigned __int128)(uint64_t)panels_of(n) * (uint64_t)chunks_of(K) * (uint64_t)kImageBytes;
  return b > (unsigned __int128)SIZE_MAX ? SIZE_MAX : (size_t)b;
}

// bytes of the images of all blocks, block j at the sum of the blocks before it; 0 for a bad argument
inline size_t total_bytes(const int64_t* K, int nblocks, int64_t n) {
  if (!K || nblocks <= 0 || n <= 0) return 0;
  size_t sum = 0;
  for (int j = 0; j < nblocks; ++j) {
    if (K[j] < 1) return 0;
    sum = saturating_add(sum, block_bytes(K[j], n));
  }
  return sum;
}

// byte offset, from a block's first image, of the 16-k group `group` (0 .. 2 chunks - 1) of panel pn
inline int64_t group_offset(int64_t pn, int64_t chunks, int64_t group) { return (pn * chunks) * kImageBytes + group * kHalfBytes; }

// [a, a + na) and [b, b + nb) share no byte (differences: nothing wraps, whatever the pointers); empty ranges overlap nothing
inline bool disjoint(const void* a, size_t na, const void* b, size_t nb) {
  if (na == 0 || nb == 0) return true;
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return b0 >= a0 ? b0 - a0 >= na : a0 - b0 >= nb;
}

}  // namespace plane_image
