// csrc/plane_image.h alone, with the host compiler (tests/test_host_plane_image.py builds it under
// -fsanitize=undefined,address): the image index, the slot formula against a literal transcription of the in-kernel
// split's packing (gemm_tn.hip, DMDX_SPLIT_GROUP), and the byte counts by hand.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../dmd_era5_amd/csrc/bf16_split.h"
#include "../../dmd_era5_amd/csrc/plane_image.h"

static int failed = 0;
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      ++failed;                     \
      printf("FAILED: " __VA_ARGS__); \
      printf("\n");                 \
    }                               \
  } while (0)

// the image of one 32-row x 128-column tile x[k][c] as the layout's own words say it: piece_index, piece_k
static std::vector<uint16_t> image_by_formula(const float (*x)[128]) {
  std::vector<uint16_t> img(plane_image::kImagePieces * 8, 0xDEAD);
  for (int c = 0; c < 128; ++c)
    for (int g = 0; g < 2; ++g)
      for (int h = 0; h < 2; ++h)
        for (int e = 0; e < 8; ++e) {
          uint32_t hh, mm, ll;
          bf16split::split1(x[plane_image::piece_k(g, h, e)][c], hh, mm, ll);
          const uint32_t pl[3] = {hh, mm, ll};
          for (int p = 0; p < 3; ++p) img[(size_t)plane_image::piece_index(c, p, g, h) * 8 + e] = (uint16_t)(pl[p] >> 16);
        }
  return img;
}

// DMDX_SPLIT_GROUP, transcribed: lane (column, h) holds for group g the 16-byte piece e_ of k-step 2g (k = 16 g + 4 h
// + 0 .. 3) and o_ of k-step 2g + 1 (k = 16 g + 8 + 4 h + 0 .. 3); q_ = 0, 1 pack the pairs of e_, q_ = 2, 3 those of
// o_; the MFMA operand of a plane is the four dwords P[0 .. 3]
static void split_group(const float (*x)[128], int c, int g, int h, uint32_t PH[4], uint32_t PM[4], uint32_t PL[4]) {
  float e_[4], o_[4];
  for (int i = 0; i < 4; ++i) {
    e_[i] = x[16 * g + 4 * h + i][c];
    o_[i] = x[16 * g + 8 + 4 * h + i][c];
  }
  for (int q_ = 0; q_ < 4; ++q_) {
    const float x0 = q_ < 2 ? e_[2 * (q_ & 1)] : o_[2 * (q_ & 1)];
    const float x1 = q_ < 2 ? e_[2 * (q_ & 1) + 1] : o_[2 * (q_ & 1) + 1];
    bf16split::split2_fast(x0, x1, PH[q_], PM[q_], PL[q_]);
  }
}

int main() {
  using namespace plane_image;
  // ---- the index is a bijection onto [0, 24 576 / 16)
  {
    std::vector<int> hit(kImagePieces, 0);
    for (int c = 0; c < kCols; ++c)
      for (int p = 0; p < kPlanes; ++p)
        for (int g = 0; g < 2; ++g)
          for (int h = 0; h < 2; ++h) {
            const int i = piece_index(c, p, g, h);
            CHECK(i >= 0 && i < kImagePieces, "piece_index(%d, %d, %d, %d) = %d outside the image", c, p, g, h, i);
            if (i >= 0 && i < kImagePieces) ++hit[i];
          }
    int once = 0;
    for (int i = 0; i < kImagePieces; ++i) once += hit[i] == 1;
    CHECK(once == kImagePieces && kImagePieces == 24576 / 16, "%d of %d pieces hit exactly once", once, kImagePieces);
    // the 64 lanes of one operand read (lane & 31 -> column of the block, lane >> 5 -> h) are 64 consecutive pieces
    for (int p = 0; p < kPlanes; ++p)
      for (int g = 0; g < 2; ++g)
        for (int blk = 0; blk < 4; ++blk)
          for (int lane = 0; lane < 64; ++lane)
            CHECK(piece_index(32 * blk + (lane & 31), p, g, lane >> 5) == piece_index(32 * blk, p, g, 0) + lane,
                  "operand read of plane %d, group %d, block %d is not in lane order at lane %d", p, g, blk, lane);
    // a 16-k group of the panel is one contiguous half image
    CHECK(piece_index(0, 0, 1, 0) == kHalfPieces && kHalfBytes == 12288 && kImageBytes == 24576, "half image");
  }
  // ---- every k of the image sits in exactly one (g, h, e)
  {
    int seen[32] = {0};
    for (int g = 0; g < 2; ++g)
      for (int h = 0; h < 2; ++h)
        for (int e = 0; e < 8; ++e) ++seen[piece_k(g, h, e)];
    for (int k = 0; k < 32; ++k) CHECK(seen[k] == 1, "k = %d is in %d slots", k, seen[k]);
  }
  // ---- the slot formula against the in-kernel packing
  {
    static float x[32][128];
    uint32_t s = 12345u;
    for (int k = 0; k < 32; ++k)
      for (int c = 0; c < 128; ++c) {
        s = s * 1664525u + 1013904223u;
        x[k][c] = (float)((int32_t)s) * (1.0f / 65536.0f) * (1.0f + (float)(c % 7));
      }
    x[3][5] = -0.0f;
    x[17][100] = 0.0f;
    x[31][127] = 1.0f;
    const std::vector<uint16_t> img = image_by_formula(x);
    int bad = 0;
    for (int c = 0; c < 128; ++c)
      for (int g = 0; g < 2; ++g)
        for (int h = 0; h < 2; ++h) {
          uint32_t P[3][4];
          split_group(x, c, g, h, P[0], P[1], P[2]);
          for (int p = 0; p < 3; ++p) bad += memcmp(&img[(size_t)piece_index(c, p, g, h) * 8], P[p], 16) != 0;
        }
    CHECK(bad == 0, "%d of 1536 pieces differ from the dwords DMDX_SPLIT_GROUP packs", bad);
  }
  // ---- byte counts by hand
  {
    struct { int64_t K, n; size_t want; } cases[] = {
        {31, 100, (size_t)1 * 1 * 24576},
        {32, 128, (size_t)1 * 1 * 24576},
        {20481, 312, (size_t)3 * 641 * 24576},
        {129780, 8760, (size_t)69 * 4056 * 24576},
    };
    for (const auto& c : cases) {
      CHECK(block_bytes(c.K, c.n) == c.want, "block_bytes(%lld, %lld) = %zu, by hand %zu", (long long)c.K, (long long)c.n,
            block_bytes(c.K, c.n), c.want);
      CHECK(total_bytes(&c.K, 1, c.n) == c.want, "total_bytes of one block (%lld, %lld)", (long long)c.K, (long long)c.n);
    }
    const int64_t cfg2[8] = {129780, 129780, 129780, 129780, 129780, 129780, 129780, 129780};
    CHECK(total_bytes(cfg2, 8, 8760) == (size_t)8 * 69 * 4056 * 24576, "the eight cfg2 blocks");
    CHECK((size_t)8 * 69 * 4056 * 24576 == 55023501312ull, "cfg2 by hand: 55 023 501 312 bytes");
    const int64_t three[3] = {20481, 4097, 31};
    CHECK(total_bytes(three, 3, 312) == (size_t)3 * (641 + 129 + 1) * 24576, "three blocks");
    CHECK(total_bytes(nullptr, 1, 8) == 0 && total_bytes(three, 0, 8) == 0 && total_bytes(three, 3, 0) == 0, "bad arguments give 0");
    const int64_t zero[2] = {5, 0};
    CHECK(total_bytes(zero, 2, 8) == 0, "an empty block gives 0");
    CHECK(group_offset(2, 641, 0) == (int64_t)2 * 641 * 24576 && group_offset(0, 641, 3) == 3 * 12288, "group_offset");
  }
  // ---- saturation near 2^63
  {
    const int64_t big = INT64_MAX;
    CHECK(block_bytes(big, big) == SIZE_MAX, "block_bytes(2^63 - 1, 2^63 - 1) saturates");
    CHECK(block_bytes(big, 128) == SIZE_MAX, "block_bytes(2^63 - 1, 128) saturates");
    CHECK(block_bytes((int64_t)1 << 40, (int64_t)1 << 30) == SIZE_MAX, "2^35 chunks x 2^23 panels x 24 576 saturates");
    const int64_t K = ((int64_t)1 << 40);
    const size_t one = block_bytes(K, 128 * 1000);   // 2^35 chunks x 1000 panels x 24 576 = 8.4e17: fits
    CHECK(one == (size_t)1000 * ((size_t)1 << 35) * 24576, "a large block that fits");
    const int64_t many[32] = {K, K, K, K, K, K, K, K, K, K, K, K, K, K, K, K, K, K, K, K, K, K, K, K, K, K, K, K, K, K, K, K};
    CHECK(total_bytes(many, 32, 128 * 1000) == SIZE_MAX, "the sum of 32 such blocks saturates");
    CHECK(total_bytes(many, 16, 128 * 1000) == 16 * one, "the sum of 16 fits");
    CHECK(saturating_add(SIZE_MAX - 1, 1) == SIZE_MAX && saturating_add(SIZE_MAX - 1, 2) == SIZE_MAX && saturating_add(1, 2) == 3,
          "saturating_add");
  }
  // ---- disjoint ranges
  {
    char buf[64];
    CHECK(disjoint(buf, 16, buf + 16, 16) && disjoint(buf + 16, 16, buf, 16), "adjacent ranges are disjoint");
    CHECK(!disjoint(buf, 17, buf + 16, 16) && !disjoint(buf + 16, 16, buf, 17), "one shared byte");
    CHECK(!disjoint(buf, 64, buf + 8, 8) && !disjoint(buf + 8, 8, buf, 64), "containment");
    CHECK(disjoint(buf, 0, buf, 64) && disjoint(buf, 64, buf + 3, 0), "an empty range overlaps nothing");
  }
  printf("plane_image: %d failed\n", failed);
  return failed ? 1 : 0;
}
