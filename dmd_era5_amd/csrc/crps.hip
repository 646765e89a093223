// K19: the sums behind the continuous ranked probability score and the rank histogram of B member fields
// x_b = mu + sigma .* (U C_b) against the analysis X, no member field stored.  U: m x k, C: k x (B T), column
// b T + t = the coefficients of member b at snapshot t, X: m x T.  Per element, fp32:
//   abs = sum_b |x_b - y|     pair = sum_{b < b'} |x_b - x_b'|     rank = #{b : x_b < y}      y = X[i, t]
// One more body on K12's shape (expand_tile.h, which see for the tile, the MFMA orientation and the k order), with
// a member loop like K15's and an analysis operand like K16's: a workgroup (4 waves) owns 128 rows, every wave keeps
// its 32 x k panel of U in registers, the 32 x k slice of C of a (tile, member) step goes through LDS, double
// buffered, one barrier per step; X is read once per tile.  A member field is K12's chain and K12's affine(): bit for
// bit what dmdx_expand_f32 gives for C_b.
//
// The pair term.  All B members of an element are needed at once and fit neither the register file nor LDS, so the
// members are HELD in blocks of HB (16 accumulator registers each) and the chains are REPEATED: for the block that
// starts at member jb the steps run over b = jb, jb + 1, ..., B - 1.  The first HB of them are the block's own
// members: each adds its |x_b - y| to abs, its (x_b < y) to rank, its distances to the members of the block held so
// far to pair, and is then held.  Every later member lives for one chain and adds its distance to the HB held ones.
// HB = 16 (256 registers) up to k = 128, where the panel of U leaves room for them in the 512-entry file, and 8 (128
// registers) above: B + B^2 / (2 HB) chains per tile, roughly, where K15 runs B (B = 100: 364 / 676); the
// B (B - 1) / 2 distances (a subtract and an add with |.| each) are inherent.  Every pair (b, b') with b < b' is
// formed exactly once, in the order (block of b, b', b): a function of B and HB, i.e. of (B, k), only.  One loop body
// serves both kinds of step: the held block is indexed by unrolled, wave-uniform comparisons with b - jb.
//
// Rounding.  x_b - y and x_b - x_b' are rounded once each, and every quantity is ONE fp32 chain per element: abs over
// B terms (b = 0, 1, ...), pair over B (B - 1) / 2 terms -- the header states it, and the bound of the tests
// uses it.  All terms are >= 0.  Identical members give |x - x| = +0.0 and pair = +0.0 exactly.  A non-finite abs
// (a non-finite y, or a non-finite member) is passed on to pair as pair + (abs - abs): + 0.0 where abs is finite, NaN
// where it is not, so that an element poisons both quantities or none.  Contraction is off: the contract counts
// roundings.
//
// Sums of the two quantities: K16's, twice -- over the 32 rows of a wave through the per-wave LDS transpose, over the
// 4 waves through 8 LDS slots in a fixed order, fp32 over the DMDX_CRPS_FP32_ROWS = 128 rows of the workgroup into
// colpart[row block][2][T], fp64 over the row blocks in a second kernel; over t per lane (16 values in fp32, tiles in
// fp64) into rowpart[T split][2][m], added by a third kernel.  No floating-point atomics.
//
// Rank counts.  After the last member of a tile every selected, finite element adds 1 to bin `rank` of the
// workgroup's LDS histogram (B + 1 <= 257 uint32 bins, integer LDS atomics: an integer sum has no order).  Behind the
// tile's barrier thread j moves bins j and j + 256 into its own int64 registers and zeroes them, so an LDS bin never
// holds more than the 128 x 32 = 4096 elements of one tile and the running counts are 64 bits wide: no overflow for
// any T.  At its end the workgroup writes its counts to its slot histpart[row block, T split][B + 1] (int64) of the
// workspace, and a fourth kernel adds the slots.
//
// Registers.  k / 2 of U, 16 HB held, 16 each of X, abs, pair, rank and the accumulator, k / 32 x 4 of staging: more
// than 256 from k = 1 on, so every instantiation is given the unified 512-entry file (__launch_bounds__(256, 1)), one
// workgroup per CU, as K15 / K16 do from KG = 13; none has scratch (what the compiler reports is in MEASUREMENTS.md,
// K19).
#include "expand_tile.h"

#pragma clang fp contract(off)

namespace {

constexpr int NQ = DMDX_CRPS_NQ;
// members held in registers: 16 where U leaves room for them in the 512-entry file (k <= 128), 8 above
template <int KG>
constexpr int hb_of() { return KG <= 8 ? DMDX_CRPS_MEMBER_BLOCK_SMALL_K : DMDX_CRPS_MEMBER_BLOCK; }
constexpr int MAXB = DMDX_CRPS_MAX_B;
constexpr int NBIN = MAXB + 1;
constexpr int TRS = 33;                        // row stride of the per-wave transpose image
static_assert(RWG == DMDX_CRPS_FP32_ROWS, "the header documents the fp32 row count");
static_assert(NQ == 2, "abs and pair");
static_assert(hb_of<8>() == 16 && hb_of<9>() == 8, "the header documents the member blocks and the k at which they change");
static_assert(NBIN <= 2 * 256, "thread j owns bins j and j + 256");

template <int KG>
__global__ __launch_bounds__(256, 1) void crps_kernel(
    const float* __restrict__ U, int64_t m, int k, int64_t ldu, const float* __restrict__ C, int64_t ldc, int64_t T,
    int B, const float* __restrict__ mu, const float* __restrict__ sigma, const float* __restrict__ X, int64_t ldx,
    const float* __restrict__ w, int64_t tiles_per_wg, int64_t ntiles, int cvec, float* __restrict__ colpart,
    double* __restrict__ rowpart, long long* __restrict__ histpart) {
  __shared__ __attribute__((aligned(16))) float ctile[2][Geom<KG>::STAGE];
  __shared__ float tr[4 * TT * TRS];
  __shared__ float wgcol[NQ * 8 * TT];         // [quantity][wave, half][t]
  __shared__ unsigned lhist[2 * 256];

  constexpr int HB = hb_of<KG>();
  const Lane L = lane_of(m);
  float ureg[8 * KG];
  load_panel<KG>(ureg, U, ldu, k, L);
  const float mu_i = (mu != nullptr && L.rowok) ? mu[L.row] : 0.f;
  const float sg_i = (sigma != nullptr && L.rowok) ? sigma[L.row] : 1.f;
  const float w_i = (w != nullptr && L.rowok) ? w[L.row] : 1.f;
  const bool sel = L.rowok && w_i != 0.f;      // the row takes part in the column sums and the counts

  const int64_t tile0 = (int64_t)blockIdx.y * tiles_per_wg;
  const int64_t tile1 = tile0 + tiles_per_wg < ntiles ? tile0 + tiles_per_wg : ntiles;
  double rowacc[NQ] = {0.0, 0.0};
  long long histacc[2] = {0, 0};
  lhist[L.tid] = 0u;
  lhist[L.tid + 256] = 0u;

  Stager<KG> cs;
  cs.load(C, ldc, 0, tile0 * TT, T, k, cvec, L.tid);
  cs.store(ctile[0], L.tid);
  __syncthreads();
  int cur = 0;
  for (int64_t tile = tile0; tile < tile1; ++tile) {
    const int64_t t0 = tile * TT;
    float xv[16], absq[16], pairq[16];
    int rank[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t t = t0 + col_of(r, L.h);
      xv[r] = (L.rowok && t < T) ? X[t * ldx + L.row] : 0.f;
      absq[r] = 0.f;
      pairq[r] = 0.f;
      rank[r] = 0;
    }

    for (int jb = 0; jb < B; jb += HB) {
      float held[HB][16];
#pragma unroll
      for (int g = 0; g < HB; ++g)
#pragma unroll
        for (int r = 0; r < 16; ++r) held[g][r] = 0.f;

      for (int b = jb; b < B; ++b) {
        // the step after this one: the next member of this block's run, the first member of the next block, or
        // member 0 of the next tile
        const bool more = b + 1 < B, more_blocks = jb + HB < B;
        const bool has_next = more || more_blocks || tile + 1 < tile1;
        if (has_next)
          cs.load(C, ldc, more ? b + 1 : (more_blocks ? jb + HB : 0), (more || more_blocks) ? t0 : t0 + TT, T, k, cvec,
                  L.tid);

        const f32x16 acc = mfma_chain<KG>(ctile[cur], ureg, L);
        float x[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) x[r] = affine(acc[r], sigma != nullptr, sg_i, mu != nullptr, mu_i);

        const int hb = b - jb;               // wave-uniform
        if (hb < HB) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            absq[r] += __builtin_fabsf(x[r] - xv[r]);
            rank[r] += x[r] < xv[r] ? 1 : 0;
          }
        }
#pragma unroll
        for (int g = 0; g < HB; ++g) {
          if (g < hb) {
#pragma unroll
            for (int r = 0; r < 16; ++r) pairq[r] += __builtin_fabsf(x[r] - held[g][r]);
          }
        }
#pragma unroll
        for (int g = 0; g < HB; ++g) {
          if (g == hb) {
#pragma unroll
            for (int r = 0; r < 16; ++r) held[g][r] = x[r];
          }
        }

        if (has_next) cs.store(ctile[cur ^ 1], L.tid);
        __syncthreads();
        cur ^= 1;
      }
    }

    // the tile's two quantities and its counts; wgcol and lhist were read last behind the previous tile's second
    // barrier, and at least one step's barrier lies between
    float* trw = &tr[L.wave * TT * TRS];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      float rs = 0.f;
      wave_col_sum<TRS>(trw, &wgcol[q * 8 * TT], L, [&](int r) {
        const bool ok = L.rowok && t0 + col_of(r, L.h) < T;
        const float val = q == 0 ? absq[r] : pairq[r] + (absq[r] - absq[r]);
        rs += ok ? val : 0.f;
        return (ok && sel) ? (w != nullptr ? w_i * val : val) : 0.f;
      });
      rowacc[q] += (double)rs;
    }
    if (histpart != nullptr) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const bool ok = sel && t0 + col_of(r, L.h) < T;
        // finite: abs - abs is 0 for a finite abs and NaN for Inf and NaN; rank is in 0 .. B <= 256
        if (ok && absq[r] - absq[r] == 0.f) atomicAdd(&lhist[rank[r]], 1u);
      }
    }
    __syncthreads();
    flush_cols<NQ>(wgcol, colpart, t0, T, L.tid);
    if (histpart != nullptr) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int bin = L.tid + 256 * s;
        if (bin <= B) {
          histacc[s] += (long long)lhist[bin];
          lhist[bin] = 0u;
        }
      }
    }
  }

  if (rowpart != nullptr) store_row_sums<NQ>(rowacc, rowpart, m, L);
  if (histpart != nullptr) {
    long long* slot = histpart + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (int64_t)(B + 1);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int bin = L.tid + 256 * s;
      if (bin <= B) slot[bin] = histacc[s];
    }
  }
}

// [score workspace of 2 quantities, both with row sums][histpart: row blocks x T splits x (B + 1) int64]; the score
// part is a multiple of 8 bytes past its 16-byte boundary (colpart holds 2 floats per (row block, t))
inline size_t hist_offset(int64_t m, int64_t T) { return score_ws_bytes(m, T, NQ, NQ); }

}  // namespace

extern "C" int dmdx_crps_max_k(void) { return MAXK; }
extern "C" int dmdx_crps_max_members(void) { return MAXB; }

extern "C" size_t dmdx_crps_workspace_bytes(int64_t m, int64_t k, int64_t T, int64_t B) {
  (void)k;
  if (m < 1 || T < 1 || m >= DIM_LIMIT || T >= DIM_LIMIT || B < 1 || B > MAXB) return 16;
  const Plan p = plan_for(m, T);
  return hist_offset(m, T) + (size_t)p.nrb * (size_t)p.nsplit * (size_t)(B + 1) * sizeof(long long);
}

extern "C" int dmdx_crps_f32(const float* U, int64_t m, int64_t k, int64_t ldu, const float* C, int64_t ldc, int64_t T,
                             int64_t B, const float* mu, const float* sigma, const float* X, int64_t ldx, const float* w,
                             double* col, int64_t ldcol, double* row, int64_t ldrow, int64_t* hist, int accumulate,
                             void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "dmdx_crps_f32";
  DMDX_CHECK_ARG(U != nullptr && C != nullptr && X != nullptr && col != nullptr, "%s: U, C, X and col must not be null", who);
  DMDX_CHECK_ARG(B >= 1 && B <= MAXB, "%s: B = %lld outside 1 .. %d", who, (long long)B, MAXB);
  if (int rc = check_common(U, m, k, ldu, C, ldc, T, who)) return rc;
  DMDX_CHECK_ARG(B * T < DIM_LIMIT, "%s: B T = %lld x %lld columns of C must be < 2^31", who, (long long)B, (long long)T);
  if (int rc = check_score_lds(m, T, ldx, ldcol, row, ldrow, who)) return rc;
  if (int rc = check_workspace(workspace, workspace_bytes, dmdx_crps_workspace_bytes(m, k, T, B), who)) return rc;
  const Plan p = plan_for(m, T);
  hipStream_t st = (hipStream_t)stream;
  const ScoreWs ws = score_ws(workspace, p, m, NQ);
  char* base = reinterpret_cast<char*>(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
  long long* histpart = hist != nullptr ? reinterpret_cast<long long*>(base + hist_offset(m, T) - 16) : nullptr;
  const int cvec = cvec_of(C, ldc);
  double* rowpart = row != nullptr ? ws.rowpart : nullptr;
#define DMDX_LAUNCH(KG)                                                                                                 \
  hipLaunchKernelGGL((crps_kernel<KG>), p.grid(), dim3(256), 0, st, U, m, (int)k, ldu, C, ldc, T, (int)B, mu, sigma, X, ldx, \
                     w, p.tiles_per_wg, p.ntiles, cvec, ws.colpart, rowpart, histpart)
  DMDX_DISPATCH_KG(k, who, DMDX_LAUNCH)
#undef DMDX_LAUNCH
  DMDX_LAUNCH_CHECK();
  if (int rc = reduce_score<NQ, NQ>(ws, p, m, T, NQ, ColsOf{col, ldcol}, accumulate, row, ldrow, st)) return rc;
  if (hist != nullptr) {
    hipLaunchKernelGGL(reduce_hist_kernel, dim3((unsigned)(B + 1)), dim3(256), 0, st, histpart, p.nrb * p.nsplit, (int)(B + 1),
                       reinterpret_cast<long long*>(hist), accumulate);
    DMDX_LAUNCH_CHECK();
  }
  return 0;
}
