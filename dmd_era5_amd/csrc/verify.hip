// K16: area-weighted verification of Xhat = mu + sigma .* (U C) against the analysis X and a climatology,
// Xhat never stored.  One more body on K12's shape (expand_tile.h, which see for the tile, the MFMA orientation
// and the k order): a workgroup (4 waves) owns 128 rows, every wave keeps its 32 x k panel of U in registers,
// the 32 x k slice of C of a tile goes through LDS, double buffered, X is read once.  Instead of K12's two
// column sums it accumulates the six weighted sums every grid score is a ratio of:
//   e = xhat - x, f = xhat - clim, a = x - clim (each rounded to fp32)
//   q = 0: w e^2   1: w e   2: w a   3: w f^2   4: w a^2   5: w f a
// per column over the rows with w != 0 (a SELECT: 0 * NaN is never formed, a masked row may hold anything),
// and the same six sums per row over t, unweighted.
//
// Sums.  K12's, six times: over the 32 rows of a wave through the per-wave LDS transpose, over the 4 waves
// through 8 LDS slots in a fixed order -- fp32 over the DMDX_VERIFY_FP32_ROWS = 128 rows of the workgroup,
// written to the workgroup's slot colpart[row block][6][T]; a second kernel adds the row blocks in fp64.
// Over t per lane: 16 values of a tile in fp32, tiles in fp64, rowpart[T split][6][m], added by a third
// kernel.  The quantities go through the transpose one after the other, each formed from xhat and x in
// registers when its turn comes: no quantity costs registers, and q = 0 and q = 4 run through exactly the
// instructions of K12's sse and ref, so that without w and clim they ARE sse_col, ref_col and sse_row, bit for
// bit (e = xhat - x is K12's x - xhat negated, its square the same).  No atomics anywhere.
//
// Rounding.  The contract counts roundings (q rounded, then w * q rounded), so contraction is switched off for the
// file; K12's sigma * acc + mu is two operations by its own definition (expand_tile.h, affine).
#include "expand_tile.h"

#pragma clang fp contract(off)

namespace {

constexpr int NQ = DMDX_VERIFY_NQ;
static_assert(RWG == DMDX_VERIFY_FP32_ROWS, "the header documents the fp32 row count");
static_assert(NQ == 6, "the six sums of the header");

// The second __launch_bounds__ argument is WAVES PER SIMD: 2 keeps the body within 256 registers per lane, i.e. two
// 4-wave workgroups per CU (their LDS, 34 - 79 KB each, fits twice up to k = 192).  The body wants ~190 registers
// at k <= 16 already (e, f and a of a tile's 16 columns live across the six passes, the addresses of the 16 loads of
// X, six fp64 row sums) and spills 40 - 256 bytes per lane at 96 < k <= 192: the first knob to revisit.  From
// k = 193 on a workgroup holds > 80 KB of LDS, is alone on its CU anyway and is given the whole register file, as
// K12's score body is.
template <int KG>
__global__ __launch_bounds__(256, KG >= 13 ? 1 : 2) void verify_kernel(
    const float* __restrict__ U, int64_t m, int k, int64_t ldu, const float* __restrict__ C, int64_t ldc, int64_t T,
    const float* __restrict__ mu, const float* __restrict__ sigma, const float* __restrict__ X, int64_t ldx,
    const float* __restrict__ w, const float* __restrict__ clim, int64_t tiles_per_wg, int64_t ntiles, int cvec,
    float* __restrict__ colpart, double* __restrict__ rowpart) {
  __shared__ __attribute__((aligned(16))) float ctile[2][Geom<KG>::STAGE];
  // Row stride of the per-wave transpose image.  36: rows on 16-byte boundaries, a lane's 16 values are four
  // 16-byte LDS reads instead of sixteen 4-byte ones (the order of the sum is the same: the identity with K12
  // holds) -- 7 - 10 % faster where it was measured (k = 10, 50, 200) and 13 - 20 registers more, which the
  // instantiations that are at the register budget with scratch (64 < k <= 192) would pay for with more of it:
  // they keep K12's 33.
  constexpr int TRS = (KG <= 4 || KG >= 13) ? 36 : 33;
  __shared__ __attribute__((aligned(16))) float tr[4 * TT * TRS];
  __shared__ float wgcol[2 * NQ * 8 * TT];   // [tile parity][quantity][wave, half][t]

  const Lane L = lane_of(m);
  float ureg[8 * KG];
  load_panel<KG>(ureg, U, ldu, k, L);
  const float mu_i = (mu != nullptr && L.rowok) ? mu[L.row] : 0.f;
  const float sg_i = (sigma != nullptr && L.rowok) ? sigma[L.row] : 1.f;
  const float cl_i = clim != nullptr ? (L.rowok ? clim[L.row] : 0.f) : mu_i;
  const float w_i = (w != nullptr && L.rowok) ? w[L.row] : 1.f;
  const bool sel = L.rowok && w_i != 0.f;      // the row takes part in the column sums

  const int64_t tile0 = (int64_t)blockIdx.y * tiles_per_wg;
  const int64_t tile1 = tile0 + tiles_per_wg < ntiles ? tile0 + tiles_per_wg : ntiles;
  double rowacc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) rowacc[q] = 0.0;

  Stager<KG> cs;
  cs.load(C, ldc, 0, tile0 * TT, T, k, cvec, L.tid);
  cs.store(ctile[0], L.tid);
  __syncthreads();
  int cur = 0;
  for (int64_t tile = tile0; tile < tile1; ++tile) {
    const int64_t t0 = tile * TT;
    const bool has_next = tile + 1 < tile1;
    if (has_next) cs.load(C, ldc, 0, t0 + TT, T, k, cvec, L.tid);
    float xv[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t t = t0 + col_of(r, L.h);
      xv[r] = (L.rowok && t < T) ? X[t * ldx + L.row] : 0.f;
    }

    const f32x16 acc = mfma_chain<KG>(ctile[cur], ureg, L);
    float xh[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) xh[r] = affine(acc[r], sigma != nullptr, sg_i, mu != nullptr, mu_i);

    float* trw = &tr[L.wave * TT * TRS];
    const int par = (int)((tile - tile0) & 1);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      float rs = 0.f;
      wave_col_sum<TRS>(trw, &wgcol[(par * NQ + q) * 8 * TT], L, [&](int r) {
        const bool ok = L.rowok && t0 + col_of(r, L.h) < T;
        const float e = xh[r] - xv[r], f = xh[r] - cl_i, a = xv[r] - cl_i;
        const float val = q == 0 ? e * e : q == 1 ? e : q == 2 ? a : q == 3 ? f * f : q == 4 ? a * a : f * a;
        rs += ok ? val : 0.f;
        return (ok && sel) ? (w != nullptr ? w_i * val : val) : 0.f;
      });
      rowacc[q] += (double)rs;
      __builtin_amdgcn_sched_barrier(0);   // one quantity at a time: the next one's 16 terms are not formed early
    }

    if (has_next) cs.store(ctile[cur ^ 1], L.tid);
    __syncthreads();
    // (the slots of this parity are written again two tiles on, behind the next barrier)
    flush_cols<NQ>(&wgcol[par * NQ * 8 * TT], colpart, t0, T, L.tid);
    cur ^= 1;
  }

  if (rowpart != nullptr) store_row_sums<NQ>(rowacc, rowpart, m, L);
}

}  // namespace

extern "C" int dmdx_verify_max_k(void) { return MAXK; }

extern "C" size_t dmdx_verify_workspace_bytes(int64_t m, int64_t k, int64_t T) {
  (void)k;
  if (m < 1 || T < 1 || m >= DIM_LIMIT || T >= DIM_LIMIT) return 16;
  return score_ws_bytes(m, T, NQ, NQ);
}

extern "C" int dmdx_verify_f32(const float* U, int64_t m, int64_t k, int64_t ldu, const float* C, int64_t ldc, int64_t T,
                               const float* mu, const float* sigma, const float* X, int64_t ldx, const float* w,
                               const float* clim, double* col, int64_t ldcol, double* row, int64_t ldrow, int accumulate,
                               void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "dmdx_verify_f32";
  DMDX_CHECK_ARG(U != nullptr && C != nullptr && X != nullptr && col != nullptr, "%s: U, C, X and col must not be null", who);
  if (int rc = check_common(U, m, k, ldu, C, ldc, T, who)) return rc;
  if (int rc = check_score_lds(m, T, ldx, ldcol, row, ldrow, who)) return rc;
  if (int rc = check_workspace(workspace, workspace_bytes, dmdx_verify_workspace_bytes(m, k, T), who)) return rc;
  const Plan p = plan_for(m, T);
  hipStream_t st = (hipStream_t)stream;
  const ScoreWs ws = score_ws(workspace, p, m, NQ);
  const int cvec = cvec_of(C, ldc);
  double* rowpart = row != nullptr ? ws.rowpart : nullptr;
#define DMDX_LAUNCH(KG)                                                                                                  \
  hipLaunchKernelGGL((verify_kernel<KG>), p.grid(), dim3(256), 0, st, U, m, (int)k, ldu, C, ldc, T, mu, sigma, X, ldx, w, \
                     clim, p.tiles_per_wg, p.ntiles, cvec, ws.colpart, rowpart)
  DMDX_DISPATCH_KG(k, who, DMDX_LAUNCH)
#undef DMDX_LAUNCH
  DMDX_LAUNCH_CHECK();
  return reduce_score<NQ, NQ>(ws, p, m, T, NQ, ColsOf{col, ldcol}, accumulate, row, ldrow, st);
}
