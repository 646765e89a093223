// K15: ensemble spread S = |sigma| .* sqrt(sum_b (U D_b)^2) of B member deviations in the rank-k coordinates, and
// its sums without storing S.  U: m x k (m huge, k <= 256), D: k x (B T), column b T + t = the scaled deviation
// d_b(t) = (c_b(t) - mean_b c_b(t)) / sqrt(B - ddof) of member b at snapshot t, S: m x T.
//
// Shape.  K12's (expand_tile.h, which see for the tile, the MFMA orientation and the k order), with a member loop
// inside: a workgroup (4 waves) owns 128 rows, every wave keeps ITS 32 x k panel of U in registers for its whole
// life, and the workgroup walks the T axis in tiles of 32 columns.  For every tile the B members follow each
// other: the 32 x k slice of D of a (tile, member) step goes
// through LDS, double buffered -- the next step's slice is loaded from global memory before the MFMAs of the
// current step and stored to the other stage behind them; one barrier per step.  A member field lives for one
// MFMA chain and one multiply-add: after the chain V[r] = fma(acc[r], acc[r], V[r]) for the 16 accumulator
// registers (one rounding per member, fixed order b = 0, 1, ...), after the last member the epilogue.
//
// MFMA orientation and k order are K12's, so that with B = 1 the chain result is K12's bit for bit:
// v_mfma_f32_32x32x2_f32 computes the TRANSPOSED tile P[t][i] = sum_j D[j][t] U[i][j] (A = D^T, B = U^T), the
// space index i on the lanes and t in the 16 registers (t = t0 + (r & 3) + 8 (r >> 2) + 4 h); step 4 q + e of
// lane half h contracts j = 8 q + 4 h + e; k is padded to a multiple of 16 with zeros on BOTH sides.  S, U and
// sigma have ONE path for every base and leading dimension, only the staging of D has a 16-byte fast path.
//
// Sums (dmdx_spread_score_f32).  w = sigma_i^2 V[i, t] per element, summed
//   over the 32 rows of a wave through a per-wave LDS transpose, over the 4 waves through 8 LDS slots in a fixed
//     order: fp32 over the DMDX_SPREAD_FP32_ROWS = 128 rows of the workgroup, written to the workgroup's own
//     slot colpart[row block][T]; a second kernel adds the row blocks in fp64;
//   over t per lane (16 values of a tile in fp32, tiles in fp64): rowpart[T split][m], added by a third kernel.
// No atomics anywhere: every sum has a fixed order that depends on (m, T, B) only.
#include "expand_tile.h"

namespace {

constexpr int TRS = 33;     // row stride of the per-wave transpose image
static_assert(RWG == DMDX_SPREAD_FP32_ROWS, "the header documents the fp32 row count");

// The second __launch_bounds__ argument is WAVES PER SIMD: 2 keeps the body within 256 registers per lane, i.e. at
// least two 4-wave workgroups per CU, one's epilogue under the other's MFMAs.  That holds without scratch up to
// k = 192 (k / 2 registers of U, the staging registers, 16 + 16 accumulators: 243 VGPRs at k = 192); above it K12's
// body already sits at the budget and this one holds 16 registers more (20 - 212 bytes of scratch per lane under a
// bound of 2), so those instantiations are given the whole unified file: up to 256 VGPRs + 16 - 39 AGPRs, no
// scratch, one workgroup per CU (what the compiler reports for each is in MEASUREMENTS.md, K15).
template <int KG, bool SCORE>
__global__ __launch_bounds__(256, KG > 12 ? 1 : 2) void spread_kernel(
    const float* __restrict__ U, int64_t m, int k, int64_t ldu, const float* __restrict__ D, int64_t ldd, int64_t T,
    int64_t B, const float* __restrict__ sigma, float* __restrict__ S, int64_t lds, int64_t tiles_per_wg,
    int64_t ntiles, int dvec, float* __restrict__ colpart, double* __restrict__ rowpart) {
  __shared__ __attribute__((aligned(16))) float dtile[2][Geom<KG>::STAGE];
  __shared__ float tr[SCORE ? 4 * TT * TRS : 1];
  __shared__ float wgcol[SCORE ? 2 * 8 * TT : 1];   // [tile parity][wave, half][t]

  const Lane L = lane_of(m);
  float ureg[8 * KG];
  load_panel<KG>(ureg, U, ldu, k, L);
  const float sg_i = (sigma != nullptr && L.rowok) ? sigma[L.row] : 1.f;

  const int64_t tile0 = (int64_t)blockIdx.y * tiles_per_wg;
  const int64_t tile1 = tile0 + tiles_per_wg < ntiles ? tile0 + tiles_per_wg : ntiles;
  double rowacc[1] = {0.0};

  float var[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) var[r] = 0.f;

  Stager<KG> ds;
  ds.load(D, ldd, 0, tile0 * TT, T, k, dvec, L.tid);
  ds.store(dtile[0], L.tid);
  __syncthreads();
  int cur = 0;
  for (int64_t tile = tile0; tile < tile1; ++tile) {
    const int64_t t0 = tile * TT;
    for (int64_t b = 0; b < B; ++b) {
      const bool last = b + 1 == B;
      const bool has_next = !last || tile + 1 < tile1;
      if (has_next) ds.load(D, ldd, last ? 0 : b + 1, last ? t0 + TT : t0, T, k, dvec, L.tid);

      const f32x16 acc = mfma_chain<KG>(dtile[cur], ureg, L);
#pragma unroll
      for (int r = 0; r < 16; ++r) var[r] = __builtin_fmaf(acc[r], acc[r], var[r]);

      if (last) {
        if constexpr (!SCORE) {
          const float asg = __builtin_fabsf(sg_i);
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int64_t t = t0 + col_of(r, L.h);
            float v = __builtin_sqrtf(var[r]);
            if (sigma != nullptr) v *= asg;
            if (L.rowok && t < T) S[t * lds + L.row] = v;
          }
        } else {
          const float s2 = sg_i * sg_i;
          float w[16];
          float rs = 0.f;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            float v = var[r];
            if (sigma != nullptr) v *= s2;
            w[r] = (L.rowok && t0 + col_of(r, L.h) < T) ? v : 0.f;
            rs += w[r];
          }
          rowacc[0] += (double)rs;
          wave_col_sum<TRS>(&tr[L.wave * TT * TRS], &wgcol[(int)((tile - tile0) & 1) * 8 * TT], L,
                            [&](int r) { return w[r]; });
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) var[r] = 0.f;
      }

      if (has_next) ds.store(dtile[cur ^ 1], L.tid);
      __syncthreads();
      // (the slots of this parity are written again two tiles on, behind the next barrier)
      if constexpr (SCORE) {
        if (last) flush_cols<1>(&wgcol[(int)((tile - tile0) & 1) * 8 * TT], colpart, t0, T, L.tid);
      }
      cur ^= 1;
    }
  }

  if constexpr (SCORE) {
    if (rowpart != nullptr) store_row_sums<1>(rowacc, rowpart, m, L);
  }
}

// the B members first (one message for m, T and B), then the factors as K12 checks them, then the B T columns of D
int check_spread(const float* U, int64_t m, int64_t k, int64_t ldu, const float* D, int64_t ldd, int64_t T, int64_t B,
                 const char* who) {
  DMDX_CHECK_ARG(U != nullptr && D != nullptr, "%s: U and D must not be null", who);
  DMDX_CHECK_ARG(m >= 1 && T >= 1 && B >= 1, "%s: m = %lld, T = %lld, B = %lld must be >= 1", who, (long long)m,
                 (long long)T, (long long)B);
  if (int rc = check_common(U, m, k, ldu, D, ldd, T, who, "D", "ldd")) return rc;
  DMDX_CHECK_ARG(B < DIM_LIMIT && B * T < DIM_LIMIT, "%s: B T = %lld x %lld columns of D must be < 2^31", who,
                 (long long)B, (long long)T);
  return 0;
}

template <bool SCORE>
int launch(const float* U, int64_t m, int k, int64_t ldu, const float* D, int64_t ldd, int64_t T, int64_t B,
           const float* sigma, float* S, int64_t lds, float* colpart, double* rowpart, hipStream_t st) {
  const Plan p = plan_for(m, T);
  const int dvec = cvec_of(D, ldd);
#define DMDX_LAUNCH(KG)                                                                                              \
  hipLaunchKernelGGL((spread_kernel<KG, SCORE>), p.grid(), dim3(256), 0, st, U, m, k, ldu, D, ldd, T, B, sigma, S, lds, \
                     p.tiles_per_wg, p.ntiles, dvec, colpart, rowpart)
  DMDX_DISPATCH_KG(k, "spread", DMDX_LAUNCH)
#undef DMDX_LAUNCH
  DMDX_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int dmdx_spread_max_k(void) { return MAXK; }

extern "C" int dmdx_spread_f32(const float* U, int64_t m, int64_t k, int64_t ldu, const float* D, int64_t ldd, int64_t T,
                               int64_t B, const float* sigma, float* S, int64_t lds, void* stream) {
  if (int rc = check_spread(U, m, k, ldu, D, ldd, T, B, "dmdx_spread_f32")) return rc;
  DMDX_CHECK_ARG(S != nullptr, "dmdx_spread_f32: S must not be null");
  DMDX_CHECK_ARG(lds >= m && lds < DIM_LIMIT, "dmdx_spread_f32: lds = %lld must be in m .. 2^31 - 1", (long long)lds);
  return launch<false>(U, m, (int)k, ldu, D, ldd, T, B, sigma, S, lds, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" size_t dmdx_spread_score_workspace_bytes(int64_t m, int64_t k, int64_t T, int64_t B) {
  (void)k;
  (void)B;
  if (m < 1 || T < 1) return 16;
  return score_ws_bytes(m, T, 1, 1);
}

extern "C" int dmdx_spread_score_f32(const float* U, int64_t m, int64_t k, int64_t ldu, const float* D, int64_t ldd,
                                     int64_t T, int64_t B, const float* sigma, double* var_col, double* var_row,
                                     int accumulate, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_spread(U, m, k, ldu, D, ldd, T, B, "dmdx_spread_score_f32")) return rc;
  DMDX_CHECK_ARG(var_col != nullptr, "dmdx_spread_score_f32: var_col must not be null");
  if (int rc = check_workspace(workspace, workspace_bytes, dmdx_spread_score_workspace_bytes(m, k, T, B), "dmdx_spread_score_f32"))
    return rc;
  const Plan p = plan_for(m, T);
  hipStream_t st = (hipStream_t)stream;
  const ScoreWs ws = score_ws(workspace, p, m, 1);
  if (int rc = launch<true>(U, m, (int)k, ldu, D, ldd, T, B, sigma, nullptr, 0, ws.colpart,
                            var_row != nullptr ? ws.rowpart : nullptr, st))
    return rc;
  return reduce_score<1, 1>(ws, p, m, T, 1, ColsOf{var_col, 0}, accumulate, var_row, 0, st);
}
