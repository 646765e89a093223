// K12: full-field expansion Xhat = mu + sigma .* (U C) of the rank-k factors, and its score against the
// true snapshots without storing Xhat.  U: m x k (m huge, k <= 256), C: k x T, Xhat / X: m x T.
//
// The tile, the MFMA orientation, the k order, the sums and the T split are expand_tile.h's, which see; this file
// is their first user: the store of Xhat, and the score.
//
// Score.  e = X - Xhat per element; its square (q = 0: sse) and (X - mu)^2 (q = 1: ref) are the NQ = 2 quantities
// of expand_tile.h's sums, fp32 over the DMDX_EXPAND_FP32_ROWS = 128 rows of the workgroup; only sse has row sums.
#include "expand_tile.h"

namespace {

constexpr int TRS = 33;     // row stride of the per-wave transpose image
static_assert(RWG == DMDX_EXPAND_FP32_ROWS, "the header documents the fp32 row count");

// The second __launch_bounds__ argument is WAVES PER SIMD: 2 keeps the body within 256 registers per lane, i.e.
// at least two 4-wave workgroups per CU; small k needs far fewer registers and the compiler reports 3 - 5 waves
// per SIMD.  Above k = 192 both bodies sit at 234 - 256 VGPRs, right at that budget, and spill 20 - 32 bytes per
// lane at k > 224 (expand) / 48 - 76 at 192 < k <= 224 (score): the first knob to revisit.  The
// score body at k > 224 holds 84 KB of LDS, fits one workgroup per CU anyway and is given the whole file.
template <int KG, bool SCORE>
__global__ __launch_bounds__(256, (SCORE && KG >= 15) ? 1 : 2) void expand_kernel(
    const float* __restrict__ U, int64_t m, int k, int64_t ldu, const float* __restrict__ C, int64_t ldc,
    int64_t T, const float* __restrict__ mu, const float* __restrict__ sigma, float* __restrict__ Xhat,
    int64_t ldxh, const float* __restrict__ X, int64_t ldx, int64_t tiles_per_wg, int64_t ntiles, int cvec,
    float* __restrict__ colpart, double* __restrict__ rowpart, unsigned long long* clk) {
  __shared__ __attribute__((aligned(16))) float ctile[2][Geom<KG>::STAGE];
  __shared__ float tr[SCORE ? 4 * TT * TRS : 1];
  __shared__ float wgcol[SCORE ? 2 * 2 * 8 * TT : 1];   // [tile parity][sse, ref][wave, half][t]

  unsigned long long pc0 = 0, pr0 = 0;   // measurement aid (dmdx_set_clock_probe; null on the product path)
  if (clk != nullptr) {
    pc0 = __builtin_amdgcn_s_memtime();
    pr0 = __builtin_amdgcn_s_memrealtime();
  }

  const Lane L = lane_of(m);
  float ureg[8 * KG];
  load_panel<KG>(ureg, U, ldu, k, L);
  const float mu_i = (mu != nullptr && L.rowok) ? mu[L.row] : 0.f;
  const float sg_i = (sigma != nullptr && L.rowok) ? sigma[L.row] : 1.f;

  const int64_t tile0 = (int64_t)blockIdx.y * tiles_per_wg;
  const int64_t tile1 = tile0 + tiles_per_wg < ntiles ? tile0 + tiles_per_wg : ntiles;
  double rowacc[1] = {0.0};

  Stager<KG> cs;
  cs.load(C, ldc, 0, tile0 * TT, T, k, cvec, L.tid);
  cs.store(ctile[0], L.tid);
  __syncthreads();
  int cur = 0;
  for (int64_t tile = tile0; tile < tile1; ++tile) {
    const int64_t t0 = tile * TT;
    const bool has_next = tile + 1 < tile1;
    if (has_next) cs.load(C, ldc, 0, t0 + TT, T, k, cvec, L.tid);
    float xv[SCORE ? 16 : 1];
    if constexpr (SCORE) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t t = t0 + col_of(r, L.h);
        xv[r] = (L.rowok && t < T) ? X[t * ldx + L.row] : 0.f;
      }
    }

    const f32x16 acc = mfma_chain<KG>(ctile[cur], ureg, L);

    const int par = (int)((tile - tile0) & 1);
    if constexpr (!SCORE) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t t = t0 + col_of(r, L.h);
        const float v = affine(acc[r], sigma != nullptr, sg_i, mu != nullptr, mu_i);
        if (L.rowok && t < T) Xhat[t * ldxh + L.row] = v;
      }
    } else {
      float d2[16], g2[16];
      float rs = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const bool ok = L.rowok && t0 + col_of(r, L.h) < T;
        const float v = affine(acc[r], sigma != nullptr, sg_i, mu != nullptr, mu_i);
        const float e = xv[r] - v, g = xv[r] - mu_i;
        d2[r] = ok ? e * e : 0.f;
        g2[r] = ok ? g * g : 0.f;
        rs += d2[r];
      }
      rowacc[0] += (double)rs;
      float* trw = &tr[L.wave * TT * TRS];
      wave_col_sum<TRS>(trw, &wgcol[(par * 2 + 0) * 8 * TT], L, [&](int r) { return d2[r]; });
      wave_col_sum<TRS>(trw, &wgcol[(par * 2 + 1) * 8 * TT], L, [&](int r) { return g2[r]; });
    }

    if (has_next) cs.store(ctile[cur ^ 1], L.tid);
    __syncthreads();
    // (the slots of this parity are written again two tiles on, behind the next barrier)
    if constexpr (SCORE) flush_cols<2>(&wgcol[par * 2 * 8 * TT], colpart, t0, T, L.tid);
    cur ^= 1;
  }

  if constexpr (SCORE) {
    if (rowpart != nullptr) store_row_sums<1>(rowacc, rowpart, m, L);
  }
  if (clk != nullptr) {
    const unsigned long long pc1 = __builtin_amdgcn_s_memtime(), pr1 = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0) {
      atomicAdd(&clk[0], pc1 - pc0);
      atomicAdd(&clk[1], pr1 - pr0);
      atomicAdd(&clk[2], 1ull);
    }
  }
}

struct SseRef {
  double *sse, *ref;
  __device__ double* operator()(int q) const { return q == 0 ? sse : ref; }
};

template <bool SCORE>
int launch(const float* U, int64_t m, int k, int64_t ldu, const float* C, int64_t ldc, int64_t T, const float* mu,
           const float* sigma, float* Xhat, int64_t ldxh, const float* X, int64_t ldx, float* colpart, double* rowpart,
           hipStream_t st) {
  const Plan p = plan_for(m, T);
  const int cvec = cvec_of(C, ldc);
#define DMDX_LAUNCH(KG)                                                                                                \
  hipLaunchKernelGGL((expand_kernel<KG, SCORE>), p.grid(), dim3(256), 0, st, U, m, k, ldu, C, ldc, T, mu, sigma, Xhat, \
                     ldxh, X, ldx, p.tiles_per_wg, p.ntiles, cvec, colpart, rowpart, dmdx_clock_probe_ptr)
  DMDX_DISPATCH_KG(k, "expand", DMDX_LAUNCH)
#undef DMDX_LAUNCH
  DMDX_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int dmdx_expand_max_k(void) { return MAXK; }

extern "C" int dmdx_expand_f32(const float* U, int64_t m, int64_t k, int64_t ldu, const float* C, int64_t ldc, int64_t T,
                               const float* mu, const float* sigma, float* Xhat, int64_t ldxh, void* stream) {
  if (int rc = check_common(U, m, k, ldu, C, ldc, T, "dmdx_expand_f32")) return rc;
  DMDX_CHECK_ARG(Xhat != nullptr, "dmdx_expand_f32: Xhat must not be null");
  DMDX_CHECK_ARG(ldxh >= m && ldxh < DIM_LIMIT, "dmdx_expand_f32: ldxh = %lld must be in m .. 2^31 - 1", (long long)ldxh);
  return launch<false>(U, m, (int)k, ldu, C, ldc, T, mu, sigma, Xhat, ldxh, nullptr, 0, nullptr, nullptr,
                       (hipStream_t)stream);
}

extern "C" size_t dmdx_expand_score_workspace_bytes(int64_t m, int64_t k, int64_t T) {
  (void)k;
  if (m < 1 || T < 1) return 16;
  return score_ws_bytes(m, T, 2, 1);
}

extern "C" int dmdx_expand_score_f32(const float* U, int64_t m, int64_t k, int64_t ldu, const float* C, int64_t ldc,
                                     int64_t T, const float* mu, const float* sigma, const float* X, int64_t ldx,
                                     double* sse_col, double* ref_col, double* sse_row, int accumulate, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  if (int rc = check_common(U, m, k, ldu, C, ldc, T, "dmdx_expand_score_f32")) return rc;
  DMDX_CHECK_ARG(X != nullptr && sse_col != nullptr, "dmdx_expand_score_f32: X and sse_col must not be null");
  DMDX_CHECK_ARG(ldx >= 1 && ldx < DIM_LIMIT, "dmdx_expand_score_f32: ldx = %lld must be in 1 .. 2^31 - 1", (long long)ldx);
  if (int rc = check_workspace(workspace, workspace_bytes, dmdx_expand_score_workspace_bytes(m, k, T), "dmdx_expand_score_f32"))
    return rc;
  const Plan p = plan_for(m, T);
  hipStream_t st = (hipStream_t)stream;
  const ScoreWs ws = score_ws(workspace, p, m, 1);
  if (int rc = launch<true>(U, m, (int)k, ldu, C, ldc, T, mu, sigma, nullptr, 0, X, ldx, ws.colpart,
                            sse_row != nullptr ? ws.rowpart : nullptr, st))
    return rc;
  // sse and ref go to two vectors of the caller's; without ref_col its plane of the launch is left out
  return reduce_score<2, 1>(ws, p, m, T, ref_col != nullptr ? 2 : 1, SseRef{sse_col, ref_col}, accumulate, sse_row, 0, st);
}
