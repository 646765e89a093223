// K12: full-field expansion Xhat = mu + sigma .* (U C) of the rank-k factors, and its score against the
// true snapshots without storing Xhat.  U: m x k (m huge, k <= 256), C: k x T, Xhat / X: m x T.
//
// Shape.  The opposite of K2: a short contraction and a huge output.  A workgroup (4 waves) owns 128
// rows; every wave keeps ITS 32 x k panel of U in registers for its whole life (k / 2 registers per
// lane, zero beyond k and beyond m), and the workgroup walks the T axis in tiles of 32 columns.  The
// 32 x k slice of C of a tile (small, L2 resident, shared by the four waves) goes through LDS, double
// buffered: the next tile's slice is loaded from global memory before the MFMAs of the current tile and
// stored to the other stage behind them; one barrier per tile.  At least two workgroups per CU: one's epilogue
// (HBM stores, or loads of X) runs under the other's MFMAs.
//
// MFMA orientation.  v_mfma_f32_32x32x2_f32 computes the TRANSPOSED tile D[t][i] = sum_j C[j][t] U[i][j]:
// A = C^T (lane (t, h) holds C[j][t0 + t]), B = U^T (lane (i, h) holds U[row0 + i][j]).  The result then
// has the space index i on the lanes and t in the 16 registers, so register r of the wave is two runs of
// 32 consecutive floats of Xhat (t = t0 + (r & 3) + 8 (r >> 2) + 4 h): two 128-byte segments per store,
// with no alignment requirement at all -- Xhat, X, U, mu and sigma have ONE path for every base and
// leading dimension.  Only the staging of C has a 16-byte fast path.
//
// k order.  The contraction order of an MFMA chain is free as long as A and B agree: step 4 q + e of
// lane half h contracts j = 8 q + 4 h + e, so a lane reads its four A values of a group q with one
// 16-byte LDS read ([t][k] image, row stride 16 KG + 4 floats).  One fp32 chain over all of k (padded to
// a multiple of 16 with zeros on BOTH sides: 0 * 0, never a clamped duplicate), then sigma * acc + mu.
//
// Score.  e = X - Xhat per element; its square and (X - mu)^2 are summed
//   over the 32 rows of a wave through a per-wave LDS transpose (16 writes, 16 reads per lane and tile:
//     the sum runs over the lane index, which no MFMA contracts), over the 4 waves through 8 LDS slots
//     in a fixed order: fp32 over the DMDX_EXPAND_FP32_ROWS = 128 rows of the workgroup, written to
//     the workgroup's own slot colpart[row block][2][T]; a second kernel adds the row blocks in fp64;
//   over t per lane (16 values of a tile in fp32, tiles in fp64): rowpart[T split][m], added by a
//     third kernel.
// No atomics anywhere: every sum has a fixed order that depends on the shapes only.
#include "dmdx_common.h"

namespace {

constexpr int RWG = 128;    // rows per workgroup (4 waves x 32)
constexpr int TT = 32;      // columns of a tile
constexpr int MAXK = 256;
constexpr int TRS = 33;     // row stride of the per-wave transpose image
static_assert(RWG == DMDX_EXPAND_FP32_ROWS, "the header documents the fp32 row count");

// The second __launch_bounds__ argument is WAVES PER SIMD: 2 keeps the body within 256 registers per lane, i.e.
// at least two 4-wave workgroups per CU; small k needs far fewer registers and the compiler reports 3 - 5 waves
// per SIMD.  Above k = 128 (expand) / k = 64 (score) the body sits at 246 - 256 VGPRs, right at that budget, and
// spills 32 - 96 bytes per lane at k > 224 (expand) / 192 < k <= 224 (score): the first knob to revisit.  The
// score body at k > 224 holds 84 KB of LDS, fits one workgroup per CU anyway and is given the whole file.
template <int KG, bool SCORE>
__global__ __launch_bounds__(256, (SCORE && KG >= 15) ? 1 : 2) void expand_kernel(
    const float* __restrict__ U, int64_t m, int k, int64_t ldu, const float* __restrict__ C, int64_t ldc,
    int64_t T, const float* __restrict__ mu, const float* __restrict__ sigma, float* __restrict__ Xhat,
    int64_t ldxh, const float* __restrict__ X, int64_t ldx, int64_t tiles_per_wg, int64_t ntiles, int cvec,
    float* __restrict__ colpart, double* __restrict__ rowpart, unsigned long long* clk) {
  constexpr int KP = 16 * KG;        // padded k
  constexpr int KS = KP + 4;         // LDS row stride of the [t][k] image
  constexpr int PPT = KP / 4;        // 16-byte pieces per column of C
  constexpr int NPIECE = TT * PPT;
  constexpr int NPT = (NPIECE + 255) / 256;
  __shared__ __attribute__((aligned(16))) float ctile[2][TT * KS];
  __shared__ float tr[SCORE ? 4 * TT * TRS : 1];
  __shared__ float wgcol[SCORE ? 2 * 2 * 8 * TT : 1];   // [tile parity][sse, ref][wave, half][t]

  unsigned long long pc0 = 0, pr0 = 0;   // measurement aid (dmdx_set_clock_probe; null on the product path)
  if (clk != nullptr) {
    pc0 = __builtin_amdgcn_s_memtime();
    pr0 = __builtin_amdgcn_s_memrealtime();
  }

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, h = lane >> 5;
  const int64_t row = (int64_t)blockIdx.x * RWG + wave * 32 + li;
  const bool rowok = row < m;

  // the wave's U panel: register 4 q + e = U[row][8 q + 4 h + e]; exact zeros past k and past m
  float ureg[8 * KG];
#pragma unroll
  for (int s = 0; s < 8 * KG; ++s) {
    const int j = 8 * (s >> 2) + 4 * h + (s & 3);
    ureg[s] = (rowok && j < k) ? U[(int64_t)j * ldu + row] : 0.f;
  }
  const float mu_i = (mu != nullptr && rowok) ? mu[row] : 0.f;
  const float sg_i = (sigma != nullptr && rowok) ? sigma[row] : 1.f;

  f32x4 creg[NPT];
  auto load_c = [&](int64_t t0) {
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
      const int idx = tid + 256 * i;
      if (NPIECE % 256 != 0 && idx >= NPIECE) continue;
      const int tl = idx / PPT, j = 4 * (idx % PPT);
      const int64_t t = t0 + tl;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (t < T && j < k) {
        const float* q = C + t * ldc + j;
        if (cvec && j + 4 <= k) {
          v = *reinterpret_cast<const f32x4*>(q);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (j + e < k) v[e] = q[e];
        }
      }
      creg[i] = v;
    }
  };
  auto store_c = [&](int st) {
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
      const int idx = tid + 256 * i;
      if (NPIECE % 256 != 0 && idx >= NPIECE) continue;
      *reinterpret_cast<f32x4*>(&ctile[st][(idx / PPT) * KS + 4 * (idx % PPT)]) = creg[i];
    }
  };

  const int64_t tile0 = (int64_t)blockIdx.y * tiles_per_wg;
  const int64_t tile1 = tile0 + tiles_per_wg < ntiles ? tile0 + tiles_per_wg : ntiles;
  double rowacc = 0.0;

  // sums the 8 (wave, half) slots of a finished tile in a fixed order into the workgroup's partial slot
  auto flush_cols = [&](int par, int64_t t0) {
    if constexpr (SCORE) {
      if (tid < 64) {
        const int q = tid >> 5, tl = tid & 31;
        const float* w = &wgcol[(par * 2 + q) * 8 * TT + tl];
        float s = w[0];
#pragma unroll
        for (int v = 1; v < 8; ++v) s += w[v * TT];
        if (t0 + tl < T) colpart[((int64_t)blockIdx.x * 2 + q) * T + t0 + tl] = s;
      }
    }
  };

  load_c(tile0 * TT);
  store_c(0);
  __syncthreads();
  int cur = 0;
  for (int64_t tile = tile0; tile < tile1; ++tile) {
    const int64_t t0 = tile * TT;
    const bool has_next = tile + 1 < tile1;
    if (has_next) load_c(t0 + TT);
    float xv[SCORE ? 16 : 1];
    if constexpr (SCORE) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t t = t0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        xv[r] = (rowok && t < T) ? X[t * ldx + row] : 0.f;
      }
    }

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float* ct = &ctile[cur][li * KS + 4 * h];
#pragma unroll
    for (int q = 0; q < 2 * KG; ++q) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(ct + 8 * q);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], ureg[4 * q + e], acc, 0, 0, 0);
    }

    if constexpr (!SCORE) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t t = t0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        float v = acc[r];
        if (sigma != nullptr) v *= sg_i;
        if (mu != nullptr) v += mu_i;
        if (rowok && t < T) Xhat[t * ldxh + row] = v;
      }
    } else {
      float d2[16], g2[16];
      float rs = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t t = t0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        const bool ok = rowok && t < T;
        float v = acc[r];
        if (sigma != nullptr) v *= sg_i;
        if (mu != nullptr) v += mu_i;
        const float e = xv[r] - v, g = xv[r] - mu_i;
        d2[r] = ok ? e * e : 0.f;
        g2[r] = ok ? g * g : 0.f;
        rs += d2[r];
      }
      rowacc += (double)rs;
      // sums over the wave's 32 rows: [t][i] image of the wave, lane (t = li, h) adds rows 16 h .. 16 h + 15
      // (LDS operations of one wave execute in order: no barrier between its writes and its reads)
      float* trw = &tr[wave * TT * TRS];
      const int par = (int)((tile - tile0) & 1);
#pragma unroll
      for (int q = 0; q < 2; ++q) {
#pragma unroll
        for (int r = 0; r < 16; ++r) trw[((r & 3) + 8 * (r >> 2) + 4 * h) * TRS + li] = q == 0 ? d2[r] : g2[r];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        float s = trw[li * TRS + 16 * h];
#pragma unroll
        for (int j = 1; j < 16; ++j) s += trw[li * TRS + 16 * h + j];
        wgcol[((par * 2 + q) * 8 + 2 * wave + h) * TT + li] = s;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
      }
    }

    if (has_next) store_c(cur ^ 1);
    __syncthreads();
    // (the slots of this parity are written again two tiles on, behind the next barrier)
    flush_cols((int)((tile - tile0) & 1), t0);
    cur ^= 1;
  }

  if constexpr (SCORE) {
    if (rowpart != nullptr) {
      const double other = __shfl_xor(rowacc, 32, 64);
      if (h == 0 && rowok) rowpart[(int64_t)blockIdx.y * m + row] = rowacc + other;
    }
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

// out[t] (+)= sum over the row blocks of colpart[rb][q][t] in fp64: 32 columns x 8 slot lanes per workgroup, every
// thread adds its row blocks sl, sl + 8, ..., the 8 lanes meet in LDS in a fixed order
__global__ __launch_bounds__(256) void expand_reduce_cols_kernel(const float* __restrict__ colpart, int64_t nrb, int64_t T,
                                                                 double* __restrict__ sse_col, double* __restrict__ ref_col,
                                                                 int accumulate) {
  __shared__ double part[8][32];
  const int q = blockIdx.y;
  double* out = q == 0 ? sse_col : ref_col;
  if (out == nullptr) return;
  const int j = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int64_t t = (int64_t)blockIdx.x * 32 + j;
  double s = 0.0;
  if (t < T)
    for (int64_t rb = sl; rb < nrb; rb += 8) s += (double)colpart[(rb * 2 + q) * T + t];
  part[sl][j] = s;
  __syncthreads();
  if (sl != 0 || t >= T) return;
#pragma unroll
  for (int v = 1; v < 8; ++v) s += part[v][j];
  out[t] = accumulate ? out[t] + s : s;
}

__global__ __launch_bounds__(256) void expand_reduce_rows_kernel(const double* __restrict__ rowpart, int64_t nsplit, int64_t m,
                                                                 double* __restrict__ sse_row) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  double s = rowpart[i];
  for (int64_t y = 1; y < nsplit; ++y) s += rowpart[y * m + i];
  sse_row[i] = s;
}

// the T axis is split over blockIdx.y until the launch has ~2048 workgroups (8 per CU); a function of the
// shapes only, so that the partial sums -- and with them the results -- do not depend on the device
struct Plan {
  int64_t nrb, ntiles, tiles_per_wg, nsplit;
};
Plan plan_for(int64_t m, int64_t T) {
  Plan p;
  p.nrb = (m + RWG - 1) / RWG;
  p.ntiles = (T + TT - 1) / TT;
  int64_t want = (2048 + p.nrb - 1) / p.nrb;
  if (want > p.ntiles) want = p.ntiles;
  if (want < 1) want = 1;
  p.tiles_per_wg = (p.ntiles + want - 1) / want;
  p.nsplit = (p.ntiles + p.tiles_per_wg - 1) / p.tiles_per_wg;
  return p;
}

constexpr int64_t DIM_LIMIT = int64_t(1) << 31;

int check_common(const float* U, int64_t m, int64_t k, int64_t ldu, const float* C, int64_t ldc, int64_t T, const char* who) {
  DMDX_CHECK_ARG(U != nullptr && C != nullptr, "%s: U and C must not be null", who);
  DMDX_CHECK_ARG(m >= 1 && T >= 1, "%s: m = %lld, T = %lld must be >= 1", who, (long long)m, (long long)T);
  DMDX_CHECK_ARG(k >= 1 && k <= MAXK, "%s: k = %lld outside 1 .. %d", who, (long long)k, MAXK);
  DMDX_CHECK_ARG(ldu >= m && ldc >= k, "%s: ldu = %lld < m = %lld or ldc = %lld < k = %lld", who, (long long)ldu,
                 (long long)m, (long long)ldc, (long long)k);
  DMDX_CHECK_ARG(m < DIM_LIMIT && T < DIM_LIMIT && ldu < DIM_LIMIT && ldc < DIM_LIMIT,
                 "%s: m, T, ldu, ldc must be < 2^31", who);
  return 0;
}

template <bool SCORE>
int launch(const float* U, int64_t m, int k, int64_t ldu, const float* C, int64_t ldc, int64_t T, const float* mu,
           const float* sigma, float* Xhat, int64_t ldxh, const float* X, int64_t ldx, float* colpart, double* rowpart,
           hipStream_t st) {
  const Plan p = plan_for(m, T);
  const int cvec = dmdx_aligned16(C) && ldc % 4 == 0;
  const dim3 grid((unsigned)p.nrb, (unsigned)p.nsplit);
  switch ((k + 15) / 16) {
#define DMDX_CASE(KG)                                                                                              \
  case KG:                                                                                                         \
    hipLaunchKernelGGL((expand_kernel<KG, SCORE>), grid, dim3(256), 0, st, U, m, k, ldu, C, ldc, T, mu, sigma, Xhat, \
                       ldxh, X, ldx, p.tiles_per_wg, p.ntiles, cvec, colpart, rowpart, dmdx_clock_probe_ptr);       \
    break
    DMDX_CASE(1); DMDX_CASE(2); DMDX_CASE(3); DMDX_CASE(4); DMDX_CASE(5); DMDX_CASE(6); DMDX_CASE(7); DMDX_CASE(8);
    DMDX_CASE(9); DMDX_CASE(10); DMDX_CASE(11); DMDX_CASE(12); DMDX_CASE(13); DMDX_CASE(14); DMDX_CASE(15);
    DMDX_CASE(16);
#undef DMDX_CASE
    default:
      dmdx_set_error("expand: unsupported k %d", k);
      return DMDX_E_INVALID;
  }
  DMDX_LAUNCH_CHECK();
  return 0;
}

inline size_t align16(size_t n) { return (n + 15) & ~size_t(15); }

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

// [<= 15 bytes to a 16-byte boundary][rowpart: nsplit x m fp64][colpart: row blocks x 2 x T fp32]
extern "C" size_t dmdx_expand_score_workspace_bytes(int64_t m, int64_t k, int64_t T) {
  (void)k;
  if (m < 1 || T < 1) return 16;
  const Plan p = plan_for(m, T);
  return 16 + align16((size_t)p.nsplit * (size_t)m * sizeof(double)) + (size_t)p.nrb * 2 * (size_t)T * sizeof(float);
}

extern "C" int dmdx_expand_score_f32(const float* U, int64_t m, int64_t k, int64_t ldu, const float* C, int64_t ldc,
                                     int64_t T, const float* mu, const float* sigma, const float* X, int64_t ldx,
                                     double* sse_col, double* ref_col, double* sse_row, int accumulate, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  if (int rc = check_common(U, m, k, ldu, C, ldc, T, "dmdx_expand_score_f32")) return rc;
  DMDX_CHECK_ARG(X != nullptr && sse_col != nullptr, "dmdx_expand_score_f32: X and sse_col must not be null");
  DMDX_CHECK_ARG(ldx >= 1 && ldx < DIM_LIMIT, "dmdx_expand_score_f32: ldx = %lld must be in 1 .. 2^31 - 1", (long long)ldx);
  const size_t need = dmdx_expand_score_workspace_bytes(m, k, T);
  if (workspace == nullptr || workspace_bytes < need) {
    dmdx_set_error("dmdx_expand_score_f32: workspace of %zu bytes, %zu needed", workspace == nullptr ? (size_t)0 : workspace_bytes,
                   need);
    return DMDX_E_WORKSPACE;
  }
  const Plan p = plan_for(m, T);
  hipStream_t st = (hipStream_t)stream;
  char* base = reinterpret_cast<char*>(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
  double* rowpart = reinterpret_cast<double*>(base);
  float* colpart = reinterpret_cast<float*>(base + align16((size_t)p.nsplit * (size_t)m * sizeof(double)));
  if (int rc = launch<true>(U, m, (int)k, ldu, C, ldc, T, mu, sigma, nullptr, 0, X, ldx, colpart,
                            sse_row != nullptr ? rowpart : nullptr, st))
    return rc;
  hipLaunchKernelGGL(expand_reduce_cols_kernel, dim3((unsigned)p.ntiles, 2), dim3(256), 0, st, colpart, p.nrb, T, sse_col,
                     ref_col, accumulate);
  DMDX_LAUNCH_CHECK();
  if (sse_row != nullptr) {
    hipLaunchKernelGGL(expand_reduce_rows_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, rowpart, p.nsplit, m,
                       sse_row);
    DMDX_LAUNCH_CHECK();
  }
  return 0;
}
