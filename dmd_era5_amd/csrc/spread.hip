// K15: ensemble spread S = |sigma| .* sqrt(sum_b (U D_b)^2) of B member deviations in the rank-k coordinates, and
// its sums without storing S.  U: m x k (m huge, k <= 256), D: k x (B T), column b T + t = the scaled deviation
// d_b(t) = (c_b(t) - mean_b c_b(t)) / sqrt(B - ddof) of member b at snapshot t, S: m x T.
//
// Shape.  K12's (expand.hip), with a member loop inside: a workgroup (4 waves) owns 128 rows, every wave keeps
// ITS 32 x k panel of U in registers for its whole life, and the workgroup walks the T axis in tiles of 32
// columns.  For every tile the B members follow each other: the 32 x k slice of D of a (tile, member) step goes
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
#include "dmdx_common.h"

namespace {

constexpr int RWG = 128;    // rows per workgroup (4 waves x 32)
constexpr int TT = 32;      // columns of a tile
constexpr int MAXK = 256;
constexpr int TRS = 33;     // row stride of the per-wave transpose image
static_assert(RWG == DMDX_SPREAD_FP32_ROWS, "the header documents the fp32 row count");

// The second __launch_bounds__ argument is WAVES PER SIMD: 2 keeps the body within 256 registers per lane, i.e. at
// least two 4-wave workgroups per CU, one's epilogue under the other's MFMAs.  That holds without scratch up to
// k = 192 (k / 2 registers of U, the staging registers, 16 + 16 accumulators: 249 VGPRs at k = 192); above it K12's
// body already sits at the budget and this one holds 16 registers more (20 - 212 bytes of scratch per lane under a
// bound of 2), so those instantiations are given the whole unified file: 256 VGPRs + 16 - 48 AGPRs, no scratch, one
// workgroup per CU (what the compiler reports for each is in MEASUREMENTS.md, K15).
template <int KG, bool SCORE>
__global__ __launch_bounds__(256, KG > 12 ? 1 : 2) void spread_kernel(
    const float* __restrict__ U, int64_t m, int k, int64_t ldu, const float* __restrict__ D, int64_t ldd, int64_t T,
    int64_t B, const float* __restrict__ sigma, float* __restrict__ S, int64_t lds, int64_t tiles_per_wg,
    int64_t ntiles, int dvec, float* __restrict__ colpart, double* __restrict__ rowpart) {
  constexpr int KP = 16 * KG;        // padded k
  constexpr int KS = KP + 4;         // LDS row stride of the [t][k] image
  constexpr int PPT = KP / 4;        // 16-byte pieces per column of D
  constexpr int NPIECE = TT * PPT;
  constexpr int NPT = (NPIECE + 255) / 256;
  __shared__ __attribute__((aligned(16))) float dtile[2][TT * KS];
  __shared__ float tr[SCORE ? 4 * TT * TRS : 1];
  __shared__ float wgcol[SCORE ? 2 * 8 * TT : 1];   // [tile parity][wave, half][t]

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
  const float sg_i = (sigma != nullptr && rowok) ? sigma[row] : 1.f;

  f32x4 dreg[NPT];
  auto load_d = [&](int64_t t0, int64_t b) {
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
      const int idx = tid + 256 * i;
      if (NPIECE % 256 != 0 && idx >= NPIECE) continue;
      const int tl = idx / PPT, j = 4 * (idx % PPT);
      const int64_t t = t0 + tl;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (t < T && j < k) {
        const float* q = D + (b * T + t) * ldd + j;
        if (dvec && j + 4 <= k) {
          v = *reinterpret_cast<const f32x4*>(q);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (j + e < k) v[e] = q[e];
        }
      }
      dreg[i] = v;
    }
  };
  auto store_d = [&](int st) {
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
      const int idx = tid + 256 * i;
      if (NPIECE % 256 != 0 && idx >= NPIECE) continue;
      *reinterpret_cast<f32x4*>(&dtile[st][(idx / PPT) * KS + 4 * (idx % PPT)]) = dreg[i];
    }
  };

  const int64_t tile0 = (int64_t)blockIdx.y * tiles_per_wg;
  const int64_t tile1 = tile0 + tiles_per_wg < ntiles ? tile0 + tiles_per_wg : ntiles;
  double rowacc = 0.0;

  // sums the 8 (wave, half) slots of a finished tile in a fixed order into the workgroup's partial slot
  auto flush_cols = [&](int par, int64_t t0) {
    if constexpr (SCORE) {
      if (tid < TT) {
        const float* w = &wgcol[par * 8 * TT + tid];
        float s = w[0];
#pragma unroll
        for (int v = 1; v < 8; ++v) s += w[v * TT];
        if (t0 + tid < T) colpart[(int64_t)blockIdx.x * T + t0 + tid] = s;
      }
    }
  };

  float var[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) var[r] = 0.f;

  load_d(tile0 * TT, 0);
  store_d(0);
  __syncthreads();
  int cur = 0;
  for (int64_t tile = tile0; tile < tile1; ++tile) {
    const int64_t t0 = tile * TT;
    for (int64_t b = 0; b < B; ++b) {
      const bool last = b + 1 == B;
      const bool has_next = !last || tile + 1 < tile1;
      if (has_next) load_d(last ? t0 + TT : t0, last ? 0 : b + 1);

      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      const float* dt = &dtile[cur][li * KS + 4 * h];
#pragma unroll
      for (int q = 0; q < 2 * KG; ++q) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(dt + 8 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], ureg[4 * q + e], acc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) var[r] = __builtin_fmaf(acc[r], acc[r], var[r]);

      if (last) {
        if constexpr (!SCORE) {
          const float asg = __builtin_fabsf(sg_i);
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int64_t t = t0 + (r & 3) + 8 * (r >> 2) + 4 * h;
            float v = __builtin_sqrtf(var[r]);
            if (sigma != nullptr) v *= asg;
            if (rowok && t < T) S[t * lds + row] = v;
          }
        } else {
          const float s2 = sg_i * sg_i;
          float w[16];
          float rs = 0.f;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int64_t t = t0 + (r & 3) + 8 * (r >> 2) + 4 * h;
            float v = var[r];
            if (sigma != nullptr) v *= s2;
            w[r] = (rowok && t < T) ? v : 0.f;
            rs += w[r];
          }
          rowacc += (double)rs;
          // sums over the wave's 32 rows: [t][i] image of the wave, lane (t = li, h) adds rows 16 h .. 16 h + 15
          // (LDS operations of one wave execute in order: no barrier between its writes and its reads)
          float* trw = &tr[wave * TT * TRS];
          const int par = (int)((tile - tile0) & 1);
#pragma unroll
          for (int r = 0; r < 16; ++r) trw[((r & 3) + 8 * (r >> 2) + 4 * h) * TRS + li] = w[r];
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          float s = trw[li * TRS + 16 * h];
#pragma unroll
          for (int j = 1; j < 16; ++j) s += trw[li * TRS + 16 * h + j];
          wgcol[(par * 8 + 2 * wave + h) * TT + li] = s;
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) var[r] = 0.f;
      }

      if (has_next) store_d(cur ^ 1);
      __syncthreads();
      // (the slots of this parity are written again two tiles on, behind the next barrier)
      if (last) flush_cols((int)((tile - tile0) & 1), t0);
      cur ^= 1;
    }
  }

  if constexpr (SCORE) {
    if (rowpart != nullptr) {
      const double other = __shfl_xor(rowacc, 32, 64);
      if (h == 0 && rowok) rowpart[(int64_t)blockIdx.y * m + row] = rowacc + other;
    }
  }
}

// var_col[t] (+)= sum over the row blocks of colpart[rb][t] in fp64: 32 columns x 8 slot lanes per workgroup, every
// thread adds its row blocks sl, sl + 8, ..., the 8 lanes meet in LDS in a fixed order
__global__ __launch_bounds__(256) void spread_reduce_cols_kernel(const float* __restrict__ colpart, int64_t nrb, int64_t T,
                                                                 double* __restrict__ var_col, int accumulate) {
  __shared__ double part[8][32];
  const int j = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int64_t t = (int64_t)blockIdx.x * 32 + j;
  double s = 0.0;
  if (t < T)
    for (int64_t rb = sl; rb < nrb; rb += 8) s += (double)colpart[rb * T + t];
  part[sl][j] = s;
  __syncthreads();
  if (sl != 0 || t >= T) return;
#pragma unroll
  for (int v = 1; v < 8; ++v) s += part[v][j];
  var_col[t] = accumulate ? var_col[t] + s : s;
}

__global__ __launch_bounds__(256) void spread_reduce_rows_kernel(const double* __restrict__ rowpart, int64_t nsplit, int64_t m,
                                                                 double* __restrict__ var_row) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  double s = rowpart[i];
  for (int64_t y = 1; y < nsplit; ++y) s += rowpart[y * m + i];
  var_row[i] = s;
}

// the T axis is split over blockIdx.y until the launch has ~2048 workgroups (8 per CU), as K12 does; a function of
// the shapes only, so that the partial sums -- and with them the results -- do not depend on the device
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

int check_common(const float* U, int64_t m, int64_t k, int64_t ldu, const float* D, int64_t ldd, int64_t T, int64_t B,
                 const char* who) {
  DMDX_CHECK_ARG(U != nullptr && D != nullptr, "%s: U and D must not be null", who);
  DMDX_CHECK_ARG(m >= 1 && T >= 1 && B >= 1, "%s: m = %lld, T = %lld, B = %lld must be >= 1", who, (long long)m,
                 (long long)T, (long long)B);
  DMDX_CHECK_ARG(k >= 1 && k <= MAXK, "%s: k = %lld outside 1 .. %d", who, (long long)k, MAXK);
  DMDX_CHECK_ARG(ldu >= m && ldd >= k, "%s: ldu = %lld < m = %lld or ldd = %lld < k = %lld", who, (long long)ldu,
                 (long long)m, (long long)ldd, (long long)k);
  DMDX_CHECK_ARG(m < DIM_LIMIT && T < DIM_LIMIT && ldu < DIM_LIMIT && ldd < DIM_LIMIT,
                 "%s: m, T, ldu, ldd must be < 2^31", who);
  DMDX_CHECK_ARG(B < DIM_LIMIT && B * T < DIM_LIMIT, "%s: B T = %lld x %lld columns of D must be < 2^31", who,
                 (long long)B, (long long)T);
  return 0;
}

template <bool SCORE>
int launch(const float* U, int64_t m, int k, int64_t ldu, const float* D, int64_t ldd, int64_t T, int64_t B,
           const float* sigma, float* S, int64_t lds, float* colpart, double* rowpart, hipStream_t st) {
  const Plan p = plan_for(m, T);
  const int dvec = dmdx_aligned16(D) && ldd % 4 == 0;
  const dim3 grid((unsigned)p.nrb, (unsigned)p.nsplit);
  switch ((k + 15) / 16) {
#define DMDX_CASE(KG)                                                                                              \
  case KG:                                                                                                         \
    hipLaunchKernelGGL((spread_kernel<KG, SCORE>), grid, dim3(256), 0, st, U, m, k, ldu, D, ldd, T, B, sigma, S,   \
                       lds, p.tiles_per_wg, p.ntiles, dvec, colpart, rowpart);                                     \
    break
    DMDX_CASE(1); DMDX_CASE(2); DMDX_CASE(3); DMDX_CASE(4); DMDX_CASE(5); DMDX_CASE(6); DMDX_CASE(7); DMDX_CASE(8);
    DMDX_CASE(9); DMDX_CASE(10); DMDX_CASE(11); DMDX_CASE(12); DMDX_CASE(13); DMDX_CASE(14); DMDX_CASE(15);
    DMDX_CASE(16);
#undef DMDX_CASE
    default:
      dmdx_set_error("spread: unsupported k %d", k);
      return DMDX_E_INVALID;
  }
  DMDX_LAUNCH_CHECK();
  return 0;
}

inline size_t align16(size_t n) { return (n + 15) & ~size_t(15); }

}  // namespace

extern "C" int dmdx_spread_max_k(void) { return MAXK; }

extern "C" int dmdx_spread_f32(const float* U, int64_t m, int64_t k, int64_t ldu, const float* D, int64_t ldd, int64_t T,
                               int64_t B, const float* sigma, float* S, int64_t lds, void* stream) {
  if (int rc = check_common(U, m, k, ldu, D, ldd, T, B, "dmdx_spread_f32")) return rc;
  DMDX_CHECK_ARG(S != nullptr, "dmdx_spread_f32: S must not be null");
  DMDX_CHECK_ARG(lds >= m && lds < DIM_LIMIT, "dmdx_spread_f32: lds = %lld must be in m .. 2^31 - 1", (long long)lds);
  return launch<false>(U, m, (int)k, ldu, D, ldd, T, B, sigma, S, lds, nullptr, nullptr, (hipStream_t)stream);
}

// [<= 15 bytes to a 16-byte boundary][rowpart: nsplit x m fp64][colpart: row blocks x T fp32]
extern "C" size_t dmdx_spread_score_workspace_bytes(int64_t m, int64_t k, int64_t T, int64_t B) {
  (void)k;
  (void)B;
  if (m < 1 || T < 1) return 16;
  const Plan p = plan_for(m, T);
  return 16 + align16((size_t)p.nsplit * (size_t)m * sizeof(double)) + (size_t)p.nrb * (size_t)T * sizeof(float);
}

extern "C" int dmdx_spread_score_f32(const float* U, int64_t m, int64_t k, int64_t ldu, const float* D, int64_t ldd,
                                     int64_t T, int64_t B, const float* sigma, double* var_col, double* var_row,
                                     int accumulate, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_common(U, m, k, ldu, D, ldd, T, B, "dmdx_spread_score_f32")) return rc;
  DMDX_CHECK_ARG(var_col != nullptr, "dmdx_spread_score_f32: var_col must not be null");
  const size_t need = dmdx_spread_score_workspace_bytes(m, k, T, B);
  if (workspace == nullptr || workspace_bytes < need) {
    dmdx_set_error("dmdx_spread_score_f32: workspace of %zu bytes, %zu needed", workspace == nullptr ? (size_t)0 : workspace_bytes,
                   need);
    return DMDX_E_WORKSPACE;
  }
  const Plan p = plan_for(m, T);
  hipStream_t st = (hipStream_t)stream;
  char* base = reinterpret_cast<char*>(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
  double* rowpart = reinterpret_cast<double*>(base);
  float* colpart = reinterpret_cast<float*>(base + align16((size_t)p.nsplit * (size_t)m * sizeof(double)));
  if (int rc = launch<true>(U, m, (int)k, ldu, D, ldd, T, B, sigma, nullptr, 0, colpart,
                            var_row != nullptr ? rowpart : nullptr, st))
    return rc;
  hipLaunchKernelGGL(spread_reduce_cols_kernel, dim3((unsigned)p.ntiles), dim3(256), 0, st, colpart, p.nrb, T, var_col,
                     accumulate);
  DMDX_LAUNCH_CHECK();
  if (var_row != nullptr) {
    hipLaunchKernelGGL(spread_reduce_rows_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, rowpart, p.nsplit, m,
                       var_row);
    DMDX_LAUNCH_CHECK();
  }
  return 0;
}
