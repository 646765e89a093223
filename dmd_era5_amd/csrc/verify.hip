// K16: area-weighted verification of Xhat = mu + sigma .* (U C) against the analysis X and a climatology,
// Xhat never stored.  One more body on K12's shape (expand.hip, which see for the tile, the MFMA orientation
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
// Rounding.  The contract counts roundings (q rounded, then w * q rounded; K12's sigma * acc + mu as two
// operations, which is what the compiler makes of expand.hip), so contraction is switched off for the file.
#include "dmdx_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int RWG = 128;    // rows per workgroup (4 waves x 32)
constexpr int TT = 32;      // columns of a tile
constexpr int MAXK = 256;
constexpr int NQ = DMDX_VERIFY_NQ;
static_assert(RWG == DMDX_VERIFY_FP32_ROWS, "the header documents the fp32 row count");
static_assert(NQ == 6, "the six sums of the header");

// The second __launch_bounds__ argument is WAVES PER SIMD: 2 keeps the body within 256 registers per lane, i.e. two
// 4-wave workgroups per CU (their LDS, 34 - 79 KB each, fits twice up to k = 192).  The body wants ~190 registers
// at k <= 16 already (e, f and a of a tile's 16 columns live across the six passes, the addresses of the 16 loads of
// X, six fp64 row sums) and spills 60 - 320 bytes per lane at 96 < k <= 192: the first knob to revisit.  From
// k = 193 on a workgroup holds > 80 KB of LDS, is alone on its CU anyway and is given the whole register file, as
// K12's score body is.
template <int KG>
__global__ __launch_bounds__(256, KG >= 13 ? 1 : 2) void verify_kernel(
    const float* __restrict__ U, int64_t m, int k, int64_t ldu, const float* __restrict__ C, int64_t ldc, int64_t T,
    const float* __restrict__ mu, const float* __restrict__ sigma, const float* __restrict__ X, int64_t ldx,
    const float* __restrict__ w, const float* __restrict__ clim, int64_t tiles_per_wg, int64_t ntiles, int cvec,
    float* __restrict__ colpart, double* __restrict__ rowpart) {
  constexpr int KP = 16 * KG;        // padded k
  constexpr int KS = KP + 4;         // LDS row stride of the [t][k] image
  constexpr int PPT = KP / 4;        // 16-byte pieces per column of C
  constexpr int NPIECE = TT * PPT;
  constexpr int NPT = (NPIECE + 255) / 256;
  __shared__ __attribute__((aligned(16))) float ctile[2][TT * KS];
  // Row stride of the per-wave transpose image.  36: rows on 16-byte boundaries, a lane's 16 values are four
  // 16-byte LDS reads instead of sixteen 4-byte ones (the order of the sum is the same: the identity with K12
  // holds) -- 7 - 10 % faster where it was measured (k = 10, 50, 200) and 13 - 20 registers more, which the
  // instantiations that are at the register budget with scratch (64 < k <= 192) would pay for with more of it:
  // they keep K12's 33.
  constexpr int TRS = (KG <= 4 || KG >= 13) ? 36 : 33;
  __shared__ __attribute__((aligned(16))) float tr[4 * TT * TRS];
  __shared__ float wgcol[2 * NQ * 8 * TT];   // [tile parity][quantity][wave, half][t]

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
  const float cl_i = clim != nullptr ? (rowok ? clim[row] : 0.f) : mu_i;
  const float w_i = (w != nullptr && rowok) ? w[row] : 1.f;
  const bool sel = rowok && w_i != 0.f;      // the row takes part in the column sums

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
  double rowacc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) rowacc[q] = 0.0;

  // sums the 8 (wave, half) slots of a finished tile in a fixed order into the workgroup's partial slot
  auto flush_cols = [&](int par, int64_t t0) {
    if (tid < NQ * TT) {
      const int q = tid >> 5, tl = tid & 31;
      const float* p = &wgcol[(par * NQ + q) * 8 * TT + tl];
      float s = p[0];
#pragma unroll
      for (int v = 1; v < 8; ++v) s += p[v * TT];
      if (t0 + tl < T) colpart[((int64_t)blockIdx.x * NQ + q) * T + t0 + tl] = s;
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
    float xv[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t t = t0 + (r & 3) + 8 * (r >> 2) + 4 * h;
      xv[r] = (rowok && t < T) ? X[t * ldx + row] : 0.f;
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

    // K12's epilogue
    float xh[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float v = acc[r];
      if (sigma != nullptr) v *= sg_i;
      if (mu != nullptr) v += mu_i;
      xh[r] = v;
    }

    // sums over the wave's 32 rows: [t][i] image of the wave, lane (t = li, h) adds rows 16 h .. 16 h + 15
    // (LDS operations of one wave execute in order: no barrier between its writes and its reads)
    float* trw = &tr[wave * TT * TRS];
    const int par = (int)((tile - tile0) & 1);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      float rs = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int tl = (r & 3) + 8 * (r >> 2) + 4 * h;
        const bool ok = rowok && t0 + tl < T;
        const float e = xh[r] - xv[r], f = xh[r] - cl_i, a = xv[r] - cl_i;
        const float val = q == 0 ? e * e : q == 1 ? e : q == 2 ? a : q == 3 ? f * f : q == 4 ? a * a : f * a;
        rs += ok ? val : 0.f;
        trw[tl * TRS + li] = (ok && sel) ? (w != nullptr ? w_i * val : val) : 0.f;
      }
      rowacc[q] += (double)rs;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      float s = trw[li * TRS + 16 * h];
#pragma unroll
      for (int j = 1; j < 16; ++j) s += trw[li * TRS + 16 * h + j];
      wgcol[((par * NQ + q) * 8 + 2 * wave + h) * TT + li] = s;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_sched_barrier(0);   // one quantity at a time: the next one's 16 terms are not formed early
    }

    if (has_next) store_c(cur ^ 1);
    __syncthreads();
    // (the slots of this parity are written again two tiles on, behind the next barrier)
    flush_cols(par, t0);
    cur ^= 1;
  }

  if (rowpart != nullptr) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const double other = __shfl_xor(rowacc[q], 32, 64);
      if (h == 0 && rowok) rowpart[((int64_t)blockIdx.y * NQ + q) * m + row] = rowacc[q] + other;
    }
  }
}

// col[q][t] (+)= sum over the row blocks of colpart[rb][q][t] in fp64: K12's reduce, blockIdx.y = quantity
__global__ __launch_bounds__(256) void verify_reduce_cols_kernel(const float* __restrict__ colpart, int64_t nrb, int64_t T,
                                                                 double* __restrict__ col, int64_t ldcol, int accumulate) {
  __shared__ double part[8][32];
  const int q = blockIdx.y;
  double* out = col + (int64_t)q * ldcol;
  const int j = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int64_t t = (int64_t)blockIdx.x * 32 + j;
  double s = 0.0;
  if (t < T)
    for (int64_t rb = sl; rb < nrb; rb += 8) s += (double)colpart[(rb * NQ + q) * T + t];
  part[sl][j] = s;
  __syncthreads();
  if (sl != 0 || t >= T) return;
#pragma unroll
  for (int v = 1; v < 8; ++v) s += part[v][j];
  out[t] = accumulate ? out[t] + s : s;
}

__global__ __launch_bounds__(256) void verify_reduce_rows_kernel(const double* __restrict__ rowpart, int64_t nsplit, int64_t m,
                                                                 double* __restrict__ row, int64_t ldrow) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int q = blockIdx.y;
  if (i >= m) return;
  double s = rowpart[(int64_t)q * m + i];
  for (int64_t y = 1; y < nsplit; ++y) s += rowpart[(y * NQ + q) * m + i];
  row[(int64_t)q * ldrow + i] = s;
}

// K12's plan (expand.hip, plan_for), repeated: the identity of col[0], col[4] and row[0] with K12's sums rests on
// the same row blocks and the same T split.  A function of the shapes only.
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

inline size_t align16(size_t n) { return (n + 15) & ~size_t(15); }

}  // namespace

extern "C" int dmdx_verify_max_k(void) { return MAXK; }

// [<= 15 bytes to a 16-byte boundary][rowpart: nsplit x 6 x m fp64][colpart: row blocks x 6 x T fp32]
extern "C" size_t dmdx_verify_workspace_bytes(int64_t m, int64_t k, int64_t T) {
  (void)k;
  if (m < 1 || T < 1 || m >= DIM_LIMIT || T >= DIM_LIMIT) return 16;
  const Plan p = plan_for(m, T);
  return 16 + align16((size_t)p.nsplit * NQ * (size_t)m * sizeof(double)) + (size_t)p.nrb * NQ * (size_t)T * sizeof(float);
}

extern "C" int dmdx_verify_f32(const float* U, int64_t m, int64_t k, int64_t ldu, const float* C, int64_t ldc, int64_t T,
                               const float* mu, const float* sigma, const float* X, int64_t ldx, const float* w,
                               const float* clim, double* col, int64_t ldcol, double* row, int64_t ldrow, int accumulate,
                               void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "dmdx_verify_f32";
  DMDX_CHECK_ARG(U != nullptr && C != nullptr && X != nullptr && col != nullptr, "%s: U, C, X and col must not be null", who);
  DMDX_CHECK_ARG(m >= 1 && T >= 1, "%s: m = %lld, T = %lld must be >= 1", who, (long long)m, (long long)T);
  DMDX_CHECK_ARG(k >= 1 && k <= MAXK, "%s: k = %lld outside 1 .. %d", who, (long long)k, MAXK);
  DMDX_CHECK_ARG(ldu >= m && ldc >= k, "%s: ldu = %lld < m = %lld or ldc = %lld < k = %lld", who, (long long)ldu,
                 (long long)m, (long long)ldc, (long long)k);
  DMDX_CHECK_ARG(m < DIM_LIMIT && T < DIM_LIMIT && ldu < DIM_LIMIT && ldc < DIM_LIMIT, "%s: m, T, ldu, ldc must be < 2^31", who);
  DMDX_CHECK_ARG(ldx >= 1 && ldx < DIM_LIMIT, "%s: ldx = %lld must be in 1 .. 2^31 - 1", who, (long long)ldx);
  DMDX_CHECK_ARG(ldcol >= T && ldcol < DIM_LIMIT, "%s: ldcol = %lld must be in T = %lld .. 2^31 - 1", who, (long long)ldcol,
                 (long long)T);
  DMDX_CHECK_ARG(row == nullptr || (ldrow >= m && ldrow < DIM_LIMIT), "%s: ldrow = %lld must be in m = %lld .. 2^31 - 1", who,
                 (long long)ldrow, (long long)m);
  const size_t need = dmdx_verify_workspace_bytes(m, k, T);
  if (workspace == nullptr || workspace_bytes < need) {
    dmdx_set_error("%s: workspace of %zu bytes, %zu needed", who, workspace == nullptr ? (size_t)0 : workspace_bytes, need);
    return DMDX_E_WORKSPACE;
  }
  const Plan p = plan_for(m, T);
  hipStream_t st = (hipStream_t)stream;
  char* base = reinterpret_cast<char*>(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
  double* rowpart = reinterpret_cast<double*>(base);
  float* colpart = reinterpret_cast<float*>(base + align16((size_t)p.nsplit * NQ * (size_t)m * sizeof(double)));
  const int cvec = dmdx_aligned16(C) && ldc % 4 == 0;
  const dim3 grid((unsigned)p.nrb, (unsigned)p.nsplit);
  switch ((int)((k + 15) / 16)) {
#define DMDX_CASE(KG)                                                                                               \
  case KG:                                                                                                          \
    hipLaunchKernelGGL((verify_kernel<KG>), grid, dim3(256), 0, st, U, m, (int)k, ldu, C, ldc, T, mu, sigma, X, ldx, w, \
                       clim, p.tiles_per_wg, p.ntiles, cvec, colpart, row != nullptr ? rowpart : nullptr);           \
    break
    DMDX_CASE(1); DMDX_CASE(2); DMDX_CASE(3); DMDX_CASE(4); DMDX_CASE(5); DMDX_CASE(6); DMDX_CASE(7); DMDX_CASE(8);
    DMDX_CASE(9); DMDX_CASE(10); DMDX_CASE(11); DMDX_CASE(12); DMDX_CASE(13); DMDX_CASE(14); DMDX_CASE(15);
    DMDX_CASE(16);
#undef DMDX_CASE
    default:
      dmdx_set_error("%s: unsupported k %lld", who, (long long)k);
      return DMDX_E_INVALID;
  }
  DMDX_LAUNCH_CHECK();
  hipLaunchKernelGGL(verify_reduce_cols_kernel, dim3((unsigned)p.ntiles, NQ), dim3(256), 0, st, colpart, p.nrb, T, col, ldcol,
                     accumulate);
  DMDX_LAUNCH_CHECK();
  if (row != nullptr) {
    hipLaunchKernelGGL(verify_reduce_rows_kernel, dim3((unsigned)((m + 255) / 256), NQ), dim3(256), 0, st, rowpart, p.nsplit, m,
                       row, ldrow);
    DMDX_LAUNCH_CHECK();
  }
  return 0;
}
