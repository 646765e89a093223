// K12's tile, once: the shape expand.hip (K12), spread.hip (K15), verify.hip (K16) and pack.hip (K17) share.  The
// four kernels form the same field Xhat = U C the same way -- tile, k order, T split, epilogue rounding -- and their
// contracts are identities between them (verify without w / clim IS expand_score, expand_pack packs exactly expand's
// field, spread with B = 1 is |expand|): those hold because the pieces below have one definition.
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
// a multiple of 16 with zeros on BOTH sides: 0 * 0, never a clamped duplicate), then sigma * acc + mu:
// two operations, two roundings (affine()).
//
// Sums of NQ quantities per element (the scores of K12, K15, K16), each
//   over the 32 rows of a wave through a per-wave LDS transpose (16 writes, 16 reads per lane and tile:
//     the sum runs over the lane index, which no MFMA contracts), over the 4 waves through 8 LDS slots
//     in a fixed order: fp32 over the 128 rows of the workgroup, written to the workgroup's own slot
//     colpart[row block][NQ][T]; a second kernel adds the row blocks in fp64;
//   over t per lane (16 values of a tile in fp32, tiles in fp64): rowpart[T split][NQ][m], added by a
//     third kernel.
// No atomics anywhere: every sum has a fixed order that depends on the shapes only.
#pragma once

#include "dmdx_common.h"

namespace {

constexpr int RWG = 128;    // rows per workgroup (4 waves x 32)
constexpr int TT = 32;      // columns of a tile
constexpr int MAXK = 256;
constexpr int64_t DIM_LIMIT = int64_t(1) << 31;

inline size_t align16(size_t n) { return (n + 15) & ~size_t(15); }

// ---------------------------------------------------------------- device: the tile
// Two compile results shaped the signatures below (make resource-usage, MEASUREMENTS.md "shared tile header").
// Lane goes by value: by reference the two KG = 16 bodies at the register budget spill 8 - 12 bytes per lane more.
// Pointers are plain: the kernels' own parameters carry __restrict__, and a second one on an inlined parameter made
// the compiler duplicate spread's member loop (spread_kernel<1, true>: 100 instead of 96 VGPRs, a wave per SIMD less).
template <int KG>   // k in granules of 16
struct Geom {
  static constexpr int KP = 16 * KG;        // padded k
  static constexpr int KS = KP + 4;         // LDS row stride of the [t][k] image
  static constexpr int PPT = KP / 4;        // 16-byte pieces per column of C
  static constexpr int NPIECE = TT * PPT;
  static constexpr int NPT = (NPIECE + 255) / 256;
  static constexpr int STAGE = TT * KS;     // floats of one LDS stage
};

struct Lane {
  int tid, wave, li, h;     // lane (li, h) of wave `wave` holds row `row` and, in register r, column col_of(r, h)
  int64_t row;
  bool rowok;
};

__device__ __forceinline__ Lane lane_of(int64_t m) {
  Lane L;
  L.tid = threadIdx.x;
  L.wave = __builtin_amdgcn_readfirstlane(L.tid >> 6);
  L.li = L.tid & 31;
  L.h = (L.tid & 63) >> 5;
  L.row = (int64_t)blockIdx.x * RWG + L.wave * 32 + L.li;
  L.rowok = L.row < m;
  return L;
}

// the column of a tile that accumulator register r of lane half h holds
__device__ __forceinline__ int col_of(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// the wave's U panel: register 4 q + e = U[row][8 q + 4 h + e]; exact zeros past k and past m
template <int KG>
__device__ __forceinline__ void load_panel(float (&ureg)[8 * KG], const float* U, int64_t ldu, int k, const Lane L) {
#pragma unroll
  for (int s = 0; s < 8 * KG; ++s) {
    const int j = 8 * (s >> 2) + 4 * L.h + (s & 3);
    ureg[s] = (L.rowok && j < k) ? U[(int64_t)j * ldu + L.row] : 0.f;
  }
}

// A tile's 32 x k slice of C on its way to LDS: load() into registers before the MFMAs, store() behind them.
template <int KG>
struct Stager {
  using G = Geom<KG>;
  f32x4 reg[G::NPT];

  // snapshots t0 .. t0 + 31 (zeros from T on) of member b: the columns b T + t of C (b = 0 but for spread's B T
  // columns of D); vec: C is 16-byte aligned with ldc % 4 == 0 (cvec_of)
  __device__ __forceinline__ void load(const float* C, int64_t ldc, int64_t b, int64_t t0, int64_t T, int k, int vec,
                                       int tid) {
#pragma unroll
    for (int i = 0; i < G::NPT; ++i) {
      const int idx = tid + 256 * i;
      if (G::NPIECE % 256 != 0 && idx >= G::NPIECE) continue;
      const int tl = idx / G::PPT, j = 4 * (idx % G::PPT);
      const int64_t t = t0 + tl;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (t < T && j < k) {
        const float* q = C + (b * T + t) * ldc + j;
        if (vec && j + 4 <= k) {
          v = *reinterpret_cast<const f32x4*>(q);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (j + e < k) v[e] = q[e];
        }
      }
      reg[i] = v;
    }
  }

  __device__ __forceinline__ void store(float* stage, int tid) const {
#pragma unroll
    for (int i = 0; i < G::NPT; ++i) {
      const int idx = tid + 256 * i;
      if (G::NPIECE % 256 != 0 && idx >= G::NPIECE) continue;
      *reinterpret_cast<f32x4*>(&stage[(idx / G::PPT) * G::KS + 4 * (idx % G::PPT)]) = reg[i];
    }
  }
};

// the tile of a stage: acc[r] = sum_j C[j][col_of(r, h)] U[row][j], one chain in the fixed k order
template <int KG>
__device__ __forceinline__ f32x16 mfma_chain(const float* stage, const float (&ureg)[8 * KG], const Lane L) {
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const float* ct = &stage[L.li * Geom<KG>::KS + 4 * L.h];
#pragma unroll
  for (int q = 0; q < 2 * KG; ++q) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(ct + 8 * q);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], ureg[4 * q + e], acc, 0, 0, 0);
  }
  return acc;
}

// K12's epilogue sigma * acc + mu: a multiply and an add, each rounded -- never one fused operation, whatever the
// including file's contraction mode is
__device__ __forceinline__ float affine(float acc, bool has_sigma, float sg_i, bool has_mu, float mu_i) {
#pragma clang fp contract(off)
  float v = acc;
  if (has_sigma) v *= sg_i;
  if (has_mu) v += mu_i;
  return v;
}

// ---------------------------------------------------------------- device: the sums
// One quantity of a tile summed over the wave's 32 rows: val(r), the lane's value in column col_of(r, h), goes into
// the wave's [t][i] image trw (32 rows of stride TRS) as it is formed, lane (t = li, h) adds rows 16 h .. 16 h + 15 in
// index order and writes slot 2 wave + h of `slots` (8 x 32 floats).  LDS operations of one wave execute in order:
// no workgroup barrier between its writes and its reads.  Contract: val is called exactly once for each r, in the
// order r = 0 .. 15 -- verify's callable adds its row sum on the way, and the order of that sum is part of its result.
template <int TRS, class F>
__device__ __forceinline__ void wave_col_sum(float* trw, float* slots, const Lane L, F&& val) {
#pragma unroll
  for (int r = 0; r < 16; ++r) trw[col_of(r, L.h) * TRS + L.li] = val(r);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  float s = trw[L.li * TRS + 16 * L.h];
#pragma unroll
  for (int j = 1; j < 16; ++j) s += trw[L.li * TRS + 16 * L.h + j];
  slots[(2 * L.wave + L.h) * TT + L.li] = s;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// after the tile's barrier: the 8 (wave, half) slots of each of the NQ quantities (slots: [NQ][8][32]) summed in a
// fixed order into the workgroup's partial slot colpart[row block][q][t]
template <int NQ>
__device__ __forceinline__ void flush_cols(const float* slots, float* colpart, int64_t t0, int64_t T, int tid) {
  if (tid < NQ * TT) {
    const int q = tid >> 5, tl = tid & 31;
    const float* w = &slots[q * 8 * TT + tl];
    float s = w[0];
#pragma unroll
    for (int v = 1; v < 8; ++v) s += w[v * TT];
    if (t0 + tl < T) colpart[((int64_t)blockIdx.x * NQ + q) * T + t0 + tl] = s;
  }
}

// the end of a score kernel: a lane's sums over t (one half of its row's columns) meet the other half's
template <int NQ>
__device__ __forceinline__ void store_row_sums(const double (&rowacc)[NQ], double* rowpart, int64_t m, const Lane L) {
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const double other = __shfl_xor(rowacc[q], 32, 64);
    if (L.h == 0 && L.rowok) rowpart[((int64_t)blockIdx.y * NQ + q) * m + L.row] = rowacc[q] + other;
  }
}

// out(q)[t] (+)= sum over the row blocks of colpart[rb][q][t] in fp64, q = blockIdx.y: 32 columns x 8 slot lanes per
// workgroup, every thread adds its row blocks sl, sl + 8, ..., the 8 lanes meet in LDS in a fixed order.  Where
// quantity q goes is the caller's: the columns of a matrix (ColsOf), or vectors of its own (expand.hip).
struct ColsOf {
  double* p;
  int64_t ld;
  __device__ double* operator()(int q) const { return p + (int64_t)q * ld; }
};
template <int NQ, class Out>
__global__ __launch_bounds__(256) void reduce_cols_kernel(const float* __restrict__ colpart, int64_t nrb, int64_t T,
                                                          Out where, int accumulate) {
  __shared__ double part[8][32];
  const int q = blockIdx.y;
  double* out = where(q);
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

// out[q][i] = sum over the T splits of rowpart[split][q][i], q = blockIdx.y
template <int NQ>
__global__ __launch_bounds__(256) void reduce_rows_kernel(const double* __restrict__ rowpart, int64_t nsplit, int64_t m,
                                                          double* __restrict__ out, int64_t ldout) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int q = blockIdx.y;
  if (i >= m) return;
  double s = rowpart[(int64_t)q * m + i];
  for (int64_t y = 1; y < nsplit; ++y) s += rowpart[(y * NQ + q) * m + i];
  out[(int64_t)q * ldout + i] = s;
}

// Integer counts (K19, K24): hist[r] (+)= sum over the workgroups' slots of histpart[slot][r], r = blockIdx.x: integers, any order
__global__ __launch_bounds__(256) void reduce_hist_kernel(const long long* __restrict__ histpart, int64_t nslot, int nbin,
                                                          long long* __restrict__ hist, int accumulate) {
  __shared__ long long part[256];
  const int r = blockIdx.x;
  long long s = 0;
  for (int64_t j = threadIdx.x; j < nslot; j += 256) s += histpart[j * nbin + r];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int half = 128; half >= 1; half >>= 1) {
    if ((int)threadIdx.x < half) part[threadIdx.x] += part[threadIdx.x + half];
    __syncthreads();
  }
  if (threadIdx.x == 0) hist[r] = accumulate ? hist[r] + part[0] : part[0];
}

// ---------------------------------------------------------------- host
// the T axis is split over blockIdx.y until the launch has ~2048 workgroups (8 per CU); a function of the
// shapes only, so that the partial sums -- and with them the results -- do not depend on the device
struct Plan {
  int64_t nrb, ntiles, tiles_per_wg, nsplit;
  dim3 grid() const { return dim3((unsigned)nrb, (unsigned)nsplit); }
};
inline Plan plan_for(int64_t m, int64_t T) {
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

// the 16-byte fast path of the stager
inline int cvec_of(const float* C, int64_t ldc) { return dmdx_aligned16(C) && ldc % 4 == 0; }

// the factors U (m x k) and C (k x T); cname and ldname are what the messages call the second one ("D", "ldd" in K15)
inline int check_common(const float* U, int64_t m, int64_t k, int64_t ldu, const float* C, int64_t ldc, int64_t T,
                        const char* who, const char* cname = "C", const char* ldname = "ldc") {
  DMDX_CHECK_ARG(U != nullptr && C != nullptr, "%s: U and %s must not be null", who, cname);
  DMDX_CHECK_ARG(m >= 1 && T >= 1, "%s: m = %lld, T = %lld must be >= 1", who, (long long)m, (long long)T);
  DMDX_CHECK_ARG(k >= 1 && k <= MAXK, "%s: k = %lld outside 1 .. %d", who, (long long)k, MAXK);
  DMDX_CHECK_ARG(ldu >= m && ldc >= k, "%s: ldu = %lld < m = %lld or %s = %lld < k = %lld", who, (long long)ldu,
                 (long long)m, ldname, (long long)ldc, (long long)k);
  DMDX_CHECK_ARG(m < DIM_LIMIT && T < DIM_LIMIT && ldu < DIM_LIMIT && ldc < DIM_LIMIT,
                 "%s: m, T, ldu, %s must be < 2^31", who, ldname);
  return 0;
}

// The workspace of a score of nq quantities, nq_rows of them with row sums (all of them but for K12, whose ref has none):
// [<= 15 bytes to a 16-byte boundary][rowpart: nsplit x nq_rows x m fp64][colpart: row blocks x nq x T fp32]
inline size_t score_ws_bytes(int64_t m, int64_t T, int nq, int nq_rows) {
  const Plan p = plan_for(m, T);
  return 16 + align16((size_t)p.nsplit * nq_rows * (size_t)m * sizeof(double)) + (size_t)p.nrb * nq * (size_t)T * sizeof(float);
}
struct ScoreWs {
  double* rowpart;
  float* colpart;
};
inline ScoreWs score_ws(void* workspace, const Plan& p, int64_t m, int nq_rows) {
  char* base = reinterpret_cast<char*>(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
  return {reinterpret_cast<double*>(base),
          reinterpret_cast<float*>(base + align16((size_t)p.nsplit * nq_rows * (size_t)m * sizeof(double)))};
}

// the workspace of an entry point against what its *_workspace_bytes asks for
inline int check_workspace(const void* workspace, size_t workspace_bytes, size_t need, const char* who) {
  if (workspace == nullptr || workspace_bytes < need) {
    dmdx_set_error("%s: workspace of %zu bytes, %zu needed", who, workspace == nullptr ? (size_t)0 : workspace_bytes, need);
    return DMDX_E_WORKSPACE;
  }
  return 0;
}

// X and the (NQ, T) / (NQ, m) results of a score that hands its sums back as matrices (K16, K19)
inline int check_score_lds(int64_t m, int64_t T, int64_t ldx, int64_t ldcol, const double* row, int64_t ldrow,
                           const char* who) {
  DMDX_CHECK_ARG(ldx >= 1 && ldx < DIM_LIMIT, "%s: ldx = %lld must be in 1 .. 2^31 - 1", who, (long long)ldx);
  DMDX_CHECK_ARG(ldcol >= T && ldcol < DIM_LIMIT, "%s: ldcol = %lld must be in T = %lld .. 2^31 - 1", who, (long long)ldcol,
                 (long long)T);
  DMDX_CHECK_ARG(row == nullptr || (ldrow >= m && ldrow < DIM_LIMIT), "%s: ldrow = %lld must be in m = %lld .. 2^31 - 1", who,
                 (long long)ldrow, (long long)m);
  return 0;
}

// The end of a score entry point, behind its tile kernel: the first `planes` of the NQ column quantities go from
// colpart to where(q) in fp64 and, if `row` is given, the NQ_ROWS row quantities from rowpart to row[q * ldrow + i].
template <int NQ, int NQ_ROWS, class Out>
int reduce_score(const ScoreWs& ws, const Plan& p, int64_t m, int64_t T, int planes, Out where, int accumulate, double* row,
                 int64_t ldrow, hipStream_t st) {
  hipLaunchKernelGGL((reduce_cols_kernel<NQ, Out>), dim3((unsigned)p.ntiles, planes), dim3(256), 0, st, ws.colpart, p.nrb, T,
                     where, accumulate);
  DMDX_LAUNCH_CHECK();
  if (row != nullptr) {
    hipLaunchKernelGGL(reduce_rows_kernel<NQ_ROWS>, dim3((unsigned)((m + 255) / 256), NQ_ROWS), dim3(256), 0, st, ws.rowpart,
                       p.nsplit, m, row, ldrow);
    DMDX_LAUNCH_CHECK();
  }
  return 0;
}

// One instantiation per granule count: LAUNCH(KG) for KG = ceil(k / 16) in 1 .. 16.
#define DMDX_DISPATCH_KG(k, who, LAUNCH)                                   \
  switch (((k) + 15) / 16) {                                               \
    case 1: LAUNCH(1); break;                                              \
    case 2: LAUNCH(2); break;                                              \
    case 3: LAUNCH(3); break;                                              \
    case 4: LAUNCH(4); break;                                              \
    case 5: LAUNCH(5); break;                                              \
    case 6: LAUNCH(6); break;                                              \
    case 7: LAUNCH(7); break;                                              \
    case 8: LAUNCH(8); break;                                              \
    case 9: LAUNCH(9); break;                                              \
    case 10: LAUNCH(10); break;                                            \
    case 11: LAUNCH(11); break;                                            \
    case 12: LAUNCH(12); break;                                            \
    case 13: LAUNCH(13); break;                                            \
    case 14: LAUNCH(14); break;                                            \
    case 15: LAUNCH(15); break;                                            \
    case 16: LAUNCH(16); break;                                            \
    default:                                                               \
      dmdx_set_error("%s: unsupported k %lld", who, (long long)(k));       \
      return DMDX_E_INVALID;                                               \
  }

}  // namespace
