// K24: the probability that the B member fields x_b = mu + sigma .* (U C_b) exceed (or fall below) a threshold, and
// the sums behind the Brier score, the reliability diagram and the ROC curve against the analysis X -- no member field
// stored.  U: m x k, C: k x (B T), column b T + t = the coefficients of member b at snapshot t, thr: m x (J S), column
// j S + s = threshold j of every row for slot s, slot[t] the slot of snapshot t.  Per element and threshold j, fp32:
//   c = #{b : x_b <> thr}      p = fl(c / B)      o = (y <> thr) ? 1 : 0      y = X[i, t],  <> is > (above) or <
// One more body on K12's shape (expand_tile.h, which see for the tile, the MFMA orientation and the k order) with
// K19's member loop: a workgroup (4 waves) owns 128 rows, every wave keeps its 32 x k panel of U in registers, the
// 32 x k slice of C of a (tile, member) step goes through LDS, double buffered, one barrier per step.  A member field
// is K12's chain and K12's affine(): bit for bit what dmdx_expand_f32 gives for C_b.
//
// One pass for all thresholds.  The 16 x J thresholds of a lane's elements are loaded once per tile (J is a
// run-time, wave-uniform value: the loops over j are unrolled to DMDX_EXCEED_MAX_THR = 4 and guarded by j < J, so
// every array stays in registers and the 16 instantiations over k are not multiplied), and a member costs, behind its
// chain, one compare and one add per threshold and element.  B chains per tile whatever J is: K15's count.
//
// The direction is folded into the sign: for `below` the thresholds, the members and y have their sign bit flipped
// (x < thr  <=>  -x > -thr for every IEEE value, zeros and infinities included), so the loop has one strict compare.
// A NaN on either side compares false: no event.  A snapshot whose slot lies outside 0 .. S - 1 reads nothing of thr
// and has NaN thresholds.
//
// Finite.  fin = fma(x_b, 0, fin) over the members is +0.0 while every member is finite and NaN from the first Inf
// or NaN on (one exact operation per member); the score adds (y - y).  It is ADDED to every quantity: q + (+0.0) = q
// for the non-negative quantities here, NaN otherwise.
//
// p.  c / B for c = 0 .. B is divided once per workgroup in fp64 and rounded to fp32 into an LDS table of B + 1
// entries: for c <= B <= 256 that is the fp32 nearest to c / B.
//
// Sums of the 4 J quantities (d^2, o, p, p^2 with d = fl(p - o), per threshold): K16's / K19's -- over the 32 rows of
// a wave through the per-wave LDS transpose, over the 4 waves through 8 LDS slots in a fixed order, fp32 over the
// DMDX_EXCEED_FP32_ROWS = 128 rows of the workgroup into colpart[row block][4 J][T], fp64 over the row blocks in a
// second kernel; over t per lane (16 values in fp32, tiles in fp64) into rowpart[T split][4 J][m], added by a third
// kernel.  No floating-point atomics.  flush_cols<NQ> serves NQ * 32 <= 256 threads; its strided twin below walks the
// 4 J * 32 sums with the same order inside each sum.
//
// Counts.  After the last member of a tile every selected, finite element adds 1 to bin ((2 j + o) (B + 1) + c) of
// the workgroup's LDS counters (2 J (B + 1) <= 2056 uint32 bins, integer LDS atomics: an integer sum has no order).
// Behind the tile's barrier thread i moves bins i, i + 256, ... into its own int64 registers and zeroes them, so a
// bin never holds more than the 128 x 32 = 4096 elements of one tile and the running counts are 64 bits wide.  At its
// end the workgroup writes its counts to its slot of the workspace, and reduce_hist_kernel adds the slots.
//
// Registers.  k / 2 of U, 16 J of thresholds, 8 J of counts (two 16-bit counts per register: with one count each the
// score body at k = 240 spilled 20 bytes per lane), 16 each of X, fin and the accumulator, k / 32 x 4 of staging, 32
// of row sums, 18 of counts: every instantiation is given the unified 512-entry file (__launch_bounds__(256, 1)), as
// K19's; none has scratch (what the compiler reports is in MEASUREMENTS.md, K24).
#include "expand_tile.h"

#pragma clang fp contract(off)

namespace {

constexpr int NQ = DMDX_EXCEED_NQ;
constexpr int MAXJ = DMDX_EXCEED_MAX_THR;
constexpr int MAXB = DMDX_EXCEED_MAX_B;
constexpr int NBIN = 2 * MAXJ * (MAXB + 1);    // 2056
constexpr int BINS_PER_THREAD = (NBIN + 255) / 256;
constexpr int TRS = 33;                        // row stride of the per-wave transpose image
static_assert(RWG == DMDX_EXCEED_FP32_ROWS, "the header documents the fp32 row count");
static_assert(NQ == 4, "d^2, o, p, p^2");
static_assert(MAXJ == 4, "the host switches over J = 1 .. 4");

__device__ __forceinline__ float flip(float v, unsigned sgn) { return __uint_as_float(__float_as_uint(v) ^ sgn); }

// threshold j's count in its packed register
__device__ __forceinline__ int count_of(int packed, int j) { return (packed >> (16 * (j & 1))) & 0xffff; }

// flush_cols for nq * 32 > 256 sums: sum idx = q * 32 + tl, the 8 (wave, half) slots in flush_cols' order
__device__ __forceinline__ void flush_cols_strided(const float* slots, float* colpart, int nq, int64_t t0, int64_t T, int tid) {
  for (int idx = tid; idx < nq * TT; idx += 256) {
    const int q = idx >> 5, tl = idx & 31;
    const float* w = &slots[q * 8 * TT + tl];
    float s = w[0];
#pragma unroll
    for (int v = 1; v < 8; ++v) s += w[v * TT];
    if (t0 + tl < T) colpart[((int64_t)blockIdx.x * nq + q) * T + t0 + tl] = s;
  }
}

// SCORE: the sums and the counts against X; otherwise the J probability planes
template <int KG, bool SCORE>
__global__ __launch_bounds__(256, 1) void exceed_kernel(
    const float* __restrict__ U, int64_t m, int k, int64_t ldu, const float* __restrict__ C, int64_t ldc, int64_t T,
    int B, const float* __restrict__ mu, const float* __restrict__ sigma, const float* __restrict__ thr, int64_t ldthr,
    int J, int64_t S, const int32_t* __restrict__ slot, unsigned sgn, const float* __restrict__ X, int64_t ldx,
    const float* __restrict__ w, int64_t tiles_per_wg, int64_t ntiles, int cvec, float* __restrict__ P, int64_t ldp,
    int64_t pstride, float* __restrict__ colpart, double* __restrict__ rowpart, long long* __restrict__ histpart) {
  __shared__ __attribute__((aligned(16))) float ctile[2][Geom<KG>::STAGE];
  __shared__ float ptab[MAXB + 1];
  __shared__ float tr[SCORE ? 4 * TT * TRS : 1];
  __shared__ float wgcol[SCORE ? MAXJ * NQ * 8 * TT : 1];   // [threshold, quantity][wave, half][t]
  __shared__ unsigned lhist[SCORE ? BINS_PER_THREAD * 256 : 1];

  const Lane L = lane_of(m);
  float ureg[8 * KG];
  load_panel<KG>(ureg, U, ldu, k, L);
  const float mu_i = (mu != nullptr && L.rowok) ? mu[L.row] : 0.f;
  const float sg_i = (sigma != nullptr && L.rowok) ? sigma[L.row] : 1.f;
  const float w_i = (SCORE && w != nullptr && L.rowok) ? w[L.row] : 1.f;
  const bool sel = L.rowok && w_i != 0.f;      // the row takes part in the column sums and the counts
  const int nbin = 2 * J * (B + 1);

  const int64_t tile0 = (int64_t)blockIdx.y * tiles_per_wg;
  const int64_t tile1 = tile0 + tiles_per_wg < ntiles ? tile0 + tiles_per_wg : ntiles;
  double rowacc[MAXJ * NQ];
  long long histacc[BINS_PER_THREAD];
  if (SCORE) {
#pragma unroll
    for (int q = 0; q < MAXJ * NQ; ++q) rowacc[q] = 0.0;
#pragma unroll
    for (int s = 0; s < BINS_PER_THREAD; ++s) {
      histacc[s] = 0;
      lhist[L.tid + 256 * s] = 0u;
    }
  }
  for (int c = L.tid; c <= B; c += 256) ptab[c] = (float)((double)c / (double)B);

  Stager<KG> cs;
  cs.load(C, ldc, 0, tile0 * TT, T, k, cvec, L.tid);
  cs.store(ctile[0], L.tid);
  __syncthreads();
  int cur = 0;
  for (int64_t tile = tile0; tile < tile1; ++tile) {
    const int64_t t0 = tile * TT;
    float thrs[MAXJ][16], fin[16];
    int cnt2[MAXJ / 2][16];                       // two 16-bit counts (<= 256 each) per register: thresholds 2 i, 2 i + 1
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t t = t0 + col_of(r, L.h);
      const bool in = L.rowok && t < T;
      const int32_t sl = (slot != nullptr && t < T) ? slot[t] : 0;
      const bool has = in && sl >= 0 && (int64_t)sl < S;
      fin[r] = 0.f;
#pragma unroll
      for (int j = 0; j < MAXJ / 2; ++j) cnt2[j][r] = 0;
#pragma unroll
      for (int j = 0; j < MAXJ; ++j) {
        thrs[j][r] = __uint_as_float(kQuietNaN);
        if (j < J && has) thrs[j][r] = flip(thr[((int64_t)j * S + sl) * ldthr + L.row], sgn);
      }
    }

    for (int b = 0; b < B; ++b) {
      const bool more = b + 1 < B;
      const bool has_next = more || tile + 1 < tile1;
      if (has_next) cs.load(C, ldc, more ? b + 1 : 0, more ? t0 : t0 + TT, T, k, cvec, L.tid);

      const f32x16 acc = mfma_chain<KG>(ctile[cur], ureg, L);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float x = affine(acc[r], sigma != nullptr, sg_i, mu != nullptr, mu_i);
        fin[r] = __builtin_fmaf(x, 0.f, fin[r]);
        const float xs = flip(x, sgn);
#pragma unroll
        for (int j = 0; j < MAXJ; ++j)
          if (j < J) cnt2[j >> 1][r] += xs > thrs[j][r] ? 1 << (16 * (j & 1)) : 0;
      }

      if (has_next) cs.store(ctile[cur ^ 1], L.tid);
      __syncthreads();
      cur ^= 1;
    }

    if constexpr (!SCORE) {
#pragma unroll
      for (int j = 0; j < MAXJ; ++j) {
        if (j < J) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int64_t t = t0 + col_of(r, L.h);
            if (L.rowok && t < T) P[(int64_t)j * pstride + t * ldp + L.row] = ptab[count_of(cnt2[j >> 1][r], j)] + fin[r];
          }
        }
      }
    } else {
      // the tile's quantities and its counts; wgcol and lhist were read last behind the previous tile's second
      // barrier, and at least one step's barrier lies between
      float ys[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t t = t0 + col_of(r, L.h);
        const float y = (L.rowok && t < T) ? X[t * ldx + L.row] : 0.f;
        fin[r] += y - y;
        ys[r] = flip(y, sgn);
      }
      float* trw = &tr[L.wave * TT * TRS];
#pragma unroll
      for (int j = 0; j < MAXJ; ++j) {
        if (j < J) {
          float pj[16], oj[16];
          int cj[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            cj[r] = count_of(cnt2[j >> 1][r], j);
            pj[r] = ptab[cj[r]];
            oj[r] = ys[r] > thrs[j][r] ? 1.f : 0.f;
          }
#pragma unroll
          for (int q = 0; q < NQ; ++q) {
            float rs = 0.f;
            wave_col_sum<TRS>(trw, &wgcol[(j * NQ + q) * 8 * TT], L, [&](int r) {
              const bool ok = L.rowok && t0 + col_of(r, L.h) < T;
              const float d = pj[r] - oj[r];
              const float val = (q == 0 ? d * d : q == 1 ? oj[r] : q == 2 ? pj[r] : pj[r] * pj[r]) + fin[r];
              rs += ok ? val : 0.f;
              return (ok && sel) ? (w != nullptr ? w_i * val : val) : 0.f;
            });
            rowacc[j * NQ + q] += (double)rs;
          }
          if (histpart != nullptr) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const bool ok = sel && t0 + col_of(r, L.h) < T;
              // fin is +0.0 or NaN; the count is in 0 .. B <= 256
              if (ok && fin[r] == 0.f) atomicAdd(&lhist[(2 * j + (oj[r] != 0.f ? 1 : 0)) * (B + 1) + cj[r]], 1u);
            }
          }
        }
      }
      __syncthreads();
      flush_cols_strided(wgcol, colpart, J * NQ, t0, T, L.tid);
      if (histpart != nullptr) {
#pragma unroll
        for (int s = 0; s < BINS_PER_THREAD; ++s) {
          const int bin = L.tid + 256 * s;
          if (bin < nbin) {
            histacc[s] += (long long)lhist[bin];
            lhist[bin] = 0u;
          }
        }
      }
    }
  }

  if constexpr (SCORE) {
    if (rowpart != nullptr) {
      const int nq = J * NQ;
#pragma unroll
      for (int q = 0; q < MAXJ * NQ; ++q) {
        if (q < nq) {
          const double other = __shfl_xor(rowacc[q], 32, 64);
          if (L.h == 0 && L.rowok) rowpart[((int64_t)blockIdx.y * nq + q) * m + L.row] = rowacc[q] + other;
        }
      }
    }
    if (histpart != nullptr) {
      long long* mine = histpart + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (int64_t)nbin;
#pragma unroll
      for (int s = 0; s < BINS_PER_THREAD; ++s) {
        const int bin = L.tid + 256 * s;
        if (bin < nbin) mine[bin] = histacc[s];
      }
    }
  }
}

// [score workspace of 4 J quantities, all with row sums][histpart: row blocks x T splits x 2 J (B + 1) int64]; the
// score part is a multiple of 16 bytes past its 16-byte boundary (colpart holds 4 J floats per (row block, t))
inline size_t hist_offset(int64_t m, int64_t T, int J) { return score_ws_bytes(m, T, NQ * J, NQ * J); }

template <int JJ>
int reduce_exceed(const ScoreWs& ws, const Plan& p, int64_t m, int64_t T, double* col, int64_t ldcol, int accumulate,
                  double* row, int64_t ldrow, hipStream_t st) {
  return reduce_score<NQ * JJ, NQ * JJ>(ws, p, m, T, NQ * JJ, ColsOf{col, ldcol}, accumulate, row, ldrow, st);
}

// what the two entry points share: the factors, the members and the threshold table
int check_exceed(const float* U, int64_t m, int64_t k, int64_t ldu, const float* C, int64_t ldc, int64_t T, int64_t B,
                 const float* thr, int64_t ldthr, int64_t J, int64_t S, const char* who) {
  DMDX_CHECK_ARG(thr != nullptr, "%s: thr must not be null", who);
  DMDX_CHECK_ARG(B >= 1 && B <= MAXB, "%s: B = %lld outside 1 .. %d", who, (long long)B, MAXB);
  DMDX_CHECK_ARG(J >= 1 && J <= MAXJ, "%s: J = %lld outside 1 .. %d", who, (long long)J, MAXJ);
  DMDX_CHECK_ARG(S >= 1 && S < DIM_LIMIT, "%s: S = %lld must be in 1 .. 2^31 - 1", who, (long long)S);
  if (int rc = check_common(U, m, k, ldu, C, ldc, T, who)) return rc;
  DMDX_CHECK_ARG(B * T < DIM_LIMIT, "%s: B T = %lld x %lld columns of C must be < 2^31", who, (long long)B, (long long)T);
  DMDX_CHECK_ARG(J * S < DIM_LIMIT, "%s: J S = %lld x %lld columns of thr must be < 2^31", who, (long long)J, (long long)S);
  DMDX_CHECK_ARG(ldthr >= m && ldthr < DIM_LIMIT, "%s: ldthr = %lld must be in m = %lld .. 2^31 - 1", who, (long long)ldthr,
                 (long long)m);
  return 0;
}

}  // namespace

extern "C" int dmdx_exceed_max_k(void) { return MAXK; }
extern "C" int dmdx_exceed_max_members(void) { return MAXB; }
extern "C" int dmdx_exceed_max_thresholds(void) { return MAXJ; }

extern "C" int dmdx_exceed_prob_f32(const float* U, int64_t m, int64_t k, int64_t ldu, const float* C, int64_t ldc, int64_t T,
                                    int64_t B, const float* mu, const float* sigma, const float* thr, int64_t ldthr, int64_t J,
                                    int64_t S, const int32_t* slot, int above, float* P, int64_t ldp, int64_t pstride,
                                    void* stream) {
  const char* who = "dmdx_exceed_prob_f32";
  DMDX_CHECK_ARG(U != nullptr && C != nullptr && P != nullptr, "%s: U, C and P must not be null", who);
  if (int rc = check_exceed(U, m, k, ldu, C, ldc, T, B, thr, ldthr, J, S, who)) return rc;
  DMDX_CHECK_ARG(ldp >= m && ldp < DIM_LIMIT, "%s: ldp = %lld must be in m = %lld .. 2^31 - 1", who, (long long)ldp, (long long)m);
  DMDX_CHECK_ARG(J == 1 || pstride >= (T - 1) * ldp + m, "%s: pstride = %lld, the planes of %lld x %lld with ldp = %lld overlap",
                 who, (long long)pstride, (long long)m, (long long)T, (long long)ldp);
  const Plan p = plan_for(m, T);
  const int cvec = cvec_of(C, ldc);
  const unsigned sgn = above ? 0u : 0x80000000u;
#define DMDX_LAUNCH(KG)                                                                                                  \
  hipLaunchKernelGGL((exceed_kernel<KG, false>), p.grid(), dim3(256), 0, (hipStream_t)stream, U, m, (int)k, ldu, C, ldc, T,   \
                     (int)B, mu, sigma, thr, ldthr, (int)J, S, slot, sgn, (const float*)nullptr, (int64_t)0,                  \
                     (const float*)nullptr, p.tiles_per_wg, p.ntiles, cvec, P, ldp, pstride, (float*)nullptr,                \
                     (double*)nullptr, (long long*)nullptr)
  DMDX_DISPATCH_KG(k, who, DMDX_LAUNCH)
#undef DMDX_LAUNCH
  DMDX_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t dmdx_exceed_score_workspace_bytes(int64_t m, int64_t k, int64_t T, int64_t B, int64_t J) {
  (void)k;
  if (m < 1 || T < 1 || m >= DIM_LIMIT || T >= DIM_LIMIT || B < 1 || B > MAXB || J < 1 || J > MAXJ) return 16;
  const Plan p = plan_for(m, T);
  return hist_offset(m, T, (int)J) + (size_t)p.nrb * (size_t)p.nsplit * (size_t)(2 * J * (B + 1)) * sizeof(long long);
}

extern "C" int dmdx_exceed_score_f32(const float* U, int64_t m, int64_t k, int64_t ldu, const float* C, int64_t ldc, int64_t T,
                                     int64_t B, const float* mu, const float* sigma, const float* thr, int64_t ldthr, int64_t J,
                                     int64_t S, const int32_t* slot, int above, const float* X, int64_t ldx, const float* w,
                                     double* col, int64_t ldcol, double* row, int64_t ldrow, int64_t* cnt, int accumulate,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "dmdx_exceed_score_f32";
  DMDX_CHECK_ARG(U != nullptr && C != nullptr && X != nullptr && col != nullptr, "%s: U, C, X and col must not be null", who);
  if (int rc = check_exceed(U, m, k, ldu, C, ldc, T, B, thr, ldthr, J, S, who)) return rc;
  if (int rc = check_score_lds(m, T, ldx, ldcol, row, ldrow, who)) return rc;
  if (int rc = check_workspace(workspace, workspace_bytes, dmdx_exceed_score_workspace_bytes(m, k, T, B, J), who)) return rc;
  const Plan p = plan_for(m, T);
  hipStream_t st = (hipStream_t)stream;
  const ScoreWs ws = score_ws(workspace, p, m, NQ * (int)J);
  char* base = reinterpret_cast<char*>(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
  long long* histpart = cnt != nullptr ? reinterpret_cast<long long*>(base + hist_offset(m, T, (int)J) - 16) : nullptr;
  const int cvec = cvec_of(C, ldc);
  const unsigned sgn = above ? 0u : 0x80000000u;
  double* rowpart = row != nullptr ? ws.rowpart : nullptr;
#define DMDX_LAUNCH(KG)                                                                                                  \
  hipLaunchKernelGGL((exceed_kernel<KG, true>), p.grid(), dim3(256), 0, st, U, m, (int)k, ldu, C, ldc, T, (int)B, mu, sigma,  \
                     thr, ldthr, (int)J, S, slot, sgn, X, ldx, w, p.tiles_per_wg, p.ntiles, cvec, (float*)nullptr,            \
                     (int64_t)0, (int64_t)0, ws.colpart, rowpart, histpart)
  DMDX_DISPATCH_KG(k, who, DMDX_LAUNCH)
#undef DMDX_LAUNCH
  DMDX_LAUNCH_CHECK();
  int rc = 0;
  switch (J) {
    case 1: rc = reduce_exceed<1>(ws, p, m, T, col, ldcol, accumulate, row, ldrow, st); break;
    case 2: rc = reduce_exceed<2>(ws, p, m, T, col, ldcol, accumulate, row, ldrow, st); break;
    case 3: rc = reduce_exceed<3>(ws, p, m, T, col, ldcol, accumulate, row, ldrow, st); break;
    default: rc = reduce_exceed<4>(ws, p, m, T, col, ldcol, accumulate, row, ldrow, st); break;
  }
  if (rc) return rc;
  if (cnt != nullptr) {
    const int nbin = (int)(2 * J * (B + 1));
    hipLaunchKernelGGL(reduce_hist_kernel, dim3((unsigned)nbin), dim3(256), 0, st, histpart, p.nrb * p.nsplit, nbin,
                       reinterpret_cast<long long*>(cnt), accumulate);
    DMDX_LAUNCH_CHECK();
  }
  return 0;
}
