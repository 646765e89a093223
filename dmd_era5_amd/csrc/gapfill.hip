// K31: the three kernels of DINEOF gap filling (dmd_era5_amd/gapfill.py) -- which elements of a row block are gaps, the
// block standardised with zeros at the gaps, and the rank-k field mu + sigma (U C) stored at the gaps ALONE.
//
// The mask is one bit per element, packed along time: W[tw ldw + i] bit b <=> element (i, 32 tw + b) is a gap.  The word
// width is the tile width of expand_tile.h (TT = 32 snapshots), so a wave of the fill reads the 32 words of its 32 rows
// in a tile with one coalesced 128-byte load, and the lane that owns row i holds in ONE register the bits of its own 16
// accumulator registers (bit col_of(r, h)).  Packed along the rows instead, a lane would need the words of 16 snapshots.
//
//   mask          one read of X in the row-lane frame of time_rows.h: a lane owns R rows, walks time in segments of
//                 kSeg = 1024 snapshots (32 words) and forms, per row, the words, the count of gaps and the fp64 sum and
//                 sum of squares of the finite values.  A segment is one fp64 chain in ascending t from +0.0, the segment
//                 sums are added in ascending order (K21 / K26).  With a workspace the segments are spread over grid.y
//                 and a combine kernel adds their partials in order; without one a lane walks them: the same bits.
//   standardize   in place, one read and one write, the same lanes: a workgroup row (grid.y) is one word of time.
//   fill          one more body on K12's tile (expand_tile.h): the panel of U in registers, C through LDS, one MFMA chain
//                 per tile, affine() -- and then a store only where the lane's word has a bit.  old is loaded only there.
//                 A wave whose 32 words of a tile are all zero skips the chain and the epilogue of that tile (it still
//                 meets the tile's barrier); a workgroup whose words are zero over its whole tile range writes its zero
//                 row partials and returns before it loads its panel.  change_row = sum_t bit (new - old)^2: fp32 over the
//                 16 values of a lane in a tile, fp64 over tiles and T splits (rowpart, reduce_rows_kernel), no atomics.
//
// "Gap" is K20's test of the bit pattern: exponent all ones.  Contraction is off for the whole file: the roundings of
// standardize and of (new - old)^2 are part of the contract.
#include "expand_tile.h"
#include "time_rows.h"

#pragma clang fp contract(off)

namespace {

constexpr int kSeg = 1024;                   // snapshots of one fp64 chain: 32 words
constexpr int kLoads = 8;                    // snapshot loads of a lane in flight
static_assert(TT == 32 && kSeg % TT == 0, "a word of the mask is one tile of K12 wide, a segment whole words");

__device__ __forceinline__ uint32_t gap_bit(float x) { return finite_bits(x) ? 0u : 1u; }

// ---------------------------------------------------------------- mask
// Workspace of the split form: [nseg][2][m] fp64 partial sums, then [nseg][m] int32 partial counts.
struct MaskWs {
  double* sums;
  int32_t* cnt;
};
inline size_t mask_ws_bytes(int64_t m, int64_t T) {
  return saturating_bytes((T + kSeg - 1) / kSeg, m, 2 * sizeof(double) + sizeof(int32_t), 1);
}
inline MaskWs mask_ws(void* workspace, int64_t m, int64_t nseg) {
  return {(double*)workspace, (int32_t*)((char*)workspace + (size_t)nseg * 2 * (size_t)m * sizeof(double))};
}

// One lane: rows r0 .. r0 + nr - 1.  Segments s = blockIdx.y, blockIdx.y + gridDim.y, ...
template <int R, bool FULL, bool SPLIT>
__device__ __forceinline__ void mask_rows(const float* __restrict__ xp, int nr, int64_t m, int64_t T, int64_t ldx,
                                          uint32_t* __restrict__ wp, int64_t ldw, int64_t nseg, double* __restrict__ wsum,
                                          int32_t* __restrict__ wcnt, int32_t* __restrict__ nmiss,
                                          double* __restrict__ sums, int64_t ldsum) {
  typedef typename VecOf<R>::type vec;
  double tot1[R], tot2[R];
  int32_t totc[R];
#pragma unroll
  for (int e = 0; e < R; ++e) tot1[e] = tot2[e] = 0.0, totc[e] = 0;

  for (int64_t s = blockIdx.y; s < nseg; s += gridDim.y) {
    const int64_t a = s * kSeg;
    const int64_t b = T - a < kSeg ? T : a + kSeg;
    double acc1[R], acc2[R];
    int32_t cnt[R];
#pragma unroll
    for (int e = 0; e < R; ++e) acc1[e] = acc2[e] = 0.0, cnt[e] = 0;

    for (int64_t t0 = a; t0 < b; t0 += TT) {
      uint32_t word[R];
#pragma unroll
      for (int e = 0; e < R; ++e) word[e] = 0u;
      // snapshot t0 + j: its bit, and its value (a gap: +0.0, which leaves a chain that is never -0.0 as it is)
      auto take = [&](int j, vec v) {
#pragma unroll
        for (int e = 0; e < R; ++e) {
          const uint32_t g = gap_bit(v[e]);
          word[e] |= g << j;
          const double d = g ? 0.0 : (double)v[e];
          const double q = d * d;
          acc1[e] = acc1[e] + d;
          acc2[e] = acc2[e] + q;
        }
      };
      const float* px = xp + t0 * ldx;
      if (b - t0 >= TT) {
#pragma unroll
        for (int j0 = 0; j0 < TT; j0 += kLoads) {
          vec v[kLoads];
#pragma unroll
          for (int u = 0; u < kLoads; ++u) v[u] = ld_rows<R, FULL>(px + (j0 + u) * ldx, nr);
#pragma unroll
          for (int u = 0; u < kLoads; ++u) take(j0 + u, v[u]);
        }
      } else {
        const int nb = (int)(b - t0);                            // the ragged last word: the bits from T on stay 0
        for (int j = 0; j < nb; ++j) take(j, ld_rows<R, FULL>(px + j * ldx, nr));
      }
#pragma unroll
      for (int e = 0; e < R; ++e) {
        if (e < nr) wp[(t0 / TT) * ldw + e] = word[e];
        cnt[e] += __popc(word[e]);
      }
    }

    if (SPLIT) {
#pragma unroll
      for (int e = 0; e < R; ++e)
        if (e < nr) {
          wsum[(s * 2 + 0) * m + e] = acc1[e];
          wsum[(s * 2 + 1) * m + e] = acc2[e];
          wcnt[s * m + e] = cnt[e];
        }
    } else {
#pragma unroll
      for (int e = 0; e < R; ++e) {
        tot1[e] = tot1[e] + acc1[e];
        tot2[e] = tot2[e] + acc2[e];
        totc[e] += cnt[e];
      }
    }
  }
  if (!SPLIT) {
#pragma unroll
    for (int e = 0; e < R; ++e)
      if (e < nr) {
        if (nmiss) nmiss[e] = totc[e];
        if (sums) {
          sums[e] = tot1[e];
          sums[ldsum + e] = tot2[e];
        }
      }
  }
}

template <int R, bool SPLIT>
__global__ __launch_bounds__(256) void gap_mask_kernel(const float* __restrict__ X, int64_t m, int64_t T, int64_t ldx,
                                                       uint32_t* __restrict__ W, int64_t ldw, int64_t nseg,
                                                       double* __restrict__ wsum, int32_t* __restrict__ wcnt,
                                                       int32_t* __restrict__ nmiss, double* __restrict__ sums,
                                                       int64_t ldsum) {
  const int64_t r0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * R;
  if (r0 >= m) return;
  const int nr = (m - r0) < R ? (int)(m - r0) : R;
  double* ws = SPLIT ? wsum + r0 : nullptr;
  int32_t* wc = SPLIT ? wcnt + r0 : nullptr;
  int32_t* nm = (!SPLIT && nmiss) ? nmiss + r0 : nullptr;
  double* sm = (!SPLIT && sums) ? sums + r0 : nullptr;
  if (nr == R)
    mask_rows<R, true, SPLIT>(X + r0, nr, m, T, ldx, W + r0, ldw, nseg, ws, wc, nm, sm, ldsum);
  else
    mask_rows<R, false, SPLIT>(X + r0, nr, m, T, ldx, W + r0, ldw, nseg, ws, wc, nm, sm, ldsum);
}

// The tail of the split form: one lane per row adds the segment partials in ascending order, from +0.0.
__global__ __launch_bounds__(256) void gap_mask_combine_kernel(const double* __restrict__ wsum,
                                                               const int32_t* __restrict__ wcnt, int64_t m, int64_t nseg,
                                                               int32_t* __restrict__ nmiss, double* __restrict__ sums,
                                                               int64_t ldsum) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  double t1 = 0.0, t2 = 0.0;
  int32_t c = 0;
  for (int64_t s = 0; s < nseg; ++s) {
    t1 = t1 + wsum[(s * 2 + 0) * m + i];
    t2 = t2 + wsum[(s * 2 + 1) * m + i];
    c += wcnt[s * m + i];
  }
  if (nmiss) nmiss[i] = c;
  if (sums) {
    sums[i] = t1;
    sums[ldsum + i] = t2;
  }
}

struct MaskScan {
  template <int R, bool SPLIT> static constexpr auto kernel() { return gap_mask_kernel<R, SPLIT>; }
};

// ---------------------------------------------------------------- standardize
// A lane owns R rows; a workgroup row (blockIdx.y, strided) is one word of time.  BACK: x sigma + mu, W not looked at.
template <int R, bool BACK>
__global__ __launch_bounds__(256) void gap_standardize_kernel(float* __restrict__ X, int64_t m, int64_t T, int64_t ldx,
                                                              const uint32_t* __restrict__ W, int64_t ldw,
                                                              const float* __restrict__ mu,
                                                              const float* __restrict__ sigma) {
  typedef typename VecOf<R>::type vec;
  const int64_t r0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * R;
  if (r0 >= m) return;
  const int nr = (m - r0) < R ? (int)(m - r0) : R;
  const bool full = nr == R;
  float mu_e[R], sg_e[R];
#pragma unroll
  for (int e = 0; e < R; ++e) {
    mu_e[e] = (mu != nullptr && e < nr) ? mu[r0 + e] : 0.f;
    sg_e[e] = (sigma != nullptr && e < nr) ? sigma[r0 + e] : 1.f;
  }
  const int64_t nw = (T + TT - 1) / TT;
  for (int64_t tw = blockIdx.y; tw < nw; tw += gridDim.y) {
    uint32_t word[R];
#pragma unroll
    for (int e = 0; e < R; ++e) word[e] = (!BACK && W != nullptr && e < nr) ? W[tw * ldw + r0 + e] : 0u;
    const int64_t t0 = tw * TT;
    const int nb = T - t0 < TT ? (int)(T - t0) : TT;
    float* px = X + t0 * ldx + r0;
    for (int j0 = 0; j0 < nb; j0 += kLoads) {
      vec v[kLoads];
#pragma unroll
      for (int u = 0; u < kLoads; ++u)
        if (j0 + u < nb) v[u] = full ? ld_rows<R, true>(px + (j0 + u) * ldx, nr) : ld_rows<R, false>(px + (j0 + u) * ldx, nr);
#pragma unroll
      for (int u = 0; u < kLoads; ++u) {
        if (j0 + u >= nb) continue;
        vec o;
#pragma unroll
        for (int e = 0; e < R; ++e) {
          if (BACK) {
            const float p = v[u][e] * sg_e[e];
            o[e] = p + mu_e[e];
          } else {
            const float d = v[u][e] - mu_e[e];
            o[e] = ((word[e] >> (j0 + u)) & 1u) ? 0.f : d / sg_e[e];
          }
        }
        float* q = px + (j0 + u) * ldx;
        if (full) {
          *reinterpret_cast<vec*>(q) = o;
        } else {
#pragma unroll
          for (int e = 0; e < R; ++e)
            if (e < nr) q[e] = o[e];
        }
      }
    }
  }
}

// ---------------------------------------------------------------- fill
// expand_kernel<KG, false> of expand.hip with the lane's word of the tile between the chain and the store.  rowpart
// (null: change_row is not asked for, old is not loaded): [T split][m] fp64.
template <int KG>
__global__ __launch_bounds__(256, 2) void gap_fill_kernel(const float* __restrict__ U, int64_t m, int k, int64_t ldu,
                                                          const float* __restrict__ C, int64_t ldc, int64_t T,
                                                          const float* __restrict__ mu, const float* __restrict__ sigma,
                                                          const uint32_t* __restrict__ W, int64_t ldw,
                                                          float* __restrict__ X, int64_t ldx, int64_t tiles_per_wg,
                                                          int64_t ntiles, int cvec, double* __restrict__ rowpart) {
  __shared__ __attribute__((aligned(16))) float ctile[2][Geom<KG>::STAGE];

  const Lane L = lane_of(m);
  const int64_t tile0 = (int64_t)blockIdx.y * tiles_per_wg;
  const int64_t tile1 = tile0 + tiles_per_wg < ntiles ? tile0 + tiles_per_wg : ntiles;
  // the word of tile `tile` of this lane's row: the bits of snapshots >= T are the caller's and are dropped
  auto word_of = [&](int64_t tile) -> uint32_t {
    if (!L.rowok) return 0u;
    const uint32_t w = W[tile * ldw + L.row];
    const int64_t left = T - tile * TT;
    return left >= TT ? w : (w & ((1u << (int)left) - 1u));
  };

  // nothing to fill in this workgroup's rows and tiles: its row partials are +0.0, the panel is never loaded
  uint32_t any = 0u;
  for (int64_t tile = tile0; tile < tile1; ++tile) any |= word_of(tile);
  if (!__syncthreads_or((int)(any != 0u))) {
    if (rowpart != nullptr && L.h == 0 && L.rowok) rowpart[(int64_t)blockIdx.y * m + L.row] = 0.0;
    return;
  }

  float ureg[8 * KG];
  load_panel<KG>(ureg, U, ldu, k, L);
  const float mu_i = (mu != nullptr && L.rowok) ? mu[L.row] : 0.f;
  const float sg_i = (sigma != nullptr && L.rowok) ? sigma[L.row] : 1.f;
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
    const uint32_t word = word_of(tile);

    if (__ballot(word != 0u) != 0ull) {                          // (wave-uniform: the MFMAs run with all lanes)
      const f32x16 acc = mfma_chain<KG>(ctile[cur], ureg, L);
      float rs = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = col_of(r, L.h);
        const float v = affine(acc[r], sigma != nullptr, sg_i, mu != nullptr, mu_i);
        float d2 = 0.f;
        if ((word >> c) & 1u) {                                  // (a set bit: row < m and t0 + c < T)
          float* q = X + (t0 + c) * ldx + L.row;
          if (rowpart != nullptr) {
            const float d = v - *q;
            d2 = d * d;
          }
          *q = v;
        }
        rs += d2;
      }
      rowacc[0] += (double)rs;
    }

    if (has_next) cs.store(ctile[cur ^ 1], L.tid);
    __syncthreads();
    cur ^= 1;
  }
  if (rowpart != nullptr) store_row_sums<1>(rowacc, rowpart, m, L);
}

}  // namespace

extern "C" int dmdx_gap_mask_segment(void) { return kSeg; }

extern "C" size_t dmdx_gap_mask_workspace_bytes(int64_t m, int64_t T) {
  if (m < 0 || T < 0 || m >= kMaxSize || T >= kMaxSize) return 0;
  return mask_ws_bytes(m, T);
}

extern "C" int dmdx_gap_mask_f32(const float* X, int64_t m, int64_t T, int64_t ldx, uint32_t* W, int64_t ldw,
                                 int32_t* nmiss, double* sums, int64_t ldsum, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  const char* who = "dmdx_gap_mask_f32";
  if (int rc = check_block(who, m, T, {{"ldx", ldx}, {"ldw", ldw}, {"ldsum", sums ? ldsum : m}}, {X, W, nmiss},
                           {sums, workspace}))
    return rc;
  if (m == 0 || T == 0) return 0;
  DMDX_CHECK_ARG(X && W, "%s: null X or W", who);
  if (workspace != nullptr && workspace_bytes < mask_ws_bytes(m, T)) {
    dmdx_set_error("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, mask_ws_bytes(m, T));
    return DMDX_E_WORKSPACE;
  }
  const int64_t nseg = (T + kSeg - 1) / kSeg;
  hipStream_t st = (hipStream_t)stream;
  const bool split = workspace != nullptr;
  const MaskWs ws = split ? mask_ws(workspace, m, nseg) : MaskWs{nullptr, nullptr};
  const RowLanes ln = row_lanes(X, ldx, m, nseg, split);
  launch_lanes<MaskScan>(ln, split, st, X, m, T, ldx, W, ldw, nseg, ws.sums, ws.cnt, nmiss, sums, ldsum);
  DMDX_LAUNCH_CHECK();
  if (split && (nmiss != nullptr || sums != nullptr)) {
    hipLaunchKernelGGL(gap_mask_combine_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, ws.sums, ws.cnt, m,
                       nseg, nmiss, sums, ldsum);
    DMDX_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int dmdx_gap_standardize_f32(float* X, int64_t m, int64_t T, int64_t ldx, const uint32_t* W, int64_t ldw,
                                        const float* mu, const float* sigma, int back, void* stream) {
  const char* who = "dmdx_gap_standardize_f32";
  const bool masked = !back && W != nullptr;
  if (int rc = check_block(who, m, T, {{"ldx", ldx}, {"ldw", masked ? ldw : m}}, {X, W, mu, sigma})) return rc;
  if (m == 0 || T == 0) return 0;
  DMDX_CHECK_ARG(X, "%s: null X", who);
  hipStream_t st = (hipStream_t)stream;
  const RowLanes ln = row_lanes(X, ldx, m, (T + TT - 1) / TT, true);
  const dim3 grid(ln.gx, ln.gy), block(256);
  if (ln.quad && back)
    hipLaunchKernelGGL((gap_standardize_kernel<4, true>), grid, block, 0, st, X, m, T, ldx, W, ldw, mu, sigma);
  else if (ln.quad)
    hipLaunchKernelGGL((gap_standardize_kernel<4, false>), grid, block, 0, st, X, m, T, ldx, W, ldw, mu, sigma);
  else if (back)
    hipLaunchKernelGGL((gap_standardize_kernel<1, true>), grid, block, 0, st, X, m, T, ldx, W, ldw, mu, sigma);
  else
    hipLaunchKernelGGL((gap_standardize_kernel<1, false>), grid, block, 0, st, X, m, T, ldx, W, ldw, mu, sigma);
  DMDX_LAUNCH_CHECK();
  return 0;
}

extern "C" int dmdx_gap_fill_max_k(void) { return MAXK; }

extern "C" size_t dmdx_gap_fill_workspace_bytes(int64_t m, int64_t k, int64_t T) {
  (void)k;
  if (m < 1 || T < 1 || m >= DIM_LIMIT || T >= DIM_LIMIT) return 16;
  return score_ws_bytes(m, T, 0, 1);
}

extern "C" int dmdx_gap_fill_f32(const float* U, int64_t m, int64_t k, int64_t ldu, const float* C, int64_t ldc, int64_t T,
                                 const float* mu, const float* sigma, const uint32_t* W, int64_t ldw, float* X, int64_t ldx,
                                 double* change_row, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "dmdx_gap_fill_f32";
  if (int rc = check_block(who, m, T, {{"ldu", ldu}, {"ldw", ldw}, {"ldx", ldx}}, {U, C, mu, sigma, W, X}, {change_row}))
    return rc;
  DMDX_CHECK_ARG(k >= 1 && k <= MAXK, "%s: k = %lld outside 1 .. %d", who, (long long)k, MAXK);
  DMDX_CHECK_ARG(ldc >= k && ldc < DIM_LIMIT, "%s: ldc = %lld must be in k = %lld .. 2^31 - 1", who, (long long)ldc,
                 (long long)k);
  if (m == 0 || T == 0) return 0;
  DMDX_CHECK_ARG(U && C && W && X, "%s: U, C, W and X must not be null", who);
  const Plan p = plan_for(m, T);
  double* rowpart = nullptr;
  if (change_row != nullptr) {
    if (int rc = check_workspace(workspace, workspace_bytes, dmdx_gap_fill_workspace_bytes(m, k, T), who)) return rc;
    rowpart = score_ws(workspace, p, m, 1).rowpart;
  }
  hipStream_t st = (hipStream_t)stream;
  const int cvec = cvec_of(C, ldc);
#define DMDX_LAUNCH(KG)                                                                                                  \
  hipLaunchKernelGGL((gap_fill_kernel<KG>), p.grid(), dim3(256), 0, st, U, m, (int)k, ldu, C, ldc, T, mu, sigma, W, ldw, \
                     X, ldx, p.tiles_per_wg, p.ntiles, cvec, rowpart)
  DMDX_DISPATCH_KG(k, who, DMDX_LAUNCH)
#undef DMDX_LAUNCH
  DMDX_LAUNCH_CHECK();
  if (change_row != nullptr) {
    hipLaunchKernelGGL(reduce_rows_kernel<1>, dim3((unsigned)((m + 255) / 256), 1), dim3(256), 0, st, rowpart, p.nsplit, m,
                       change_row, m);
    DMDX_LAUNCH_CHECK();
  }
  return 0;
}
