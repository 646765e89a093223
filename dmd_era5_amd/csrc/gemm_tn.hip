// K1 / K3: D = OpA^T OpB for K-contiguous (column-major, tall) operands, on the
// fp32-input MFMA (v_mfma_f32_32x32x2_f32).  K1 (Gram, G = X^T X) is the SYRK
// mode: OpA = OpB = X and only the tiles of one triangle are computed.
//
// Decomposition
//   work unit = (K-split s, 128x128 output tile t); one 256-thread workgroup
//   (4 waves, 2x2, each wave a 64x64 sub-tile = 2x2 MFMA blocks of 32x32) per
//   unit, two workgroups resident per CU.
//   K loop: 32-row chunks through two LDS stages.  Aligned operands are staged by
//   LDS-DMA (global_load_lds_dwordx4 along K, the contiguous axis of both
//   operands; SGPR base + 32-bit per-lane byte offset, no VALU per piece); the LDS
//   panels are unpadded [column][32 k] with the 16-byte k-chunks XOR-swizzled by
//   (column >> 1) & 7 on the DMA source and on the fragment reads, which makes the
//   ds_read_b128 fragment reads bank-conflict free.  Unaligned operands and the
//   K tail go through registers.  One ds_read_b128 per operand block feeds four
//   MFMAs: lane (r, h) reads k = 8t+4h .. 8t+4h+3 of its column, MFMA j uses
//   element j of both operands -- the same k permutation on both sides, so
//   the contraction is unchanged.
//   Numerics: fp32 MFMA chains of at most 128 chunks * 32 = 4096 rows; the chain
//   results of a unit (at most 16) are summed in a second fp32 register
//   accumulator (blocked summation: the error bound stays that of a 4096-row
//   chain) and stored once, as fp64, into the unit's own partial tile (no
//   atomics => deterministic); a second kernel sums the K-splits in fp64 and
//   writes D (both triangles in SYRK mode).  Row blocks are accumulated into D
//   in fp64 (`accumulate`).
//   K1's full 128 x 128 SYRK tiles (n > 96) run the same products on the bf16 matrix core instead (tn_unit with
//   PL = 1, bf16_split.h): every fp32 value is split exactly into three bf16 planes h + m + l and six of the nine
//   plane products (h h, h m, m h, h l, m m, l h) go as v_mfma_f32_32x32x16_bf16 into the same accumulator -- 24
//   MFMAs of 8 passes per 16 k and wave instead of 32 of 16 passes.  The three dropped products stay below
//   2^-21 |a b| per pair, about 2^-23 sum |a b| over a sum.  The bf16 MFMA truncates its sum a few bits below the
//   fp32 ulp of its accumulator (one-signed: it shows on the diagonal of a Gram), so this body keeps its MFMA chains to
//   ONE chunk of 32 rows and adds every chunk result into the second accumulator with rounded fp32 adds: at most
//   2048 of them per unit, the same order as the 4096-row chain bound.  Inf / NaN keep numpy's classes, and finite
//   data pays nothing for it in the loop: every unit runs on the fast planes, whose l plane is NaN for every Inf and
//   NaN, so that each output such a value feeds is NaN at the end of the unit; one NaN test on the unit's result, a
//   workgroup-wide verdict, and a unit that raised the alarm runs once more from its first chunk on the class-safe
//   planes (the class rule of bf16_split.h on every group) before anything is committed.  A unit with a non-finite
//   value in its K-range of its 256 columns therefore costs twice; the rule assumes normal fp32 partners: Inf times
//   a subnormal below 2^-133 gives NaN, not Inf.  Planes of values below ~2^-103 turn
//   subnormal and lose bits; the host's magnitude guard rescales such data before it gets here.  K3, K3s, the 32- to
//   112-row tiles and the small-n Gram stay on the fp32 MFMA; DMDX_K1_ARITH=f32 keeps K1 there too.
//
//   Chunk pipeline: both stages filled up front; chunk c runs k-steps 0..2, then the
//   barrier, then k-step 3 (its fragments are already in registers), the refill of the
//   freed stage with chunk c+2 and the first fragment reads of chunk c+1.
//
// L2 locality: units are ordered tile-fastest inside a K-split, the tiles of
// the triangle are enumerated in 8-row super-rows, column by column, so 64
// consecutive units form an 8x8 patch of tiles; blockIdx is remapped so that
// the 64 blocks of a group of 512 that land on one XCD (blockIdx % 8 equal)
// take one patch (xcd_unit).
//
// Entry points: dmdx_syrk_blocks_f32 / dmdx_gemm_tn_blocks_f32 (the sum over up to 16 row blocks per
// launch) and dmdx_syrk_f32 / dmdx_gemm_tn_f32 (one pair of operands: a batch of one block).  One
// path for all four: tn_refusal, run_batch, syrk_batch_kernel (body tn_unit), and the reduce kernel
// that sums the K-splits; dmdx_gemm_tn_blocks_f32 alone also takes the small-l kernel (K3s).
// dmdx_syrk_blocks_planes_f32 is dmdx_syrk_blocks_f32 with the bf16 planes of K1's full tiles made once per call
// (plane_split.hip) and streamed by the fast pass (tn_unit_planes, PL = 2; the units it marks run again as PL = 3).
// Environment knobs (tuning / A-B only, no result changes beyond rounding): DMDX_TN_MAX_CPS (chunks
// per unit, default 2048), DMDX_TN_ROUNDS (rounds of 512 workgroups the K-splits aim at),
// DMDX_TN_FORCE_TM, DMDX_TN_NO_TAILFIT, DMDX_NO_K3S, DMDX_K3S_32, DMDX_K1_ARITH (f32: K1 on the fp32 MFMA).  The timing-only ablations of
// tn_unit (results are wrong) are a compile-time macro of the diagnostic build, DMDX_TN_ABL
// (`make stamps ABL=2`): the product library has no such switch.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "bf16_split.h"
#include "dmdx_common.h"
#include "plane_image.h"

thread_local unsigned long long* dmdx_clock_probe_ptr = nullptr;  // dmdx_set_clock_probe (measurement aid)

int dmdx_device_cus() {
  static int cached[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return -1;
  if (cached[dev] == 0) {
    int v = 0;
    cached[dev] = (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) ? v : -1;
  }
  return cached[dev];
}

namespace {

constexpr int BT = 128;            // output tile edge
constexpr int BK = 32;             // K rows per stage
constexpr int FOLD = 128;          // chunks per fp32 chain (128 * 32 = 4096 rows) before it is folded into acc2
constexpr int NTH = 256;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct TnParams {
  const float* A;   // MFMA "A" operand source: D rows
  const float* B;   // MFMA "B" operand source: D cols (fast index of D)
  int64_t lda, ldb;
  int64_t K;
  int nrow, ncol;   // D is nrow x ncol (nrow = cols of A, ncol = cols of B)
  int ntr, ntc;     // tiles along rows / cols
  int ntiles;
  int syrk;
  int nsplit;
  int chunks_total;
  int chunks_per_split;
  double* P;        // [slab][ntiles][tile rows x 128] fp64 partial tiles; slab = K-split (of a block)
};

// A batch of row blocks in one launch: the Gram of a row-blocked snapshot matrix (and X^T Y) is
// the sum over its blocks, and one launch per block leaves the GPU draining / refilling 8 times
// (last partial round of units, reduce kernel, launch gap: ~1.5 % at cfg2).  Block j owns the
// grid range [unit_begin[j], unit_begin[j+1]) (padded to multiples of 512 so that the XCD
// patch mapping stays aligned; padding blocks exit at once) and the partial-tile slabs
// [slab_begin[j], slab_begin[j+1]); the reduce kernel sums all slabs.
constexpr int MAXB = 16;
struct TnBatch {
  const float* A[MAXB];   // D rows <- columns of A_j; SYRK: A_j == B_j == X_j
  const float* B[MAXB];   // D cols <- columns of B_j
  int64_t lda[MAXB];
  int64_t ldb[MAXB];
  int64_t K[MAXB];
  int chunks_total[MAXB];
  int chunks_per_split[MAXB];
  int nsplit[MAXB];
  int unit_begin[MAXB + 1];
  int slab_begin[MAXB + 1];
  int nblocks;
  const unsigned char* planes[MAXB];   // PL = 2 only: the first plane image of block j (plane_image.h)
  // measurement aid (dmdx_set_clock_probe; null on the product path): every workgroup adds the
  // core-clock cycles and the 100 MHz reference ticks of its lifetime and 1 to clk[0..2]
  unsigned long long* clk;
};

// upper-triangle tile enumeration: super-rows of SR tile rows, column-major
// inside a super-row (see header comment).
constexpr int SR = 8;  // tile rows per super-row: 64 consecutive tiles ~ an 8x8 patch
__device__ __host__ inline void decode_tri(int t, int nt, int& ta, int& tb) {
  int r0 = 0;
  for (;;) {
    int nrows = nt - r0 < SR ? nt - r0 : SR;
    int ncols = nt - r0;
    int cnt = nrows * (nrows + 1) / 2 + (ncols - nrows) * nrows;
    if (t < cnt) break;
    t -= cnt;
    r0 += SR;
  }
  int nrows = nt - r0 < SR ? nt - r0 : SR;
  int head = nrows * (nrows + 1) / 2;
  if (t < head) {
    int c = 0;
    while (t >= c + 1) { t -= c + 1; ++c; }
    tb = r0 + c;
    ta = r0 + t;
  } else {
    t -= head;
    tb = r0 + nrows + t / nrows;
    ta = r0 + t % nrows;
  }
}

__device__ inline void decode_tile(int syrk, int ntr, int ntc, int t, int& ta, int& tb) {
  if (syrk) {
    decode_tri(t, ntr, ta, tb);
  } else {  // SR-row super-rows, column-major inside (same patch idea)
    int per_sr = SR * ntc;
    int sr = t / per_sr;
    int r0 = sr * SR;
    int nrows = ntr - r0 < SR ? ntr - r0 : SR;
    int tt = t - sr * per_sr;
    tb = tt / nrows;
    ta = r0 + tt % nrows;
  }
}

// LDS image of one operand stage: [128 columns][32 k] floats, 128 B per column and NOT
// padded (an LDS-DMA wave-instruction writes 1 KiB linearly = 8 columns).  Bank
// conflicts of the ds_read_b128 fragment reads are removed by an XOR swizzle of the
// 16-byte k-chunk index with f(col) = (col >> 1) & 7, applied on the SOURCE address of
// the DMA (and on the register-staged tail path) and on the read address.
__device__ __forceinline__ int swz(int col) { return (col >> 1) & 7; }

// K tail (last chunk of the last split only): rows >= kend read as zero
__device__ inline f32x4 load4_tail(const float* p, int64_t k, int64_t kend) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (k + e < kend) v[e] = p[e];
  return v;
}

#ifdef DMDX_STAMPS
// diagnostic build only (make stamps): per-segment cycle totals of the chunk loop, summed over
// all waves: [0] DMA issue, [1] fragment reads + MFMA issue, [5] wait for the LDS-DMA (vmcnt),
// [2] barrier, [3] post-barrier (first fragment read, fold), [4] chunks counted,
// [6] / [7] chunk-loop time in core cycles / in 100 MHz ticks (their ratio = sustained clock)
__device__ unsigned long long dmdx_stamp[12];   // [8] unit prologue, [9] partial-tile commit (stores drained), [10] waves counted
#define DMDX_STAMP(var)                                                        \
  do {                                                                         \
    __builtin_amdgcn_sched_barrier(0);                                         \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(var)::"memory"); \
    __builtin_amdgcn_sched_barrier(0);                                         \
  } while (0)
#else
#define DMDX_STAMP(var) do { } while (0)
#endif

// The lane's index, derived where it is asked for (two VALU instructions) and not carried in a register from
// the kernel's entry: the plane k-step of tn_unit has none to spare across its chunk loop.
__device__ __forceinline__ int lane_now() {
  unsigned z = 0u;
  asm volatile("" : "+v"(z));   // (not hoisted out of a loop, not merged with an earlier one)
  return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, z));
}

#define DMDX_LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))
#define DMDX_GLB_PTR(p) ((const __attribute__((address_space(1))) void*)(p))

// DMA = true : global -> LDS by global_load_lds_dwordx4 (needs 16-byte aligned
//              bases and leading dimensions); the K-tail chunk goes through registers.
// DMA = false: everything register-staged with scalar loads (any alignment).
// ABL: timing-only ablations for diagnosis (results are wrong when ABL != 0):
//   1 no global->LDS staging, 2 no barrier, 8 no chain fold (none of them changes an address), or their sum.  Set for
//   every unit of a diagnostic build by the macro DMDX_TN_ABL (`make stamps ABL=2`); the product is built with 0.
// SK ("skinny rows", 0 / 1 / 2 / 3): a (32 SK) x 128 output tile, the four waves side by side (each
//   32 SK rows x 32 columns = SK x 1 MFMA blocks) -- for D with few rows (Z = X^T Y with l <= 32,
//   <= 64 or <= 96 columns of Y): a quarter / half / three quarters of the MFMA work of a 128-row
//   tile that would be padding for the rest.
// One work unit: the K-range of `split` of the TM x 128 output tile at (row0, col0) (D rows <-
// columns of A, D cols <- columns of B), written as fp64 into the partial tile Pt.
// lds: 2 stages of (TM + 128) x 32 floats (PL: and what syrk_batch_kernel adds behind them).
// H16 (round 3): one more 16-row block below the SK 32-row blocks, on v_mfma_f32_16x16x4_f32 (same flop
//   rate, half the rows): tile heights 48 / 80 / 112, so that l = 70 columns of Y (BASELINE config 4:
//   rank 50 + 20 oversamples) run 80 rows instead of 96.  Its fragments are 16-byte reads, one per operand
//   and half chunk (lane (i = lane & 15, kk = lane >> 4) takes the piece 4 u + kk of its column: MFMA e
//   contracts k = 16 u + 4 kk + e, two MFMAs per k-step and 16-column half of the wave's 32 columns).
//   (8-byte reads per k-step -- the first version -- were two-way bank-conflicted: columns 2j and 2j + 1
//   share a bank group under the piece swizzle; PMC: 27 % of the LDS-active cycles.)
// PL ("planes", the 128 x 128 SYRK tiles of K1 only): the k-step runs on the bf16 matrix core.  The same
//   ds_read_b128 pieces feed two groups of 16 k per chunk: a lane's 8 k-values of group g are its pieces of
//   the k-steps 2g and 2g + 1 (k = 16g + 4h + e and 16g + 8 + 4h + e, the same on both operands); every
//   value is split into three bf16 planes (bf16_split.h) and the six products h h, h' m, m h', h' l, m m,
//   l h' of a 32 x 32 block go as v_mfma_f32_32x32x16_bf16 into the same `acc` (its 16-register layout is
//   that of the fp32 instruction).  Non-finite input: nothing in the loop.  The chunk loop is instantiated twice, one
//   pass behind the other (plane_pass): the fast pass, then -- if any lane of the workgroup finds a NaN in its 64
//   values of acc + acc2 (a ballot per wave, one LDS word behind the stages, one barrier) -- the same unit again with
//   make_safe2 on every pair and sanitise2 between h h and the cross products; both give the same planes on finite
//   values, so outputs that no non-finite value feeds come out of the rerun as from a clean run.
//   Everything outside the k-step (staging, barrier, refill order, fold, commit) is that of the fp32 body.
//   (The former ablation ABL 16, the loop without its per-group detector, is what the product now runs.)
template <bool DMA, int ABL, int SK, int H16 = 0, int PL = 0>
__device__ __forceinline__ void tn_unit(const TnParams& p, const int split, const int row0_, const int col0_,
                                        double* Pt, float* lds) {
  static_assert(!H16 || SK >= 1, "a 16-row block only below at least one 32-row block");
  static_assert(!PL || (SK == 0 && H16 == 0), "the plane k-step is built for the 128 x 128 tile only");
#ifdef DMDX_STAMPS
  unsigned long long pt0;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(pt0)::"memory");
#endif
  // (plane k-step: the tile origin is wave-uniform, but the compiler carries it, and the panel bases made of it, in
  // vector registers past the tile decode's loops; it has none to spare)
  const int row0 = PL ? __builtin_amdgcn_readfirstlane(row0_) : row0_, col0 = PL ? __builtin_amdgcn_readfirstlane(col0_) : col0_;
  constexpr int TM = SK ? 32 * SK + 16 * H16 : BT;  // tile rows    (columns of OpA)
  constexpr int MI = SK ? SK : 2;        // 32-row MFMA blocks per wave
  constexpr int NI = SK ? 1 : 2;         // 32-column MFMA blocks per wave
  constexpr int NPA = (TM + 31) / 32;    // 1 KiB pieces of the A panel per wave (or 16 B pieces per thread)
  constexpr int NPIECE = TM / 8;         // 1 KiB pieces of the A panel in all (H16: wave w takes pieces w, w + 4, ...)
  constexpr int OPA = TM * BK, OPB = BT * BK, STG = OPA + OPB;  // floats per stage
  // stage st: A panel at lds + st * STG, B panel at lds + st * STG + OPA

  const int c_begin = split * p.chunks_per_split;
  int c_end = c_begin + p.chunks_per_split;
  if (c_end > p.chunks_total) c_end = p.chunks_total;
  const int nchunks = c_end - c_begin;
  const int64_t kend = p.K;
  // index of the one chunk that may be partial (K % 32 != 0), else -1
  const int tail_chunk = (kend % BK) ? p.chunks_total - 1 : -1;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = SK ? 0 : wave >> 1, wc = SK ? wave : wave & 1;
  const int l31 = lane & 31, lh = lane >> 5;

  // ---- staging assignment.  Columns past the matrix edge are clamped onto the last
  // valid column: they only feed rows/columns of D that the reduce kernel never stores.
  // DMA: wave w, instruction i (0..3) fills columns 32w + 8i + (lane >> 3), the lane's
  // 16-byte slot (lane & 7) holds global k-chunk (lane & 7) ^ swz(col).
  // Register path: thread -> column (tid >> 3) + 32 i, k-chunk (tid & 7).
  // addresses = wave-uniform tile base (SGPRs, advanced along K) + 32-bit per-lane element
  // offset: the LDS-DMA then needs no per-instruction 64-bit VALU add
  const int ra0 = row0 < p.nrow ? row0 : p.nrow - 1;
  const int cb0 = col0 < p.ncol ? col0 : p.ncol - 1;
  const float* Abase = p.A + (int64_t)ra0 * p.lda;
  const float* Bbase = p.B + (int64_t)cb0 * p.ldb;
  unsigned aoff[NPA], boff[4];
  int stsa[NPA], stsb[4];  // register path: float offset inside an operand stage
  int kqa[NPA], kqb[4];    // 4 * (global k-chunk of this piece)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int lc = DMA ? 32 * wave + 8 * i + (lane >> 3) : (tid >> 3) + 32 * i;  // local column
    const int q = DMA ? ((lane & 7) ^ swz(lc)) : (tid & 7);                       // global k-chunk
    int cb = col0 + lc;
    cb = cb < p.ncol ? cb : p.ncol - 1;
    boff[i] = (unsigned)((int64_t)(cb - cb0) * p.ldb + 4 * q);  // < 128 * ld: host checks it fits
    stsb[i] = lc * BK + 4 * (DMA ? (lane & 7) : ((tid & 7) ^ swz(lc)));
    kqb[i] = 4 * q;
  }
#pragma unroll
  for (int i = 0; i < NPA; ++i) {
    // (H16: the A panel has TM / 8 pieces, not a multiple of 4: wave w takes the pieces w + 4 i < NPIECE;
    // register path: the columns (tid >> 3) + 32 i < TM)
    const int lc = DMA ? (H16 ? 8 * (wave + 4 * i) : (TM / 4) * wave + 8 * i) + (lane >> 3) : (tid >> 3) + 32 * i;
    const int q = DMA ? ((lane & 7) ^ swz(lc)) : (tid & 7);
    int ca = row0 + (lc < TM ? lc : TM - 1);
    ca = ca < p.nrow ? ca : p.nrow - 1;
    aoff[i] = (unsigned)((int64_t)(ca - ra0) * p.lda + 4 * q);
    stsa[i] = lc * BK + 4 * (DMA ? (lane & 7) : ((tid & 7) ^ swz(lc)));
    kqa[i] = 4 * q;
  }

  // LDS-DMA addressing: wave-uniform byte pointer (SGPR pair, advanced along K) + 32-bit
  // per-lane BYTE offset, the `saddr` form of global_load_lds -- no VALU work per piece.
  // Piece i of an operand lands at LDS base (M0) + 1024 i through the instruction's immediate
  // offset, which the hardware adds to the global address too: offsets carry + 3072 - 1024 i
  // and the base pointer - 3072, so that every offset stays non-negative.
  const char* Adma = reinterpret_cast<const char*>(Abase) - (H16 ? 0 : 3072);
  const char* Bdma = reinterpret_cast<const char*>(Bbase) - 3072;
  unsigned aoffb[NPA], boffb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) boffb[i] = 4u * boff[i] + 3072u - 1024u * i;
#pragma unroll
  for (int i = 0; i < NPA; ++i) aoffb[i] = H16 ? 4u * aoff[i] : 4u * aoff[i] + 3072u - 1024u * i;

  f32x16 acc[MI][NI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

  // ---- two-level fp32 accumulation inside a unit, fp64 across units.
  // acc holds fp32 chains of at most FOLD*32 = 4096 rows.  Every FOLD chunks block
  // q = (mi, ni) of the wave is added into acc2 (registers) and cleared; the four blocks
  // are staggered by FOLD/4 chunks.  A unit runs <= max_cps chunks, so acc2 sums <= 16
  // chain results: the rounding error stays that of a 4096-row fp32 chain (blocked
  // summation), and the loop touches no memory except the operand stream.  (Folding
  // into an fp64 tile in HBM instead cost 4.6 % -- ~115 VALU/VMEM instructions per fold,
  // each of which waits for an MFMA slot while the SIMD's other wave streams MFMAs.)
  // At the end of the unit acc + acc2 is stored once, as fp64, into the unit's partial tile.
  // (All of the above is the fp32 k-step.  The plane k-step, PL, folds all four blocks after EVERY chunk: acc holds
  // the 12 bf16 MFMAs of one chunk, 32 rows, and acc2 sums up to max_cps = 2048 chunk results with rounded fp32
  // adds -- the bf16 MFMA cuts its sum below the ulp of a grown accumulator, one-signed; see the file header.)
  f32x16 acc2[MI][NI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc2[mi][ni][r] = 0.f;
  // the 16-row block: two 16 x 16 results (column halves of the wave's 32 columns)
  f32x4 acch[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}, acch2[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  const int l15 = lane & 15, lkk = lane >> 4;
  const int lane_off = (64 * wr + 4 * lh) * BT + (SK ? 32 : 64) * wc + l31;
  // (the commit's copy: the plane k-step derives it where it commits, from lane_now())
  auto lane_off_of = [&](int ln) { return (64 * wr + 4 * (ln >> 5)) * BT + (SK ? 32 : 64) * wc + (ln & 31); };
  int lane_off_c = PL ? 0 : lane_off;
#define DMDX_BLOCK_OFF(mi, ni, r) ((32 * (mi) + ((r) & 3) + 8 * ((r) >> 2)) * BT + 32 * (ni))
#define DMDX_FOLD(mi, ni)                                                         \
  do {                                                                            \
    acc2[mi][ni] += acc[mi][ni];                                                  \
    _Pragma("unroll") for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;          \
  } while (0)
#define DMDX_COMMIT(mi, ni)                                                       \
  do {                                                                            \
    double* q_ = Pt + lane_off_c;                                                 \
    _Pragma("unroll") for (int r = 0; r < 16; ++r)                                \
        __builtin_nontemporal_store((double)(acc[mi][ni][r] + acc2[mi][ni][r]),   \
                                    q_ + DMDX_BLOCK_OFF(mi, ni, r));              \
  } while (0)
#define DMDX_COMMIT_H16()                                                         \
  do {                                                                            \
    _Pragma("unroll") for (int hh = 0; hh < 2; ++hh)                              \
        _Pragma("unroll") for (int r = 0; r < 4; ++r)                             \
            __builtin_nontemporal_store((double)(acch[hh][r] + acch2[hh][r]),     \
                                        Pt + (32 * SK + 4 * lkk + r) * BT + 32 * wc + 16 * hh + l15); \
  } while (0)
#define DMDX_COMMIT_ALL()                                                         \
  do {                                                                            \
    if constexpr (H16 != 0) DMDX_COMMIT_H16();                                    \
    DMDX_COMMIT(0, 0);                                                            \
    if constexpr (MI >= 2) DMDX_COMMIT(MI >= 2 ? 1 : 0, 0);                       \
    if constexpr (NI == 2) {                                                      \
      DMDX_COMMIT(0, NI - 1);                                                     \
      DMDX_COMMIT(1, NI - 1);                                                     \
    }                                                                             \
    if constexpr (MI == 3) DMDX_COMMIT(MI - 1, 0);                                \
  } while (0)

  if (nchunks <= 0) {  // empty split: the partial tile must still be defined
    if constexpr (PL != 0) lane_off_c = lane_off_of(lane_now());
    DMDX_COMMIT_ALL();
    return;
  }

  // ---- global -> LDS for one chunk into stage st
  // (the lambdas take the DMA byte offsets as arguments: the plane k-step hands in the copies it parks in LDS)
  auto stage_regs = [&](int chunk, int st, bool tail, const unsigned (&aoffb)[NPA], const unsigned (&boffb)[4]) {  // register path (tail / unaligned)
    const int64_t k0 = (int64_t)chunk * BK;
    f32x4 ra[NPA], rb[4];
    // (plane k-step: no registers to spare for these offsets over the whole loop -- the LDS-DMA path needs them
    // for its one tail chunk only.  The same values are derived here: from the DMA byte offsets and the lane's
    // position, or, on the register path, as in the staging assignment above)
    unsigned boff_[4], aoff_[NPA];
    int stsb_[4], kqb_[4], stsa_[NPA], kqa_[NPA];
    int tid_ = tid;
    if constexpr (PL != 0) tid_ = 64 * wave + lane_now();   // (derived HERE: not hoisted out of the chunk loop again)
    const int lane_ = tid_ & 63;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if constexpr (PL != 0 && DMA) {
        const int lcb = 32 * wave + 8 * i + (lane_ >> 3), lca = (TM / 4) * wave + 8 * i + (lane_ >> 3);
        kqb_[i] = 4 * ((lane_ & 7) ^ swz(lcb));
        kqa_[i] = 4 * ((lane_ & 7) ^ swz(lca));
        stsb_[i] = lcb * BK + 4 * (lane_ & 7);
        stsa_[i] = lca * BK + 4 * (lane_ & 7);
        boff_[i] = (boffb[i] - 3072u + 1024u * i) >> 2;
        aoff_[i] = (aoffb[i] - 3072u + 1024u * i) >> 2;
        asm volatile("" : "+v"(boff_[i]), "+v"(aoff_[i]));   // (no per-piece 64-bit pointer carried along the loop)
      } else if constexpr (PL != 0) {
        const int lc = (tid_ >> 3) + 32 * i, q = tid_ & 7;
        int cb = col0 + lc, ca = row0 + lc;
        cb = cb < p.ncol ? cb : p.ncol - 1;
        ca = ca < p.nrow ? ca : p.nrow - 1;
        boff_[i] = (unsigned)((int64_t)(cb - cb0) * p.ldb + 4 * q);
        aoff_[i] = (unsigned)((int64_t)(ca - ra0) * p.lda + 4 * q);
        stsb_[i] = stsa_[i] = lc * BK + 4 * (q ^ swz(lc));
        kqb_[i] = kqa_[i] = 4 * q;
      } else {
        boff_[i] = boff[i]; stsb_[i] = stsb[i]; kqb_[i] = kqb[i];
        if (i < NPA) {
          const int ia = i < NPA ? i : 0;   // (the clamp is for the compiler's array-bounds warning alone: NPA < 4 for the short tiles)
          aoff_[ia] = aoff[ia]; stsa_[ia] = stsa[ia]; kqa_[ia] = kqa[ia];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float* pb = Bbase + k0 + boff_[i];
      rb[i] = tail ? load4_tail(pb, k0 + kqb_[i], kend) : f32x4{pb[0], pb[1], pb[2], pb[3]};
    }
#pragma unroll
    for (int i = 0; i < NPA; ++i) {
      const float* pa = Abase + k0 + aoff_[i];
      ra[i] = tail ? load4_tail(pa, k0 + kqa_[i], kend) : f32x4{pa[0], pa[1], pa[2], pa[3]};
    }
    // (H16: the last piece / the last group of 32 columns is only half inside the panel)
    const bool a_last_ok = !H16 || (DMA ? wave + 4 * (NPA - 1) < NPIECE : (tid >> 3) + 32 * (NPA - 1) < TM);
    float* as = lds + st * STG;
    float* bs = lds + st * STG + OPA;
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(bs + stsb_[i]) = rb[i];
#pragma unroll
    for (int i = 0; i < NPA; ++i)
      if (i + 1 < NPA || a_last_ok) *reinterpret_cast<f32x4*>(as + stsa_[i]) = ra[i];
  };
// The 8 pieces of the next chunk in one asm block: 2 SALU (M0) + 8 VMEM, no VALU.  A wave
// whose SIMD partner streams MFMAs gets ~one instruction issued per MFMA slot (stamps:
// ~64-95 cycles each), so every VALU address add in this phase cost a whole MFMA slot.
#define DMDX_DMA_OP4(ptr, la, o0, o1, o2, o3)                                                      \
  asm volatile("s_mov_b32 m0, %[la_]\n\ts_nop 0\n\t"                                               \
               "global_load_lds_dwordx4 %[a0], %[ap_]\n\t"                                         \
               "global_load_lds_dwordx4 %[a1], %[ap_] offset:1024\n\t"                             \
               "global_load_lds_dwordx4 %[a2], %[ap_] offset:2048\n\t"                             \
               "global_load_lds_dwordx4 %[a3], %[ap_] offset:3072"                                 \
               :: [la_] "s"(la), [ap_] "s"(ptr), [a0] "v"(o0), [a1] "v"(o1), [a2] "v"(o2), [a3] "v"(o3) \
               : "memory")
#define DMDX_DMA_OP3(ptr, la, o0, o1, o2)                                                          \
  asm volatile("s_mov_b32 m0, %[la_]\n\ts_nop 0\n\t"                                               \
               "global_load_lds_dwordx4 %[a0], %[ap_]\n\t"                                         \
               "global_load_lds_dwordx4 %[a1], %[ap_] offset:1024\n\t"                             \
               "global_load_lds_dwordx4 %[a2], %[ap_] offset:2048"                                 \
               :: [la_] "s"(la), [ap_] "s"(ptr), [a0] "v"(o0), [a1] "v"(o1), [a2] "v"(o2)           \
               : "memory")
#define DMDX_DMA_OP1(ptr, la, o0)                                                                  \
  asm volatile("s_mov_b32 m0, %[la_]\n\ts_nop 0\n\t"                                               \
               "global_load_lds_dwordx4 %[a0], %[ap_]"                                             \
               :: [la_] "s"(la), [ap_] "s"(ptr), [a0] "v"(o0)                                       \
               : "memory")
#define DMDX_DMA_OP2(ptr, la, o0, o1)                                                              \
  asm volatile("s_mov_b32 m0, %[la_]\n\ts_nop 0\n\t"                                               \
               "global_load_lds_dwordx4 %[a0], %[ap_]\n\t"                                         \
               "global_load_lds_dwordx4 %[a1], %[ap_] offset:1024"                                 \
               :: [la_] "s"(la), [ap_] "s"(ptr), [a0] "v"(o0), [a1] "v"(o1)                         \
               : "memory")
#define DMDX_DMA_A(ap, la)                                                                         \
  do {                                                                                             \
    if constexpr (H16 != 0) {                                                                      \
      _Pragma("unroll") for (int i_ = 0; i_ < NPA; ++i_)                                           \
          if (i_ + 1 < NPA || wave + 4 * (NPA - 1) < NPIECE) DMDX_DMA_OP1(ap, (la) + 4096u * i_, aoffb[i_]); \
    } else if constexpr (NPA == 4) DMDX_DMA_OP4(ap, la, aoffb[0], aoffb[1], aoffb[NPA - 2], aoffb[NPA - 1]); \
    else if constexpr (NPA == 3) DMDX_DMA_OP3(ap, la, aoffb[0], aoffb[1], aoffb[NPA - 1]);         \
    else if constexpr (NPA == 2) DMDX_DMA_OP2(ap, la, aoffb[0], aoffb[NPA - 1]);                   \
    else DMDX_DMA_OP1(ap, la, aoffb[0]);                                                           \
  } while (0)
#define DMDX_DMA_B(bp, lb) DMDX_DMA_OP4(bp, lb, boffb[0], boffb[1], boffb[2], boffb[3])
#define DMDX_DMA_NEXT(ap, bp, la, lb) \
  do {                                \
    DMDX_DMA_A(ap, la);               \
    DMDX_DMA_B(bp, lb);               \
  } while (0)
  auto stage_dma = [&](int chunk, int st, const unsigned (&aoffb)[NPA], const unsigned (&boffb)[4]) {
    const int64_t k0 = (int64_t)chunk * BK;
    float* as = lds + st * STG + (H16 ? 8 * wave : (TM / 4) * wave) * BK;
    float* bs = lds + st * STG + OPA + (32 * wave) * BK;
    // (readfirstlane: wave-uniform by construction, but the "s" constraint of the asm block does not make it an SGPR)
    DMDX_DMA_NEXT(Adma + 4 * k0, Bdma + 4 * k0, __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)DMDX_LDS_PTR(as)),
                  __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)DMDX_LDS_PTR(bs)));
  };
  auto stage_with = [&](int chunk, int st, const unsigned (&ao)[NPA], const unsigned (&bo)[4]) {
    if (DMA) {
      if (chunk != tail_chunk) stage_dma(chunk, st, ao, bo);
      else stage_regs(chunk, st, true, ao, bo);
    } else {
      stage_regs(chunk, st, chunk == tail_chunk, ao, bo);
    }
  };
  auto stage = [&](int chunk, int st) { stage_with(chunk, st, aoffb, boffb); };

  // ---- MFMA operand fragments, two register sets: the set for k-step t+1 is read from
  // LDS while the 16 MFMAs of k-step t run.  Lane (r = lane&31, h = lane>>5) reads, for
  // k-step t, the 16-byte k-chunk (2t + h) of its column, stored at slot (2t+h) ^ swz.
  f32x4 fa0[MI], fb0[NI], fa1[MI], fb1[NI];
  // the 16-row block: one 16-byte read per operand and HALF chunk (k-steps 2u, 2u + 1): lane (i = lane & 15,
  // kk = lane >> 4) takes the piece 4u + kk of its column, MFMA e (two per k-step) contracts k = 16u + 4kk + e
  f32x4 hA[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  f32x4 hB[2][2] = {{{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}, {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}};
  int foff[4], foffh[2];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    foff[t] = l31 * BK + 4 * ((2 * t + lh) ^ swz(l31));
    if (t < 2) foffh[t] = l15 * BK + 4 * ((4 * t + lkk) ^ swz(l15));
  }
  const int frag_a = 64 * wr * BK, frag_b = (SK ? 32 : 64) * wc * BK;
#define DMDX_READ_FRAGS(FA, FB, st, t)                                               \
  do {                                                                               \
    if constexpr (H16 != 0) {                                                        \
      if constexpr ((t) % 2 == 0) {                                                  \
        const float* ah_ = lds + (st) * STG + 32 * SK * BK + foffh[(t) / 2];         \
        const float* bh_ = lds + (st) * STG + OPA + frag_b + foffh[(t) / 2];         \
        hA[(t) / 2] = *reinterpret_cast<const f32x4*>(ah_);                          \
        hB[(t) / 2][0] = *reinterpret_cast<const f32x4*>(bh_);                       \
        hB[(t) / 2][1] = *reinterpret_cast<const f32x4*>(bh_ + 16 * BK);             \
      }                                                                              \
    }                                                                                \
    const float* as_ = lds + (st) * STG + frag_a + foff[t];                          \
    const float* bs_ = lds + (st) * STG + OPA + frag_b + foff[t];                    \
    FA[0] = *reinterpret_cast<const f32x4*>(as_);                                    \
    if constexpr (MI >= 2) FA[MI >= 2 ? 1 : 0] = *reinterpret_cast<const f32x4*>(as_ + 32 * BK); \
    if constexpr (MI == 3) FA[MI - 1] = *reinterpret_cast<const f32x4*>(as_ + 64 * BK); \
    FB[0] = *reinterpret_cast<const f32x4*>(bs_);                                    \
    if constexpr (NI == 2) FB[NI - 1] = *reinterpret_cast<const f32x4*>(bs_ + 32 * BK); \
  } while (0)

  // ---- chunk pipeline.  Both stages are filled up front; chunk c computes k-steps 0..2 from
  // stage `cur`, then the barrier (all waves are done reading `cur`: the k-step-3 fragments
  // are already in registers; chunk c+1 has landed in the other stage), then the refill of
  // `cur` with chunk c+2 and the first fragment reads of chunk c+1 are issued and k-step 3
  // runs behind them -- the wave leaves the barrier with 16 MFMAs to issue while its LDS
  // reads and LDS-DMA pieces are in flight, and every LDS-DMA has a whole chunk to land.
  // Measured on cfg2 blocks: barrier after k-step 3 + refill before it 85.6 %, this order
  // 87.4 %; pieces issued between the MFMAs of k-step 3 81 %; s_setprio 3 around the
  // refill 68 %.
  // (plane k-step: the workgroup's alarm word, behind the stages and the parked DMA offsets; cleared ahead of the
  // first barrier, raised and read once at the end of the unit)
  int* const alarm_word = reinterpret_cast<int*>(lds + 2 * STG + (DMA ? 8 * NTH : 0));
  if constexpr (PL != 0) *alarm_word = 0;
  stage(c_begin, 0);
  if (nchunks > 1 && !(ABL & 1)) stage(c_begin + 1, 1);
  if (DMA) __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0), see the main loop
  __syncthreads();
  DMDX_READ_FRAGS(fa0, fb0, 0, 0);

#define DMDX_MFMA4(FA, FB, j)                                                                   \
  do {                                                                                          \
    _Pragma("unroll") for (int mi_ = 0; mi_ < MI; ++mi_)                                        \
        _Pragma("unroll") for (int ni_ = 0; ni_ < NI; ++ni_) acc[mi_][ni_] =                    \
            __builtin_amdgcn_mfma_f32_32x32x2f32(FA[mi_][j], FB[ni_][j], acc[mi_][ni_], 0, 0, 0); \
  } while (0)
  // k-step: [MI + NI ds_read of the next fragments] 4 * MI * NI MFMA
#define DMDX_KSTEP(FA, FB, i)                                      \
  do {                                                             \
    DMDX_MFMA4(FA, FB, 0);                                         \
    DMDX_MFMA4(FA, FB, 1);                                         \
    DMDX_MFMA4(FA, FB, 2);                                         \
    DMDX_MFMA4(FA, FB, 3);                                         \
    if constexpr (H16 != 0) {                                      \
      _Pragma("unroll") for (int s_ = 0; s_ < 2; ++s_)             \
          _Pragma("unroll") for (int hh_ = 0; hh_ < 2; ++hh_) acch[hh_] = \
              __builtin_amdgcn_mfma_f32_16x16x4f32(hA[(i) / 2][2 * ((i) % 2) + s_], hB[(i) / 2][hh_][2 * ((i) % 2) + s_], acch[hh_], 0, 0, 0); \
    }                                                              \
    __builtin_amdgcn_sched_group_barrier(0x008, 4 * MI * NI + 4 * H16, 0);   \
  } while (0)

#ifdef DMDX_STAMPS
  unsigned long long rt0, rt1, ct0;
  asm volatile("s_memrealtime %0\n\ts_memtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(rt0), "=s"(ct0)::"memory");
  unsigned long long st0 = 0, st1 = 0, st2 = 0, st2b = 0, st3 = 0, st4 = 0, sa0 = 0, sa1 = 0, sa2 = 0, sa3 = 0, sa5 = 0;
#endif
  int cur = 0;
  if constexpr (PL != 0) {
    // ---- plane k-step.  Blocks 0, 1: the A fragments (mi), 2, 3: the B fragments (ni).  One raw set: fa0 / fb0
    // hold the piece of k-step 2g, fa1 / fb1 that of k-step 2g + 1; the next group's pieces are read once the
    // planes of this one are there, and land behind its 24 MFMAs.
    // SAFE (the rerun of a unit whose fast pass ended with a NaN, see below): the class rule of bf16_split.h on every
    // group -- make_safe2 on the fresh planes, sanitise2 on PH between h h and the cross products.  Both are the
    // identity on finite values.
    unsigned PH[4][4], PM[4][4], PLo[4][4];
#define DMDX_SPLIT_GROUP()                                                                       \
  do {                                                                                           \
    __builtin_amdgcn_sched_barrier(0);  /* not among the MFMAs before it: two plane sets do not fit */ \
    _Pragma("unroll") for (int b_ = 0; b_ < 4; ++b_) {                                           \
      const f32x4 e_ = b_ < 2 ? fa0[b_ & 1] : fb0[b_ & 1], o_ = b_ < 2 ? fa1[b_ & 1] : fb1[b_ & 1]; \
      _Pragma("unroll") for (int q_ = 0; q_ < 4; ++q_) {                                         \
        const bf16split::f32x2_t x_ = q_ < 2 ? bf16split::f32x2_t{e_[2 * (q_ & 1)], e_[2 * (q_ & 1) + 1]} \
                                             : bf16split::f32x2_t{o_[2 * (q_ & 1)], o_[2 * (q_ & 1) + 1]}; \
        unsigned h_, m_, l_;                                                                     \
        bf16split::split2_fast_pair(x_, h_, m_, l_);                                             \
        if constexpr (SAFE) bf16split::make_safe2(x_[0], x_[1], h_, m_, l_);                     \
        PH[b_][q_] = h_; PM[b_][q_] = m_; PLo[b_][q_] = l_;                                      \
      }                                                                                          \
    }                                                                                            \
  } while (0)
#define DMDX_PLANE(P, b) __builtin_bit_cast(bf16x8, (u32x4){P[b][0], P[b][1], P[b][2], P[b][3]})
#define DMDX_MFMA_PL(PA, PB)                                                                     \
  do {                                                                                           \
    _Pragma("unroll") for (int mi_ = 0; mi_ < 2; ++mi_)                                          \
        _Pragma("unroll") for (int ni_ = 0; ni_ < 2; ++ni_) acc[mi_][ni_] =                      \
            __builtin_amdgcn_mfma_f32_32x32x16_bf16(DMDX_PLANE(PA, mi_), DMDX_PLANE(PB, 2 + ni_), acc[mi_][ni_], 0, 0, 0); \
  } while (0)
    // The 24 MFMAs of a group.  SAFE: h h sees the raw h, the cross products the copy with 0 in place of a non-finite
    // value (PH in place).  The l products come first: their registers take the B pieces of the next group
    // (rd: read the pieces of k-steps t0, t0 + 1 of stage st for it -- the A pieces up front).
#define DMDX_GROUP_MFMA(rd, st, t0, fresh)                                                            \
  do {                                                                                           \
    /* (foff[t] = foff[0] ^ 8 t -- the k-chunk index sits in bits 2 .. 4 -- derived here: one register, not four) */ \
    int f0_ = foff[0];                                                                           \
    asm volatile("" : "+v"(f0_));                                                                \
    const int fe_ = f0_ ^ (8 * (t0)), fo_ = f0_ ^ (8 * ((t0) + 1));                              \
    if (rd && !SAFE) {                                                                           \
      const float* as_ = lds + (st) * STG + frag_a;                                              \
      fa0[0] = *reinterpret_cast<const f32x4*>(as_ + fe_);                                       \
      fa0[1] = *reinterpret_cast<const f32x4*>(as_ + fe_ + 32 * BK);                             \
      fa1[0] = *reinterpret_cast<const f32x4*>(as_ + fo_);                                       \
      fa1[1] = *reinterpret_cast<const f32x4*>(as_ + fo_ + 32 * BK);                             \
    }                                                                                            \
    if (fresh) {  /* the chunk's first products start from zero: acc was folded into acc2 behind the last chunk */ \
      _Pragma("unroll") for (int mi_ = 0; mi_ < 2; ++mi_)                                        \
          _Pragma("unroll") for (int ni_ = 0; ni_ < 2; ++ni_) acc[mi_][ni_] =                    \
              __builtin_amdgcn_mfma_f32_32x32x16_bf16(DMDX_PLANE(PH, mi_), DMDX_PLANE(PH, 2 + ni_), f32x16(0.f), 0, 0, 0); \
    } else {                                                                                     \
      DMDX_MFMA_PL(PH, PH);                                                                      \
    }                                                                                            \
    if constexpr (SAFE) {  /* (between scheduling barriers: the rule's temporaries not next to anything in flight) */ \
      __builtin_amdgcn_sched_barrier(0);                                                         \
      _Pragma("unroll") for (int b_ = 0; b_ < 4; ++b_)                                           \
          _Pragma("unroll") for (int q_ = 0; q_ < 4; ++q_) {                                     \
            asm volatile("" : "+v"(PH[b_][q_]));  /* (the mask derived HERE: make_safe2's copy is not kept over the h h products) */ \
            PH[b_][q_] = bf16split::sanitise2(PH[b_][q_]);                                       \
          }                                                                                      \
      __builtin_amdgcn_sched_barrier(0);                                                         \
      if (rd) {  /* (the A pieces behind the rule, not next to its temporaries) */                \
        const float* as_ = lds + (st) * STG + frag_a;                                            \
        fa0[0] = *reinterpret_cast<const f32x4*>(as_ + fe_);                                     \
        fa0[1] = *reinterpret_cast<const f32x4*>(as_ + fe_ + 32 * BK);                           \
        fa1[0] = *reinterpret_cast<const f32x4*>(as_ + fo_);                                     \
        fa1[1] = *reinterpret_cast<const f32x4*>(as_ + fo_ + 32 * BK);                           \
      }                                                                                          \
    }                                                                                            \
    DMDX_MFMA_PL(PH, PLo);                                                                       \
    DMDX_MFMA_PL(PLo, PH);                                                                       \
    __builtin_amdgcn_sched_barrier(0);                                                           \
    if (rd) {                                                                                    \
      const float* bs_ = lds + (st) * STG + OPA + frag_b;                                        \
      fb0[0] = *reinterpret_cast<const f32x4*>(bs_ + fe_);                                       \
      fb0[1] = *reinterpret_cast<const f32x4*>(bs_ + fe_ + 32 * BK);                             \
      fb1[0] = *reinterpret_cast<const f32x4*>(bs_ + fo_);                                       \
      fb1[1] = *reinterpret_cast<const f32x4*>(bs_ + fo_ + 32 * BK);                             \
    }                                                                                            \
    DMDX_MFMA_PL(PH, PM);                                                                        \
    DMDX_MFMA_PL(PM, PH);                                                                        \
    DMDX_MFMA_PL(PM, PM);                                                                        \
  } while (0)
    DMDX_READ_FRAGS(fa1, fb1, 0, 1);
    // The DMA byte offsets do not fit into the registers next to the planes: every thread parks its eight in LDS
    // behind the stages (its own 32 bytes: no synchronisation) and reads them back ahead of every refill.
    if constexpr (DMA) {
      u32x4* park = reinterpret_cast<u32x4*>(lds + 2 * STG) + 2 * tid;
      park[0] = u32x4{aoffb[0], aoffb[1], aoffb[2], aoffb[3]};
      park[1] = u32x4{boffb[0], boffb[1], boffb[2], boffb[3]};
    }
    // One pass over the unit's chunks, from both stages filled and the first group's pieces in fa0 / fb0 / fa1 / fb1.
    // Two instantiations, one behind the other: the fast pass holds no trace of the class rule.
    auto plane_pass = [&](auto safe_) __attribute__((always_inline)) {
      constexpr bool SAFE = decltype(safe_)::value;
      for (int c = 0; c < nchunks; ++c) {
        DMDX_STAMP(st0);
        const bool has_next = (c + 1 < nchunks) && !(ABL & 1);
        DMDX_STAMP(st1);
        DMDX_SPLIT_GROUP();
        DMDX_GROUP_MFMA(true, cur, 2, true);
        DMDX_SPLIT_GROUP();
        DMDX_STAMP(st2);
        unsigned pa[NPA] = {0u, 0u, 0u, 0u}, pb[4] = {0u, 0u, 0u, 0u};
        if (DMA && c + 2 < nchunks) {
          const u32x4* park = reinterpret_cast<const u32x4*>(lds + 2 * STG) + 2 * (64 * wave + lane_now());
          const u32x4 a_ = park[0], b_ = park[1];
          pa[0] = a_[0]; pa[1] = a_[1]; pa[2] = a_[2]; pa[3] = a_[3];
          pb[0] = b_[0]; pb[1] = b_[1]; pb[2] = b_[2]; pb[3] = b_[3];
        }

        if (DMA) __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0): the asm LDS-DMA pieces are invisible to the compiler's counters
        DMDX_STAMP(st2b);
        if (!(ABL & 2)) __syncthreads();
        if (c + 2 < nchunks && !(ABL & 1)) stage_with(c_begin + c + 2, cur, pa, pb);
        cur ^= 1;
        DMDX_STAMP(st3);
        DMDX_GROUP_MFMA(has_next, cur, 0, false);
        // The bf16 MFMA truncates its sum a few bits below the fp32 ulp of the accumulator (measured: a one-signed
        // 6e-7 on the diagonal of a Gram with 1312-row chains, growing with the chain), so the plane body keeps its
        // MFMA chains to ONE chunk: every chunk's 32-row result is added into acc2 by rounded fp32 adds (32 packed
        // adds per chunk) and the next chunk starts from zero.  acc2 then sums at most 2048 chunk results.
        if (!(ABL & 8)) {
          DMDX_FOLD(0, 0); DMDX_FOLD(0, NI - 1); DMDX_FOLD(MI - 1, 0); DMDX_FOLD(MI - 1, NI - 1);
        }
#ifdef DMDX_STAMPS
        DMDX_STAMP(st4);
        sa0 += st1 - st0; sa1 += st2 - st1; sa2 += st3 - st2b; sa3 += st4 - st3; sa5 += st2b - st2;
#endif
      }
    };
    // (PL = 3, the rerun launch behind the plane-fed fast pass: tn_unit_planes has run the unit on the fast planes and
    // raised the alarm; the class-safe pass alone, from the same prologue)
    if constexpr (PL != 3) plane_pass(std::false_type{});
    // ---- the verdict, once per unit.  The fast planes of an Inf or NaN carry a NaN in l (Inf - Inf), and l h' and
    // h' l are contracted for every pair: every output that a non-finite input of this K-range feeds holds NaN by
    // now, whatever its partners were (NaN * 0 included), and the fold kept it.  No NaN in acc + acc2: the fast
    // result is the result.  A NaN: the whole workgroup (the four waves share stages and barriers; an A-panel value
    // poisons two of them only) runs the unit again on class-safe planes and commits that.  Nothing has been written
    // to Pt so far.  Finite input that overflows to Inf - Inf raises the alarm too and gets the same classes again.
    bool nan_ = false;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
#pragma unroll
        for (int r = 0; r < 16; ++r) nan_ |= bf16split::alarm(acc[mi][ni][r] + acc2[mi][ni][r]);
    if (PL == 3 || __builtin_amdgcn_ballot_w64(nan_) != 0ull) *alarm_word = 1;   // (PL = 3: the verdict has been given)
    __syncthreads();   // (also: every wave is done with the stages of the fast pass)
    if (__builtin_amdgcn_readfirstlane(*alarm_word) != 0) {
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[mi][ni][r] = acc2[mi][ni][r] = 0.f;
      unsigned pa[NPA] = {0u, 0u, 0u, 0u}, pb[4] = {0u, 0u, 0u, 0u};
      if (DMA) {
        const u32x4* park = reinterpret_cast<const u32x4*>(lds + 2 * STG) + 2 * (64 * wave + lane_now());
        const u32x4 a_ = park[0], b_ = park[1];
        pa[0] = a_[0]; pa[1] = a_[1]; pa[2] = a_[2]; pa[3] = a_[3];
        pb[0] = b_[0]; pb[1] = b_[1]; pb[2] = b_[2]; pb[3] = b_[3];
      }
      cur = 0;
      stage_with(c_begin, 0, pa, pb);
      if (nchunks > 1 && !(ABL & 1)) stage_with(c_begin + 1, 1, pa, pb);
      if (DMA) __builtin_amdgcn_s_waitcnt(0x0f70);
      __syncthreads();
      {  // the first group's pieces, as DMDX_READ_FRAGS reads them for k-steps 0 and 1 (foff[1] = foff[0] ^ 8)
        int f0_ = foff[0];
        asm volatile("" : "+v"(f0_));
        const float* as_ = lds + frag_a;
        const float* bs_ = lds + OPA + frag_b;
        fa0[0] = *reinterpret_cast<const f32x4*>(as_ + f0_);
        fa0[1] = *reinterpret_cast<const f32x4*>(as_ + f0_ + 32 * BK);
        fa1[0] = *reinterpret_cast<const f32x4*>(as_ + (f0_ ^ 8));
        fa1[1] = *reinterpret_cast<const f32x4*>(as_ + (f0_ ^ 8) + 32 * BK);
        fb0[0] = *reinterpret_cast<const f32x4*>(bs_ + f0_);
        fb0[1] = *reinterpret_cast<const f32x4*>(bs_ + f0_ + 32 * BK);
        fb1[0] = *reinterpret_cast<const f32x4*>(bs_ + (f0_ ^ 8));
        fb1[1] = *reinterpret_cast<const f32x4*>(bs_ + (f0_ ^ 8) + 32 * BK);
      }
      plane_pass(std::true_type{});
    }
    {  // (no register held across the loop for the commit)
      lane_off_c = lane_off_of(lane_now());
    }
#undef DMDX_GROUP_MFMA
#undef DMDX_MFMA_PL
#undef DMDX_PLANE
#undef DMDX_SPLIT_GROUP
  } else {
  for (int c = 0; c < nchunks; ++c) {
    DMDX_STAMP(st0);
    const bool has_next = (c + 1 < nchunks) && !(ABL & 1);
    const int phase = c & (FOLD / 4 - 1), fq = (c / (FOLD / 4)) & 3;
    DMDX_STAMP(st1);
    DMDX_READ_FRAGS(fa1, fb1, cur, 1);
    __builtin_amdgcn_sched_group_barrier(0x100, MI + NI, 0);   // ds_reads of the next fragments (the 16-row block reads at even k-steps)
    DMDX_KSTEP(fa0, fb0, 0);
    DMDX_READ_FRAGS(fa0, fb0, cur, 2);
    __builtin_amdgcn_sched_group_barrier(0x100, MI + NI + 3 * H16, 0);
    DMDX_KSTEP(fa1, fb1, 1);
    DMDX_READ_FRAGS(fa1, fb1, cur, 3);
    __builtin_amdgcn_sched_group_barrier(0x100, MI + NI, 0);
    DMDX_KSTEP(fa0, fb0, 2);
    DMDX_STAMP(st2);

    if (DMA) __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0): the asm LDS-DMA pieces are invisible to the compiler's counters
    DMDX_STAMP(st2b);
    if (!(ABL & 2)) __syncthreads();
    if (c + 2 < nchunks && !(ABL & 1)) stage(c_begin + c + 2, cur);
    cur ^= 1;
    DMDX_STAMP(st3);
    if (has_next) DMDX_READ_FRAGS(fa0, fb0, cur, 0);
    __builtin_amdgcn_sched_group_barrier(0x100, MI + NI + 3 * H16, 0);
    DMDX_KSTEP(fa1, fb1, 3);
    if (!(ABL & 8) && phase == FOLD / 4 - 1) {
      switch (fq) {
        case 0: DMDX_FOLD(0, 0); break;
        case 1:
          if constexpr (NI == 2) { DMDX_FOLD(0, NI - 1); }
          else if constexpr (MI == 3) { DMDX_FOLD(MI - 1, 0); }
          break;
        case 2: if constexpr (MI >= 2) { DMDX_FOLD(MI >= 2 ? 1 : 0, 0); } break;
        default:
          if constexpr (NI == 2) { DMDX_FOLD(1, NI - 1); }
          if constexpr (H16 != 0) {
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
              acch2[hh] += acch[hh];
              acch[hh] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
          }
          break;
      }
    }
#ifdef DMDX_STAMPS
    DMDX_STAMP(st4);
    sa0 += st1 - st0; sa1 += st2 - st1; sa2 += st3 - st2b; sa3 += st4 - st3; sa5 += st2b - st2;
#endif
  }
  }
#ifdef DMDX_STAMPS
  if (lane == 0) {
    atomicAdd(&dmdx_stamp[0], sa0); atomicAdd(&dmdx_stamp[1], sa1);
    atomicAdd(&dmdx_stamp[2], sa2); atomicAdd(&dmdx_stamp[3], sa3);
    atomicAdd(&dmdx_stamp[5], sa5);
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rt1)::"memory");
    atomicAdd(&dmdx_stamp[6], st4 - ct0);   // core-clock cycles of this wave's chunk loop
    atomicAdd(&dmdx_stamp[7], rt1 - rt0);   // the same interval in 100 MHz reference ticks
    atomicAdd(&dmdx_stamp[4], (unsigned long long)nchunks);
    atomicAdd(&dmdx_stamp[8], ct0 - pt0);
    atomicAdd(&dmdx_stamp[10], 1ull);
  }
#endif
  DMDX_COMMIT_ALL();
#ifdef DMDX_STAMPS
  {
    unsigned long long et1;
    asm volatile("s_waitcnt vmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(et1)::"memory");
    if (lane == 0) atomicAdd(&dmdx_stamp[9], et1 - st4);
  }
#endif
#undef DMDX_READ_FRAGS
#undef DMDX_MFMA4
#undef DMDX_KSTEP
#undef DMDX_DMA_NEXT
#undef DMDX_DMA_A
#undef DMDX_DMA_B
#undef DMDX_DMA_OP4
#undef DMDX_DMA_OP2
#undef DMDX_DMA_OP1
#undef DMDX_DMA_OP3
#undef DMDX_FOLD
#undef DMDX_COMMIT_ALL
#undef DMDX_COMMIT_H16
#undef DMDX_COMMIT
#undef DMDX_BLOCK_OFF
}

// The plane-fed fast pass of K1 (syrk_batch_kernel with PL = 2; aligned blocks whose planes dmdx_syrk_blocks_planes_f32
// has made, plane_image.h): the fast pass of tn_unit's plane k-step with the split taken out of the loop.  The unit's
// two panels are two contiguous streams of 16-k groups (12 288 bytes each: 128 columns x 3 planes x 2 lane halves x 16
// bytes); LDS holds a ring of three stages of one A and one B group (24 KB each, 72 KB: what the fp32 stages and the
// parked offsets take).  Every wave copies a quarter of both groups of a stage with six LDS-DMA instructions whose lane
// offset is the constant 16 lane, and reads its 12 MFMA operands of a group (2 + 2 blocks of 32 columns x 3 planes)
// straight from LDS, one ds_read_b128 each: a wave-instruction reads 1 KiB in lane order, no swizzle anywhere.
// Group q: [operands in registers] 12 MFMAs (h h, h l, l h) -- wait for this wave's pieces of group q + 1, barrier
// (every wave's pieces of q + 1 have landed, every wave holds its operands of q: the stage of q is free) -- LDS-DMA of
// group q + 3 into the stage of q -- operand reads of q + 1 into the other register set -- 12 MFMAs (h m, m h, m m).
// A group is loaded three groups ahead and waited for two groups after its issue: 48 MFMAs of 32 cycles of this wave,
// about 3000 cycles with the SIMD's second wave issuing as many, against 1000 - 2000 of an HBM miss.
// The arithmetic is tn_unit's to the bit: the same planes (the pre-split kernel runs split2_fast; the padding of the
// images holds the zero planes the tail chunk's zero rows give -- and zero planes where tn_unit repeats the last
// column, which only feeds outputs the reduce kernel never stores and, being a copy, never changes the verdict), the
// same 24 MFMAs per group in the same order into the same accumulators, every chunk from the constant 0, the fold after
// every chunk, the same verdict.  A unit whose verdict is the alarm commits nothing but a NaN in the first element of its
// partial tile (a committed tile of a unit without alarm holds none): the rerun launch behind this one (PL = 3) runs
// exactly the marked units again from raw X on the class-safe planes (tn_unit with PL = 3: its prologue and its
// plane_pass(std::true_type{}), the fast pass and the verdict compiled out) and commits that.
// (Two launches and not one kernel: with tn_unit inlined behind this pass the register allocator spilled the class-safe
// loop, 216 bytes per lane; a launch whose workgroups read one word and leave costs some tens of microseconds.)
__device__ __forceinline__ void tn_unit_planes(const TnParams& p, const unsigned char* planes, const int split, const int row0_,
                                               const int col0_, double* Pt, float* lds_f) {
  constexpr unsigned HALF = 12288u, STAGE = 2u * HALF;   // bytes: one group of a panel; one ring stage (A group, B group)
  const int row0 = __builtin_amdgcn_readfirstlane(row0_), col0 = __builtin_amdgcn_readfirstlane(col0_);
  const int c_begin = split * p.chunks_per_split;
  int c_end = c_begin + p.chunks_per_split;
  if (c_end > p.chunks_total) c_end = p.chunks_total;
  const int nchunks = c_end - c_begin;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 1, wc = wave & 1;

  f32x16 acc[2][2], acc2[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = acc2[mi][ni][r] = 0.f;
  auto commit = [&]() {
    const int ln = lane_now();
    double* q_ = Pt + (64 * wr + 4 * (ln >> 5)) * BT + 64 * wc + (ln & 31);
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          __builtin_nontemporal_store((double)(acc[mi][ni][r] + acc2[mi][ni][r]),
                                      q_ + (32 * mi + (r & 3) + 8 * (r >> 2)) * BT + 32 * ni);
  };
  if (nchunks <= 0) {  // empty split: the partial tile must still be defined
    commit();
    return;
  }

  unsigned char* const lds = reinterpret_cast<unsigned char*>(lds_f);
  int* const alarm_word = reinterpret_cast<int*>(lds + 3 * STAGE);
  *alarm_word = 0;
  // ---- the two streams of this wave's quarter: group q of the unit at + q * HALF
  const int64_t ct = p.chunks_total;
  const unsigned char* Ag = planes + ((int64_t)(row0 / BT) * ct + c_begin) * (2 * (int64_t)HALF) + 3072 * wave;
  const unsigned char* Bg = planes + ((int64_t)(col0 / BT) * ct + c_begin) * (2 * (int64_t)HALF) + 3072 * wave;
  const unsigned lds0 = (unsigned)(uintptr_t)DMDX_LDS_PTR(lds);
  const unsigned voff = 16u * (unsigned)lane;   // the one per-lane offset: of every LDS-DMA piece (the hardware adds it on the LDS side itself)
  // (M0, the LDS-DMA's destination base, is written and read inside ONE statement, as in DMDX_DMA_OP4 and xty_dma.  It is
  // not in the clobber list: the register is reserved, the compiler answers an "m0" clobber with -Winline-asm and
  // ignores it.  It keeps no value in M0 across statements: on gfx950 neither its LDS instructions nor anything else it
  // emits for this kernel reads M0 -- the only M0 in the kernel's assembly are these writes.)
#define DMDX_PDMA3(ptr, la)                                                                        \
  asm volatile("s_mov_b32 m0, %[la_]\n\ts_nop 0\n\t"                                               \
               "global_load_lds_dwordx4 %[vo_], %[ap_]\n\t"                                        \
               "global_load_lds_dwordx4 %[vo_], %[ap_] offset:1024\n\t"                            \
               "global_load_lds_dwordx4 %[vo_], %[ap_] offset:2048"                                \
               :: [la_] "s"(la), [ap_] "s"(ptr), [vo_] "v"(voff) : "memory")
  auto issue = [&](int q, unsigned soff) {   // six pieces: this wave's quarter of group q into the stage at soff
    const unsigned la = lds0 + soff + 3072u * (unsigned)wave;
    DMDX_PDMA3(Ag + (int64_t)q * HALF, __builtin_amdgcn_readfirstlane(la));
    DMDX_PDMA3(Bg + (int64_t)q * HALF, __builtin_amdgcn_readfirstlane(la + HALF));
  };
  // ---- operands: [plane h, m, l][block]; A blocks 2 wr + mi, B blocks 2 wc + ni of the group's four 32-column blocks
  const unsigned char* const fa_base = lds + 2048 * wr + 16 * lane;
  const unsigned char* const fb_base = lds + HALF + 2048 * wc + 16 * lane;
  bf16x8 FA0[3][2], FB0[3][2], FA1[3][2], FB1[3][2];
#define DMDX_PREAD(FA, FB, soff)                                                                   \
  do {                                                                                             \
    const unsigned char* a_ = fa_base + (soff);                                                    \
    const unsigned char* b_ = fb_base + (soff);                                                    \
    _Pragma("unroll") for (int pl_ = 0; pl_ < 3; ++pl_)                                            \
        _Pragma("unroll") for (int b2_ = 0; b2_ < 2; ++b2_) {                                      \
          FA[pl_][b2_] = *reinterpret_cast<const bf16x8*>(a_ + 4096 * pl_ + 1024 * b2_);           \
          FB[pl_][b2_] = *reinterpret_cast<const bf16x8*>(b_ + 4096 * pl_ + 1024 * b2_);           \
        }                                                                                          \
  } while (0)
#define DMDX_PMFMA(FA, pa, FB, pb)                                                                 \
  do {                                                                                             \
    _Pragma("unroll") for (int mi_ = 0; mi_ < 2; ++mi_)                                            \
        _Pragma("unroll") for (int ni_ = 0; ni_ < 2; ++ni_) acc[mi_][ni_] =                        \
            __builtin_amdgcn_mfma_f32_32x32x16_bf16(FA[pa][mi_], FB[pb][ni_], acc[mi_][ni_], 0, 0, 0); \
  } while (0)
  // the first 12 MFMAs of a group: h h (fresh: from the constant 0, the chunk's first products), h l, l h
#define DMDX_PHEAD(FA, FB, fresh)                                                                  \
  do {                                                                                             \
    if (fresh) {                                                                                   \
      _Pragma("unroll") for (int mi_ = 0; mi_ < 2; ++mi_)                                          \
          _Pragma("unroll") for (int ni_ = 0; ni_ < 2; ++ni_) acc[mi_][ni_] =                      \
              __builtin_amdgcn_mfma_f32_32x32x16_bf16(FA[0][mi_], FB[0][ni_], f32x16(0.f), 0, 0, 0); \
    } else {                                                                                       \
      DMDX_PMFMA(FA, 0, FB, 0);                                                                    \
    }                                                                                              \
    DMDX_PMFMA(FA, 0, FB, 2);                                                                      \
    DMDX_PMFMA(FA, 2, FB, 0);                                                                      \
  } while (0)
  // the last 12: h m, m h, m m
#define DMDX_PTAIL(FA, FB)                                                                         \
  do {                                                                                             \
    DMDX_PMFMA(FA, 0, FB, 1);                                                                      \
    DMDX_PMFMA(FA, 1, FB, 0);                                                                      \
    DMDX_PMFMA(FA, 1, FB, 1);                                                                      \
  } while (0)
  // The hand-over in the middle of group q (q + 1 exists): this wave's pieces of q + 1 have landed (those of q + 2, six,
  // may still be in flight), its operand reads of q are done; behind the barrier that holds for every wave.  A raw
  // barrier: the pieces in flight stay in flight across it.  Then the refill of q's stage and the operands of q + 1.
#define DMDX_PHANDOVER(FA, FB, q)                                                                  \
  do {                                                                                             \
    if ((q) + 2 < ngroups) asm volatile("s_waitcnt vmcnt(6) lgkmcnt(0)\n\ts_barrier" ::: "memory"); \
    else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");                  \
    if ((q) + 3 < ngroups) issue((q) + 3, soff);                                                   \
    soff = soff == 2u * STAGE ? 0u : soff + STAGE;                                                 \
    DMDX_PREAD(FA, FB, soff);                                                                      \
  } while (0)

  const int ngroups = 2 * nchunks;
  issue(0, 0u);
  issue(1, STAGE);
  if (ngroups > 2) {
    issue(2, 2u * STAGE);
    asm volatile("s_waitcnt vmcnt(12) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(6) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  }
  unsigned soff = 0u;   // the stage of the group in the MFMAs
  DMDX_PREAD(FA0, FB0, soff);
  for (int c = 0; c < nchunks; ++c) {
    const int q = 2 * c;
    DMDX_PHEAD(FA0, FB0, true);
    DMDX_PHANDOVER(FA1, FB1, q);
    DMDX_PTAIL(FA0, FB0);
    DMDX_PHEAD(FA1, FB1, false);
    if (c + 1 < nchunks) {
      DMDX_PHANDOVER(FA0, FB0, q + 1);
    }
    DMDX_PTAIL(FA1, FB1);
    // (one chunk per MFMA chain, as in tn_unit: the bf16 MFMA cuts its sum below the ulp of a grown accumulator)
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        acc2[mi][ni] += acc[mi][ni];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;
      }
  }
#undef DMDX_PHANDOVER
#undef DMDX_PTAIL
#undef DMDX_PHEAD
#undef DMDX_PMFMA
#undef DMDX_PREAD
#undef DMDX_PDMA3
  // ---- the verdict (tn_unit's): a NaN in the unit's result <= a non-finite input fed it: nothing is committed here
  bool nan_ = false;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) nan_ |= bf16split::alarm(acc[mi][ni][r] + acc2[mi][ni][r]);
  if (__builtin_amdgcn_ballot_w64(nan_) != 0ull) *alarm_word = 1;
  __syncthreads();   // (every LDS-DMA piece has been waited for: nothing in flight)
  if (__builtin_amdgcn_readfirstlane(*alarm_word) != 0) {
    // the mark: a committed tile of a unit without alarm holds no NaN anywhere
    if (tid == 0) __builtin_nontemporal_store(__builtin_nan(""), Pt);
    return;
  }
  commit();
}

// XCD-aware unit order: groups of 512 consecutive blocks; the 64 blocks of a group that land on
// one XCD (blockIdx % 8) take 64 consecutive units (an 8 x 8 patch of tiles).  `b` counts from
// the start of a range whose first block index is a multiple of 8.
__device__ __forceinline__ int xcd_unit(int b, int total) {
  const int g = b >> 9;
  return ((g << 9) + 512 <= total) ? (g << 9) + (b & 7) * 64 + ((b & 511) >> 3) : b;
}

#ifndef DMDX_TN_ABL
#define DMDX_TN_ABL 0   // timing-only ablations of tn_unit: the diagnostic build alone sets it (csrc/Makefile)
#endif

// D (+)= sum_j A_j^T B_j over a batch of row blocks (TnBatch); p carries what the blocks share
// (shape of D, tiles, P).  SYRK: A_j == B_j, triangle tiles.  A single product is the batch of one
// block: unit_begin = {0, units}, slab_begin = {0, nsplit}, no padding.
// PL: the plane k-step of tn_unit (the 128 x 128 SYRK tiles of K1, unless DMDX_K1_ARITH=f32).  PL = 2 / 3 (aligned
// blocks with stored planes, dmdx_syrk_blocks_planes_f32): the plane-fed fast pass, tn_unit_planes, and the launch
// behind it that runs the class-safe pass of the units it marked.
template <bool DMA, int SK = 0, int H16 = 0, int PL = 0>
__global__ __launch_bounds__(NTH, 2) void syrk_batch_kernel(TnParams p, TnBatch bt) {
  constexpr int TM = SK ? 32 * SK + 16 * H16 : BT;
  // (plane k-step: + 32 bytes per thread for the parked DMA offsets of the LDS-DMA path, + 16 bytes for the alarm word
  // of the unit's verdict; 72 KiB + 16 bytes, two workgroups per CU)
  __shared__ __attribute__((aligned(16))) float lds[2 * (TM + BT) * BK + (PL && DMA ? 8 * NTH : 0) + (PL ? 4 : 0)];
  const int b = blockIdx.x;
  int j = 0;
  while (j + 1 < bt.nblocks && b >= bt.unit_begin[j + 1]) ++j;
  const int total = bt.nsplit[j] * p.ntiles;
  const int local = b - bt.unit_begin[j];
  if (local >= total) return;  // padding up to the next multiple of 512
  const int pos = xcd_unit(local, total);
  const int split = pos / p.ntiles;
  const int tile = pos - split * p.ntiles;
  int ta, tb;
  decode_tile(p.syrk, p.ntr, p.ntc, tile, ta, tb);
  p.A = bt.A[j];
  p.B = bt.B[j];
  p.lda = bt.lda[j];
  p.ldb = bt.ldb[j];
  p.K = bt.K[j];
  p.chunks_total = bt.chunks_total[j];
  p.chunks_per_split = bt.chunks_per_split[j];
  double* Pt = p.P + ((size_t)(bt.slab_begin[j] + split) * p.ntiles + tile) * (TM * BT);
  // (measurement aid: two scalar clock reads around the unit, three atomics per workgroup; the
  // sustained core clock of the launch = 100 MHz * sum(cycles) / sum(ticks))
  unsigned long long c0 = 0, r0 = 0;
  const int wave0 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (an SGPR: no VGPR held across the unit for the probe)
  if (bt.clk != nullptr) {
    c0 = __builtin_amdgcn_s_memtime();
    r0 = __builtin_amdgcn_s_memrealtime();
  }
  if constexpr (PL == 2) {   // the fast pass on the stored planes; a unit that raised the alarm leaves its mark
    tn_unit_planes(p, bt.planes[j], split, ta * TM, tb * BT, Pt, lds);
  } else if constexpr (PL == 3) {   // the rerun launch behind PL = 2: the class-safe pass of the marked units alone
    if (!bf16split::alarm((float)__builtin_nontemporal_load(Pt))) return;
    tn_unit<DMA, DMDX_TN_ABL, SK, H16, PL>(p, split, ta * TM, tb * BT, Pt, lds);
  } else {
    tn_unit<DMA, DMDX_TN_ABL, SK, H16, PL>(p, split, ta * TM, tb * BT, Pt, lds);
  }
  if (bt.clk != nullptr) {
    const unsigned long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    if (wave0 == 0 && lane_now() == 0) {
      atomicAdd(&bt.clk[0], c1 - c0);
      atomicAdd(&bt.clk[1], r1 - r0);
      atomicAdd(&bt.clk[2], 1ull);
    }
  }
}

// Sum the K-splits in fp64 and scatter the tile into D (row-major view:
// D[i*ld + j], which is the column-major C of the C ABI with the operand
// roles swapped by the host wrapper).  SYRK mode also writes the mirror.
__global__ __launch_bounds__(256) void gemm_tn_reduce_kernel(
    const double* P, int nsplit, int ntiles, int ntr, int ntc, int syrk, int nrow, int ncol,
    double* D64, int64_t ld64, float* D32, int64_t ld32, int accumulate, int tm) {
  __shared__ double tr[32][33];
  // one workgroup per (tile, 32x32 sub-block); a tile is tm (32 ... 128, a multiple of 16) rows x 128 columns
  const int nsb = ((tm + 31) / 32) * 4;
  const int tile = blockIdx.x / nsb;
  const int sb = blockIdx.x - tile * nsb;
  const int tile_elems = tm * BT;
  int ta, tb;
  decode_tile(syrk, ntr, ntc, tile, ta, tb);
  const int row0 = ta * tm, col0 = tb * BT;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const bool diag = syrk && (ta == tb);
  const int si = (sb >> 2) * 32, sj = (sb & 3) * 32;
  if (diag && si > sj) return;  // lower sub-blocks of a diagonal tile: mirrored from the upper ones
  if (row0 + si >= nrow || col0 + sj >= ncol) return;
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  const double* src = P + (size_t)tile * tile_elems + (si + ty) * BT + sj + tx;
  for (int sp = 0; sp < nsplit; ++sp) {
    const double* q = src + (size_t)sp * ntiles * tile_elems;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (si + ty + 8 * k < tm) v[k] += q[8 * k * BT];   // (a 48- / 80- / 112-row tile ends inside its last sub-block row)
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = si + ty + 8 * k, j = sj + tx;
    const int gi = row0 + i, gj = col0 + j;
    const bool keep = !(diag && i > j) && i < tm;
    if (keep && gi < nrow && gj < ncol) {
      double o = v[k];
      if (accumulate) o += D64[(int64_t)gi * ld64 + gj];
      D64[(int64_t)gi * ld64 + gj] = o;
      if (D32) D32[(int64_t)gi * ld32 + gj] = (float)o;
    }
    tr[ty + 8 * k][tx] = v[k];
  }
  if (syrk) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      // mirrored element: source (i = si+tx, j = sj+ty+8k) -> D[gj][gi]
      const int i = si + tx, j = sj + ty + 8 * k;
      const double s = tr[tx][ty + 8 * k];
      const int gi = row0 + i, gj = col0 + j;
      const bool keep = !(diag && i >= j) && i < tm;
      if (keep && gi < nrow && gj < ncol) {
        double o = s;
        if (accumulate) o += D64[(int64_t)gj * ld64 + gi];
        D64[(int64_t)gj * ld64 + gi] = o;
        if (D32) D32[(int64_t)gj * ld32 + gi] = (float)o;
      }
    }
  }
}

struct Plan {
  int tm;  // tile rows: 128, or 96 / 64 when that cuts the row padding of a non-SYRK product
  int syrk;  // triangle of tiles + mirror; a Gram of <= 96 columns runs as one 64- / 96-row tile of the
             // plain product X^T X instead (both triangles computed: half / three quarters of the MFMA
             // work of the 128 x 128 tile, no mirror pass)
  int ntr, ntc, ntiles, nsplit, chunks_total, chunks_per_split;
};

// The tail of a launch: its units are equally long and 512 of them are resident, so a launch of
// r = units / 512 rounds takes ceil(r) of them.  With few rounds, take the split count in (want, hi]
// that fills the last round best; the first one that fills it to 97 % wins.  Only when the wanted
// count leaves the last round less than 92 % full (measurements: make_plan, xty_small_plan).
// units_per_split: tiles x blocks of the launch; a block of no chunk has no units and keeps `want`.
int64_t fit_last_round(int64_t chunks, int64_t units_per_split, int64_t want, int64_t hi) {
  if (getenv("DMDX_TN_NO_TAILFIT") != nullptr) return want;
  auto fill = [&](int64_t w) {
    const int64_t cps = (chunks + w - 1) / w;
    const int64_t ns = cps > 0 ? (chunks + cps - 1) / cps : 0;
    const double r = (double)(units_per_split * ns) / 512.0;
    return r > 0.0 ? r / (double)(int64_t)(r + 0.999999) : 1.0;
  };
  int64_t best = want;
  double bf = fill(want);
  if (bf < 0.92)
    for (int64_t w = want + 1; bf < 0.97 && w <= hi; ++w)
      if (fill(w) > bf) { bf = fill(w); best = w; }
  return best;
}

// share: number of equally sized row blocks that share the launch (batched SYRK)
Plan make_plan(int64_t K, int64_t nrow, int64_t ncol, int syrk, int share = 1) {
  Plan pl;
  pl.tm = BT;
  const int gram = syrk;
  if (syrk && nrow <= 96) syrk = 0;
  pl.syrk = syrk;
  if (!syrk) {  // fewest padded rows; ties go to the taller tile (fewer re-reads of the B panels)
    int64_t best = (nrow + BT - 1) / BT * BT;
    for (int tm : {112, 96, 80, 64, 48, 32}) {
      // (a Gram keeps to the 32-row blocks: the 16-row block contracts k in another order, and
      // G[i][j] would differ from G[j][i] in the last bits)
      if (gram && tm % 32) continue;
      const int64_t padded = (nrow + tm - 1) / tm * tm;
      if (padded < best && (tm > 48 || nrow <= tm)) { best = padded; pl.tm = tm; }   // 32- / 48-row tiles: single tile row only
    }
  }
  if (const char* e = getenv("DMDX_TN_FORCE_TM")) {   // A/B knob (scripts/ab_k3.py): a tile height for the plain products
    const int f = atoi(e);
    if (!syrk && f >= 32 && f <= 128 && f % 16 == 0 && (f > 48 || nrow <= f)) pl.tm = f;
  }
  pl.ntr = (int)((nrow + pl.tm - 1) / pl.tm);
  pl.ntc = (int)((ncol + BT - 1) / BT);
  pl.ntiles = syrk ? pl.ntr * (pl.ntr + 1) / 2 : pl.ntr * pl.ntc;
  pl.chunks_total = (int)((K + BK - 1) / BK);
  if (pl.chunks_total < 1) pl.chunks_total = 1;
  // aim at >= ~20 rounds of 512 resident workgroups, keep >= 8 chunks per split, and
  // keep units short enough (<= max_cps chunks) that the workgroups sharing panels in
  // L2 / Infinity Cache do not drift apart along K
  // (round 2, cfg2 Gram incl. the reduce kernel, interleaved on one box: 256 -> 564-567 ms, 512 / 1024 /
  // 2048 -> 560-562 ms, 4096 -> 575-577 ms (38 rounds of 512: the last one shows).  2048 halves the
  // partial-tile workspace of 1024: 5 GB instead of 10 GB at cfg2, 9.5 instead of 19 GB at a cfg3 shard)
  int64_t max_cps = 2048;
  if (const char* e = getenv("DMDX_TN_MAX_CPS")) max_cps = atoll(e) > 0 ? atoll(e) : max_cps;
  // Rounds of 512 resident workgroups to aim at.  Every split costs a partial tile (written,
  // then read by the reduce kernel): many rounds only pay where the tiles are many and the
  // operands are re-read from L2 anyway (big SYRK); few-tile products and the HBM-streaming
  // X^T Y / Q^T X products (every X panel is read once) want few, long units
  // (cfg2 randomized: K3 97.6 ms at 20 rounds, 91.5 at 4..8; l x l Grams 12.5 -> 7.6 ms at 2).
  int64_t rounds = gram ? (pl.ntiles >= 64 ? 20 : 2) : 6;
  if (const char* e = getenv("DMDX_TN_ROUNDS")) rounds = atoll(e) > 0 ? atoll(e) : rounds;
  const int64_t per_split = (int64_t)pl.ntiles * share;
  int64_t want = (rounds * 512 + per_split - 1) / per_split;
  int64_t by_len = (pl.chunks_total + max_cps - 1) / max_cps;
  if (want < by_len) want = by_len;
  int64_t maxs = pl.chunks_total / 8;
  if (maxs < 1) maxs = 1;
  if (want > maxs) want = maxs;
  if (want < 1) want = 1;
  if (want > 256) want = 256;
  // The tail of the launch: its units are equally long and 512 of them are resident, so a launch of
  // r = units / 512 rounds takes ceil(r) of them -- 6.34 rounds (X^T Y of 16 cfg4 blocks, l = 70: 29 tiles x 7
  // splits x 16) cost 7.  With few rounds, take the split count (up to twice the wanted one) that fills the
  // last round best; the first one that fills it to 97 % wins.  (The Gram of cfg2 runs 75 rounds: unchanged.)
  // Only when the wanted count leaves the last round less than 92 % full: measured on 16 cfg4 blocks
  // (n = 3653) l = 70 11.58 -> 11.09 ms, l = 100 15.14 -> 14.24, l = 220 30.07 -> 27.95; on 8 cfg2 blocks
  // (n = 8760, last round 92.4 % full as it is) twice the splits cost 2 % (l = 60 10.60 -> 10.82 ms).
  want = fit_last_round(pl.chunks_total, per_split, want, std::min({maxs, (int64_t)256, 2 * want + 2}));
  pl.chunks_per_split = (int)((pl.chunks_total + want - 1) / want);
  pl.nsplit = (pl.chunks_total + pl.chunks_per_split - 1) / pl.chunks_per_split;
  return pl;
}

// ---- batched products: D (+)= sum_j A_j^T B_j, blocks in groups of MAXB per launch: the blocks
// [j0, j0 + group_len) share one
inline int group_len(int nblocks, int j0) { return std::min(nblocks - j0, MAXB); }

// partial tiles of the largest launch
size_t batch_ws(const int64_t* K, int nblocks, int64_t nrow, int64_t ncol, int syrk) {
  size_t need = 0;
  for (int j0 = 0; j0 < nblocks; j0 += MAXB) {
    const int nb = group_len(nblocks, j0);
    size_t slabs = 0;
    Plan pl{};
    for (int j = 0; j < nb; ++j) {
      pl = make_plan(K[j0 + j], nrow, ncol, syrk, nb);
      slabs += (size_t)pl.nsplit;
    }
    need = std::max(need, slabs * (size_t)pl.ntiles * pl.tm * BT * sizeof(double));
  }
  return need;
}

// The one launch path of all four entry points.  Nothing is refused here: the entry points have
// put the leading dimensions and the workspace (batch_ws) through tn_refusal before the first launch.
// probe: the launches feed dmdx_set_clock_probe (include/dmdx.h lists which entry points do).
// planes: null, or the first plane image of every block (dmdx_syrk_blocks_planes_f32 alone: a Gram of full tiles whose
// blocks are all aligned, not under DMDX_K1_ARITH=f32): the fast pass of K1 streams them (PL = 2).
inline bool tn_block_aligned(const float* A, int64_t la) { return la % 4 == 0 && dmdx_aligned16(A) && la < (int64_t(1) << 22); }
inline bool k1_arith_f32() {   // A/B knob: K1's full tiles on the fp32 MFMA (rounding only)
  const char* arith = getenv("DMDX_K1_ARITH");
  return arith != nullptr && strcmp(arith, "f32") == 0;
}
int run_batch(const float* const* A, const int64_t* lda, const float* const* B, const int64_t* ldb,
              const int64_t* K, int nblocks, int64_t nrow, int64_t ncol, int syrk, double* D64, int64_t ld64,
              float* D32, int64_t ld32, int accumulate, void* ws, hipStream_t stream, bool probe,
              const unsigned char* const* planes = nullptr) {
  for (int j0 = 0; j0 < nblocks; j0 += MAXB) {
    const int nb = group_len(nblocks, j0);
    TnBatch bt{};
    TnParams p{};
    bool aligned = true;
    int units = 0, slabs = 0;
    Plan pl{};
    for (int j = 0; j < nb; ++j) {
      const int64_t la = lda[j0 + j], lb = ldb[j0 + j];
      pl = make_plan(K[j0 + j], nrow, ncol, syrk, nb);
      bt.A[j] = A[j0 + j];
      bt.B[j] = B[j0 + j];
      bt.lda[j] = la;
      bt.ldb[j] = lb;
      bt.K[j] = K[j0 + j];
      bt.chunks_total[j] = pl.chunks_total;
      bt.chunks_per_split[j] = pl.chunks_per_split;
      bt.nsplit[j] = pl.nsplit;
      bt.unit_begin[j] = units;
      bt.slab_begin[j] = slabs;
      const int u = pl.nsplit * pl.ntiles;
      units += (j + 1 < nb) ? (u + 511) / 512 * 512 : u;
      slabs += pl.nsplit;
      aligned = aligned && tn_block_aligned(A[j0 + j], la) && tn_block_aligned(B[j0 + j], lb);
      bt.planes[j] = planes ? planes[j0 + j] : nullptr;
    }
    bt.unit_begin[nb] = units;
    bt.slab_begin[nb] = slabs;
    bt.nblocks = nb;
    bt.clk = probe ? dmdx_clock_probe_ptr : nullptr;
    p.nrow = (int)nrow;
    p.ncol = (int)ncol;
    p.ntr = pl.ntr; p.ntc = pl.ntc; p.ntiles = pl.ntiles; p.syrk = pl.syrk;
    p.nsplit = slabs;
    p.P = reinterpret_cast<double*>(ws);
    const dim3 grid((unsigned)units);
    // K1's full tiles run the bf16-plane k-step; DMDX_K1_ARITH=f32 keeps them on the fp32 MFMA (A/B, rounding only)
    if (pl.tm == BT && pl.syrk && !k1_arith_f32()) {
      if (aligned && planes) {
        hipLaunchKernelGGL((syrk_batch_kernel<true, 0, 0, 2>), grid, dim3(NTH), 0, stream, p, bt);
        DMDX_LAUNCH_CHECK();
        bt.clk = nullptr;   // (the probe counts the fast launch's workgroups)
        hipLaunchKernelGGL((syrk_batch_kernel<true, 0, 0, 3>), grid, dim3(NTH), 0, stream, p, bt);
      } else if (aligned) hipLaunchKernelGGL((syrk_batch_kernel<true, 0, 0, 1>), grid, dim3(NTH), 0, stream, p, bt);
      else hipLaunchKernelGGL((syrk_batch_kernel<false, 0, 0, 1>), grid, dim3(NTH), 0, stream, p, bt);
    } else
    switch (pl.tm) {
#define DMDX_TN_CASE(TMV, SKV, HV)                                                                          \
      case TMV:                                                                                             \
        if (aligned) hipLaunchKernelGGL((syrk_batch_kernel<true, SKV, HV>), grid, dim3(NTH), 0, stream, p, bt);    \
        else hipLaunchKernelGGL((syrk_batch_kernel<false, SKV, HV>), grid, dim3(NTH), 0, stream, p, bt);    \
        break
      DMDX_TN_CASE(32, 1, 0); DMDX_TN_CASE(48, 1, 1); DMDX_TN_CASE(64, 2, 0); DMDX_TN_CASE(80, 2, 1);
      DMDX_TN_CASE(96, 3, 0); DMDX_TN_CASE(112, 3, 1); DMDX_TN_CASE(128, 0, 0);
#undef DMDX_TN_CASE
      default: dmdx_set_error("gemm_tn: no kernel for tile height %d", pl.tm); return DMDX_E_INVALID;
    }
    DMDX_LAUNCH_CHECK();
    hipLaunchKernelGGL(gemm_tn_reduce_kernel, dim3(pl.ntiles * ((pl.tm + 31) / 32) * 4), dim3(256), 0, stream, p.P, slabs,
                       pl.ntiles, pl.ntr, pl.ntc, pl.syrk, (int)nrow, (int)ncol, D64, ld64, D32, ld32,
                       (accumulate || j0 > 0) ? 1 : 0, pl.tm);
    DMDX_LAUNCH_CHECK();
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------
// K3s: D (nb x na) (+)= sum_j Y_j^T X_j for nb <= 32 (the HBM-bound small-l products of the range
// finder at the reference's default n_components = 10, l = 20; the single-column product
// w = A^T mu of the mean deflation).  The generic body above stages 32-row chunks: every LDS-DMA
// piece is 8 columns x 128 B, i.e. every 128-byte request opens another DRAM page of a matrix
// whose columns are 0.5 MB apart, and the pass over cfg2's X runs at 4.85 TB/s where K2 (1 KB
// runs) streams the same bytes at 6.0 TB/s.  Here a chunk is 64 rows -- pieces of 4 columns x
// 256 B -- and the four waves of a workgroup split the ROWS of a chunk (16 each) instead of the
// columns of the tile, so that one workgroup still covers 128 time columns with 40 KB per stage:
//   tile  = 32 (l) x 128 (time columns), unit = (row block, K split, tile), 2 workgroups per CU;
//   stage = Y panel [32 col][64 k] + X panel [128 col][64 k] fp32, 16-byte k-pieces XOR-swizzled
//           with (col & 15) on the DMA source and on the fragment reads (conflict-free b128);
//   wave w contracts rows 16 w .. 16 w + 15 of every chunk: 2 k-steps x (1 + 4) ds_read_b128 and
//           32 MFMAs per chunk; fp32 chains of <= 2048 rows folded into a second accumulator;
//   end of unit: the four waves' 32 x 128 accumulators meet in LDS, one fp64 partial tile per
//           unit (no atomics), a second kernel sums the units of a tile into D.
// Rows beyond the last full 64-row chunk of a block (K % 64) go through the generic path
// (one extra batched launch over the tails, accumulate).
constexpr int XT = 128, XL = 32, XK = 64;
constexpr int XSTG = (XL + XT) * XK;   // floats per stage: 40 KB
constexpr int XFOLD = 128;             // chunks per fp32 chain (16 rows of each per wave: 2048 rows)

struct XtyBatch {
  const float* X[MAXB];   // big operand (D cols): K x na, ldx
  const float* Y[MAXB];   // small operand (D rows): K x nb, ldy
  int64_t ldx[MAXB], ldy[MAXB];
  int chunks[MAXB], cps[MAXB], nsplit[MAXB];
  int unit_begin[MAXB + 1];
  int nblocks, ntiles, na, nb;
  double* P;              // [unit][32][128] fp64
};

__device__ __forceinline__ void xty_dma(unsigned lds_addr, unsigned off, const char* base) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2"
               :: "s"(lds_addr), "v"(off), "s"(base) : "memory");
}

// T4 < 0: the body described above (32 rows of D on v_mfma_f32_32x32x2_f32).
// T4 = 0 / 1 / 2 (nb <= 16 / 20 / 24, round 3): 16 rows of D on v_mfma_f32_16x16x4_f32 -- lane (i, kk) reads the piece
//   4 wave + kk of its column: MFMA e contracts the wave's rows 16 wave + 4 kk + e -- and T4 groups of 4 more rows on
//   v_mfma_f32_4x4x1_16b_f32 with the sixteen blocks of an instruction on sixteen groups of 4 time columns: A = X[row]
//   [64 h + lane], B = Y[row][16 + 4 q + (lane & 3)], one row per instruction, 4 accumulator registers per 64 time
//   columns and no cross-lane sum.  The reference's default rank (l = 20) executes 20 columns of MFMA work per
//   X element instead of 32: PMC had the 32-column body at 79 % matrix-core occupancy under a 5.5 TB/s stream.
template <int T4>
__global__ __launch_bounds__(NTH, 2) void xty_small_kernel(XtyBatch bt) {
  __shared__ __attribute__((aligned(16))) float lds[2 * XSTG];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, lh = lane >> 5;
  const int u = blockIdx.x;
  int j = 0;
  while (j + 1 < bt.nblocks && u >= bt.unit_begin[j + 1]) ++j;
  const int local = u - bt.unit_begin[j];
  const int split = local / bt.ntiles, tile = local - split * bt.ntiles;
  const int c_begin = split * bt.cps[j];
  int c_end = c_begin + bt.cps[j];
  if (c_end > bt.chunks[j]) c_end = bt.chunks[j];
  const int nch = c_end - c_begin;
  const int col0 = tile * XT;
  const int64_t ldx = bt.ldx[j], ldy = bt.ldy[j];
  const int cb0 = col0 < bt.na ? col0 : bt.na - 1;
  const char* Xb = reinterpret_cast<const char*>(bt.X[j] + (int64_t)cb0 * ldx) + (int64_t)c_begin * XK * 4;
  const char* Yb = reinterpret_cast<const char*>(bt.Y[j]) + (int64_t)c_begin * XK * 4;

  // per-lane source byte offsets of this wave's pieces (columns past the edge clamp onto the last one)
  unsigned xoff[8], yoff[2];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int lc = 32 * wave + 4 * i + (lane >> 4);
    int cg = col0 + lc;
    cg = cg < bt.na ? cg : bt.na - 1;
    const int g = (lane & 15) ^ (lc & 15);
    xoff[i] = (unsigned)(((int64_t)(cg - cb0) * ldx + 4 * g) * 4);
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int lc = 8 * wave + 4 * i + (lane >> 4);
    const int cg = lc < bt.nb ? lc : bt.nb - 1;
    const int g = (lane & 15) ^ (lc & 15);
    yoff[i] = (unsigned)(((int64_t)cg * ldy + 4 * g) * 4);
  }
  auto issue = [&](int c, int st) {
    const char* xb = Xb + (int64_t)c * (XK * 4);
    const char* yb = Yb + (int64_t)c * (XK * 4);
    float* ys = lds + st * XSTG + (8 * wave) * XK;
    float* xs = lds + st * XSTG + XL * XK + (32 * wave) * XK;
#pragma unroll
    for (int i = 0; i < 2; ++i) xty_dma((unsigned)(uintptr_t)DMDX_LDS_PTR(ys + 4 * i * XK), yoff[i], yb);
#pragma unroll
    for (int i = 0; i < 8; ++i) xty_dma((unsigned)(uintptr_t)DMDX_LDS_PTR(xs + 4 * i * XK), xoff[i], xb);
  };

  if constexpr (T4 >= 0) {
    constexpr int NT = T4 > 0 ? T4 : 1;
    const int c15 = lane & 15, kk = lane >> 4;
    f32x4 a16[8], a16b[8], at[2][NT], atb[2][NT];
#pragma unroll
    for (int b = 0; b < 8; ++b) { a16[b] = f32x4{0.f, 0.f, 0.f, 0.f}; a16b[b] = f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int q = 0; q < NT; ++q) { at[h][q] = f32x4{0.f, 0.f, 0.f, 0.f}; atb[h][q] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    if (nch > 0) issue(0, 0);
    if (nch > 1) issue(1, 1);
    const int ko16 = 4 * ((4 * wave + kk) ^ c15);          // the 16-column operands: piece 4 wave + kk of column c15 (+ 16 b)
    for (int c = 0; c < nch; ++c) {
      const int st = c & 1;
      if (c + 1 < nch) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      const float* ys = lds + st * XSTG;
      const float* xs = ys + XL * XK;
      const f32x4 fa = *reinterpret_cast<const f32x4*>(ys + c15 * XK + ko16);
      f32x4 fb[8];
#pragma unroll
      for (int b = 0; b < 8; ++b) fb[b] = *reinterpret_cast<const f32x4*>(xs + (16 * b + c15) * XK + ko16);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int b = 0; b < 8; ++b) a16[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[e], fb[b][e], a16[b], 0, 0, 0);
      if constexpr (T4 > 0) {
#pragma unroll
        for (int p4 = 0; p4 < 4; ++p4) {                     // rows 16 wave + 4 p4 + e
          f32x4 ax[2], by[NT];
#pragma unroll
          for (int h = 0; h < 2; ++h)
            ax[h] = *reinterpret_cast<const f32x4*>(xs + (64 * h + lane) * XK + 4 * ((4 * wave + p4) ^ (lane & 15)));
#pragma unroll
          for (int q = 0; q < NT; ++q) {
            const int yc = 16 + 4 * q + (lane & 3);
            by[q] = *reinterpret_cast<const f32x4*>(ys + yc * XK + 4 * ((4 * wave + p4) ^ (yc & 15)));
          }
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
              for (int q = 0; q < NT; ++q) at[h][q] = __builtin_amdgcn_mfma_f32_4x4x1f32(ax[h][e], by[q][e], at[h][q], 0, 0, 0);
        }
      }
      __syncthreads();   // every wave has read stage st for the last time
      if (c + 2 < nch) issue(c + 2, st);
      if ((c & (XFOLD - 1)) == XFOLD - 1) {
#pragma unroll
        for (int b = 0; b < 8; ++b) { a16b[b] += a16[b]; a16[b] = f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int q = 0; q < NT; ++q) { atb[h][q] += at[h][q]; at[h][q] = f32x4{0.f, 0.f, 0.f, 0.f}; }
      }
    }
    // ---- this wave's 32 x 128 image: rows 0..15 from the 16 x 16 results (lane (j, q), register r: row 4 q + r,
    // column 16 b + j), rows 16 + 4 q + (lane & 3) from the 4 x 4 blocks (register i: column 64 h + 4 (lane >> 2) + i),
    // the rest zero
    float* red = lds + wave * (XL * XT);
#pragma unroll
    for (int b = 0; b < 8; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[(4 * kk + r) * XT + 16 * b + c15] = a16[b][r] + a16b[b][r];
    for (int o = 4 * lane; o < 16 * XT; o += 256)            // rows 16 .. 31
      *reinterpret_cast<f32x4*>(red + 16 * XT + o) = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (T4 > 0) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // (the wave's own zeros before its own values: same addresses)
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int q = 0; q < NT; ++q) {
          const f32x4 v = at[h][q] + atb[h][q];
          *reinterpret_cast<f32x4*>(red + (16 + 4 * q + (lane & 3)) * XT + 64 * h + 4 * (lane >> 2)) = v;
        }
    }
    __syncthreads();
    double* Pt = bt.P + (size_t)u * (XL * XT);
    const float* r0 = lds;
    for (int o = tid; o < XL * XT; o += NTH) {
      const double v = (double)r0[o] + (double)r0[XL * XT + o] + (double)r0[2 * XL * XT + o] + (double)r0[3 * XL * XT + o];
      __builtin_nontemporal_store(v, Pt + o);
    }
    return;
  }
  f32x16 acc[4], acc2[4];
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[b][r] = 0.f; acc2[b][r] = 0.f; }

  if (nch > 0) issue(0, 0);
  if (nch > 1) issue(1, 1);
  const int sw = l31 & 15;
  for (int c = 0; c < nch; ++c) {
    const int st = c & 1;
    if (c + 1 < nch) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");   // this wave's 10 pieces of chunk c have landed
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const float* ys = lds + st * XSTG;
    const float* xs = ys + XL * XK;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const int c16 = 4 * wave + 2 * s2 + lh;
      const int ko = 4 * (c16 ^ sw);
      const f32x4 fa = *reinterpret_cast<const f32x4*>(ys + l31 * XK + ko);
      f32x4 fb[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) fb[b] = *reinterpret_cast<const f32x4*>(xs + (32 * b + l31) * XK + ko);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[e], fb[b][e], acc[b], 0, 0, 0);
    }
    __syncthreads();   // every wave has read stage st for the last time
    if (c + 2 < nch) issue(c + 2, st);
    if ((c & (XFOLD - 1)) == XFOLD - 1) {
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        acc2[b] += acc[b];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
      }
    }
  }
  // ---- the four waves' partial tiles meet in LDS (64 KB of the 80), wave w finishes column block w
  float* red = lds;
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int q = 0; q < 16; ++q)
      red[wave * (XL * XT) + ((q & 3) + 8 * (q >> 2) + 4 * lh) * XT + 32 * b + l31] = acc[b][q] + acc2[b][q];
  __syncthreads();
  double* Pt = bt.P + (size_t)u * (XL * XT);
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int i = (q & 3) + 8 * (q >> 2) + 4 * lh;
    const int o = i * XT + 32 * wave + l31;
    const double v = (double)red[o] + (double)red[XL * XT + o] + (double)red[2 * XL * XT + o] + (double)red[3 * XL * XT + o];
    __builtin_nontemporal_store(v, Pt + o);
  }
}

// D[i][col] (+)= sum over the units of tile (col / 128) of their partial tiles
__global__ __launch_bounds__(128) void xty_small_reduce_kernel(XtyBatch bt, double* D64, int64_t ld64, int accumulate) {
  const int tile = blockIdx.x, i = blockIdx.y, jj = threadIdx.x;
  const int col = tile * XT + jj;
  if (i >= bt.nb || col >= bt.na) return;
  double s = 0.0;
  for (int j = 0; j < bt.nblocks; ++j)
    for (int sp = 0; sp < bt.nsplit[j]; ++sp)
      s += bt.P[(size_t)(bt.unit_begin[j] + sp * bt.ntiles + tile) * (XL * XT) + i * XT + jj];
  double* d = D64 + (int64_t)i * ld64 + col;
  *d = accumulate ? *d + s : s;
}

bool xty_small_ok(const float* const* X, const int64_t* ldx, const float* const* Y, const int64_t* ldy,
                  const int64_t* K, int nblocks, int64_t nb, int64_t na, const float* D32) {
  if (getenv("DMDX_NO_K3S")) return false;   // A/B knob
  if (D32 || nb > XL || na < XT) return false;
  for (int j = 0; j < nblocks; ++j) {
    if (K[j] < 8 * XK || ldx[j] % 4 || ldy[j] % 4 || !dmdx_aligned16(X[j]) || !dmdx_aligned16(Y[j])) return false;
    if (ldx[j] >= (int64_t(1) << 22) || ldy[j] >= (int64_t(1) << 22)) return false;
  }
  return true;
}

void xty_small_plan(const int64_t* K, int nb_, int ntiles, int* chunks, int* cps, int* nsplit, int* units) {
  int total = 0;
  for (int j = 0; j < nb_; ++j) {
    chunks[j] = (int)(K[j] / XK);
    int64_t want = (4 * 512 + (int64_t)ntiles * nb_ - 1) / ((int64_t)ntiles * nb_);   // ~4 rounds of 512 workgroups
    const int64_t maxs = chunks[j] / 16 > 0 ? chunks[j] / 16 : 1;
    if (want > maxs) want = maxs;
    if (want < 1) want = 1;
    // (the tail of the launch, as in make_plan: cfg2 at l = 20 is 69 tiles x 8 blocks x 4 splits = 4.31
    // rounds of 512 that cost 5; 12 splits are 12.94)
    want = fit_last_round(chunks[j], (int64_t)ntiles * nb_, want, std::min(maxs, 4 * want + 2));
    cps[j] = (int)((chunks[j] + want - 1) / want);
    // a block of fewer than 64 rows has no full chunk: no units here, all of it goes to the tail launch
    nsplit[j] = cps[j] > 0 ? (chunks[j] + cps[j] - 1) / cps[j] : 0;
    total += nsplit[j] * ntiles;
  }
  *units = total;
}

size_t xty_small_ws(const int64_t* K, int nblocks, int64_t na) {
  const int ntiles = (int)((na + XT - 1) / XT);
  size_t need = 0;
  for (int j0 = 0; j0 < nblocks; j0 += MAXB) {
    int ch[MAXB], cp[MAXB], ns[MAXB], units = 0;
    xty_small_plan(K + j0, group_len(nblocks, j0), ntiles, ch, cp, ns, &units);
    need = std::max(need, (size_t)units * XL * XT * sizeof(double));
  }
  return need;
}

int run_xty_small(const float* const* X, const int64_t* ldx, const float* const* Y, const int64_t* ldy,
                  const int64_t* K, int nblocks, int64_t nb, int64_t na, double* D64, int64_t ld64, int accumulate,
                  void* ws, hipStream_t stream) {
  const int ntiles = (int)((na + XT - 1) / XT);
  for (int j0 = 0; j0 < nblocks; j0 += MAXB) {
    const int ng = group_len(nblocks, j0);
    XtyBatch bt{};
    int units = 0;
    xty_small_plan(K + j0, ng, ntiles, bt.chunks, bt.cps, bt.nsplit, &units);
    int ub = 0;
    for (int j = 0; j < ng; ++j) {
      bt.X[j] = X[j0 + j];
      bt.Y[j] = Y[j0 + j];
      bt.ldx[j] = ldx[j0 + j];
      bt.ldy[j] = ldy[j0 + j];
      bt.unit_begin[j] = ub;
      ub += bt.nsplit[j] * ntiles;
    }
    bt.unit_begin[ng] = ub;
    bt.nblocks = ng;
    bt.ntiles = ntiles;
    bt.na = (int)na;
    bt.nb = (int)nb;
    bt.P = reinterpret_cast<double*>(ws);
    if (units > 0) {   // (a group of blocks that are all shorter than one chunk: the reduce kernel still defines D)
      // (16 + 4 T4 rows of MFMA work for nb <= 16 / 20 / 24; DMDX_K3S_32=1: the 32-row body for everything, A/B)
      const bool wide = nb > 24 || getenv("DMDX_K3S_32") != nullptr;
      if (wide) hipLaunchKernelGGL(xty_small_kernel<-1>, dim3((unsigned)units), dim3(NTH), 0, stream, bt);
      else if (nb <= 16) hipLaunchKernelGGL(xty_small_kernel<0>, dim3((unsigned)units), dim3(NTH), 0, stream, bt);
      else if (nb <= 20) hipLaunchKernelGGL(xty_small_kernel<1>, dim3((unsigned)units), dim3(NTH), 0, stream, bt);
      else hipLaunchKernelGGL(xty_small_kernel<2>, dim3((unsigned)units), dim3(NTH), 0, stream, bt);
      DMDX_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(xty_small_reduce_kernel, dim3((unsigned)ntiles, (unsigned)nb), dim3(XT), 0, stream, bt, D64, ld64,
                       (accumulate || j0 > 0) ? 1 : 0);
    DMDX_LAUNCH_CHECK();
  }
  // rows past the last full 64-row chunk of every block: the generic path, accumulated on top (one split
  // per block: its partial tiles fit into what batch_ws asks for the whole blocks)
  std::vector<const float*> Xt, Yt;
  std::vector<int64_t> lx, ly, Kt;
  for (int j = 0; j < nblocks; ++j) {
    const int64_t tail = K[j] % XK;
    if (tail == 0) continue;
    Xt.push_back(X[j] + (K[j] - tail));
    Yt.push_back(Y[j] + (K[j] - tail));
    lx.push_back(ldx[j]);
    ly.push_back(ldy[j]);
    Kt.push_back(tail);
  }
  if (!Kt.empty())
    return run_batch(Yt.data(), ly.data(), Xt.data(), lx.data(), Kt.data(), (int)Kt.size(), nb, na, 0, D64, ld64, nullptr,
                     0, 1, ws, stream, true);
  return 0;
}

// A call that runs as several launches (row split, groups of 16 blocks, K3s + its tail launch) checks
// everything BEFORE the first one: a refused call leaves the outputs and the workspace untouched, and the
// launch paths above check nothing.  (Per-launch checks used to fire between launches: a group of blocks
// behind the first 16 with a larger plan or a too long leading dimension left C half accumulated.)
// ld_limit: the per-lane offsets inside a 128-column panel are 32-bit: elements on the register path
// (127 columns: ld < 2^25), bytes (+ 4 KiB of slack) on the LDS-DMA path (taken for ld < 2^22).  The blocks
// entry points promise less, 2^24 per block; include/dmdx.h states both limits and neither moves here.
int tn_refusal(const char* who, const int64_t* lda, const int64_t* ldb, int nblocks, int64_t ld_limit,
               const void* ws, size_t ws_bytes, size_t need) {
  for (int j = 0; j < nblocks; ++j)
    if (lda[j] >= ld_limit || ldb[j] >= ld_limit) {
      dmdx_set_error("%s: leading dimension %lld / %lld >= %lld not supported (use smaller row blocks)", who,
                     (long long)lda[j], (long long)ldb[j], (long long)ld_limit);
      return DMDX_E_UNSUPPORTED;
    }
  if (ws == nullptr || ws_bytes < need) {
    dmdx_set_error("%s: workspace %zu bytes < required %zu", who, ws_bytes, need);
    return DMDX_E_WORKSPACE;
  }
  return 0;
}
#define DMDX_REFUSE_BEFORE_LAUNCH(expr) \
  do {                                  \
    if (const int rc_ = (expr)) return rc_; \
  } while (0)
constexpr int64_t LD_LIMIT_SINGLE = int64_t(1) << 25, LD_LIMIT_BLOCKS = int64_t(1) << 24;

// D rows beyond one 128-row tile (l > 128 columns of Y in Z = X^T Y): the full 128-row tiles in one
// launch, the remaining rows in a second one with the tile height that pads least (64 / 96) -- when
// that is less MFMA work than any uniform tile height (l = 220: 128 + 96 = 224 rows instead of
// 256).  The second launch streams the big operand once more; these products are MFMA-bound by a
// factor > 3 at such l, so the extra HBM pass is hidden.  Returns the split row, or 0.
int64_t tn_row_split(int64_t nrow) {
  if (nrow <= BT) return 0;
  const int64_t full = nrow / BT * BT, rem = nrow - full;
  if (rem == 0 || rem > 112) return 0;
  const int64_t rem_pad = rem <= 32 ? 32 : (rem + 15) / 16 * 16;
  int64_t best = (nrow + BT - 1) / BT * BT;
  for (int tm : {112, 96, 80, 64}) {
    const int64_t padded = (nrow + tm - 1) / tm * tm;
    if (padded < best) best = padded;
  }
  return full + rem_pad < best ? full : 0;
}

// K3, C (na x nb, column-major) (+)= sum_j A_j^T B_j: workspace and launches, with the row split.
// column-major C[a + b*ldc] == row-major D[b][a]: D rows <- B columns, D cols <- A columns
size_t product_ws(const int64_t* K, int nblocks, int64_t na, int64_t nb) {
  if (const int64_t cut = tn_row_split(nb))
    return std::max(batch_ws(K, nblocks, cut, na, 0), batch_ws(K, nblocks, nb - cut, na, 0));
  return batch_ws(K, nblocks, nb, na, 0);
}

int run_product(const float* const* A, const int64_t* lda, const float* const* B, const int64_t* ldb,
                const int64_t* K, int nblocks, int64_t na, int64_t nb, double* C64, int64_t ldc, float* C32,
                int64_t ldc32, int accumulate, void* ws, hipStream_t stream, bool probe) {
  const int64_t cut = tn_row_split(nb);
  if (cut == 0)
    return run_batch(B, ldb, A, lda, K, nblocks, nb, na, 0, C64, ldc, C32, ldc32, accumulate, ws, stream, probe);
  if (const int rc = run_batch(B, ldb, A, lda, K, nblocks, cut, na, 0, C64, ldc, C32, ldc32, accumulate, ws, stream, probe))
    return rc;
  std::vector<const float*> B2((size_t)nblocks);
  for (int j = 0; j < nblocks; ++j) B2[j] = B[j] + cut * ldb[j];
  return run_batch(B2.data(), ldb, A, lda, K, nblocks, nb - cut, na, 0, C64 + cut * ldc, ldc,
                   C32 ? C32 + cut * ldc32 : nullptr, ldc32, accumulate, ws, stream, probe);
}

}  // namespace

extern "C" {

#ifdef DMDX_STAMPS
int dmdx_debug_read_stamps(unsigned long long* out8, int reset) {
  hipError_t e = hipMemcpyFromSymbol(out8, HIP_SYMBOL(dmdx_stamp), 12 * sizeof(unsigned long long));   // (12 entries)
  if (reset) {
    unsigned long long z[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(dmdx_stamp), z, sizeof(z));
  }
  return (int)e;
}
#endif

int dmdx_set_clock_probe(unsigned long long* dev_counters3) {
  dmdx_clock_probe_ptr = dev_counters3;
  return 0;
}

size_t dmdx_syrk_workspace_bytes(int64_t m, int64_t n) {
  if (m < 0 || n <= 0) return 0;
  return batch_ws(&m, 1, n, n, 1);
}

int dmdx_syrk_f32(const float* X, int64_t m, int64_t n, int64_t ldx, double* G64, int64_t ldg,
                  float* G32, int64_t ldg32, int accumulate, void* workspace,
                  size_t workspace_bytes, void* stream) {
  DMDX_CHECK_ARG(X && G64, "syrk: null pointer");
  DMDX_CHECK_ARG(m >= 1 && n >= 1 && n < (1 << 30), "syrk: bad shape m=%lld n=%lld", (long long)m,
                 (long long)n);
  DMDX_CHECK_ARG(ldx >= 1 && ldg >= n && (!G32 || ldg32 >= n), "syrk: bad leading dimension");
  DMDX_REFUSE_BEFORE_LAUNCH(tn_refusal("syrk", &ldx, &ldx, 1, LD_LIMIT_SINGLE, workspace, workspace_bytes,
                                       dmdx_syrk_workspace_bytes(m, n)));
  return run_batch(&X, &ldx, &X, &ldx, &m, 1, n, n, 1, G64, ldg, G32, ldg32, accumulate, workspace,
                   (hipStream_t)stream, false);
}

size_t dmdx_syrk_blocks_workspace_bytes(const int64_t* m, int nblocks, int64_t n) {
  if (!m || nblocks <= 0 || n <= 0) return 0;
  for (int j = 0; j < nblocks; ++j)
    if (m[j] < 1) return 0;
  return batch_ws(m, nblocks, n, n, 1);
}

int dmdx_syrk_blocks_f32(const float* const* X, const int64_t* m, const int64_t* ldx, int nblocks, int64_t n,
                         double* G64, int64_t ldg, float* G32, int64_t ldg32, int accumulate,
                         void* workspace, size_t workspace_bytes, void* stream) {
  DMDX_CHECK_ARG(X && m && ldx && G64 && nblocks >= 1, "syrk_blocks: null pointer or no blocks");
  DMDX_CHECK_ARG(n >= 1 && n < (1 << 30) && ldg >= n && (!G32 || ldg32 >= n), "syrk_blocks: bad n / ldg");
  for (int j = 0; j < nblocks; ++j)
    DMDX_CHECK_ARG(X[j] && m[j] >= 1 && ldx[j] >= 1, "syrk_blocks: bad block %d", j);
  DMDX_REFUSE_BEFORE_LAUNCH(tn_refusal("syrk_blocks", ldx, ldx, nblocks, LD_LIMIT_BLOCKS, workspace, workspace_bytes,
                                       dmdx_syrk_blocks_workspace_bytes(m, nblocks, n)));
  return run_batch(X, ldx, X, ldx, m, nblocks, n, n, 1, G64, ldg, G32, ldg32, accumulate, workspace,
                   (hipStream_t)stream, true);
}

size_t dmdx_syrk_planes_bytes(const int64_t* m, int nblocks, int64_t n) { return plane_image::total_bytes(m, nblocks, n); }

// Every LDS-DMA address of the plane-fed pass (tn_unit_planes: the groups 2 c_begin .. 2 c_end - 1 of the unit's two
// panels, 12 288 bytes each) lies in [0, planes_bytes), block j's first image at off[j]: walked on the host over the
// plan the launch will use, first and last panel, every K-split.  Not an independent bound per block: it recomputes
// make_plan and group_offset as the kernel does, so what it can catch is a plan whose chunks or panels are not those
// the images were sized with, and a buffer shorter than the blocks' sum.
static bool planes_dma_inside(const int64_t* m, int nblocks, int64_t n, const size_t* off, size_t planes_bytes) {
  for (int j0 = 0; j0 < nblocks; j0 += MAXB) {
    const int nb = group_len(nblocks, j0);
    for (int j = j0; j < j0 + nb; ++j) {
      const Plan pl = make_plan(m[j], n, n, 1, nb);
      if (pl.chunks_total != plane_image::chunks_of(m[j]) || pl.ntr != plane_image::panels_of(n)) return false;
      for (const int64_t pn : {(int64_t)0, (int64_t)pl.ntr - 1})
        for (int s = 0; s < pl.nsplit; ++s) {
          const int64_t cb = (int64_t)s * pl.chunks_per_split, ce = std::min<int64_t>(cb + pl.chunks_per_split, pl.chunks_total);
          if (ce <= cb) continue;
          const int64_t first = plane_image::group_offset(pn, pl.chunks_total, 2 * cb);
          const int64_t end = plane_image::group_offset(pn, pl.chunks_total, 2 * ce - 1) + plane_image::kHalfBytes;
          if (first < 0 || end < first || off[j] > planes_bytes || (size_t)end > planes_bytes - off[j]) return false;
        }
    }
  }
  return true;
}

int dmdx_syrk_blocks_planes_f32(const float* const* X, const int64_t* m, const int64_t* ldx, int nblocks, int64_t n,
                                double* G64, int64_t ldg, float* G32, int64_t ldg32, int accumulate, void* workspace,
                                size_t workspace_bytes, void* planes, size_t planes_bytes, void* stream) {
  DMDX_CHECK_ARG(X && m && ldx && G64 && nblocks >= 1, "syrk_blocks_planes: null pointer or no blocks");
  DMDX_CHECK_ARG(n >= 1 && n < (1 << 30) && ldg >= n && (!G32 || ldg32 >= n), "syrk_blocks_planes: bad n / ldg");
  for (int j = 0; j < nblocks; ++j)
    DMDX_CHECK_ARG(X[j] && m[j] >= 1 && ldx[j] >= 1, "syrk_blocks_planes: bad block %d", j);
  const size_t ws_need = dmdx_syrk_blocks_workspace_bytes(m, nblocks, n);
  DMDX_REFUSE_BEFORE_LAUNCH(tn_refusal("syrk_blocks_planes", ldx, ldx, nblocks, LD_LIMIT_BLOCKS, workspace, workspace_bytes,
                                       ws_need));
  // the plane buffer: present, large enough for every block (a size that saturated fits nothing), and apart from
  // everything else the call reads or writes
  const size_t need = dmdx_syrk_planes_bytes(m, nblocks, n);
  if (planes == nullptr || need == SIZE_MAX || planes_bytes < need) {
    dmdx_set_error("syrk_blocks_planes: plane buffer %zu bytes < required %zu", planes ? planes_bytes : (size_t)0, need);
    return DMDX_E_WORKSPACE;
  }
  DMDX_CHECK_ARG(((uintptr_t)planes & 15u) == 0, "syrk_blocks_planes: the plane buffer is not 16-byte aligned");
  bool apart = plane_image::disjoint(planes, need, workspace, ws_need) &&
               plane_image::disjoint(planes, need, G64, sizeof(double) * (size_t)((n - 1) * ldg + n)) &&
               (!G32 || plane_image::disjoint(planes, need, G32, sizeof(float) * (size_t)((n - 1) * ldg32 + n)));
  for (int j = 0; j < nblocks; ++j)   // (ldx < 2^24, n < 2^30: the extent fits 64 bits)
    apart = apart && plane_image::disjoint(planes, need, X[j], sizeof(float) * (size_t)((n - 1) * ldx[j] + m[j]));
  DMDX_CHECK_ARG(apart, "syrk_blocks_planes: the plane buffer overlaps X, G or the workspace");
  // the plane-fed pass takes what the aligned plane k-step takes today; anything else runs as dmdx_syrk_blocks_f32
  // does and leaves the planes untouched
  bool fed = n > 96 && !k1_arith_f32();
  for (int j = 0; j < nblocks && fed; ++j) fed = tn_block_aligned(X[j], ldx[j]) && dmdx_plane_split_fits(m[j], n);
  std::vector<size_t> off((size_t)nblocks);
  std::vector<const unsigned char*> img((size_t)nblocks);
  size_t at = 0;
  for (int j = 0; j < nblocks; ++j) {
    off[j] = at;
    img[j] = reinterpret_cast<const unsigned char*>(planes) + at;
    at += plane_image::block_bytes(m[j], n);
  }
  if (fed && !planes_dma_inside(m, nblocks, n, off.data(), planes_bytes)) {
    dmdx_set_error("syrk_blocks_planes: the unit plan reaches outside the plane buffer");
    return DMDX_E_INVALID;
  }
  if (!fed)
    return run_batch(X, ldx, X, ldx, m, nblocks, n, n, 1, G64, ldg, G32, ldg32, accumulate, workspace,
                     (hipStream_t)stream, true);
  for (int j = 0; j < nblocks; ++j)
    if (const int rc = dmdx_plane_split_launch(X[j], m[j], n, ldx[j], const_cast<unsigned char*>(img[j]), (hipStream_t)stream))
      return rc;
  return run_batch(X, ldx, X, ldx, m, nblocks, n, n, 1, G64, ldg, G32, ldg32, accumulate, workspace,
                   (hipStream_t)stream, true, img.data());
}

size_t dmdx_gemm_tn_workspace_bytes(int64_t K, int64_t na, int64_t nb) {
  if (K < 0 || na <= 0 || nb <= 0) return 0;
  return product_ws(&K, 1, na, nb);
}

int dmdx_gemm_tn_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t K,
                     int64_t na, int64_t nb, double* C64, int64_t ldc, float* C32, int64_t ldc32,
                     int accumulate, void* workspace, size_t workspace_bytes, void* stream) {
  DMDX_CHECK_ARG(A && B && C64, "gemm_tn: null pointer");
  DMDX_CHECK_ARG(K >= 1 && na >= 1 && nb >= 1 && na < (1 << 30) && nb < (1 << 30),
                 "gemm_tn: bad shape");
  DMDX_CHECK_ARG(lda >= 1 && ldb >= 1 && ldc >= na && (!C32 || ldc32 >= na),
                 "gemm_tn: bad leading dimension");
  DMDX_REFUSE_BEFORE_LAUNCH(tn_refusal("gemm_tn", &lda, &ldb, 1, LD_LIMIT_SINGLE, workspace, workspace_bytes,
                                       dmdx_gemm_tn_workspace_bytes(K, na, nb)));
  // (never the small-l kernel: svd._accumulate_tn relies on the generic body here)
  return run_product(&A, &lda, &B, &ldb, &K, 1, na, nb, C64, ldc, C32, ldc32, accumulate, workspace,
                     (hipStream_t)stream, false);
}

size_t dmdx_gemm_tn_blocks_workspace_bytes(const int64_t* K, int nblocks, int64_t na, int64_t nb) {
  if (!K || nblocks <= 0 || na <= 0 || nb <= 0) return 0;
  for (int j = 0; j < nblocks; ++j)
    if (K[j] < 1) return 0;
  size_t need = product_ws(K, nblocks, na, nb);
  if (nb <= XL && na >= XT) need = std::max(need, xty_small_ws(K, nblocks, na));   // K3s has its own partial tiles
  return need;
}

int dmdx_gemm_tn_blocks_f32(const float* const* A, const int64_t* lda, const float* const* B,
                            const int64_t* ldb, const int64_t* K, int nblocks, int64_t na, int64_t nb,
                            double* C64, int64_t ldc, float* C32, int64_t ldc32, int accumulate,
                            void* workspace, size_t workspace_bytes, void* stream) {
  DMDX_CHECK_ARG(A && B && lda && ldb && K && C64 && nblocks >= 1, "gemm_tn_blocks: null pointer or no blocks");
  DMDX_CHECK_ARG(na >= 1 && nb >= 1 && na < (1 << 30) && nb < (1 << 30) && ldc >= na && (!C32 || ldc32 >= na),
                 "gemm_tn_blocks: bad shape / ldc");
  for (int j = 0; j < nblocks; ++j)
    DMDX_CHECK_ARG(A[j] && B[j] && K[j] >= 1 && lda[j] >= 1 && ldb[j] >= 1, "gemm_tn_blocks: bad block %d", j);
  DMDX_REFUSE_BEFORE_LAUNCH(tn_refusal("gemm_tn_blocks", lda, ldb, nblocks, LD_LIMIT_BLOCKS, workspace, workspace_bytes,
                                       dmdx_gemm_tn_blocks_workspace_bytes(K, nblocks, na, nb)));
  if (xty_small_ok(A, lda, B, ldb, K, nblocks, nb, na, C32))
    return run_xty_small(A, lda, B, ldb, K, nblocks, nb, na, C64, ldc, accumulate, workspace, (hipStream_t)stream);
  return run_product(A, lda, B, ldb, K, nblocks, na, nb, C64, ldc, C32, ldc32, accumulate, workspace,
                     (hipStream_t)stream, true);
}

}  // extern "C"
