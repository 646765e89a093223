/*
 * dmdx.h -- C ABI of libdmdx.so, the MI355X (gfx950) kernels behind the
 * ERA5 snapshot-matrix SVD hot path.
 *
 * What it replaces in the reference (ClimeTrend/DMD-ERA5, paths relative to
 * the reference root): the reference has no FFI; its hot loop is two
 * third-party CPU calls made from
 *     src/dmd_era5/era5_svd/era5_svd.py:251   np.linalg.svd(X, full_matrices=False)
 *     src/dmd_era5/era5_svd/era5_svd.py:258   sklearn randomized_svd(X, n_components)
 * plus the pre-processing passes that build X
 *     src/dmd_era5/slice_tools/slice_tools.py:171-179  (mean / std / centre / scale)
 *     src/dmd_era5/slice_tools/slice_tools.py:207-211  (delay embedding)
 * Each entry point below names the reference line whose arithmetic it takes
 * over.  The Python host (dmd_era5_amd/) binds these with ctypes and keeps the
 * reference's function signatures (svd_on_era5, main, ...).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless named host_*;
 *   - matrices are COLUMN-MAJOR with a leading dimension in elements,
 *     (ptr, rows, cols, ld); rows > ld is allowed for the input X only: that is
 *     the zero-copy delay-embedding view E[k*m+s, t] = X[s, t+k] = ptr[(k*m+s) + t*ld]
 *     with ld = m (slice_tools.py:207-211);
 *   - stream is a hipStream_t passed as void* (NULL = default stream);
 *   - calls enqueue work on `stream` and return; no hidden synchronisation,
 *     no allocation (workspaces are caller-provided);
 *   - return value 0 = ok, < 0 = error (-(hipError_t) or DMDX_E_*);
 *     dmdx_last_error() gives the message for the calling thread.
 *
 * Memory contract (tests/test_gpu_memory_edges.py holds every entry point to it)
 *   - only the logical rows x cols elements of an operand take part: the ld - rows elements behind
 *     every column, the rows past K and whatever lies before or behind a matrix are never used for
 *     a result (they may hold NaN) and never written -- also by the in-place kernels (K5,
 *     dmdx_scale_columns_f32) and for outputs with a leading dimension larger than the matrix
 *     (ldg, ldg32, ldc, ldc32, ldy, ldgd, ldv, ldz, ldl, ldi);
 *   - with accumulate == 0 every logical element of an output is written and none is read;
 *   - a workspace needs no initialisation, `*_workspace_bytes` is sufficient, and nothing is
 *     written behind it; K7L / K10 zero their barrier words themselves;
 *   - a call that is refused (DMDX_E_*) has written nothing, even when it would have run as
 *     several launches (groups of 16 blocks, the row split of K3);
 *   - alignment: NO fp32 entry point requires one.  16-byte aligned bases with leading dimensions
 *     that are multiples of 4 select the fast paths -- K1 / K3: LDS-DMA staging (all operands of a
 *     launch, ld < 2^22; K3s also wants K >= 512 per block and no fp32 copy); K2: 16-byte loads and
 *     stores (X, W, Y, and m % 4 == 0); K5: the tiled float4 kernel (X) -- everything else takes
 *     the register / scalar paths with the same results to rounding.  K % 4 and n % 4 are free.
 *     The fp64 MFMA kernels K8 / K9 / K11 REQUIRE what their comments state (even widths and
 *     leading dimensions of the inputs, 16-byte aligned inputs and workspace) and return
 *     DMDX_E_INVALID otherwise; their outputs and K6 / K7 / K7L / K10 take any leading dimension;
 *   - leading dimensions of K1 / K3 operands: < 2^25 on the single entry points, < 2^24 per block
 *     on the blocks entry points, DMDX_E_UNSUPPORTED beyond; K2: m + 4 ldx < 2^29
 *     (DMDX_E_INVALID beyond);
 *   - K12 (dmdx_expand_f32, dmdx_expand_score_f32): U, C, mu, sigma and X are only read, inside their
 *     logical elements (U: m x k, C: k x T, X: m x T with rows > ldx allowed); every logical element of
 *     Xhat, sse_row and -- with accumulate == 0 -- sse_col / ref_col is written, nothing else.  Xhat, X,
 *     U, mu and sigma are addressed with 64-bit offsets and one dword per lane: no alignment is asked
 *     for and none selects another path; a 16-byte aligned C with ldc % 4 == 0 is staged with 16-byte
 *     loads.  m, T and every leading dimension must be < 2^31 (DMDX_E_INVALID beyond, before anything
 *     is written);
 *   - K13 (dmdx_project_f32): U, X, mu and sigma are only read, inside their logical elements (U: m x k,
 *     X: m x T with rows > ldx allowed); every logical element of C (k x T, ldc) and -- when given -- of
 *     energy is written with accumulate == 0 and read and written with accumulate != 0, nothing else.  No
 *     alignment is asked for: a 16-byte aligned U with ldu % 4 == 0, X with ldx % 4 == 0, mu, sigma each
 *     select 16-byte loads for that operand, anything else one dword per lane with the same values.  m, T
 *     and every leading dimension must be < 2^31 (DMDX_E_INVALID beyond, before anything is written);
 *   - K15 (dmdx_spread_f32, dmdx_spread_score_f32): U, D and sigma are only read, inside their logical elements
 *     (U: m x k, D: k x (B T), column b T + t = member b at snapshot t); every logical element of S, var_row and
 *     -- with accumulate == 0 -- var_col is written, nothing else.  S, U and sigma are addressed with 64-bit
 *     offsets and one dword per lane: no alignment is asked for and none selects another path; a 16-byte aligned D
 *     with ldd % 4 == 0 is staged with 16-byte loads, with identical values.  m, T, B T and every leading
 *     dimension must be < 2^31 (DMDX_E_INVALID beyond, before anything is written);
 *   - K19 (dmdx_crps_f32): U, C (k x (B T)), mu, sigma, X and w are only read, inside their logical elements; every
 *     logical element of row and -- with accumulate == 0 -- of col and hist is written, nothing else; addressing
 *     and alignment as K15;
 *   - K24 (dmdx_exceed_prob_f32, dmdx_exceed_score_f32): as K19, with thr (m x (J S)) and slot (T) only read, inside
 *     their logical elements and, for thr, only in the columns slot names; every logical element of the J planes of
 *     P, of row and -- with accumulate == 0 -- of col and cnt is written, nothing else.
 *   - K31 (dmdx_gap_mask_f32, dmdx_gap_standardize_f32, dmdx_gap_fill_f32): the mask W is ceil(T / 32) columns of m
 *     uint32 words (ldw); the delay view (rows > ldx) is refused by all three.  mask: X is only read, every logical
 *     word of W and -- when given -- every element of nmiss and sums is written, nothing else.  standardize: every
 *     logical element of X is read and written, W, mu and sigma are only read.  fill: U, C, mu, sigma and W are only
 *     read, inside their logical elements; X is read (only when change_row is given) and written EXACTLY at the
 *     elements whose bit is set, with row < m and snapshot < T: an element with a clear bit is neither read nor
 *     written, the bits of the last word from snapshot T on are ignored; every element of change_row is written.  No
 *     alignment is asked for: a 16-byte aligned X with ldx % 4 == 0 selects 16-byte accesses in mask and standardize, a
 *     16-byte aligned C with ldc % 4 == 0 16-byte staging in fill, with the same bits.
 *
 * Value contract (tests/test_gpu_value_domain.py holds every fp32 entry point to it)
 *   - NaN / Inf propagate like IEEE arithmetic on the logical operands, nothing more and nothing less:
 *     the class (finite / NaN / +Inf / -Inf) of every output element is the one numpy's fp64 product of
 *     the same fp32 inputs has, and an output element a non-finite input element does not take part in
 *     is bit-identical to the result without it.  K1 (single and blocks): X[i, j] non-finite makes row
 *     and column j of G (G[j, j] included) non-finite; K3 / K3 blocks / K3s: an element of A hits one
 *     row of C, an element of B one column; K2: X[i, k] hits row i of Y, W[k, c] column c, and the
 *     fused Gram is non-finite exactly where Y^T Y is; the fp32 copies (G32, C32) have the class of the
 *     fp64 result.  Clamped addresses (rows past m, columns past n or l, padded 16-column granules)
 *     never carry a value into a result: where a clamped duplicate would meet a zero pad it is replaced
 *     by zero (Inf * 0 would be NaN).  The host relies on this: it raises LinAlgError when diag(G) or
 *     the range-finder iterate Z is not finite (svd.py) instead of iterating on NaN.  K5: a NaN in row i
 *     makes mean[i], std[i] and row i NaN and leaves every other row alone, also the three others of
 *     its float4.  The small fp64 solvers (K7, K7L, K10) are only called with finite input;
 *     K12: U[i, j] hits row i of Xhat, C[j, t] column t, mu[i] / sigma[i] row i; k is padded to a
 *     multiple of 16 with zeros in U AND in C (0 * 0), so an Inf in the last column of U meets no pad.  In
 *     the score a non-finite X[i, t] makes exactly sse_col[t], ref_col[t] and sse_row[i] non-finite, and
 *     a non-finite Xhat[i, t] does the same to sse_col[t] and sse_row[i];
 *     K13: X[i, t] hits column t of C and energy[t], U[i, j] row j of C, mu[i] / sigma[i] (sigma[i] = 0
 *     included: xt = +-Inf or NaN) every energy and every C[j, t] with the class of numpy's fp64
 *     U^T ((X - mu) / sigma); rows past m, snapshots past T and columns past k are zeros on both sides;
 *   - a CONSTANT row under K5 with scale: mean[i] is the constant exactly, std[i] is exactly 0 and the
 *     row becomes 0 / 0 = NaN, as numpy's (x - mean) / std of the reference's standardize_data does
 *     (slice_tools.py:171-179).  That is the contract, not an accident: the SVD that follows raises
 *     LinAlgError, it never returns factors of such a matrix.  (The ingest's all-zero filler rows are
 *     kept away from K5 by the host for this reason.)  Without scale the row becomes exactly 0;
 *   - magnitudes: the kernels are correct for |x| in [2^-40, 2^40] (products 2^-80 .. 2^80, sums of 2^20
 *     and more of them stay inside fp32; subnormals are not flushed), which is what the host's magnitude
 *     guard hands them: it rescales by a power of two only when max|x| leaves that interval.  Inside it a
 *     power-of-two factor commutes with every rounding: K1 / K3 of 2^e X equal 2^2e times the result for
 *     X bit for bit, K2 of 2^e X gives 2^e Y and 2^2e G.  All-positive (un-centred) data keep the error
 *     bound of one fp32 chain of at most 4096 rows + a blocked fp32 sum of at most 16 chain results + fp64
 *     beyond: ((min(K, 4096) / 2 + 18) 2^-24) sum |a||b|, whatever K is.  K1 for n > 96 forms the products from
 *     three bf16 planes per value on the bf16 matrix core and has a bound of its own, (c + 26) 2^-24 sum |a||b|
 *     with c the chunks of 32 rows per work unit (at most 2048 unless DMDX_TN_MAX_CPS raises it): c - 1 rounded
 *     fp32 adds of the chunk results, 13 for the 12 matrix instructions of a chunk (each rounds its sum and
 *     cuts it five to six bits below the ulp first: (1 + 2^-4) 2^-24), 8 for the three dropped plane products
 *     (at most 2^-21 |a||b| a pair), 2 for the fp32 copy and the fp64 sums, 4 to spare.  At c = 2048 that is
 *     8 units of 2^-24 above the fp32 bodies' bound and inside what the tests hold both to (1.01 times
 *     (2048 + 18) 2^-24); DMDX_K1_ARITH=f32 selects the fp32 products.  The class rule of the plane products
 *     (Inf times a non-zero value stays Inf) needs the partner's leading plane to be non-zero: normal fp32
 *     partners, which the magnitude interval above guarantees; a subnormal partner below 2^-133 truncates to
 *     a zero plane and gives NaN where numpy has Inf;
 *   - small integers are exact: while a_A a_B K < 2^24 for operands with integer entries |a| <= a_A,
 *     |b| <= a_B (K2: n a_X a_W < 2^24; its fused Gram: max|y|^2 m < 2^24) every partial sum is an
 *     exactly representable integer in any order, and K1 / K3 / K2 return the integer result bit for bit
 *     in fp64 and in the fp32 copy -- a dropped, repeated or clamped row anywhere in millions of rows
 *     changes the result.  K5 on integer rows with an integer mean: mean and the centred rows are exact,
 *     std is the fp64 root rounded to fp32, the scaled row is the correctly rounded fp32 quotient (the
 *     library is built without fast-math flags).  K6 / K8 / K9 / K11 are exact below 2^53.
 *     K12: k a_U a_C < 2^24 gives the integer U C bit for bit, and with integer sigma, mu and X (every
 *     intermediate below 2^24) Xhat, sse_col, ref_col and sse_row are the integer results; a power-of-two
 *     factor on U and its inverse on C leave every output bit unchanged (magnitudes as above).
 *     K13: xt = fl(fl(X - mu) / sigma) is bit for bit what K5 leaves in place for the same mean and std.  With
 *     integer U, mu, X, sigma a power of two dividing X - mu and m a_U a_xt < 2^24 (energy: a_xt^2 times the rows
 *     of a row range < 2^24) C and energy are the integer results bit for bit.  (2^e X, 2^e mu, 2^e sigma) leaves
 *     every bit of C and energy unchanged, 2^e U gives exactly 2^e C.  Error: one fp32 chain of at most
 *     DMDX_PROJECT_FP32_ROWS rows per row range, fp64 across: (DMDX_PROJECT_FP32_ROWS + 4) 2^-24 sum |u||xt|.
 *     K15: a non-finite D[j, b T + t] makes exactly column t of S non-finite, and with it var_col[t] and every
 *     var_row[i]; a non-finite U[i, j] or sigma[i] hits row i of S only (and var_row[i], every var_col).  The class
 *     is NaN where numpy's fp64 evaluation of |sigma| sqrt(sum_b (U D_b)^2) is NaN and +Inf where it is +Inf; every
 *     element not involved is bit-identical to the result without the non-finite value.  S is never negative and
 *     never -0.  k is padded with zeros in U AND in D, as in K12, and the k order of the chain is K12's: with B = 1
 *     and normal magnitudes sqrt(fl(a^2)) = |a| exactly (the root is correctly rounded: no fast-math), so S is bit
 *     for bit |Xhat| of dmdx_expand_f32(U, D, mu = NULL, sigma).  Integer U and D with every P_b^2 summed below 2^24
 *     and sigma a power of two give the integer V, var_col and var_row bit for bit (S = |sigma| sqrt(V) correctly
 *     rounded); (2^e U, 2^-e D) leaves every output bit unchanged (magnitudes as above).
 *     K31: a gap is an element whose exponent bits are all ones (every NaN payload, +-Inf); denormals, +-0 and
 *     +-FLT_MAX are finite.  mask: nmiss and sums of row i depend on row i alone, and sums are always finite for fp32
 *     input (fp64 sums of at most 2^31 finite fp32 values and squares).  standardize forward: a set bit gives +0.0
 *     whatever X holds; a clear bit gives fl(fl(x - mu) / sigma), K13's xt (sigma[i] = 0: +-Inf or NaN in row i alone).
 *     fill is K12 restricted to the set bits: the stored value is bit for bit what dmdx_expand_f32 stores there, so a
 *     non-finite U[i, j], mu[i] or sigma[i] reaches exactly the set-bit elements of row i and change_row[i], a
 *     non-finite C[j, t] the set-bit elements of column t and the change_row of their rows; a non-finite old value at a
 *     set bit makes change_row[i] non-finite and nothing else.  A tile or workgroup without a set bit is skipped and
 *     contributes exact +0.0.  Integer U, C, mu, sigma and X with every intermediate below 2^24 give the integer
 *     change_row bit for bit.
 */
#ifndef DMDX_H
#define DMDX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DMDX_VERSION 110 /* 0.1.1 */

#define DMDX_E_INVALID (-1000)  /* bad argument (shape, ld, null pointer)  */
#define DMDX_E_WORKSPACE (-1001) /* workspace too small                      */
#define DMDX_E_UNSUPPORTED (-1002)

int dmdx_version(void);
const char* dmdx_last_error(void);

/* ---- K1: Gram matrix G = X^T X  (method of snapshots) ---------------------
 * Takes over the O(m n^2) part of np.linalg.svd (era5_svd.py:251).
 * X: m x n fp32 (ldx), G64: n x n fp64 (ldg), both triangles written.
 * G32 (nullable): fp32 copy of G (ldg32).
 * accumulate != 0: G64 += X^T X (G32, if given, receives the rounded new G64): the
 * snapshot matrix is kept in HBM as row (space) blocks with a short leading
 * dimension -- a 4 MB column stride makes every 128-byte access of a 128-column
 * panel hit a different 2 MB page and thrashes the TLB -- and the Gram is summed
 * over the blocks in fp64.
 * fp32 MFMA products, fp32 chains of at most 4096 rows, fp64 across chains.
 * Deterministic (no atomics).  */
size_t dmdx_syrk_workspace_bytes(int64_t m, int64_t n);
int dmdx_syrk_f32(const float* X, int64_t m, int64_t n, int64_t ldx,
                  double* G64, int64_t ldg, float* G32, int64_t ldg32, int accumulate,
                  void* workspace, size_t workspace_bytes, void* stream);

/* K1 over a list of row blocks in ONE launch per 16 blocks:  G (+)= sum_j X_j^T X_j.
 * X, m, ldx: HOST arrays of nblocks device pointers / row counts / leading dimensions (block j is
 * m[j] x n, column-major, ldx[j]); everything else as dmdx_syrk_f32.  Same arithmetic per block;
 * the K-splits of all blocks are summed by one reduce kernel.  Replaces the per-block loop of
 * launches (last partial round of units, reduce kernel and launch gap per block). */
size_t dmdx_syrk_blocks_workspace_bytes(const int64_t* m, int nblocks, int64_t n);
int dmdx_syrk_blocks_f32(const float* const* X, const int64_t* m, const int64_t* ldx, int nblocks,
                         int64_t n, double* G64, int64_t ldg, float* G32, int64_t ldg32,
                         int accumulate, void* workspace, size_t workspace_bytes, void* stream);

/* The same Gram with the bf16 planes of X made ONCE per call instead of in every tile (K1's full 128 x 128 tiles
 * split every fp32 value into three bf16 planes; a value is staged by about 138 wave passes per call at n = 8760).
 * A streaming kernel writes the planes of every block into `planes` (images of 128 columns x 32 rows x 3 planes:
 * csrc/plane_image.h), K1's fast pass reads its MFMA operands from them.  Same planes, same MFMAs in the same order,
 * same folds: G64 and G32 are those of dmdx_syrk_blocks_f32 in every bit, non-finite input included (a work unit whose
 * result holds a NaN runs again from X on the class-safe planes, in a second launch over the marked units).
 * dmdx_syrk_planes_bytes: sum over the blocks of ceil(n / 128) ceil(m[j] / 32) 24 576 bytes; 0 for a bad argument,
 * SIZE_MAX where the sum does not fit.  planes: a device buffer of at least that many bytes, 16-byte aligned, apart
 * from X, G64, G32 and the workspace; its contents after the call are unspecified.  The workspace is that of
 * dmdx_syrk_blocks_f32 (dmdx_syrk_blocks_workspace_bytes).
 * The planes are used when n > 96, every block is 16-byte aligned with ldx % 4 == 0 and ldx < 2^22, and
 * DMDX_K1_ARITH is not f32; any other call runs exactly as dmdx_syrk_blocks_f32 does and does not touch `planes`.
 * Refused before the first launch, outputs, workspace and planes untouched: what dmdx_syrk_blocks_f32 refuses; a
 * null, misaligned or too small plane buffer (DMDX_E_WORKSPACE when null or small); a plane buffer that overlaps X, G or
 * the workspace; a unit plan that would read outside the plane buffer (checked on the host for every call). */
size_t dmdx_syrk_planes_bytes(const int64_t* m, int nblocks, int64_t n);
int dmdx_syrk_blocks_planes_f32(const float* const* X, const int64_t* m, const int64_t* ldx, int nblocks,
                                int64_t n, double* G64, int64_t ldg, float* G32, int64_t ldg32,
                                int accumulate, void* workspace, size_t workspace_bytes, void* planes,
                                size_t planes_bytes, void* stream);

/* ---- K3: C = A^T B, A: K x na, B: K x nb (both K-contiguous) ---------------
 * Z = X^T Y of the randomized range finder (extmath.py:351, `A.T @ Q`) and
 * B = Q^T X (extmath.py:577).  C64: na x nb fp64 (ldc); C32 nullable.  */
size_t dmdx_gemm_tn_workspace_bytes(int64_t K, int64_t na, int64_t nb);
int dmdx_gemm_tn_f32(const float* A, int64_t lda, const float* B, int64_t ldb,
                     int64_t K, int64_t na, int64_t nb,
                     double* C64, int64_t ldc, float* C32, int64_t ldc32, int accumulate,
                     void* workspace, size_t workspace_bytes, void* stream);

/* K3 over lists of row blocks in ONE launch per 16 blocks:  C (+)= sum_j A_j^T B_j  (A_j: K[j] x na,
 * lda[j]; B_j: K[j] x nb, ldb[j]; all five arrays live on the HOST).  The randomized path's
 * Z = X^T Y and B = Q^T X are sums over the row blocks of X; per-block launches of this
 * HBM-streaming product are only ~4 rounds of workgroups each. */
size_t dmdx_gemm_tn_blocks_workspace_bytes(const int64_t* K, int nblocks, int64_t na, int64_t nb);
int dmdx_gemm_tn_blocks_f32(const float* const* A, const int64_t* lda, const float* const* B,
                            const int64_t* ldb, const int64_t* K, int nblocks, int64_t na, int64_t nb,
                            double* C64, int64_t ldc, float* C32, int64_t ldc32, int accumulate,
                            void* workspace, size_t workspace_bytes, void* stream);

/* ---- K2: tall-skinny Y = X W -----------------------------------------------
 * X: m x n (ldx, rows > ldx allowed), W: n x l (ldw), Y: m x l (ldy); l is processed in column
 * groups of at most 224, 16-column granular (X is re-read once per group).
 * U = X (V_r S^-1) of the method of snapshots and `A @ Q` of the range finder
 * (extmath.py:349,355).  Fast path (16-byte loads of X, W and stores of Y): m, ldx, ldw, ldy
 * multiples of 4 and X, W, Y 16-byte aligned; anything else takes the scalar-load path (same
 * results, about half the rate).  When n % 4 != 0 give the small W a padded ldw rather than a
 * tight one -- the Python host does (HipKernels.pitch). */
int dmdx_gemm_nn_skinny_f32(const float* X, int64_t m, int64_t n, int64_t ldx,
                            const float* W, int64_t ldw, int64_t l,
                            float* Y, int64_t ldy, void* stream);

/* K2 with the Gram of its output fused in: Y = X W as above (l <= dmdx_gemm_nn_skinny_gram_max_l(),
 * 224) and G (+)= Y^T Y (l x l fp64, ldg, both triangles), formed from the accumulators before
 * they leave the registers: the CholeskyQR rounds of the range finder (the LU / QR normalisers of
 * extmath.py:349-355 in this engine) need that Gram, and computing it separately is another pass
 * over the m x l matrix.  Per-workgroup fp32 partial tiles in the workspace (summed over the
 * workgroup's waves in a fixed order), added up in fp64 (deterministic). */
int dmdx_gemm_nn_skinny_gram_max_l(void);
size_t dmdx_gemm_nn_skinny_gram_workspace_bytes(int64_t m, int64_t l);
int dmdx_gemm_nn_skinny_gram_f32(const float* X, int64_t m, int64_t n, int64_t ldx,
                                 const float* W, int64_t ldw, int64_t l, float* Y, int64_t ldy,
                                 double* G, int64_t ldg, int accumulate,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* ---- K5: per-row (space point) mean / std over time, centre, scale ---------
 * slice_tools.py:171-179.  X: m x n (ldx) modified in place:
 *   mean[i] = sum_j X[i,j] / n ; X[i,:] -= mean[i];
 *   if (scale) { std[i] = sqrt(sum_j X[i,j]^2 / n) of the centred row (ddof 0);
 *                X[i,:] /= std[i]; }
 * mean: m floats (required), std: m floats (required iff scale).
 * Sums are accumulated in fp64.  */
int dmdx_row_center_scale_f32(float* X, int64_t m, int64_t n, int64_t ldx,
                              float* mean, float* std, int scale, void* stream);

/* ---- K6: Gram of the delay-embedded matrix from the plain Gram -------------
 * Gd[i,j] = sum_{k<d} G[i+k, j+k], Gd is (n-d+1)^2  (slice_tools.py:207-211
 * applied to X^T X).  fp64 in, fp64 out (Gd32 nullable fp32 copy).  */
int dmdx_delay_shift_sum_f64(const double* G, int64_t n, int64_t ldg, int d,
                             double* Gd, int64_t ldgd, float* Gd32, int64_t ldgd32,
                             void* stream);

/* ---- small helpers on the same stream --------------------------------------
 * Y[:, j] *= alpha[j]  (m x l, ldy)  -- S^-1 scaling / sign flip of U columns */
int dmdx_scale_columns_f32(float* Y, int64_t m, int64_t l, int64_t ldy,
                           const float* alpha, void* stream);

/* ---- K7: eigenpairs of a small symmetric fp64 matrix, one launch -------------
 * A (n x n, lda, either storage order: only (A + A^T)/2 is used), n <= dmdx_eigh_small_max_n()
 * (96).  w[0..n) eigenvalues in DESCENDING order, V (n x n, row-major, ldv): column j is the
 * unit eigenvector of w[j].  sweeps: nullable device int, number of Jacobi sweeps used (the
 * rotation-free last one included); limit + 1 (31) = no rotation-free sweep within the limit.
 * Replaces the LAPACK syevd calls on the projected matrices of the method of snapshots (the
 * part of np.linalg.svd, era5_svd.py:251, that is left once X is reduced to its Gram matrix). */
int dmdx_eigh_small_max_n(void);
int dmdx_eigh_small_f64(const double* A, int64_t n, int64_t lda, double* w, double* V,
                        int64_t ldv, int* sweeps, void* stream);

/* ---- K7L: one-sided Jacobi SVD of a square fp64 matrix, 2 <= n <= dmdx_svd_jacobi_max_n() (1024),
 * one launch of <= 64 workgroups (they synchronise through a counter in the workspace: the launch
 * must be able to run them all at once, i.e. nothing else may occupy the device for good).
 * C: n x n, COLUMN c at C + c * ldc (contiguous), overwritten.  sigma[0..n): singular values in
 * DESCENDING order; Zt (n x n, ldz): ROW j = unit left singular vector of sigma[j] (zero rows for
 * zero singular values).  sweeps (nullable device int): sweeps used (the rotation-free last one
 * included), 41 = the limit of 40 was hit without one, -1 if the workgroups could not synchronise
 * (results invalid); a grid larger than the device's CU count is refused (DMDX_E_UNSUPPORTED;
 * dmdx_svd_jacobi_max_n() already accounts for it).  With C = chol(T) (or S L for T = S L L^T S) this gives
 * the eigenpairs of the positive definite T = C C^T with errors relative to each eigenvalue:
 * the (b x b) Rayleigh-Ritz matrices and the graded refinement matrix of the method of
 * snapshots beyond K7's n <= 96 -- the LAPACK syevd / gesvd calls left of np.linalg.svd
 * (era5_svd.py:251) once X is reduced to its Gram matrix. */
int dmdx_svd_jacobi_max_n(void);
size_t dmdx_svd_jacobi_workspace_bytes(int64_t n);
int dmdx_svd_jacobi_f64(double* C, int64_t n, int64_t ldc, double* sigma, double* Zt, int64_t ldz,
                        int* sweeps, void* workspace, size_t workspace_bytes, void* stream);

/* ---- K8: Y = G Q - shift Q, G symmetric n x n fp64, Q / Y n x b row-major (ldq, ldy) ------
 * The products of the top-eigenpair solver on the Gram matrix (the part of np.linalg.svd,
 * era5_svd.py:251, left once X is reduced to G): fp64 MFMA, G streamed once, Q staged in LDS,
 * K split over workgroups with per-split partial tiles in the workspace (deterministic), summed
 * and shifted by a second kernel.  n, b, ldg, ldq even; G, Q, workspace 16-byte aligned; only
 * G = G^T is supported (row k of G is read as column k).  Y must not alias Q. */
size_t dmdx_symm_skinny_workspace_bytes(int64_t n, int64_t b);
int dmdx_symm_skinny_f64(const double* G, int64_t n, int64_t ldg, const double* Q, int64_t ldq,
                         int64_t b, double shift, double* Y, int64_t ldy,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ---- K9: C = A^T B for tall fp64 blocks, A n x b1 (lda), B n x b2 (ldb), C b1 x b2 (ldc), all
 * row-major.  The Grams of the CholeskyQR rounds, the Rayleigh-Ritz matrices and the block
 * projections of the top-eigenpair solver (the same part of np.linalg.svd, era5_svd.py:251, as K8).
 * fp64 MFMA, K split over workgroups, per-split partial tiles in the workspace (deterministic).
 * b1, b2, lda, ldb even; A, B, workspace 16-byte aligned. */
size_t dmdx_gemm_tn_f64_workspace_bytes(int64_t n, int64_t b1, int64_t b2);
int dmdx_gemm_tn_f64(const double* A, int64_t lda, const double* B, int64_t ldb, int64_t n,
                     int64_t b1, int64_t b2, double* C, int64_t ldc,
                     void* workspace, size_t workspace_bytes, void* stream);

/* ---- K10: Cholesky factor and its inverse of a small symmetric positive definite fp64 matrix, one launch --
 * A (n x n, lda, row-major; only the lower triangle is read), n <= dmdx_potrf_trtri_max_n() (1024):
 * A + shift I = L L^T, L (n x n, ldl) lower triangular (zeros above), Linv (n x n, ldi, nullable) = L^-1
 * (lower triangular).  info: 3 device doubles -- [0] status: 0 ok, j + 1 = first non-positive or
 * non-finite pivot (it is replaced by 1 and the factorisation goes on, so the outputs stay finite: the
 * caller shifts and retries), -1 = the workgroups of the launch could not synchronise;
 * [1] / [2] = min / max of diag(L) (~ 1 / cond).  One workgroup per 32-row block row (<= 32), one
 * grid barrier per block column (counter in the workspace: the launch must be co-resident).
 * Replaces LAPACK potrf + trtri / trsm behind the CholeskyQR rounds (the LU / QR normalisers of
 * sklearn's randomized_svd, extmath.py:349-355, era5_svd.py:258) and the Cholesky factors fed to the
 * Jacobi kernel (part of np.linalg.svd, era5_svd.py:251). */
int dmdx_potrf_trtri_max_n(void);
size_t dmdx_potrf_trtri_workspace_bytes(int64_t n);
int dmdx_potrf_trtri_f64(const double* A, int64_t n, int64_t lda, double shift, double* L, int64_t ldl,
                         double* Linv, int64_t ldi, double* info, void* workspace, size_t workspace_bytes,
                         void* stream);

/* ---- K11: Y = Q Mt^T for a tall fp64 block Q (n x b1, ldq) and a small Mt (b2 x b1, ldm), Y n x b2 (ldy),
 * all row-major: Q L^-T of a CholeskyQR round (Mt = L^-1 from K10) and S Z of a Rayleigh-Ritz step
 * (Mt = Z^T as K7L returns it).  fp64 MFMA, operands straight from global memory.  b1, ldq, ldm even;
 * Q, Mt 16-byte aligned; Y must not alias an input. */
int dmdx_gemm_nt_f64(const double* Q, int64_t ldq, int64_t n, int64_t b1, const double* Mt, int64_t ldm,
                     int64_t b2, double* Y, int64_t ldy, void* stream);

/* ---- K12: full fields from the rank-k factors, Xhat = mu + sigma .* (U C), and their score ------------------
 * The step from the reduced coordinates back to ERA5 fields: U (m x k, ldu) are the left singular vectors
 * (np.linalg.svd / randomized_svd, era5_svd.py:251,258), C (k x T, ldc) the coefficients of T snapshots
 * (diag(s) Vh for the rank-k reconstruction, the optimized-DMD model evaluated at T times for a forecast),
 * mu / sigma (m floats each, nullable: 0 / 1) undo slice_tools.py:171-179.  1 <= k <= dmdx_expand_max_k() (256).
 *   Xhat[i, t] = mu[i] + sigma[i] * sum_j U[i, j] C[j, t]        (m x T, ldxh)
 * One fp32 MFMA chain over k (any order), then sigma * acc + mu in fp32.
 *
 * dmdx_expand_score_f32 forms the same Xhat, never stores it, and compares it with X (m x T, ldx; rows > ldx
 * allowed, the zero-copy delay view):
 *   sse_col[t] (+)= sum_i (X[i,t] - Xhat[i,t])^2     T doubles, required
 *   ref_col[t] (+)= sum_i (X[i,t] - mu[i])^2         T doubles, nullable
 *   sse_row[i]  =  sum_t (X[i,t] - Xhat[i,t])^2      m doubles, nullable, always overwritten
 * accumulate != 0 adds to sse_col / ref_col (X and U given as row blocks).  Squared residuals are summed in
 * fp32 over at most DMDX_EXPAND_FP32_ROWS rows (columns: the rows of one workgroup; rows: 16 snapshots) and
 * in fp64 beyond, through per-workgroup partial slots in the workspace and reduce kernels: no atomics, the
 * order of every sum depends on (m, T) only, results are bit-wise reproducible.  X is read once. */
#define DMDX_EXPAND_FP32_ROWS 128
int dmdx_expand_max_k(void);
int dmdx_expand_f32(const float* U, int64_t m, int64_t k, int64_t ldu, const float* C, int64_t ldc, int64_t T,
                    const float* mu, const float* sigma, float* Xhat, int64_t ldxh, void* stream);
size_t dmdx_expand_score_workspace_bytes(int64_t m, int64_t k, int64_t T);
int dmdx_expand_score_f32(const float* U, int64_t m, int64_t k, int64_t ldu, const float* C, int64_t ldc, int64_t T,
                          const float* mu, const float* sigma, const float* X, int64_t ldx,
                          double* sse_col, double* ref_col, double* sse_row, int accumulate,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ---- K13: coefficients of raw snapshots in the basis U, and their energy ---------------------------------------
 * The other direction of K12: snapshots that were not part of the decomposition are standardised as
 * slice_tools.py:171-179 does (mu / sigma: m floats each, nullable: 0 / 1) and projected on the left singular
 * vectors U (m x k, ldu; np.linalg.svd / randomized_svd, era5_svd.py:251,258) without a standardised copy of X:
 *   xt[i, t]   = fl( fl(X[i, t] - mu[i]) / sigma[i] )            what K5 leaves in place for the same mu, sigma
 *   C[j, t]   (+)= sum_i U[i, j] xt[i, t]                          k x T fp64, ldc
 *   energy[t] (+)= sum_i xt[i, t]^2                                T doubles, nullable
 * X: m x T (ldx; rows > ldx allowed, the zero-copy delay view), read once.  1 <= k <= dmdx_project_max_k() (256).
 * accumulate != 0 adds to C and energy (X and U given as row blocks).  fp32 MFMA products; fp32 sums cover at
 * most DMDX_PROJECT_FP32_ROWS rows (one row range of the launch), fp64 beyond, through per-unit slots in the
 * workspace and a reduce kernel: no atomics, the order of every sum depends on (m, k, T) only, results are
 * bit-wise reproducible.  One call covers fewer than 2^24 (row range, 128-snapshot tile) units
 * (DMDX_E_UNSUPPORTED beyond: terabytes of X; pass row blocks). */
#define DMDX_PROJECT_FP32_ROWS 4096
int dmdx_project_max_k(void);
size_t dmdx_project_workspace_bytes(int64_t m, int64_t k, int64_t T);
int dmdx_project_f32(const float* U, int64_t m, int64_t k, int64_t ldu, const float* X, int64_t ldx, int64_t T,
                     const float* mu, const float* sigma, double* C, int64_t ldc, double* energy, int accumulate,
                     void* workspace, size_t workspace_bytes, void* stream);

/* ---- K15: ensemble spread of B models in the rank-k coordinates, and its sums --------------------------------
 * What a bagged optimized-DMD fit (bopdmd(keep_trials=True)) says about its own uncertainty, on the grid.  The
 * member coefficients c_b(t), b < B, have the mean cbar(t); D (k x (B T), ldd) holds the scaled deviations
 * d_b(t) = (c_b(t) - cbar(t)) / sqrt(B - ddof) in column b T + t.  U (m x k, ldu) and sigma (m floats, nullable: 1)
 * as in K12; there is no mu: a spread has no offset.  1 <= k <= dmdx_spread_max_k() (256).
 *   P_b[i, t] = sum_j U[i, j] D[j, b T + t]           one fp32 MFMA chain over k per member, K12's chain
 *   V[i, t]   = sum_b P_b[i, t]^2                     fp32, b = 0, 1, ... in this order, one rounding per member
 *   S[i, t]   = |sigma[i]| * sqrt(V[i, t])            m x T, lds; the sample standard deviation of the B fields
 * The ensemble-mean field itself is K12 with cbar.  No member field is ever stored.
 *
 * dmdx_spread_score_f32 forms the same V and never stores S:
 *   var_col[t] (+)= sum_i sigma[i]^2 V[i, t]          T doubles, required
 *   var_row[i]  =  sum_t sigma[i]^2 V[i, t]           m doubles, nullable, always overwritten
 * accumulate != 0 adds to var_col (U given as row blocks).  fp32 sums cover at most DMDX_SPREAD_FP32_ROWS rows
 * (columns: the rows of one workgroup; rows: 16 snapshots), fp64 beyond, through per-workgroup partial slots in
 * the workspace and reduce kernels: no atomics, the order of every sum depends on (m, T, B) only, results are
 * bit-wise reproducible. */
#define DMDX_SPREAD_FP32_ROWS 128
int dmdx_spread_max_k(void);
int dmdx_spread_f32(const float* U, int64_t m, int64_t k, int64_t ldu, const float* D, int64_t ldd, int64_t T, int64_t B,
                    const float* sigma, float* S, int64_t lds, void* stream);
size_t dmdx_spread_score_workspace_bytes(int64_t m, int64_t k, int64_t T, int64_t B);
int dmdx_spread_score_f32(const float* U, int64_t m, int64_t k, int64_t ldu, const float* D, int64_t ldd, int64_t T, int64_t B,
                          const float* sigma, double* var_col, double* var_row, int accumulate,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ---- K16: area-weighted verification of Xhat = mu + sigma .* (U C) on the grid --------------------------------
 * What a forecast of ERA5 fields is judged by: the root-mean-square error, the bias and the anomaly correlation
 * against a climatology, weighted by the area of the grid cells (cos(latitude) on the regular grid of
 * era5_svd.py:132), per variable and level.  The operands are K12's -- U (m x k, ldu), C (k x T, ldc), mu / sigma
 * (m floats each, nullable: 0 / 1), X (m x T, ldx; rows > ldx allowed, the zero-copy delay view) -- and two more:
 * w (m floats, nullable: 1) the weight of every row, clim (m floats, nullable: mu, and 0 if that is NULL too) the
 * climatology.  1 <= k <= dmdx_verify_max_k() (256: whatever K12 can expand can be verified).  Per element, fp32:
 *   xhat = sigma * acc + mu       K12's chain over k (padded with zeros on both sides) and K12's two-step epilogue
 *   e = fl(xhat - x)   f = fl(xhat - clim[i])   a = fl(x - clim[i])
 * and the DMDX_VERIFY_NQ = 6 quantities   0: e^2   1: e   2: a   3: f^2   4: a^2   5: f a   (each rounded once):
 *   col[q * ldcol + t] (+)= sum over the rows i with w[i] != 0 of fl(w[i] * quantity_q[i, t])    ldcol >= T
 *   row[q * ldrow + i]  =  sum_t quantity_q[i, t]       nullable, ldrow >= m, unweighted, always overwritten
 * With w == NULL there is no multiply.  RMSE^2 = col0 / W, bias = col1 / W, ACC = col5 / sqrt(col3 col4), the centred
 * ACC needs col1 + col2 and col2 as well, W = sum of the weights (the host's); with clim = the initial analysis
 * col4 / W is the squared error of persistence.  The weight is per row, so the host applies it to `row`.
 * A row with w[i] == 0 is SELECTED out of the column sums, not multiplied in: whatever X, U, mu, sigma or clim hold
 * in that row (NaN, Inf: the fill values of K14, a land / sea mask), no column sum changes by a bit; its `row` sums
 * are still the plain sums.  With every w == 0 the column sums are +0.0.
 * accumulate != 0 adds to col (X and U given as row blocks; a group of rows -- one variable at one level -- is a
 * pointer offset, the kernel knows no groups); otherwise every logical element of col is written and none read.
 * Sums as K12's score: fp32 over at most DMDX_VERIFY_FP32_ROWS rows (columns: the rows of one workgroup; rows: 16
 * snapshots), fp64 beyond, through per-workgroup partial slots in the workspace and reduce kernels: no atomics, the
 * order of every sum depends on (m, T) only, results are bit-wise reproducible.  The row blocks, the T split and
 * the order of the sums are K12's: with w == NULL and clim == NULL, col[0] and col[4] are bit for bit sse_col and
 * ref_col of dmdx_expand_score_f32 on the same operands, and row[0] is its sse_row.
 * Values: a non-finite X[i, t] with w[i] != 0 makes column t of the sums it enters non-finite and row i of `row`; a
 * non-finite U[i, j], mu[i], sigma[i] or clim[i] row i and, if w[i] != 0, every column of the sums it enters;
 * everything else keeps its bits.  Integer U, C, mu, sigma, X, clim with w a power of two and partial sums below
 * 2^24 give the integer results exactly; (2^e U, 2^-e C) changes no bit, 2^e w scales the column sums by 2^e.
 * Memory as for K12: only logical elements are read, only logical elements of col / row are written, nothing is
 * written behind the workspace, no alignment is required.  m, T and the leading dimensions must be < 2^31.  A
 * refused call (DMDX_E_INVALID: a null U, C, X or col, k outside 1 .. 256, ldu < m, ldc < k, ldx < 1, ldcol < T,
 * ldrow < m with row given, a size >= 2^31; DMDX_E_WORKSPACE: a null or short workspace) has written nothing. */
#define DMDX_VERIFY_NQ 6
#define DMDX_VERIFY_FP32_ROWS 128
int dmdx_verify_max_k(void);
size_t dmdx_verify_workspace_bytes(int64_t m, int64_t k, int64_t T);
int dmdx_verify_f32(const float* U, int64_t m, int64_t k, int64_t ldu, const float* C, int64_t ldc, int64_t T,
                    const float* mu, const float* sigma, const float* X, int64_t ldx,
                    const float* w, const float* clim, double* col, int64_t ldcol,
                    double* row, int64_t ldrow, int accumulate,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ---- K19: fair CRPS and rank histogram of B member fields on the grid ------------------------------------------
 * What an ensemble forecast of gridded fields is published with besides its spread-skill ratio: the continuous
 * ranked probability score, area-weighted, and the rank histogram -- without storing a member field.  The operands
 * are K16's -- U (m x k, ldu), mu / sigma (m floats each, nullable: 0 / 1), X (m x T, ldx; rows > ldx allowed, the
 * zero-copy delay view), w (m floats, nullable: 1) -- but C (k x (B T), ldc) carries the members the way K15's D
 * does: column b T + t holds the coefficients of member b at snapshot t (the members themselves, not deviations).
 * 1 <= k <= dmdx_crps_max_k() (256), 1 <= B <= dmdx_crps_max_members() = DMDX_CRPS_MAX_B (256).  Per element, fp32:
 *   x_b  = sigma * acc_b + mu        K12's chain over k for the columns of member b and K12's two-step epilogue:
 *                                    member b's field is bit for bit what dmdx_expand_f32 gives for C_b
 *   abs  = sum_b |x_b - y|           y = X[i, t]; b = 0, 1, ... in this order, each term rounded once
 *   pair = sum_{b < b'} |x_b - x_b'| each term rounded once; ONE fp32 chain of B (B - 1) / 2 terms per element, in an
 *                                    order that depends on (B, k) only (members are held in registers in blocks of
 *                                    DMDX_CRPS_MEMBER_BLOCK_SMALL_K = 16 for k <= 128 and DMDX_CRPS_MEMBER_BLOCK = 8
 *                                    above, and the chains of the later members are repeated per block); where abs
 *                                    is not finite pair is made NaN
 *   rank = #{ b : x_b < y }          an integer in 0 .. B; a tie counts as "not below"
 * and the outputs
 *   col[q * ldcol + t] (+)= sum over the rows i with w[i] != 0 of fl(w[i] * quantity_q[i, t])    ldcol >= T
 *                           q = 0: abs, q = 1: pair (DMDX_CRPS_NQ = 2)
 *   row[q * ldrow + i]  =  sum_t quantity_q[i, t]       nullable, ldrow >= m, unweighted, always overwritten
 *   hist[r]           (+)= number of elements (i, t) with w[i] != 0, a FINITE abs[i, t], and rank == r
 *                           B + 1 int64, nullable
 * The host forms the scores: CRPS = col0 / (B W) - col1 / (B (B - 1) W) (the fair estimator) or
 * col0 / (B W) - col1 / (B^2 W) (the plain ensemble estimator), W = sum of the weights.
 * A row with w[i] == 0 is SELECTED out of col and hist, whatever it holds; its `row` sums are the plain sums.  With
 * every w == 0 col is +0.0 and hist is 0.  accumulate != 0 adds to col and hist (row blocks; a group of rows is a
 * pointer offset); otherwise every logical element of col and hist is written and none read.
 * Sums as K16's: fp32 over at most DMDX_CRPS_FP32_ROWS rows (columns: the rows of one workgroup; rows: 16
 * snapshots), fp64 beyond, through per-workgroup partial slots in the workspace and reduce kernels.  No
 * floating-point atomics: the order of every fp sum depends on (m, T, B, k) only, two calls give the same bits.  The
 * counts are integers: a workgroup counts a tile in 32-bit LDS counters (integer atomics; a tile has 128 x 32 = 4096
 * elements, and the counters are emptied into 64-bit registers after every tile, so no width overflows for any T),
 * writes its 64-bit counts to its own slot of the workspace, and a reduce kernel adds the slots.
 * Values: a non-finite X[i, t] with w[i] != 0 makes column t of both sums non-finite and row i of `row`; that
 * element enters no bin.  A non-finite U[i, j], mu[i] or sigma[i] does the same to row i and, if w[i] != 0, to every
 * column.  Everything else keeps its bits.  Integer operands with power-of-two w and partial sums below 2^24 give
 * exact integers; identical members give pair == +0.0 exactly; (2^e U, 2^-e C) changes no bit.
 * Memory as for K12 / K16: only logical elements are read or written, the workspace is exactly
 * dmdx_crps_workspace_bytes(m, k, T, B) and needs no initialisation, no alignment is required.  m, T, B T and the
 * leading dimensions must be < 2^31.  A refused call (DMDX_E_INVALID: a null U, C, X or col, k outside 1 .. 256, B
 * outside 1 .. DMDX_CRPS_MAX_B, ldu < m, ldc < k, ldx < 1, ldcol < T, ldrow < m with row given, a size >= 2^31;
 * DMDX_E_WORKSPACE: a null or short workspace) has written nothing. */
#define DMDX_CRPS_NQ 2
#define DMDX_CRPS_FP32_ROWS 128
#define DMDX_CRPS_MAX_B 256
#define DMDX_CRPS_MEMBER_BLOCK 8
#define DMDX_CRPS_MEMBER_BLOCK_SMALL_K 16
int dmdx_crps_max_k(void);
int dmdx_crps_max_members(void);
size_t dmdx_crps_workspace_bytes(int64_t m, int64_t k, int64_t T, int64_t B);
int dmdx_crps_f32(const float* U, int64_t m, int64_t k, int64_t ldu, const float* C, int64_t ldc, int64_t T, int64_t B,
                  const float* mu, const float* sigma, const float* X, int64_t ldx, const float* w,
                  double* col, int64_t ldcol, double* row, int64_t ldrow, int64_t* hist, int accumulate,
                  void* workspace, size_t workspace_bytes, void* stream);

/* ---- K24: exceedance probability and Brier sums of B member fields on the grid ---------------------------------
 * What an ensemble forecast is consumed as besides its mean and spread: the probability that a field exceeds (or
 * falls below) a threshold -- the share of the members that do -- and what that probability is scored with: the
 * Brier score, the reliability diagram and the ROC curve.  No member field is stored.  The shared operands are
 * K19's: U (m x k, ldu), C (k x (B T), ldc; column b T + t holds the coefficients of member b at snapshot t), mu /
 * sigma (m floats each, nullable: 0 / 1).  1 <= k <= dmdx_exceed_max_k() (256), 1 <= B <= dmdx_exceed_max_members()
 * = DMDX_EXCEED_MAX_B (256).  New operands:
 *   thr    m x (J S) floats, ldthr >= m: column j S + s holds threshold j of every row for slot s (a slot is a class
 *          of the calendar, K18's); 1 <= J <= dmdx_exceed_max_thresholds() = DMDX_EXCEED_MAX_THR (4), S >= 1
 *   slot   T int32, nullable (every snapshot in slot 0): the slot of snapshot t.  As in dmdx_clim_apply_f32 a value
 *          outside 0 .. S - 1 means "no slot": nothing of thr is read for that snapshot and its thresholds are NaN
 *          (no event); the host refuses such values before the call
 *   above  != 0: the event is value > thr;  0: the event is value < thr.  A strict IEEE comparison: a tie is no
 *          event, a NaN threshold gives no event.
 * Per element (i, t) and threshold j, fp32, no fused operation:
 *   x_b = sigma * acc_b + mu         K12's chain over k for the columns of member b and K12's two-step epilogue:
 *                                    member b's field is bit for bit what dmdx_expand_f32 gives for C_b
 *   c   = #{ b : x_b <> thr }        an integer in 0 .. B; <> is the comparison `above` selects
 *   p   = the fp32 nearest to c / B  (for c <= B <= 256: fp32(fp64(c) / fp64(B)))
 * The element is FINITE iff all B members are finite; the score wants a finite y = X[i, t] as well.  All J
 * thresholds are counted in one pass of B chains per element: the cost does not grow with J but for the epilogue.
 *
 * dmdx_exceed_prob_f32 writes J planes: P[j * pstride + t * ldp + i] = p, or NaN where the element is not finite
 * (ldp >= m; the planes must not overlap: pstride >= (T - 1) ldp + m unless J == 1).  Every logical element of the J
 * planes is written and nothing else; no X, no workspace, no reduce kernel.
 *
 * dmdx_exceed_score_f32 adds X (m x T, ldx; rows > ldx allowed, the zero-copy delay view) and w (m floats,
 * nullable: 1).  Per element and threshold:   o = (y <> thr) ? 1 : 0     d = fl(p - o)   and the DMDX_EXCEED_NQ = 4
 * quantities   0: fl(d d)   1: o   2: p   3: fl(p p);   a non-finite element makes all four NaN for every j.
 *   col[(4 j + q) * ldcol + t] (+)= sum over the rows i with w[i] != 0 of fl(w[i] * quantity_q[i, t])   ldcol >= T
 *   row[(4 j + q) * ldrow + i]  =  sum_t quantity_q[i, t]     nullable, ldrow >= m, unweighted, always overwritten
 *   cnt[(2 j + o) * (B + 1) + c] (+)= number of elements (i, t) with w[i] != 0 that are finite, have outcome o and
 *                                  count c;  2 J (B + 1) int64, nullable
 * With w == NULL there is no multiply.  The host forms the scores: Brier = col0 / W, its fair (ensemble-size
 * corrected) form col0 / W - (col2 - col3) / ((B - 1) W), the base rate col1 / W, the forecast rate col2 / W, W = sum
 * of the weights; reliability O_c / N_c and the ROC curve come from cnt.
 * A row with w[i] == 0 is SELECTED out of col and cnt, whatever it holds; its `row` sums are the plain sums.  With
 * every w == 0 col is +0.0 and cnt is 0.  accumulate != 0 adds to col and cnt (row blocks; a group of rows is a
 * pointer offset); otherwise every logical element of col and cnt is written and none read.
 * Sums as K16's / K19's: fp32 over at most DMDX_EXCEED_FP32_ROWS rows (columns: the rows of one workgroup; rows: 16
 * snapshots), fp64 beyond, through per-workgroup partial slots in the workspace and reduce kernels.  No
 * floating-point atomics: the order of every fp sum depends on (m, T, J) only, two calls give the same bits.  The
 * counts are integers: a workgroup counts a tile in 32-bit LDS counters (integer atomics; a tile has 128 x 32 = 4096
 * elements, and the counters are emptied into 64-bit registers after every tile, so no width overflows for any T),
 * writes its 64-bit counts to its own slot of the workspace, and a reduce kernel adds the slots.
 * Values: every quantity lies in [0, 1], so only the sums round.  A non-finite X[i, t] with w[i] != 0 makes column t
 * of all 4 J sums NaN and row i of `row`; that element enters no bin.  A non-finite U[i, j], mu[i] or sigma[i] does
 * the same to row i and, if w[i] != 0, to every column; a non-finite C[j, b T + t] to column t and every row.
 * Everything else keeps its bits; (2^e U, 2^-e C) changes no bit.  A NaN threshold gives c = 0 and o = 0, finite.
 * Memory as for K19: only logical elements are read or written, the workspace is exactly
 * dmdx_exceed_score_workspace_bytes(m, k, T, B, J) and needs no initialisation, no alignment is required.  m, T, B T,
 * J S, S and the leading dimensions must be < 2^31.  A refused call (DMDX_E_INVALID: a null U, C, thr, P (prob), X or
 * col (score), k outside 1 .. 256, B outside 1 .. DMDX_EXCEED_MAX_B, J outside 1 .. DMDX_EXCEED_MAX_THR, S < 1, ldu < m,
 * ldc < k, ldthr < m, ldp < m, overlapping planes, ldx < 1, ldcol < T, ldrow < m with row given, a size >= 2^31;
 * DMDX_E_WORKSPACE: a null or short workspace) has written nothing. */
#define DMDX_EXCEED_NQ 4
#define DMDX_EXCEED_FP32_ROWS 128
#define DMDX_EXCEED_MAX_B 256
#define DMDX_EXCEED_MAX_THR 4
int dmdx_exceed_max_k(void);
int dmdx_exceed_max_members(void);
int dmdx_exceed_max_thresholds(void);
int dmdx_exceed_prob_f32(const float* U, int64_t m, int64_t k, int64_t ldu, const float* C, int64_t ldc, int64_t T, int64_t B,
                         const float* mu, const float* sigma, const float* thr, int64_t ldthr, int64_t J, int64_t S,
                         const int32_t* slot, int above, float* P, int64_t ldp, int64_t pstride, void* stream);
size_t dmdx_exceed_score_workspace_bytes(int64_t m, int64_t k, int64_t T, int64_t B, int64_t J);
int dmdx_exceed_score_f32(const float* U, int64_t m, int64_t k, int64_t ldu, const float* C, int64_t ldc, int64_t T, int64_t B,
                          const float* mu, const float* sigma, const float* thr, int64_t ldthr, int64_t J, int64_t S,
                          const int32_t* slot, int above, const float* X, int64_t ldx, const float* w,
                          double* col, int64_t ldcol, double* row, int64_t ldrow, int64_t* cnt, int accumulate,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ---- K14: CF-packed int16 codes -> fp32 snapshots of one row block ---------------------------------------------
 * What xr.open_dataset's mask_and_scale decoding (reference era5_svd.py:132 through retrieve_era5_slice) does to a
 * variable stored as int16 with scale_factor / add_offset / _FillValue / missing_value, done in HBM so that the
 * packed bytes are what crosses the file system, the pinned staging and PCIe.
 *   S     time slab of codes as it sits in the file: snapshot-major, space contiguous, snapshot stride lds (elements)
 *   X     the row block's snapshots to write: T columns of `rows` floats, leading dimension ldx (already advanced
 *         to the first snapshot); output snapshot j is source snapshot j * tstep (tstep >= 1)
 *   row g = row0 + r of the variable (r < rows) is source element host_seg_offset[g / plane] + g % plane of its
 *         snapshot: `plane` space points per segment, 1 <= nseg <= 64 segment offsets (>= 0) in a HOST array that
 *         is copied into the launch -- a level selection, the latitude band of a shard and a block that
 *         straddles two levels are all one table.  row0 + rows <= nseg * plane < 2^31.
 *   x = fp32( fp64(q) * scale_factor + add_offset ): an fp64 multiply and an fp64 add (two roundings, not an FMA),
 *         then one round-to-nearest conversion -- bit for bit numpy's
 *         (q.astype(float64) * scale_factor + add_offset).astype(float32)
 *   a code equal to one of the nfill (0, 1 or 2) fill codes fill0 / fill1 becomes the quiet NaN 0x7FC00000 and is
 *         counted: fill_count (device, nullable) ACCUMULATES, one atomicAdd per workgroup that saw a fill; the
 *         caller zeroes it once per variable.
 * Memory: only the logical rows x T elements of X are written (not the ldx - rows behind a column: the zero rows of
 * a padded block stay zero) and only the addressed codes of S are read (not the snapshots tstep skips).  No
 * alignment is asked for beyond that of the element types: whatever X, ldx and row0 are, full 8-row chunks are
 * stored as two aligned 16-byte stores and the ragged ends element by element; a chunk whose 8 codes lie in one
 * segment at a 16-byte aligned address is read with one 16-byte load, any other as 2-byte loads of exactly the
 * addressed codes, with identical bits.
 * A refused call (negative sizes, tstep < 1, nseg outside 1..64, nfill outside 0..2, ldx < rows, plane < 1, rows
 * outside the segments) returns DMDX_E_INVALID before any launch; T == 0 or rows == 0 returns 0 and writes nothing. */
int dmdx_unpack_i16_f32(const int16_t* S, int64_t lds, int64_t T, int64_t tstep, int64_t rows, int64_t row0,
                        int64_t plane, int nseg, const int64_t* host_seg_offset, double scale_factor,
                        double add_offset, int nfill, int fill0, int fill1, float* X, int64_t ldx,
                        unsigned long long* fill_count, void* stream);

/* ---- K17: fields -> CF-packed int16 codes, and the value range a packing is chosen from ------------------------
 * The inverse of K14: what xarray's CF encoder does to a variable written with scale_factor / add_offset / _FillValue
 * (np.around((x - add_offset) / scale_factor)), done where the field is formed, so that the codes (2 bytes per value)
 * are what HBM, PCIe and the file system see.  The fill code is -32768, the live codes are -32767 .. 32767.
 *   code(x) = -32768                                                     x not finite (NaN, +-Inf): counted as FILLED
 *           = clamp(rint((fp64(x) - add_offset) / scale_factor), -32767, 32767)     an fp64 subtract, an IEEE fp64
 *             divide (no reciprocal, no FMA), round half to even; an element that needed the clamp counts as SATURATED
 * -- bit for bit labeled.Packing.encode.  A packing of a range is labeled.Packing.for_range (host, fp64):
 * scale_factor = (vmax - vmin) / 65534, add_offset = (vmax + vmin) / 2, so that vmin -> -32767 and vmax -> 32767.
 *
 * dmdx_expand_range_f32 / dmdx_expand_pack_i16 form Xhat = mu + sigma .* (U C) and never store it.  The operands are
 * K12's -- U (m x k, ldu), C (k x T, ldc), mu / sigma (m floats each, nullable: 0 / 1), 1 <= k <= dmdx_pack_max_k()
 * (256) -- and every xhat[i, t] is bit for bit what dmdx_expand_f32 stores for them (K12's chain over k, padded with
 * zeros on both sides, and K12's two-step epilogue).
 *   range[0] / range[1]   the minimum / maximum of the finite xhat (2 floats, device): exact, min and max do not round;
 *                         (+Inf, -Inf) when nothing is finite
 *   count[0]              the number of non-finite xhat (device)
 *   accumulate != 0 merges with what range and count hold (row blocks; a group of rows -- one variable -- given as
 *   several row ranges: a group is a pointer offset and a row count, the kernel knows none); otherwise both are
 *   written and not read.  Per-workgroup slots in the workspace and a reduce kernel: no atomics, the result depends
 *   on the values only.
 *   Q                     the codes, m x T int16, snapshot stride ldq >= m, space contiguous: a time slab of the file,
 *                         K14's S.  Q needs its 2-byte alignment only and ldq may be odd: the bits do not depend on
 *                         the base or on ldq.
 *   counts                (device, 2 x unsigned long long, nullable) ACCUMULATES [filled, saturated]: one atomicAdd per
 *                         counter and workgroup that saw one; the caller zeroes it once per variable.
 * dmdx_range_f32 / dmdx_pack_f32_i16: the same two contracts for a field X (m x T, ldx >= 1) that exists -- the K15
 * spread, an ensemble mean, real snapshots.  Streaming: X is read once, 4 bytes read and 2 written per element.
 * Memory: only logical elements of U, C, mu, sigma and X are read, only the logical m x T elements of Q are written
 * (not the ldq - m behind a snapshot), nothing is written behind the workspace, no alignment is asked for beyond that
 * of the element types.  m, T and the leading dimensions must be < 2^31.  A refused call (DMDX_E_INVALID: a null U, C,
 * X, Q, range or count, k outside 1 .. 256, ldu < m, ldc < k, ldq < m, ldx < 1, a size >= 2^31, a scale_factor that is
 * 0 or not finite, an add_offset that is not finite; DMDX_E_WORKSPACE: a null or short workspace) has written nothing.
 * Values: a non-finite U[i, j], mu[i] or sigma[i] makes the codes of row i the fill code, a non-finite C[j, t] those of
 * snapshot t, a non-finite X[i, t] that one code; every other code keeps its bits. */
int dmdx_pack_max_k(void);
size_t dmdx_expand_range_workspace_bytes(int64_t m, int64_t k, int64_t T);
int dmdx_expand_range_f32(const float* U, int64_t m, int64_t k, int64_t ldu, const float* C, int64_t ldc, int64_t T,
                          const float* mu, const float* sigma, float* range, unsigned long long* count,
                          int accumulate, void* workspace, size_t workspace_bytes, void* stream);
int dmdx_expand_pack_i16(const float* U, int64_t m, int64_t k, int64_t ldu, const float* C, int64_t ldc, int64_t T,
                         const float* mu, const float* sigma, double scale_factor, double add_offset,
                         int16_t* Q, int64_t ldq, unsigned long long* counts, void* stream);
size_t dmdx_range_workspace_bytes(int64_t m, int64_t T);
int dmdx_range_f32(const float* X, int64_t m, int64_t T, int64_t ldx, float* range, unsigned long long* count,
                   int accumulate, void* workspace, size_t workspace_bytes, void* stream);
int dmdx_pack_f32_i16(const float* X, int64_t m, int64_t T, int64_t ldx, double scale_factor, double add_offset,
                      int16_t* Q, int64_t ldq, unsigned long long* counts, void* stream);

/* ---- K18: slot climatology of the snapshots of one row block, and the anomalies against it -------------------------
 * What everybody who fits a DMD to ERA5 removes first: the mean (and spread) of every grid point per class of the
 * calendar -- an hour of the day, a (month, hour) pair, a day of the year -- where K5 (slice_tools.py:171-179) knows
 * the mean over all of time only.  X is a row block as everywhere: T columns (snapshots) of m floats, ldx >= m.
 *   order, start   (device int32) a CSR list: slot s < S owns the snapshot indices order[a .. b) with
 *                  a = clamp(start[s], 0, n_order), b = clamp(start[s + 1], a, n_order); start holds S + 1 offsets.  A
 *                  snapshot may sit in several slots (a window of days around a day of the year) or in none.  An entry
 *                  outside [0, T) is skipped and NOT counted: the lists are data, a wrong one gives wrong means and never
 *                  an access outside X.  n_s = the number of counted entries of slot s.
 *   mean[s ldc + i] = fp32( acc / n_s ),  acc = +0.0 (fp64), acc += fp64(X[i, order[j]]) for j = a .. b - 1 IN THIS ORDER,
 *                  whatever the launch geometry; an IEEE fp64 divide, then one rounding.  n_s == 0: the quiet NaN
 *                  0x7FC00000.  mean is S x m (slot-major, ldc >= m).
 *   sd[s lds + i]  = fp32( sqrt( acc / (n_s - ddof) ) ),  d = fp64(x) - fp64(mean[s ldc + i]), q = d d (rounded), acc += q in
 *                  the same order; the root is correctly rounded.  ddof is 0 or 1; n_s - ddof <= 0: the same NaN.
 *   slot           (device int32, T labels) the slot whose climatology snapshot t takes in apply.  A label outside [0, S)
 *                  (-1 is the documented spelling) leaves the snapshot alone: its column of Y equals its column of X --
 *                  copied when Y != X, not touched when Y == X.
 *   apply, restore == 0:  y = fl(x - mean), then y = fl(y / sd) if sd is given (the correctly rounded fp32 divide of K13)
 *   apply, restore != 0:  y = x, then y = fl(y sd) if sd is given, then y = fl(y + mean): two roundings, never an FMA
 *                  Y == X with ldy == ldx runs in place; any other overlap of the two address ranges is refused.
 * No workspace, no allocation, no synchronisation, no atomics: results are bit-wise reproducible.
 * Memory: only the logical elements of X, mean, sd, order[0 .. n_order), start[0 .. S] and slot[0 .. T) are read, only the
 * logical S x m elements of mean / sd and m x T elements of Y are written.  No alignment is asked for beyond that of the
 * element types: a 16-byte aligned X with ldx % 4 == 0 is summed with 16-byte loads (4 rows per lane) when the launch
 * still fills the chip that way, anything else one dword per lane; apply stores full chunks of Y as aligned 16-byte
 * stores whatever Y and ldy are and reads X, mean and sd with 16-byte loads where their addresses allow it -- all with
 * the same bits.
 * Values: a non-finite X[i, t] reaches row i of the slots that list t (apply: element (i, t)) and nothing else; integer
 * data with sums below 2^53 and exact quotients come out exactly; 2^e X gives 2^e mean and 2^e sd bit for bit, and in
 * apply 2^e on X and mean scales Y by 2^e bit for bit (magnitudes as above).
 * A refused call (DMDX_E_INVALID: a null X, order, start, mean, sd of dmdx_clim_std_f32, slot or Y; S < 1; ldx, ldc, ldy
 * or -- with sd given -- lds < m; ddof outside 0 .. 1; a negative size; a size >= 2^31; X and Y overlapping other than in
 * place) has written nothing.  dmdx_clim_apply_f32 also refuses, in place too, (T - 1) ldx + m or (T - 1) ldy + m >= 2^60
 * elements, as K22 does.  m == 0 or T == 0 returns 0 after the checks; mean and std still fill their S x m output
 * (with NaN) when T == 0 and m > 0. */
int dmdx_clim_mean_f32(const float* X, int64_t m, int64_t T, int64_t ldx, const int32_t* order, int64_t n_order,
                       const int32_t* start, int64_t S, float* mean, int64_t ldc, void* stream);
int dmdx_clim_std_f32(const float* X, int64_t m, int64_t T, int64_t ldx, const int32_t* order, int64_t n_order,
                      const int32_t* start, int64_t S, const float* mean, int64_t ldc, int ddof, float* sd, int64_t lds,
                      void* stream);
int dmdx_clim_apply_f32(const float* X, int64_t m, int64_t T, int64_t ldx, const int32_t* slot, int64_t S,
                        const float* mean, int64_t ldc, const float* sd /* nullable */, int64_t lds, int restore,
                        float* Y, int64_t ldy, void* stream);

/* ---- K25: empirical quantiles of the snapshots per slot -- the percentile thresholds of K24 ------------------------------
 * The thresholds published for fields that are not normal (precipitation, wind speed, daily maxima) are percentiles of
 * a calendar slot: the 10th / 90th percentile of a +-2-day window (ETCCDI, TX90p), terciles.  X, order, n_order, start
 * and S are those of dmdx_clim_mean_f32, read the same way: start clamped to [0, n_order], an entry of order outside
 * [0, T) skipped, not counted and never used as an address; a snapshot may be listed in several slots and more than
 * once in one.  n_s = the counted entries of slot s.  q: J doubles ON THE HOST, each in [0, 1], 1 <= J <=
 * dmdx_clim_quantile_max_q() = DMDX_CLIM_QUANTILE_MAX_Q (4 = DMDX_EXCEED_MAX_THR).
 *   out[(j S + s) ldo + i]   quantile q[j] of row i over the members of slot s, ldo >= m: K24's thr layout ("column
 *                            j S + s"), so out is the thr operand of dmdx_exceed_* with ldthr = ldo.
 * Order: by the key of the bit pattern u -- ~u if the sign bit is set, u | 0x80000000 otherwise --, a total order:
 * -0.0 before +0.0, the infinities and the denormals ordinary values, nothing flushed; x_(0) <= ... <= x_(n_s - 1).
 * Position, IEEE fp64, the product rounded once:  h = q[j] (n_s - 1),  lo = floor(h),  g = h - floor(h).
 *   method 0 (linear, numpy's default, type 7) as above;  1 (lower) g := 0;  2 (higher) lo := ceil(h), g := 0.
 * Result: with g == 0 the bits of x_(lo), unchanged; otherwise d = fp64(x_(lo + 1)) - fp64(x_(lo)), p = d g,
 * r = fp64(x_(lo)) + p, each rounded, none fused, then one rounding to fp32 (Inf - Inf: a NaN of arithmetic, no
 * contractual bits).  n_s == 0: the quiet NaN 0x7FC00000 for every j; a NaN among the counted members of (slot, row):
 * 0x7FC00000 for every j of that (slot, row) and nothing else changes.  2^e X gives 2^e out bit for bit (no overflow,
 * no underflow).  No atomics, no workspace, no allocation, no synchronisation; the bits depend on the operands only --
 * not on the body that ran, the launch geometry, the alignment of X or ldx.
 * Bodies, chosen per slot by the length L of its clamped list (skipped entries included): with C =
 * dmdx_clim_quantile_max_staged() / 4, L <= C stages the keys of 64 rows in LDS, L <= 2 C those of 32 rows, L <= 4 C
 * those of 16 rows (one read of X each); a longer list, or every list with streamed != 0, re-reads its members from
 * global memory in every step of the selection (no limit on L, no speed).
 * Memory: only logical elements of X are read, every logical element of out is written, nothing else; no alignment
 * beyond that of the elements.  A refused call (DMDX_E_INVALID: a null X, order, start, q or out; S < 1; J outside
 * 1 .. 4; a q[j] that is NaN or outside [0, 1]; method outside 0 .. 2; ldx < m or ldo < m; a negative size; a size or
 * J S >= 2^31) has written nothing.  m == 0 returns 0 after the checks; T == 0 with m > 0 fills out with the NaN. */
#define DMDX_CLIM_QUANTILE_MAX_Q 4
int dmdx_clim_quantile_max_q(void);
int dmdx_clim_quantile_max_staged(void);
int dmdx_clim_quantile_f32(const float* X, int64_t m, int64_t T, int64_t ldx, const int32_t* order, int64_t n_order,
                           const int32_t* start, int64_t S, const double* q /* HOST, J values */, int64_t J, int method,
                           int streamed, float* out, int64_t ldo, void* stream);

/* ---- K20: rows (grid points) with a missing value, and one value for all of them -------------------------------------
 * What lets a field with a static mask -- sea-surface temperature, missing over land in every file -- through the
 * decomposition: a grid point that is missing in any snapshot takes no part (its row of X becomes 0, which gives a zero
 * row of U) and comes back as missing.  X is a row block as everywhere, here with the snapshots first: n snapshots of m
 * floats, snapshot j at X + j ldx, ldx >= m.
 *   count   count[i] += the number of j < n with X[j, i] not finite, i < m (device int32).  It ADDS: time slabs and
 *           repeated calls accumulate, the caller zeroes it once.  "Not finite" is the bit pattern with an exponent of
 *           all ones (every NaN payload, +Inf, -Inf), tested on integers: denormals, +-0 and +-FLT_MAX are finite
 *           whatever floating-point options the build has.  One read of X; the partial counts of the time splits of the
 *           launch meet in integer atomics, whose result does not depend on their order: bit-wise reproducible.
 *   apply   X[j, i] = value for every j < n of the rows with count[i] != 0.  A row with count[i] == 0 is neither read
 *           nor written; X is not read at all: the traffic is the stores of the masked rows and m ints.  `value` is
 *           stored with its bits (-0.0, a NaN).  The same call zeroes the masked rows of X, of a (k, rows) block of U^T,
 *           and puts NaN on the masked rows of a stored field.
 * Memory: only logical elements of X are read (count) or written (apply), only count[0 .. m) is read / updated.  No
 * alignment is asked for beyond that of the elements: a 16-byte aligned X with ldx % 4 == 0 moves 16 bytes per lane
 * (the ragged last quad element by element), anything else one dword per lane, with the same results.  m need not be
 * a multiple of 4.  n == 0 or m == 0 returns 0 and touches nothing (null pointers are allowed then).  A refused call
 * (DMDX_E_INVALID: a negative size, a size >= 2^31, ldx < m, a null or misaligned X or count) has written nothing. */
int dmdx_row_missing_count_f32(const float* X, int64_t n, int64_t m, int64_t ldx, int32_t* count, void* stream);
int dmdx_row_mask_apply_f32(float* X, int64_t n, int64_t m, int64_t ldx, const int32_t* count, float value, void* stream);

/* ---- K21: least-squares regression of every row of a row block on a small temporal design, fitted and removed --------
 * The companion of K18 for what is not a class of the calendar: an intercept, a polynomial trend, annual and diurnal
 * harmonics and user series (an ENSO index) as the p <= dmdx_treg_max_p() (8) columns of a design matrix D (T x p).  The
 * host forms D and W = (D^T D)^-1 D^T (p x T) in fp64; both are data here.  X is a row block as everywhere: T columns
 * (snapshots) of m floats, ldx >= m.
 *   W      (device fp64) W[j ldw + t], ldw >= T.         D   (device fp64) D[t ldd + j], ldd >= p.
 *   coef   (device fp32) coef[j ldc + i], p x m, ldc >= m.
 *   fit    time is cut into segments of `seg` >= 1 snapshots, [0, seg), [seg, 2 seg), ...  For row i and regressor j:
 *            tot = +0.0; for every segment in ascending order { acc = +0.0;
 *              for t ascending in the segment { q = fp64(X[i, t]) * W[j, t] (rounded); acc = acc + q; }  tot = tot + acc; }
 *            coef[j, i] = fp32(tot)
 *          all in fp64, never an FMA.  The partition is part of the result and the launch geometry is not: with
 *          `workspace` (dmdx_treg_fit_workspace_bytes(m, T, p, seg) bytes = ceil(T / seg) p m doubles, no initialisation
 *          needed) every segment is summed by workgroups of its own and a second kernel adds the partials in ascending
 *          order; with workspace == NULL one lane walks the segments of its rows one after another.  Both give the same
 *          bits.  seg >= T is the single chain.  All p sums of a row are formed in one lane: X is read once whatever p is.
 *   apply  f = +0.0; for j ascending { q = fp64(coef[j, i]) * D[t, j] (rounded); f = f + q; }
 *          restore == 0: y = fp32(fp64(x) - f)      restore != 0: y = fp32(fp64(x) + f)      -- one rounding to fp32.
 *          Y == X with ldy == ldx runs in place; any other overlap of the two address ranges is refused.
 * No allocation, no synchronisation, no atomics: results are bit-wise reproducible.
 * Memory: only the logical elements of X, W, D and coef are read, only the logical p x m elements of coef, m x T elements
 * of Y and the declared workspace bytes are written.  No alignment is asked for beyond that of the element types: a
 * 16-byte aligned X with ldx % 4 == 0 is summed with 16-byte loads (4 rows per lane, the ragged last quad element by
 * element), anything else one dword per lane; apply stores full chunks of Y as aligned 16-byte stores whatever Y and
 * ldy are -- all with the same bits.
 * Values: a non-finite X[i, t] makes the p coefficients of row i non-finite and reaches nothing else; a row of zeros has
 * coefficients of +0.0 whatever the signs of W; integer X with W on a binary grid and sums below 2^53 come out exactly.
 * A refused call (DMDX_E_INVALID: a null X, W, D, coef or Y; a negative size; m, T, seg or a leading dimension >= 2^31;
 * ldx, ldc or ldy < m; ldw < T; ldd < p; p outside 1 .. 8; seg < 1; a pointer not aligned to its element; a workspace
 * smaller than asked for; X and Y overlapping other than in place) has written nothing.  dmdx_treg_apply_f32 also
 * refuses, in place too, (T - 1) ldx + m or (T - 1) ldy + m >= 2^60 elements, as K22 does.  m == 0 or T == 0 returns 0
 * after the checks without a launch: coef of T == 0 is not written. */
int dmdx_treg_max_p(void);
size_t dmdx_treg_fit_workspace_bytes(int64_t m, int64_t T, int64_t p, int64_t seg);
int dmdx_treg_fit_f32(const float* X, int64_t m, int64_t T, int64_t ldx, const double* W, int p, int64_t ldw, int64_t seg,
                      float* coef, int64_t ldc, void* workspace /* nullable */, size_t workspace_bytes, void* stream);
int dmdx_treg_apply_f32(const float* X, int64_t m, int64_t T, int64_t ldx, const double* D, int p, int64_t ldd,
                        const float* coef, int64_t ldc, int restore, float* Y, int64_t ldy, void* stream);

/* ---- K26: lagged second moments of every row of a row block: autocorrelation and the persistence baselines ------------
 * The sums behind autocovariance / autocorrelation, the persistence, damped-persistence and climatology baselines of a
 * forecast score and the effective sample size of a trend map, for L <= dmdx_lag_moments_max_lags() (8) lags in one read
 * of X.  X is a row block as everywhere: T columns (snapshots) of m floats, ldx >= m.
 *   mu     (device fp32, nullable) one centre per row.       lags   (HOST int32) L lags, strictly ascending, 0 <= tau < T.
 *   out    (device fp64) 1 + 3L planes of m doubles, plane q at out + q ldo, ldo >= m.  Nothing is rounded to fp32.
 * For row i:  d_t = fp64(x_t) - fp64(mu) (one rounded subtraction; with mu == NULL d_t = fp64(x_t), no operation),
 * sq_t = d_t d_t (rounded), pr_u = d_{u - tau} d_u (rounded), indexed by the LATER snapshot u in [tau, T).
 * segsum(v, I): time is cut into segments of `seg` >= 1 snapshots, [0, seg), [seg, 2 seg), ... as in K21;
 *     tot = +0.0; for every segment in ascending order { acc = +0.0; for t ascending in I and the segment { acc = acc + v_t; }
 *     tot = tot + acc; }            -- all in fp64, never an FMA; segments that hold no index of I are included.
 *   plane 0           S   = segsum(sq, [0, T))
 *   plane 1 + l       P_l = segsum(pr, [tau_l, T))
 *   plane 1 + L + l   H_l = segsum(sq, [0, tau_l))        the head the later members of the pairs miss
 *   plane 1 + 2L + l  E_l = segsum(sq, [T - tau_l, T))    the tail the earlier members miss
 * so that S - E_l and S - H_l are the squares of the earlier and of the later members, and T - tau_l the pairs.
 * The partition is part of the result and the launch is not: with `workspace` (dmdx_lag_moments_workspace_bytes(m, T, L,
 * seg) bytes = ceil(T / seg) (1 + L) m doubles, no initialisation needed) every segment of S and P is summed by workgroups
 * of its own and a second kernel adds the partials in ascending order; with workspace == NULL one lane walks the segments
 * of its rows.  Both give the same bits.  The walk is meant for a T of a few segments or few rows: it has 1 / segments of
 * the split's workgroups, re-reads the ring's snapshots at every segment start, and with more than 4 lags its 16-byte
 * body runs one wave per SIMD where the split runs two: pass the workspace whenever T > seg on a full row block.
 * H and E come from a small pass of their own over the first and the last tau_max
 * snapshots.  The earlier member of a pair with tau <= dmdx_lag_moments_ring() (16) is kept by its lane in LDS; for a
 * larger lag, or for every lag with flags bit 0 set, it is a second load from the caches: the same bits either way, and
 * a mixed list uses each per lag in one launch.  No other bit of flags is defined.
 * No allocation, no synchronisation, no atomics: results are bit-wise reproducible.
 * Memory: only the logical elements of X and mu are read (X is never written), only the logical (1 + 3L) x m elements of
 * out and the declared workspace bytes are written.  out and workspace are 8-byte aligned; X and mu need no alignment
 * beyond their elements: a 16-byte aligned X with ldx % 4 == 0 is read with 16-byte loads (4 rows per lane, the ragged
 * last quad element by element), anything else one dword per lane, with the same bits.
 * Values: a non-finite X[i, t] reaches the planes of row i whose index sets hold t and nothing else; a row of zeros
 * with mu == NULL gives +0.0 in every plane.
 * A refused call (DMDX_E_INVALID: L outside 1 .. 8; null lags; lags not strictly ascending, negative or >= T; seg < 1; an
 * undefined flag bit; a negative size; m, T, seg or a leading dimension >= 2^31; ldx or ldo < m; a pointer not aligned
 * to its element; out overlapping X; a workspace smaller than asked for; a null X or out with m T > 0) has written
 * nothing.  m == 0 or T == 0 returns 0 after the checks without a launch (no lag is compared with T == 0). */
int dmdx_lag_moments_max_lags(void);
int dmdx_lag_moments_ring(void);
size_t dmdx_lag_moments_workspace_bytes(int64_t m, int64_t T, int64_t L, int64_t seg);
int dmdx_lag_moments_f32(const float* X, int64_t m, int64_t T, int64_t ldx, const float* mu /* nullable */,
                         const int32_t* lags /* host */, int L, int64_t seg, double* out, int64_t ldo, int flags,
                         void* workspace /* nullable */, size_t workspace_bytes, void* stream);

/* ---- K27: spell and exceedance-count indices of every row of a row block, per threshold and period ------------------
 * What climate users compute first from percentile thresholds (K25) or fixed ones, on an analysis or a forecast field:
 * the snapshots of a year beyond the threshold (TX90p / TN10p), those in runs of at least 6 (WSDI / CSDI), the longest
 * run (CDD / CWD), and where the first and the last such run of a season lie (heat-wave onset, first and last frost).  X
 * is a row block as everywhere: T columns (snapshots) of m floats, ldx >= m, only read.  thr (m x (J S), ldthr >= m) and
 * slot (T device int32, nullable: every snapshot in slot 0) are K24's: column j S + s holds threshold j of every row for
 * slot s; 1 <= J <= dmdx_spell_max_thresholds() = DMDX_SPELL_MAX_THR (4), S >= 1.
 *   bounds     (HOST int32) P + 1 values, 0 <= b_0 < b_1 < ... < b_P <= T, 1 <= P <= dmdx_spell_max_periods() =
 *              DMDX_SPELL_MAX_PERIODS (128; they travel by value, a caller with more periods makes several calls).
 *              Period p is the snapshots [b_p, b_{p+1}); snapshots outside [b_0, b_P) are not read.
 *   min_len    (HOST int32) J values >= 1: the shortest run of threshold j that qualifies.
 *   above_mask bit j set: the event of threshold j is x > h;  clear: x < h.  Bits at or above J must be 0.
 * For row i, threshold j and snapshot t of a period, with x = X[i, t] and h = thr[i, j S + slot[t]]:
 *   valid  v_t = x is finite (K20's test of the bit pattern)  and  slot[t] lies in 0 .. S - 1  and  h is not NaN
 *   event  e_t = v_t and (x > h or x < h, as above_mask says): a strict IEEE comparison, a tie is no event, an infinite
 *          threshold is a threshold
 *   run    a maximal set of consecutive t INSIDE ONE PERIOD with e_t true: a period boundary cuts a run (spells do not
 *          span years, as in climdex), an invalid snapshot ends one.  A run QUALIFIES if its length is >= min_len[j].
 * The DMDX_SPELL_NQ = 7 results, int32, at out[((j 7 + q) P + p) ldo + i], ldo >= m:
 *   0 n_valid     the number of v_t               1 n_event      the number of e_t
 *   2 n_spell     the qualifying runs             3 n_in_spell   the sum of their lengths
 *   4 longest     the length of the longest run, qualifying or not; 0 if there is none
 *   5 first       t - b_p of the first snapshot of the first qualifying run; -1 if there is none
 *   6 last        t - b_p of the last snapshot of the last qualifying run; -1 if there is none
 * Every period is cut from its own start into pieces of `seg` >= 1 snapshots, N = sum_p ceil((b_{p+1} - b_p) / seg)
 * pieces in all.  With `workspace` (dmdx_spell_workspace_bytes(m, bounds, P, J, seg) bytes = N J m DMDX_SPELL_WS_WORDS
 * int32, no initialisation needed) every piece is scanned by workgroups of its own into a record per (row, j) -- valid,
 * events, the run at its head, the run at its tail, and what the runs strictly inside closed to -- and a second kernel
 * merges the records of a period in ascending order: a piece of events only extends the carry; otherwise carry + head
 * is a run, the interior is added and the carry becomes the tail; the carry is closed at the period's end.  With
 * workspace == NULL one lane walks the periods of its rows.  The results are integers and the merge is exact: both forms
 * and every seg give the same values -- here the partition is NOT part of the result.  The walk has one workgroup row:
 * pass the workspace whenever there is more than one piece on a full row block.
 * The thresholds of a row are loaded again only when slot[t] changes: X is read once, thr once per change of slot.
 * No allocation, no synchronisation, no atomics, no copy.
 * Memory: only the logical elements of X in [b_0, b_P), of slot in [b_0, b_P) and of the columns of thr they name are
 * read; only the logical J x 7 x P x m elements of out, every one of them, and the declared workspace bytes are written.
 * X, thr, slot, out and workspace need no alignment beyond 4 bytes: a 16-byte aligned X with ldx % 4 == 0 is read with
 * 16-byte loads (4 rows per lane, the ragged last quad element by element), anything else one dword per lane.
 * A refused call (DMDX_E_INVALID: J outside 1 .. 4; S < 1; P outside 1 .. 128; null bounds or min_len; bounds not
 * strictly ascending or outside [0, T]; min_len[j] < 1; seg < 1; a bit of above_mask at or above J; any bit of flags
 * (none is defined; reserved for spells that span periods); a negative size; m, T, S, J S, seg or a leading dimension
 * >= 2^31; ldx, ldthr or ldo < m; a pointer not aligned to its element; out overlapping X or thr; a workspace smaller
 * than asked for; a null X, thr or out with m > 0) has written nothing.  m == 0 returns 0 after the checks without a
 * launch.  dmdx_spell_workspace_bytes returns 0 for arguments the call would refuse. */
#define DMDX_SPELL_NQ 7
#define DMDX_SPELL_MAX_THR 4
#define DMDX_SPELL_MAX_PERIODS 128
#define DMDX_SPELL_WS_WORDS 9
int dmdx_spell_max_thresholds(void);
int dmdx_spell_max_periods(void);
size_t dmdx_spell_workspace_bytes(int64_t m, const int32_t* bounds /* host */, int P, int J, int64_t seg);
int dmdx_spell_f32(const float* X, int64_t m, int64_t T, int64_t ldx, const float* thr, int64_t ldthr, int J, int64_t S,
                   const int32_t* slot /* device, nullable */, unsigned above_mask, const int32_t* min_len /* host, J */,
                   const int32_t* bounds /* host, P + 1 */, int P, int64_t seg, int32_t* out, int64_t ldo, int flags,
                   void* workspace /* nullable */, size_t workspace_bytes, void* stream);

/* ---- K29: per-period extremes and totals of a daily statistic of every row of a row block ------------------------------
 * The other half of the standard climate indices next to K27's counts: the hottest and the coldest day of a year and when
 * they fell (TXx, TNn, TXn, TNx), the mean diurnal range (DTR), the wettest day and the wettest five days (Rx1day, Rx5day),
 * totals and wet-day totals (PRCPTOT, SDII), the share of very wet days (R95pTOT), degree days.  X is a row block as
 * everywhere: T columns (snapshots) of m floats, ldx >= m, only read.
 *   bounds     (HOST int32) P + 1 values, 0 <= b_0 < b_1 < ... < b_P <= T, 1 <= P <= dmdx_period_stats_max_periods() =
 *              DMDX_PSTAT_MAX_PERIODS (128; they travel by value, a caller with more periods makes several calls).
 *              Period p is the snapshots [b_p, b_{p+1}); snapshots outside [b_0, b_P) are not read.
 *   thr        (device fp32, nullable) one threshold per row.
 * For row i and period p:
 *   days   the period is cut from its own start into groups of `group` = g >= 1 snapshots: day k is [b_p + k g,
 *          min(b_p + (k + 1) g, b_{p+1})), D_p = ceil((b_{p+1} - b_p) / g) days, the last one may be ragged.  A snapshot
 *          counts if it is finite (K20's test of the bit pattern: NaN and +-Inf are missing); c_k is the number of finite
 *          snapshots of day k, and the day is VALID iff c_k >= min_count, 1 <= min_count <= g (a ragged day shorter than
 *          min_count is never valid).
 *   d_k    the day value, fp64, from the finite snapshots of the day in ascending t:  s = +0.0; s = s + fp64(x)
 *          (rounded, never an FMA);  hi = the first finite value, replaced when x > hi;  lo likewise when x < lo (strict:
 *          a tie keeps the earlier value, -0.0 followed by +0.0 stays -0.0).  inner selects  SUM: s;  MEAN: s / fp64(c_k)
 *          (one correctly rounded division);  MAX: fp64(hi);  MIN: fp64(lo);  RANGE: fp64(hi) - fp64(lo) (one rounded
 *          subtraction).
 *   r_k    the running sum over `window` = w days, 1 <= w <= dmdx_period_stats_max_window() = DMDX_PSTAT_MAX_WINDOW (8),
 *          that never crosses a period: r_k exists for k >= w - 1 iff the days k - w + 1 .. k are all valid;
 *          r = d_{k-w+1}, then r = r + d_u for u ascending -- recomputed for every k in that order, never a sliding
 *          update, so it does not depend on where a piece starts.  w = 1: r_k = d_k, no operation.
 *   e_k    the event: r_k exists, thr != NULL, h = thr[i] is not NaN, and r_k > fp64(h); r_k < fp64(h) with
 *          DMDX_PSTAT_BELOW; >= / <= with DMDX_PSTAT_INCLUSIVE.  An infinite threshold is a threshold.
 * The DMDX_PSTAT_NQ = 8 planes, fp64, at out[(q P + p) ldo + i], ldo >= m:
 *   0 n            the number of existing r_k
 *   1 max          the first r_k, replaced when r_k > max (strict); NaN when n = 0
 *   2 argmax       the k of that value (the day of the period that is the window's last); -1 when n = 0
 *   3 min          as plane 1, replaced when r_k < min           4 argmin   as plane 2
 *   5 total        segsum(r_k over the existing k)
 *   6 event total  segsum(r_k over e_k)                          7 event count   the number of e_k
 * With thr == NULL planes 6 and 7 are +0.0.
 * segsum is K26's, applied to days: the period is cut from its own start into pieces of `seg` >= 1 days; per piece in
 * ascending order { acc = +0.0; acc = acc + v for its terms ascending; } tot = tot + acc, from tot = +0.0; pieces
 * without a term are included.  The partition is part of planes 5 and 6 and of nothing else; the launch form is part of
 * nothing: with `workspace` (dmdx_period_stats_workspace_bytes(m, bounds, P, group, seg) bytes = N 8 m doubles, N = sum_p
 * ceil(D_p / seg), no initialisation needed) every piece is scanned by workgroups of its own -- it reads the up to
 * (w - 1) g snapshots before its start inside its period again -- into a record per row, and a second kernel merges
 * the records of a period in ascending order: a strict compare (the earlier piece wins a tie), counts added, tot + acc.
 * With workspace == NULL one lane walks the periods of its rows.  Both give the same bits.  The walk has one workgroup
 * row: pass the workspace whenever there is more than one piece on a full row block.
 * No allocation, no synchronisation, no atomics.
 * Memory: only the logical elements of X in [b_0, b_P) and of thr are read; only the logical 8 x P x m elements of out,
 * every one of them, and the declared workspace bytes are written.  out and workspace are 8-byte aligned; X and thr need
 * no alignment beyond their elements: a 16-byte aligned X with ldx % 4 == 0 is read with 16-byte loads (4 rows per lane,
 * the ragged last quad element by element), anything else one dword per lane, with the same bits.
 * A refused call (DMDX_E_INVALID: P outside 1 .. 128; null bounds; bounds not strictly ascending or outside [0, T];
 * group < 1; inner outside 0 .. 4; window outside 1 .. 8; min_count outside 1 .. group; seg < 1; an undefined flag bit; a
 * negative size; m, T, group, seg or a leading dimension >= 2^31; ldx or ldo < m; a pointer not aligned to its element;
 * out overlapping X or thr; a workspace smaller than asked for; a null X or out with m > 0) has written nothing.  m == 0
 * returns 0 after the checks without a launch.  dmdx_period_stats_workspace_bytes returns 0 for arguments the call
 * would refuse. */
#define DMDX_PSTAT_NQ 8
#define DMDX_PSTAT_MAX_WINDOW 8
#define DMDX_PSTAT_MAX_PERIODS 128
enum { DMDX_PSTAT_SUM = 0, DMDX_PSTAT_MEAN = 1, DMDX_PSTAT_MAX = 2, DMDX_PSTAT_MIN = 3, DMDX_PSTAT_RANGE = 4 };
#define DMDX_PSTAT_BELOW 1u       /* event: r < h instead of r > h */
#define DMDX_PSTAT_INCLUSIVE 2u   /* >= / <= instead of the strict comparison */
int dmdx_period_stats_max_window(void);
int dmdx_period_stats_max_periods(void);
size_t dmdx_period_stats_workspace_bytes(int64_t m, const int32_t* bounds /* host */, int P, int64_t group, int64_t seg);
int dmdx_period_stats_f32(const float* X, int64_t m, int64_t T, int64_t ldx,
                          const int32_t* bounds /* host, P + 1 */, int P, int64_t group, int inner, int window,
                          int64_t min_count, const float* thr /* device, m, nullable */, int64_t seg,
                          double* out, int64_t ldo, unsigned flags,
                          void* workspace /* nullable */, size_t workspace_bytes, void* stream);

/* ---- K22: a FIR filter along time with an output stride: daily means, low-pass + decimation, band-pass ----------------
 * The fourth preparation step on the device, before K18 and K21: a weighted sum over a sliding window of snapshots.  X
 * and Y are row blocks as everywhere: snapshot t of X at X + t ldx, output snapshot u of Y at Y + u ldy, m floats each,
 * ldx, ldy >= m.  h holds L <= dmdx_tfilt_max_taps() (2048) device doubles.  The caller chooses T_out with
 * (T_out - 1) stride + L <= T: "valid" windows only, no padding, no reflection; a time slab with its halo is a pointer
 * offset.  For row i and output u:
 *     acc = +0.0; for j = 0 .. L - 1 ascending { q = fp64(X[i, u stride + j]) * h[j] (rounded); acc = acc + q; }
 *     Y[i, u] = fp32(acc)
 * all in fp64, never an FMA, one rounding to fp32; taps are not folded.  The launch geometry is not part of the result:
 * a lane that walks the union window of a run of outputs adds every snapshot to each output whose window holds it, in
 * ascending t, which is ascending j for every one of them.
 * No workspace, no allocation, no atomics, no synchronisation: results are bit-wise reproducible.
 * Memory: only the logical elements of X that some window addresses are read -- never the snapshots behind the last
 * window, never the snapshots between two windows where stride > L -- and only h[0 .. L); only the logical m x T_out
 * elements of Y are written.  No alignment is asked for beyond that of the element types: full chunks of 4 rows of Y go
 * out as aligned 16-byte stores whatever Y and ldy are (the chunks of an output start at the 16-byte boundary at or
 * before its row 0, the ragged first and last chunk element by element); X is read with 16-byte loads, 4 rows per lane,
 * where ldx % 4 == 0 and X + u ldx shares the 16-byte phase of Y + u ldy (an aligned X and an aligned Y with ldx % 4 ==
 * ldy % 4 == 0), element by element otherwise -- all with the same bits.
 * Values: IEEE, nothing more.  A non-finite X[i, t] reaches exactly the outputs of row i whose window holds t -- under a
 * zero tap too (Inf * 0 is NaN) -- and nothing else; a row of zeros gives +0.0 whatever the signs of h; 2^e X gives 2^e Y
 * bit for bit (magnitudes as above); integer X with taps on a binary grid and sums below 2^53 come out exactly.
 * A refused call (DMDX_E_INVALID: a null X, h or Y; a negative size; L < 1 or L > dmdx_tfilt_max_taps(); stride < 1;
 * (T_out - 1) stride + L > T; ldx or ldy < m; m, T, T_out, stride or a leading dimension >= 2^31; (T - 1) ldx + m or
 * (T_out - 1) ldy + m >= 2^60 elements (the overlap test works on byte extents that fit 64 bits); a pointer not aligned to
 * its element; any overlap of the address ranges of X (all T snapshots) and Y: there is no in-place form) has written
 * nothing.  m == 0 or T_out == 0 returns 0 after the checks without a launch. */
int dmdx_tfilt_max_taps(void);
int dmdx_tfilt_f32(const float* X, int64_t m, int64_t T, int64_t ldx, const double* h, int64_t L, int64_t stride,
                   float* Y, int64_t T_out, int64_t ldy, void* stream);

/* ---- K23: the area-weighted block mean over fy x fx cells of the latitude / longitude grid (coarsening) -----------------
 * The preparation step of the space axis, before K22: ERA5 at 0.25 degrees becomes the 1 degree grid a DMD is fitted on,
 * with one read of X and one write of X / (fy fx).  X is a row block as everywhere: snapshot t at X + t ldx.  A snapshot
 * holds P planes (variable x level), plane p at p ldp, ldp >= nlat nlon; the slack is pad (that of pad4) and is never
 * read.  Inside a plane latitude row i and longitude j sit at i nlon + j, the project's flatten order.  Y is laid out the
 * same way: Y[t ldy + p ldq + I NLON + J], ldq >= NLAT NLON.  Output cell (I, J) covers the fine rows lat0 + I fy .. + fy - 1
 * and the longitudes lon0 + J fx .. + fx - 1: whole cells only, as K22 has valid windows only -- the caller chooses NLAT and
 * NLON with lat0 + NLAT fy <= nlat and lon0 + NLON fx <= nlon, and rows and longitudes outside the cells are not looked at
 * (721 latitudes and fy = 4: one pole row is dropped).  w holds nlat device doubles, one weight per fine latitude row of
 * the plane (cos of the latitude, an exact band area, or ones; the host forms it).  Per snapshot t, plane p, cell (I, J):
 *     num = +0.0; den = +0.0; full = +0.0
 *     for a = 0 .. fy - 1 ascending, i = lat0 + I fy + a:
 *         r = +0.0; c = 0
 *         for b = 0 .. fx - 1 ascending: x = X[t, p, i, lon0 + J fx + b];
 *                                        if (!skipna || finite(x)) { r = r + fp64(x); c = c + 1; }
 *         num = num + w[i] * r; den = den + w[i] * fp64(c); full = full + w[i] * fp64(fx);   (products rounded, then the sums)
 *     Y = (den == 0 || den < min_frac * full) ? quiet NaN (0x7fc00000) : fp32(num / den)
 * all in fp64, never an FMA, one rounding to fp32.  finite(x) is K20's test of the bit pattern: an exponent of all ones is
 * not finite.  With skipna == 0, den == full, and a non-finite x reaches its own cell by IEEE arithmetic and nothing else.
 * The launch geometry is not part of the result: a cell is formed by one lane; no atomics, no workspace, no allocation, no
 * synchronisation: results are bit-wise reproducible.  So a constant field comes out constant bit for bit, 2^e X gives
 * 2^e Y, a cell of zeros of either sign gives +0.0, and integer X with unit weights and fy fx a power of two gives the
 * exact mean.
 * Memory: only elements of X inside some cell are read -- no dropped trailing rows or longitudes, nothing before lat0 or
 * lon0, no plane pad, nothing between (P - 1) ldp + nlat nlon and ldx -- and only w[lat0 .. lat0 + NLAT fy); only the
 * logical P NLAT NLON x T elements of Y are written.  No alignment is asked for beyond that of the element types: the fx
 * floats of a cell's fine row are read with 16-byte loads (fx = 4, 8; at fx = 2 a lane forms four neighbouring cells of a
 * coarse row from two such loads and stores them with 16 bytes) where the addresses allow it, and element by element
 * otherwise and for every other fx; a wave stores 64 (256) consecutive cells.  All give the same bits.
 * A refused call (DMDX_E_INVALID: a null X, w or Y; a negative size; fy or fx outside 1 .. dmdx_coarsen_max_factor() (64);
 * lat0 or lon0 negative, or cells that do not fit; ldp < nlat nlon or ldq < NLAT NLON; ldx < (P - 1) ldp + nlat nlon or
 * ldy < (P - 1) ldq + NLAT NLON; any size or leading dimension >= 2^31; an extent >= 2^60 elements; min_frac outside [0, 1]
 * or NaN; a pointer not aligned to its element; any overlap of the address ranges of X and Y: there is no in-place form)
 * has written nothing and made no HIP call.  T, P, NLAT or NLON == 0 returns 0 after the checks without a launch. */
int dmdx_coarsen_max_factor(void);
int dmdx_coarsen_f32(const float* X, int64_t T, int64_t ldx, int64_t P, int64_t ldp, int64_t nlat, int64_t nlon,
                     const double* w, int fy, int fx, int64_t lat0, int64_t lon0, int64_t NLAT, int64_t NLON, int skipna,
                     double min_frac, float* Y, int64_t ldy, int64_t ldq, void* stream);

/* ---- K28: first-order conservative remapping onto another regular latitude / longitude grid ---------------------------
 * K23 takes whole fy x fx blocks.  The grids other data sets live on (1 degree with the poles, 181 x 360; 1.5 degrees,
 * 121 x 240; 5.625 degrees, offset by half a cell) cut source cells, wrap around in longitude and end in a clipped cap at
 * the poles.  Both grids are regular, so the remapping is separable: six device tables say what a target cell is made of.
 * X and Y are laid out exactly as in K23: snapshot t at X + t ldx, plane p at p ldp, ldp >= nlat nlon, the slack is pad
 * and is never read; Y[t ldy + p ldq + I NLON + J], ldq >= NLAT NLON.  Target row I overlaps the ny[I] source rows from
 * iy0[I] on, with the weights wy[I SY + a] (NLAT x SY doubles, row-major: the area of the overlap of the two latitude
 * bands); target column J overlaps the nx[J] source columns (jx0[J] + b) mod nlon, with the weights wx[J SX + b]
 * (NLON x SX doubles: the overlap in degrees).  Entries of wy and wx beyond the count are never read.  The host forms
 * the tables in fp64 (regrid.Remap).  Per snapshot t, plane p, cell (I, J):
 *     num = +0.0; den = +0.0; full = +0.0
 *     for a = 0 .. ny[I] - 1 ascending, i = iy0[I] + a:
 *         r = +0.0; c = +0.0; f = +0.0
 *         for b = 0 .. nx[J] - 1 ascending, j = (jx0[J] + b) mod nlon, u = wx[J][b], x = X[t, p, i, j]:
 *             if (!skipna || finite(x)) { r = r + u * fp64(x); c = c + u; }
 *             f = f + u
 *         num = num + wy[I][a] * r; den = den + wy[I][a] * c; full = full + wy[I][a] * f;   (products rounded, then the sums)
 *     Y = (den == 0 || den < min_frac * full) ? quiet NaN (0x7fc00000) : fp32(num / den)
 * all in fp64, every product rounded on its own, never an FMA, one rounding to fp32.  finite(x) is K20's test of the bit
 * pattern.  With wx == 1.0 and wy[I][a] = w[lat0 + I fy + a] this is K23's contract term for term: block tables give the
 * bits of dmdx_coarsen_f32.  A cell is formed by one lane; no atomics, no workspace, no allocation, no synchronisation:
 * the launch geometry is not part of the result.  So a constant field comes out constant bit for bit, 2^e X gives 2^e Y,
 * and a cell of zeros of either sign gives +0.0.
 * Memory: the contents of the tables live on the device and cannot be checked here, so the kernel is safe for any
 * contents: counts are clamped to 0 .. SY and 0 .. SX, row indices into [0, nlat), column indices are reduced modulo
 * nlon.  A bad table gives a wrong number and never an access outside the planes of X; plane pads and the slack of ldx
 * are never read, and only the logical P NLAT NLON x T elements of Y are written.  No alignment is asked for beyond that
 * of the element types: with SX <= 8 a lane reads its run of a source row as the aligned quads of that row that cover it
 * (16-byte loads; floats of the row beside the run are loaded and not used) where the run does not wrap and the address
 * of the row allows it, and element by element otherwise and for every wider SX.  All give the same bits.
 * A refused call (DMDX_E_INVALID: a null X, Y or table; a negative size; SY or SX outside 1 .. dmdx_remap_max_span() (64);
 * cells of an empty plane (NLAT NLON > 0 with nlat nlon == 0); ldp < nlat nlon or ldq < NLAT NLON; ldx < (P - 1) ldp +
 * nlat nlon or ldy < (P - 1) ldq + NLAT NLON; any size or leading dimension >= 2^31; an extent >= 2^60 elements; min_frac
 * outside [0, 1] or NaN; a pointer not aligned to its element; any overlap of the address ranges of X and Y: there is no
 * in-place form) has written nothing and made no HIP call.  T, P, NLAT or NLON == 0 returns 0 after the checks without
 * a launch. */
int dmdx_remap_max_span(void);
int dmdx_remap_f32(const float* X, int64_t T, int64_t ldx, int64_t P, int64_t ldp, int64_t nlat, int64_t nlon,
                   const int32_t* iy0, const int32_t* ny, const double* wy, int SY, const int32_t* jx0, const int32_t* nx,
                   const double* wx, int SX, int64_t NLAT, int64_t NLON, int skipna, double min_frac, float* Y, int64_t ldy,
                   int64_t ldq, void* stream);

/* ---- K30: one step of the orthomax (varimax) rotation of the leading k modes, and Kaiser's row norms --------------
 * U: m x k (ldu), the left singular vectors; R: k x k column-major (ldr), any values -- the host hands over
 * diag(s) R rounded to fp32; w: m floats, nullable (= 1), Kaiser's 1 / h.  1 <= k <= dmdx_varimax_max_k() (64).
 *     a[i, j]  = w ? fl(U[i, j] w[i]) : U[i, j]
 *     L[i, c]  = sum_j a[i, j] R[j, c]            fp32 MFMA chain, j ascending, k padded with zeros in a AND in R
 *     G[j, c] (+)= sum_i a[i, j] fl(fl(L L) L)    G: k x k column-major (ldg), fp64
 *     q[c]    (+)= sum_i fl(L L)                  k doubles
 *     f[c]    (+)= sum_i fl(fl(L L) fl(L L))      k doubles, nullable
 * U is read exactly once per call and L is never stored.  The sums over i are fp32 over one row range of at most
 * DMDX_VARIMAX_FP32_ROWS rows (shortened, as K13's, while the launch would leave CUs idle) and fp64 across the row
 * ranges, through per-unit slots in the workspace and a reduce kernel that adds the ranges in order.  No floating-point
 * atomics: the order of every sum is a function of (m, k) only, two calls give the same bits.  accumulate != 0 adds to
 * G, q and f, so that U can be passed as row blocks.
 * Error against the exact sums of the fp32 inputs, with Labs = |a| |R| and u = 2^-24:
 *     |dG| <= (4096 + 3 k + 8) u |a|^T Labs^3,  |dq| <= (4096 + 2 k + 6) u colsum(Labs^2),
 *     |df| <= (4096 + 4 k + 8) u colsum(Labs^4).
 * Memory: the operands are only read, and only inside their logical elements; with accumulate == 0 every logical
 * element of G, q and f is written and nothing else, with accumulate != 0 they are read and written.  The pads
 * ldu - m, ldr - k and ldg - k are never read for a result and never written.  No alignment is required beyond that of
 * the elements; a 16-byte aligned U with ldu % 4 == 0 selects 16-byte loads with the same values.  The workspace needs
 * no initialisation; dmdx_varimax_workspace_bytes is non-decreasing in m.
 * Values: a non-finite U[i, j] or w[i] makes every element of G, q and f non-finite, of the class numpy's fp64
 * evaluation of the formulas has.  A non-finite R[j, c] makes column c of G, q[c] and f[c] non-finite; every other
 * element keeps the bits of the run without it.  Rows past m and columns past k are exact zeros on both sides, and L
 * is zero for the rows past a row range before it is cubed: an Inf meets no pad.
 * A refused call (DMDX_E_INVALID: a null U, R, G or q; k outside 1 .. 64; m < 1; ldu < m, ldr < k or ldg < k; any size
 * >= 2^31; DMDX_E_WORKSPACE: a null or short workspace) has written nothing and made no HIP call; dmdx_last_error()
 * names the entry point.
 *
 * dmdx_row_norms_f32: h[i] = fp32(sqrt(sum_j fp64(fl(U[i, j] cscale[j]))^2)), j ascending, every square rounded before
 * it is added, cscale k floats, nullable (= 1): the communalities of Kaiser's normalisation, one streaming read of U,
 * bit for bit the numpy expression.  Any k >= 1.  Refused (DMDX_E_INVALID): a null U or h, m < 1, k < 1, ldu < m, a size
 * >= 2^31. */
#define DMDX_VARIMAX_FP32_ROWS 4096
int dmdx_varimax_max_k(void);
size_t dmdx_varimax_workspace_bytes(int64_t m, int64_t k);
int dmdx_varimax_step_f32(const float* U, int64_t m, int64_t k, int64_t ldu, const float* R, int64_t ldr, const float* w,
                          double* G, int64_t ldg, double* q, double* f, int accumulate, void* workspace,
                          size_t workspace_bytes, void* stream);
int dmdx_row_norms_f32(const float* U, int64_t m, int64_t k, int64_t ldu, const float* cscale, float* h, void* stream);

/* ---- K31: DINEOF gap filling -- the packed mask of the gaps, the standardised block, the rank-k field at the gaps ----
 * The mask is one bit per element, packed along time in words of K12's tile width: W[tw ldw + i] bit b <=> element
 * (i, 32 tw + b) is a gap, tw < ceil(T / 32), i < m, ldw >= m.  X: m x T fp32 (ldx >= m: no delay view).
 *
 * dmdx_gap_mask_f32: one read of X.  W: every logical word is written; the bit is K20's test of the bit pattern
 * (exponent all ones); bits at snapshots >= T are 0.  nmiss (int32, m entries, nullable): the gaps of every row,
 * overwritten.  sums (fp64, 2 x m, ldsum >= m, nullable): per row the sum (plane 0) and the sum of squares (plane 1) of
 * the FINITE values.  Per segment of dmdx_gap_mask_segment() (1024) snapshots one fp64 chain in ascending t from +0.0;
 * the segment results are added in ascending order; a square is the (exact) fp64 product of the converted value.  The
 * bits depend on (X, T) only: with a workspace of dmdx_gap_mask_workspace_bytes(m, T) the segments are spread over the
 * launch and a combine kernel adds their partials in order, with workspace == NULL one lane walks all segments of its
 * row.  m == 0 or T == 0 returns 0 and touches nothing.
 *
 * dmdx_gap_standardize_f32: in place, one read and one write.  mu, sigma: m floats each, nullable (0 and 1).
 *   back == 0: an element with its bit set becomes +0.0, every other fl(fl(x - mu[i]) / sigma[i]) (K13's xt, what K5
 *              leaves for the same moments); W nullable = no gaps.
 *   back != 0: every element becomes fl(fl(x sigma[i]) + mu[i]) (K12's two roundings); W is ignored.
 *
 * dmdx_gap_fill_f32: K12's field mu + sigma (U C) (U: m x k, C: k x T, 1 <= k <= dmdx_gap_fill_max_k() = 256) stored
 * into X where the bit is set, bit for bit what dmdx_expand_f32 stores at (i, t) for the same operands; where the bit is
 * clear X is neither read nor written.  change_row (m doubles, nullable, always overwritten) = sum_t bit (new - old)^2,
 * old loaded only at set bits: one rounded subtraction, one rounded square, fp32 over the 16 values of a lane in a
 * tile, fp64 over tiles and T splits in an order that is a function of (m, T); no atomics.  The workspace
 * (dmdx_gap_fill_workspace_bytes) is needed only with change_row.  A wave whose 32 words of a tile are zero skips the
 * MFMA chain and the epilogue of the tile, a workgroup whose words are all zero returns before it loads its panel of U:
 * neither changes a result.
 *
 * A refused call (DMDX_E_INVALID: a null X, W, U or C; a negative size; k outside 1 .. 256; ldx, ldw, ldu or ldsum < m,
 * ldc < k; any size or leading dimension >= 2^31; a pointer not aligned to its element; DMDX_E_WORKSPACE: a short
 * workspace, or a null one where change_row is given) has written nothing and made no HIP call; dmdx_last_error() names
 * the entry point.  m == 0 or T == 0 returns 0 after the checks without a launch. */
int dmdx_gap_mask_segment(void);
size_t dmdx_gap_mask_workspace_bytes(int64_t m, int64_t T);
int dmdx_gap_mask_f32(const float* X, int64_t m, int64_t T, int64_t ldx, uint32_t* W, int64_t ldw, int32_t* nmiss,
                      double* sums, int64_t ldsum, void* workspace, size_t workspace_bytes, void* stream);
int dmdx_gap_standardize_f32(float* X, int64_t m, int64_t T, int64_t ldx, const uint32_t* W, int64_t ldw, const float* mu,
                             const float* sigma, int back, void* stream);
int dmdx_gap_fill_max_k(void);
size_t dmdx_gap_fill_workspace_bytes(int64_t m, int64_t k, int64_t T);
int dmdx_gap_fill_f32(const float* U, int64_t m, int64_t k, int64_t ldu, const float* C, int64_t ldc, int64_t T,
                      const float* mu, const float* sigma, const uint32_t* W, int64_t ldw, float* X, int64_t ldx,
                      double* change_row, void* workspace, size_t workspace_bytes, void* stream);

/* ---- K32: the Mann-Kendall test and the Theil-Sen slope of every row of a row block ------------------------------------
 * The trend of an index series (K27 / K29: one value per year and grid point) as it is reported: annual maxima, wet-day
 * totals and spell lengths are skewed, tied and partly missing, so the slope is the median of all pairwise slopes, its
 * confidence interval two other order statistics of them, and the significance a rank test.  Y is a row block as
 * everywhere: n columns (time points) of m floats, ldy >= m, only read; 1 <= n <= dmdx_mk_max_n() = DMDX_MK_MAX_N (128).
 *   tc     (HOST fp64) the n time coordinates, finite and strictly ascending; they travel by value.
 *   rank   (device int32) J x m, ldr >= m, 1 <= J <= dmdx_sen_max_ranks() = DMDX_SEN_MAX_RANKS (4): 0-based ranks per row.
 * A point of row i is VALID iff it is finite (K20's test of the bit pattern: NaN and +-Inf are missing, as in K29);
 * y_0 .. y_{v-1} and t_0 .. t_{v-1} are the valid points of the row in ascending time, N = v (v - 1) / 2 their pairs.
 *
 * dmdx_mk_stats_f32: the DMDX_MK_NQ = 4 planes, int32, at out[q ldo + i], ldo >= m, every value an exact integer:
 *   0 v   the number of valid points
 *   1 S   sum over a < b of sgn(y_b - y_a); IEEE comparisons: > gives +1, < gives -1, equal 0; -0.0 equals +0.0
 *   2 E   the number of pairs a < b with y_a == y_b
 *   3 G   sum over a of (c_a - 1) (2 c_a + 5), c_a the number of valid b (a included) with y_b == y_a: the sum over the
 *         tie groups of g (g - 1) (2 g + 5), the tie term of Var(S); at most 128 127 261
 *
 * dmdx_sen_slopes_f32: for every pair a < b of valid points, in IEEE fp64: d = fp64(y_b) - fp64(y_a) (rounded once),
 * h = t_b - t_a (rounded once, > 0), s = d / h (one correctly rounded division), e = fp32(s) (to nearest even).  Nothing
 * is fused and nothing is flushed; no e is a NaN, +-Inf and denormals are ordinary values.  The N values are ordered by
 * K25's key of the bit pattern (~u if the sign bit is set, else u | 0x80000000: a total order, -0.0 before +0.0):
 * e_(0) <= ... <= e_(N-1).  out[j ldo + i] holds the bits of e_(rank[j ldr + i]) if 0 <= rank < N and the quiet NaN
 * 0x7fc00000 otherwise.  Rounding to fp32 is monotone: this is the fp32 rounding of the same order statistic of the
 * fp64 slopes.
 *
 * No atomics, no workspace, no allocation, no synchronisation.  The bits depend on the operands only -- not on the body
 * that ran, the launch geometry or the alignment of Y or ldy.  Memory: only the logical elements of Y and rank are
 * read; every logical element of out is written and nothing else.  No alignment is required beyond that of the elements.
 * A refused call (DMDX_E_INVALID: a null Y, out, tc or rank; n outside 1 .. 128; J outside 1 .. 4; a negative size; m or
 * a leading dimension >= 2^31; ldy, ldo or ldr < m; a pointer not aligned to its element; tc not finite or not strictly
 * ascending; out overlapping Y or rank) names the entry point in dmdx_last_error(), has written nothing and made no HIP
 * call.  m == 0 returns 0 after the checks without a launch. */
#define DMDX_MK_MAX_N 128
#define DMDX_MK_NQ 4
#define DMDX_SEN_MAX_RANKS 4
int dmdx_mk_max_n(void);
int dmdx_sen_max_ranks(void);
int dmdx_mk_stats_f32(const float* Y, int64_t m, int64_t n, int64_t ldy, int32_t* out, int64_t ldo, void* stream);
int dmdx_sen_slopes_f32(const float* Y, int64_t m, int64_t n, int64_t ldy, const double* tc /* HOST, n */,
                        const int32_t* rank /* device */, int64_t ldr, int J, float* out, int64_t ldo, void* stream);

/* ---- upper triangle of a symmetric fp64 matrix <-> packed row by row ---------------------
 * packed[i (2n - i + 1) / 2 + (j - i)] = A[i][j], j >= i: what the Gram all-reduce of the
 * row-sharded path moves (n (n + 1) / 2 doubles instead of n^2).  unpack writes both triangles. */
int dmdx_pack_triu_f64(const double* A, int64_t n, int64_t lda, double* packed, void* stream);
int dmdx_unpack_triu_f64(const double* packed, int64_t n, double* A, int64_t lda, void* stream);

/* ---- exponential basis of the optimized-DMD fit (BASELINE config 5; the reference announces the fit,
 * README.md:85,139, and holds no code for it) -----------------------------------------------------
 * Phi[i][j] = exp(alpha_j t_i), W = diag(t) Phi (nullable): alpha r complex128 (re, im interleaved),
 * t n fp64, Phi / W n x r row-major complex64 (single_precision != 0) or complex128.  The exponent
 * is formed and range-reduced in fp64 whatever the output type. */
int dmdx_exp_basis(const double* alpha, const double* t, int64_t n, int64_t r, void* Phi, void* W,
                   int single_precision, void* stream);

/* ---- measurement aid (not on the path): sustained core clock of the Gram launches ----------
 * While dev_counters3 (3 device uint64, caller-zeroed) is set, every workgroup of the batched
 * launches (dmdx_syrk_blocks_f32, dmdx_gemm_tn_blocks_f32), of dmdx_gemm_nn_skinny_f32, of K12 and of K13 adds its
 * core-clock cycles (s_memtime), its 100 MHz reference ticks
 * (s_memrealtime) and 1 to it: clock = 100 MHz * [0] / [1].  NULL (the default) switches the
 * stamps off again; bench.py's calibration block is the only caller. */
int dmdx_set_clock_probe(unsigned long long* dev_counters3);

/* ---- measurement aid (not on the path): register-only fp32 MFMA loop -----------
 * 2 workgroups of 4 waves per CU, 16 * iters v_mfma_f32_32x32x2_f32 per wave; *flops_out
 * (host pointer, nullable) receives the flops of the launch.  bench.py --calibrate times it. */
int dmdx_calib_mfma_f32(int iters, int num_cus, float* sink, double* flops_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DMDX_H */
