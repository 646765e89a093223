"""GPU parity tests: every call goes through the C ABI (libdmdx.so) and is
checked against the CPU oracle / golden fixtures.  Run on the MI355X box with
`pytest -m gpu`.  Tolerances are stated next to each check.
"""
import os

import numpy as np
import pytest
import torch

from oracle import era5_oracle as orc
from parity_utils import EPS32, col_cosines, load_golden, sv_tolerance

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def K():
    from dmd_era5_amd.kernels import default_kernels

    return default_kernels()  # raises (test fails) if libdmdx.so or the GPU is missing


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rand(rs, m, n, scale=1.0):
    return (rs.standard_normal((m, n)) * scale).astype(np.float32)


# ---------------------------------------------------------------- K1 SYRK
@pytest.mark.parametrize(
    "m,n",
    [(32, 1), (33, 5), (1, 7), (1000, 128), (4096, 192), (5000, 129), (777, 300), (20011, 515),
     (6000, 312), (4099, 440), (8192, 193)],     # last tile column of 56 columns (cfg2's n % 128): the half-width edge unit
)
def test_syrk_matches_fp64_gram(K, m, n):
    rs = np.random.RandomState(m * 1000 + n)
    X = _rand(rs, m, n)                      # (space, time)
    Xt = _dev(X.T)                           # (time, space)
    G = K.syrk(Xt).cpu().numpy()
    X64 = X.astype(np.float64)
    ref = X64.T @ X64
    absref = np.abs(X64).T @ np.abs(X64)
    # fp32 MFMA chains of <= 4096 rows (blocked summation of <= 16 chains per unit), fp64 across
    # units: error <= ~1e-6 * sum|a||b|
    assert np.all(np.abs(G - ref) <= 2e-6 * absref + 1e-30)
    assert np.array_equal(G, G.T), "both triangles must hold identical values"


def test_syrk_unaligned_ld_and_fp32_copy(K):
    rs = np.random.RandomState(7)
    m, n, ld = 1001, 67, 1003                # ld % 4 != 0 -> scalar-load path
    buf = torch.zeros((n, ld), dtype=torch.float32, device="cuda")
    X = _rand(rs, m, n)
    buf[:, :m] = _dev(X.T)
    G64, G32 = K.syrk(buf[:, :m], want32=True)
    ref = X.astype(np.float64).T @ X.astype(np.float64)
    assert np.allclose(G64.cpu().numpy(), ref, rtol=0, atol=2e-6 * np.abs(ref).max() * 10)
    assert np.allclose(G32.cpu().numpy(), ref.astype(np.float32), rtol=1e-6, atol=1e-3)


def test_syrk_is_deterministic(K):
    rs = np.random.RandomState(11)
    Xt = _dev(_rand(rs, 30000, 260).T)
    a = K.syrk(Xt).clone()
    b = K.syrk(Xt)
    assert torch.equal(a, b)


def test_syrk_large_properties(K):
    """Size-independent properties at a size the oracle cannot afford: trace(G) =
    ||X||_F^2, symmetry, G e_j column vs a direct fp64 dot for a few columns."""
    g = torch.Generator(device="cuda").manual_seed(5)
    n, m = 1300, 200000
    Xt = torch.randn((n, m), generator=g, device="cuda", dtype=torch.float32)
    G = K.syrk(Xt)
    fro = (Xt.double() ** 2).sum()
    assert abs(float(torch.trace(G) / fro) - 1.0) < 1e-7
    assert torch.equal(G, G.T)
    for j in (0, 517, 1299):
        ref = Xt.double() @ Xt[j].double()
        assert float((G[:, j] - ref).abs().max() / ref.abs().max()) < 1e-6


# ---------------------------------------------------------------- K3 GEMM_TN
@pytest.mark.parametrize("K_,na,nb", [(64, 3, 2), (5000, 200, 190), (4099, 130, 131), (1000, 130, 60), (4097, 300, 70), (50000, 192, 220),
                                       (3001, 257, 33), (20000, 140, 150), (777, 64, 64), (5000, 1000, 129),
                                       (200000, 300, 90), (99999, 128, 96), (65536, 3653, 70),   # 96-row tiles (round 2); 70 -> one 80-row tile (round 3)
                                       # round 3, tile heights with a 16-row block on the 16x16x4 MFMA: 48 / 80 / 112 rows, alone, stacked,
                                       # below full 128-row tiles (200 = 128 + 80, 220 = 128 + 96), unaligned ld (K odd), K % 32 != 0
                                       (5000, 200, 40), (4099, 130, 48), (30000, 257, 72), (30001, 257, 80), (3000, 150, 100),
                                       (3002, 150, 112), (30000, 192, 200), (8191, 129, 160), (100, 128, 70)])
def test_gemm_tn(K, K_, na, nb):
    rs = np.random.RandomState(K_ + na + nb)
    A = _rand(rs, K_, na)
    B = _rand(rs, K_, nb)
    Ct = K.gemm_tn(_dev(A.T), _dev(B.T)).cpu().numpy()      # (nb, na)
    ref = (A.astype(np.float64).T @ B.astype(np.float64)).T
    absref = (np.abs(A).astype(np.float64).T @ np.abs(B).astype(np.float64)).T
    assert Ct.shape == (nb, na)
    assert np.all(np.abs(Ct - ref) <= 2e-6 * absref + 1e-30)


# ---------------------------------------------------------------- K2 skinny
@pytest.mark.parametrize(
    "m,n,l",
    [(4, 2, 1), (512, 32, 32), (1000, 33, 50), (1003, 64, 64), (4096, 192, 60),
     (5000, 191, 100), (3000, 100, 128), (2048, 77, 200), (130, 500, 7), (8192, 3653, 70),
     # round 3, the 16x16x4 body: 16-column granules (l = 70 runs 80 columns, 72 -> 80, 80 -> 80), one pass up
     # to 224 columns, two column groups above, rows that are no multiple of 256 / 64 / 4, n % 32 != 0
     (8192, 3653, 80), (5000, 100, 72), (3000, 257, 220), (2048, 130, 224), (1030, 64, 256), (2050, 96, 300),
     (7, 5, 3), (1001, 37, 70), (70000, 61, 17), (263, 31, 209),
     # 4-column blocks behind the 16-column ones (33 <= l <= 72, l % 16 in 1 .. 8): 36 = 32 + 4, 40 = 32 + 8,
     # 52 = 48 + 4, 65 -> 68, 33 -> 36; ragged rows and n % 32 != 0
     (1000, 40, 36), (4099, 130, 40), (2051, 301, 52), (70003, 61, 65), (6, 9, 33), (12288, 3653, 56)],
)
def test_skinny(K, m, n, l):
    rs = np.random.RandomState(m + 13 * n + 7 * l)
    X = _rand(rs, m, n)
    W = _rand(rs, n, l)
    Yt = K.skinny(_dev(X.T), _dev(W.T)).cpu().numpy()       # (l, m)
    ref = (X.astype(np.float64) @ W.astype(np.float64)).T
    absref = (np.abs(X).astype(np.float64) @ np.abs(W).astype(np.float64)).T
    assert Yt.shape == (l, m)
    # one fp32 fma chain over n: error <= n * eps32 * sum|x||w| (worst case), ~sqrt(n) typical
    assert np.all(np.abs(Yt - ref) <= (4 + np.sqrt(n)) * EPS32 * absref + 1e-30)


@pytest.mark.parametrize("m,n,l", [(4, 2, 1), (512, 32, 32), (1003, 64, 20), (4096, 192, 60), (5000, 191, 70),
                                   (130000, 96, 96), (777, 33, 64), (2048, 3653, 70),
                                   # round 3: fused up to 224 columns (cfg4's l = 220), odd block counts, ragged rows
                                   (2048, 3653, 72), (4099, 130, 130), (3000, 100, 220), (1000, 64, 224), (777, 33, 200),
                                   (66000, 40, 150), (5, 3, 2)])
def test_skinny_with_fused_gram(K, m, n, l):
    """K2 with the Gram of its output formed from the accumulators in the same launch: Y must be
    bit-identical to the plain K2 launch (where both run the same blocks) and G = Y^T Y (of the stored fp32 Y, fp64 reference)
    within 4e-6 sum|y||y| (fp32 MFMA chains of 128 rows, fp64 across waves and workgroups) --
    including row counts that are not multiples of 512 / 128 / 4 (the clamped rows past the end
    must not be counted), l not a multiple of 32, and accumulation over row blocks."""
    rs = np.random.RandomState(m + 13 * n + 7 * l)
    X = _rand(rs, m, n)
    W = _rand(rs, n, l)
    Xt, Wt = _dev(X.T), _dev(W.T)
    Y0 = K.skinny(Xt, Wt)
    G = torch.zeros((l, l), dtype=torch.float64, device="cuda")
    Y1 = K.skinny(Xt, Wt, gram=G)
    if 32 < l <= 72 and 1 <= l % 16 <= 8:
        # the plain launch runs the last columns on 4-column blocks (another summation order over k):
        # the same product to fp32 rounding, not bit for bit
        absref = (np.abs(X).astype(np.float64) @ np.abs(W).astype(np.float64)).T
        assert np.all(np.abs(Y0.cpu().numpy().astype(np.float64) - Y1.cpu().numpy()) <= 2 * (4 + np.sqrt(n)) * EPS32 * absref + 1e-30)
    else:
        assert torch.equal(Y0, Y1)
    Yd = Y1.double()
    ref = Yd @ Yd.T
    bound = 4e-6 * (Yd.abs() @ Yd.abs().T) + 1e-30
    assert bool(((G - ref).abs() <= bound).all()) and torch.equal(G, G.T)
    K.skinny(Xt, Wt, gram=G)                                    # accumulates
    assert bool(((G - 2 * ref).abs() <= 2 * bound).all())
    G2 = torch.zeros_like(G)
    K.skinny(Xt, Wt, gram=G2)
    assert torch.equal(G2 * 2, G) or bool(((G2 * 2 - G).abs() <= 1e-12 * ref.abs().max()).all())   # deterministic
    from dmd_era5_amd._lib import DmdxError

    with pytest.raises(DmdxError):
        K.skinny(Xt, Wt, gram=torch.zeros((l, l), dtype=torch.float32, device="cuda"))


def test_skinny_on_delay_view_equals_explicit_embedding(K):
    """rows > ld: the zero-copy embedded view must give the same product as the
    materialised embedding of the oracle (reference slice_tools.py:207-211)."""
    rs = np.random.RandomState(3)
    m, n, d, l = 1024, 40, 3, 20
    X = _rand(rs, m, n)
    Xe = orc.delay_embed(X, d)                                # (d*m, n-d+1)
    W = _rand(rs, n - d + 1, l)
    from dmd_era5_amd.svd import embed_view

    Yt = K.skinny(embed_view(_dev(X.T), d), _dev(W.T)).cpu().numpy()
    ref = (Xe.astype(np.float64) @ W.astype(np.float64)).T
    assert np.allclose(Yt, ref, rtol=0, atol=1e-5 * np.abs(ref).max())


# ---------------------------------------------------------------- K5 / K6
@pytest.mark.parametrize("m,n,scale", [(1024, 24, False), (1024, 24, True), (1001, 50, True), (5, 9, False)])
def test_row_center_scale_matches_oracle(K, m, n, scale):
    rs = np.random.RandomState(m + n)
    data = (rs.rand(n, m) * 30 + 250).astype(np.float32)      # (time, space) like an ERA5 field
    ref, mean, std = orc.standardize(data, axis=0, scale=scale)
    Xt = _dev(data)
    gmean, gstd = K.row_center_scale_(Xt, scale)
    # reference semantics: fp32 mean; ours accumulates in fp64 -> within fp32 rounding of the mean
    assert np.allclose(gmean.cpu().numpy(), mean, rtol=1e-6, atol=0)
    tol = 1e-4 if not scale else 1e-4
    assert np.allclose(Xt.cpu().numpy(), ref, rtol=0, atol=tol * (1 if scale else 30))
    if scale:
        assert np.allclose(gstd.cpu().numpy(), std, rtol=1e-5)
        assert np.allclose(Xt.cpu().numpy().std(axis=0), 1, atol=1e-4)
    assert np.allclose(Xt.cpu().numpy().mean(axis=0), 0, atol=1e-4)


@pytest.mark.parametrize("d", [1, 2, 3, 5])
def test_delay_shift_sum_equals_gram_of_embedding(K, d):
    rs = np.random.RandomState(d)
    m, n = 300, 37
    X = rs.standard_normal((m, n))
    G = X.T @ X
    Xe = orc.delay_embed(X, d)
    ref = Xe.T @ Xe
    Gd = K.delay_shift_sum(_dev(G), d).cpu().numpy()
    assert np.allclose(Gd, ref, rtol=1e-12, atol=1e-10)


# ---------------------------------------------------------------- full SVD vs golden
def _check_against(U, s, V, Uref, sref, Vref, s_tol, cos_min):
    assert np.all(np.abs(s - sref) <= s_tol), (np.abs(s - sref) / s_tol).max()
    assert col_cosines(U, Uref).min() >= cos_min
    assert col_cosines(V.T, Vref.T).min() >= cos_min


@pytest.mark.parametrize("refine", [True, False])
def test_standard_svd_matches_numpy_golden(refine):
    from dmd_era5_amd.engine import svd_numpy

    g = load_golden(GOLDEN, "lowrank_4096x192")
    X = orc.lowrank_matrix(4096, 192, 100, 0)
    U, s, V = svd_numpy(X, "standard", 50, refine=refine)
    assert U.shape == (4096, 50) and s.shape == (50,) and V.shape == (50, 192)
    assert U.dtype == np.float32
    # stated tolerance of the Gram route: |ds_i| <= 64 eps32 s_1^2 / s_i
    _check_against(U, s, V, g["U64"], g["s64"], g["V64"], sv_tolerance(g["s64"]), 1 - 1e-4)
    # and it is as close to the fp64 truth as the reference's own fp32 LAPACK answer, x10
    err_ref = np.abs(g["s32"] - g["s64"]).max()
    assert np.abs(s - g["s64"]).max() <= 10 * max(err_ref, EPS32 * g["s64"][0])
    assert np.abs(U.T.astype(np.float64) @ U - np.eye(50)).max() < (2e-5 if refine else 2e-3)


def test_standard_svd_cfg1_mock_slice():
    """BASELINE config 1: seeded mock slice, d=2, rank 4 (fp64 in -> fp32 engine)."""
    from dmd_era5_amd.engine import svd_numpy

    g = np.load(os.path.join(GOLDEN, "mock_cfg1.npz"))
    variables, _, _ = orc.mock_era5(25, ["temperature"], [1000], int(g["seed"]))
    X, _, _ = orc.preprocess(variables, True, False, 2)
    U, s, V = svd_numpy(X, "standard", 4)
    assert U.dtype == np.float64 and U.shape == (5184, 4) and V.shape == (4, 24)
    assert np.allclose(s, g["s"], rtol=5e-6)
    # white-noise mock data: singular values are nearly degenerate, so compare the
    # reconstruction instead of individual vectors
    rec = (U * s) @ V
    rec_ref = (g["U"] * g["s"]) @ g["V"]
    assert np.linalg.norm(rec - rec_ref) <= 1e-3 * np.linalg.norm(rec_ref)


def test_randomized_svd_matches_sklearn_golden():
    from dmd_era5_amd.engine import svd_numpy

    g = load_golden(GOLDEN, "lowrank_4096x192")
    X = orc.lowrank_matrix(4096, 192, 100, 0)
    U, s, V = svd_numpy(X, "randomized", 50, random_state=0)     # reference defaults
    # same Omega, same subspaces; normaliser differs (CholeskyQR vs LU) -> rounding-level
    assert np.allclose(s, g["rdef_s"], rtol=2e-5)
    assert col_cosines(U, g["rdef_U"]).min() > 1 - 1e-4
    assert np.all(np.sum(U * g["rdef_U"], axis=0) > 0), "u-based sign convention must match"
    # BASELINE config 4 setting: sklearn's un-normalised fp32 power iterations are far
    # from the truth there (see make_golden.py); we must be at least as close to fp64.
    U, s, V = svd_numpy(X, "randomized", 50, random_state=0, n_oversamples=20, n_iter=2)
    err_ours = np.abs(s - g["s64"]) / g["s64"]
    err_skl = np.abs(g["rcfg4_s"] - g["s64"]) / g["s64"]
    assert err_ours.max() <= max(err_skl.max(), 1e-4)


def test_wide_matrix_both_types():
    from dmd_era5_amd.engine import svd_numpy

    g = np.load(os.path.join(GOLDEN, "lowrank_wide_160x1024.npz"))
    X = orc.lowrank_matrix(160, 1024, 60, 0)
    U, s, V = svd_numpy(X, "standard", 20)
    assert U.shape == (160, 20) and V.shape == (20, 1024)
    assert np.all(np.abs(s - g["s64"]) <= sv_tolerance(g["s64"]))
    assert col_cosines(U, g["U64"]).min() > 1 - 1e-4
    U, s, V = svd_numpy(X, "randomized", 20, random_state=0)
    assert np.allclose(s, g["rdef_s"], rtol=1e-4)


def test_delay_embedded_svd_equals_svd_of_materialised_embedding():
    from dmd_era5_amd.engine import to_device_matrix
    from dmd_era5_amd.svd import svd_snapshots

    X = orc.lowrank_matrix(2048, 96, 40, 1)
    Xe = orc.delay_embed(X, 2)
    Ue, se, Ve = orc.svd_standard(Xe.astype(np.float64), 10)
    r = svd_snapshots(to_device_matrix(X), 10, delay=2)
    assert np.all(np.abs(r.s.cpu().numpy() - se) <= sv_tolerance(se))
    assert col_cosines(r.Ut.cpu().numpy().T, Ue).min() > 1 - 1e-4


def test_unsupported_type_raises_like_reference():
    from dmd_era5_amd.engine import svd_numpy

    with pytest.raises(ValueError, match="SVD type bogus is not supported."):
        svd_numpy(np.zeros((8, 4), dtype=np.float32), "bogus", 2)


# ---------------------------------------------------------------- row blocks / accumulate
def test_syrk_accumulates_over_row_blocks(K):
    rs = np.random.RandomState(21)
    X = _rand(rs, 3000, 150)
    G = K.syrk(_dev(X[:1000].T))
    K.syrk(_dev(X[1000:2200].T), out=G)
    K.syrk(_dev(X[2200:].T), out=G)
    ref = X.astype(np.float64).T @ X.astype(np.float64)
    assert np.allclose(G.cpu().numpy(), ref, rtol=0, atol=2e-6 * np.abs(ref).max())
    assert torch.equal(G, G.T)


def test_blocked_svd_equals_unblocked(monkeypatch):
    """The row-blocked HBM layout (svd.BLOCK_ROWS) must not change the result beyond
    rounding (the fp32 chains are cut at different rows), for both svd types and with
    delay embedding (which also checks the embedded row order of the assembled U)."""
    from dmd_era5_amd import svd as dsvd
    from dmd_era5_amd.engine import to_device_matrix

    X = orc.lowrank_matrix(4096, 96, 40, 2)
    Xt = to_device_matrix(X)
    base = dsvd.svd_snapshots(Xt, 12, delay=2)
    brand = dsvd.svd_randomized(Xt, 12, delay=2, random_state=0)
    monkeypatch.setattr(dsvd, "BLOCK_ROWS", 500)
    blk = dsvd.svd_snapshots(Xt, 12, delay=2)
    assert blk.info["row_blocks"] > 1
    assert torch.allclose(blk.s, base.s, rtol=1e-6)
    assert torch.allclose(blk.Ut, base.Ut, atol=1e-5)
    rr = dsvd.svd_randomized(Xt, 12, delay=2, random_state=0)
    assert torch.allclose(rr.s, brand.s, rtol=1e-5)
    assert torch.allclose(rr.Ut, brand.Ut, atol=1e-4)


# ---------------------------------------------------------------- BASELINE cfg2 at full size
def test_cfg2_full_size_svd_properties(K):
    """cfg2 (1 038 240 x 8760 fp32, rank 50) is far beyond what the oracle can factor, so the
    full-size run is checked through properties that do not depend on the size:
      * the planted spectrum: X = A diag(sigma) B^T + noise with Gaussian A, B has singular values
        ~ sigma_i sqrt(m n) (tolerance 5 %: B^T B / n = I + O(n^-1/2) for the Gaussian factor),
      * s non-increasing, V V^T = I (fp64, 1e-10), U^T U = I (fp64 torch products, 2e-5),
      * the defining relation X^T u_j = s_j v_j, evaluated in fp64 by torch on one row block
        at a time (1e-6 s_1 -- fp32 storage of X and U -- and 1e-4 s_j),
      * Gram invariants of one full-size row block: symmetry (exact), trace(G) = ||X||_F^2 (1e-6).
    """
    import bench
    from dmd_era5_amd import svd as dsvd

    free, _ = torch.cuda.mem_get_info()
    if free < 60 * 2**30:
        pytest.skip("needs ~45 GB of HBM")
    m, n, r, _ = bench.WORKLOADS["cfg2"]
    blocks = bench.make_snapshot_blocks(m, n, 1234, torch.device("cuda"))
    for B in blocks:
        K.row_center_scale_(B, False)
    res = dsvd.svd_snapshots(blocks, r, kern=K)
    s, Vh, Ut = res.s, res.Vh, res.Ut
    assert Ut.shape == (r, m) and Vh.shape == (r, n) and s.shape == (r,)
    assert bool((s[:-1] >= s[1:]).all())
    sig = 100.0 * 0.9 ** np.arange(r)
    planted = sig * np.sqrt(float(m) * n)
    assert np.all(np.abs(s.cpu().numpy() / planted - 1.0) < 0.05)
    eye = torch.eye(r, dtype=torch.float64, device="cuda")
    assert float((Vh @ Vh.T - eye).abs().max()) < 1e-10
    UtU = torch.zeros((r, r), dtype=torch.float64, device="cuda")
    XtU = torch.zeros((n, r), dtype=torch.float64, device="cuda")
    r0 = 0
    for B in blocks:                                   # B: (n, mb) = block of X^T
        Ub = Ut[:, r0:r0 + B.shape[1]].double()        # (r, mb)
        UtU += Ub @ Ub.T
        for j0 in range(0, n, 2190):                   # fp64 copies of the block in column slabs
            XtU[j0:j0 + 2190] += B[j0:j0 + 2190].double() @ Ub.T
        r0 += B.shape[1]
    assert float((UtU - eye).abs().max()) < 2e-5
    err = (XtU - (Vh.T * s)).norm(dim=0)
    assert float((err / s[0]).max()) < 1e-6        # fp32 data: errors scale with eps32 * s_1
    assert float((err / s).max()) < 1e-4           # ... so s_50 = 0.006 s_1 keeps 4 digits
    G = K.syrk(blocks[0])
    assert torch.equal(G, G.T)
    fro = sum(float((blocks[0][j0:j0 + 1024].double() ** 2).sum()) for j0 in range(0, n, 1024))
    assert abs(float(torch.trace(G)) / fro - 1.0) < 1e-6

    # the randomized path (sklearn defaults: l = 60, 7 power iterations) on the same resident
    # matrix: behind 15 applications of X the 60-column sketch has converged on the leading 50
    # directions ((sigma_61 / sigma_50)^15 ~ 3e-8), so it must reproduce the decomposition above
    rr = dsvd.svd_randomized(blocks, r, random_state=0, kern=K)
    assert rr.Ut.shape == (r, m) and rr.Vh.shape == (r, n) and rr.info["n_iter"] == 7
    assert float(((rr.s - s).abs() / s).max()) < 1e-5
    assert float((rr.Vh @ rr.Vh.T - eye).abs().max()) < 1e-10
    assert float(((rr.Vh * Vh).sum(dim=1).abs() - 1.0).abs().max()) < 1e-6      # same right vectors, one by one
    UrU = torch.zeros((r, r), dtype=torch.float64, device="cuda")
    r0 = 0
    for B in blocks:
        UrU += rr.Ut[:, r0:r0 + B.shape[1]].double() @ Ut[:, r0:r0 + B.shape[1]].double().T
        r0 += B.shape[1]
    assert float((UrU.diagonal() - 1.0).abs().max()) < 1e-5                       # same left vectors and signs


def test_cfg3_shard_full_size_svd_properties(K):
    """BASELINE config 3, one GPU's share: 1 946 700 x 8760 fp32 (68 GB, 15 row blocks), rank 200.
    The 200 wanted pairs reach into the noise bulk of the rank-64 + noise matrix (s_k / s_1 = 5e-7):
    block-Krylov eigensolver, polish step, two column groups in K2, 128-row tiles in K3.  Checked
    through size-independent properties: planted leading spectrum, s non-increasing, V V^T = I,
    U^T U = I, X^T u_j = s_j v_j (fp64 torch products, one row block at a time)."""
    import bench
    from dmd_era5_amd import svd as dsvd

    free, _ = torch.cuda.mem_get_info()
    if free < 110 * 2**30:
        pytest.skip("needs ~100 GB of HBM")
    m, n, r = 15 * 721 * 1440 // 8, 8760, 200
    blocks = bench.make_snapshot_blocks(m, n, 4321, torch.device("cuda"))
    for B in blocks:
        K.row_center_scale_(B, False)
    res = dsvd.svd_snapshots(blocks, r, kern=K)
    s, Vh, Ut = res.s, res.Vh, res.Ut
    assert Ut.shape == (r, m) and Vh.shape == (r, n) and s.shape == (r,)
    assert bool((s[:-1] >= s[1:]).all()) and res.info.get("polished")
    planted = 100.0 * 0.9 ** np.arange(60) * np.sqrt(float(m) * n)
    assert np.all(np.abs(s[:60].cpu().numpy() / planted - 1.0) < 0.05)
    # behind the 64 planted terms: the noise bulk, singular values ~ 0.01 (sqrt(m) + sqrt(n))
    bulk = 0.01 * (np.sqrt(m) + np.sqrt(n))
    assert 0.8 * bulk < float(s[-1]) < float(s[70]) < 1.1 * bulk
    eye = torch.eye(r, dtype=torch.float64, device="cuda")
    assert float((Vh @ Vh.T - eye).abs().max()) < 1e-10
    UtU = torch.zeros((r, r), dtype=torch.float64, device="cuda")
    XtU = torch.zeros((n, r), dtype=torch.float64, device="cuda")
    r0 = 0
    for B in blocks:
        Ub = Ut[:, r0:r0 + B.shape[1]].double()
        UtU += Ub @ Ub.T
        for j0 in range(0, n, 2190):
            XtU[j0:j0 + 2190] += B[j0:j0 + 2190].double() @ Ub.T
        r0 += B.shape[1]
    assert float((UtU - eye).abs().max()) < 2e-5
    err = (XtU - (Vh.T * s)).norm(dim=0)
    assert float((err / s[0]).max()) < 1e-6


@pytest.mark.parametrize("k", [50, 200])
def test_cfg4_shape_randomized_properties(K, k):
    """BASELINE config 4's shape at 1/8 of its rows: 1 946 700 x 3653 fp32 (28 GB; n % 4 != 0, so
    the small operand of K2 is re-pitched), randomized SVD with oversample 20 and 2 power
    iterations, k = 50 (l = 70: 96-row K3 tiles, 96-column Grams) and k = 200 (l = 220: two K2
    column groups, 128-row tiles).  Properties: U^T U = I, V V^T = I, s non-increasing, and the
    planted part of the spectrum equal to the method-of-snapshots result on the same matrix."""
    import bench
    from dmd_era5_amd import svd as dsvd

    free, _ = torch.cuda.mem_get_info()
    if free < 60 * 2**30:
        pytest.skip("needs ~45 GB of HBM")
    m, n = 15 * 721 * 1440 // 8, 3653
    blocks = bench.make_snapshot_blocks(m, n, 99, torch.device("cuda"))
    for B in blocks:
        K.row_center_scale_(B, False)
    rr = dsvd.svd_randomized(blocks, k, n_oversamples=20, n_iter=2, random_state=0, kern=K)
    st = dsvd.svd_snapshots(blocks, 60, kern=K)
    assert rr.Ut.shape == (k, m) and rr.Vh.shape == (k, n) and rr.info["l"] == k + 20
    assert bool((rr.s[:-1] >= rr.s[1:]).all())
    lead = min(k, 60)
    # (sigma_{l+1} / sigma_j)^5 with sigma_{l+1} at the noise level: the leading values are exact to fp32
    assert float(((rr.s[:lead] - st.s[:lead]).abs() / st.s[:lead]).max()) < (1e-5 if k == 200 else 2e-3)
    assert float(((rr.s[:40] - st.s[:40]).abs() / st.s[:40]).max()) < 1e-5
    eye = torch.eye(k, dtype=torch.float64, device="cuda")
    assert float((rr.Vh @ rr.Vh.T - eye).abs().max()) < 1e-10
    UtU = torch.zeros((k, k), dtype=torch.float64, device="cuda")
    r0 = 0
    for B in blocks:
        Ub = rr.Ut[:, r0:r0 + B.shape[1]].double()
        UtU += Ub @ Ub.T
        r0 += B.shape[1]
    assert float((UtU - eye).abs().max()) < 2e-5


def _full_size_checks(blocks, res, r, n, tol_u=2e-5, rel_sj=1e-4):
    """Size-independent properties of a rank-r SVD of a resident row-blocked matrix, evaluated
    with fp64 torch products one row block at a time: s non-increasing, V V^T = I (1e-10),
    U^T U = I, X^T u_j = s_j v_j (1e-6 s_1: fp32 storage of X and U; rel_sj s_j)."""
    s, Vh, Ut = res.s, res.Vh, res.Ut
    assert bool((s[:-1] >= s[1:]).all())
    eye = torch.eye(r, dtype=torch.float64, device="cuda")
    assert float((Vh @ Vh.T - eye).abs().max()) < 1e-10
    UtU = torch.zeros((r, r), dtype=torch.float64, device="cuda")
    XtU = torch.zeros((n, r), dtype=torch.float64, device="cuda")
    r0 = 0
    for B in blocks:
        Ub = Ut[:, r0:r0 + B.shape[1]].double()
        UtU += Ub @ Ub.T
        step = max(1, min(n, (1 << 27) // max(1, B.shape[1])))      # <= 1 GiB of fp64 copy at a time
        for j0 in range(0, n, step):
            XtU[j0:j0 + step] += B[j0:j0 + step].double() @ Ub.T
        r0 += B.shape[1]
    assert float((UtU - eye).abs().max()) < tol_u
    err = (XtU - (Vh.T * s)).norm(dim=0)
    assert float((err / s[0]).max()) < 1e-6
    if rel_sj is not None:
        assert float((err / s).max()) < rel_sj
    return err


def test_cfg2_full_size_gap_free_spectrum(K):
    """cfg2's size with the spectrum ERA5 anomalies actually have: sigma_i ~ 1/i over all 8760
    columns, no gap anywhere (bench.make_powerlaw_blocks).  The power steps of the eigen stage
    cannot finish here; the Chebyshev-filtered iteration must, without the 0.8 s library syevd.
    Same size-independent checks as the planted-rank test, plus the spectrum itself:
    s_i = sigma_i sqrt(m) within the Marchenko-Pastur edge factors 1 +- sqrt(n/m) (9 %)."""
    import bench
    from dmd_era5_amd import svd as dsvd

    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < 60 * 2**30:
        pytest.skip("needs ~45 GB of HBM")
    m, n, r, _ = bench.WORKLOADS["cfg2"]
    blocks = bench.make_powerlaw_blocks(m, n, 1234, torch.device("cuda"))
    for B in blocks:
        K.row_center_scale_(B, False)
    res = dsvd.svd_snapshots(blocks, r, kern=K, timings=True)
    assert res.Ut.shape == (r, m) and res.Vh.shape == (r, n) and res.s.shape == (r,)
    assert res.info["eig_method"] in ("cheb", "power"), res.info     # never the full solver at n = 8760
    assert res.info["eig_products"] <= 24
    expect = 100.0 / np.arange(1, r + 1) * np.sqrt(float(m))
    ratio = res.s.cpu().numpy() / expect
    assert np.all(np.abs(ratio - 1.0) < 0.12), ratio
    _full_size_checks(blocks, res, r, n)
    # the eigen stage stays a small share of the step (the Gram is ~0.57 s)
    res = dsvd.svd_snapshots(blocks, r, kern=K, timings=True)
    assert res.info["t_eig"] < 0.08 * res.info["t_total"], res.info


def test_cfg4_full_size_randomized(K):
    """BASELINE config 4 at its stated size: 15 573 600 x 3653 fp32 = 227.6 GB resident on one
    MI355X (119 row blocks; n % 4 != 0), randomized SVD with oversample 20 and 2 power
    iterations, k = 50 (l = 70) and k = 200 (l = 220).  Properties: U^T U = I, V V^T = I,
    s non-increasing, X^T u_j = s_j v_j, and the planted part of the spectrum (64 terms
    100 * 0.9^i * sqrt(m n), 5 %: the Gaussian factors are orthogonal to O(n^-1/2)) -- the
    leading 40 also against the method of snapshots on the same resident matrix."""
    import bench
    from dmd_era5_amd import svd as dsvd

    K.release_workspace()
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < 253 * 2**30:
        pytest.skip(f"needs ~270 GB (252 GiB) of free HBM, {free / 2**30:.0f} GiB available")
    m, n = 15 * 721 * 1440, 3653
    blocks = bench.make_snapshot_blocks(m, n, 99, torch.device("cuda"))
    for B in blocks:
        K.row_center_scale_(B, False)
    planted = 100.0 * 0.9 ** np.arange(64) * np.sqrt(float(m) * n)
    st = dsvd.svd_snapshots(blocks, 40, kern=K)
    s_ref = st.s.clone()
    del st
    for k in (50, 200):
        rr = dsvd.svd_randomized(blocks, k, n_oversamples=20, n_iter=2, random_state=0, kern=K)
        assert rr.Ut.shape == (k, m) and rr.Vh.shape == (k, n) and rr.info["l"] == k + 20
        assert rr.info["passes_over_X"] == 6 and rr.info["row_blocks"] == len(blocks)
        lead = min(k, 60)
        assert np.all(np.abs(rr.s[:lead].cpu().numpy() / planted[:lead] - 1.0) < 0.05)
        assert float(((rr.s[:40] - s_ref).abs() / s_ref).max()) < 1e-5
        # beyond the planted rank (k = 200) the wanted values sit in the noise bulk, where two
        # power iterations resolve s but not individual vectors: the relation is asserted
        # against s_1 only there
        _full_size_checks(blocks, rr, k, n, rel_sj=1e-3 if k == 50 else None)
        del rr
        torch.cuda.empty_cache()
    del blocks
    K.release_workspace()
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- K7L one-sided Jacobi SVD
@pytest.mark.parametrize("n", [2, 9, 97, 128, 250, 312, 513, 936, 1024])
def test_eigh_large_matches_lapack(K, n):
    """The multi-workgroup one-sided Jacobi kernel behind `_eigh_desc` for 96 < n <= 1024, on the
    same graded matrices as K7's test (eigenvalues over 12 decades): eigenvalues to 1e-13 of the
    largest, V orthonormal to 1e-13, A V = V diag(w) to 1e-13 |A| -- times n / 128 beyond n = 128."""
    from dmd_era5_amd import svd as dsvd

    rs = np.random.RandomState(n)
    Qm, _ = np.linalg.qr(rs.standard_normal((n, n)))
    lam = 10.0 ** np.linspace(6, -6, n)
    A = (Qm * lam) @ Qm.T
    A = 0.5 * (A + A.T)
    L = np.linalg.cholesky(A)
    sig, Zt = K.svd_jacobi(_dev(L.T))
    assert 1 <= K.last_jacobi_sweeps <= 20
    w, V = (sig * sig).cpu().numpy(), Zt.cpu().numpy().T
    ref = np.linalg.eigvalsh(A)[::-1]
    # K7's bounds (1e-13) up to n = 128, growing like n beyond: the Cholesky factor handed in,
    # LAPACK's reference values and the sums over n terms all carry ~n eps (n = 936: 7e-13)
    bound = 1e-13 * max(1.0, n / 128.0)
    assert np.all(np.diff(w) <= 0)
    assert np.abs(w - ref).max() <= bound * ref[0]
    assert np.abs(V.T @ V - np.eye(n)).max() <= bound
    assert np.abs(A @ V - V * w).max() <= bound * ref[0]
    if n > 96:
        w2, V2 = dsvd._eigh_desc(_dev(A), K)            # the route the Rayleigh-Ritz steps take
        assert np.abs(w2.cpu().numpy() - ref).max() <= bound * ref[0]
        assert np.abs(A @ V2.cpu().numpy() - V2.cpu().numpy() * w2.cpu().numpy()).max() <= bound * ref[0]


@pytest.mark.parametrize("l,n,decades", [(20, 8760, 4), (60, 8760, 7), (220, 3653, 6), (2, 50, 1)])
def test_svd_wide_factor_of_the_randomized_path(K, l, n, decades):
    """svd._svd_wide (CholeskyQR2 on K9 + K7L's one-sided Jacobi instead of the library's gesvd)
    on the l x n factor B = Q^T X at the sizes of cfg2 (k = 10, 50) and cfg4 (k = 200): singular
    values against the planted ones (1e-14 s_1 + 1e-12 s_j), B reproduced, orthonormal factors."""
    from dmd_era5_amd import svd as dsvd

    rs = np.random.RandomState(l * 7 + n)
    U0, _ = np.linalg.qr(rs.standard_normal((l, l)))
    V0, _ = np.linalg.qr(rs.standard_normal((n, l)))
    s0 = np.logspace(0, -decades, l) * 3e6
    B = (U0 * s0) @ V0.T
    K.last_jacobi_sweeps = None
    Uh, s, Vh = dsvd._svd_wide(_dev(B), K)
    assert K.last_jacobi_sweeps is not None                  # the Jacobi kernel ran, not gesvd
    Uh, s, Vh = Uh.cpu().numpy(), s.cpu().numpy(), Vh.cpu().numpy()
    # the planted values: B itself carries eps * s_1 of rounding, LAPACK on the host no less
    assert np.all(np.abs(s - s0) <= 1e-14 * s0[0] + 1e-12 * s0)
    assert np.linalg.norm((Uh * s) @ Vh - B) <= 1e-13 * np.linalg.norm(B)
    assert np.abs(Uh.T @ Uh - np.eye(l)).max() < 1e-12
    assert np.abs(Vh @ Vh.T - np.eye(l)).max() < 1e-12


def test_svd_jacobi_relative_accuracy_and_zero_columns(K):
    """Singular values over 14 decades come out with RELATIVE accuracy (what the graded refinement
    matrix needs and syevd / gesvd do not promise) -- checked against a 40-digit mpmath SVD --,
    rank-deficient input gives zero singular values with zero vectors, and an indefinite
    Rayleigh-Ritz matrix takes the shifted route."""
    from dmd_era5_amd import svd as dsvd

    mpmath = pytest.importorskip("mpmath")
    rs = np.random.RandomState(3)
    # C = B D, B well conditioned, D graded: the orientation one-sided Jacobi (rotations from the
    # right) resolves with relative accuracy -- and the one the engine hands it (C = S L, L ~ I)
    n0 = 48
    d0 = np.logspace(3, -11, n0)
    C0 = (np.eye(n0) + 0.05 * rs.standard_normal((n0, n0))) * d0[None, :]
    mpmath.mp.dps = 40
    exact = np.array([float(x) for x in mpmath.svd_r(mpmath.matrix(C0.tolist()), compute_uv=False)])
    sig, Zt = K.svd_jacobi(_dev(C0.T))
    assert np.abs(sig.cpu().numpy() / np.sort(exact)[::-1] - 1).max() < 1e-13          # every one of them
    n = 200
    s_true = np.logspace(3, -11, n)
    Cm = (np.eye(n) + 0.05 * rs.standard_normal((n, n))) * s_true[None, :]
    sig, Zt = K.svd_jacobi(_dev(Cm.T))
    sig = sig.cpu().numpy()
    assert np.abs(sig[:100] / np.linalg.svd(Cm, compute_uv=False)[:100] - 1).max() < 1e-9
    Z = Zt.cpu().numpy().T
    assert np.abs(Z.T @ Z - np.eye(n)).max() < 1e-13
    # left singular vectors: Z^T C has orthogonal rows of norm sigma
    R = Z.T @ Cm                                      # (numpy's product resolves the leading rows only)
    assert np.abs(np.linalg.norm(R, axis=1)[:60] / sig[:60] - 1).max() < 1e-11
    # rank deficiency
    Cz = Cm.copy()
    Cz[:, 150:] = 0.0
    sig, Zt = K.svd_jacobi(_dev(Cz.T))
    assert float(sig[150:].abs().max()) == 0.0 and float(Zt[150:].abs().max()) == 0.0
    assert float((Zt[:150] @ Zt[:150].T - torch.eye(150, dtype=torch.float64, device="cuda")).abs().max()) < 1e-13
    # an indefinite matrix through _eigh_desc: shift, factor, shift back
    A = rs.standard_normal((160, 160))
    A = A @ A.T
    A[-1, -1] -= 1e-9 * np.abs(A).max() + np.linalg.eigvalsh(A)[0]      # smallest eigenvalue just below zero
    w, V = dsvd._eigh_desc(_dev(A), K)
    ref = np.linalg.eigvalsh(A)[::-1]
    assert np.abs(w.cpu().numpy() - ref).max() <= 1e-12 * ref[0]


# ---------------------------------------------------------------- K8 fp64 symmetric product
@pytest.mark.parametrize("n,b,shift", [(2, 2, 0.0), (34, 2, 0.5), (256, 32, 0.0), (258, 34, -1.25), (1000, 78, 3.0),
                                        (1500, 124, 0.0), (1024, 130, 7.5), (2050, 312, 1e3), (8760, 78, 2.0)])
def test_symm_skinny_matches_fp64_gemm(K, n, b, shift):
    """Y = G Q - shift Q on the fp64 MFMA path against torch's fp64 GEMM: |dY| <= 1e-13 sum|g||q|
    (fp64 products and sums in a different order), all row / column / K-split edge cases: n not
    a multiple of the 256-row tile or of the 32-row chunk, b not a multiple of 32, b > 128 (two
    column passes), one and several K splits."""
    g = torch.Generator(device="cuda").manual_seed(n * 7 + b)
    A = torch.randn((n, n), generator=g, device="cuda", dtype=torch.float64)
    G = A + A.T
    Q = torch.randn((n, b), generator=g, device="cuda", dtype=torch.float64)
    Y = K.symm_skinny(G, Q, shift)
    ref = G @ Q - shift * Q
    bound = 1e-13 * (G.abs() @ Q.abs() + abs(shift) * Q.abs()) + 1e-300
    assert Y.shape == (n, b) and bool(((Y - ref).abs() <= bound).all())
    # deterministic (per-split partial tiles, no atomics), and `out=` writes in place
    out = torch.empty_like(Y)
    assert K.symm_skinny(G, Q, shift, out=out) is out and torch.equal(out, Y)


def test_symm_skinny_odd_shapes_take_the_library_path(K):
    g = torch.Generator(device="cuda").manual_seed(5)
    A = torch.randn((301, 301), generator=g, device="cuda", dtype=torch.float64)
    G = A + A.T
    Q = torch.randn((301, 77), generator=g, device="cuda", dtype=torch.float64)
    assert torch.allclose(K.symm_skinny(G, Q, 2.0), G @ Q - 2.0 * Q, rtol=1e-12, atol=1e-10)
    from dmd_era5_amd._lib import DmdxError

    with pytest.raises(DmdxError):
        K.symm_skinny(G.float(), Q.float())


@pytest.mark.parametrize("n,b1,b2", [(256, 2, 2), (300, 34, 78), (1000, 124, 124), (8760, 78, 78), (8760, 124, 46),
                                     (5000, 312, 250), (777, 130, 2)])
def test_gemm_tn64_matches_fp64_gemm(K, n, b1, b2):
    """C = A^T B on the fp64 MFMA path (K9) against torch's fp64 GEMM: |dC| <= 1e-13 sum|a||b|;
    widths that are not multiples of 32 / 128, several output tiles, a K tail (n % 128 != 0,
    n % 4 != 0), and the symmetric use (A is B: the Gram of a CholeskyQR round)."""
    g = torch.Generator(device="cuda").manual_seed(n + b1 * 7 + b2)
    A = torch.randn((n, b1), generator=g, device="cuda", dtype=torch.float64)
    B = torch.randn((n, b2), generator=g, device="cuda", dtype=torch.float64)
    Cm = K.gemm_tn64(A, B)
    ref = A.T @ B
    bound = 1e-13 * (A.abs().T @ B.abs()) + 1e-300
    assert Cm.shape == (b1, b2) and bool(((Cm - ref).abs() <= bound).all())
    assert torch.equal(K.gemm_tn64(A, B), Cm)                                   # deterministic
    G = K.gemm_tn64(A, A)
    assert bool(((G - A.T @ A).abs() <= 1e-13 * (A.abs().T @ A.abs())).all())
    # odd widths take the library path
    assert torch.allclose(K.gemm_tn64(A[:, :b1 - 1].contiguous(), B), A[:, :b1 - 1].T @ B, rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize("n", [1, 2, 65, 300, 1031])
def test_pack_unpack_triu_roundtrip(K, n):
    g = torch.Generator(device="cuda").manual_seed(n)
    A = torch.randn((n, n), generator=g, device="cuda", dtype=torch.float64)
    S = A + A.T
    packed = K.pack_triu(S)
    i, j = torch.triu_indices(n, n, device="cuda")
    assert packed.shape == (n * (n + 1) // 2,) and torch.equal(packed, S[i, j])
    assert torch.equal(K.unpack_triu(packed, n), S)
    # only the upper triangle of the input is read
    assert torch.equal(K.unpack_triu(K.pack_triu(torch.triu(S)), n), S)


# ---------------------------------------------------------------- K7 small eigensolver
@pytest.mark.parametrize("n", [1, 2, 3, 17, 62, 77, 96])
def test_eigh_small_matches_lapack(K, n):
    """One-launch Jacobi vs numpy's LAPACK on a graded matrix (eigenvalues over 12 decades):
    eigenvalues to 1e-13 of the largest (the stored A determines the small ones no better),
    V orthonormal to 1e-13, A V = V diag(w) to 1e-13 ||A||."""
    rs = np.random.RandomState(n)
    Qm, _ = np.linalg.qr(rs.standard_normal((n, n)))
    lam = 10.0 ** np.linspace(6, -6, n)
    A = (Qm * lam) @ Qm.T
    A = 0.5 * (A + A.T)
    w, V = K.eigh_small(_dev(A))
    assert (n > 1) <= K.last_eigh_sweeps < 30  # the kernel reports its sweeps; 30 = its limit = not converged (raises)
    w, V = w.cpu().numpy(), V.cpu().numpy()
    ref = np.linalg.eigvalsh(A)[::-1]
    assert np.all(np.diff(w) <= 0)
    assert np.abs(w - ref).max() <= 1e-13 * ref[0]
    assert np.abs(V.T @ V - np.eye(n)).max() <= 1e-13
    assert np.abs(A @ V - V * w).max() <= 1e-13 * ref[0]


def test_eigh_small_indefinite_repeated_and_limits(K):
    A = np.diag([3.0, 3.0, -1.0, 0.0, 3.0])
    A[0, 1] = A[1, 0] = 1e-3
    w, V = K.eigh_small(_dev(A))
    ref = np.linalg.eigvalsh(A)[::-1]
    assert np.abs(w.cpu().numpy() - ref).max() < 1e-14
    assert np.abs(A @ V.cpu().numpy() - V.cpu().numpy() * w.cpu().numpy()).max() < 1e-14
    assert K.eigh_small_max_n == 96
    from dmd_era5_amd._lib import DmdxError

    with pytest.raises(DmdxError):
        K.eigh_small(torch.zeros((97, 97), dtype=torch.float64, device="cuda"))


# ---------------------------------------------------------------- K1 over a list of row blocks
@pytest.mark.parametrize("sizes,n", [([5000, 3000, 4097], 260), ([700] * 19, 70), ([1024, 7], 129), ([4096] * 3 + [4100], 1336), ([3000] * 17, 1290),
                                     ([30001, 29999], 384)])
def test_syrk_blocks_equals_sum_of_block_grams(K, sizes, n):
    """dmdx_syrk_blocks_f32 (one launch per 16 blocks) against the fp64 Gram of the stacked rows,
    same bound as the single-block test; ragged block sizes, > 16 blocks, unaligned blocks,
    and accumulation into an existing G."""
    rs = np.random.RandomState(sum(sizes) + n)
    mats = [_rand(rs, m, n) for m in sizes]
    blocks = [_dev(a.T) for a in mats]
    G = K.syrk_blocks(blocks).cpu().numpy()
    X = np.concatenate(mats).astype(np.float64)
    ref = X.T @ X
    absref = np.abs(X).T @ np.abs(X)
    assert np.all(np.abs(G - ref) <= 2e-6 * absref + 1e-30)
    assert np.array_equal(G, G.T)
    G0 = torch.full((n, n), 3.0, dtype=torch.float64, device="cuda")
    G2 = K.syrk_blocks(blocks, out=G0).cpu().numpy()
    assert G2 is not None and np.allclose(G2 - 3.0, G, rtol=0, atol=1e-9 * np.abs(ref).max())
    seq = K.syrk(blocks[0])
    for B in blocks[1:]:
        K.syrk(B, out=seq)
    # (the per-block and the batched launch cut K into different fp32 chains: same bound, not same bits)
    assert np.all(np.abs(seq.cpu().numpy() - G) <= 4e-6 * absref + 1e-30)


@pytest.mark.parametrize("sizes,na,nb", [([5000, 3000, 4097], 60, 260), ([700] * 19, 70, 200), ([30001, 29999], 130, 129),
                                         ([40000] * 5 + [39996], 200, 80), ([8191, 4093], 129, 65),
                                         ([4096] * 3, 300, 72), ([5000, 3001], 129, 104), ([130872] * 3, 3653, 70), ([999] * 18, 140, 210)])
def test_gemm_tn_blocks_equals_sum_of_block_products(K, sizes, na, nb):
    """dmdx_gemm_tn_blocks_f32 against the fp64 product of the stacked rows: ragged block sizes,
    > 16 blocks, 64-, 96- and 128-row tiles, accumulation into an existing C."""
    rs = np.random.RandomState(sum(sizes) + na + nb)
    As = [_rand(rs, m, na) for m in sizes]
    Bs = [_rand(rs, m, nb) for m in sizes]
    Ct = K.gemm_tn_blocks([_dev(a.T) for a in As], [_dev(b.T) for b in Bs]).cpu().numpy()   # (nb, na)
    A, B = np.concatenate(As).astype(np.float64), np.concatenate(Bs).astype(np.float64)
    ref = (A.T @ B).T
    absref = (np.abs(A).T @ np.abs(B)).T
    assert Ct.shape == (nb, na)
    assert np.all(np.abs(Ct - ref) <= 2e-6 * absref + 1e-30)
    C0 = torch.full((nb, na), -2.0, dtype=torch.float64, device="cuda")
    C2 = K.gemm_tn_blocks([_dev(a.T) for a in As], [_dev(b.T) for b in Bs], out=C0).cpu().numpy()
    assert np.allclose(C2 + 2.0, Ct, rtol=0, atol=1e-9 * np.abs(ref).max())


@pytest.mark.parametrize("sizes,na,nb", [([4096, 4096], 300, 20), ([5000, 3001, 4097], 260, 32), ([640] * 19, 129, 7),
                                         ([30001, 29999], 1000, 1), ([129780, 129780], 8760, 20), ([70000], 515, 10),
                                         # round 3: 16 rows on 16x16x4 + 0 / 1 / 2 groups of 4 rows on 4x4x1 (nb <= 16 / 20 / 24)
                                         ([4096, 4160], 300, 16), ([5000, 3001], 260, 17), ([6400, 6400, 130], 131, 21),
                                         ([8192] * 3, 1000, 24), ([4099, 4100], 64 + 128, 18), ([12800, 6400], 8760, 25)])
def test_gemm_tn_blocks_small_l_path(K, sizes, na, nb):
    """nb <= 32 takes K3s (64-row chunks, waves split the rows of a chunk): against the fp64 product
    of the stacked rows with the bound of the generic path; block lengths that are not multiples
    of 64 (the tails go through the generic kernel), na not a multiple of 128, nb = 1, > 16
    blocks, accumulation into an existing C, determinism, and equality with the generic path
    (DMDX_NO_K3S) to rounding."""
    rs = np.random.RandomState(sum(sizes) + na + nb)
    As = [_rand(rs, m, na) for m in sizes]
    Bs = [_rand(rs, m, nb) for m in sizes]
    Ad, Bd = [_dev(a.T) for a in As], [_dev(b.T) for b in Bs]
    if len(sizes) == 1:
        Ad, Bd = Ad * 2, [Bd[0], torch.zeros_like(Bd[0])]          # (the blocks entry point needs >= 2 blocks)
    Ct = K.gemm_tn_blocks(Ad, Bd).cpu().numpy()               # (nb, na)
    A, B = np.concatenate(As).astype(np.float64), np.concatenate(Bs).astype(np.float64)
    ref = (A.T @ B).T
    absref = (np.abs(A).T @ np.abs(B)).T
    assert Ct.shape == (nb, na)
    assert np.all(np.abs(Ct - ref) <= 2e-6 * absref + 1e-30)
    assert np.array_equal(K.gemm_tn_blocks(Ad, Bd).cpu().numpy(), Ct)
    C0 = torch.full((nb, na), -2.0, dtype=torch.float64, device="cuda")
    C2 = K.gemm_tn_blocks(Ad, Bd, out=C0).cpu().numpy()
    assert np.allclose(C2 + 2.0, Ct, rtol=0, atol=1e-9 * np.abs(ref).max())
    os.environ["DMDX_NO_K3S"] = "1"
    try:
        Cg = K.gemm_tn_blocks(Ad, Bd).cpu().numpy()
    finally:
        del os.environ["DMDX_NO_K3S"]
    assert np.all(np.abs(Cg - Ct) <= 4e-6 * absref + 1e-30)


def test_uncentred_temperature_like_data_matches_numpy_fp64():
    """mean_center = False on temperature-like data (s_1 ~ 3e4 s_2): the plain Gram route loses
    the trailing singular values in the rounding of the fp32 products (76 % error on s_2 measured);
    the engine detects the dominant time mean and deflates it exactly.  Bound: 2e-6
    relative on every singular value against numpy fp64 (numpy's own fp32 LAPACK: 6e-8)."""
    from dmd_era5_amd.engine import svd_numpy

    g = load_golden(GOLDEN, "conditioning_2048x160")
    k = int(g["k"])
    for tag in ("raw", "cen"):
        U, s, V = svd_numpy(g[f"{tag}_X"], "standard", k, device="cuda:0")
        assert np.abs(s / g[f"{tag}_s64"] - 1).max() < 2e-6, tag
        assert col_cosines(U, g[f"{tag}_U64"]).min() > 1 - 1e-5
        assert col_cosines(V.T, g[f"{tag}_V64"].T).min() > 1 - 1e-5


# ---------------------------------------------------------------- differential sweep
def _fuzz_cases():
    rs = np.random.RandomState(2024)
    cases = []
    for i in range(36):
        m = int(rs.choice([3, 17, 64, 257, 1000, 4099, 20000]))
        n = int(rs.choice([2, 5, 24, 96, 130, 300]))
        k = int(rs.randint(1, min(m, n, 40) + 1))
        kind = ["gauss", "lowrank", "deficient", "offset", "graded"][i % 5]
        typ = "standard" if i % 3 else "randomized"
        cases.append((i, m, n, k, kind, typ))
    return cases


@pytest.mark.parametrize("i,m,n,k,kind,typ", _fuzz_cases())
def test_differential_sweep_against_numpy(i, m, n, k, kind, typ):
    """Random shapes / spectra (tall, wide, tiny, rank-deficient, un-centred, graded), both SVD
    types, against numpy fp64: singular values to 2e-5 s_1 (a Gram matrix of fp32 products alone
    resolves ~3e-5 s_1, sqrt of its 1e-9 lambda_1 floor; the graded cases whose s_k is below
    3e-4 s_1 get the extra subspace iteration on X itself and land at ~2e-7 s_1; randomized: where
    sklearn itself is that good -- low-rank inputs), orthonormal factors, and the Eckart-Young property
    ||X - U S V|| <= (1 + 1e-3) x the optimal rank-k error (+ 5e-5 ||X||), which does not care
    about degenerate singular values."""
    from dmd_era5_amd.engine import svd_numpy

    rs = np.random.RandomState(1000 + i)
    if kind == "gauss":
        X = rs.standard_normal((m, n))
    elif kind == "lowrank":
        r = max(1, min(m, n) // 3)
        X = rs.standard_normal((m, r)) @ (rs.standard_normal((r, n)) * (0.8 ** np.arange(r))[:, None])
        X += 1e-3 * rs.standard_normal((m, n))
    elif kind == "deficient":
        r = max(1, min(m, n, k) // 2)
        X = rs.standard_normal((m, r)) @ rs.standard_normal((r, n))
    elif kind == "offset":
        X = 300.0 + rs.standard_normal((m, 1)) * 5 + rs.standard_normal((m, n))
    else:
        X = rs.standard_normal((m, n)) * (0.7 ** np.arange(n))
    X = X.astype(np.float32)
    opts = {"random_state": 0} if typ == "randomized" else {}
    U, s, V = svd_numpy(X, typ, k, device="cuda:0", **opts)
    X64 = X.astype(np.float64)
    sref = np.linalg.svd(X64, compute_uv=False)
    kk = min(k, m, n)
    assert U.shape == (m, kk) and s.shape == (kk,) and V.shape == (kk, n)
    assert np.all(np.diff(s) <= 1e-6 * s[0])
    exact_type = typ == "standard" or kind in ("lowrank", "deficient")
    if exact_type:
        assert np.abs(s - sref[:kk]).max() <= 2e-5 * sref[0], (kind, typ, m, n, k)
    live = s > 1e-6 * s[0]                                        # directions below the fp32 resolution of X carry no constraint
    Ul, Vl = U[:, live].astype(np.float64), V[live].astype(np.float64)
    assert np.abs(Ul.T @ Ul - np.eye(live.sum())).max() < 5e-4
    assert np.abs(Vl @ Vl.T - np.eye(live.sum())).max() < 5e-4
    err = np.linalg.norm(X64 - (U.astype(np.float64) * s) @ V.astype(np.float64))
    opt = np.sqrt((sref[kk:] ** 2).sum())
    if exact_type:
        assert err <= (1 + 1e-3) * opt + 5e-5 * np.linalg.norm(X64), (kind, typ, m, n, k, err, opt)


def test_steep_spectrum_gets_the_polish_step(K):
    """s_k / s_1 = 5e-7 (columns scaled by 0.7^j): below what the Gram matrix of fp32 products
    resolves (~3e-5 s_1).  The engine must notice (lambda_k < 1e-7 lambda_1), run the extra
    subspace iteration on X and reach 1e-6 s_1 (measured 1.8e-7; numpy fp32 LAPACK 3e-8)."""
    from dmd_era5_amd import svd as dsvd

    rs = np.random.RandomState(1029)
    X = (rs.standard_normal((5000, 120)) * (0.7 ** np.arange(120))).astype(np.float32)
    k = 40
    sref = np.linalg.svd(X.astype(np.float64), compute_uv=False)
    r = dsvd.svd_snapshots(_dev(X.T), k, kern=K)
    assert r.info.get("polished") and "warning" not in r.info
    s = r.s.cpu().numpy()
    assert np.abs(s - sref[:k]).max() <= 1e-6 * sref[0]
    assert (np.abs(s - sref[:k]) / sref[:k]).max() <= 1e-3          # even the smallest, 6e-7 s_1
    plain = dsvd.svd_snapshots(_dev(X.T), 10, kern=K)                # s_10 / s_1 = 0.04: no polish
    assert not plain.info.get("polished")


@pytest.mark.parametrize("typ", ["standard", "randomized"])
def test_constant_matrix(typ):
    """A constant matrix (exactly rank 1, identical addends in every fp32 chain: the rounding of
    the Gram accumulates coherently, ~2e-6 of its trace, and makes it indefinite).  Both SVD
    types must return s_1 = c sqrt(m n) and (numerically) zero for the rest, like numpy/sklearn."""
    from dmd_era5_amd.engine import svd_numpy

    m, n, k = 20000, 300, 6
    X = np.full((m, n), 3.5, dtype=np.float32)
    U, s, V = svd_numpy(X, typ, k, device="cuda:0", **({"random_state": 0} if typ == "randomized" else {}))
    assert abs(s[0] / (3.5 * np.sqrt(m * n)) - 1) < 5e-6      # sklearn's fp32 answer is off by 2.4e-6 here
    assert np.all(s[1:] < 1e-4 * s[0])
    assert np.abs(np.abs(U[:, 0]) - 1 / np.sqrt(m)).max() < 1e-6 and np.abs(np.abs(V[0]) - 1 / np.sqrt(n)).max() < 1e-6


# ---------------------------------------------------------------- K10 / K11 (round 3)
@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 62, 64, 65, 124, 250, 500, 513, 1024])
def test_chol_inv_matches_lapack(K, n):
    """K10 against np.linalg.cholesky / scipy.linalg.solve_triangular on a Gram-type matrix whose
    spectrum spans 8 decades (what CholeskyQR factors): L to 1e-13 |L|, L^-1 to cond-scaled rounding
    (|L Linv - I| <= 1e-10), the triangles above the diagonal exactly zero, status 0 and the
    min / max of diag(L); and with a diagonal shift."""
    import scipy.linalg as sla

    rs = np.random.RandomState(n)
    Q, _ = np.linalg.qr(rs.standard_normal((n, n)))
    lam = 10.0 ** np.linspace(0, -8, n)
    A = (Q * lam) @ Q.T
    A = 0.5 * (A + A.T)
    for shift in (0.0, 1e-3):
        L, Linv, info = K.chol_inv(_dev(A), shift=shift)
        ref = np.linalg.cholesky(A + shift * np.eye(n))
        st, dmin, dmax = info.cpu().tolist()
        assert st == 0.0
        Lh, Xh = L.cpu().numpy(), Linv.cpu().numpy()
        assert np.array_equal(np.triu(Lh, 1), np.zeros_like(Lh)) and np.array_equal(np.triu(Xh, 1), np.zeros_like(Xh))
        As = A + shift * np.eye(n)
        assert np.abs(Lh @ Lh.T - As).max() <= 4e-15 * max(n, 16) * np.abs(As).max()        # backward error
        assert np.abs(Lh - ref).max() <= 1e-8 * np.abs(ref).max()                            # forward: cond(A) eps
        assert np.isclose(dmin, np.diag(ref).min(), rtol=1e-9) and np.isclose(dmax, np.diag(ref).max(), rtol=1e-12)
        Xref = sla.solve_triangular(ref, np.eye(n), lower=True)
        assert np.abs(Lh @ Xh - np.eye(n)).max() <= 1e-9
        assert np.abs(Xh - Xref).max() <= 1e-7 * np.abs(Xref).max()
    L2, none, _ = K.chol_inv(_dev(A), want_inv=False)
    assert none is None and torch.equal(L2, K.chol_inv(_dev(A))[0])


def test_chol_inv_flags_an_indefinite_matrix_without_nans(K):
    """An indefinite input: status = index + 1 of the first non-positive pivot (as LAPACK's info),
    every output finite; a NaN input likewise; a strided (non-contiguous) input view."""
    rs = np.random.RandomState(5)
    for n in (40, 200):
        B = rs.standard_normal((n, n))
        A = B @ B.T + n * np.eye(n)
        A[n // 2, n // 2] = -1.0
        L, Linv, info = K.chol_inv(_dev(A))
        st = int(info[0].item())
        try:
            np.linalg.cholesky(A)
            raise AssertionError("the test matrix must be indefinite")
        except np.linalg.LinAlgError:
            pass
        assert st == n // 2 + 1
        assert bool(torch.isfinite(L).all()) and bool(torch.isfinite(Linv).all())
        A[0, 0] = np.nan
        _, _, info = K.chol_inv(_dev(A))
        assert int(info[0].item()) == 1
    big = torch.zeros((64, 80), dtype=torch.float64, device="cuda")
    A = rs.standard_normal((64, 64))
    A = A @ A.T + 64 * np.eye(64)
    big[:, :64] = _dev(A)
    L, _, info = K.chol_inv(big[:, :64])
    assert int(info[0].item()) == 0 and np.allclose(L.cpu().numpy(), np.linalg.cholesky(A), rtol=0, atol=1e-11)


@pytest.mark.parametrize("n,b1,b2", [(1, 2, 1), (17, 2, 3), (300, 34, 78), (8760, 124, 124), (8760, 500, 500), (8759, 250, 63),
                                     (1000, 62, 200), (3653, 220, 220)])
def test_gemm_nt64_matches_fp64_gemm(K, n, b1, b2):
    """K11 (Y = Q Mt^T, fp64 MFMA) against numpy: dense and lower-triangular Mt, ragged n / b2."""
    rs = np.random.RandomState(n + b1 + b2)
    Q = rs.standard_normal((n, b1))
    Mt = rs.standard_normal((b2, b1))
    for M in (Mt, np.tril(Mt) if b1 == b2 else Mt[::-1].copy()):
        Y = K.gemm_nt64(_dev(Q), _dev(M)).cpu().numpy()
        ref = Q @ M.T
        assert Y.shape == (n, b2)
        assert np.abs(Y - ref).max() <= 1e-13 * (np.abs(Q) @ np.abs(M).T).max()
    # odd inner dimension: the library path
    Y = K.gemm_nt64(_dev(Q[:, :b1 - 1] if b1 > 2 else Q), _dev(Mt[:, :b1 - 1] if b1 > 2 else Mt))
    assert Y.shape == (n, b2)


@pytest.mark.parametrize("n_iter,norm", [("auto", "auto"), (2, "auto"), (4, "QR"), (3, "none")])
def test_fp64_randomized_branch_follows_sklearns_normaliser(n_iter, norm):
    """float64 input (the reference's mock slices) takes the fp64 engine path; its randomized branch
    follows sklearn's power_iteration_normalizer choices literally (it hard-coded QR):
    against sklearn.utils.extmath.randomized_svd itself with the same random_state, to fp64 rounding
    amplified by the conditioning of the iterates."""
    from sklearn.utils.extmath import randomized_svd

    from dmd_era5_amd.engine import svd_numpy

    X = orc.lowrank_matrix(3000, 120, 40, seed=11).astype(np.float64)
    k = 6
    Ur, sr, Vr = randomized_svd(X, k, n_iter=n_iter, power_iteration_normalizer=norm, random_state=0)
    U, s, V = svd_numpy(X, "randomized", k, device="cuda", random_state=0, n_iter=n_iter, power_iteration_normalizer=norm)
    assert U.dtype == np.float64 and np.allclose(s, sr, rtol=1e-9)
    assert np.all(np.abs(np.sum(U * Ur, axis=0)) > 1 - 1e-8) and np.all(np.abs(np.sum(V * Vr, axis=1)) > 1 - 1e-8)


@pytest.mark.parametrize("typ", ["standard", "randomized"])
def test_rank_deficient_input_gets_an_orthonormal_completion(typ):
    """An exactly rank-3 matrix asked for 6 components: s_4.. are zero to rounding; LAPACK (the
    reference's np.linalg.svd) returns an arbitrary orthonormal completion of U there.  Round 3: so
    does the engine (zero columns before): U^T U = I over all six columns, the three resolved
    triplets are numpy's."""
    from dmd_era5_amd.engine import svd_numpy

    rs = np.random.RandomState(9)
    m, n, k = 30000, 200, 6
    X = (rs.standard_normal((m, 3)) * np.array([30.0, 10.0, 3.0])) @ rs.standard_normal((3, n))
    X = X.astype(np.float32)
    U, s, V = svd_numpy(X, typ, k, device="cuda:0", **({"random_state": 0} if typ == "randomized" else {}))
    sr = np.linalg.svd(X.astype(np.float64), compute_uv=False)[:k]
    assert np.allclose(s[:3], sr[:3], rtol=2e-5) and np.all(s[3:] < 1e-5 * s[0])
    G = U.astype(np.float64).T @ U.astype(np.float64)
    assert np.abs(G - np.eye(k)).max() < 5e-5
    Ur = np.linalg.svd(X.astype(np.float64), full_matrices=False)[0][:, :3]
    assert np.all(np.abs(np.sum(U[:, :3] * Ur, axis=0)) > 1 - 1e-5)
    assert np.abs(V.astype(np.float64) @ V.astype(np.float64).T - np.eye(k)).max() < 5e-5
