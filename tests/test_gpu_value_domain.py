"""Value-domain tests of the C ABI (include/dmdx.h, "Value contract").

tests/test_gpu_parity.py covers the SHAPES, tests/test_gpu_memory_edges.py the MEMORY; this file
covers the VALUES the kernels are handed:

  A. integer-valued operands built from a small dictionary of rows (tests/exact_inputs.py): the
     closed-form int64 reference costs milliseconds at any m, and under a_A a_B K < 2^24 every fp32
     partial sum of every order is an exact integer, so the assertion is torch.equal -- one dropped,
     repeated or clamped row among millions changes the expected result by a non-zero integer matrix.
     That reaches what only runs at production sizes: the 4096-row chain fold of K1 / K3, units of
     2048 chunks, the split that `by_len` forces, groups of 16 blocks accumulating between launches,
     K2's last ragged rows.  Which unit length a K1 case runs is asserted from the public workspace
     size, not assumed;
  B. one NaN / +Inf / -Inf planted in an operand: the class (finite / NaN / +Inf / -Inf) of every
     output element equals numpy fp64's on the same fp32 inputs, and every output the element does
     not take part in is bit-identical to the clean run -- the host's LinAlgError rests on it
     (svd.py: finiteness of diag(G) and of Z);
  C. data scaled by 2^40 and 2^-40 (the range the host's magnitude guard leaves to the kernels) gives
     the unscaled result times 2^+-80 bit for bit, and un-centred all-positive fields stay inside the
     chain bound the header promises, which does not grow with K.

Every call goes through the ctypes table (explicit accumulate flag, workspace of exactly
`*_workspace_bytes`) or, for the host and fp64 cases, the HipKernels wrappers.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import exact_inputs as ei
from oracle import era5_oracle as orc

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DEV = "cuda"
D = ei.D_DEFAULT
N_CFG2, N_CFG4 = 8760, 3653
SYRK_TILE_BYTES = 128 * 128 * 8          # one partial tile of the Gram (n > 96): 128 x 128 fp64


@pytest.fixture(scope="module")
def L():
    from dmd_era5_amd.kernels import default_kernels

    return default_kernels()._lib          # raises (test fails) if libdmdx.so or the GPU is missing


@pytest.fixture(scope="module")
def KERN():
    from dmd_era5_amd.kernels import default_kernels

    return default_kernels()


@pytest.fixture(autouse=True)
def _release_device_memory():
    """Nothing of this file stays cached on the device (the full-size tests ask for most of the HBM)."""
    yield
    from dmd_era5_amd.kernels import release_cached_workspaces

    release_cached_workspaces()
    torch.cuda.empty_cache()


def _need_free(gib, what):
    """The free-memory convention of the full-size tests of test_gpu_parity.py."""
    from dmd_era5_amd.kernels import release_cached_workspaces

    release_cached_workspaces()
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < gib * 2 ** 30:
        pytest.skip(f"needs ~{what} of HBM, {free / 2 ** 30:.0f} GiB free")


# ------------------------------------------------------------------ ctypes calls on torch tensors
# A column-major matrix (rows x cols, ld) is the tensor of shape (cols, rows) with strides (ld, 1).
def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ws(nbytes):
    assert nbytes > 0
    return torch.empty(int(nbytes), dtype=torch.uint8, device=DEV)


def _ld(t):
    return t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1)


def _p(t):
    return None if t is None else t.data_ptr()


def _i64(xs):
    return (C.c_int64 * len(xs))(*[int(x) for x in xs])


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _outs(nrow, ncol, out, want32):
    """(C64, C32) tensors of the column-major nrow x ncol result (shape (ncol, nrow))."""
    C64 = out if out is not None else torch.full((ncol, nrow), float("nan"), dtype=F64, device=DEV)
    C32 = torch.full((ncol, nrow), float("nan"), dtype=F32, device=DEV) if want32 else None
    return C64, C32


def syrk(L, Xt, out=None, want32=True):
    n, m = Xt.shape
    G64, G32 = _outs(n, n, out, want32)
    ws = _ws(L.dmdx_syrk_workspace_bytes(m, n))
    rc = L.dmdx_syrk_f32(_p(Xt), m, n, _ld(Xt), _p(G64), n, _p(G32), n, int(out is not None), _p(ws), ws.numel(), _stream())
    assert rc == 0, L.dmdx_last_error()
    torch.cuda.synchronize()
    return G64, G32


def syrk_blocks(L, blocks, out=None, want32=True):
    n = blocks[0].shape[0]
    ms = _i64([b.shape[1] for b in blocks])
    G64, G32 = _outs(n, n, out, want32)
    ws = _ws(L.dmdx_syrk_blocks_workspace_bytes(ms, len(blocks), n))
    rc = L.dmdx_syrk_blocks_f32(_ptrs(blocks), ms, _i64([_ld(b) for b in blocks]), len(blocks), n, _p(G64), n, _p(G32), n,
                                int(out is not None), _p(ws), ws.numel(), _stream())
    assert rc == 0, L.dmdx_last_error()
    torch.cuda.synchronize()
    return G64, G32


def gemm_tn(L, At, Bt, out=None, want32=True):
    (na, K), nb = At.shape, Bt.shape[0]
    C64, C32 = _outs(na, nb, out, want32)
    ws = _ws(L.dmdx_gemm_tn_workspace_bytes(K, na, nb))
    rc = L.dmdx_gemm_tn_f32(_p(At), _ld(At), _p(Bt), _ld(Bt), K, na, nb, _p(C64), na, _p(C32), na, int(out is not None),
                            _p(ws), ws.numel(), _stream())
    assert rc == 0, L.dmdx_last_error()
    torch.cuda.synchronize()
    return C64, C32


def gemm_tn_blocks(L, As, Bs, out=None, want32=True):
    na, nb = As[0].shape[0], Bs[0].shape[0]
    ks = _i64([a.shape[1] for a in As])
    C64, C32 = _outs(na, nb, out, want32)
    ws = _ws(L.dmdx_gemm_tn_blocks_workspace_bytes(ks, len(As), na, nb))
    rc = L.dmdx_gemm_tn_blocks_f32(_ptrs(As), _i64([_ld(a) for a in As]), _ptrs(Bs), _i64([_ld(b) for b in Bs]), ks, len(As),
                                   na, nb, _p(C64), na, _p(C32), na, int(out is not None), _p(ws), ws.numel(), _stream())
    assert rc == 0, L.dmdx_last_error()
    torch.cuda.synchronize()
    return C64, C32


def skinny(L, Et, Wt, gram=None, accumulate=0):
    """Y = E W for the (n, m) tensor / delay view Et (strides (ld, 1), m > ld allowed) and W^T (l, n)."""
    n, m = Et.shape
    l = Wt.shape[0]
    Yt = torch.full((l, m), float("nan"), dtype=F32, device=DEV)
    if gram is None:
        rc = L.dmdx_gemm_nn_skinny_f32(_p(Et), m, n, _ld(Et), _p(Wt), _ld(Wt), l, _p(Yt), m, _stream())
    else:
        ws = _ws(L.dmdx_gemm_nn_skinny_gram_workspace_bytes(m, l))
        rc = L.dmdx_gemm_nn_skinny_gram_f32(_p(Et), m, n, _ld(Et), _p(Wt), _ld(Wt), l, _p(Yt), m, _p(gram), l, accumulate,
                                            _p(ws), ws.numel(), _stream())
    assert rc == 0, L.dmdx_last_error()
    torch.cuda.synchronize()
    return Yt


def _pitched(W):
    """W^T (l, n) on the device with a leading dimension that is a multiple of 4 (the production layout)."""
    Wt = torch.from_numpy(np.ascontiguousarray(np.asarray(W, dtype=np.float32).T)).to(DEV)
    l, n = Wt.shape
    buf = torch.zeros((l, (n + 3) // 4 * 4), dtype=F32, device=DEV)
    buf[:, :n] = Wt
    return buf[:, :n]


def _dev64(ref):
    """An int64 / fp64 host matrix (rows x cols) as the device tensor of the column-major result."""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(ref, dtype=np.float64).T)).to(DEV)


def _int_start(shape, seed, symmetric):
    g = torch.Generator(device=DEV).manual_seed(seed)
    G0 = torch.randint(-1000, 1001, shape, device=DEV, generator=g).to(F64)
    return G0 + G0.T if symmetric else G0


def _assert_exact(got64, got32, ref_t, what):
    bad = int((got64 != ref_t).sum())
    assert torch.equal(got64, ref_t), f"{what}: {bad} of {ref_t.numel()} fp64 entries differ from the integer reference"
    if got32 is not None:
        assert torch.equal(got32, ref_t.to(F32)), f"{what}: the fp32 copy is not the rounded fp64 result"


def _exact_product_case(run, ref, symmetric, seed, what):
    """accumulate = 0, then accumulate = 1 onto an integer-valued start; both bit for bit."""
    ref_t = _dev64(ref)
    G64, G32 = run(None)
    _assert_exact(G64, G32, ref_t, what)
    if symmetric:
        assert torch.equal(G64, G64.T)
    del G64, G32
    G0 = _int_start(tuple(ref_t.shape), seed, symmetric)
    want = G0 + ref_t                                   # integers far below 2^53: exact
    G64, G32 = run(G0)
    assert G64.data_ptr() == G0.data_ptr()
    _assert_exact(G64, G32, want, what + ", accumulate = 1")


def _blocks_of(R, sizes, salt=0, Dn=D):
    """Contiguous (n, m_j) device blocks of the operand with rows R[d(i)], i running over all blocks."""
    out, start = [], 0
    for m in sizes:
        out.append(ei.device_operand(R, ei.row_map_torch(m, Dn, salt, start, DEV)))
        start += m
    return out


# =================================================================== A. exact integer results
def _syrk_units(L, K, n):
    """(nsplit, chunks per unit) of dmdx_syrk_f32 from its public workspace size (n > 96)."""
    ntr = (n + 127) // 128
    ntiles = ntr * (ntr + 1) // 2
    nbytes = L.dmdx_syrk_workspace_bytes(K, n)
    assert nbytes % (ntiles * SYRK_TILE_BYTES) == 0
    nsplit = nbytes // (ntiles * SYRK_TILE_BYTES)
    chunks = (K + 31) // 32
    return nsplit, -(-chunks // nsplit)


# (K, chunks per unit the case is there for).  FOLD = 128 chunks: 127 never folds, 128 folds once at
# the very end, 129 folds and goes on for one chunk, 256 / 257 twice, 2048 sixteen times (the longest
# unit there is); 327 681 rows are one chunk more than 5 units of 2048 hold: `by_len` forces a sixth split.
K1_FOLD_CASES = [(20289, 127), (20479, 128), (20481, 129), (40960, 256), (41090, 257), (327680, 2048), (327681, 1707)]


@pytest.mark.parametrize("K,cps", K1_FOLD_CASES)
def test_syrk_exact_across_the_chain_fold(L, K, cps):
    n = N_CFG2
    nsplit, got_cps = _syrk_units(L, K, n)
    print(f"K = {K} (K % 32 = {K % 32}, K % 4 = {K % 4}): {nsplit} splits of {got_cps} chunks")
    assert got_cps == cps, "the plan changed: pick K anew so that this case runs the intended unit length"
    if K == 327681:
        chunks = (K + 31) // 32
        assert nsplit == -(-chunks // 2048) > _syrk_units(L, K - 1, n)[0] and _syrk_units(L, K - 1, n)[1] == 2048
    a = min(ei.max_a_product(K), 9)
    assert ei.product_exact(a, a, K)
    R = ei.dictionary(D, n, a, seed=K)
    d = ei.row_map_torch(K, D, device=DEV)
    Xt = ei.device_operand(R, d)
    ref = ei.gram_ref(R, ei.counts(ei.row_map(K, D)))
    assert int(np.abs(ref).max()) < ei.TWO24
    _exact_product_case(lambda out: syrk(L, Xt, out), ref, True, K, f"syrk K={K}")


def test_syrk_fold_cases_cover_the_row_remainders():
    assert {K % 32 for K, _ in K1_FOLD_CASES} >= {0, 1, 31} and any(K % 4 for K, _ in K1_FOLD_CASES)
    assert all(K * N_CFG2 * 4 < 12e9 for K, _ in K1_FOLD_CASES)


def test_syrk_exact_at_cfg2_single_call_and_blocks(L):
    """1 038 240 x 8760 (36 GB): one call (16 splits of ~2028 chunks), and the 131 072-row blocks of
    svd.BLOCK_ROWS through the blocks entry point (8 blocks: one group)."""
    from dmd_era5_amd import svd as dsvd

    _need_free(60, "45 GB")
    m, n = 1038240, N_CFG2
    a = ei.max_a_product(m)
    assert a == 4 and ei.product_exact(a, a, m)
    R = ei.dictionary(D, n, a, seed=2)
    Xt = ei.device_operand(R, ei.row_map_torch(m, D, device=DEV))
    ref = ei.gram_ref(R, ei.counts(ei.row_map(m, D)))
    nsplit, cps = _syrk_units(L, m, n)
    print(f"cfg2 single call: {nsplit} splits of {cps} chunks")
    assert cps > 128
    _exact_product_case(lambda out: syrk(L, Xt, out), ref, True, 2, "syrk cfg2")
    blocks = [Xt[:, s:e] for s, e in dsvd.split_rows(m, dsvd.BLOCK_ROWS)]
    assert len(blocks) == 8 and sum(b.shape[1] for b in blocks) == m
    _exact_product_case(lambda out: syrk_blocks(L, blocks, out), ref, True, 3, "syrk_blocks cfg2")


def test_syrk_blocks_exact_over_two_groups(L):
    """19 unequal blocks at n = 3653: the second launch (blocks 17 - 19) accumulates onto the first; a
    block of a single chunk, blocks with K % 4 = 1, 2, 3, two of svd.BLOCK_ROWS."""
    n = N_CFG4
    sizes = [131072, 5000, 32, 4099, 3001, 131072, 777, 1030, 64, 2051, 4096, 4160, 333, 20481, 1, 700, 9999, 40961, 17]
    assert len(sizes) > 16 and min(sizes[16:]) >= 17 and 32 in sizes
    Kt = sum(sizes)
    a = ei.max_a_product(Kt)
    assert a >= 2 and ei.product_exact(a, a, Kt)
    R = ei.dictionary(D, n, a, seed=19)
    blocks = _blocks_of(R, sizes)
    ref = ei.gram_ref(R, ei.counts(ei.row_map(Kt, D)))
    _exact_product_case(lambda out: syrk_blocks(L, blocks, out), ref, True, 19, "syrk_blocks 19 blocks")


@pytest.mark.parametrize("n", [40, 64, 96, 129])
def test_syrk_exact_small_n_long_K(L, n):
    """n <= 96: the plain-product route (one 64- / 96-row tile, 255 splits); n = 129: two tile rows."""
    K = 1000003
    a = ei.max_a_product(K)
    assert a == 4 and ei.product_exact(a, a, K)
    R = ei.dictionary(D, n, a, seed=n)
    Xt = ei.device_operand(R, ei.row_map_torch(K, D, device=DEV))
    ref = ei.gram_ref(R, ei.counts(ei.row_map(K, D)))
    _exact_product_case(lambda out: syrk(L, Xt, out), ref, True, n, f"syrk n={n}")


def _tn_operands(sizes, na, nb, aA, aB, seed):
    Kt = sum(sizes)
    assert ei.product_exact(aA, aB, Kt)
    DA, DB = 61, 53
    RA, RB = ei.dictionary(DA, na, aA, seed=seed), ei.dictionary(DB, nb, aB, seed=seed + 1)
    As, Bs = _blocks_of(RA, sizes, 1, DA), _blocks_of(RB, sizes, 2, DB)
    ref = ei.tn_ref(RA, RB, ei.cooccurrence(ei.row_map(Kt, DA, 1), ei.row_map(Kt, DB, 2), DA, DB))
    return As, Bs, ref


@pytest.mark.parametrize("nb", [70, 220])
def test_gemm_tn_blocks_exact_at_cfg4_shapes(L, nb):
    """17 blocks of 131 072 x 3653 against 131 072 x nb (the X^T Y of the range finder at cfg4): a second
    group runs and accumulates.  nb = 70: 80-row tiles; nb = 220: stacked 128 + 96."""
    _need_free(60, "45 GB")
    sizes = [131072] * 17
    As, Bs, ref = _tn_operands(sizes, N_CFG4, nb, 3, 2, nb)
    _exact_product_case(lambda out: gemm_tn_blocks(L, As, Bs, out), ref, False, nb, f"gemm_tn_blocks nb={nb}")


@pytest.mark.parametrize("na,nb", [(300, 200), (1300, 70), (129, 220)])
def test_gemm_tn_exact_single_call_long_K(L, na, nb):
    """K = 2 000 003 in one call.  nb = 200: stacked 128 + 80; 220: 128 + 96; 70: one 80-row tile."""
    K = 2000003
    As, Bs, ref = _tn_operands([K], na, nb, 4, 2, na + nb)
    _exact_product_case(lambda out: gemm_tn(L, As[0], Bs[0], out), ref, False, na, f"gemm_tn {na}x{nb}")


@pytest.mark.parametrize("sizes", [[131072, 4160, 5000, 512], [131072, 300, 4160]], ids=["k3s", "one-block-below-512"])
@pytest.mark.parametrize("nb", [16, 20, 24, 32])
def test_gemm_tn_blocks_exact_small_l(L, nb, sizes):
    """K3s: nb <= 32, every block 16-byte aligned with K % 4 == 0 and K >= 512, no fp32 copy; one block of
    300 rows sends the same call down the generic path.  Both exact."""
    As, Bs, ref = _tn_operands(sizes, N_CFG4, nb, 5, 3, nb)
    assert all(a.data_ptr() % 16 == 0 and _ld(a) % 4 == 0 for a in As + Bs)
    _exact_product_case(lambda out: gemm_tn_blocks(L, As, Bs, out, want32=False), ref, False, nb, f"K3s nb={nb}")


K2_LS = [17, 56, 70, 72, 220, 256, 300]


def _k2_impl_env(old):
    class _ctx:
        def __enter__(self):
            if old:
                os.environ["DMDX_K2_IMPL"] = "old"

        def __exit__(self, *exc):
            if old:
                del os.environ["DMDX_K2_IMPL"]
    return _ctx()


@pytest.mark.parametrize("m", [131072, 1000003])
def test_skinny_exact_every_row(L, m):
    """Y = X W with dense integer W, every one of the m x l elements exact: a clamped, repeated or
    shifted row anywhere shows.  l = 17: the 32x32x2 body; above: the 16x16x4 body (56, 70: with
    4-column tail blocks; 256, 300: two column groups); the 32x32x2 body for l > 32 through DMDX_K2_IMPL=old.
    m = 1 000 003: m % 4 = 3 (scalar-load path, ragged last workgroup); 131 072: the 16-byte path."""
    n = N_CFG4
    a = ei.max_a_skinny(n)
    assert a == 67 and ei.skinny_exact(n, a, a)
    R = ei.dictionary(D, n, a, seed=m)
    d = ei.row_map_torch(m, D, device=DEV)
    Xt = ei.device_operand(R, d)
    for l, old in [(l, False) for l in K2_LS] + [(70, True), (128, True)]:
        W = np.random.RandomState(l).randint(-a, a + 1, size=(n, l))
        YD = ei.skinny_ref(R, W)
        assert int(np.abs(YD).max()) < ei.TWO24
        want = torch.index_select(torch.from_numpy(np.ascontiguousarray(YD.T).astype(np.float32)).to(DEV), 1, d)
        with _k2_impl_env(old):
            Yt = skinny(L, Xt, _pitched(W))
        bad = (Yt != want).any(dim=0).nonzero().flatten()
        assert torch.equal(Yt, want), f"l = {l}{' (old body)' if old else ''}: rows {bad[:8].tolist()} ... ({bad.numel()}) differ"
        del Yt, want


@pytest.mark.parametrize("mm", [100000, 100003])
@pytest.mark.parametrize("l", [20, 70])
def test_skinny_exact_on_the_delay_view(L, mm, l):
    """rows > ld: E[k mm + s, t] = X[s, t + k], d = 3.  mm % 4 = 0 (16-byte path) and 3 (scalar path)."""
    nn, delay = 300, 3
    nd = nn - delay + 1
    a = ei.max_a_skinny(nd)
    assert ei.skinny_exact(nd, a, a)
    R = ei.dictionary(D, nn, a, seed=mm)
    d = ei.row_map_torch(mm, D, device=DEV)
    Xt = ei.device_operand(R, d)                                    # (nn, mm): the snapshots back to back
    Et = Xt.as_strided((nd, delay * mm), (mm, 1))
    W = np.random.RandomState(l).randint(-a, a + 1, size=(nd, l))
    YD = ei.skinny_ref(ei.embed_dictionary(R, delay), W)
    de = torch.cat([k * D + d for k in range(delay)])
    want = torch.index_select(torch.from_numpy(np.ascontiguousarray(YD.T).astype(np.float32)).to(DEV), 1, de)
    Yt = skinny(L, Et, _pitched(W))
    assert torch.equal(Yt, want)


@pytest.mark.parametrize("l", [20, 70, 220])
def test_skinny_fused_gram_exact(L, l):
    """X in {-1, 0, 1}, every column of W with two +-1 entries: |y| <= 2, so max|y|^2 m < 2^24 and the
    Gram is exact whatever rows a workgroup, a wave or a partial tile groups (no weaker, documented
    grouping is leaned on).  m = 1 000 003 is no multiple of 256 / 64 / 4.  accumulate = 0, then two
    accumulating calls."""
    m, n = 1000003, N_CFG4
    assert m % 4 and m % 64 and m % 256
    R = ei.dictionary(D, n, 1, seed=l)
    rs = np.random.RandomState(l)
    W = np.zeros((n, l), dtype=np.int64)
    for c in range(l):
        W[rs.choice(n, 2, replace=False), c] = rs.choice([-1, 1], 2)
    YD = ei.skinny_ref(R, W)
    ymax = int(np.abs(YD).max())
    assert ymax <= 2 and ymax * ymax * m < ei.TWO24 and ei.skinny_exact(n, 1, 1)
    d = ei.row_map_torch(m, D, device=DEV)
    Xt = ei.device_operand(R, d)
    want_y = torch.index_select(torch.from_numpy(np.ascontiguousarray(YD.T).astype(np.float32)).to(DEV), 1, d)
    ref = _dev64(ei.gram_ref(YD, ei.counts(ei.row_map(m, D))))
    Wt = _pitched(W)
    G = torch.full((l, l), float("nan"), dtype=F64, device=DEV)
    Yt = skinny(L, Xt, Wt, gram=G, accumulate=0)
    assert torch.equal(Yt, want_y)
    assert torch.equal(G, ref), f"{int((G != ref).sum())} Gram entries differ"
    for k in (2, 3):
        Yt = skinny(L, Xt, Wt, gram=G, accumulate=1)
        assert torch.equal(Yt, want_y) and torch.equal(G, k * ref)
    G0 = _int_start((l, l), l, True)
    G = G0.clone()
    skinny(L, Xt, Wt, gram=G, accumulate=1)
    assert torch.equal(G, G0 + ref)


def _ulps32(x, y):
    """Distance in units of the last place between two fp32 arrays of equal sign."""
    xi, yi = x.astype(np.float32).view(np.int32).astype(np.int64), y.astype(np.float32).view(np.int32).astype(np.int64)
    return np.abs(xi - yi)


def _k5_rows(m, n, seed):
    """(n, m) fp32 (time, space): integer series whose time mean is an integer."""
    rs = np.random.RandomState(seed)
    V = rs.randint(-40, 41, size=(n, m)).astype(np.int64)
    mu = rs.randint(250, 300, size=m)
    V[-1] -= V.sum(axis=0) - 0                         # now every column sums to 0 ...
    assert np.all(V.sum(axis=0) == 0)
    return (V + mu).astype(np.float32), mu, V          # ... and the mean of V + mu is mu


def _k5_buffer(data, ld, off=0):
    """The (n, m) view with row stride ld (base `off` floats past a 16-byte boundary) holding `data`."""
    n, m = data.shape
    buf = torch.zeros(n * ld + 8, dtype=F32, device=DEV)
    Xt = buf[off:off + n * ld].view(n, ld)[:, :m]
    Xt.copy_(torch.from_numpy(data))
    return Xt


K5_LAYOUTS = [("tiled", 1004, 0), ("scalar-odd-ld", 1003, 0), ("scalar-base", 1004, 1)]


@pytest.mark.parametrize("name,ld,off", K5_LAYOUTS)
@pytest.mark.parametrize("scale", [False, True])
def test_row_center_scale_exact_on_integer_rows(L, scale, name, ld, off):
    """mean exact, centred X exact; with scale std is within 1 ulp of fl32(sqrt(var)) (the kernel rounds
    the fp64 root once more), and X == fl32(c / std_returned) EXACTLY: the library is built without any
    fast-math flag and hipcc's default fp32 division is the correctly rounded one (established on the
    device by this very assertion).  m = 1003: m % 4 = 3 on both the tiled and the scalar kernel."""
    m, n = 1003, 24
    data, mu, V = _k5_rows(m, n, 5)
    Xt = _k5_buffer(data, ld, off)
    assert (Xt.data_ptr() % 16 == 0 and ld % 4 == 0) == (name == "tiled")
    mean = torch.full((m,), float("nan"), dtype=F32, device=DEV)
    std = torch.full((m,), float("nan"), dtype=F32, device=DEV)
    rc = L.dmdx_row_center_scale_f32(_p(Xt), m, n, ld, _p(mean), _p(std) if scale else None, int(scale), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(mean.cpu().numpy(), mu.astype(np.float32))
    got = Xt.cpu().numpy()
    c = V.astype(np.float32)
    if not scale:
        assert np.array_equal(got, c)
        return
    var = (V.astype(np.float64) ** 2).sum(axis=0) / n              # exact integer sums, one division
    sd_ref = np.sqrt(var).astype(np.float32)
    sd = std.cpu().numpy()
    print(f"std: max distance {int(_ulps32(sd, sd_ref).max())} ulp; ", end="")
    assert _ulps32(sd, sd_ref).max() <= 1
    want = c / sd[None, :]                                          # numpy fp32 division: correctly rounded
    print(f"scaled X: {int((got != want).sum())} of {got.size} elements differ from fl32(c / std)")
    assert np.array_equal(got, want)


def test_fp64_small_kernels_exact_on_integers(L, KERN):
    """K6 / K8 / K9 / K11 at n = 8760 on small integers: every sum is far below 2^53, exact in any order."""
    n, b1, b2 = N_CFG2, 20, 12
    rs = np.random.RandomState(8)
    A = rs.randint(-1000, 1001, size=(n, n)).astype(np.float64)
    G = A + A.T
    Gd = torch.from_numpy(G).to(DEV)
    # K6
    d = 3
    nd = n - d + 1
    ref = sum(G[k:k + nd, k:k + nd] for k in range(d))
    out, out32 = KERN.delay_shift_sum(Gd, d, want32=True)
    assert torch.equal(out, torch.from_numpy(ref).to(DEV)) and torch.equal(out32, torch.from_numpy(ref).to(DEV).to(F32))
    # K8, integer shift
    Q = rs.randint(-50, 51, size=(n, b1)).astype(np.float64)
    Qd = torch.from_numpy(Q).to(DEV)
    for shift in (0.0, 3.0, -1000.0):
        Y = torch.full((n, b1), float("nan"), dtype=F64, device=DEV)
        ws = _ws(L.dmdx_symm_skinny_workspace_bytes(n, b1))
        assert L.dmdx_symm_skinny_f64(_p(Gd), n, n, _p(Qd), b1, b1, shift, _p(Y), b1, _p(ws), ws.numel(), _stream()) == 0
        ref = ei._exact_matmul(G, Q).astype(np.float64) - shift * Q
        assert torch.equal(Y, torch.from_numpy(ref).to(DEV)), f"K8 shift = {shift}"
    # K9
    B = rs.randint(-50, 51, size=(n, b2)).astype(np.float64)
    Bd = torch.from_numpy(B).to(DEV)
    Cm = torch.full((b1, b2), float("nan"), dtype=F64, device=DEV)
    ws = _ws(L.dmdx_gemm_tn_f64_workspace_bytes(n, b1, b2))
    assert L.dmdx_gemm_tn_f64(_p(Qd), b1, _p(Bd), b2, n, b1, b2, _p(Cm), b2, _p(ws), ws.numel(), _stream()) == 0
    assert torch.equal(Cm, torch.from_numpy(ei._exact_matmul(Q.T, B).astype(np.float64)).to(DEV))
    # K11
    Mt = rs.randint(-50, 51, size=(b2, b1)).astype(np.float64)
    Md = torch.from_numpy(Mt).to(DEV)
    Y = torch.full((n, b2), float("nan"), dtype=F64, device=DEV)
    assert L.dmdx_gemm_nt_f64(_p(Qd), b1, n, b1, _p(Md), b1, b2, _p(Y), b2, _stream()) == 0
    assert torch.equal(Y, torch.from_numpy(ei._exact_matmul(Q, Mt.T).astype(np.float64)).to(DEV))


# =================================================================== B. NaN / Inf propagation
NAN, PINF, NINF = float("nan"), float("inf"), float("-inf")


def _t(a, ld=None):
    """Host matrix (rows x cols) -> device tensor (cols, rows) with row stride ld (default tight)."""
    a = np.asarray(a, dtype=np.float32)
    rows, cols = a.shape
    ld = ld or rows
    buf = torch.zeros((cols, ld), dtype=F32, device=DEV)
    buf[:, :rows] = torch.from_numpy(np.ascontiguousarray(a.T))
    return buf[:, :rows]


def _ld_for(path, rows):
    """LDS-DMA / 16-byte path: ld % 4 == 0; register / scalar path: odd ld."""
    r4 = (rows + 3) // 4 * 4
    return r4 + 4 if path == "dma" else r4 + 1


def _check_propagation(got, clean, A, B, what):
    """got / clean: device results (nb, na) of A^T B with and without the planted elements."""
    cls = ei.tn_class_ref(A, B)                                   # (na, nb)
    g = got.cpu().numpy().T
    assert np.array_equal(ei.value_class(g), cls), f"{what}: classes differ from numpy fp64 at " \
        f"{np.argwhere(ei.value_class(g) != cls)[:5].tolist()}"
    touched = ei.touched_tn(A, B)
    assert np.all(cls[touched] != ei.FINITE), f"{what}: an output the element takes part in is finite"
    c = clean.cpu().numpy().T
    assert np.array_equal(g[~touched].view(np.int64), c[~touched].view(np.int64)), f"{what}: an untouched output changed"


def _syrk_rows_of_interest(L, K, n):
    nsplit, cps = _syrk_units(L, K, n)
    assert nsplit >= 2
    last_full = (K // 32 - 1) * 32
    rows = {0, 31, 32, last_full, last_full + 31, cps * 32 - 1, cps * 32, (nsplit - 1) * cps * 32, K - 1, K - 2, K - 3}
    return sorted(r for r in rows if 0 <= r < K)


@pytest.mark.parametrize("path", ["dma", "reg"])
@pytest.mark.parametrize("K", [4097, 4098, 4099])
def test_syrk_propagates_non_finite(L, K, path):
    """n = 312 (n % 128 = 56).  One element planted at a time; rows: 0, 31 / 32, the last full chunk, the
    last three rows (K % 4 = 1, 2, 3: inside the ragged last quad), the first and last row of a K-split."""
    n = 312
    rs = np.random.RandomState(K)
    X = rs.standard_normal((K, n)).astype(np.float32)
    ld = _ld_for(path, K)
    clean, _ = syrk(L, _t(X, ld), want32=False)
    rows = _syrk_rows_of_interest(L, K, n)
    cols = [0, 127, 128, n - 1]
    plan = [(i, cols[k % 4], NAN) for k, i in enumerate(rows)] + [(K - 1, j, NAN) for j in cols] + \
           [(rows[3], 128, PINF), (K - 1, n - 1, NINF), (0, 0, PINF)]
    for i, j, v in plan:
        Xp = X.copy()
        Xp[i, j] = v
        if v == v:
            Xp[i, (j + 5) % n] = 0.0                               # Inf * 0 = NaN in that column
        Xc = Xp.copy()
        Xc[i, j] = X[i, j]
        cl = clean if v != v else syrk(L, _t(Xc, ld), want32=False)[0]
        got, got32 = syrk(L, _t(Xp, ld), want32=True)
        assert not bool(torch.isfinite(got[j, j])), "the host's convergence check reads diag(G)"
        assert not bool(torch.isfinite(got[j, :]).any()) and not bool(torch.isfinite(got[:, j]).any())
        _check_propagation(got, cl, Xp, Xp, f"syrk plant {v} at ({i}, {j})")
        assert np.array_equal(ei.value_class(got32.cpu().numpy()), ei.value_class(got.cpu().numpy()))
    # +Inf and -Inf in one column: numpy's classes (+Inf on the diagonal, NaN where Inf - Inf meets)
    Xp = X.copy()
    Xp[5, 127], Xp[K - 2, 127] = PINF, NINF
    got, _ = syrk(L, _t(Xp, ld), want32=False)
    _check_propagation(got, clean, Xp, Xp, "syrk +Inf and -Inf")
    assert not bool(torch.isfinite(got[127, 127]))


@pytest.mark.parametrize("path", ["dma", "reg"])
def test_syrk_blocks_propagates_non_finite(L, path):
    """The element at the block boundaries of the blocks entry point (last row of a block, first of the next),
    in the single-chunk block and in a block behind the 16th."""
    n = 312
    sizes = [1001, 32, 2050] + [64] * 14 + [515]
    rs = np.random.RandomState(6)
    mats = [rs.standard_normal((m, n)).astype(np.float32) for m in sizes]
    X = np.concatenate(mats)

    def run(ms):
        return syrk_blocks(L, [_t(a, _ld_for(path, a.shape[0])) for a in ms], want32=False)[0]

    clean = run(mats)
    for b, i, j in [(0, 1000, 0), (1, 0, 127), (1, 31, 128), (2, 0, n - 1), (2, 2049, 128), (17, 0, 127), (17, 514, n - 1)]:
        for v in (NAN, PINF):
            ms = [a.copy() for a in mats]
            ms[b][i, j] = v
            Xp = np.concatenate(ms)
            got = run(ms)
            assert not bool(torch.isfinite(got[j, j]))
            # (an Inf meets no zero in standard_normal data: its row is +-Inf, still non-finite)
            _check_propagation(got, clean, Xp, Xp, f"syrk_blocks plant {v} in block {b} at ({i}, {j})")
    assert X.shape[0] == sum(sizes)


@pytest.mark.parametrize("path", ["dma", "reg"])
@pytest.mark.parametrize("K,na,nb", [(4099, 312, 70), (4098, 312, 200), (4097, 130, 20)])
def test_gemm_tn_propagates_non_finite(L, K, na, nb, path):
    """The element in A or in B: only that row or column of C is hit."""
    rs = np.random.RandomState(K + nb)
    A, B = rs.standard_normal((K, na)).astype(np.float32), rs.standard_normal((K, nb)).astype(np.float32)
    ld = _ld_for(path, K)
    clean, _ = gemm_tn(L, _t(A, ld), _t(B, ld), want32=False)
    for which, i, j, v in [("A", 0, 0, NAN), ("A", K - 1, na - 1, NAN), ("A", K - 2, 128, PINF), ("A", 4064, 127, NAN),
                           ("B", 0, nb - 1, NAN), ("B", K - 1, 0, NAN), ("B", K - 3, nb - 1, NINF), ("B", 32, nb // 2, NAN)]:
        Ap, Bp = A.copy(), B.copy()
        (Ap if which == "A" else Bp)[i, j] = v
        got, got32 = gemm_tn(L, _t(Ap, ld), _t(Bp, ld), want32=True)
        hit = got[:, j] if which == "A" else got[j, :]
        assert not bool(torch.isfinite(hit).any())
        _check_propagation(got, clean, Ap, Bp, f"gemm_tn plant {v} in {which} at ({i}, {j})")
        assert np.array_equal(ei.value_class(got32.cpu().numpy()), ei.value_class(got.cpu().numpy()))


@pytest.mark.parametrize("nb", [16, 20, 70])
def test_gemm_tn_blocks_propagates_non_finite(L, nb):
    """K3 blocks (nb = 70) and K3s (nb <= 32, aligned blocks of K >= 512, no fp32 copy; 4160 + 1030: the rows
    behind the last 64-row chunk of a block go through the generic launch on top)."""
    na, sizes = 300, [4160, 1030, 512]
    rs = np.random.RandomState(nb)
    As = [rs.standard_normal((m, na)).astype(np.float32) for m in sizes]
    Bs = [rs.standard_normal((m, nb)).astype(np.float32) for m in sizes]

    def run(As_, Bs_):
        return gemm_tn_blocks(L, [_t(a, _ld_for("dma", a.shape[0])) for a in As_],
                              [_t(b, _ld_for("dma", b.shape[0])) for b in Bs_], want32=False)[0]

    clean = run(As, Bs)
    for which, b, i, j, v in [("A", 0, 0, 0, NAN), ("A", 0, 4159, na - 1, NAN), ("A", 1, 1029, 128, NAN), ("A", 1, 1024, 127, PINF),
                              ("B", 2, 511, nb - 1, NAN), ("B", 1, 1025, 0, NAN), ("B", 0, 4096, nb - 1, NINF)]:
        Ap, Bp = [a.copy() for a in As], [x.copy() for x in Bs]
        (Ap if which == "A" else Bp)[b][i, j] = v
        got = run(Ap, Bp)
        hit = got[:, j] if which == "A" else got[j, :]
        assert not bool(torch.isfinite(hit).any())
        _check_propagation(got, clean, np.concatenate(Ap), np.concatenate(Bp), f"blocks plant {v} in {which}[{b}] at ({i}, {j})")


@pytest.mark.parametrize("m", [1027, 1024])
@pytest.mark.parametrize("l,old", [(20, False), (56, False), (70, False), (100, False), (300, False), (70, True)])
def test_skinny_propagates_non_finite(L, l, old, m):
    """X[i, k] hits row i of Y only -- the last row with m % 4 = 3 and m % 256 != 0 is the clamped-row case,
    with its neighbours in the same 4-row register; W[k, c] hits column c only -- c = l - 1 with l % 16 != 0
    sits next to the padded granule.  With the fused Gram (l <= 224), G is non-finite where Y^T Y is."""
    n = 101
    rs = np.random.RandomState(m + l)
    X, W = rs.standard_normal((m, n)).astype(np.float32), rs.standard_normal((n, l)).astype(np.float32)
    ldx = (m + 3) // 4 * 4 + 4
    gram_ok = l <= (96 if old else 224)
    with _k2_impl_env(old):
        def run(Xh, Wh):
            G = torch.full((l, l), NAN, dtype=F64, device=DEV) if gram_ok else None
            Yt = skinny(L, _t(Xh, ldx), _pitched(Wh), gram=G, accumulate=0)
            return Yt, G

        Yc, Gc = run(X, W)
        plan = [("X", i, k, v) for i, k, v in [(m - 1, 0, NAN), (m - 2, n - 1, NAN), (m - 3, 50, NAN), (m - 4, 7, NAN),
                                                (0, 0, NAN), (255, 3, PINF), (256, n - 1, NINF), (m - 1, n - 1, PINF)]] + \
               [("W", k, c, v) for k, c, v in [(0, l - 1, NAN), (n - 1, 0, NAN), (50, l // 2, PINF), (n - 1, l - 1, NINF),
                                                (3, min(l - 1, 15), NAN), (3, min(l - 1, 16), NAN)]]
        for which, r, c, v in plan:
            Xp, Wp = X.copy(), W.copy()
            (Xp if which == "X" else Wp)[r, c] = v
            Yt, G = run(Xp, Wp)
            cls = ei.nn_class_ref(Xp, Wp)                           # (m, l)
            y = Yt.cpu().numpy().T
            what = f"skinny plant {v} in {which} at ({r}, {c})"
            assert np.array_equal(ei.value_class(y), cls), what
            touched = np.zeros((m, l), dtype=bool)
            if which == "X":
                touched[r, :] = True
            else:
                touched[:, c] = True
            assert np.all(cls[touched] != ei.FINITE), what
            yc = Yc.cpu().numpy().T
            assert np.array_equal(y[~touched].view(np.int32), yc[~touched].view(np.int32)), what + ": an untouched element of Y changed"
            if G is not None:
                g = G.cpu().numpy()
                with np.errstate(all="ignore"):
                    gcls = ei.value_class(y.astype(np.float64).T @ y.astype(np.float64))
                assert np.array_equal(ei.value_class(g), gcls), what + ": Gram classes"
                gt = np.ones((l, l), dtype=bool) if which == "X" else (np.arange(l) == c)[:, None] | (np.arange(l) == c)[None, :]
                assert np.array_equal(g[~gt].view(np.int64), Gc.cpu().numpy()[~gt].view(np.int64)), what + ": untouched Gram entry"


@pytest.mark.parametrize("name,ld,off", K5_LAYOUTS)
def test_row_center_scale_propagates_non_finite_and_constant_rows(L, name, ld, off):
    """A NaN in one row: that row, its mean and its std are NaN; the other three rows of its quad and
    everything else are bit-identical to the clean run.  A CONSTANT row with scale: mean is the constant
    exactly, std exactly 0, the row becomes 0 / 0 = NaN -- the contract (numpy's, and the reference's
    standardize, do the same), not an accident; neighbours clean."""
    m, n = 1003, 24
    data, mu, V = _k5_rows(m, n, 9)
    for scale in (0, 1):
        def run(dat):
            Xt = _k5_buffer(dat, ld, off)
            mean = torch.full((m,), 7.0, dtype=F32, device=DEV)
            std = torch.full((m,), 7.0, dtype=F32, device=DEV)
            assert L.dmdx_row_center_scale_f32(_p(Xt), m, n, ld, _p(mean), _p(std) if scale else None, scale, _stream()) == 0
            torch.cuda.synchronize()
            return Xt.cpu().numpy(), mean.cpu().numpy(), std.cpu().numpy()

        Xc, mc, sc = run(data)
        for r, t in [(0, 0), (1001, n - 1), (1002, 5), (514, 11), (3, 23)]:
            dat = data.copy()
            dat[t, r] = np.nan
            Xg, mg_, sg = run(dat)
            rest = np.arange(m) != r
            assert np.isnan(Xg[:, r]).all() and np.isnan(mg_[r]) and (not scale or np.isnan(sg[r]))
            assert np.array_equal(Xg[:, rest].view(np.int32), Xc[:, rest].view(np.int32))
            assert np.array_equal(mg_[rest], mc[rest]) and np.array_equal(sg[rest], sc[rest])
        for r in (0, 513, 1002):
            dat = data.copy()
            dat[:, r] = 273.15
            Xg, mg_, sg = run(dat)
            rest = np.arange(m) != r
            assert mg_[r] == np.float32(273.15)
            if scale:
                assert sg[r] == 0.0 and np.isnan(Xg[:, r]).all()
            else:
                assert np.all(Xg[:, r] == 0.0)
            assert np.array_equal(Xg[:, rest].view(np.int32), Xc[:, rest].view(np.int32))
            assert np.array_equal(mg_[rest], mc[rest]) and np.array_equal(sg[rest], sc[rest])


def _xt(X):
    return torch.from_numpy(np.ascontiguousarray(X.T)).to(DEV)


@pytest.mark.parametrize("delay", [1, 2])
@pytest.mark.parametrize("layout", ["resident", "blocked"])
@pytest.mark.parametrize("algo", ["snapshots", "randomized"])
def test_host_raises_on_non_finite_input(KERN, algo, layout, delay):
    """The GPU twin of test_host_algorithms.py::test_non_finite_input_raises_like_numpy: one NaN in X, the
    real HipKernels; np.linalg.svd (the reference's call) raises LinAlgError, and so does the engine."""
    from dmd_era5_amd import svd as dsvd

    X = orc.lowrank_matrix(512, 40, 10, 1)
    X[17, 3] = np.nan
    Xt = _xt(X)
    arg = Xt if layout == "resident" else [Xt[:, :300].contiguous(), Xt[:, 300:].contiguous()]
    with pytest.raises(np.linalg.LinAlgError):
        if algo == "snapshots":
            dsvd.svd_snapshots(arg, 5, delay=delay, kern=KERN)
        else:
            dsvd.svd_randomized(arg, 5, delay=delay, random_state=0, kern=KERN)


def test_constant_point_with_scale_does_not_reach_the_svd_silently(KERN):
    """A space point that is constant in time, standardised with scale: K5 turns its row into NaN (0 / 0, as
    numpy does for the reference); the SVD that follows raises instead of returning factors of a NaN matrix."""
    from dmd_era5_amd import svd as dsvd

    X = orc.lowrank_matrix(512, 40, 10, 2).astype(np.float32) + 280.0
    X[100, :] = 273.15
    Xt = _xt(X)
    mean, std = KERN.row_center_scale_(Xt, True)
    assert float(mean[100]) == float(np.float32(273.15)) and float(std[100]) == 0.0
    assert bool(torch.isnan(Xt[:, 100]).all()) and bool(torch.isfinite(Xt[:, :100]).all())
    with pytest.raises(np.linalg.LinAlgError):
        dsvd.svd_snapshots(Xt, 5, kern=KERN)


# =================================================================== C. 2^k scaling, all-positive data
def _mag_data(rs, rows, cols):
    """Magnitudes 2^u, u uniform in [-4, 2], random signs."""
    return (np.exp2(rs.uniform(-4.0, 2.0, size=(rows, cols))) * rs.choice([-1.0, 1.0], size=(rows, cols))).astype(np.float32)


def _bits_equal(a, b):
    return torch.equal(a, b)


@pytest.mark.parametrize("path", ["dma", "reg"])
@pytest.mark.parametrize("e", [40, -40])
def test_products_commute_with_power_of_two_scaling(L, e, path):
    """K1, K1 blocks, K3 on X, 2^e X: a power of two commutes with every rounding while nothing overflows
    or turns subnormal (products reach 2^84 and 2^-88: inside fp32)."""
    K, n, nb = 20481, 312, 70
    rs = np.random.RandomState(40)
    X, B = _mag_data(rs, K, n), _mag_data(rs, K, nb)
    s = np.float32(2.0 ** e)
    Xs, Bs = X * s, B * s
    assert np.array_equal(Xs.astype(np.float64), X.astype(np.float64) * 2.0 ** e) and np.all(np.abs(Xs) >= 2.0 ** -126)
    ld = _ld_for(path, K)
    f = 2.0 ** (2 * e)
    G, G32 = syrk(L, _t(X, ld))
    Gs, Gs32 = syrk(L, _t(Xs, ld))
    assert bool(torch.isfinite(Gs).all()) and _bits_equal(Gs, G * f), f"syrk: {int((Gs != G * f).sum())} entries differ"
    assert _bits_equal(Gs32, G32 * f)
    cuts = [0, 4099, 4099 + 32, K]
    blk = lambda M: [_t(M[a:b], _ld_for(path, b - a)) for a, b in zip(cuts[:-1], cuts[1:])]      # noqa: E731
    Gb, _ = syrk_blocks(L, blk(X), want32=False)
    Gbs, _ = syrk_blocks(L, blk(Xs), want32=False)
    assert _bits_equal(Gbs, Gb * f)
    Cm, C32 = gemm_tn(L, _t(X, ld), _t(B, ld))
    Cs, Cs32 = gemm_tn(L, _t(Xs, ld), _t(Bs, ld))
    assert bool(torch.isfinite(Cs).all()) and _bits_equal(Cs, Cm * f) and _bits_equal(Cs32, C32 * f)


@pytest.mark.parametrize("e", [40, -40])
@pytest.mark.parametrize("l", [20, 70, 220])
def test_skinny_commutes_with_power_of_two_scaling(L, l, e):
    """K2 (+ Gram) with 2^e on X and 1 on W: Y scales by 2^e, G by 2^2e, bit for bit."""
    m, n = 20483, 101
    rs = np.random.RandomState(l)
    X, W = _mag_data(rs, m, n), _mag_data(rs, n, l)
    Xs = X * np.float32(2.0 ** e)
    ldx = (m + 3) // 4 * 4 + 4
    G = torch.full((l, l), NAN, dtype=F64, device=DEV)
    Gs = torch.full((l, l), NAN, dtype=F64, device=DEV)
    Y = skinny(L, _t(X, ldx), _pitched(W), gram=G)
    Ys = skinny(L, _t(Xs, ldx), _pitched(W), gram=Gs)
    assert bool(torch.isfinite(Ys).all()) and _bits_equal(Ys, Y * 2.0 ** e), f"{int((Ys != Y * 2.0 ** e).sum())} elements of Y differ"
    assert _bits_equal(Gs, G * 2.0 ** (2 * e)), f"{int((Gs != G * 2.0 ** (2 * e)).sum())} Gram entries differ"
    # without the Gram (for 32 < l <= 96 another launch than the fused one, with its own k order)
    Yp, Yps = skinny(L, _t(X, ldx), _pitched(W)), skinny(L, _t(Xs, ldx), _pitched(W))
    assert _bits_equal(Yps, Yp * 2.0 ** e)


def test_products_stay_finite_at_the_documented_edge(L):
    """amax = 2^40 (the largest magnitude the host's guard passes on un-rescaled), K = 1 000 003: sums of
    2^80 products stay far inside fp32 and keep the chain bound."""
    K, n = 1000003, 40
    rs = np.random.RandomState(41)
    X = (rs.uniform(-1.0, 1.0, size=(K, n)) * 2.0 ** 40).astype(np.float32)
    X[K - 1, n - 1] = 2.0 ** 40
    assert np.abs(X).max() == 2.0 ** 40
    G, G32 = syrk(L, _t(X))
    assert bool(torch.isfinite(G).all()) and bool(torch.isfinite(G32).all())
    X64 = X.astype(np.float64)
    err = np.abs(G.cpu().numpy() - X64.T @ X64)
    bound = ei.chain_bound_factor(K) * (np.abs(X64).T @ np.abs(X64))
    print(f"max err / bound = {(err / bound).max():.4f}")
    assert np.all(err <= bound)


@pytest.mark.parametrize("K", [4096, 4097, 131072, 1000003])
def test_uncentred_field_keeps_the_chain_bound(L, K):
    """Values uniform in [250, 300] (un-centred temperature): no cancellation, partial sums grow linearly.
    Bound: Higham's worst case for what the header promises (exact_inputs.chain_bound_factor), which does
    NOT grow with K; reference numpy fp64.  The measured ratios are recorded in MEASUREMENTS.md."""
    n, nb = 300, 70
    rs = np.random.RandomState(K)
    X = (rs.rand(K, n) * 50 + 250).astype(np.float32)
    B = (rs.rand(K, nb) * 50 + 250).astype(np.float32)
    X64, B64 = X.astype(np.float64), B.astype(np.float64)
    f = ei.chain_bound_factor(K)
    Xt, Bt = _t(X), _t(B)
    G, _ = syrk(L, Xt, want32=False)
    ref = X64.T @ X64                                         # all positive: sum |a||b| is the reference itself
    r1 = float((np.abs(G.cpu().numpy() - ref) / (f * ref)).max())
    Cm, _ = gemm_tn(L, Xt, Bt, want32=False)
    refc = X64.T @ B64
    r3 = float((np.abs(Cm.cpu().numpy().T - refc) / (f * refc)).max())
    print(f"K = {K}: max err / bound  K1 {r1:.4f}  K3 {r3:.4f}  (bound factor {f:.3e})")
    assert r1 <= 1.0 and r3 <= 1.0


# =================================================================== D. a single product is a batch of one
# The single entry points run the blocks path with one block: same plan, same units, same partial tiles.
# Gram n: 70 / 96 the plain-product Gram (96-row tile), 130 / 300 two / three tile rows with the mirror;
# product nb at na = 130: tile heights 32, 48, 64, 80, 96, 112, 128 and the 128 + 96 row split.
ONE_CASES = [("gram", n) for n in (70, 96, 130, 300)] + [("tn", nb) for nb in (20, 40, 64, 70, 96, 100, 128, 220)]


@pytest.mark.parametrize("path", ["dma", "reg"])
@pytest.mark.parametrize("K", [1029, 4100])
@pytest.mark.parametrize("kind,n", ONE_CASES)
def test_single_entry_equals_batch_of_one(L, kind, n, K, path):
    """dmdx_syrk_f32 / dmdx_gemm_tn_f32 against the blocks entry points with nblocks = 1: the fp64 result and
    the fp32 copy bit for bit, accumulate = 0 and 1.  K = 1029 / 4100: 33 / 129 chunks (several K-splits, a
    5- / 4-row tail); ld = K rounded up to a multiple of 4 (LDS-DMA) and the next odd number (registers).
    The C32 the helpers pass keeps K3s out of the way."""
    ld = (K + 3) // 4 * 4 if path == "dma" else K | 1
    rs = np.random.RandomState(K + n)
    At = _t(rs.standard_normal((K, 130 if kind == "tn" else n)).astype(np.float32), ld)
    Bt = _t(rs.standard_normal((K, n)).astype(np.float32), ld) if kind == "tn" else None
    assert (At.data_ptr() % 16 == 0 and ld % 4 == 0) == (path == "dma") and ld >= K
    if kind == "gram":
        single, blocks = (lambda out: syrk(L, At, out)), (lambda out: syrk_blocks(L, [At], out))
    else:
        single, blocks = (lambda out: gemm_tn(L, At, Bt, out)), (lambda out: gemm_tn_blocks(L, [At], [Bt], out))
    S64, S32 = single(None)
    B64, B32 = blocks(None)
    assert bool(torch.isfinite(S64).all()) and S32 is not None and B32 is not None
    assert torch.equal(S64, B64), f"{int((S64 != B64).sum())} fp64 entries differ"
    assert torch.equal(S32, B32), f"{int((S32 != B32).sum())} fp32 entries differ"
    start = torch.from_numpy(rs.standard_normal(tuple(S64.shape))).to(DEV)
    A64, A32 = single(start.clone())
    C64, C32 = blocks(start.clone())
    assert not torch.equal(A64, S64)
    assert torch.equal(A64, C64), f"accumulate = 1: {int((A64 != C64).sum())} fp64 entries differ"
    assert torch.equal(A32, C32), f"accumulate = 1: {int((A32 != C32).sum())} fp32 entries differ"
