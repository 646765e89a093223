"""Memory-edge tests of the C ABI (include/dmdx.h): poisoned pads, guard zones, exact workspaces.

tests/test_gpu_parity.py covers the SHAPES of every kernel; this file covers how they touch
MEMORY.  Every call goes through the ctypes table with explicit pointers, leading dimensions,
workspace pointer and workspace size (the Python wrappers pin exactly those), on operands built by
tests/memguard.py: every pad, every row past K, everything before and behind a matrix is a NaN
with a recognisable payload, every workspace is exactly `*_workspace_bytes` of 0xFF bytes.

Every case asserts four things at once:
  1. the result is within the bound of the matching parity test (numpy fp64 reference from the
     same fp32 inputs; tolerances copied from test_gpu_parity.py, not re-tuned);
  2. every logical output element is written (accumulate == 0);
  3. everything outside the outputs is untouched bit for bit, and the inputs are unmodified;
  4. the guard behind (and before) the workspace is untouched.
Two layouts of the same data must agree within twice the bound (different paths chain
differently, so not bit for bit): every case also runs the tight, aligned control on its data.

Which tile height / kernel body / dispatch branch a case enters is stated next to the case lists.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import memguard as mg
from oracle import era5_oracle as orc
from parity_utils import EPS32

pytestmark = pytest.mark.gpu

E_INVALID, E_WORKSPACE, E_UNSUPPORTED = -1000, -1001, -1002
F32, F64 = torch.float32, torch.float64
EPS64 = 2.0 ** -52


@pytest.fixture(scope="module")
def L():
    from dmd_era5_amd.kernels import default_kernels

    return default_kernels()._lib          # raises (test fails) if libdmdx.so or the GPU is missing


@pytest.fixture(autouse=True)
def _release_device_memory():
    """Nothing of this file stays cached on the device (the full-size tests elsewhere in the
    suite ask for most of the HBM)."""
    yield
    from dmd_era5_amd.kernels import release_cached_workspaces

    release_cached_workspaces()
    torch.cuda.empty_cache()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rand(rs, rows, cols):
    return rs.standard_normal((rows, cols)).astype(np.float32)


def _seed(*xs):
    s = 12345
    for x in xs:
        s = (s * 1000003 + int(x)) % (2 ** 31 - 1)
    return s


# ------------------------------------------------------------------ operands
def _r4(k):
    return (k + 3) // 4 * 4


def _ld_off(layout, rows):
    """(ld, base offset in elements) of an fp32 operand with `rows` contiguous elements per column:
       tight  ld = rows, 16-byte aligned base (aligned only if rows % 4 == 0)
       pad    ld % 4 == 0, ld > rows, aligned base   -> the 16-byte / LDS-DMA paths
       off1..3 as pad, base 1 / 2 / 3 floats past a 16-byte boundary -> the register / scalar paths
       odd    odd ld, aligned base                   -> the register / scalar paths"""
    if layout == "tight":
        return rows, 0
    if layout == "pad":
        return _r4(rows) + 4, 0
    if layout in ("off1", "off2", "off3"):
        return _r4(rows) + 4, int(layout[-1])
    if layout == "odd":
        return (rows + 1 if rows % 2 == 0 else rows + 2), 0
    raise ValueError(layout)


def _input(a, layout, dtype=F32):
    """A guarded, snapshotted input holding the rows x cols host matrix `a`."""
    ld, off = _ld_off(layout, a.shape[0]) if isinstance(layout, str) else layout
    _, h = mg.guarded(a.shape[0], a.shape[1], ld, dtype, off)
    h.fill(a).snapshot()
    return h


def _output(rows, cols, ld, dtype, off=0, init=None):
    _, h = mg.guarded(rows, cols, ld, dtype, off)
    if init is not None:
        h.fill(init)
    return h


def _all_canary(h):
    return bool((h.iview == h.canary).all())


# (ldc, ldc32 or None, base offset of both outputs) as a function of the output's row count
OUT_VARIANTS = [
    lambda n: (n + 3, None, 0),
    lambda n: (n + 8, n + 5, 0),
    lambda n: (n + 3, n + 8, 1),
    lambda n: (n, n + 1, 1),
]


def _check_after(inputs, outputs, ws, written=True):
    for h in outputs:
        if h is None:
            continue
        if written:
            mg.assert_fully_written(h)
        mg.assert_untouched(h, "output")
    for h in inputs:
        mg.assert_unchanged(h)
        mg.assert_untouched(h, "input")
    if ws is not None:
        mg.assert_untouched(ws)


# =================================================================== a. K1 / K3 / K3s
# layouts of the K-contiguous operands: (id, K % 4 forced to, layout of A, layout of B)
TN_LAYOUTS = [
    ("tight", None, "tight", "tight"),             # the control
    ("pad-k1", 1, "pad", "pad"),                   # LDS-DMA path, ragged last quad (K % 4 = 1, 2, 3):
    ("pad-k2", 2, "pad", "pad"),                   #   the tail chunk's load4_tail ends inside the pad
    ("pad-k3", 3, "pad", "pad"),
    ("off1", None, "off1", "off1"),                # ld % 4 == 0, base off by 4 / 8 / 12 bytes:
    ("off2", None, "off2", "off2"),                #   `aligned` false through dmdx_aligned16 alone
    ("off3", None, "off3", "off3"),
    ("odd", None, "odd", "odd"),                   # the one way in the parity suite knows
    ("A-al_B-mis", None, "pad", "off1"),           # one operand aligned, the other not
    ("A-mis_B-al", None, "off2", "pad"),
]

# (K, na, nb): D = C^T has nb rows, so nb picks the tile height make_plan chooses
TN_SHAPES = [
    (64, 3, 2),          # 32-row tile, two chunks, one split
    (3000, 150, 20),     # 32
    (4099, 130, 40),     # 48  (32 + the 16-row block on v_mfma_f32_16x16x4_f32)
    (3001, 257, 60),     # 64
    (3001, 257, 72),     # 80
    (5000, 130, 96),     # 96
    (3000, 150, 100),    # 112
    (4097, 130, 128),    # 128
    (3000, 192, 200),    # stacked: 128 + 80 (tn_row_split)
    (3002, 150, 346),    # stacked: 128 + 128 + 96 (tn_row_split after two full tile rows)
    (100, 128, 70),      # 80, K < 8 chunks, K % 32 != 0
]


def _tn_bound(A, B):
    return 2e-6 * (np.abs(A).astype(np.float64).T @ np.abs(B).astype(np.float64)) + 1e-30


def _call_gemm_tn(L, hA, hB, K, na, nb, hC, hC32, acc, ws, ws_bytes=None):
    return L.dmdx_gemm_tn_f32(hA.ptr, hA.ld, hB.ptr, hB.ld, K, na, nb, hC.ptr, hC.ld,
                              hC32.ptr if hC32 else None, hC32.ld if hC32 else 0, acc, ws.ptr,
                              ws.nbytes if ws_bytes is None else ws_bytes, _stream())


def _call_syrk(L, hX, m, n, hG, hG32, acc, ws, ws_bytes=None):
    return L.dmdx_syrk_f32(hX.ptr, m, n, hX.ld, hG.ptr, hG.ld, hG32.ptr if hG32 else None,
                           hG32.ld if hG32 else 0, acc, ws.ptr, ws.nbytes if ws_bytes is None else ws_bytes, _stream())


def _product_case(call, need, inputs, nrows, ncols, ref, bound, variant, rs, ctl=None, symmetric=False):
    """The common body of the K1 / K3 cases.  `call(hC, hC32, acc, ws, ws_bytes)` launches on the
    guarded `inputs`; the column-major nrows x ncols result is checked against `ref` +- `bound`."""
    ldc, ldc32, off = OUT_VARIANTS[variant](nrows)
    hC = _output(nrows, ncols, ldc, F64, off)
    hC32 = _output(nrows, ncols, ldc32, F32, off) if ldc32 else None
    assert need > 0
    ws = mg.exact_workspace(need)
    # one byte less than the planner asks for: refused, nothing touched
    assert call(hC, hC32, 0, ws, need - 1) == E_WORKSPACE
    torch.cuda.synchronize()
    assert _all_canary(hC) and (hC32 is None or _all_canary(hC32))
    ws.check_unused()
    _check_after(inputs, [hC, hC32], ws, written=False)
    # accumulate = 0 onto canaries, workspace exactly as large as declared, poisoned
    assert call(hC, hC32, 0, ws, None) == 0
    _check_after(inputs, [hC, hC32], ws)
    got = hC.logical()
    err = np.abs(got - ref)
    print(f"max err / bound = {(err / bound).max():.3f}")
    assert np.all(err <= bound)
    if symmetric:
        assert np.array_equal(got, got.T), "both triangles must hold identical values"
    if hC32:
        assert np.array_equal(hC32.logical(), got.astype(np.float32)), "the fp32 copy is the rounded fp64 result"
    if ctl is not None:
        assert np.all(np.abs(got - ctl) <= 2 * bound), "two layouts of the same data differ by more than twice the bound"
    # accumulate = 1 onto known finite values (fresh poison in the workspace)
    C0 = rs.standard_normal((nrows, ncols)) * 10.0
    if symmetric:
        C0 = C0 + C0.T
    hC.fill(C0)
    if hC32:
        hC32.fill(np.full((nrows, ncols), -7.0, dtype=np.float32))
    ws = mg.exact_workspace(need)
    assert call(hC, hC32, 1, ws, None) == 0
    _check_after(inputs, [hC, hC32], ws)
    got1 = hC.logical()
    # (one more fp64 addition: half an ulp of the sum)
    assert np.all(np.abs(got1 - (C0 + ref)) <= bound + EPS64 * (np.abs(C0) + np.abs(ref) + bound))
    if hC32:
        assert np.array_equal(hC32.logical(), got1.astype(np.float32))
    return got


@pytest.mark.parametrize("lay", TN_LAYOUTS, ids=[x[0] for x in TN_LAYOUTS])
@pytest.mark.parametrize("K,na,nb", TN_SHAPES)
def test_gemm_tn_layouts(L, K, na, nb, lay):
    """dmdx_gemm_tn_f32: every tile height, every way into the aligned / unaligned dispatch of
    run_batch, outputs with ldc > na, a fp32 copy with another ldc32, an output base offset."""
    _, kmod, la, lb = lay
    if kmod is not None:
        K = K // 4 * 4 + kmod
    rs = np.random.RandomState(_seed(K, na, nb))
    A, B = _rand(rs, K, na), _rand(rs, K, nb)
    ref = A.astype(np.float64).T @ B.astype(np.float64)           # na x nb, column-major C
    bound = _tn_bound(A, B)
    need = L.dmdx_gemm_tn_workspace_bytes(K, na, nb)
    variant = _seed(K, na, nb, len(la), len(lb), kmod or 0) % len(OUT_VARIANTS)

    def run(hA, hB):
        return lambda hC, hC32, acc, ws, wsb: _call_gemm_tn(L, hA, hB, K, na, nb, hC, hC32, acc, ws, wsb)

    cA, cB = _input(A, "tight"), _input(B, "tight")
    ctl = _product_case(run(cA, cB), need, [cA, cB], na, nb, ref, bound, 0, rs)
    if la == lb == "tight":
        return
    hA, hB = _input(A, la), _input(B, lb)
    _product_case(run(hA, hB), need, [hA, hB], na, nb, ref, bound, variant, rs, ctl=ctl)


# (m, n): the Gram.  n <= 96 runs as a plain product on 32-row blocks (64- / 96-row tile, no mirror pass);
# above, the triangle of 128 x 128 tiles and the mirror pass of the reduce kernel
SYRK_SHAPES = [
    (33, 5),             # plain product, 32-row tile
    (3001, 40),          # plain product, 64-row tile
    (1000, 67),          # plain product, 96-row tile
    (4099, 130),         # 2 tile rows: 3 tiles, one off the diagonal (mirror pass)
    (5000, 129),
    (2000, 300),         # 3 tile rows
]
SYRK_LAYOUTS = [x for x in TN_LAYOUTS if x[2] == x[3]]


@pytest.mark.parametrize("lay", SYRK_LAYOUTS, ids=[x[0] for x in SYRK_LAYOUTS])
@pytest.mark.parametrize("m,n", SYRK_SHAPES)
def test_syrk_layouts(L, m, n, lay):
    """dmdx_syrk_f32: Grams of <= 96 columns (plain product) and of more than one tile row (mirror
    pass), both triangles written inside ldg > n, G32 with another ldg32."""
    _, kmod, la, _ = lay
    if kmod is not None:
        m = m // 4 * 4 + kmod
    rs = np.random.RandomState(_seed(m, n))
    X = _rand(rs, m, n)
    X64 = X.astype(np.float64)
    ref, bound = X64.T @ X64, _tn_bound(X, X)
    need = L.dmdx_syrk_workspace_bytes(m, n)
    variant = _seed(m, n, len(la), kmod or 0) % len(OUT_VARIANTS)

    def run(hX):
        return lambda hG, hG32, acc, ws, wsb: _call_syrk(L, hX, m, n, hG, hG32, acc, ws, wsb)

    cX = _input(X, "tight")
    ctl = _product_case(run(cX), need, [cX], n, n, ref, bound, 1, rs, symmetric=True)
    if la == "tight":
        return
    hX = _input(X, la)
    _product_case(run(hX), need, [hX], n, n, ref, bound, variant, rs, ctl=ctl, symmetric=True)


def _ptrs(hs):
    return (C.c_void_p * len(hs))(*[h.ptr for h in hs])


def _i64(xs):
    return (C.c_int64 * len(xs))(*[int(x) for x in xs])


# per-block layouts of the blocks entry points.  `aligned` is the AND over a group of 16 blocks:
# one misaligned block sends the whole group down the register path
def _block_layouts(kind, nblocks):
    if kind == "tight":
        return ["tight"] * nblocks
    if kind == "pad":
        return ["pad"] * nblocks
    if kind == "one-mis":
        return ["pad"] * (nblocks // 2) + ["off1"] + ["pad"] * (nblocks - nblocks // 2 - 1)
    if kind == "odd":
        return ["odd"] * nblocks
    if kind == "mixed":
        return [("pad", "off2", "odd", "off3")[j % 4] for j in range(nblocks)]
    raise ValueError(kind)


BLOCK_KINDS = ["tight", "pad", "one-mis", "odd", "mixed"]


@pytest.mark.parametrize("kind", BLOCK_KINDS)
@pytest.mark.parametrize("sizes,n", [([1000, 777, 1030], 140),      # 2 tile rows, mirror pass; sizes % 4 = 0, 1, 2
                                     ([700] * 17 + [333], 70),       # > 16 blocks: two launches, the second accumulates
                                     ([2051, 64], 260)])             # 3 tile rows, a block of two chunks
def test_syrk_blocks_layouts(L, sizes, n, kind):
    rs = np.random.RandomState(_seed(sum(sizes), n))
    mats = [_rand(rs, m, n) for m in sizes]
    X = np.concatenate(mats)
    X64 = X.astype(np.float64)
    ref, bound = X64.T @ X64, _tn_bound(X, X)
    ms = _i64(sizes)
    need = L.dmdx_syrk_blocks_workspace_bytes(ms, len(sizes), n)

    def run(hs):
        ptrs, lds = _ptrs(hs), _i64([h.ld for h in hs])
        return lambda hG, hG32, acc, ws, wsb: L.dmdx_syrk_blocks_f32(
            ptrs, ms, lds, len(hs), n, hG.ptr, hG.ld, hG32.ptr if hG32 else None, hG32.ld if hG32 else 0, acc,
            ws.ptr, ws.nbytes if wsb is None else wsb, _stream())

    cs = [_input(a, "tight") for a in mats]
    ctl = _product_case(run(cs), need, cs, n, n, ref, bound, 0, rs, symmetric=True)
    if kind == "tight":
        return
    hs = [_input(a, lay) for a, lay in zip(mats, _block_layouts(kind, len(sizes)))]
    variant = 1 + _seed(sum(sizes), n, len(kind)) % 3
    _product_case(run(hs), need, hs, n, n, ref, bound, variant, rs, ctl=ctl, symmetric=True)


def _gemm_tn_blocks_case(L, sizes, na, nb, lays_a, lays_b, variant, no_c32=False):
    rs = np.random.RandomState(_seed(sum(sizes), na, nb))
    As = [_rand(rs, m, na) for m in sizes]
    Bs = [_rand(rs, m, nb) for m in sizes]
    A, B = np.concatenate(As), np.concatenate(Bs)
    ref = A.astype(np.float64).T @ B.astype(np.float64)
    bound = _tn_bound(A, B)
    ks = _i64(sizes)
    need = L.dmdx_gemm_tn_blocks_workspace_bytes(ks, len(sizes), na, nb)

    def run(ha, hb):
        pa, pb, la, lb = _ptrs(ha), _ptrs(hb), _i64([h.ld for h in ha]), _i64([h.ld for h in hb])
        return lambda hC, hC32, acc, ws, wsb: L.dmdx_gemm_tn_blocks_f32(
            pa, la, pb, lb, ks, len(sizes), na, nb, hC.ptr, hC.ld, hC32.ptr if hC32 else None,
            hC32.ld if hC32 else 0, acc, ws.ptr, ws.nbytes if wsb is None else wsb, _stream())

    ca, cb = [_input(a, "tight") for a in As], [_input(b, "tight") for b in Bs]
    ctl = _product_case(run(ca, cb), need, ca + cb, na, nb, ref, bound, 0, rs)
    ha = [_input(a, lay) for a, lay in zip(As, lays_a)]
    hb = [_input(b, lay) for b, lay in zip(Bs, lays_b)]
    if no_c32:
        variant = 0                     # (a fp32 copy sends the call down the generic path)
    _product_case(run(ha, hb), need, ha + hb, na, nb, ref, bound, variant, rs, ctl=ctl)


@pytest.mark.parametrize("kind", BLOCK_KINDS[1:])
@pytest.mark.parametrize("sizes,na,nb", [([3000, 2001, 1030], 150, 72),      # 80-row tiles
                                         ([640] * 17 + [100], 140, 200),      # > 16 blocks, stacked 128 + 80
                                         ([1000, 999], 129, 104)])            # 112-row tile, 2 tile columns
def test_gemm_tn_blocks_layouts(L, sizes, na, nb, kind):
    lays = _block_layouts(kind, len(sizes))
    # the A blocks take the layouts in order, the B blocks in reverse: A aligned with B not, and the reverse
    _gemm_tn_blocks_case(L, sizes, na, nb, lays, lays[::-1], 1 + _seed(sum(sizes), na, nb, len(kind)) % 3)


# K3s (xty_small_kernel<T4>): nb <= 16 -> T4 = 0, <= 20 -> 1, <= 24 -> 2, above -> the 32-row body (-1);
# block lengths that are (4096, 4160) and are not (5000, 3001) multiples of the 64-row chunk -- the rows
# behind the last full chunk go through the generic batched launch, accumulated on top
@pytest.mark.parametrize("nb", [1, 16, 17, 21, 25, 32])
@pytest.mark.parametrize("sizes,na", [([4096, 4160], 300), ([5000, 3001], 260), ([640] * 17 + [1000], 129)])
def test_k3s_small_l_path(L, sizes, na, nb):
    """All blocks 16-byte aligned with ld % 4 == 0, K >= 512 and no fp32 copy: xty_small_ok holds."""
    _gemm_tn_blocks_case(L, sizes, na, nb, ["pad"] * len(sizes), ["pad"] * len(sizes), 0, no_c32=True)


@pytest.mark.parametrize("why", ["short-block", "A-misaligned", "B-misaligned", "odd-ld", "fp32-copy"])
@pytest.mark.parametrize("nb", [1, 20, 32])
def test_k3s_group_with_one_ineligible_block_takes_the_generic_path(L, nb, why):
    """One block that fails xty_small_ok (K < 512, a base off by 4 bytes, an odd ld) or a requested
    fp32 copy sends the whole call down the generic path: same answer, same memory discipline."""
    sizes = [4096, 300 if why == "short-block" else 4160, 1030]
    la, lb = ["pad"] * 3, ["pad"] * 3
    if why == "A-misaligned":
        la[1] = "off1"
    if why == "B-misaligned":
        lb[2] = "off1"
    if why == "odd-ld":
        la[0] = "odd"
    _gemm_tn_blocks_case(L, sizes, 300, nb, la, lb, 1 if why == "fp32-copy" else 0, no_c32=why != "fp32-copy")


def test_blocks_refusals_leave_everything_untouched(L):
    """A group of blocks BEHIND the first 16 that needs a larger workspace or carries a leading
    dimension the kernel cannot address: refused before the first launch, C still all canary.
    (The buffers are what the arguments describe: a missing check gives a wrong answer, not a fault.)"""
    rs = np.random.RandomState(3)
    n = 70
    sizes = [64] * 16 + [16384]                      # the second group's plan has more K-splits than the first's
    mats = [_rand(rs, m, n) for m in sizes]
    hs = [_input(a, "pad") for a in mats]
    ms, lds, ptrs = _i64(sizes), _i64([h.ld for h in hs]), _ptrs(hs)
    need = L.dmdx_syrk_blocks_workspace_bytes(ms, len(sizes), n)
    first = L.dmdx_syrk_blocks_workspace_bytes(ms, 16, n)
    assert first < need
    hG = _output(n, n, n + 3, F64)
    ws = mg.exact_workspace(need)
    rc = L.dmdx_syrk_blocks_f32(ptrs, ms, lds, len(sizes), n, hG.ptr, hG.ld, None, 0, 0, ws.ptr, first, _stream())
    torch.cuda.synchronize()
    assert rc == E_WORKSPACE and _all_canary(hG)
    ws.check_unused()
    hs[16] = _input(mats[16], (1 << 24, 0))          # 70 columns of 64 MiB
    lds, ptrs = _i64([h.ld for h in hs]), _ptrs(hs)
    rc = L.dmdx_syrk_blocks_f32(ptrs, ms, lds, len(sizes), n, hG.ptr, hG.ld, None, 0, 0, ws.ptr, need, _stream())
    torch.cuda.synchronize()
    assert rc == E_UNSUPPORTED and _all_canary(hG)
    ws.check_unused()
    _check_after(hs, [hG], ws, written=False)


# =================================================================== b. K2
# Bodies: l <= 32 runs skinny_kernel<1> (32x32x2, the production path of the reference's default rank);
# 32 < l runs the 16x16x4 body: 33 -> launch16<2, TAIL4 = 1>, 56 -> <3, 2>, 70 -> <4, 2>, 100 -> <7>, 224 -> <14>,
# 300 -> two column groups <10> + <9>; DMDX_K2_IMPL=old: 40 -> skinny_kernel<2>, 70 -> <3>, 100 / 128 -> <4>,
# 200 -> <4> + <3>, fused Gram 40 -> <2, GRAM>, 70 / 96 -> <3, GRAM>.
# (m, n, layout of X, of W, of Y): launch_skinny / launch16 take the 16-byte path only when m % 4 == 0,
# ldx, ldw, ldy % 4 == 0 and all three bases are aligned; every combo below breaks exactly one of them or none
K2_COMBOS = [
    (1024, 96, "tight", "tight", "tight"),     # aligned, nothing padded
    (1024, 101, "pad", "pad", "pad"),          # aligned: pitched W with n % 4 != 0 (the production layout), ldy > m
    (1324, 96, "pad", "pad", "pad"),           # aligned, m no multiple of 256 / 512
    (1001, 101, "pad", "pad", "pad"),          # m % 4 = 1
    (1002, 101, "pad", "tight", "tight"),      # m % 4 = 2, tight W with n % 4 != 0
    (1003, 96, "off1", "pad", "pad"),          # m % 4 = 3, X base off by 4 bytes
    (1024, 96, "off2", "tight", "tight"),      # only X misaligned (base)
    (1024, 96, "tight", "tight", "off1"),      # only Y misaligned (base): a column slice of a larger result
    (1024, 96, "odd", "tight", "tight"),       # only ldx odd
    (1028, 101, "pad", "off3", "pad"),         # only W misaligned (base)
    (1024, 101, "tight", "tight", "tight"),    # only ldw odd (tight W, n % 4 != 0)
    (1024, 96, "tight", "tight", "odd"),       # only ldy odd
]
K2_IDS = [f"m{m}-n{n}-X{x}-W{w}-Y{y}" for m, n, x, w, y in K2_COMBOS]


def _k2_bound(X, W):
    n = X.shape[1]
    return (4 + np.sqrt(n)) * EPS32 * (np.abs(X).astype(np.float64) @ np.abs(W).astype(np.float64)) + 1e-30


class _k2_impl:
    """DMDX_K2_IMPL=old around a block (read per call by the library)."""

    def __init__(self, old):
        self.old = old

    def __enter__(self):
        if self.old:
            os.environ["DMDX_K2_IMPL"] = "old"

    def __exit__(self, *exc):
        if self.old:
            del os.environ["DMDX_K2_IMPL"]


def _k2_plain(L, xptr, m, n, ldx, hW, l, hY):
    return L.dmdx_gemm_nn_skinny_f32(xptr, m, n, ldx, hW.ptr, hW.ld, l, hY.ptr, hY.ld, _stream())


def _k2_gram(L, xptr, m, n, ldx, hW, l, hY, hG, acc, ws, wsb=None):
    return L.dmdx_gemm_nn_skinny_gram_f32(xptr, m, n, ldx, hW.ptr, hW.ld, l, hY.ptr, hY.ld, hG.ptr, hG.ld, acc,
                                          ws.ptr, ws.nbytes if wsb is None else wsb, _stream())


def _k2_check_gram(hG, Y, G0=None):
    Yd = Y.astype(np.float64)
    ref = Yd.T @ Yd
    bound = 4e-6 * (np.abs(Yd).T @ np.abs(Yd)) + 1e-30
    G = hG.logical()
    if G0 is None:
        assert np.all(np.abs(G - ref) <= bound) and np.array_equal(G, G.T)
    else:
        assert np.all(np.abs(G - (G0 + ref)) <= bound + EPS64 * (np.abs(G0) + np.abs(ref) + bound))


def _k2_case(L, m, n, l, lx, lw, ly, gram, old=False):
    rs = np.random.RandomState(_seed(m, n, l))
    X, W = _rand(rs, m, n), _rand(rs, n, l)
    ref = X.astype(np.float64) @ W.astype(np.float64)
    bound = _k2_bound(X, W)
    with _k2_impl(old):
        # control: everything tight
        cX, cW, cY = _input(X, "tight"), _input(W, "tight"), _output(m, l, m, F32)
        assert _k2_plain(L, cX.ptr, m, n, cX.ld, cW, l, cY) == 0
        _check_after([cX, cW], [cY], None)
        Yctl = cY.logical()
        assert np.all(np.abs(Yctl - ref) <= bound)
        hX, hW = _input(X, lx), _input(W, lw)
        ldy, offy = _ld_off(ly, m)
        hY = _output(m, l, ldy, F32, offy)
        if not gram:
            assert _k2_plain(L, hX.ptr, m, n, hX.ld, hW, l, hY) == 0
            _check_after([hX, hW], [hY], None)
        else:
            need = L.dmdx_gemm_nn_skinny_gram_workspace_bytes(m, l)
            assert need > 0
            hG = _output(l, l, l + 3, F64, 1)
            ws = mg.exact_workspace(need)
            # (when both bodies could run the planner declares the larger need: one byte less may still do)
            if old or l <= 32 or l > 96:
                assert _k2_gram(L, hX.ptr, m, n, hX.ld, hW, l, hY, hG, 0, ws, need - 1) == E_WORKSPACE
                torch.cuda.synchronize()
                assert _all_canary(hG) and _all_canary(hY)
                ws.check_unused()
            assert _k2_gram(L, hX.ptr, m, n, hX.ld, hW, l, hY, hG, 0, ws) == 0
            _check_after([hX, hW], [hY, hG], ws)
            _k2_check_gram(hG, hY.logical())
        Y = hY.logical()
        err = np.abs(Y - ref)
        print(f"max err / bound = {(err / bound).max():.3f}")
        assert np.all(err <= bound)
        assert np.all(np.abs(Y.astype(np.float64) - Yctl) <= 2 * bound)
        if gram:
            G0 = rs.standard_normal((l, l)) * 100.0
            hG.fill(G0)
            ws = mg.exact_workspace(need)
            assert _k2_gram(L, hX.ptr, m, n, hX.ld, hW, l, hY, hG, 1, ws) == 0
            _check_after([hX, hW], [hY, hG], ws)
            assert np.array_equal(hY.logical(), Y), "deterministic"
            _k2_check_gram(hG, Y, G0)


K2_PLAIN = [("new", l) for l in (1, 20, 32, 33, 56, 70, 100, 224, 300)] + [("old", l) for l in (40, 70, 100, 128, 200)]
K2_GRAM = [("new", l) for l in (1, 20, 32, 33, 56, 70, 100, 224)] + [("old", l) for l in (40, 70, 96)]


@pytest.mark.parametrize("combo", K2_COMBOS, ids=K2_IDS)
@pytest.mark.parametrize("impl,l", K2_PLAIN)
def test_skinny_layouts(L, impl, l, combo):
    m, n, lx, lw, ly = combo
    _k2_case(L, m, n, l, lx, lw, ly, gram=False, old=impl == "old")


@pytest.mark.parametrize("combo", K2_COMBOS, ids=K2_IDS)
@pytest.mark.parametrize("impl,l", K2_GRAM)
def test_skinny_gram_layouts(L, impl, l, combo):
    m, n, lx, lw, ly = combo
    _k2_case(L, m, n, l, lx, lw, ly, gram=True, old=impl == "old")


@pytest.mark.parametrize("impl,l", [("new", 20), ("new", 70), ("old", 70)])
@pytest.mark.parametrize("mm", [256, 255])
def test_skinny_on_delay_view_with_poisoned_tail(L, mm, impl, l):
    """rows > ldx: the zero-copy delay embedding E[k mm + s, t] = X[s, t + k].  The last column of the
    view ends on the last element of the buffer; what follows is canary."""
    nn, d = 40, 3
    rs = np.random.RandomState(_seed(mm, l))
    X = _rand(rs, mm, nn)
    Xe = orc.delay_embed(X, d)                                  # (d mm, nn - d + 1)
    m, n = d * mm, nn - d + 1
    W = _rand(rs, n, l)
    ref, bound = Xe.astype(np.float64) @ W.astype(np.float64), _k2_bound(Xe, W)
    hX = _input(X.T.reshape(1, -1).T.copy(), "tight")           # the nn snapshots back to back, one flat column
    for lw, ly in (("pad", "pad"), ("tight", "odd")):
        hW = _input(W, lw)
        ldy, offy = _ld_off(ly, m)
        hY = _output(m, l, ldy, F32, offy)
        with _k2_impl(impl == "old"):
            assert _k2_plain(L, hX.ptr, m, n, mm, hW, l, hY) == 0
        _check_after([hX, hW], [hY], None)
        assert np.all(np.abs(hY.logical() - ref) <= bound)


def test_skinny_old_body_through_the_real_condition(L):
    """ldx = 2^23 fails dmdx_skinny16_shape_ok: l = 40 runs skinny_kernel<2> (and its fused Gram) without
    any environment switch; fast_ok is false there (scalar byte offsets would leave 32 bits), so every
    chunk takes the 64-bit address path.  192 MiB of X of which 4100 rows per column are logical."""
    m, n, l, ldx = 4100, 6, 40, 1 << 23
    rs = np.random.RandomState(23)
    X, W = _rand(rs, m, n), _rand(rs, n, l)
    ref, bound = X.astype(np.float64) @ W.astype(np.float64), _k2_bound(X, W)
    hX, hW = _input(X, (ldx, 0)), _input(W, "pad")
    hY = _output(m, l, m + 4, F32)
    assert _k2_plain(L, hX.ptr, m, n, ldx, hW, l, hY) == 0
    _check_after([hX, hW], [hY], None)
    Y = hY.logical()
    assert np.all(np.abs(Y - ref) <= bound)
    # the fused Gram: l = 40 <= 96 is accepted by the old body, 100 is not (the new body would take it)
    need = L.dmdx_gemm_nn_skinny_gram_workspace_bytes(m, l)
    hG, ws = _output(l, l, l + 3, F64), mg.exact_workspace(need)
    hY2 = _output(m, l, m + 4, F32)
    assert _k2_gram(L, hX.ptr, m, n, ldx, hW, l, hY2, hG, 0, ws) == 0
    _check_after([hX, hW], [hY2, hG], ws)
    assert np.array_equal(hY2.logical(), Y)
    _k2_check_gram(hG, Y)


def test_skinny_refuses_lane_offsets_beyond_32_bits(L):
    """m + 4 ldx >= 2^29: the per-lane byte offsets of both bodies would wrap.  DMDX_E_INVALID, nothing
    touched; the buffers are what the arguments describe (2 columns of 2^27 floats)."""
    m, n, l, ldx = 4, 2, 3, 1 << 27
    rs = np.random.RandomState(29)
    X, W = _rand(rs, m, n), _rand(rs, n, l)
    hX, hW = _input(X, (ldx, 0)), _input(W, "pad")
    hY, hG = _output(m, l, m + 4, F32), _output(l, l, l + 1, F64)
    ws = mg.exact_workspace(max(L.dmdx_gemm_nn_skinny_gram_workspace_bytes(m, l), 16))
    assert m + 4 * ldx >= 1 << 29
    assert _k2_plain(L, hX.ptr, m, n, ldx, hW, l, hY) == E_INVALID
    assert _k2_gram(L, hX.ptr, m, n, ldx, hW, l, hY, hG, 0, ws) == E_INVALID
    torch.cuda.synchronize()
    assert _all_canary(hY) and _all_canary(hG)
    ws.check_unused()
    _check_after([hX, hW], [hY, hG], ws, written=False)
    # just below: accepted, and right
    ldx = (1 << 27) - 4
    hX = _input(X, (ldx, 0))
    assert m + 4 * ldx < 1 << 29
    assert _k2_plain(L, hX.ptr, m, n, ldx, hW, l, hY) == 0
    _check_after([hX, hW], [hY], None)
    assert np.all(np.abs(hY.logical() - X.astype(np.float64) @ W.astype(np.float64)) <= _k2_bound(X, W))


@pytest.mark.parametrize("which", ["below", "above"])
def test_skinny_body_switch_at_the_lane_offset_limit(L, which):
    """m + 12 ldx just below 2^29 (the 16x16x4 body: its lane group kk = 3 sits 12 ldx elements in, so the
    last rows' byte offsets end 16 bytes below 2^31) and at 2^29 (dmdx_skinny16_shape_ok says no: l = 33
    runs skinny_kernel<2>, whose farthest lane sits 4 ldx in).  m that large needs the delay-embedded
    view (rows > ldx = 4); Y is 33 columns of 2 GiB.  The reference is evaluated on the first and last
    4096 rows, the rows around a few workgroup boundaries and 8192 random ones; no element of Y may be
    NaN, none may be left unwritten."""
    _release(L)
    ldx, n, l = 4, 8, 33
    m = (1 << 29) - 12 * ldx - (4 if which == "below" else 0)
    assert (m + 12 * ldx < 1 << 29) == (which == "below") and m + 4 * ldx < 1 << 29 and m % 4 == 0
    total = m + (n - 1) * ldx
    _, hX = mg.guarded(total, 1, total, F32)
    hX.view.normal_(generator=torch.Generator(device="cuda").manual_seed(29))
    hX.snapshot()
    rs = np.random.RandomState(29)
    W = _rand(rs, n, l)
    hW, hY = _input(W, "pad"), _output(m, l, m, F32)
    assert _k2_plain(L, hX.ptr, m, n, ldx, hW, l, hY) == 0
    _check_after([hX, hW], [hY], None)
    for j in range(l):
        assert not bool(torch.isnan(hY.view[j]).any())
    edges = np.concatenate([np.arange(-64, 64) + b for b in (1 << 20, 1 << 28, (1 << 28) + (1 << 27), m - (1 << 20))])
    idx = np.unique(np.concatenate([np.arange(4096), np.arange(m - 4096, m), edges, rs.randint(0, m, 8192)]))
    it = torch.from_numpy(idx).cuda()
    Xs = torch.stack([hX.view[0][it + t * ldx] for t in range(n)], dim=1).cpu().numpy()
    Ys = hY.view[:, it].cpu().numpy().T
    assert np.all(np.abs(Ys - Xs.astype(np.float64) @ W.astype(np.float64)) <= _k2_bound(Xs, W))


# =================================================================== c. K5 and scale_columns
@pytest.mark.parametrize("scale", [False, True])
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("m,ld", [(1001, 1004), (1002, 1004), (1003, 1004), (1000, 1000), (1001, 1001),
                                  (1000, 1004), (2, 4), (257, 260)])
def test_row_center_scale_in_place_pads(L, m, ld, off, scale):
    """K5 works in place: the float4 path (ldx % 4 == 0, aligned base) ends inside the pad when
    m % 4 != 0.  Values as in test_row_center_scale_matches_oracle; the ld - m pad rows of every
    column and the guards around mean / std stay canary."""
    n = 24
    rs = np.random.RandomState(m + n)
    data = (rs.rand(n, m) * 30 + 250).astype(np.float32)          # (time, space) like an ERA5 field
    ref, mean, std = orc.standardize(data, axis=0, scale=scale)
    hX = _input(data.T, (ld, off))
    hmean = _output(m, 1, m, F32, off)
    hstd = _output(m, 1, m, F32, 1 - off)
    rc = L.dmdx_row_center_scale_f32(hX.ptr, m, n, ld, hmean.ptr, hstd.ptr if scale else None, int(scale), _stream())
    assert rc == 0
    _check_after([], [hX, hmean] + ([hstd] if scale else []), None)
    mg.assert_untouched(hstd)
    assert scale or _all_canary(hstd)
    got = hX.logical().T                                          # (time, space)
    assert np.allclose(hmean.logical()[:, 0], mean, rtol=1e-6, atol=0)
    assert np.allclose(got, ref, rtol=0, atol=1e-4 * (1 if scale else 30))
    if scale:
        assert np.allclose(hstd.logical()[:, 0], std, rtol=1e-5)
        assert np.allclose(got.std(axis=0), 1, atol=1e-4)
    assert np.allclose(got.mean(axis=0), 0, atol=1e-4)


@pytest.mark.parametrize("m,l,extra", [(1001, 1, 3), (1001, 3, 8), (1000, 70, 4), (5, 70, 1),
                                       (4096 * 256 + 300, 3, 4)])       # gx > 4096: the grid-stride loop
def test_scale_columns_exact(L, m, l, extra):
    """One fp32 multiply per element: exactly numpy's; ldy > m, the pad and alpha's surroundings untouched."""
    rs = np.random.RandomState(m + l)
    Y, alpha = _rand(rs, m, l), _rand(rs, l, 1)
    hY, ha = _input(Y, (m + extra, 1)), _input(alpha, "tight")
    assert L.dmdx_scale_columns_f32(hY.ptr, m, l, hY.ld, ha.ptr, _stream()) == 0
    _check_after([ha], [hY], None)
    assert np.array_equal(hY.logical(), Y * alpha[:, 0][None, :])


# =================================================================== d. leading-dimension thresholds
# 32-bit per-lane offsets inside a 128-column panel: bytes (+ 4 KiB) on the LDS-DMA path -> lda < 2^22, else
# the register path (elements) -> lda < 2^25 on the single entry points, < 2^24 on the blocks entry points;
# beyond: DMDX_E_UNSUPPORTED.  Only a few thousand rows of every column are logical, the rest is canary.
def _release(L):
    from dmd_era5_amd.kernels import release_cached_workspaces

    release_cached_workspaces()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("ld,n", [((1 << 22) - 4, 130),      # last leading dimension of the LDS-DMA path; 2 tile rows
                                  (1 << 22, 130),            # first one of the register path
                                  ((1 << 25) - 4, 128)])     # last one accepted: column 127 starts 2^32 - 2032 bytes / 4 in
def test_syrk_leading_dimension_thresholds(L, ld, n):
    _release(L)
    m = 3000
    rs = np.random.RandomState(_seed(ld, n))
    X = _rand(rs, m, n)
    X64 = X.astype(np.float64)
    ref, bound = X64.T @ X64, _tn_bound(X, X)
    need = L.dmdx_syrk_workspace_bytes(m, n)
    cX = _input(X, "tight")
    ctl = _product_case(lambda hG, hG32, acc, ws, wsb: _call_syrk(L, cX, m, n, hG, hG32, acc, ws, wsb),
                        need, [cX], n, n, ref, bound, 0, rs, symmetric=True)
    hX = _input(X, (ld, 0))
    _product_case(lambda hG, hG32, acc, ws, wsb: _call_syrk(L, hX, m, n, hG, hG32, acc, ws, wsb),
                  need, [hX], n, n, ref, bound, 1, rs, ctl=ctl, symmetric=True)


@pytest.mark.parametrize("big", ["A", "B"])
@pytest.mark.parametrize("ld", [(1 << 22) - 4, 1 << 22])
def test_gemm_tn_leading_dimension_thresholds(L, ld, big):
    _release(L)
    K, na, nb = 3000, 130, 72
    if big == "B":
        na, nb = nb, 130                   # D rows <- B: the long leading dimension on the other MFMA operand
    rs = np.random.RandomState(_seed(ld, na))
    A, B = _rand(rs, K, na), _rand(rs, K, nb)
    ref, bound = A.astype(np.float64).T @ B.astype(np.float64), _tn_bound(A, B)
    need = L.dmdx_gemm_tn_workspace_bytes(K, na, nb)
    cA, cB = _input(A, "tight"), _input(B, "tight")
    ctl = _product_case(lambda hC, hC32, acc, ws, wsb: _call_gemm_tn(L, cA, cB, K, na, nb, hC, hC32, acc, ws, wsb),
                        need, [cA, cB], na, nb, ref, bound, 0, rs)
    hA = _input(A, (ld, 0) if big == "A" else "pad")
    hB = _input(B, (ld, 0) if big == "B" else "pad")
    _product_case(lambda hC, hC32, acc, ws, wsb: _call_gemm_tn(L, hA, hB, K, na, nb, hC, hC32, acc, ws, wsb),
                  need, [hA, hB], na, nb, ref, bound, 2, rs, ctl=ctl)


@pytest.mark.parametrize("entry", ["syrk_blocks", "gemm_tn_blocks"])
def test_blocks_leading_dimension_threshold(L, entry):
    """lda = 2^24 - 4 on the blocks entry points with 129 columns: two tile rows / columns, so the
    element offsets inside a panel span 127 columns of 64 MiB."""
    _release(L)
    sizes, n, ld = [2000, 1000], 129, (1 << 24) - 4
    rs = np.random.RandomState(_seed(ld, n))
    mats = [_rand(rs, m, n) for m in sizes]
    ks = _i64(sizes)
    X = np.concatenate(mats)
    if entry == "syrk_blocks":
        X64 = X.astype(np.float64)
        ref, bound = X64.T @ X64, _tn_bound(X, X)
        need = L.dmdx_syrk_blocks_workspace_bytes(ks, 2, n)
        hs = [_input(mats[0], (ld, 0)), _input(mats[1], "pad")]
        ptrs, lds = _ptrs(hs), _i64([h.ld for h in hs])
        _product_case(lambda hG, hG32, acc, ws, wsb: L.dmdx_syrk_blocks_f32(
            ptrs, ks, lds, 2, n, hG.ptr, hG.ld, hG32.ptr if hG32 else None, hG32.ld if hG32 else 0, acc, ws.ptr,
            ws.nbytes if wsb is None else wsb, _stream()), need, hs, n, n, ref, bound, 1, rs, symmetric=True)
    else:
        nb = 40
        Bs = [_rand(rs, m, nb) for m in sizes]
        B = np.concatenate(Bs)
        ref, bound = X.astype(np.float64).T @ B.astype(np.float64), _tn_bound(X, B)
        need = L.dmdx_gemm_tn_blocks_workspace_bytes(ks, 2, n, nb)
        ha = [_input(mats[0], "pad"), _input(mats[1], (ld, 0))]
        hb = [_input(b, "pad") for b in Bs]
        pa, pb, la, lb = _ptrs(ha), _ptrs(hb), _i64([h.ld for h in ha]), _i64([h.ld for h in hb])
        _product_case(lambda hC, hC32, acc, ws, wsb: L.dmdx_gemm_tn_blocks_f32(
            pa, la, pb, lb, ks, 2, n, nb, hC.ptr, hC.ld, hC32.ptr if hC32 else None, hC32.ld if hC32 else 0, acc,
            ws.ptr, ws.nbytes if wsb is None else wsb, _stream()), need, ha + hb, n, nb, ref, bound, 2, rs)


def test_leading_dimensions_beyond_the_thresholds_are_refused(L):
    """2^24 on the blocks entry points, 2^25 on the single ones: DMDX_E_UNSUPPORTED, nothing touched
    (two columns of that leading dimension are allocated: what the arguments describe)."""
    _release(L)
    m, n = 1000, 2
    rs = np.random.RandomState(5)
    X, B = _rand(rs, m, n), _rand(rs, m, 3)
    hB = _input(B, "pad")
    hG, hC = _output(n, n, n + 3, F64), _output(n, 3, n + 3, F64)
    for ld, single in ((1 << 24, False), (1 << 25, True)):
        hX = _input(X, (ld, 0))
        ks = _i64([m])
        ws = mg.exact_workspace(max(L.dmdx_syrk_workspace_bytes(m, n), L.dmdx_gemm_tn_workspace_bytes(m, n, 3),
                                    L.dmdx_syrk_blocks_workspace_bytes(ks, 1, n),
                                    L.dmdx_gemm_tn_blocks_workspace_bytes(ks, 1, n, 3)))
        if single:
            assert _call_syrk(L, hX, m, n, hG, None, 0, ws) == E_UNSUPPORTED
            assert _call_gemm_tn(L, hX, hB, m, n, 3, hC, None, 0, ws) == E_UNSUPPORTED
            assert _call_gemm_tn(L, hB, hX, m, 3, n, hC, None, 0, ws) == E_UNSUPPORTED
        else:
            # the single entry points still take 2^24 (register path) ...
            assert _call_syrk(L, hX, m, n, hG, None, 0, ws) == 0
            mg.assert_fully_written(hG)
            X64 = X.astype(np.float64)
            assert np.all(np.abs(hG.logical() - X64.T @ X64) <= _tn_bound(X, X))
            hG = _output(n, n, n + 3, F64)
            ws = mg.exact_workspace(ws.nbytes)
            # ... the blocks entry points do not
            assert L.dmdx_syrk_blocks_f32(_ptrs([hX]), ks, _i64([ld]), 1, n, hG.ptr, hG.ld, None, 0, 0, ws.ptr,
                                          ws.nbytes, _stream()) == E_UNSUPPORTED
            assert L.dmdx_gemm_tn_blocks_f32(_ptrs([hX]), _i64([ld]), _ptrs([hB]), _i64([hB.ld]), ks, 1, n, 3, hC.ptr,
                                             hC.ld, None, 0, 0, ws.ptr, ws.nbytes, _stream()) == E_UNSUPPORTED
        torch.cuda.synchronize()
        assert _all_canary(hG) and _all_canary(hC)
        ws.check_unused()
        _check_after([hX, hB], [hG, hC], ws, written=False)
        del hX


# =================================================================== e. fp64 kernels
def _rm_in(a, ld, off=0):
    """A guarded row-major R x C fp64 input (row i at ptr + i ld)."""
    return _input(np.ascontiguousarray(a.T), (ld, off), F64)


def _rm_out(R, Cc, ld, off=0):
    return _output(Cc, R, ld, F64, off)


def _rm_get(h):
    return h.logical().T


@pytest.mark.parametrize("n,b,shift", [(34, 2, 0.5), (258, 34, -1.25), (1000, 78, 3.0), (1024, 130, 7.5)])
def test_symm_skinny_f64_memory(L, n, b, shift):
    rs = np.random.RandomState(n * 7 + b)
    A = rs.standard_normal((n, n))
    G, Q = A + A.T, rs.standard_normal((n, b))
    ref = G @ Q - shift * Q
    bound = 1e-13 * (np.abs(G) @ np.abs(Q) + abs(shift) * np.abs(Q)) + 1e-300
    hG, hQ, hY = _rm_in(G, n + 2), _rm_in(Q, b + 2), _rm_out(n, b, b + 3, 1)
    need = L.dmdx_symm_skinny_workspace_bytes(n, b)
    ws = mg.exact_workspace(need)

    def call(n_=n, b_=b, ldg=n + 2, ldq=b + 2, gp=hG.ptr, qp=hQ.ptr, wsb=need):
        return L.dmdx_symm_skinny_f64(gp, n_, ldg, qp, ldq, b_, shift, hY.ptr, hY.ld, ws.ptr, wsb, _stream())

    # the documented preconditions: n, b, ldg, ldq even; G, Q 16-byte aligned -> refused, nothing touched
    assert call(n_=n - 1) == E_INVALID and call(b_=b + 1) == E_INVALID
    assert call(ldg=n + 1) == E_INVALID and call(ldq=b + 1) == E_INVALID
    assert call(gp=hG.ptr + 8) == E_INVALID and call(qp=hQ.ptr + 8) == E_INVALID
    assert call(wsb=need - 1) == E_WORKSPACE
    torch.cuda.synchronize()
    assert _all_canary(hY)
    ws.check_unused()
    assert call() == 0
    _check_after([hG, hQ], [hY], ws)
    assert np.all(np.abs(_rm_get(hY) - ref) <= bound)


@pytest.mark.parametrize("n,b1,b2", [(1, 2, 2), (300, 34, 78), (1000, 124, 124), (777, 130, 2)])
def test_gemm_tn_f64_memory(L, n, b1, b2):
    rs = np.random.RandomState(n + b1 * 7 + b2)
    A, B = rs.standard_normal((n, b1)), rs.standard_normal((n, b2))
    ref, bound = A.T @ B, 1e-13 * (np.abs(A).T @ np.abs(B)) + 1e-300
    hA, hB, hC = _rm_in(A, b1 + 2), _rm_in(B, b2 + 4), _rm_out(b1, b2, b2 + 1, 1)
    need = L.dmdx_gemm_tn_f64_workspace_bytes(n, b1, b2)
    ws = mg.exact_workspace(need)

    def call(b1_=b1, b2_=b2, lda=b1 + 2, ldb=b2 + 4, ap=hA.ptr, bp=hB.ptr, wsb=need):
        return L.dmdx_gemm_tn_f64(ap, lda, bp, ldb, n, b1_, b2_, hC.ptr, hC.ld, ws.ptr, wsb, _stream())

    assert call(b1_=b1 + 1) == E_INVALID and call(b2_=b2 + 1) == E_INVALID
    assert call(lda=b1 + 3) == E_INVALID and call(ldb=b2 + 5) == E_INVALID
    assert call(ap=hA.ptr + 8) == E_INVALID and call(bp=hB.ptr + 8) == E_INVALID
    assert call(wsb=need - 1) == E_WORKSPACE
    torch.cuda.synchronize()
    assert _all_canary(hC)
    ws.check_unused()
    assert call() == 0
    _check_after([hA, hB], [hC], ws)
    assert np.all(np.abs(_rm_get(hC) - ref) <= bound)


@pytest.mark.parametrize("n,b1,b2", [(1, 2, 1), (17, 2, 3), (300, 34, 78), (1000, 62, 200)])
def test_gemm_nt_f64_memory(L, n, b1, b2):
    rs = np.random.RandomState(n + b1 + b2)
    Q, Mt = rs.standard_normal((n, b1)), rs.standard_normal((b2, b1))
    ref = Q @ Mt.T
    hQ, hM, hY = _rm_in(Q, b1 + 2), _rm_in(Mt, b1 + 4), _rm_out(n, b2, b2 + 3, 1)

    def call(b1_=b1, ldq=b1 + 2, ldm=b1 + 4, qp=hQ.ptr, mp=hM.ptr):
        return L.dmdx_gemm_nt_f64(qp, ldq, n, b1_, mp, ldm, b2, hY.ptr, hY.ld, _stream())

    assert call(b1_=b1 + 1) == E_INVALID and call(ldq=b1 + 3) == E_INVALID and call(ldm=b1 + 5) == E_INVALID
    assert call(qp=hQ.ptr + 8) == E_INVALID and call(mp=hM.ptr + 8) == E_INVALID
    torch.cuda.synchronize()
    assert _all_canary(hY)
    assert call() == 0
    _check_after([hQ, hM], [hY], None)
    assert np.abs(_rm_get(hY) - ref).max() <= 1e-13 * (np.abs(Q) @ np.abs(Mt).T).max()


@pytest.mark.parametrize("d", [1, 3, 5])
def test_delay_shift_sum_f64_memory(L, d):
    rs = np.random.RandomState(d)
    m, n = 300, 37
    X = rs.standard_normal((m, n))
    G = X.T @ X
    Xe = orc.delay_embed(X, d)
    ref = Xe.T @ Xe
    nd = n - d + 1
    hG = _input(G, (n + 3, 1), F64)
    hGd, hGd32 = _output(nd, nd, nd + 2, F64, 1), _output(nd, nd, nd + 5, F32, 3)
    assert L.dmdx_delay_shift_sum_f64(hG.ptr, n, hG.ld, d, hGd.ptr, hGd.ld, hGd32.ptr, hGd32.ld, _stream()) == 0
    _check_after([hG], [hGd, hGd32], None)
    assert np.allclose(hGd.logical(), ref, rtol=1e-12, atol=1e-10)
    assert np.array_equal(hGd32.logical(), hGd.logical().astype(np.float32))


@pytest.mark.parametrize("n", [1, 2, 65, 300])
def test_pack_unpack_triu_memory(L, n):
    """pack reads the upper triangle only (NaN below it), unpack writes both triangles inside lda > n."""
    rs = np.random.RandomState(n)
    A = rs.standard_normal((n, n))
    S = A + A.T
    Su = S.copy()
    Su[np.tril_indices(n, -1)] = np.nan
    hA = _rm_in(Su, n + 3, 1)
    np_ = n * (n + 1) // 2
    hp = _output(np_, 1, np_, F64, 1)
    assert L.dmdx_pack_triu_f64(hA.ptr, n, hA.ld, hp.ptr, _stream()) == 0
    _check_after([hA], [hp], None)
    assert np.array_equal(hp.logical()[:, 0], S[np.triu_indices(n)])
    hp.snapshot()
    hS = _rm_out(n, n, n + 1, 1)
    assert L.dmdx_unpack_triu_f64(hp.ptr, n, hS.ptr, hS.ld, _stream()) == 0
    _check_after([hp], [hS], None)
    assert np.array_equal(_rm_get(hS), S)


def _graded(n, hi, lo, seed):
    rs = np.random.RandomState(seed)
    Qm, _ = np.linalg.qr(rs.standard_normal((n, n)))
    A = (Qm * 10.0 ** np.linspace(hi, lo, n)) @ Qm.T
    return 0.5 * (A + A.T)


@pytest.mark.parametrize("n", [1, 17, 62, 96])
def test_eigh_small_f64_memory(L, n):
    A = _graded(n, 6, -6, n)
    hA, hw, hV = _rm_in(A, n + 3, 1), _output(n, 1, n, F64, 1), _rm_out(n, n, n + 2, 1)
    sweeps = torch.full((3,), -77, dtype=torch.int32, device="cuda")
    assert L.dmdx_eigh_small_f64(hA.ptr, n, hA.ld, hw.ptr, hV.ptr, hV.ld, sweeps.data_ptr() + 4, _stream()) == 0
    _check_after([hA], [hw, hV], None)
    s = sweeps.cpu().tolist()
    assert s[0] == -77 and s[2] == -77 and (n > 1) <= s[1] < 30
    w, V = hw.logical()[:, 0], _rm_get(hV)
    ref = np.linalg.eigvalsh(A)[::-1]
    assert np.all(np.diff(w) <= 0)
    assert np.abs(w - ref).max() <= 1e-13 * ref[0]
    assert np.abs(V.T @ V - np.eye(n)).max() <= 1e-13
    assert np.abs(A @ V - V * w).max() <= 1e-13 * ref[0]


@pytest.mark.parametrize("n", [2, 9, 97, 250])
def test_svd_jacobi_f64_memory(L, n):
    """K7L with ldc, ldz > n and a workspace of exactly the declared size holding 0xFF: the library
    zeroes its barrier words itself."""
    A = _graded(n, 6, -6, n)
    Lc = np.linalg.cholesky(A)
    hC = _input(Lc, (n + 3, 0), F64)                    # COLUMN c at C + c ldc; overwritten
    hs, hZ = _output(n, 1, n, F64, 1), _rm_out(n, n, n + 5, 1)
    sweeps = torch.full((3,), -77, dtype=torch.int32, device="cuda")
    need = L.dmdx_svd_jacobi_workspace_bytes(n)
    ws = mg.exact_workspace(need)
    args = (hC.ptr, n, hC.ld, hs.ptr, hZ.ptr, hZ.ld, sweeps.data_ptr() + 4, ws.ptr)
    assert L.dmdx_svd_jacobi_f64(*args, need - 1, _stream()) == E_WORKSPACE
    torch.cuda.synchronize()
    assert _all_canary(hs) and _all_canary(hZ)
    ws.check_unused()
    mg.assert_unchanged(hC)
    assert L.dmdx_svd_jacobi_f64(*args, need, _stream()) == 0
    _check_after([], [hC, hs, hZ], ws)
    s = sweeps.cpu().tolist()
    assert s[0] == -77 and s[2] == -77 and 1 <= s[1] <= 20
    sig = hs.logical()[:, 0]
    w, V = sig * sig, hZ.logical()                      # row j of Zt = left singular vector j
    ref = np.linalg.eigvalsh(A)[::-1]
    bound = 1e-13 * max(1.0, n / 128.0)
    assert np.all(np.diff(w) <= 0)
    assert np.abs(w - ref).max() <= bound * ref[0]
    assert np.abs(V.T @ V - np.eye(n)).max() <= bound
    assert np.abs(A @ V - V * w).max() <= bound * ref[0]


@pytest.mark.parametrize("want_inv", [True, False])
@pytest.mark.parametrize("n", [1, 33, 64, 250])
def test_potrf_trtri_f64_memory(L, n, want_inv):
    """K10: only the lower triangle of A is read (NaN above it); L / Linv inside ldl / ldi > n with the
    upper triangles exactly zero; exact poisoned workspace."""
    import scipy.linalg as sla

    A = _graded(n, 0, -8, n)
    An = A.copy()
    An[np.triu_indices(n, 1)] = np.nan
    hA = _rm_in(An, n + 3, 1)
    hL, hI = _rm_out(n, n, n + 1, 1), (_rm_out(n, n, n + 2) if want_inv else None)
    hinfo = _output(3, 1, 3, F64, 1)
    need = L.dmdx_potrf_trtri_workspace_bytes(n)
    ws = mg.exact_workspace(need)
    args = (hA.ptr, n, hA.ld, 0.0, hL.ptr, hL.ld, hI.ptr if hI else None, hI.ld if hI else 0, hinfo.ptr, ws.ptr)
    assert L.dmdx_potrf_trtri_f64(*args, need - 1, _stream()) == E_WORKSPACE
    torch.cuda.synchronize()
    assert _all_canary(hL) and _all_canary(hinfo) and (hI is None or _all_canary(hI))
    ws.check_unused()
    assert L.dmdx_potrf_trtri_f64(*args, need, _stream()) == 0
    _check_after([hA], [hL, hI, hinfo], ws)
    ref = np.linalg.cholesky(A)
    st, dmin, dmax = hinfo.logical()[:, 0].tolist()
    Lh = _rm_get(hL)
    assert st == 0.0
    assert np.array_equal(np.triu(Lh, 1), np.zeros_like(Lh))
    assert np.abs(Lh @ Lh.T - A).max() <= 4e-15 * max(n, 16) * np.abs(A).max()
    assert np.abs(Lh - ref).max() <= 1e-8 * np.abs(ref).max()
    assert np.isclose(dmin, np.diag(ref).min(), rtol=1e-9) and np.isclose(dmax, np.diag(ref).max(), rtol=1e-12)
    if want_inv:
        Xh = _rm_get(hI)
        Xref = sla.solve_triangular(ref, np.eye(n), lower=True)
        assert np.array_equal(np.triu(Xh, 1), np.zeros_like(Xh))
        assert np.abs(Lh @ Xh - np.eye(n)).max() <= 1e-9
        assert np.abs(Xh - Xref).max() <= 1e-7 * np.abs(Xref).max()
