"""K1 with the bf16 planes made once per call (dmdx_syrk_blocks_planes_f32: csrc/plane_image.h, plane_split.hip, and
tn_unit_planes in gemm_tn.hip).

  * the plane images against a numpy port of bf16split::split2_fast and of the image layout: every byte, pad columns
    and pad rows zero, guard zones in front of and behind a buffer of exactly the declared size untouched;
  * the Gram of the new entry against dmdx_syrk_blocks_f32 on the same input: G64 and G32 through their bytes, NaN
    payloads taken as equal classes (as test_gpu_syrk_rerun.py compares), finite input also against the golden Gram;
  * the plants of test_gpu_syrk_rerun.py (the marked units run again in the launch behind the fast one);
  * DMDX_K1_PLANES=0 against the default through kernels.syrk_blocks.

Non-finite values in the port: the m and l planes of an Inf or NaN are the NaN that Inf - Inf or NaN - NaN leaves, whose
sign and payload IEEE 754 leaves to the implementation, so the port does not take them from the host's FPU but from an
integer rule, and every byte is compared, those planes included: m = l = 0xFFC0 for +-Inf (the default NaN of the
subtraction, sign set), and the value's own high half with the quiet bit set for a NaN (a NaN operand comes back
quieted; x, its h and the m made of them share that half, so which operand an implementation hands back does not
matter).  x86-64 and gfx950 both follow the rule.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DEV = "cuda"
N = 312
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "k1_plane_gram_312.npy")
IMAGE = 24576
GUARD = 4096
PAYLOAD_NAN = np.array([0x7F800001], dtype=np.uint32).view(np.float32)[0]
PLANTS = [np.float32(np.inf), np.float32(-np.inf), np.float32(np.nan), PAYLOAD_NAN]


@pytest.fixture(scope="module")
def L():
    from dmd_era5_amd.kernels import default_kernels

    return default_kernels()._lib


def _t(a, ld=None):
    """Host matrix (rows x cols) -> device tensor (cols, rows) with row stride ld (default: rows rounded up to 4)."""
    a = np.asarray(a, dtype=np.float32)
    rows, cols = a.shape
    ld = ld or (rows + 3) // 4 * 4
    buf = torch.zeros((cols, ld), dtype=F32, device=DEV)
    buf[:, :rows] = torch.from_numpy(np.ascontiguousarray(a.T))
    return buf[:, :rows]


def _arrays(blocks):
    nb = len(blocks)
    ms = (C.c_int64 * nb)(*[int(b.shape[1]) for b in blocks])
    lds = (C.c_int64 * nb)(*[int(b.stride(0)) for b in blocks])
    ptrs = (C.c_void_p * nb)(*[b.data_ptr() for b in blocks])
    return nb, ptrs, ms, lds


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _out(n, G0):
    G64 = torch.full((n, n), float("nan"), dtype=F64, device=DEV) if G0 is None else G0.clone()
    return G64, torch.full((n, n), float("nan"), dtype=F32, device=DEV)


def gram_old(L, blocks, G0=None):
    nb, ptrs, ms, lds = _arrays(blocks)
    n = int(blocks[0].shape[0])
    G64, G32 = _out(n, G0)
    ws = torch.empty(int(L.dmdx_syrk_blocks_workspace_bytes(ms, nb, n)), dtype=torch.uint8, device=DEV)
    rc = L.dmdx_syrk_blocks_f32(ptrs, ms, lds, nb, n, G64.data_ptr(), n, G32.data_ptr(), n, int(G0 is not None),
                                ws.data_ptr(), ws.numel(), _stream())
    assert rc == 0, L.dmdx_last_error()
    torch.cuda.synchronize()
    return G64.cpu().numpy(), G32.cpu().numpy()


def gram_new(L, blocks, G0=None, want_planes=False):
    """-> (G64, G32[, the bytes of the plane buffer]): the plane buffer is exactly the declared size, between two
    guard zones of 0xFF."""
    nb, ptrs, ms, lds = _arrays(blocks)
    n = int(blocks[0].shape[0])
    G64, G32 = _out(n, G0)
    ws = torch.empty(int(L.dmdx_syrk_blocks_workspace_bytes(ms, nb, n)), dtype=torch.uint8, device=DEV)
    need = int(L.dmdx_syrk_planes_bytes(ms, nb, n))
    assert need == sum(-(-n // 128) * -(-int(m) // 32) * IMAGE for m in ms)
    buf = torch.full((GUARD + need + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    assert (buf.data_ptr() + GUARD) % 16 == 0
    rc = L.dmdx_syrk_blocks_planes_f32(ptrs, ms, lds, nb, n, G64.data_ptr(), n, G32.data_ptr(), n, int(G0 is not None),
                                       ws.data_ptr(), ws.numel(), buf.data_ptr() + GUARD, need, _stream())
    assert rc == 0, L.dmdx_last_error()
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:GUARD] == 0xFF).all() and (host[GUARD + need:] == 0xFF).all(), "a guard zone of the plane buffer was written"
    if want_planes:
        return G64.cpu().numpy(), G32.cpu().numpy(), host[GUARD:GUARD + need]
    return G64.cpu().numpy(), G32.cpu().numpy()


def same_bytes_nan_as_class(a, b, what):
    """Equal in every byte, NaN payloads taken as equal classes."""
    assert a.shape == b.shape and a.dtype == b.dtype
    na, nb_ = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb_), f"{what}: NaN in different places ({int((na != nb_).sum())} entries)"
    iv = np.int64 if a.dtype == np.float64 else np.int32
    differ = int((np.ascontiguousarray(a).view(iv)[~na] != np.ascontiguousarray(b).view(iv)[~na]).sum())
    assert differ == 0, f"{what}: {differ} of {a.size} entries differ in a bit"


def both_agree(L, blocks, what, G0=None):
    o64, o32 = gram_old(L, blocks, G0)
    n64, n32 = gram_new(L, blocks, G0)
    same_bytes_nan_as_class(n64, o64, what + " (G64)")
    same_bytes_nan_as_class(n32, o32, what + " (G32)")
    return n64


# ------------------------------------------------------------------ the numpy port
def split_port(x):
    """bf16split::split2_fast on every value of the fp32 array x -> (h, m, l) as uint16 bf16 patterns.  Finite values:
    the three operations of split1 in fp32.  Inf and NaN: the integer rule of the module's docstring."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    top = np.uint32(0xFFFF0000)
    xb = x.view(np.uint32)
    fin = np.isfinite(x)
    xf = np.where(fin, x, np.float32(0))
    r = xf - (xf.view(np.uint32) & top).view(np.float32)
    mb = r.view(np.uint32) & top
    lb = (r - mb.view(np.float32)).view(np.uint32)
    h = (xb >> 16).astype(np.uint16)
    nan_half = np.where((xb & np.uint32(0x7FFFFFFF)) == np.uint32(0x7F800000), np.uint16(0xFFC0), h | np.uint16(0x0040))
    m = np.where(fin, (mb >> 16).astype(np.uint16), nan_half)
    l = np.where(fin, (lb >> 16).astype(np.uint16), nan_half)
    return h, m.astype(np.uint16), l.astype(np.uint16)


def image_port(planes_kn, K, n, fill=0):
    """(3, K, n) uint16 -> the images of one block as csrc/plane_image.h lays them out, uint16[...]: panel-major,
    chunk-minor; inside an image piece g * 768 + (plane * 4 + column / 32) * 64 + h * 32 + column % 32, a piece = the
    bf16 of k = 16 g + 4 h + e (e = 0 .. 3), then of k = 16 g + 8 + 4 h + e.  ``fill``: what the padding holds."""
    chunks, panels = -(-K // 32), -(-n // 128)
    pad = np.full((3, chunks * 32, panels * 128), fill, dtype=np.uint16)
    pad[:, :K, :n] = planes_kn
    # k = 32 chunk + 16 g + 8 hi + 4 h + e4, column = 128 panel + 32 cblk + c31
    v = pad.reshape(3, chunks, 2, 2, 2, 4, panels, 4, 32)
    #        axes:  0 plane, 1 chunk, 2 g, 3 hi, 4 h, 5 e4, 6 panel, 7 cblk, 8 c31
    v = v.transpose(6, 1, 2, 0, 7, 4, 8, 3, 5)   # panel, chunk, g, plane, cblk, h, c31, hi, e4
    return np.ascontiguousarray(v).reshape(-1)


def check_planes(got_bytes, X, what):
    """The images of the K x n host block X against the port."""
    K, n = X.shape
    h, m, l = split_port(X)
    want = image_port(np.stack([h, m, l]), K, n)
    got = got_bytes.view(np.uint16)
    assert got.size == want.size, f"{what}: {got.size} bf16 in the images, {want.size} expected"
    differ = np.flatnonzero(got != want)
    nf = ~np.isfinite(X)
    print(f"{what}: {got.size} bf16, {int(nf.sum())} non-finite values; {differ.size} bf16 differ from the port"
          + "".join(f"; [{i}] {got[i]:#06x} != {want[i]:#06x}" for i in differ[:8]))
    assert differ.size == 0, f"{what}: {differ.size} bf16 of the images differ from the port"
    # pad columns and pad rows hold zero planes (the port's zeros, compared above; here in the test's own words)
    padding = image_port(np.zeros((3, K, n), dtype=np.uint16), K, n, fill=1).astype(bool)
    assert padding.sum() == 3 * (-(-K // 32) * 32 * -(-n // 128) * 128 - K * n)
    assert not got[padding].any(), f"{what}: the padding of the images is not zero"


def _bits(u):
    return np.array([u], dtype=np.uint32).view(np.float32)[0]


def _plant_specials(X):
    """+-Inf, NaNs of both signs with the payload in the high half, in the low half and in both, signalling and quiet,
    and -0; the last row (the tail chunk) and the last column among the places."""
    X = X.copy()
    K, n = X.shape
    X[0, 0] = np.inf
    X[min(5, K - 1), n - 1] = -np.inf
    X[K - 1, n // 2] = np.nan
    X[K // 2, 1] = PAYLOAD_NAN
    X[K // 3, 2] = -0.0
    X[K - 1, 3] = -0.0
    for i, u in enumerate([0xFFC00000, 0xFFC12345, 0x7FA00000, 0xFFA0FFFF, 0xFF800001, 0x7FFFFFFF, 0x7F80FFFF]):
        X[(7 * i + 3) % K, (11 * i + 4) % n] = _bits(u)
    return X


# ------------------------------------------------------------------ inputs, made once and never written to
@pytest.fixture(scope="module")
def normal_20481():
    """The N(0, 1) input of test_gpu_syrk_rerun.py: seed 20481, K = 20 481 (641 chunks, the last a single row)."""
    X = np.random.RandomState(20481).standard_normal((20481, N)).astype(np.float32)
    X.setflags(write=False)
    return X


@pytest.fixture(scope="module")
def small():
    """test_gpu_syrk_rerun.py's K = 4099: small integers and powers of two in columns 0 - 63, the rest N(0, 1)."""
    K = 4099
    rs = np.random.RandomState(4099)
    X = rs.standard_normal((K, N)).astype(np.float32)
    X[:, :32] = rs.randint(-9, 10, size=(K, 32)).astype(np.float32)
    X[:, 32:64] = (np.exp2(rs.randint(-6, 7, size=(K, 32))) * rs.choice([-1.0, 1.0], size=(K, 32))).astype(np.float32)
    X.setflags(write=False)
    return X


@pytest.fixture(scope="module")
def small_clean(L, small):
    g = gram_old(L, [_t(small)])
    assert np.isfinite(g[0]).all()
    return g


# ------------------------------------------------------------------ the planes
@pytest.mark.parametrize("K,n,ld", [(20481, 312, None), (31, 100, None), (32, 128, None), (4099, 312, 4099 + 33)])
def test_planes_equal_the_port(L, K, n, ld):
    """n = 312: two full panels and one of 56 columns; K = 20 481: 641 chunks, the last one row; (31, 100) and
    (32, 128): one image, with and without padding; the last case a block with ld > K.  Inf, -Inf, NaN, a NaN with its
    payload in the low bits and -0 are planted.  (n = 100 > 96: the planes are made and used.)"""
    X = _plant_specials(np.random.RandomState(K + n).standard_normal((K, n)).astype(np.float32))
    _, _, planes = gram_new(L, [_t(X, ld)], want_planes=True)
    check_planes(planes, X, f"K = {K}, n = {n}, ld = {ld}")


def test_planes_of_three_blocks_lie_one_behind_the_other(L):
    rs = np.random.RandomState(3)
    Xs = [rs.standard_normal((K, 200)).astype(np.float32) for K in (100, 31, 65)]
    _, _, planes = gram_new(L, [_t(X) for X in Xs], want_planes=True)
    at = 0
    for X in Xs:
        size = 2 * -(-X.shape[0] // 32) * IMAGE
        check_planes(planes[at:at + size], X, f"block of {X.shape[0]} rows at byte {at}")
        at += size
    assert at == planes.size


# ------------------------------------------------------------------ the Gram: new entry against old entry
def test_normal_input_and_the_golden_gram(L, normal_20481):
    got = both_agree(L, [_t(normal_20481)], "N(0, 1), K = 20 481, n = 312")
    want = np.load(GOLDEN)
    differ = int((got.view(np.int64) != want.view(np.int64)).sum())
    assert differ == 0, f"{differ} of {got.size} entries differ from the golden Gram in a bit"


def test_uniform_250_300(L):
    X = np.random.RandomState(250).uniform(250.0, 300.0, size=(20481, N)).astype(np.float32)
    both_agree(L, [_t(X)], "uniform [250, 300]")


def test_three_blocks_in_one_call_and_accumulate(L):
    rs = np.random.RandomState(7)
    blocks = [_t(rs.standard_normal((K, N)).astype(np.float32)) for K in (20481, 4097, 31)]
    both_agree(L, blocks, "blocks of 20 481, 4 097 and 31 rows")
    G0 = torch.from_numpy(rs.standard_normal((N, N))).to(DEV)
    both_agree(L, blocks, "the same with accumulate = 1", G0=G0)


@pytest.mark.parametrize("n", [128, 100])
def test_one_tile(L, n):
    X = np.random.RandomState(n).standard_normal((4099, n)).astype(np.float32)
    both_agree(L, [_t(X)], f"n = {n}")


def test_unaligned_blocks_run_the_old_path_and_leave_the_planes_alone(L, small):
    """An odd leading dimension: the call runs as dmdx_syrk_blocks_f32 does; the plane buffer keeps its 0xFF."""
    Xt = _t(small, 4099 + 2)
    o64, _ = gram_old(L, [Xt])
    n64, _, planes = gram_new(L, [Xt], want_planes=True)
    same_bytes_nan_as_class(n64, o64, "ld = K + 2")
    assert (planes == 0xFF).all()


def test_the_plants_of_the_rerun_tests(L, small, normal_20481):
    """One plant at a time: the third K-split of K = 20 481 (splits of 288 rows, test_gpu_syrk_rerun.py reads them off a
    result), and at K = 4099 both row halves of tile row 0 (columns 10, 70), tile row 1 (200) and the edge tile (300),
    at row 5 and in the tail chunk (row K - 1)."""
    Xp = normal_20481.copy()
    Xp[2 * 288 + 144, 130] = np.inf
    g = both_agree(L, [_t(Xp)], "Inf in the third K-split")
    assert np.isnan(g).any() or np.isinf(g).any()
    K = small.shape[0]
    for v in PLANTS:
        for j in (10, 70, 200, 300):
            for i in (5, K - 1):
                Xp = small.copy()
                Xp[i, j] = v
                both_agree(L, [_t(Xp)], f"plant {v!r} at ({i}, {j})")


def test_many_alarms_at_once(L, small):
    Xp = small.copy()
    Xp[:, 17] = np.nan
    Xp[100, :] = np.inf
    Xp[7, 250] = np.inf
    Xp[9, 250] = -np.inf
    both_agree(L, [_t(Xp)], "a NaN column, an Inf row, +-Inf in one column")


def test_one_plant_leaves_the_other_outputs_as_the_clean_run(L, small, small_clean):
    Xp = small.copy()
    Xp[2050, 70] = -np.inf
    got, _ = gram_new(L, [_t(Xp)])
    keep = np.ones((N, N), dtype=bool)
    keep[70, :] = keep[:, 70] = False
    assert np.array_equal(got.view(np.int64)[keep], small_clean[0].view(np.int64)[keep])
    assert not np.isfinite(got[~keep]).any()


def test_two_calls_give_the_same_bits(L, small):
    Xp = small.copy()
    Xp[2050, 70] = -np.inf
    Xp[small.shape[0] - 1, 200] = PAYLOAD_NAN
    Xt = _t(Xp)
    a, b = gram_new(L, [Xt]), gram_new(L, [Xt])
    same_bytes_nan_as_class(a[0], b[0], "two calls (G64)")
    same_bytes_nan_as_class(a[1], b[1], "two calls (G32)")
    assert np.isnan(a[0]).any() and np.isinf(a[0]).any()


# ------------------------------------------------------------------ the provider and its knob
def test_the_knob_selects_the_old_entry_with_the_same_result(monkeypatch, normal_20481, small):
    from dmd_era5_amd.kernels import HipKernels

    K = HipKernels()
    blocks = [_t(normal_20481[:9000]), _t(small)]
    monkeypatch.delenv("DMDX_K1_PLANES", raising=False)
    a = K.syrk_blocks(blocks).cpu().numpy()
    assert K._planes, "the default did not take the plane entry"
    held = K.release_workspace()
    assert held > 0 and not K._planes and not K._ws
    one, one32 = K.syrk(blocks[1], want32=True)
    assert K._planes, "syrk did not run as a batch of one through the plane entry"
    monkeypatch.setenv("DMDX_K1_PLANES", "0")
    K.release_workspace()
    b = K.syrk_blocks(blocks).cpu().numpy()
    one0, one032 = K.syrk(blocks[1], want32=True)
    assert not K._planes, "DMDX_K1_PLANES=0 still made planes"
    same_bytes_nan_as_class(a, b, "DMDX_K1_PLANES=0 against the default")
    same_bytes_nan_as_class(one.cpu().numpy(), one0.cpu().numpy(), "syrk, G64")
    same_bytes_nan_as_class(one32.cpu().numpy(), one032.cpu().numpy(), "syrk, G32")
