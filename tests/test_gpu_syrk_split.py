"""K1's plane k-step (gemm_tn.hip, tn_unit with PL = 1; csrc/bf16_split.h): the Gram of n > 96 columns runs its
128 x 128 tiles on the bf16 matrix core, six plane products per fp32 product.  tests/test_gpu_value_domain.py holds
it to the value contract on random data; this file adds the cases that data meets only by chance:

  * operands whose m and l planes are ZERO (small integers, powers of two) next to a planted Inf / NaN: a plain split
    multiplies the Inf in h by such a zero plane (Inf * 0 = NaN where numpy has Inf);
  * a NaN whose payload sits in the low 16 bits (0x7F800001): truncation alone turns it into Inf;
  * columns of 1, 1 + 2^-9, 1 + 2^-9 + 2^-18: every one of the six plane products carries a bit of the result that no
    other product carries, and every partial sum is exact -- a missing product is off by 2^-18 relative;
  * the accuracy of the plane body next to the fp32 body (DMDX_K1_ARITH=f32), both inside the chain bound;
  * the knob itself: the fp32 body through DMDX_K1_ARITH=f32 satisfies the exact-integer reference.

n = 312: two full tile rows and a 56-column edge (the remainder of 8760); leading dimensions for the LDS-DMA and
for the register path.
"""
import numpy as np
import pytest
import torch

import exact_inputs as ei

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DEV = "cuda"
N = 312


@pytest.fixture(scope="module")
def L():
    from dmd_era5_amd.kernels import default_kernels

    return default_kernels()._lib


def _t(a, ld=None):
    """Host matrix (rows x cols) -> device tensor (cols, rows) with row stride ld (default tight)."""
    a = np.asarray(a, dtype=np.float32)
    rows, cols = a.shape
    ld = ld or rows
    buf = torch.zeros((cols, ld), dtype=F32, device=DEV)
    buf[:, :rows] = torch.from_numpy(np.ascontiguousarray(a.T))
    return buf[:, :rows]


def _ld_for(path, rows):
    """LDS-DMA path: ld % 4 == 0; register path: odd ld."""
    r4 = (rows + 3) // 4 * 4
    return r4 + 4 if path == "dma" else r4 + 1


def syrk(L, Xt):
    n, m = Xt.shape
    G = torch.full((n, n), float("nan"), dtype=F64, device=DEV)
    ws = torch.empty(int(L.dmdx_syrk_workspace_bytes(m, n)), dtype=torch.uint8, device=DEV)
    ld = Xt.stride(0) if n > 1 else m
    rc = L.dmdx_syrk_f32(Xt.data_ptr(), m, n, ld, G.data_ptr(), n, None, n, 0, ws.data_ptr(), ws.numel(),
                         torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.dmdx_last_error()
    torch.cuda.synchronize()
    return G


# ------------------------------------------------------------------ zero planes next to a planted element
def _zero_plane_data(K, n):
    rs = np.random.RandomState(4099)
    X = rs.standard_normal((K, n)).astype(np.float32)
    X[:, :32] = rs.randint(-9, 10, size=(K, 32)).astype(np.float32)                    # <= 8 significant bits, zeros among them
    X[:, 32:64] = (np.exp2(rs.randint(-6, 7, size=(K, 32))) * rs.choice([-1.0, 1.0], size=(K, 32))).astype(np.float32)
    return X


PAYLOAD_NAN = np.array([0x7F800001], dtype=np.uint32).view(np.float32)[0]
PLANTS = [np.float32(np.inf), np.float32(-np.inf), np.float32(np.nan), PAYLOAD_NAN]


@pytest.mark.parametrize("path", ["dma", "reg"])
def test_zero_plane_partners_keep_numpy_classes(L, path):
    """K = 4099; columns 0 - 63 hold small integers and powers of two (m = l = 0), the rest N(0, 1).  +-Inf, NaN and
    0x7F800001 at rows 0, 31, 32, K - 1 and columns 0, 127, 128, n - 1: every value meets every row and every column
    once.  Classes as numpy fp64, untouched outputs bit-equal to the clean run."""
    K, n = 4099, N
    X = _zero_plane_data(K, n)
    assert np.isnan(PAYLOAD_NAN) and PAYLOAD_NAN.view(np.uint32) == 0x7F800001
    ld = _ld_for(path, K)
    clean = syrk(L, _t(X, ld)).cpu().numpy()
    assert np.isfinite(clean).all()
    rows, cols = [0, 31, 32, K - 1], [0, 127, 128, n - 1]
    for a, i in enumerate(rows):
        for b, j in enumerate(cols):
            v = PLANTS[(a + b) % 4]
            Xp = X.copy()
            Xp[i, j] = v
            got = syrk(L, _t(Xp, ld)).cpu().numpy()
            what = f"plant {v!r} ({Xp[i, j].view(np.uint32):#x}) at ({i}, {j})"
            cls = ei.tn_class_ref(Xp, Xp)
            wrong = np.argwhere(ei.value_class(got.T) != cls)
            assert wrong.size == 0, f"{what}: {len(wrong)} classes differ from numpy fp64, first at {wrong[:5].tolist()}"
            touched = ei.touched_tn(Xp, Xp)
            assert np.all(cls[touched] != ei.FINITE) and touched.sum() == 2 * n - 1
            assert np.array_equal(got.T[~touched].view(np.int64), clean.T[~touched].view(np.int64)), f"{what}: an untouched output changed"


# ------------------------------------------------------------------ every plane product is present
def test_every_plane_product_is_present(L):
    """K = 128, n = 130.  Column c is constant: sign(c) * (1, 1 + 2^-9, 1 + 2^-9 + 2^-18)[c % 3].  For the pairs of kinds
    (0, any), (any, 0) and (1, 1) the product of two values has at most 24 bits and every partial sum of 16-row
    groups is exact in fp32, so G[i][j] = 128 v_i v_j exactly.  (0, 2) needs h l, its mirror l h; (1, 1) needs h m,
    m h and m m: a body that drops one is off by 2^-9 or 2^-18 relative.  Both triangles, three tiles."""
    K, n = 128, 130
    kinds = np.arange(n) % 3
    mags = np.array([1.0, 1.0 + 2.0 ** -9, 1.0 + 2.0 ** -9 + 2.0 ** -18])
    sign = np.where((np.arange(n) // 3) % 2 == 0, 1.0, -1.0)
    v = (sign * mags[kinds]).astype(np.float32)
    assert np.array_equal(v.astype(np.float64), sign * mags[kinds])                    # 19 significant bits: exact in fp32
    X = np.broadcast_to(v, (K, n)).copy()
    exact = (kinds[:, None] == 0) | (kinds[None, :] == 0) | ((kinds[:, None] == 1) & (kinds[None, :] == 1))
    ref = K * np.outer(v.astype(np.float64), v.astype(np.float64))
    assert np.array_equal(ref[exact].astype(np.float32).astype(np.float64), ref[exact])
    assert exact[:128, 128:].any() and exact[128:, 128:].any() and exact[128:, :128].any()
    for ld in (K, K + 1):
        G = syrk(L, _t(X, ld))
        want = torch.from_numpy(ref).to(DEV)
        m = torch.from_numpy(exact).to(DEV)
        bad = ((G != want) & m).nonzero()
        assert torch.equal(G[m], want[m]), f"ld = {ld}: {bad.shape[0]} exact entries differ, first {bad[:5].tolist()}: " \
            f"{[(float(G[i, j]), float(want[i, j])) for i, j in bad[:3].tolist()]}"
        assert torch.equal(G, G.T)


# ------------------------------------------------------------------ accuracy beside the fp32 body
@pytest.fixture(scope="module")
def accuracy_inputs():
    K, n = 20481, N
    rs = np.random.RandomState(20481)
    out = {}
    for name, X in (("normal", rs.standard_normal((K, n)).astype(np.float32)),
                    ("uniform[250,300]", (rs.rand(K, n) * 50 + 250).astype(np.float32))):
        X64 = X.astype(np.float64)
        out[name] = (X, X64.T @ X64, np.abs(X64).T @ np.abs(X64))
    return K, out


@pytest.mark.parametrize("name", ["normal", "uniform[250,300]"])
def test_accuracy_beside_the_fp32_body(L, accuracy_inputs, name, monkeypatch):
    """K = 20 481: 641 chunks in 5 units of at most 129, the last chunk a single K-tail row.  The fp32 body folds its 4096-row chain once
    per block inside such a unit; the plane body folds after EVERY chunk: 129 rounded adds into the second
    accumulator per unit, 32-row MFMA chains.  max err / (chain_bound_factor(K) sum |a||b|) against numpy fp64 for
    the plane body and for DMDX_K1_ARITH=f32; both <= 1.  (The dropped plane products are one-signed on
    all-positive data: about 2^-23 sum |a||b|, against a bound of (2048 + 18) 2^-24.)  The two bodies round
    differently, so on such data their results differ in some bit, which an ignored knob's would not."""
    K, data = accuracy_inputs
    X, ref, refabs = data[name]
    f = ei.chain_bound_factor(K)
    Xt = _t(X, _ld_for("dma", K))
    ratios, got = {}, {}
    for arith in ("planes", "f32"):
        if arith == "f32":
            monkeypatch.setenv("DMDX_K1_ARITH", "f32")
        else:
            monkeypatch.delenv("DMDX_K1_ARITH", raising=False)
        got[arith] = syrk(L, Xt).cpu().numpy()
        ratios[arith] = float((np.abs(got[arith] - ref) / (f * refabs)).max())
    differ = int((got["planes"].view(np.int64) != got["f32"].view(np.int64)).sum())
    print(f"{name}, K = {K}: max err / bound  planes {ratios['planes']:.5f}  f32 {ratios['f32']:.5f}  (bound factor {f:.3e}); "
          f"{differ} of {got['f32'].size} entries differ in a bit between the two bodies")
    assert ratios["planes"] <= 1.0 and ratios["f32"] <= 1.0
    assert differ > 0, "DMDX_K1_ARITH=f32 gave the bits of the plane body: the knob selects nothing"


# ------------------------------------------------------------------ the knob
def test_k1_arith_f32_knob_is_exact_on_integers(L, monkeypatch):
    """DMDX_K1_ARITH=f32: the fp32 k-step, held to the closed-form integer reference of exact_inputs (and so is the
    default, on the same operand: both bodies see the same units)."""
    K, n, D = 20481, N, ei.D_DEFAULT
    a = min(ei.max_a_product(K), 9)
    assert ei.product_exact(a, a, K)
    R = ei.dictionary(D, n, a, seed=K)
    Xt = ei.device_operand(R, ei.row_map_torch(K, D, device=DEV))
    ref = torch.from_numpy(np.ascontiguousarray(np.asarray(ei.gram_ref(R, ei.counts(ei.row_map(K, D))), dtype=np.float64).T)).to(DEV)
    monkeypatch.setenv("DMDX_K1_ARITH", "f32")
    G = syrk(L, Xt)
    assert torch.equal(G, ref), f"f32 body: {int((G != ref).sum())} entries differ from the integer reference"
    monkeypatch.delenv("DMDX_K1_ARITH")
    G = syrk(L, Xt)
    assert torch.equal(G, ref), f"plane body: {int((G != ref).sum())} entries differ from the integer reference"
