"""K1's plane k-step asks for Inf / NaN once per work unit (gemm_tn.hip, tn_unit with PL = 1; csrc/bf16_split.h): the
fast planes everywhere, a NaN test on the unit's result, and a rerun of the whole unit on class-safe planes when it
fires.  tests/test_gpu_syrk_split.py and tests/test_gpu_value_domain.py hold the classes of single plants; this file
adds what the rerun brings:

  * several K-splits with the plant in one of them: the other units of the same tile commit their fast result;
  * the verdict is the workgroup's: a plant feeds the A panel of some tiles and the B panel of others, and in each
    tile only two of the four waves hold a NaN -- all four must run the unit again (they share stages and barriers);
  * the register-staged tail chunk (K % 32 != 0) in both passes;
  * many alarms in one launch, and the rerun's determinism;
  * finite input: bit-identical to the Gram the parent's kernel (per-group detector) gave.

n = 312: two full tile rows and the 56-column edge; leading dimensions for the LDS-DMA and for the register path.
"""
import os

import numpy as np
import pytest
import torch

import exact_inputs as ei

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DEV = "cuda"
N = 312
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "k1_plane_gram_312.npy")

PAYLOAD_NAN = np.array([0x7F800001], dtype=np.uint32).view(np.float32)[0]
PLANTS = [np.float32(np.inf), np.float32(-np.inf), np.float32(np.nan), PAYLOAD_NAN]


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


def gram(L, X, path):
    return syrk(L, _t(X, _ld_for(path, X.shape[0]))).cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def check_classes_and_untouched(got, clean, Xp, what, single=True):
    cls = ei.tn_class_ref(Xp, Xp)
    wrong = np.argwhere(ei.value_class(got.T) != cls)
    assert wrong.size == 0, f"{what}: {len(wrong)} classes differ from numpy fp64, first at {wrong[:5].tolist()}"
    touched = ei.touched_tn(Xp, Xp)
    if single:
        assert np.all(cls[touched] != ei.FINITE) and touched.sum() == 2 * Xp.shape[1] - 1
    assert np.array_equal(_bits(got.T[~touched]), _bits(clean.T[~touched])), f"{what}: an untouched output changed"


# ------------------------------------------------------------------ inputs, made once and never written to
@pytest.fixture(scope="module")
def small():
    """K = 4099 (128 full chunks and a 3-row tail chunk): columns 0 - 63 hold small integers and powers of two
    (m = l = 0: the partners on which a plain split breaks the classes), the rest N(0, 1)."""
    K = 4099
    rs = np.random.RandomState(4099)
    X = rs.standard_normal((K, N)).astype(np.float32)
    X[:, :32] = rs.randint(-9, 10, size=(K, 32)).astype(np.float32)
    X[:, 32:64] = (np.exp2(rs.randint(-6, 7, size=(K, 32))) * rs.choice([-1.0, 1.0], size=(K, 32))).astype(np.float32)
    X.setflags(write=False)
    return X


@pytest.fixture(scope="module")
def small_clean(L, small):
    out = {path: gram(L, small, path) for path in ("dma", "reg")}
    for g in out.values():
        assert np.isfinite(g).all()
    return out


@pytest.fixture(scope="module")
def normal_20481():
    """The N(0, 1) input of test_gpu_syrk_split.py's accuracy_inputs: seed 20481, K = 20 481 (641 chunks, the last a
    single K-tail row), n = 312."""
    X = np.random.RandomState(20481).standard_normal((20481, N)).astype(np.float32)
    X.setflags(write=False)
    return X


@pytest.fixture(scope="module")
def normal_clean(L, normal_20481):
    return {path: gram(L, normal_20481, path) for path in ("dma", "reg")}


# ------------------------------------------------------------------ several K-splits, the plant in one of them
def _first_split_rows(L, X, path):
    """The length of the first K-split, read off a result.  Column 0 becomes (2^26, 1, 1, ...): a unit sums in fp32,
    where 2^52 + 32 is 2^52, so the ones of the unit that holds row 0 are lost; the other units hand their counts to
    the fp64 sum of the splits.  G[0][0] - 2^52 = the rows outside the first split."""
    K = X.shape[0]
    Xp = X.copy()
    Xp[:, 0] = 1.0
    Xp[0, 0] = 2.0 ** 26
    g = gram(L, Xp, path)
    return K - int(g[0, 0] - 2.0 ** 52)


@pytest.mark.parametrize("path", ["dma", "reg"])
def test_plant_in_the_third_of_several_splits(L, normal_20481, normal_clean, path):
    """K = 20 481.  The split length comes from a result (not from a copy of the plan): it must be a multiple of the
    32-row chunk, and at least three splits must exist.  One Inf in the middle of the third split: only the units of
    that split run again; classes as numpy fp64, untouched outputs bit-equal to the clean run."""
    X, K = normal_20481, normal_20481.shape[0]
    rows0 = _first_split_rows(L, X, path)
    print(f"{path}: first split {rows0} rows of {K}")
    assert 0 < rows0 and rows0 % 32 == 0 and 3 * rows0 <= K, f"K = {K} does not run in three or more splits (first split: {rows0} rows)"
    i, j = 2 * rows0 + rows0 // 2, 130
    Xp = X.copy()
    Xp[i, j] = np.inf
    got = gram(L, Xp, path)
    check_classes_and_untouched(got, normal_clean[path], Xp, f"{path}: Inf at ({i}, {j}), splits of {rows0} rows")


# ------------------------------------------------------------------ the verdict reaches all four waves
@pytest.mark.parametrize("path", ["dma", "reg"])
def test_verdict_reaches_all_four_waves(L, small, small_clean, path):
    """K = 4099.  Each of +-Inf, NaN and 0x7F800001, one at a time, in columns 10 and 70 (the two row halves of tile
    row 0), 200 (tile row 1) and 300 (the edge tile), at row 5 and at row K - 1 (the register-staged tail chunk).
    The column is an A-panel column of the tiles right of the diagonal and a B-panel column of those above it: two
    of a tile's four waves see NaN, the rerun has to be the workgroup's."""
    K = small.shape[0]
    for v in PLANTS:
        for j in (10, 70, 200, 300):
            for i in (5, K - 1):
                Xp = small.copy()
                Xp[i, j] = v
                got = gram(L, Xp, path)
                check_classes_and_untouched(got, small_clean[path], Xp, f"{path}: plant {v!r} ({Xp[i, j].view(np.uint32):#x}) at ({i}, {j})")


# ------------------------------------------------------------------ many alarms at once
def _many(small):
    Xp = small.copy()
    Xp[:, 17] = np.nan          # a whole column
    Xp[100, :] = np.inf         # a whole row: every column holds one
    Xp[7, 250] = np.inf         # and both signs in one column: Inf - Inf against its partners
    Xp[9, 250] = -np.inf
    return Xp


@pytest.mark.parametrize("path", ["dma", "reg"])
def test_many_alarms_at_once(L, small, path):
    """K = 4099: a NaN column, an Inf row and +-Inf in one column.  Every unit raises the alarm.  Classes only."""
    Xp = _many(small)
    cls = ei.tn_class_ref(Xp, Xp)
    assert (cls == ei.NAN).any() and (cls == ei.PINF).any() and not (cls == ei.FINITE).any()
    got = gram(L, Xp, path)
    wrong = np.argwhere(ei.value_class(got.T) != cls)
    assert wrong.size == 0, f"{path}: {len(wrong)} classes differ from numpy fp64, first at {wrong[:5].tolist()}"


# ------------------------------------------------------------------ determinism of the rerun
@pytest.mark.parametrize("path", ["dma", "reg"])
def test_rerun_is_deterministic(L, small, path):
    """The same planted input twice: the same bits, NaN payloads compared as classes."""
    Xp = small.copy()
    Xp[2050, 70] = -np.inf
    Xp[small.shape[0] - 1, 200] = PAYLOAD_NAN
    a, b = gram(L, Xp, path), gram(L, Xp, path)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.isnan(a).any() and np.isinf(a).any()
    keep = ~np.isnan(a)
    assert np.array_equal(_bits(a[keep]), _bits(b[keep])), f"{path}: two runs of the same planted input differ"


# ------------------------------------------------------------------ finite input: the parent's bits
@pytest.mark.parametrize("path", ["dma", "reg"])
def test_finite_input_is_bit_identical_to_the_parent(L, normal_clean, path):
    """tests/golden/k1_plane_gram_312.npy is the Gram of normal_20481 (312 x 312 fp64) as commit d74a6e6 computed it
    on an MI355X, the last one with the per-group detector in the k-step (its LDS-DMA path; its register path gave
    the same bits).  The fast loop here runs the same planes through the same 24 MFMAs per group and the same folds:
    every bit must be the same, on both paths."""
    want = np.load(GOLDEN)
    got = normal_clean[path]
    assert want.shape == got.shape and want.dtype == np.float64
    differ = int((_bits(got) != _bits(want)).sum())
    assert differ == 0, f"{path}: {differ} of {got.size} entries differ from the parent's Gram in a bit"
