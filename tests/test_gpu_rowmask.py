"""K20 (dmdx_row_missing_count_f32 / dmdx_row_mask_apply_f32) through the ctypes table, against the numpy
definitions of tests/rowmask_ref.py.  Both kernels are exact: every comparison is made on integers / bit patterns,
there is no tolerance in this file.  Operands come from tests/memguard.py (NaN canaries in pads and guard zones: a
canary that was read as data would be counted, one that was overwritten is found).

The launches split the snapshots over grid.y.  count: splits of about 64 snapshots (kMinSplit in rowmask.hip, as long
as the launch has fewer than 2048 workgroups): n = 300 runs as 5 splits of 60 for every m here, n <= 64 as one.
apply: splits of 64 snapshots (kApplySplit): n = 300 runs as 4 splits of 64 and one of 44.
"""
import numpy as np
import pytest
import torch

import memguard as mg
import rowmask_ref as rr

pytestmark = pytest.mark.gpu

F32 = torch.float32
DEV = "cuda"
E_INVALID = -1000
MS = (1, 3, 4, 5, 255, 256, 257, 1029)
NS = (1, 2, 15, 16, 17, 300)
SENTINEL = -77
GUARD = 64                                                # ints of SENTINEL on both sides of count


@pytest.fixture(scope="module")
def kern():
    from dmd_era5_amd.kernels import default_kernels

    return default_kernels()


@pytest.fixture(scope="module")
def L(kern):
    return kern._lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _layouts(m):
    """(pad, base offset in floats, name): the float4 route on a tight or pitched view, and the three ways onto the
    dword route."""
    up = (-m) % 4
    return [(up, 0, "aligned, ld = m rounded up" if up else "tight, aligned"),
            (up + 8, 0, "pitched, aligned"),
            (up + 3, 0, "ld % 4 != 0"),
            (up + 4, 1, "base 4 bytes off")]


def _operand(X, pad, off):
    n, m = X.shape
    g = mg.Guarded(m, n, m + pad, F32, off, DEV)
    g.iview.copy_(torch.from_numpy(rr.bits(X).view(np.int32)).to(DEV))       # bit for bit, NaN payloads included
    return g.snapshot()


def _count_buf(m, start=0):
    buf = torch.full((m + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    buf[GUARD:GUARD + m] = start
    return buf


def _count_ptr(buf):
    return buf.data_ptr() + 4 * GUARD


def _check_count(buf, m, want, what):
    got = buf.cpu().numpy()
    assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + m:] == SENTINEL).all(), f"{what}: count written outside [0, m)"
    assert np.array_equal(got[GUARD:GUARD + m], want), f"{what}: counts differ"


def _count(L, g, buf, n=None, row0=0):
    n = g.cols if n is None else n
    return L.dmdx_row_missing_count_f32(g.col_ptr(row0), n, g.rows, g.ld, _count_ptr(buf), _stream())


def _apply(L, g, cnt, value, n=None):
    return L.dmdx_row_mask_apply_f32(g.ptr, g.cols if n is None else n, g.rows, g.ld, cnt.data_ptr(), value, _stream())


# ---------------------------------------------------------------- count
@pytest.mark.parametrize("m", MS)
def test_count_is_exact_on_every_shape_layout_and_pattern(L, m):
    for n in NS:
        for pattern in rr.PATTERNS:
            X, where = rr.planted(n, m, pattern)
            want = rr.count(X)
            assert np.array_equal(want, where.sum(axis=0))
            for pad, off, name in _layouts(m):
                what = f"n={n} m={m} {pattern} ({name})"
                g = _operand(X, pad, off)
                buf = _count_buf(m, start=3)                           # it ADDS: 3 + the count
                assert _count(L, g, buf) == 0, what
                _check_count(buf, m, want + 3, what)
                mg.assert_unchanged(g, what)
                mg.assert_untouched(g, what)


@pytest.mark.parametrize("m,n", [(257, 300), (1029, 17), (5, 300)])
def test_count_accumulates_over_time_slabs(L, m, n):
    X, _ = rr.planted(n, m, "scattered", seed=5)
    for pad, off, name in _layouts(m):
        g = _operand(X, pad, off)
        whole, slabs = _count_buf(m), _count_buf(m)
        assert _count(L, g, whole) == 0
        n1 = n // 3 + 1
        assert _count(L, g, slabs, n=n1) == 0
        assert _count(L, g, slabs, n=n - n1, row0=n1) == 0
        assert torch.equal(whole, slabs), name
        _check_count(whole, m, rr.count(X), name)
        assert _count(L, g, whole) == 0                                # a repeated call adds once more
        _check_count(whole, m, 2 * rr.count(X), name)


def test_empty_shapes_are_no_ops(L, kern):
    buf = _count_buf(7, start=4)
    before = buf.clone()
    X, _ = rr.planted(3, 7, "scattered")
    g = _operand(X, 1, 0)
    assert L.dmdx_row_missing_count_f32(g.ptr, 0, 7, g.ld, _count_ptr(buf), _stream()) == 0
    assert L.dmdx_row_missing_count_f32(g.ptr, 3, 0, g.ld, _count_ptr(buf), _stream()) == 0
    assert L.dmdx_row_missing_count_f32(None, 0, 0, 0, None, _stream()) == 0
    assert L.dmdx_row_mask_apply_f32(g.ptr, 0, 7, g.ld, _count_ptr(buf), 0.0, _stream()) == 0
    assert L.dmdx_row_mask_apply_f32(g.ptr, 3, 0, g.ld, _count_ptr(buf), 0.0, _stream()) == 0
    assert L.dmdx_row_mask_apply_f32(None, 0, 0, 0, None, 0.0, _stream()) == 0
    assert torch.equal(buf, before)
    mg.assert_unchanged(g)
    mg.assert_untouched(g)
    c = kern.row_missing_count(torch.empty((0, 5), dtype=F32, device=DEV))
    assert c.dtype == torch.int32 and c.tolist() == [0] * 5
    assert kern.row_missing_count(torch.empty((4, 0), dtype=F32, device=DEV)).numel() == 0


def test_refusals_write_nothing(L):
    X, _ = rr.planted(4, 9, "scattered")
    g = _operand(X, 3, 0)
    buf = _count_buf(9, start=1)
    before = buf.clone()
    s = _stream()
    for args in [(g.ptr, -1, 9, g.ld), (g.ptr, 4, -1, g.ld), (g.ptr, 4, 9, 8), (g.ptr, 2**31, 9, g.ld),
                 (g.ptr + 2, 4, 9, g.ld), (None, 4, 9, g.ld)]:
        assert L.dmdx_row_missing_count_f32(*args, _count_ptr(buf), s) == E_INVALID, args
        assert L.dmdx_row_mask_apply_f32(*args, _count_ptr(buf), 0.0, s) == E_INVALID, args
    assert L.dmdx_row_missing_count_f32(g.ptr, 4, 9, g.ld, None, s) == E_INVALID
    assert L.dmdx_row_mask_apply_f32(g.ptr, 4, 9, g.ld, None, 0.0, s) == E_INVALID
    assert L.dmdx_row_missing_count_f32(g.ptr, 4, 9, g.ld, _count_ptr(buf) + 1, s) == E_INVALID
    assert b"row_m" in L.dmdx_last_error()
    assert torch.equal(buf, before)
    mg.assert_unchanged(g)
    mg.assert_untouched(g)


# ---------------------------------------------------------------- apply
@pytest.mark.parametrize("m", MS)
def test_apply_touches_the_masked_rows_only(L, m):
    # the mask is an argument of its own, not the count of X: unmasked rows hold NaN and Inf that must keep their bits
    rs = np.random.RandomState(m)
    some = (rs.rand(m) < 0.3).astype(np.int32) * (1 + np.arange(m, dtype=np.int32) % 3)
    some[m // 2] = -1                                                  # != 0 is the test, not > 0
    first, last = np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int32)
    first[0], last[m - 1] = 1, 2**31 - 1
    cases = [(some, 0.0), (some, -0.0), (some, float("nan")), (first, 0.0), (last, 0.0), (np.ones(m, dtype=np.int32), 0.0)]
    for n in NS:
        for pattern in ("scattered", "ragged", "allrow"):
            X, _ = rr.planted(n, m, pattern, seed=2)
            for cnt_host, value in cases:
                cnt = torch.from_numpy(cnt_host).to(DEV)
                want = rr.apply(X, cnt_host, value)
                for pad, off, name in _layouts(m):
                    what = f"n={n} m={m} {pattern} value={value} ({name})"
                    g = _operand(X, pad, off)
                    assert _apply(L, g, cnt, value) == 0, what
                    got = g.iview.cpu().numpy().view(np.uint32)
                    assert np.array_equal(got, want), what
                    mg.assert_untouched(g, what)


def test_apply_with_a_count_of_zeros_changes_no_bit(L):
    X, _ = rr.planted(17, 1029, "scattered", seed=4)
    zeros = torch.zeros(1029, dtype=torch.int32, device=DEV)
    for pad, off, name in _layouts(1029):
        g = _operand(X, pad, off)
        assert _apply(L, g, zeros, float("nan")) == 0
        mg.assert_unchanged(g, name)
        mg.assert_untouched(g, name)


def test_apply_on_a_block_of_u_and_on_one_snapshot(kern):
    k, rows = 7, 1029
    rs = np.random.RandomState(0)
    for shape in ((k, rows), (1, rows)):
        Ut = torch.from_numpy(rs.standard_normal(shape).astype(np.float32)).to(DEV)
        cnt_host = (rs.rand(rows) < 0.3).astype(np.int32) * 5
        want = rr.apply(Ut.cpu().numpy(), cnt_host, 0.0)
        out = kern.row_mask_apply_(Ut, torch.from_numpy(cnt_host).to(DEV))
        assert out is Ut
        assert np.array_equal(rr.bits(Ut.cpu().numpy()), want)
        assert (Ut[:, torch.from_numpy(cnt_host != 0).to(DEV)] == 0).all()


# ---------------------------------------------------------------- wrappers, K5
@pytest.mark.parametrize("m,n", [(1029, 17), (257, 300), (5, 2)])
def test_count_agrees_with_the_means_of_k5(kern, m, n):
    """An fp64 sum of fewer than 2^31 finite fp32 values cannot overflow: the mean of K5 is finite exactly for the
    rows without a missing value."""
    for pattern in ("scattered", "first", "last", "allrow", "none"):
        X, _ = rr.planted(n, m, pattern, seed=7)
        Xt = torch.from_numpy(X).to(DEV)
        cnt = kern.row_missing_count(Xt)
        assert np.array_equal(cnt.cpu().numpy(), rr.count(X))
        out = torch.full((m,), 2, dtype=torch.int32, device=DEV)
        assert kern.row_missing_count(Xt, out=out) is out and torch.equal(out, cnt + 2)
        mean, _ = kern.row_center_scale_(Xt.clone(), False)
        assert torch.equal(~torch.isfinite(mean), cnt > 0), pattern


def test_wrapper_errors(kern):
    from dmd_era5_amd._lib import DmdxError

    X = torch.zeros((4, 8), dtype=F32, device=DEV)
    cnt = torch.zeros(8, dtype=torch.int32, device=DEV)
    with pytest.raises(DmdxError, match="float32"):
        kern.row_missing_count(X.double())
    with pytest.raises(DmdxError, match="device tensor"):
        kern.row_missing_count(X.cpu())
    with pytest.raises(DmdxError, match="inner stride"):
        kern.row_missing_count(X.T)
    with pytest.raises(DmdxError, match="length 8"):
        kern.row_missing_count(X, out=cnt[:7])
    with pytest.raises(DmdxError, match="int32"):
        kern.row_missing_count(X, out=cnt.long())
    with pytest.raises(DmdxError, match="float32"):
        kern.row_mask_apply_(X.double(), cnt)
    with pytest.raises(DmdxError, match="device tensor"):
        kern.row_mask_apply_(X.cpu(), cnt)
    with pytest.raises(DmdxError, match="length 8"):
        kern.row_mask_apply_(X, torch.zeros(9, dtype=torch.int32, device=DEV))
    with pytest.raises(DmdxError, match="int32"):
        kern.row_mask_apply_(X, cnt.cpu())
    with pytest.raises(DmdxError, match="int32"):
        kern.row_mask_apply_(X, cnt.float())
    assert not X.any() and not cnt.any()
