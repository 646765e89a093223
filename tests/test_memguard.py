"""Self-test of tests/memguard.py on CPU tensors: the layout is what was asked for, a stray write
into each region is caught and named, and an element that was never written is caught."""
import numpy as np
import pytest
import torch

import memguard as mg


@pytest.mark.parametrize("dtype,isz", [(torch.float32, 4), (torch.float64, 8)])
@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_layout_offsets_and_alignment(dtype, isz, off):
    rows, cols, ld = 37, 5, 44
    view, h = mg.guarded(rows, cols, ld, dtype, base_offset_elems=off, device="cpu")
    assert tuple(view.shape) == (cols, rows) and tuple(view.stride()) == (ld, 1)
    assert view.data_ptr() == h.ptr and h.col_ptr(2) == h.ptr + 2 * ld * isz
    assert (h.ptr - off * isz) % 16 == 0 and h.ptr % 16 == (off * isz) % 16
    # guard sizes: >= 64 KiB in front, >= 128 columns + 4096 elements behind
    assert h.start * isz >= 64 * 1024 and h.back >= 128 * ld + 4096
    assert h.start + h.region + h.back == h.ibuf.numel() and h.region == cols * ld
    # every element starts as the canary, a quiet NaN with a fixed payload
    canary = mg.CANARY32 if dtype == torch.float32 else mg.CANARY64
    assert bool((h.ibuf == canary).all()) and bool(torch.isnan(h.fbuf).all())
    bits = np.array([canary], dtype=np.uint32 if isz == 4 else np.uint64)
    assert np.isnan(bits.view(np.float32 if isz == 4 else np.float64)[0])
    mg.assert_untouched(h)


def test_large_leading_dimension_gets_the_small_back_guard():
    _, h = mg.guarded(3, 1, 2**20, torch.float32, device="cpu")       # 128 columns would be 512 MiB
    assert h.back * 4 >= 2**20 and h.back * 4 < 2 * 2**20 + 64


def test_fill_writes_logical_elements_only_and_roundtrips():
    rs = np.random.RandomState(0)
    a = rs.standard_normal((37, 5)).astype(np.float32)
    view, h = mg.guarded(37, 5, 44, torch.float32, base_offset_elems=1, device="cpu")
    mg.fill(view, a)
    assert np.array_equal(h.logical(), a) and np.array_equal(view.numpy(), a.T)
    mg.assert_untouched(h)
    mg.assert_fully_written(h)
    h.snapshot()
    mg.assert_unchanged(h)
    view[3, 7] += 1.0
    with pytest.raises(AssertionError, match="input.*modified"):
        mg.assert_unchanged(h)
    with pytest.raises(ValueError):
        mg.fill(view, a.T)


def test_stray_write_into_each_region_is_caught_and_named():
    for region, where in (("front guard", lambda h: h.start - 1), ("front guard", lambda h: 0),
                          ("back guard", lambda h: h.start + h.region),
                          ("back guard", lambda h: h.ibuf.numel() - 1),
                          ("pad", lambda h: h.start + 2 * h.ld + h.rows),
                          ("pad", lambda h: h.start + h.region - 1)):
        view, h = mg.guarded(10, 4, 12, torch.float64, device="cpu")
        mg.fill(view, np.ones((10, 4)))
        mg.assert_untouched(h)
        h.fbuf[where(h)] = 0.0
        with pytest.raises(AssertionError, match=region) as e:
            mg.assert_untouched(h)
        assert str(where(h)) in str(e.value) or region == "front guard"


def test_nan_written_back_over_a_canary_is_caught():
    """x * 0 of a canary is a NaN again, but not the same bits: integer comparison sees it."""
    view, h = mg.guarded(10, 4, 12, torch.float32, device="cpu")
    mg.fill(view, 1.0)
    h.fbuf[h.start + 10] = -h.fbuf[h.start + 10]          # sign flip of the NaN in the pad
    with pytest.raises(AssertionError, match="pad.*column 0, row 10"):
        mg.assert_untouched(h)


def test_element_never_written_is_caught():
    view, h = mg.guarded(10, 4, 12, torch.float32, device="cpu")
    a = np.ones((10, 4), dtype=np.float32)
    mg.fill(view, a)
    view[2, 9] = h.fbuf[0]                                 # the canary again
    with pytest.raises(AssertionError, match=r"row 9, column 2.*never written"):
        mg.assert_fully_written(h)


def test_overlapping_delay_view_has_no_pad():
    view, h = mg.guarded(30, 4, 10, torch.float32, device="cpu")       # rows > ld
    assert h.region == 3 * 10 + 30 and tuple(view.stride()) == (10, 1)
    h.fbuf[h.start:h.start + h.region] = 2.0
    mg.assert_untouched(h)
    h.fbuf[h.start + h.region] = 2.0
    with pytest.raises(AssertionError, match="back guard"):
        mg.assert_untouched(h)


@pytest.mark.parametrize("nbytes", [0, 1, 100, 4096, 131072 + 8])
def test_exact_workspace(nbytes):
    ws = mg.exact_workspace(nbytes, device="cpu")
    assert ws.ptr % 16 == 0 and ws.nbytes == nbytes
    use = ws.buf[ws.start:ws.start + nbytes]
    assert bool((use == 0xFF).all())
    if nbytes >= 8:
        assert bool(torch.isnan(use[:nbytes // 8 * 8].view(torch.float64)).all())
    mg.assert_untouched(ws)
    ws.check_unused()
    if nbytes:
        use[nbytes - 1] = 0                                 # the last usable byte is the caller's
        mg.assert_untouched(ws)
        with pytest.raises(AssertionError, match="usable"):
            ws.check_unused()
    ws.buf[ws.start + nbytes] ^= 1                          # the first byte behind it is not
    with pytest.raises(AssertionError, match="back guard.*0 bytes past"):
        mg.assert_untouched(ws)
    ws = mg.exact_workspace(nbytes, device="cpu")
    ws.buf[ws.start - 1] ^= 1
    with pytest.raises(AssertionError, match="front guard"):
        mg.assert_untouched(ws)
