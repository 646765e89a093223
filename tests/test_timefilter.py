"""dmd_era5_amd/timefilter.py on the host: the tap design against its closed-form properties, the stamps of the outputs,
every ValueError, the NetCDF round trip, and tests/tfilt_ref.py (the arithmetic contract of K22) against two
independent evaluations.  The device side is tests/test_gpu_tfilt.py and tests/test_gpu_timefilter.py."""
import math

import numpy as np
import pytest
import torch

import tfilt_ref as fr
from dmd_era5_amd import io_netcdf
from dmd_era5_amd.timefilter import TimeFilter, boxcar, lanczos_bandpass, lanczos_lowpass, response

EPS = 2.0 ** -52
# (f_c, n): hourly data with a 10-day cut-off, daily data ... ; the first two have f_c n = 2
DESIGNS = [(1.0 / 240.0, 480), (1.0 / 24.0, 48), (1.0 / 10.0, 30)]


def _hourly(start, n, step_h=1):
    return np.datetime64(start, "h") + np.arange(n) * np.timedelta64(step_h, "h")


class HostKernels:
    """``HipKernels.tfilt`` on CPU tensors through the host definition: what TimeFilter.apply needs of a provider."""

    name = "host"

    def __init__(self):
        self.calls = []

    def tfilt(self, Xt, h, stride=1, out=None):
        self.calls.append((tuple(Xt.shape), int(h.shape[0]), int(stride)))
        Y = torch.from_numpy(np.ascontiguousarray(fr.tfilt(Xt.numpy().T, h.numpy(), stride).T))
        if out is None:
            return Y
        out.copy_(Y)
        return out


# ---------------------------------------------------------------- taps
def test_taps_symmetry_and_sums():
    for L in (1, 2, 24, 25):
        b = boxcar(L)
        assert b.shape == (L,) and (b == 1.0 / L).all()
        assert response(b, 0.0) == np.sum(b)
        if L > 1:
            assert (response(b, np.arange(1, L) / L) < 1e-12).all()
    for fc, n in DESIGNS:
        lo = lanczos_lowpass(fc, n)
        L = 2 * n + 1
        assert lo.shape == (L,) and lo.dtype == np.float64
        assert np.array_equal(lo.view(np.uint64), lo[::-1].view(np.uint64))        # symmetric to the bit
        assert abs(math.fsum(lo) - 1.0) <= L * EPS
        assert response(lo, 0.0) == np.sum(lo)
        bp = lanczos_bandpass(fc / 4.0, fc, n)
        assert np.array_equal(bp.view(np.uint64), bp[::-1].view(np.uint64))
        assert abs(math.fsum(bp)) <= L * EPS
        assert response(bp, 0.0) == abs(np.sum(bp))
        assert np.array_equal(bp, lanczos_lowpass(fc, n) - lanczos_lowpass(fc / 4.0, n))
    # w_0 = 2 f_c and the Duchon weights before the normalisation, for one small case by hand
    fc, n = 0.1, 3
    k = np.arange(-n, n + 1, dtype=np.float64)
    with np.errstate(all="ignore"):
        raw = np.where(k == 0, 2 * fc, np.sin(2 * np.pi * fc * k) / (np.pi * k) * np.sin(np.pi * k / n) / (np.pi * k / n))
    assert np.allclose(lanczos_lowpass(fc, n), raw / raw.sum(), rtol=0, atol=4 * EPS)
    for bad in (dict(cutoff=0.0, half_width=3), dict(cutoff=0.5, half_width=3), dict(cutoff=0.1, half_width=0)):
        with pytest.raises(ValueError):
            lanczos_lowpass(**bad)
    with pytest.raises(ValueError):
        lanczos_bandpass(0.2, 0.1, 5)
    with pytest.raises(ValueError):
        boxcar(0)


@pytest.mark.parametrize("fc,n", DESIGNS)
def test_lanczos_response_bounds(fc, n):
    taps = lanczos_lowpass(fc, n)
    f_pass = np.linspace(0.0, fc - 1.0 / n, 200)
    f_stop = np.linspace(fc + 1.0 / n, 0.5, 400)
    r_pass, r_stop, r_c = response(taps, f_pass), response(taps, f_stop), float(response(taps, fc))
    print(f"f_c = {fc:.5f} n = {n}: pass {r_pass.min():.4f} .. {r_pass.max():.4f}, stop <= {r_stop.max():.4f}, at f_c {r_c:.4f}")
    assert r_pass.min() >= 0.99 and r_pass.max() <= 1.01
    assert r_stop.max() <= 0.01
    assert 0.49 <= r_c <= 0.51


# ---------------------------------------------------------------- stamps
def test_n_out_and_times_out():
    times = _hourly("2020-01-01T00", 100)
    tf = TimeFilter(boxcar(24), 24, "left")
    assert tf.n_out(100) == 4 and tf.n_out(24) == 1 and tf.n_out(47) == 1 and tf.n_out(48) == 2
    assert np.array_equal(tf.times_out(times), _hourly("2020-01-01T00", 4, 24))
    tc = TimeFilter(lanczos_lowpass(0.1, 4), 5, "center")                           # L = 9, windows at 0, 5, ..., 90
    assert tc.n_out(100) == 19 and tc.n_out(9) == 1
    assert np.array_equal(tc.times_out(times), _hourly("2020-01-01T04", 19, 5))
    assert np.array_equal(TimeFilter(lanczos_lowpass(0.1, 4), 5, "left").times_out(times), _hourly("2020-01-01T00", 19, 5))
    assert TimeFilter([1.0], 1).n_out(7) == 7
    assert np.array_equal(TimeFilter([1.0], 3).times_out(times[:7]), times[:7:3])
    assert tc.times_out(times).dtype == np.dtype("datetime64[ns]")


def test_value_errors():
    times = _hourly("2020-01-01T00", 100)
    tf = TimeFilter(boxcar(25), 1, "center")
    uneven = times.copy()
    uneven[50:] += np.timedelta64(1, "h")
    nat = times.copy()
    nat[3] = np.datetime64("NaT")
    kern = HostKernels()
    X = [torch.zeros((100, 3)), torch.zeros((100, 2))]
    for bad, what in ((uneven, "evenly spaced"), (nat, "NaT"), (times[::-1], "evenly spaced"), (np.arange(100), "datetime64")):
        with pytest.raises(ValueError, match=what):
            tf.times_out(bad)
        with pytest.raises(ValueError, match=what):
            TimeFilter(boxcar(25), 1, "center", kern).apply(X, bad)
        with pytest.raises(ValueError, match=what):
            TimeFilter.block_mean(bad)
        with pytest.raises(ValueError, match=what):
            TimeFilter.lowpass(bad, 1.0)
    with pytest.raises(ValueError, match="odd number of taps"):
        TimeFilter(boxcar(24), 24, "center")
    with pytest.raises(ValueError, match="label"):
        TimeFilter(boxcar(3), 1, "right")
    with pytest.raises(ValueError, match="stride"):
        TimeFilter(boxcar(3), 0)
    with pytest.raises(ValueError, match="taps"):
        TimeFilter([])
    with pytest.raises(ValueError, match="taps"):
        TimeFilter([1.0, np.nan, 1.0])
    # T < L
    with pytest.raises(ValueError, match="fewer than the 25 taps"):
        tf.n_out(24)
    with pytest.raises(ValueError, match="fewer than the 25 taps"):
        tf.times_out(times[:24])
    with pytest.raises(ValueError, match="fewer than the 25 taps"):
        TimeFilter(boxcar(25), 1, "center", kern).apply([torch.zeros((24, 3))])
    # a period the step does not divide; a start off the period boundary
    with pytest.raises(ValueError, match="does not divide"):
        TimeFilter.block_mean(_hourly("2020-01-01T00", 40, 5))
    with pytest.raises(ValueError, match="does not divide"):
        TimeFilter.block_mean(_hourly("2020-01-01T00", 40, 48))
    with pytest.raises(ValueError, match="boundary"):
        TimeFilter.block_mean(_hourly("2020-01-01T06", 100))
    with pytest.raises(ValueError, match="boundary"):
        TimeFilter.block_mean(_hourly("2020-01-02T00", 100), days=5.0)             # 18 263 days after 1970-01-01
    # decimation that aliases the pass band
    with pytest.raises(ValueError, match="Nyquist"):
        TimeFilter.lowpass(times, cutoff_days=2.0, every_days=1.5)
    with pytest.raises(ValueError, match="Nyquist"):
        TimeFilter.bandpass(times, 2.0, 10.0, every_days=2.0)
    with pytest.raises(ValueError, match="does not divide"):
        TimeFilter.lowpass(times, cutoff_days=2.0, every_days=0.03)
    with pytest.raises(ValueError):
        TimeFilter.bandpass(times, 10.0, 2.0)
    # block shapes, before any launch
    with pytest.raises(ValueError, match="block 1 holds 99"):
        TimeFilter(boxcar(25), 1, "center", kern).apply([X[0], X[1][:99]], times)
    with pytest.raises(ValueError, match=r"out\[1\]"):
        TimeFilter(boxcar(25), 1, "center", kern).apply(X, times, out=[torch.zeros((76, 3)), torch.zeros((75, 2))])
    assert kern.calls == []


def test_constructors_in_physical_units():
    times = _hourly("2020-01-01T00", 24 * 60)
    bm = TimeFilter.block_mean(times)
    assert (bm.n_taps, bm.stride, bm.label) == (24, 24, "left") and np.array_equal(bm.taps, boxcar(24))
    assert TimeFilter.block_mean(_hourly("2020-01-01T00", 50, 6)).n_taps == 4
    assert TimeFilter.block_mean(_hourly("1970-01-06T00", 500), days=5.0).stride == 120
    lp = TimeFilter.lowpass(times, cutoff_days=10.0, every_days=1.0)
    assert (lp.n_taps, lp.stride, lp.label) == (961, 24, "center")
    assert np.array_equal(lp.taps, lanczos_lowpass(1.0 / 240.0, 480))
    assert TimeFilter.lowpass(times, 10.0).stride == 1
    assert TimeFilter.lowpass(times, 10.0, width_days=5.0, every_days=5.0).n_taps == 241
    bp = TimeFilter.bandpass(_hourly("2020-01-01T00", 900, 24), 20.0, 100.0, every_days=5.0)
    assert (bp.n_taps, bp.stride) == (401, 5)
    assert np.array_equal(bp.taps, lanczos_bandpass(1.0 / 100.0, 1.0 / 20.0, 200))
    r = bp.response([0.0, 1.0 / 45.0, 1.0 / 4.0])
    assert r[0] < 1e-12 and 0.99 < r[1] < 1.01 and r[2] < 0.01


def test_apply_through_a_host_provider():
    times = _hourly("2020-01-01T00", 60)
    rs = np.random.RandomState(0)
    X = [torch.from_numpy(rs.standard_normal((60, r)).astype(np.float32)) for r in (5, 3)]
    kern = HostKernels()
    tf = TimeFilter(lanczos_lowpass(0.1, 6), 4, "center", kern)
    Y, t_out = tf.apply(X, times)
    assert kern.calls == [((60, 5), 13, 4), ((60, 3), 13, 4)]
    assert np.array_equal(t_out, _hourly("2020-01-01T06", 12, 4))
    for x, y in zip(X, Y):
        assert y.shape == (12, x.shape[1])
        assert np.array_equal(y.numpy().T, fr.tfilt(x.numpy().T, tf.taps, 4))
    out = [torch.zeros((12, 5)), torch.zeros((12, 3))]
    Y2, none = tf.apply(iter(X), out=out)
    assert none is None and all(a is b for a, b in zip(Y2, out)) and all(torch.equal(a, b) for a, b in zip(Y, Y2))


def test_dataset_round_trip(tmp_path):
    tf = TimeFilter.lowpass(_hourly("2020-01-01T00", 200), cutoff_days=2.0, every_days=0.5)
    ds = tf.to_dataset()
    assert ds["filter_taps"].dims == ("tap",) and ds["filter_taps"].shape == (193,)
    path = str(tmp_path / "filter.nc")
    io_netcdf.to_netcdf(ds, path)
    back = TimeFilter.from_dataset(io_netcdf.open_dataset(path))
    assert np.array_equal(back.taps.view(np.uint64), tf.taps.view(np.uint64))
    assert (back.stride, back.label) == (12, "center")
    left = TimeFilter.from_dataset(TimeFilter(boxcar(24), 24, "left").to_dataset())
    assert (left.n_taps, left.stride, left.label) == (24, 24, "left")


# ---------------------------------------------------------------- the host definition
def test_ref_exact_on_integers():
    """Integer X in +-100 with taps on the grid of 2^-10 in +-1/16: every product and every partial sum is an integer
    multiple of 2^-10 below 25 * 100 * 64 < 2^18 of them, so the fp64 chain is exact, fits fp32 and equals an int64
    evaluation."""
    rs = np.random.RandomState(3)
    m, T = 7, 90
    Xi = rs.randint(-100, 101, (m, T)).astype(np.int64)
    for L, stride in ((1, 1), (2, 1), (3, 5), (24, 24), (25, 3)):
        hi = rs.randint(-64, 65, L).astype(np.int64)
        n = (T - L) // stride + 1
        want = np.zeros((m, n), dtype=np.int64)
        for u in range(n):
            for j in range(L):
                want[:, u] += Xi[:, u * stride + j] * hi[j]
        got = fr.tfilt(Xi.astype(np.float32), hi.astype(np.float64) / 1024.0, stride)
        assert got.shape == (m, n) and fr.n_out(T, L, stride) == n
        assert np.array_equal(got.astype(np.float64) * 1024.0, want.astype(np.float64))
    # fewer outputs than the snapshots allow; no window at all
    h = np.array([0.5, 0.25])
    assert np.array_equal(fr.tfilt(Xi.astype(np.float32), h, 3, T_out=4), fr.tfilt(Xi.astype(np.float32), h, 3)[:, :4])
    assert fr.tfilt(Xi[:, :1].astype(np.float32), h).shape == (m, 0) and fr.n_out(1, 2) == 0


def test_ref_daily_mean_against_reshape_mean():
    rs = np.random.RandomState(4)
    m, days = 11, 6
    X = (250.0 + 30.0 * rs.standard_normal((m, 24 * days))).astype(np.float32)
    got = fr.tfilt(X, boxcar(24), 24)
    want = X.astype(np.float64).reshape(m, days, 24).mean(axis=2)
    # fp64 sums of 24 values err far below the rounding to fp32: half an ulp of the mean, and as much again for a
    # mean that sits next to a rounding boundary
    assert np.abs(got.astype(np.float64) - want).max() <= 2.0 ** -23 * np.abs(X).max()
