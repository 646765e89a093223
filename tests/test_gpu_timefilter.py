"""dmd_era5_amd/timefilter.py on the device: TimeFilter.apply over a list of row blocks against tests/tfilt_ref.py bit for
bit, the daily mean against the fp64 reshape-mean, and a decimating low-pass on a two-tone series against the bounds
its own response gives."""
import numpy as np
import pytest
import torch

import tfilt_ref as fr
from dmd_era5_amd.timefilter import TimeFilter, lanczos_lowpass

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _hourly(start, n, step_h=1):
    return np.datetime64(start, "h") + np.arange(n) * np.timedelta64(step_h, "h")


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32).view(np.uint32)


def _blocks(T, rows, seed=0):
    rs = np.random.RandomState(seed)
    host = [(250.0 + 30.0 * rs.standard_normal((T, r))).astype(np.float32) for r in rows]
    return host, [torch.from_numpy(h).to(DEV) for h in host]


def test_apply_on_two_blocks_of_unequal_width():
    T, rows = 200, (1027, 5)
    times = _hourly("2020-01-01T00", T)
    host, X = _blocks(T, rows)
    tf = TimeFilter(lanczos_lowpass(0.05, 12), 3, "center")                          # L = 25: 59 windows
    want = [fr.tfilt(h.T, tf.taps, 3).T for h in host]
    Y, t_out = tf.apply(X, times)
    assert np.array_equal(t_out, _hourly("2020-01-01T12", 59, 3))
    for y, w, r in zip(Y, want, rows):
        assert y.shape == (59, r) and y.dtype == torch.float32 and y.is_contiguous()
        assert np.array_equal(_bits(y), w.view(np.uint32))
    # into views with a row stride; a generator of blocks; no stamps
    bufs = [torch.full((59, r + 3), 7.0, dtype=torch.float32, device=DEV) for r in rows]
    out = [b[:, :r] for b, r in zip(bufs, rows)]
    Y2, none = tf.apply((x for x in X), out=out)
    assert none is None
    for y, o, b, w, r in zip(Y2, out, bufs, want, rows):
        assert y.data_ptr() == o.data_ptr()
        assert np.array_equal(_bits(o), w.view(np.uint32)) and bool((b[:, r:] == 7.0).all())
    for x, h in zip(X, host):
        assert np.array_equal(_bits(x), h.view(np.uint32))                           # the input is left alone
    # a strided input block: every other snapshot of a buffer twice as long
    wide = torch.from_numpy(np.ascontiguousarray(np.repeat(host[1], 2, axis=0))).to(DEV)
    Y3, _ = tf.apply([wide[::2]])
    assert np.array_equal(_bits(Y3[0]), want[1].view(np.uint32))
    # checked before any launch: a block of another length, a wrong out
    with pytest.raises(ValueError, match="block 1"):
        tf.apply([X[0], X[1][:150]], times)
    with pytest.raises(ValueError, match=r"out\[0\]"):
        tf.apply(X, times, out=[out[0][:58], out[1]])


def test_wrapper_checks_and_timing_record():
    from dmd_era5_amd._lib import DmdxError
    from dmd_era5_amd.kernels import HipKernels

    kern = HipKernels()
    assert kern.tfilt_max_taps >= 2048
    X = torch.zeros((10, 7), dtype=torch.float32, device=DEV)
    h = torch.full((4,), 0.25, dtype=torch.float64, device=DEV)
    for bad in (lambda: kern.tfilt(X[:3], h),                                        # T < L
                lambda: kern.tfilt(X, h.float()), lambda: kern.tfilt(X, h.cpu()), lambda: kern.tfilt(X, h[::2]),
                lambda: kern.tfilt(X, h, 0), lambda: kern.tfilt(X.double(), h), lambda: kern.tfilt(X, h.reshape(2, 2)),
                lambda: kern.tfilt(X, torch.zeros(kern.tfilt_max_taps + 1, dtype=torch.float64, device=DEV)),
                lambda: kern.tfilt(X, h, 3, out=torch.zeros((2, 7), dtype=torch.float32, device=DEV)),
                lambda: kern.tfilt(X, h, out=X[:7])):                                # overlap: refused by the library
        with pytest.raises(DmdxError):
            bad()
    kern.events = []
    Y = kern.tfilt(X, h, 3)
    assert Y.shape == (3, 7) and bool((Y == 0).all())
    assert [(n, s) for n, s, _, _ in kern.events] == [("tfilt", (7, 10, 4, 3))]


def test_block_mean_of_four_days():
    T, rows = 96, (1027, 5)
    times = _hourly("2021-03-01T00", T)
    host, X = _blocks(T, rows, seed=1)
    tf = TimeFilter.block_mean(times)
    Y, t_out = tf.apply(X, times)
    assert np.array_equal(t_out, _hourly("2021-03-01T00", 4, 24))
    for y, h in zip(Y, host):
        want = h.astype(np.float64).reshape(4, 24, -1).mean(axis=1)
        assert y.shape == want.shape
        assert np.abs(y.cpu().numpy().astype(np.float64) - want).max() <= 2.0 ** -23 * np.abs(h).max()
        assert np.array_equal(_bits(y), fr.tfilt(h.T, tf.taps, 24).T.view(np.uint32))


def test_lowpass_keeps_the_slow_tone_and_removes_the_fast_one():
    """Hourly stamps, a 2-day low-pass (f_c = 1 / 48, n = 96, L = 193) with daily output.  Per row a slow tone (period
    8 days, f = 1 / 192 <= f_c - 1 / n) and a fast one (12 hours, f = 1 / 12 >= f_c + 1 / n) of its own amplitudes and
    phases.  The taps are symmetric, so a tone of frequency f comes out at the window's centre with its phase and the
    amplitude response(f): the output differs from the slow tone by at most a |1 - response(f_slow)| +
    b response(f_fast), plus 2^-22 (a + b) for the roundings (the fp32 input: 2^-24 |x| under taps with
    sum |h| < 2; the fp32 output: 2^-24 |y|; the fp64 chain is far below both)."""
    T, m = 24 * 30, 37
    times = _hourly("2022-06-01T00", T)
    tf = TimeFilter.lowpass(times, cutoff_days=2.0, every_days=1.0)
    assert (tf.n_taps, tf.stride) == (193, 24) and np.abs(tf.taps).sum() < 2.0
    f_slow, f_fast = 1.0 / 192.0, 1.0 / 12.0
    r_slow, r_fast = float(tf.response(f_slow)), float(tf.response(f_fast))
    assert abs(1.0 - r_slow) <= 0.01 and r_fast <= 0.01
    rs = np.random.RandomState(5)
    a, b = rs.uniform(1.0, 20.0, m), rs.uniform(1.0, 20.0, m)
    pa, pb = rs.uniform(0.0, 2.0 * np.pi, m), rs.uniform(0.0, 2.0 * np.pi, m)
    t = np.arange(T, dtype=np.float64)[:, None]
    slow = a * np.cos(2.0 * np.pi * f_slow * t + pa)
    fast = b * np.cos(2.0 * np.pi * f_fast * t + pb)
    centre = 96 + 24 * np.arange(tf.n_out(T))
    X = [torch.from_numpy(s.astype(np.float32)).to(DEV) for s in (slow + fast, slow, fast)]
    (both, only_slow, only_fast), t_out = tf.apply(X, times)
    assert np.array_equal(t_out, times[centre])
    both, only_slow, only_fast = (y.cpu().numpy().astype(np.float64) for y in (both, only_slow, only_fast))
    rnd = 2.0 ** -22
    err = np.abs(only_slow - slow[centre])
    print("slow tone kept:   worst error / bound", (err / (a * (abs(1.0 - r_slow) + rnd))).max())
    assert (err <= a * (abs(1.0 - r_slow) + rnd)).all()
    print("fast tone removed: worst |y| / bound ", (np.abs(only_fast) / (b * (r_fast + rnd))).max())
    assert (np.abs(only_fast) <= b * (r_fast + rnd)).all()
    err = np.abs(both - slow[centre])
    assert (err <= a * abs(1.0 - r_slow) + b * r_fast + rnd * (a + b)).all()
    # ... where sub-sampling the same snapshots keeps the fast tone at its full amplitude
    assert np.abs((slow + fast)[centre] - slow[centre]).max() > 0.5 * b.min()
