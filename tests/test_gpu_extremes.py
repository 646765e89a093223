"""The host layer of K29 on the HIP provider: PeriodStats.fit on device blocks equals tests/pstat_ref.py bit for bit --
on hourly stamps across two year boundaries with a per-row threshold table, with an ``out`` tensor that is written in
place, and after a NetCDF round trip onto the device."""
import numpy as np
import pytest
import torch

import pstat_ref as pr
from pstat_ref import PstatDouble

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROWS = (515, 1029)


def _t(a, dtype=torch.float32, device="cpu"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(device)


@pytest.fixture(scope="module")
def hip():
    from dmd_era5_amd.kernels import default_kernels

    return default_kernels()


def _same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


def _hourly_over_two_new_years():
    """Hourly stamps of two years cut down to 300 snapshots: 2019-12-27T00 .. (120 h in 2019), then 2021-12-29T12 ..
    (60 h in 2021, 120 h in 2022): three periods of 5 days, 2.5 days and 5 days."""
    a = np.datetime64("2019-12-27T00", "h") + np.arange(120) * np.timedelta64(1, "h")
    b = np.datetime64("2021-12-29T12", "h") + np.arange(180) * np.timedelta64(1, "h")
    return np.concatenate([a, b])


def _blocks(rs, T):
    X = [(280.0 + np.round(8.0 * rs.standard_normal((T, mb)).cumsum(axis=0) / np.sqrt(np.arange(1, T + 1))[:, None]) / 4)
         .astype(np.float32) for mb in ROWS]
    X[0][7, 3], X[1][50, 11], X[1][T - 1, 0] = np.nan, np.inf, -np.inf
    X[1][120:180, 5] = np.nan                                                # no valid day in 2021
    return X


def test_fit_on_device_blocks_equals_the_reference(hip):
    from dmd_era5_amd.extremes import SEGMENT, PeriodStats

    rs = np.random.RandomState(29)
    times = _hourly_over_two_new_years()
    T = times.shape[0]
    X = _blocks(rs, T)
    Xd = [_t(x, device=DEV) for x in X]
    thr = [np.float32(280.0) + np.round(rs.standard_normal(mb) * 4).astype(np.float32) / 4 for mb in ROWS]
    thr[0][9] = np.nan
    w = [(0.1 + rs.rand(mb)).astype(np.float32) for mb in ROWS]
    w[0][5] = 0.0
    lab = [np.sort(rs.randint(0, 3, mb)) for mb in ROWS]
    for kw in (dict(group=24, inner="max", window=1), dict(group=24, inner="mean", window=2, min_count=20, below=True),
               dict(group=6, inner="range", window=5, inclusive=True), dict(group=1, inner="sum", window=8, min_count=1)):
        got = PeriodStats.fit(Xd, times, threshold=[_t(h, device=DEV) for h in thr], kern=hip, **kw)
        want = PeriodStats.fit([_t(x) for x in X], times, threshold=[_t(h) for h in thr], kern=PstatDouble(), **kw)
        assert got.bounds.tolist() == [0, 120, 180, 300] and got.labels.tolist() == ["2019", "2021", "2022"]
        for P, Q, x, h in zip(got.planes, want.planes, X, thr):
            assert P.is_cuda and P.dtype == torch.float64 and P.shape == (8, 3, x.shape[1])
            assert _same(P.cpu().numpy(), Q.numpy())
            ref = pr.period_stats(x.T, [0, 120, 180, 300], kw["group"], kw["inner"], kw["window"], kw.get("min_count"), h,
                                  kw.get("below", False), kw.get("inclusive", False), SEGMENT)
            assert _same(P.cpu().numpy(), ref)
        n = torch.cat([q.cpu() for q in got.n_valid()], dim=1)
        assert int(n.min()) == 0 and int(n.max()) >= 2
        for name in ("maximum", "minimum", "total", "total_beyond", "count_beyond", "mean", "intensity", "fraction_beyond",
                     "when_max", "when_min"):
            for g, h in zip(getattr(got, name)(), getattr(want, name)()):
                assert _same(g.cpu().numpy(), h.numpy()), name
            a = got.area_mean(name, weights=[_t(v, device=DEV) for v in w], groups=[_t(v, torch.int64) for v in lab])
            b = want.area_mean(name, weights=[_t(v) for v in w], groups=[_t(v, torch.int64) for v in lab])
            for key in ("mean", "weight", "rows"):
                assert np.array_equal(a[key].numpy(), b[key].numpy(), equal_nan=True), (name, key)
        for g, h in zip(got.when_max(as_time=True), want.when_max(as_time=True)):
            assert np.array_equal(g, h, equal_nan=True)
        for g, h in zip(got.series("maximum"), want.series("maximum")):
            assert g.is_cuda and g.dtype == torch.float32 and _same(g.cpu().numpy(), h.numpy())


def test_an_out_tensor_is_written_in_place_and_bad_arguments_are_refused_before_a_launch(hip):
    from dmd_era5_amd._lib import DmdxError

    rs = np.random.RandomState(3)
    T, mb = 300, 131
    x = _blocks(rs, T)[0][:, :mb].copy()
    X, thr = _t(x, device=DEV), torch.full((mb,), 281.0, device=DEV)
    out = torch.full((8, 2, mb), -7.0, dtype=torch.float64, device=DEV)
    for seg in (1, 3, 32, T):
        want = pr.period_stats(x.T, [0, 100, T], 6, "max", 2, 5, np.full(mb, 281.0, dtype=np.float32), False, False, seg)
        got = hip.period_stats(X, [0, 100, T], group=6, inner="max", window=2, min_count=5, thr=thr, seg=seg, out=out)
        assert got.data_ptr() == out.data_ptr() and _same(out.cpu().numpy(), want)
    # a row-strided view of the snapshots is read as it is
    wide = torch.zeros((T, mb + 5), device=DEV)
    wide[:, :mb] = X
    assert _same(hip.period_stats(wide[:, :mb], [0, 100, T], group=6, inner="max", window=2, min_count=5, thr=thr, seg=T)
                 .cpu().numpy(), want)
    out.fill_(-7.0)
    good = dict(bounds=[0, 100, T], group=6, inner="max", window=2, min_count=5, thr=thr, seg=32)
    for bad in (dict(bounds=[0, 100, T + 1]), dict(bounds=[5, 5, 9]), dict(bounds=[0, 100, 2 ** 32 + 5]), dict(bounds=[0, T]),
                dict(group=0), dict(inner="median"), dict(window=0), dict(window=9), dict(min_count=0), dict(min_count=7),
                dict(seg=0), dict(thr=thr[:-1]), dict(thr=thr.double()), dict(thr=thr.cpu())):
        with pytest.raises(DmdxError):
            hip.period_stats(X, out=out, **{**good, **bad})
    assert bool((out == -7.0).all())


@pytest.mark.skipif(not __import__("dmd_era5_amd.hdf5_lite", fromlist=["x"]).available(), reason="libhdf5 not found")
def test_from_dataset_puts_the_planes_on_the_device(hip, tmp_path):
    from dmd_era5_amd import io_netcdf
    from dmd_era5_amd.extremes import PeriodStats

    rs = np.random.RandomState(4)
    times = _hourly_over_two_new_years()
    X = _blocks(rs, times.shape[0])
    st = PeriodStats.fit([_t(x, device=DEV) for x in X], times, group=24, inner="sum", window=2, threshold=280.0 * 48, kern=hip)
    path = str(tmp_path / "extremes.nc")
    io_netcdf.to_netcdf(st.to_dataset(), path)
    back = PeriodStats.from_dataset(io_netcdf.open_dataset(path), rows=ROWS, kern=hip)
    assert (back.group, back.inner, back.window, back.min_count, back.has_threshold) == (24, "sum", 2, 24, True)
    assert back.labels.tolist() == ["2019", "2021", "2022"] and np.array_equal(back.times, st.times)
    for P, Q in zip(back.planes, st.planes):
        assert P.is_cuda and P.dtype == torch.float64 and _same(P.cpu().numpy(), Q.cpu().numpy())
    for a, b in zip(back.when_max(as_time=True), st.when_max(as_time=True)):
        assert np.array_equal(a, b, equal_nan=True)
    assert int(torch.cat([q.cpu() for q in back.count_beyond()], dim=1).max()) >= 1
