"""Host side of K21 without a GPU: design against a per-stamp loop over datetime objects, and Trend /
DmdForecast(trend=) on a kernel double whose two treg methods are tests/treg_ref.py, the host definition."""
import datetime as dt
import math

import numpy as np
import pytest
import torch

import clim_ref as cr
import treg_ref as tr
from test_climatology import ClimDouble


class TrendDouble(ClimDouble):
    """CpuKernelDouble + K18 + the two K21 methods of HipKernels, computed by treg_ref."""

    name = "cpu-double+clim+treg"
    fits = 0
    applies = 0

    def treg_fit(self, Xt, W, seg, out=None):
        type(self).fits += 1
        C = torch.from_numpy(tr.fit(Xt.numpy().T, W.numpy(), seg))
        if out is None:
            return C
        out.copy_(C)
        return out

    def treg_apply_(self, Xt, D, coef, restore=False, out=None):
        type(self).applies += 1
        Y = tr.apply(Xt.numpy().T, D.numpy(), coef.numpy(), restore)
        dst = Xt if out is None else out
        dst.copy_(torch.from_numpy(np.ascontiguousarray(Y.T)))
        return dst


def _bits(a):
    a = a.numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _hourly(start, n, step_h=1):
    return np.datetime64(start, "h") + np.arange(n) * np.timedelta64(step_h, "h")


# ---------------------------------------------------------------- design
def _design_by_hand(stamps, origin: dt.datetime, half, degree, harmonics, diurnal, period, extra):
    rows = []
    for i, s in enumerate(stamps):
        days = (s - origin) / dt.timedelta(days=1)
        row = [1.0] + [(days / half) ** q for q in range(1, degree + 1)]
        for h in range(1, harmonics + 1):
            row += [math.cos(2 * math.pi * h * days / period), math.sin(2 * math.pi * h * days / period)]
        for h in range(1, diurnal + 1):
            row += [math.cos(2 * math.pi * h * days), math.sin(2 * math.pi * h * days)]
        rows.append(row + ([] if extra is None else list(np.atleast_1d(extra[i]))))
    return np.array(rows, dtype=np.float64)


# 7-hourly over the leap day of 2020 and a year boundary, then a gap and 13-hourly stamps: uneven
TIMES = np.concatenate([_hourly("2019-12-20T00", 300, 7), _hourly("2020-06-01T05", 40, 13)])


@pytest.mark.parametrize("degree,harmonics,diurnal,nextra", [(0, 0, 0, 0), (1, 0, 0, 0), (3, 1, 1, 0), (1, 2, 0, 2), (0, 0, 2, 1)])
def test_design_equals_a_loop_over_datetime_objects(degree, harmonics, diurnal, nextra):
    from dmd_era5_amd.trend import design

    stamps = TIMES.astype("datetime64[s]").astype(dt.datetime)
    assert any((x.month, x.day) == (2, 29) for x in stamps)
    origin, half, period = np.datetime64("2020-03-01T06", "ns"), 90.25, 365.2425
    rs = np.random.RandomState(1)
    extra = None if nextra == 0 else rs.standard_normal((TIMES.shape[0], nextra))
    D = design(TIMES, origin, half, degree, harmonics, diurnal, period, None if extra is None else
               (extra[:, 0] if nextra == 1 else extra))
    p = 1 + degree + 2 * harmonics + 2 * diurnal + nextra
    assert D.dtype == np.float64 and D.shape == (TIMES.shape[0], p) and D.flags.c_contiguous
    want = _design_by_hand(stamps, dt.datetime(2020, 3, 1, 6), half, degree, harmonics, diurnal, period, extra)
    # days is one correctly rounded division both ways; the angle (up to 2 pi 2 x 165 days) carries a few ulps into
    # cos / sin, whose results are below 1: 1e-12 absolute; the powers of tau (|tau| < 2) are relative
    assert np.array_equal(D[:, 0], np.ones(TIMES.shape[0]))
    assert np.allclose(D[:, 1:1 + degree], want[:, 1:1 + degree], rtol=1e-14, atol=0)
    assert np.abs(D[:, 1 + degree:p - nextra] - want[:, 1 + degree:p - nextra]).max(initial=0) <= 1e-12
    if nextra:
        assert np.array_equal(D[:, p - nextra:], extra)


def test_design_value_errors():
    from dmd_era5_amd.trend import Trend, design, weights

    o = np.datetime64("2020-01-01", "ns")
    with pytest.raises(ValueError, match="at most 8"):
        design(TIMES, o, 10.0, degree=2, harmonics=2, diurnal=1)                     # 9 columns
    with pytest.raises(ValueError, match="at most 8"):
        design(TIMES, o, 10.0, degree=1, harmonics=1, extra=np.zeros((TIMES.shape[0], 5)))
    with pytest.raises(ValueError, match="datetime64"):
        design(np.arange(5), o, 10.0)
    with pytest.raises(ValueError, match="one row per time stamp"):
        design(TIMES, o, 10.0, extra=np.zeros(3))
    TrendDouble.fits = 0
    X = [torch.zeros((TIMES.shape[0], 3))]
    with pytest.raises(ValueError, match="condition number"):                         # a constant series next to the 1
        Trend.fit(X, TIMES, extra=np.full(TIMES.shape[0], 2.0), kern=TrendDouble())
    with pytest.raises(ValueError, match="condition number"):                         # more columns than snapshots
        Trend.fit([X[0][:3]], TIMES[:3], degree=3, kern=TrendDouble())
    with pytest.raises(ValueError, match="datetime64"):
        Trend.fit(X, np.arange(TIMES.shape[0]), kern=TrendDouble())
    with pytest.raises(ValueError, match="snapshots"):
        Trend.fit([X[0][:5]], TIMES, kern=TrendDouble())
    assert TrendDouble.fits == 0                                                      # all before any launch
    D = design(TIMES, o, 100.0, 1)
    assert np.allclose(weights(D) @ D, np.eye(2), rtol=0, atol=1e-12)


# ---------------------------------------------------------------- fit against lstsq
T1, M1 = 37, 2053


def _uneven(T=T1, days=800.0, seed=3):
    rs = np.random.RandomState(seed)
    hours = np.sort(rs.choice(int(days * 24), T, replace=False))
    hours[0], hours[-1] = 0, int(days * 24)
    return np.datetime64("2018-01-01T00", "h") + hours * np.timedelta64(1, "h")


_CASES = {1: dict(degree=0), 2: dict(degree=1), 3: dict(degree=0, harmonics=1), 5: dict(degree=0, harmonics=2),
          7: dict(degree=1, harmonics=2, extra=True)}


@pytest.fixture(scope="module")
def field():
    rs = np.random.RandomState(5)
    times = _uneven()
    tau = (times - times[0]).astype(np.float64) / (800.0 * 24) * 2 - 1
    X = 250.0 + 30.0 * rs.standard_normal((T1, M1)) + 5.0 * tau[:, None] * rs.standard_normal(M1)[None, :]
    return times, X.astype(np.float32), rs.standard_normal(T1)


@pytest.mark.parametrize("p", sorted(_CASES))
def test_fit_against_lstsq_in_fp64(field, p):
    from dmd_era5_amd.trend import SEGMENT, Trend

    times, X, enso = field
    kw = dict(_CASES[p])
    extra = enso if kw.pop("extra", False) else None
    cut = 1029
    trend = Trend.fit([torch.from_numpy(X[:, :cut].copy()), torch.from_numpy(X[:, cut:].copy())], times, extra=extra,
                      kern=TrendDouble(), **kw)
    assert SEGMENT == 1024 and trend.n_terms == p and [tuple(c.shape) for c in trend.coef] == [(p, cut), (p, M1 - cut)]
    assert trend.origin == times[0] + (times[-1] - times[0]) // 2 and trend.half_span_days == 400.0
    D = trend.design(times, extra)
    assert np.linalg.cond(D) <= 4.5
    W = tr.w_of(D)
    coef = np.concatenate([c.numpy() for c in trend.coef], axis=1)
    assert np.array_equal(_bits(coef), _bits(tr.fit(X.T, W, 1024)))                   # what the double computed
    X64 = X.astype(np.float64)
    c64 = np.linalg.lstsq(D, X64, rcond=None)[0]
    # one rounding to fp32 (2^-24) with a factor 2 for the fp64 difference between the QR route and lstsq, and the
    # sequential fp64 chain of T terms.  On these data (condition numbers 1.0 .. 2.5) the reference reaches 0.49 - 0.50
    # of the bound: the fp32 rounding is what is left.
    bound = 2.0 ** -23 * np.abs(c64) + T1 * 2.0 ** -52 * (np.abs(W) @ np.abs(X64))
    ratio = np.abs(coef.astype(np.float64) - c64) / bound
    print(f"p = {p}: cond = {np.linalg.cond(D):.3f}, worst |coef - lstsq| / bound = {ratio.max():.3f}")
    assert ratio.max() <= 1.0


def test_slope_of_a_planted_trend(field):
    from dmd_era5_amd.trend import Trend

    times, _, _ = field
    rs = np.random.RandomState(6)
    a, b = 280.0 + rs.standard_normal(M1), 0.8 * rs.standard_normal(M1)               # b: units per half span (400 days)
    tau = ((times - times[0]).astype("timedelta64[h]").astype(np.float64) / 24.0 - 400.0) / 400.0
    X = (a[None, :] + b[None, :] * tau[:, None] + 1e-3 * rs.standard_normal((T1, M1))).astype(np.float32)
    trend = Trend.fit([torch.from_numpy(X)], times, degree=1, kern=TrendDouble())
    D = trend.design(times)
    assert np.abs(D[:, 1] - tau).max() <= 2.0 ** -52             # |tau| <= 1: an ulp between two orders of the divisions
    W = tr.w_of(D)
    c64 = np.linalg.lstsq(D, X.astype(np.float64), rcond=None)[0]
    scale = 3652.425 / 400.0
    (slope,) = trend.slope()
    assert slope.dtype == torch.float64 and slope.shape == (M1,)
    bound = 2.0 ** -23 * np.abs(c64[1]) + T1 * 2.0 ** -52 * (np.abs(W[1]) @ np.abs(X.astype(np.float64)))
    # ... scaled, and one more fp64 rounding for the product with the scale
    assert (np.abs(slope.numpy() - c64[1] * scale) <= bound * scale + 2.0 ** -52 * np.abs(c64[1] * scale)).all()
    # the least-squares slope itself is the planted one up to the noise: sigma / sqrt(sum tau^2), 6 sigma of it
    assert (np.abs(c64[1] - b) <= 6 * 1.001e-3 / np.sqrt((tau * tau).sum() - tau.sum() ** 2 / T1)).all()
    (per_day,) = trend.slope(per_days=1.0)
    assert np.allclose(per_day.numpy() * 3652.425, slope.numpy(), rtol=1e-15, atol=0)
    with pytest.raises(ValueError, match="linear term"):
        Trend.fit([torch.from_numpy(X)], times, degree=0, kern=TrendDouble()).slope()


# ---------------------------------------------------------------- remove / restore / at on a 2-block toy grid
ROWS = (9, 4)


def _toy(T=60, seed=0, step_h=6):
    rs = np.random.RandomState(seed)
    times = _hourly("2020-03-01T00", T, step_h)
    ramp = np.linspace(-1.0, 1.0, T)
    X = [torch.from_numpy((rs.standard_normal((T, mb)) + 3.0 * ramp[:, None] * rs.standard_normal(mb)[None, :] + 280.0)
                          .astype(np.float32)) for mb in ROWS]
    return times, X


def test_remove_restore_at():
    from dmd_era5_amd.trend import Trend

    times, X = _toy()
    enso = np.cos(np.arange(60) / 7.0)
    trend = Trend.fit(X, times, degree=1, diurnal=1, extra=enso, kern=TrendDouble())
    D = trend.design(times, enso)
    assert D.shape == (60, 5)
    keep = [x.clone() for x in X]
    out = [torch.full_like(x, 7.0) for x in X]
    res = trend.remove_(X, times, out=out, extra=enso)
    assert all(r is o for r, o in zip(res, out)) and all(torch.equal(a, b) for a, b in zip(X, keep))
    trend.remove_(X, times, extra=enso)                          # in place
    for b in range(2):
        want = tr.apply(keep[b].numpy().T, D, trend.coef[b].numpy()).T
        assert np.array_equal(_bits(X[b]), _bits(want)) and torch.equal(X[b], out[b])
        assert np.abs(X[b].numpy()).max() < 10.0                 # the level and the ramp are gone
    trend.restore_(X, times, extra=enso)
    for b in range(2):
        anom = tr.apply(keep[b].numpy().T, D, trend.coef[b].numpy())
        want = tr.apply(anom, D, trend.coef[b].numpy(), restore=True).T
        assert np.array_equal(_bits(X[b]), _bits(want))          # the composition; no exact round trip is promised
    # .at beyond the fitted period: design(new) @ coef under the apply contract, restore on zeros
    later = _hourly("2031-07-04T05", 30, 5)
    enso2 = np.sin(np.arange(30) / 3.0)
    F = trend.at(later, extra=enso2)
    D2 = trend.design(later, enso2)
    assert D2[:, 1].min() > 100.0                                # tau far outside -1 .. 1
    for b in range(2):
        want = tr.apply(np.zeros((ROWS[b], 30), dtype=np.float32), D2, trend.coef[b].numpy(), restore=True).T
        assert F[b].shape == (30, ROWS[b]) and np.array_equal(_bits(F[b]), _bits(want))
        assert np.array_equal(want, tr.fitted(trend.coef[b].numpy(), D2).astype(np.float32).T)


def test_apply_value_errors_before_any_launch():
    from dmd_era5_amd.trend import Trend

    times, X = _toy()
    enso = np.cos(np.arange(60) / 7.0)
    trend = Trend.fit(X, times, degree=1, extra=enso, kern=TrendDouble())
    plain = Trend.fit(X, times, degree=1, kern=TrendDouble())
    TrendDouble.applies = 0
    with pytest.raises(ValueError, match="extra"):
        trend.remove_(X, times)                                  # fitted with a series, applied without
    with pytest.raises(ValueError, match="extra"):
        trend.at(times)
    with pytest.raises(ValueError, match="extra"):
        trend.remove_(X, times, extra=np.zeros((60, 2)))
    with pytest.raises(ValueError, match="extra"):
        plain.remove_(X, times, extra=enso)
    with pytest.raises(ValueError, match="one row per time stamp"):
        trend.remove_(X, times, extra=enso[:-1])
    with pytest.raises(ValueError, match="blocks"):
        plain.remove_(X[:1], times)
    with pytest.raises(ValueError, match="block 1"):
        plain.remove_([X[0], X[1][:, :-1]], times)
    with pytest.raises(ValueError, match="block 0"):
        plain.remove_(X, times[:-1])
    with pytest.raises(ValueError, match="datetime64"):
        plain.remove_(X, np.arange(60))
    assert TrendDouble.applies == 0


def test_dataset_round_trip_through_a_file(tmp_path):
    from dmd_era5_amd import io_netcdf
    from dmd_era5_amd.labeled import Coord
    from dmd_era5_amd.trend import Trend

    times, X = _toy(T=50, step_h=7)
    enso = np.cos(np.arange(50) / 7.0)
    trend = Trend.fit(X, times, degree=2, harmonics=1, diurnal=1, extra=enso, kern=TrendDouble())
    M = sum(ROWS)
    coords = {"space": Coord("space", np.arange(M, dtype=np.int64)),
              "latitude": Coord("space", np.linspace(-60.0, 60.0, M)), "time": Coord("time", times)}
    ds = trend.to_dataset(coords)
    assert ds["trend_coef"].dims == ("term", "space") and ds["trend_coef"].shape == (8, M) and "time" not in ds.coords
    path = str(tmp_path / "trend.nc")
    io_netcdf.to_netcdf(ds, path)
    back = Trend.from_dataset(io_netcdf.open_dataset(path), rows=ROWS, device="cpu", kern=TrendDouble())
    assert back.origin == trend.origin and back.half_span_days == trend.half_span_days
    assert (back.degree, back.harmonics, back.diurnal, back.n_extra, back.period_days) == (2, 1, 1, 1, 365.2425)
    for b in range(2):
        assert np.array_equal(_bits(back.coef[b]), _bits(trend.coef[b]))
    one = Trend.from_dataset(io_netcdf.open_dataset(path), device="cpu", kern=TrendDouble())
    assert len(one.coef) == 1 and one.coef[0].shape == (8, M)
    later = _hourly("2024-02-28T00", 20, 9)
    e2 = np.arange(20.0)
    assert all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(back.at(later, e2), trend.at(later, e2)))
    with pytest.raises(ValueError, match="rows sum"):
        Trend.from_dataset(io_netcdf.open_dataset(path), rows=(3, 4), device="cpu", kern=TrendDouble())


# ---------------------------------------------------------------- through the forecast
def _forecast(seed=11):
    from test_ensemble import _bundle, _members

    from dmd_era5_amd.climatology import Climatology
    from dmd_era5_amd.trend import Trend

    rs = np.random.RandomState(seed)
    f, Ub, mu, sd = _bundle(_members(1, 7, seed=2), TrendDouble, rs, rows=ROWS)
    times, X = _toy(T=48, seed=seed, step_h=1)
    clim = Climatology.fit(X, times, "hour", kern=f.kern)
    anom = clim.remove_([x.clone() for x in X], times)
    trend = Trend.fit(anom, times, degree=1, kern=f.kern)
    return f, clim, trend, times, X


def test_forecast_fields_restore_the_trend_and_then_the_climatology():
    f, clim, trend, times, _ = _forecast()
    valid = _hourly("2020-03-09T07", 10, 1)
    t = torch.from_numpy(np.linspace(0.0, 2.0, 10))
    plain = f.fields(t)
    full = f.fields(t, trend=trend, climatology=clim, times=valid)
    only = f.fields(t, trend=trend, times=valid)
    D = trend.design(valid)
    slot = clim._labels(valid, "test")
    for b in range(2):
        step1 = tr.apply(plain[b].numpy().T, D, trend.coef[b].numpy(), restore=True)
        assert np.array_equal(_bits(only[b]), _bits(step1.T))
        step2 = cr.apply(step1, slot, clim.mean[b].numpy(), None, restore=True)
        assert np.array_equal(_bits(full[b]), _bits(step2.T))
    again = f.fields(t)
    assert all(torch.equal(p, q) for p, q in zip(plain, again))  # the default path is untouched
    with pytest.raises(ValueError, match="go together"):
        f.fields(t, trend=trend)
    with pytest.raises(ValueError, match="go together"):
        f.fields(t, times=valid)


def test_a_delay_without_a_delay_block_is_refused():
    import test_pack as tp

    f = tp._mock_forecast(delay=2)
    _, _, trend, _, _ = _forecast()
    valid = _hourly("2020-03-09T07", 4, 1)
    with pytest.raises(ValueError, match="delay_block"):
        f.fields(torch.linspace(0, 1, 4).double(), delay_block=None, trend=trend, times=valid)


def test_forecast_verify_with_a_trend_scores_detrended_anomalies():
    from dmd_era5_amd.forecast import verify_blocks

    f, clim, trend, times, X = _forecast(12)
    T = 12
    t = torch.from_numpy(np.linspace(0.0, 2.0, T))
    valid, Xv = times[5:5 + T], [x[5:5 + T].contiguous() for x in X]
    keep = [x.clone() for x in Xv]
    w = [torch.linspace(0.2, 1.0, mb) for mb in ROWS]
    zeros = [torch.zeros(mb) for mb in ROWS]
    slot, D = clim._labels(valid, "test"), trend.design(valid)
    for with_clim in (True, False):
        res = f.verify(Xv, t, weights=w, trend=trend, climatology=clim if with_clim else None, times=valid, want_rows=True)
        assert all(torch.equal(a, b) for a, b in zip(Xv, keep))  # anomalised and detrended into a scratch copy
        Xa = []
        for x, m, c in zip(Xv, clim.mean, trend.coef):
            a = cr.apply(x.numpy().T, slot, m.numpy()) if with_clim else x.numpy().T
            Xa.append(torch.from_numpy(np.ascontiguousarray(tr.apply(a, D, c.numpy()).T)))
        want = verify_blocks(f.Ublocks, f.coefficients(t)[0], Xa, f.means, f.stds, w, zeros, kern=f.kern, want_rows=True)
        for key, v in want.items():
            if isinstance(v, list):
                assert all(torch.equal(a, b) for a, b in zip(res[key], v)), key
            else:
                assert torch.equal(res[key], v), key
    assert not torch.equal(f.verify(Xv, t, weights=w, climatology=clim, times=valid)["sums"], res["sums"])
    with pytest.raises(ValueError, match="clims and trend"):
        f.verify(Xv, t, clims=zeros, trend=trend, times=valid)
    with pytest.raises(ValueError, match="go together"):
        f.verify(Xv, t, trend=trend)


@pytest.mark.skipif(not __import__("dmd_era5_amd.hdf5_lite", fromlist=["x"]).available(), reason="libhdf5 not found")
@pytest.mark.parametrize("delay,with_clim", [(1, False), (2, True)])
def test_write_forecast_slice_with_a_trend(tmp_path, monkeypatch, delay, with_clim):
    """Slabs of expand -> trend restore_ -> climatology restore_ -> pack: the file holds the codes of those fields."""
    import pack_ref as pr
    import test_pack as tp

    from dmd_era5_amd import era5_svd, hdf5_lite
    from dmd_era5_amd.climatology import Climatology
    from dmd_era5_amd.trend import Trend

    class Both(TrendDouble, tp.DoubleWithPack):
        name = "cpu-double+pack+clim+treg"

    monkeypatch.setenv("DMDX_NETCDF_BACKEND", "hdf5")
    f = tp._mock_forecast(delay=delay)
    f.kern = Both()
    rows = [int(U.shape[1]) // delay for U in f.Ublocks]
    rs = np.random.RandomState(3)
    hist = _hourly("2018-06-01T00", 72, 1)
    H = [torch.from_numpy((40.0 * rs.standard_normal((72, mb)) + np.linspace(0, 90, 72)[:, None]).astype(np.float32))
         for mb in rows]
    enso = rs.standard_normal(72)
    clim = Climatology.fit(H, hist, "hour", kern=f.kern) if with_clim else None
    trend = Trend.fit(H, hist, degree=1, extra=enso, kern=f.kern)
    T = 13
    t, time = np.linspace(0.0, 3.0, T), tp._times(T)
    e2 = rs.standard_normal(T)
    plane = sum(rows) // 2
    path = str(tmp_path / "full.nc")
    res = era5_svd.write_forecast_slice(path, f, t, time, tp.NAMES, **tp.GRID, slab=4, climatology=clim, trend=trend,
                                        trend_extra=e2)
    fields = f.fields(torch.from_numpy(t), trend=trend, trend_extra=e2, climatology=clim, times=time)
    want = np.concatenate([x.numpy() for x in fields], axis=1)
    assert np.abs(want - np.concatenate([x.numpy() for x in f.fields(torch.from_numpy(t))], axis=1)).max() > 10.0
    r = hdf5_lite.Reader(path)
    for g, name in enumerate(tp.NAMES):
        w = np.ascontiguousarray(want[:, g * plane:(g + 1) * plane]).reshape(T, 2, 6, 7)
        pk = res["packing"][name]
        assert (pk.scale_factor, pk.add_offset) == pr.for_range(*pr.finite_range(w)[:2])
        assert np.array_equal(r.read(name), pr.encode(w, pk.scale_factor, pk.add_offset)[0])
        assert (res["filled"][name], res["saturated"][name]) == (0, 0)
    r.close()
    paths = [str(tmp_path / n) for n in ("a.nc", "b.nc")]
    era5_svd.write_forecast_slice(paths[0], f, t, time, tp.NAMES, **tp.GRID, slab=4, attrs={"date_downloaded": "fixed"})
    era5_svd.write_forecast_slice(paths[1], f, t, time, tp.NAMES, **tp.GRID, slab=4, attrs={"date_downloaded": "fixed"},
                                  trend=None)
    assert open(paths[0], "rb").read() == open(paths[1], "rb").read()
    with pytest.raises(ValueError, match="datetime64"):
        era5_svd.write_forecast_slice(paths[1], f, t, np.arange(T), tp.NAMES, **tp.GRID, trend=trend, trend_extra=e2)


def test_alias_package_re_exports_the_module():
    import dmd_era5.trend as alias
    import dmd_era5_amd.trend as mod

    assert alias.Trend is mod.Trend and alias.design is mod.design and set(alias.__all__) == set(mod.__all__)
