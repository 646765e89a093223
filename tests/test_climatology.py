"""Host side of K18 without a GPU: slots_of against a per-snapshot loop over datetime objects, and Climatology /
DmdForecast(climatology=) on a kernel double whose three clim methods are tests/clim_ref.py, the host definition."""
import datetime as dt

import numpy as np
import pytest
import torch

import clim_ref as cr
from kernel_double import CpuKernelDouble


class ClimDouble(CpuKernelDouble):
    """CpuKernelDouble + the three K18 methods of HipKernels, computed by clim_ref."""

    name = "cpu-double+clim"

    def clim_mean(self, Xt, order, start, out=None):
        M = torch.from_numpy(cr.mean(Xt.numpy().T, order.numpy(), start.numpy()))
        if out is None:
            return M
        out.copy_(M)
        return out

    def clim_std(self, Xt, order, start, mean, ddof=0, out=None):
        Sd = torch.from_numpy(cr.std(Xt.numpy().T, order.numpy(), start.numpy(), mean.numpy(), ddof))
        if out is None:
            return Sd
        out.copy_(Sd)
        return out

    def clim_apply_(self, Xt, slot, mean, sd=None, restore=False, out=None):
        Y = cr.apply(Xt.numpy().T, slot.numpy(), mean.numpy(), None if sd is None else sd.numpy(), restore)
        dst = Xt if out is None else out
        dst.copy_(torch.from_numpy(np.ascontiguousarray(Y.T)))
        return dst


def _bits(a):
    a = a.numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _hourly(start, n, step_h=1):
    return np.datetime64(start, "h") + np.arange(n) * np.timedelta64(step_h, "h")


# ---------------------------------------------------------------- slots_of
def _slot_by_hand(stamp: dt.datetime, kind):
    leap_day = (dt.date(2000, stamp.month, stamp.day) - dt.date(2000, 1, 1)).days      # 2000 is a leap year
    return {"hour": stamp.hour, "month_hour": (stamp.month - 1) * 24 + stamp.hour, "dayofyear": leap_day,
            "dayofyear_hour": leap_day * 24 + stamp.hour}[kind]


# 7-hourly over two year boundaries and the leap day of 2020, plus the days around Feb 29 / Mar 1 of a common year
TIMES = np.concatenate([_hourly("2019-12-20T00", 420, 7), _hourly("2021-02-27T22", 60, 1), _hourly("2020-02-28T20", 40, 1)])


@pytest.mark.parametrize("kind,S", [("hour", 24), ("month_hour", 288), ("dayofyear", 366), ("dayofyear_hour", 8784)])
def test_slots_of_equals_a_loop_over_datetime_objects(kind, S):
    from dmd_era5_amd.climatology import slots_of

    slot, order, start, n = slots_of(TIMES, kind)
    assert n == S and slot.dtype == order.dtype == start.dtype == np.int32
    assert slot.shape == TIMES.shape and start.shape == (S + 1,) and order.shape == TIMES.shape
    stamps = TIMES.astype("datetime64[s]").astype(dt.datetime)
    want = np.array([_slot_by_hand(x, kind) for x in stamps])
    assert np.array_equal(slot, want)
    members = {}
    for t in np.argsort(TIMES.astype("datetime64[s]").astype(np.int64), kind="stable"):
        members.setdefault(int(want[t]), []).append(int(t))
    assert start[0] == 0 and start[-1] == TIMES.shape[0]
    for s in range(S):
        got = order[start[s]:start[s + 1]].tolist()
        assert got == members.get(s, []), s
        assert np.all(np.diff(TIMES[got].astype("datetime64[s]").astype(np.int64)) >= 0)    # ascending in time
    if kind.startswith("dayofyear"):
        feb29 = [x for x in stamps if (x.month, x.day) == (2, 29)]
        mar1 = [x for x in stamps if (x.month, x.day) == (3, 1)]
        assert feb29 and {_slot_by_hand(x, "dayofyear") for x in feb29} == {59}
        assert len({x.year for x in mar1}) == 2 and {_slot_by_hand(x, "dayofyear") for x in mar1} == {60}


@pytest.mark.parametrize("kind", ["dayofyear", "dayofyear_hour"])
def test_a_three_day_window_wraps_from_january_into_december(kind):
    from dmd_era5_amd.climatology import slots_of

    times = _hourly("2021-12-25T00", 24 * 14, 3)                # 25 December .. 7 January, 3-hourly
    slot, order, start, S = slots_of(times, kind, window_days=3)
    own = slots_of(times, kind)[0]
    assert np.array_equal(slot, own)                             # the label is the snapshot's own class
    stamps = times.astype("datetime64[s]").astype(dt.datetime)
    doy = np.array([_slot_by_hand(x, "dayofyear") for x in stamps])
    hour = np.array([x.hour for x in stamps])
    assert order.shape[0] == 7 * times.shape[0]
    for d, h in ((1, 0), (1, 21), (0, 3), (364, 6), (365, 0), (180, 0)):   # 2 January = day 1; 365 = 31 December
        s = d if kind == "dayofyear" else d * 24 + h
        dist = np.minimum((doy - d) % 366, (d - doy) % 366)
        want = np.nonzero((dist <= 3) & ((hour == h) | (kind == "dayofyear")))[0]
        got = order[start[s]:start[s + 1]]
        assert got.tolist() == want.tolist(), (d, h)
    # 2 January (day 1) reaches back to 30 December (day 364) across the end of the 366-day circle
    s = 1 if kind == "dayofyear" else 24
    got_days = set(doy[order[start[s]:start[s + 1]]].tolist())
    assert got_days == {364, 365, 0, 1, 2, 3, 4}
    with pytest.raises(ValueError, match="day-of-year"):
        slots_of(times, "hour", window_days=1)
    with pytest.raises(TypeError, match="datetime64"):
        slots_of(np.arange(5), "hour")
    with pytest.raises(ValueError, match="kind"):
        slots_of(times, "week")


# ---------------------------------------------------------------- Climatology on a 2-block toy grid
ROWS = (9, 4)


def _toy(T=60, seed=0, kind="hour"):
    rs = np.random.RandomState(seed)
    times = _hourly("2020-03-01T00", T, 1)
    X = [torch.from_numpy((rs.standard_normal((T, mb)) + 5.0 * np.sin(np.arange(T) * 2 * np.pi / 24)[:, None])
                          .astype(np.float32)) for mb in ROWS]
    return times, X


@pytest.mark.parametrize("with_std", [False, True])
def test_fit_remove_restore_at(with_std):
    from dmd_era5_amd.climatology import Climatology, slots_of

    times, X = _toy()
    clim = Climatology.fit(X, times, "hour", with_std=with_std, ddof=1, kern=ClimDouble())
    slot, order, start, S = slots_of(times, "hour")
    assert np.array_equal(clim.counts, np.diff(start)) and clim.counts.sum() == 60 and clim.n_slots == 24
    assert (clim.sd is None) == (not with_std)
    for b, mb in enumerate(ROWS):
        Xb = X[b].numpy().T
        mu = cr.mean(Xb, order, start)
        assert clim.mean[b].shape == (24, mb) and np.array_equal(_bits(clim.mean[b]), _bits(mu))
        # the definition against numpy's own grouped mean: sums of 2 or 3 fp32 values in fp64 are exact
        for s in range(24):
            assert np.array_equal(mu[s], X[b].numpy()[slot == s].astype(np.float64).mean(axis=0).astype(np.float32))
        if with_std:
            assert np.array_equal(_bits(clim.sd[b]), _bits(cr.std(Xb, order, start, mu, 1)))
    sds = [None, None] if not with_std else [s.numpy() for s in clim.sd]
    keep = [x.clone() for x in X]
    out = [torch.full_like(x, 7.0) for x in X]
    res = clim.remove_(X, times, out=out)
    assert all(r is o for r, o in zip(res, out)) and all(torch.equal(a, b) for a, b in zip(X, keep))
    clim.remove_(X, times)                                       # in place
    for b in range(2):
        want = cr.apply(keep[b].numpy().T, slot, clim.mean[b].numpy(), sds[b]).T
        assert np.array_equal(_bits(X[b]), _bits(want)) and torch.equal(X[b], out[b])
    clim.restore_(X, times)
    for b in range(2):
        anom = cr.apply(keep[b].numpy().T, slot, clim.mean[b].numpy(), sds[b])
        want = cr.apply(anom, slot, clim.mean[b].numpy(), sds[b], restore=True).T
        assert np.array_equal(_bits(X[b]), _bits(want))          # the composition, not X to the bit
        assert np.allclose(X[b].numpy(), keep[b].numpy(), rtol=0, atol=1e-5)
    # .at of other times of the same hours: the mean of the slot, without the standard deviation
    later = _hourly("2031-07-04T05", 30, 1)
    F = clim.at(later)
    ls = slots_of(later, "hour")[0]
    for b in range(2):
        assert np.array_equal(_bits(F[b]), _bits(clim.mean[b].numpy()[ls]))


def test_an_unpopulated_slot_is_refused_before_any_launch():
    from dmd_era5_amd.climatology import Climatology

    class Counting(ClimDouble):
        calls = 0

        def clim_apply_(self, *a, **kw):
            Counting.calls += 1
            return super().clim_apply_(*a, **kw)

    times, X = _toy(T=20)                                        # hours 0 .. 19 only
    clim = Climatology.fit(X, times, "hour", kern=Counting())
    assert clim.counts[20:].sum() == 0
    with pytest.raises(ValueError, match="slot 20"):
        clim.remove_(X, _hourly("2020-03-05T12", 20, 1))
    with pytest.raises(ValueError, match="slot 23"):
        clim.at(_hourly("2020-03-05T23", 1))
    assert Counting.calls == 0
    with pytest.raises(ValueError, match="ddof"):
        Climatology.fit(X, times, "hour", with_std=True, ddof=2, kern=Counting())
    with pytest.raises(ValueError, match="snapshots"):
        Climatology.fit([X[0][:5]], times, "hour", kern=Counting())


@pytest.mark.parametrize("with_std", [False, True])
def test_dataset_round_trip_through_a_file(tmp_path, with_std):
    from dmd_era5_amd import io_netcdf
    from dmd_era5_amd.climatology import Climatology
    from dmd_era5_amd.labeled import Coord

    times, X = _toy(T=50)
    clim = Climatology.fit(X, times, "month_hour", with_std=with_std, ddof=1 if with_std else 0, kern=ClimDouble())
    M = sum(ROWS)
    coords = {"space": Coord("space", np.arange(M, dtype=np.int64)),
              "latitude": Coord("space", np.linspace(-60.0, 60.0, M)), "time": Coord("time", times)}
    ds = clim.to_dataset(coords)
    assert ds["clim_mean"].dims == ("slot", "space") and ds["clim_mean"].shape == (288, M)
    assert "time" not in ds.coords and ("clim_std" in ds) == with_std
    path = str(tmp_path / "clim.nc")
    io_netcdf.to_netcdf(ds, path)
    back = Climatology.from_dataset(io_netcdf.open_dataset(path), rows=ROWS, device="cpu", kern=ClimDouble())
    assert back.kind == "month_hour" and back.window_days == 0 and back.ddof == clim.ddof
    assert np.array_equal(back.counts, clim.counts)
    for b in range(2):
        assert np.array_equal(_bits(back.mean[b]), _bits(clim.mean[b]))          # NaN slots included, bit for bit
        if with_std:
            assert np.array_equal(_bits(back.sd[b]), _bits(clim.sd[b]))
    assert (back.sd is None) == (not with_std)
    one = Climatology.from_dataset(io_netcdf.open_dataset(path), device="cpu", kern=ClimDouble())
    assert len(one.mean) == 1 and one.mean[0].shape == (288, M)
    a = back.remove_([x.clone() for x in X], times)
    b = clim.remove_([x.clone() for x in X], times)
    assert all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(a, b))


# ---------------------------------------------------------------- through the forecast
def _forecast(seed=11):
    from test_ensemble import _bundle, _members

    from dmd_era5_amd.climatology import Climatology

    rs = np.random.RandomState(seed)
    f, Ub, mu, sd = _bundle(_members(1, 7, seed=2), ClimDouble, rs, rows=ROWS)
    times, X = _toy(T=48, seed=seed)
    clim = Climatology.fit(X, times, "hour", kern=f.kern)
    return f, clim, times, X


def test_forecast_fields_with_a_climatology_are_fields_plus_at():
    f, clim, times, _ = _forecast()
    valid = _hourly("2020-03-09T07", 10, 1)
    t = torch.from_numpy(np.linspace(0.0, 2.0, 10))
    plain = f.fields(t)
    full = f.fields(t, climatology=clim, times=valid)
    at = clim.at(valid)
    for p, q, a in zip(plain, full, at):
        assert np.array_equal(_bits(q), _bits((p.numpy() + a.numpy()).astype(np.float32)))
    again = f.fields(t)
    assert all(torch.equal(p, q) for p, q in zip(plain, again))  # the default path is untouched
    with pytest.raises(ValueError, match="go together"):
        f.fields(t, climatology=clim)
    with pytest.raises(ValueError, match="go together"):
        f.fields(t, times=valid)


def test_forecast_verify_with_a_climatology_scores_anomalies():
    from dmd_era5_amd.forecast import verify_blocks

    f, clim, times, X = _forecast(12)
    T = 12
    t = torch.from_numpy(np.linspace(0.0, 2.0, T))
    valid, Xv = times[5:5 + T], [x[5:5 + T].contiguous() for x in X]
    keep = [x.clone() for x in Xv]
    w = [torch.linspace(0.2, 1.0, mb) for mb in ROWS]
    res = f.verify(Xv, t, weights=w, climatology=clim, times=valid, want_rows=True)
    assert all(torch.equal(a, b) for a, b in zip(Xv, keep))      # the analysis is anomalised into a scratch copy
    slot = clim._labels(valid, "test")
    Xa = [torch.from_numpy(np.ascontiguousarray(cr.apply(x.numpy().T, slot, m.numpy()).T)) for x, m in zip(Xv, clim.mean)]
    zeros = [torch.zeros(mb) for mb in ROWS]
    want = verify_blocks(f.Ublocks, f.coefficients(t)[0], Xa, f.means, f.stds, w, zeros, kern=f.kern, want_rows=True)
    for key, v in want.items():
        if isinstance(v, list):
            assert all(torch.equal(a, b) for a, b in zip(res[key], v)), key
        else:
            assert torch.equal(res[key], v), key
    plain = f.verify(Xv, t, weights=w)
    assert not torch.equal(plain["sums"], res["sums"])
    with pytest.raises(ValueError, match="clims and climatology"):
        f.verify(Xv, t, clims=zeros, climatology=clim, times=valid)
    with pytest.raises(ValueError, match="go together"):
        f.verify(Xv, t, climatology=clim)


@pytest.mark.skipif(not __import__("dmd_era5_amd.hdf5_lite", fromlist=["x"]).available(), reason="libhdf5 not found")
@pytest.mark.parametrize("delay,given", [(1, False), (2, False), (1, True)])
def test_write_forecast_slice_with_a_climatology(tmp_path, monkeypatch, delay, given):
    """Slabs of expand -> restore_ -> pack: the file decodes to fields + at(times) within half a step, the range
    pass runs on the restored fields, and without a climatology the file is the one the parent path writes."""
    import pack_ref as pr
    import test_pack as tp

    from dmd_era5_amd import era5_svd, hdf5_lite, io_netcdf
    from dmd_era5_amd.climatology import Climatology
    from dmd_era5_amd.labeled import Packing

    class Both(ClimDouble, tp.DoubleWithPack):
        name = "cpu-double+pack+clim"

    monkeypatch.setenv("DMDX_NETCDF_BACKEND", "hdf5")
    f = tp._mock_forecast(delay=delay)
    f.kern = Both()
    rows = [int(U.shape[1]) // delay for U in f.Ublocks]
    rs = np.random.RandomState(3)
    hist = _hourly("2018-06-01T00", 72, 1)
    clim = Climatology.fit([torch.from_numpy((40.0 * rs.standard_normal((72, mb))).astype(np.float32)) for mb in rows], hist,
                           "hour", kern=f.kern)
    T = 13
    t, time = np.linspace(0.0, 3.0, T), tp._times(T)
    plane = sum(rows) // 2
    packing = {n: Packing.for_range(-400.0, 700.0) for n in tp.NAMES} if given else None
    path = str(tmp_path / "full.nc")
    res = era5_svd.write_forecast_slice(path, f, t, time, tp.NAMES, **tp.GRID, slab=4, climatology=clim, packing=packing)
    want = np.concatenate([(p.numpy() + a.numpy()).astype(np.float32)
                           for p, a in zip(f.fields(torch.from_numpy(t)), clim.at(time))], axis=1)
    ds = io_netcdf.open_dataset(path)
    r = hdf5_lite.Reader(path)
    for g, name in enumerate(tp.NAMES):
        w = np.ascontiguousarray(want[:, g * plane:(g + 1) * plane]).reshape(T, 2, 6, 7)
        pk = res["packing"][name]
        if not given:
            assert (pk.scale_factor, pk.add_offset) == pr.for_range(*pr.finite_range(w)[:2])
        assert np.array_equal(r.read(name), pr.encode(w, pk.scale_factor, pk.add_offset)[0])
        assert (np.abs(np.asarray(ds[name].values).astype(np.float64) - w) <= pk.scale_factor / 2 + pr.ulp32(w)).all()
        assert (res["filled"][name], res["saturated"][name]) == (0, 0)
    r.close()
    paths = [str(tmp_path / n) for n in ("a.nc", "b.nc")]
    era5_svd.write_forecast_slice(paths[0], f, t, time, tp.NAMES, **tp.GRID, slab=4, attrs={"date_downloaded": "fixed"})
    era5_svd.write_forecast_slice(paths[1], f, t, time, tp.NAMES, **tp.GRID, slab=4, attrs={"date_downloaded": "fixed"},
                                  climatology=None)
    assert open(paths[0], "rb").read() == open(paths[1], "rb").read()
    with pytest.raises(ValueError, match="datetime64"):
        era5_svd.write_forecast_slice(paths[1], f, t, np.arange(T), tp.NAMES, **tp.GRID, climatology=clim)


def test_alias_package_re_exports_the_module():
    import dmd_era5.climatology as alias
    import dmd_era5_amd.climatology as mod

    assert alias.Climatology is mod.Climatology and alias.slots_of is mod.slots_of and set(alias.__all__) == set(mod.__all__)
