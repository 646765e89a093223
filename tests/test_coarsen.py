"""K23 on the host: tests/coarsen_ref.py (the arithmetic contract of csrc/coarsen.hip) against an independent
formulation and against the exact values its chain must give, dmd_era5_amd/regrid.py (weights, geometry, refusals, round
trips, latitude bands) through the CPU double of the kernel, and every refusal of the C entry point, which answers before
any HIP call.  The device side is tests/test_gpu_coarsen.py and tests/test_gpu_regrid.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

import coarsen_ref as cr
from dmd_era5_amd import io_netcdf
from dmd_era5_amd.regrid import Coarsen, coarse_lat_band, lat_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTORS = ((4, 4), (3, 5), (2, 8), (1, 1))
NLAT, NLON = 13, 24


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _field(T=3, planes=2, nlat=NLAT, nlon=NLON, seed=0):
    rs = np.random.RandomState(seed)
    return (250.0 + 30.0 * rs.standard_normal((T, planes * nlat * nlon))).astype(np.float32)


def _weights(nlat=NLAT, seed=1):
    return lat_weights(np.linspace(80.0, -70.0, nlat), "cos") + 0.01 * np.random.RandomState(seed).uniform(size=nlat)


# ---------------------------------------------------------------- the host definition
@pytest.mark.parametrize("fy,fx", FACTORS)
def test_ref_against_numpy_average(fy, fx):
    """Positive data: both results are fp64 weighted means whose relative error is at most fy fx 2^-53 (sums of
    positive terms, a few roundings each), rounded once to fp32 -- they are neighbours in fp32 at the most."""
    T, P = 3, 2
    X, w = _field(T, P), _weights()
    got = cr.coarsen(X, P, NLAT, NLON, w, fy, fx).reshape(T, P, NLAT // fy, NLON // fx)
    fine = X.astype(np.float64).reshape(T, P, NLAT, NLON)
    want = np.empty(got.shape, dtype=np.float64)
    for I in range(NLAT // fy):
        for J in range(NLON // fx):
            cell = fine[:, :, I * fy:(I + 1) * fy, J * fx:(J + 1) * fx].reshape(T, P, fy * fx)
            want[:, :, I, J] = np.average(cell, axis=2, weights=np.repeat(w[I * fy:(I + 1) * fy], fx))
    want32 = want.astype(np.float32)
    ulp = np.abs(got.view(np.int32).astype(np.int64) - want32.view(np.int32).astype(np.int64))
    print(f"{fy} x {fx}: {int((ulp > 0).sum())} of {ulp.size} cells one ulp apart")
    assert ulp.max() <= 1


@pytest.mark.parametrize("fy,fx", FACTORS)
def test_ref_exact_values(fy, fx):
    w = _weights()
    const = np.full((2, 2 * NLAT * NLON), np.float32(287.654), dtype=np.float32)
    got = cr.coarsen(const, 2, NLAT, NLON, w, fy, fx)
    assert (_bits(got) == _bits(np.float32(287.654))).all()
    X = _field()
    base = cr.coarsen(X, 2, NLAT, NLON, w, fy, fx, lat0=1, lon0=2)
    for e in (-20, 20):
        assert np.array_equal(_bits(cr.coarsen(np.ldexp(X, e), 2, NLAT, NLON, w, fy, fx, lat0=1, lon0=2)), _bits(np.ldexp(base, e)))
    zeros = np.zeros((1, NLAT * NLON), dtype=np.float32)
    zeros[0, ::2] = -0.0
    assert (_bits(cr.coarsen(zeros, 1, NLAT, NLON, w, fy, fx)) == 0).all()
    assert (_bits(cr.coarsen(-np.abs(zeros), 1, NLAT, NLON, w, fy, fx)) == 0).all()


@pytest.mark.parametrize("fy,fx", ((1, 1), (2, 2), (4, 4), (2, 8), (8, 8)))
def test_ref_integer_mean_is_exact(fy, fx):
    """Integers in +-1000 with unit weights and fy fx a power of two: every sum is an integer below 2^17 and the
    quotient is a multiple of 2^-6 below 2^10: exact in fp64 and in fp32."""
    rs = np.random.RandomState(5)
    nlat, nlon = 17, 26
    Xi = rs.randint(-1000, 1001, (2, 3, nlat, nlon)).astype(np.int64)
    got = cr.coarsen(Xi.reshape(2, -1).astype(np.float32), 3, nlat, nlon, np.ones(nlat), fy, fx, lat0=1, lon0=2)
    NL, NO = (nlat - 1) // fy, (nlon - 2) // fx
    want = Xi[:, :, 1:1 + NL * fy, 2:2 + NO * fx].reshape(2, 3, NL, fy, NO, fx).sum(axis=(3, 5))
    assert np.array_equal(got.astype(np.float64) * (fy * fx), want.reshape(2, -1).astype(np.float64))


def test_ref_skipna_and_min_frac():
    nlat, nlon, fy, fx = 8, 8, 4, 4
    w = np.array([1.0, 2.0, 3.0, 2.0, 1.0, 1.0, 1.0, 1.0])
    X = _field(1, 1, nlat, nlon, seed=3)
    fine = X.reshape(nlat, nlon).copy()
    # cell (0, 0): the rows of weight 1 and 3 all missing: kept weight 4 (2 + 2) x 4 = 16 of 32: exactly min_frac = 0.5
    fine[0, 0:4] = np.nan
    fine[2, 0:4] = np.inf
    # cell (0, 1): one more value missing: just below one half
    fine[0, 4:8] = np.nan
    fine[2, 4:8] = -np.inf
    fine[1, 5] = np.nan
    # cell (1, 0): everything missing; cell (1, 1): one value missing
    fine[4:8, 0:4] = np.nan
    fine[6, 6] = np.nan
    Xn = fine.reshape(1, -1)
    got = cr.coarsen(Xn, 1, nlat, nlon, w, fy, fx, skipna=True, min_frac=0.5).reshape(2, 2)
    f64 = fine.astype(np.float64)
    assert got[0, 0] == np.float32((2.0 * f64[1, 0:4].sum() + 2.0 * f64[3, 0:4].sum()) / 16.0)
    assert np.isnan(got[0, 1]) and _bits(got[0, 1]) == cr.QUIET_NAN_BITS
    assert np.isnan(got[1, 0]) and _bits(got[1, 0]) == cr.QUIET_NAN_BITS
    keep = np.isfinite(fine[4:8, 4:8])
    mean15 = f64[4:8, 4:8][keep].sum() / 15.0
    assert abs(float(got[1, 1]) - mean15) <= 2.0 ** -23 * abs(mean15)
    # at the threshold (kept weight 14 of 32, min_frac = 14 / 32: "below" is strict): the mean of the rest
    above = cr.coarsen(Xn, 1, nlat, nlon, w, fy, fx, skipna=True, min_frac=14.0 / 32.0).reshape(2, 2)
    rest = 2.0 * (f64[1, 4] + f64[1, 6] + f64[1, 7]) + 2.0 * f64[3, 4:8].sum()
    assert abs(float(above[0, 1]) - rest / 14.0) <= 2.0 ** -23 * abs(rest / 14.0)
    assert np.isnan(cr.coarsen(Xn, 1, nlat, nlon, w, fy, fx, skipna=True, min_frac=14.5 / 32.0).reshape(2, 2)[0, 1])
    assert cr.coarsen(Xn, 1, nlat, nlon, w, fy, fx, skipna=True, min_frac=0.0).reshape(2, 2)[0, 1] == above[0, 1]
    # skipna off: one NaN makes exactly its own cell NaN
    one = X.copy()
    one[0, 6 * nlon + 6] = np.nan
    off = cr.coarsen(one, 1, nlat, nlon, w, fy, fx, min_frac=0.5).reshape(2, 2)
    clean = cr.coarsen(X, 1, nlat, nlon, w, fy, fx).reshape(2, 2)
    assert np.isnan(off[1, 1]) and np.array_equal(_bits(off)[[0, 0, 1], [0, 1, 0]], _bits(clean)[[0, 0, 1], [0, 1, 0]])


@pytest.mark.parametrize("fy,fx", FACTORS)
def test_ref_nan_fractions(fy, fx):
    """30 % of the values missing: under skipna with min_frac = 0.5 some cells are NaN but not most; with skipna off
    every cell of more than one value is."""
    rs = np.random.RandomState(11)
    X = _field(4, 1)
    X[rs.uniform(size=X.shape) < 0.3] = np.nan
    w = _weights()
    on = np.isnan(cr.coarsen(X, 1, NLAT, NLON, w, fy, fx, skipna=True, min_frac=0.5)).mean()
    off = np.isnan(cr.coarsen(X, 1, NLAT, NLON, w, fy, fx)).mean()
    print(f"{fy} x {fx}: NaN cells {on:.3f} with skipna, {off:.3f} without")
    # a cell is NaN with the probability that the binomial of its fy fx values leaves less than half: 0.3 at 1 x 1
    assert on <= 0.35
    # without skipna a cell of n values survives with 0.7^n: below 0.5 % from 15 values on
    assert (off >= 0.95) if fy * fx >= 15 else (0.25 <= off <= 0.35)


# ---------------------------------------------------------------- weights
def test_lat_weights():
    lat = np.linspace(90.0, -90.0, 721)
    band = lat_weights(lat, "band")
    assert band.dtype == np.float64 and (band > 0.0).all()
    assert abs(band.sum() - 2.0) <= 1e-15
    assert np.allclose(band[1:-1], np.cos(np.deg2rad(lat[1:-1])) * 2.0 * np.sin(np.deg2rad(0.125)), rtol=1e-10)
    assert abs(band[0] - (1.0 - np.sin(np.deg2rad(89.875)))) <= 1e-16
    assert abs(lat_weights(lat[::-1], "band").sum() - 2.0) <= 1e-15
    cos = lat_weights(lat, "cos")
    assert (cos >= 0.0).all() and cos[360] == 1.0 and cos[0] <= 1e-16 and cos[-1] <= 1e-16
    assert (lat_weights([90.0, -90.0], "cos") >= 0.0).all()
    assert np.array_equal(lat_weights(lat, "none"), np.ones(721))
    with pytest.raises(ValueError, match="evenly"):
        lat_weights([10.0, 20.0, 35.0], "band")
    with pytest.raises(ValueError, match="kind"):
        lat_weights(lat, "area")
    with pytest.raises(ValueError, match="latitude"):
        lat_weights([10.0, 95.0], "cos")
    lon = np.arange(8) * 45.0
    with pytest.raises(ValueError, match="negative"):
        Coarsen(lat[:4], lon, 2, 2, weights=[1.0, -1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="not finite"):
        Coarsen(lat[:4], lon, 2, 2, weights=[1.0, np.nan, 1.0, 1.0])
    with pytest.raises(ValueError, match="one weight per latitude row"):
        Coarsen(lat[:4], lon, 2, 2, weights=[1.0, 1.0, 1.0])


# ---------------------------------------------------------------- Coarsen
def test_geometry_on_the_era5_grid():
    lat, lon = 90.0 - 0.25 * np.arange(721), 0.25 * np.arange(1440)
    cz = Coarsen(lat, lon, 4, 4)
    assert cz.shape_in == (721, 1440) and cz.shape_out == (180, 360) and cz.dropped == (1, 0)
    assert cz.latitude_out[0] == 89.625 and cz.latitude_out[-1] == -89.375 and cz.longitude_out[0] == 0.375
    assert cz.latitude_out.dtype == np.float64 and cz.latitude_out.shape == (180,) and cz.longitude_out.shape == (360,)
    assert np.array_equal(cz.weights, lat_weights(lat, "cos"))
    assert np.array_equal(cz.weights_out, cz.weights[:720].reshape(180, 4).sum(axis=1))
    assert cz.rows_out(3) == 3 * 180 * 360
    rw = cz.row_weights_out(2)
    assert rw.dtype == torch.float32 and rw.shape == (2 * 180 * 360,)
    assert np.array_equal(rw.numpy().reshape(2, 180, 360)[1, :, 7], cz.weights_out.astype(np.float32))
    south = Coarsen(lat, lon, 4, 4, lat0=1)
    assert south.dropped == (1, 0) and south.latitude_out[0] == 89.375
    odd = Coarsen(lat, lon, 3, 7, lon0=2)
    assert odd.shape_out == (240, 205) and odd.dropped == (1, 5)


def test_refusals_before_any_launch():
    lat, lon = np.linspace(60.0, -60.0, NLAT), np.arange(NLON) * 15.0
    kern = cr.CoarsenDouble()
    for bad in (dict(fy=0, fx=4), dict(fy=4, fx=0), dict(fy=65, fx=4), dict(fy=14, fx=4), dict(fy=4, fx=25),
                dict(fy=4, fx=4, lat0=10), dict(fy=4, fx=4, lon0=-1), dict(fy=4, fx=4, min_frac=1.5),
                dict(fy=4, fx=4, min_frac=float("nan"))):
        with pytest.raises(ValueError):
            Coarsen(lat, lon, kern=kern, **bad)
    cz = Coarsen(lat, lon, 4, 4, kern=kern)
    X = torch.zeros((3, 2 * NLAT * NLON))
    with pytest.raises(ValueError, match="block 1 holds"):
        cz.apply([X, X[:, :-1]], 2)
    with pytest.raises(ValueError, match="planes"):
        cz.apply([X, X], [2])
    with pytest.raises(ValueError, match="planes"):
        cz.apply([X], 0)
    with pytest.raises(ValueError, match=r"out\[0\]"):
        cz.apply([X], 2, out=[torch.zeros((3, 35))])
    with pytest.raises(ValueError, match="time, rows"):
        cz.apply([X[0]], 2)
    with pytest.raises(ValueError, match="vector"):
        cz.apply_field(X, 2)
    assert kern.calls == []


@pytest.mark.parametrize("fy,fx", ((4, 4), (3, 5)))
def test_apply_through_the_host_double_and_round_trips(tmp_path, fy, fx):
    lat, lon = np.linspace(60.0, -60.0, NLAT), np.arange(NLON) * 15.0
    kern = cr.CoarsenDouble()
    cz = Coarsen(lat, lon, fy, fx, lat0=1, weights="band", skipna=True, min_frac=0.4, kern=kern)
    host = [_field(3, 2, seed=7), np.concatenate([_field(3, 1, seed=8), np.full((3, 3), np.nan, np.float32)], axis=1)]
    host[0][1, 40:44] = np.nan
    X = [torch.from_numpy(h) for h in host]
    Y = cz.apply(X, [2, 1])
    assert kern.calls == [((3, 2 * NLAT * NLON), 2, fy, fx), ((3, NLAT * NLON + 3), 1, fy, fx)]
    for y, h, p in zip(Y, host, (2, 1)):
        want = cr.coarsen(h, p, NLAT, NLON, cz.weights, fy, fx, lat0=1, skipna=True, min_frac=0.4)
        assert y.shape == (3, cz.rows_out(p)) and np.array_equal(_bits(y.numpy()), _bits(want))
    out = [torch.zeros((3, cz.rows_out(2))), torch.zeros((3, cz.rows_out(1)))]
    Y2 = cz.apply(iter(X), (2, 1), out=out)
    assert all(a is b for a, b in zip(Y2, out)) and all(np.array_equal(_bits(a.numpy()), _bits(b.numpy())) for a, b in zip(Y, Y2))
    f = cz.apply_field(X[1][0], 1)
    assert f.shape == (cz.rows_out(1),) and np.array_equal(_bits(f.numpy()), _bits(Y[1][0].numpy()))
    # round trips: a kind, and an array of weights
    arr = Coarsen(lat, lon, fy, fx, lon0=2, weights=_weights(), min_frac=0.25, kern=kern)
    for c in (cz, arr):
        ds = c.to_dataset()
        assert ds["coarsen_weights"].dims == ("latitude",)
        path = str(tmp_path / f"coarsen_{c.kind}.nc")
        c.to_netcdf(path)
        for back in (Coarsen.from_dataset(ds, kern), Coarsen.from_netcdf(path, kern),
                     Coarsen.from_dataset(io_netcdf.open_dataset(path), kern)):
            assert (back.fy, back.fx, back.lat0, back.lon0, back.kind) == (c.fy, c.fx, c.lat0, c.lon0, c.kind)
            assert (back.skipna, back.min_frac) == (c.skipna, c.min_frac)
            assert np.array_equal(back.weights.view(np.uint64), c.weights.view(np.uint64))
            assert np.array_equal(back.latitude, lat) and np.array_equal(back.longitude, lon)
            for a, b in zip(back.apply(X, [2, 1]), c.apply(X, [2, 1])):
                assert np.array_equal(_bits(a.numpy()), _bits(b.numpy()))


@pytest.mark.parametrize("world", (1, 2, 8))
def test_coarse_lat_band(world):
    nlat, nlon, fy, fx, lat0, P = 37, 12, 4, 3, 2, 2
    n_out = (nlat - lat0) // fy
    bands = [coarse_lat_band(nlat, fy, lat0, r, world) for r in range(world)]
    assert bands[0][0] == lat0 and bands[-1][1] == lat0 + n_out * fy
    assert all(a[1] == b[0] for a, b in zip(bands[:-1], bands[1:]))
    assert all((i0 - lat0) % fy == 0 and (i1 - lat0) % fy == 0 and i1 > i0 for i0, i1 in bands)
    lat, lon = np.linspace(88.0, -88.0, nlat), np.arange(nlon) * 30.0
    kern = cr.CoarsenDouble()
    fine = _field(2, P, nlat, nlon, seed=9).reshape(2, P, nlat, nlon)
    whole = Coarsen(lat, lon, fy, fx, lat0=lat0, weights="band", kern=kern)
    w_all = whole.weights
    want = whole.apply([torch.from_numpy(fine.reshape(2, -1))], P)[0].numpy().reshape(2, P, n_out, nlon // fx)
    parts = []
    for i0, i1 in bands:
        cz = Coarsen(lat[i0:i1], lon, fy, fx, weights=w_all[i0:i1], kern=kern)
        block = np.ascontiguousarray(fine[:, :, i0:i1]).reshape(2, -1)
        parts.append(cz.apply([torch.from_numpy(block)], P)[0].numpy().reshape(2, P, (i1 - i0) // fy, nlon // fx))
    assert np.array_equal(_bits(np.concatenate(parts, axis=2)), _bits(want))
    with pytest.raises(ValueError, match="ranks"):
        coarse_lat_band(nlat, fy, lat0, 0, n_out + 1)
    with pytest.raises(ValueError):
        coarse_lat_band(nlat, fy, lat0, world, world)


# ---------------------------------------------------------------- the C ABI without a GPU
@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "dmd_era5_amd", "libdmdx.so")
    if not os.path.exists(so):
        import __graft_entry__

        __graft_entry__.build()
    from dmd_era5_amd import _lib

    return _lib.load()


def test_cabi_refusals_without_a_gpu(lib):
    assert lib.dmdx_coarsen_max_factor() == 64
    # host memory stands in for the operands: a refused call touches none of it
    T, P, nlat, nlon, fy, fx = 3, 2, 9, 14, 2, 4
    ldp, NLAT_, NLON_ = nlat * nlon + 2, 4, 3
    ldq = NLAT_ * NLON_ + 1
    ldx, ldy = (P - 1) * ldp + nlat * nlon + 3, (P - 1) * ldq + NLAT_ * NLON_ + 2
    xbuf = (ctypes.c_float * (T * ldx + 64))()
    ybuf = (ctypes.c_float * (T * ldy + 64))()
    wbuf = (ctypes.c_double * nlat)()
    X, Y, W = ctypes.addressof(xbuf), ctypes.addressof(ybuf), ctypes.addressof(wbuf)
    good = dict(X=X, T=T, ldx=ldx, P=P, ldp=ldp, nlat=nlat, nlon=nlon, w=W, fy=fy, fx=fx, lat0=1, lon0=2, NLAT=NLAT_,
                NLON=NLON_, skipna=0, min_frac=0.5, Y=Y, ldy=ldy, ldq=ldq)
    big = 2 ** 31
    xbytes = 4 * ((T - 1) * ldx + (P - 1) * ldp + nlat * nlon)
    ybytes = 4 * ((T - 1) * ldy + (P - 1) * ldq + NLAT_ * NLON_)
    bad = [dict(X=None), dict(w=None), dict(Y=None), dict(T=-1), dict(P=-1), dict(nlat=-1), dict(nlon=-1), dict(NLAT=-1),
           dict(NLON=-1), dict(ldx=-1), dict(ldp=-1), dict(ldy=-1), dict(ldq=-1),
           dict(fy=0), dict(fx=0), dict(fy=65), dict(fx=65), dict(fy=-2), dict(lat0=-1), dict(lon0=-1),
           dict(NLAT=5), dict(NLON=4), dict(lat0=2), dict(lon0=3), dict(lat0=nlat + 1, NLAT=0), dict(lon0=nlon + 1, NLON=0),
           dict(ldp=nlat * nlon - 1), dict(ldq=NLAT_ * NLON_ - 1), dict(ldx=(P - 1) * ldp + nlat * nlon - 1),
           dict(ldy=(P - 1) * ldq + NLAT_ * NLON_ - 1),
           dict(T=big), dict(P=big), dict(nlat=big), dict(nlon=big), dict(ldx=big), dict(ldy=big), dict(ldp=big), dict(ldq=big),
           dict(NLAT=big), dict(NLON=big),
           dict(T=big - 1, ldx=big - 1), dict(T=big - 1, ldy=big - 1),
           dict(min_frac=-0.1), dict(min_frac=1.0001), dict(min_frac=float("nan")),
           dict(X=X + 2), dict(Y=Y + 1), dict(w=W + 4),
           dict(Y=X), dict(Y=X + 16), dict(Y=X + xbytes - 4), dict(Y=X - ybytes + 4)]
    for change in bad:
        assert lib.dmdx_coarsen_f32(*{**good, **change}.values(), None) == -1000, change
        assert b"coarsen" in lib.dmdx_last_error(), (change, lib.dmdx_last_error())
    assert b"overlap" in lib.dmdx_last_error()
    # empty shapes: the checks, then nothing to do -- no launch, so no GPU is needed for these either
    for change in (dict(T=0), dict(P=0), dict(NLAT=0), dict(NLON=0), dict(NLAT=0, NLON=0, nlat=0, nlon=0, lat0=0, lon0=0, ldp=0)):
        assert lib.dmdx_coarsen_f32(*{**good, **change}.values(), None) == 0, (change, lib.dmdx_last_error())
    assert lib.dmdx_coarsen_f32(*{**good, "T": 0, "fy": 0}.values(), None) == -1000
    assert not any(xbuf) and not any(ybuf)
