"""K28 without a GPU: the geometry regrid.Remap forms on the host (tables of the ERA5 grid, conservation, the edge cases of
regional, descending and finer targets, the refusals, row shards), tests/remap_ref.py against tests/coarsen_ref.py on
block tables, and Remap.apply through the host double: round trips and the chain behind it."""
import numpy as np
import pytest
import torch

import coarsen_ref as cr
import remap_ref as rr
from dmd_era5_amd import io_netcdf
from dmd_era5_amd.regrid import Remap, lat_weights, remap_lat_band


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _tables(rm):
    return rm.iy0, rm.ny, rm.wy, rm.jx0, rm.nx, rm.wx


def _valid(w, n):
    return np.arange(w.shape[1])[None, :] < n[:, None]


def _dense(first, count, w, n_src):
    """(n_target, n_src) fp64: the table as a matrix (wrapped columns land where they belong)."""
    M = np.zeros((first.shape[0], n_src))
    for c in range(first.shape[0]):
        for k in range(int(count[c])):
            M[c, (int(first[c]) + k) % n_src] += w[c, k]
    return M


def _cell_centred(first_edge, last_edge, n):
    """n evenly spaced centres whose outer edges are first_edge and last_edge."""
    d = (last_edge - first_edge) / n
    return first_edge + d * (np.arange(n) + 0.5)


ERA5_LAT, ERA5_LON = 90.0 - 0.25 * np.arange(721), 0.25 * np.arange(1440)


# ---------------------------------------------------------------- geometry on the ERA5 grid
def test_geometry_of_the_era5_grid_at_one_degree():
    rm = Remap.regular(ERA5_LAT, ERA5_LON, 1, 1, weights="none")
    assert rm.shape_in == (721, 1440) and rm.shape_out == (181, 360)
    assert np.array_equal(rm.latitude_out, 90.0 - np.arange(181)) and np.array_equal(rm.longitude_out, np.arange(360.0))
    assert rm.rows_in(3) == 3 * 721 * 1440 and rm.rows_out(3) == 3 * 181 * 360
    # interior rows: five source rows, the end ones cut in half; the pole caps: three
    assert (rm.ny[1:-1] == 5).all() and rm.ny[0] == 3 and rm.ny[-1] == 3 and rm.wy.shape == (181, 5)
    assert np.array_equal(rm.iy0[:3], [0, 2, 6]) and rm.iy0[-1] == 718
    assert all(np.array_equal(rm.wy[I], [0.125, 0.25, 0.25, 0.25, 0.125]) for I in range(1, 180))
    assert np.array_equal(rm.wy[0, :3], [0.125, 0.25, 0.125]) and np.array_equal(rm.wy[180, :3], [0.125, 0.25, 0.125])
    # column 0 is centred on 0 degrees and reaches back to 359.5: it wraps
    assert rm.jx0[0] == 1438 and (rm.nx == 5).all() and rm.jx0[1] == 2 and rm.jx0[-1] == 1434
    assert np.abs(np.where(_valid(rm.wx, rm.nx), rm.wx, 0.0).sum(axis=1) - 1.0).max() <= 1e-12
    # no span holds a sliver: every kept overlap is a real share of a 0.25 degree cell
    assert rm.wx[_valid(rm.wx, rm.nx)].min() >= 0.1 and rm.wy[_valid(rm.wy, rm.ny)].min() >= 0.1
    band = Remap.regular(ERA5_LAT, ERA5_LON, 1, 1)
    assert band.kind == "band" and all(np.array_equal(a, b) for a, b in zip(_tables(band)[3:], _tables(rm)[3:]))
    assert np.array_equal(band.iy0, rm.iy0) and np.array_equal(band.ny, rm.ny)
    assert abs(band.weights_out.sum() - 2.0) <= 1e-14
    assert np.abs(band.weights_out - lat_weights(band.latitude_out, "band")).max() <= 1e-15
    w = band.row_weights_out(2)
    assert w.dtype == torch.float32 and w.shape == (2 * 181 * 360,) and float(w[0]) == np.float32(band.weights_out[0])
    # the other grids people compare on: 1.5 degrees with the poles, 5.625 degrees offset by half a cell
    wb = Remap.regular(ERA5_LAT, ERA5_LON, 1.5, 1.5)
    assert wb.shape_out == (121, 240) and wb.nx.max() == 7 and wb.jx0[0] == 1437
    off = Remap.regular(ERA5_LAT, ERA5_LON, 5.625, 5.625, poles=False)
    assert off.shape_out == (32, 64) and off.latitude_out[0] == 87.1875 and off.nx.max() <= 24 and off.ny.max() <= 24
    assert abs(off.weights_out.sum() - 2.0) <= 1e-14


@pytest.mark.parametrize("descending", (True, False))
def test_conservation(descending):
    """The defining property: the area-weighted mean of the remapped field is that of the source, and a field that is
    linear in sin(latitude) is reproduced as its exact cell means.  fp64 throughout, the remapping as two dense matrices.
    The tolerance is 1e-12 relative: two fp64 sums of 10^6 terms."""
    lat = ERA5_LAT if descending else ERA5_LAT[::-1].copy()
    rm = Remap.regular(lat, ERA5_LON, 1, 1)
    A, B = _dense(rm.iy0, rm.ny, rm.wy, 721), _dense(rm.jx0, rm.nx, rm.wx, 1440)
    ws = lat_weights(lat, "band")
    assert np.abs(A.sum(axis=0) - ws).max() <= 1e-15               # every source row is handed out exactly once
    assert np.abs(B.sum(axis=0) - 0.25).max() <= 1e-15
    F = 250.0 + 30.0 * np.random.RandomState(0).standard_normal((721, 1440))
    Y = (A @ F @ B.T) / np.outer(A.sum(axis=1), B.sum(axis=1))
    src = (ws[:, None] * F).sum() / (ws.sum() * 1440)
    dst = (rm.weights_out[:, None] * Y).sum() / (rm.weights_out.sum() * 360)
    assert abs(dst - src) <= 1e-12 * abs(src)
    # Linear in sin(latitude): the mean over a band lo .. hi is a + b (sin hi + sin lo) / 2, for source and target cells.
    # A first-order scheme takes the source as constant inside a source cell, so it returns the exact cell means where
    # the target edges fall on source edges; the half cells a 1 degree node-centred target cuts off the 0.25 degree
    # rows leave a second-order term (3e-5 here), and what holds on that grid is the conservation above.  So this
    # property is checked on the cell-centred 0.25 degree grid (720 rows, no pole row) against 1 degree cells.
    def band_means(centres):
        step = centres[1] - centres[0]
        e = np.sin(np.deg2rad(np.clip(np.concatenate([[centres[0] - 0.5 * step], 0.5 * (centres[:-1] + centres[1:]),
                                                      [centres[-1] + 0.5 * step]]), -90.0, 90.0)))
        return 3.0 + 7.0 * 0.5 * (e[:-1] + e[1:])
    s = 1.0 if descending else -1.0
    cc = Remap(_cell_centred(s * 90.0, -s * 90.0, 720), ERA5_LON, _cell_centred(s * 90.0, -s * 90.0, 180), np.arange(360.0))
    assert (cc.ny == 4).all() and cc.jx0[0] == 1438
    A, B = _dense(cc.iy0, cc.ny, cc.wy, 720), _dense(cc.jx0, cc.nx, cc.wx, 1440)
    G = np.repeat(band_means(cc.latitude)[:, None], 1440, axis=1)
    Yg = (A @ G @ B.T) / np.outer(A.sum(axis=1), B.sum(axis=1))
    assert np.abs(Yg - band_means(cc.latitude_out)[:, None]).max() <= 1e-12 * 10.0


# ---------------------------------------------------------------- the reference against K23's
@pytest.mark.parametrize("fy,fx", ((1, 1), (2, 2), (4, 4), (3, 5)))
@pytest.mark.parametrize("skipna", (False, True))
def test_block_tables_give_the_bits_of_the_coarsen_reference(fy, fx, skipna):
    T, P, nlat, nlon, lat0, lon0 = 3, 2, 14, 23, 1, 2
    NLAT, NLON = (nlat - lat0) // fy, (nlon - lon0) // fx
    rs = np.random.RandomState(fy + 10 * fx)
    ldp = nlat * nlon + 3
    X = (250.0 + 30.0 * rs.standard_normal((T, (P - 1) * ldp + nlat * nlon))).astype(np.float32)
    if skipna:
        X[rs.uniform(size=X.shape) < 0.2] = np.nan
        X[rs.uniform(size=X.shape) < 0.03] = -np.inf
    w = np.cos(np.deg2rad(np.linspace(80.0, -70.0, nlat))) + 0.01 * rs.uniform(size=nlat)
    for min_frac in (0.0, 0.5, 1.0):
        want = cr.coarsen(X, P, nlat, nlon, w, fy, fx, ldp=ldp, lat0=lat0, lon0=lon0, skipna=skipna, min_frac=min_frac)
        got = rr.remap(X, P, nlat, nlon, *rr.block_tables(w, fy, fx, NLAT, NLON, lat0, lon0), ldp=ldp, skipna=skipna,
                       min_frac=min_frac)
        assert np.array_equal(_bits(got), _bits(want))
    # ... and so does Remap.blocks, the same tables from the class
    lat, lon = np.linspace(80.0, -70.0, nlat), np.arange(nlon) * 10.0
    rb = Remap.blocks(lat, lon, fy, fx, lat0=lat0, lon0=lon0, weights=w, skipna=skipna, min_frac=0.5, kern=rr.RemapDouble())
    for a, b in zip(_tables(rb), rr.block_tables(w, fy, fx, NLAT, NLON, lat0, lon0)):
        assert np.array_equal(a, b)
    got = rb.apply([torch.from_numpy(X[:, :P * nlat * nlon].copy())], P)[0].numpy()
    want = cr.coarsen(X[:, :P * nlat * nlon], P, nlat, nlon, w, fy, fx, lat0=lat0, lon0=lon0, skipna=skipna, min_frac=0.5)
    assert np.array_equal(_bits(got), _bits(want))


def test_reference_ignores_what_lies_beyond_the_counts_and_keeps_constants():
    rm = Remap.regular(90.0 - 15.0 * np.arange(13), 22.5 * np.arange(16), 30, 45)
    assert rm.shape_out == (7, 8) and rm.jx0[0] == 15 and rm.ny[0] == 2 and rm.ny[3] == 3
    X = (250.0 + 30.0 * np.random.RandomState(1).standard_normal((2, 2 * 13 * 16))).astype(np.float32)
    want = rr.remap(X, 2, 13, 16, *_tables(rm))
    wy, wx = rm.wy.copy(), rm.wx.copy()
    wy[~_valid(wy, rm.ny)], wx[~_valid(wx, rm.nx)] = np.nan, np.nan
    assert np.array_equal(_bits(rr.remap(X, 2, 13, 16, rm.iy0, rm.ny, wy, rm.jx0, rm.nx, wx)), _bits(want))
    const = rr.remap(np.full_like(X, 287.654), 2, 13, 16, *_tables(rm))
    assert (_bits(const) == _bits(np.float32(287.654))).all()
    for e in (-20, 20):
        assert np.array_equal(_bits(rr.remap(np.ldexp(X, e), 2, 13, 16, *_tables(rm))), _bits(np.ldexp(want, e)))


# ---------------------------------------------------------------- regional, descending, finer targets
def test_regional_source_and_finer_target():
    # 9 x 12 cells of 2 x 2.5 degrees, not periodic -> 4 x 5 cells over the same domain: ratios 2.25 and 2.4
    lat, lon = _cell_centred(60.0, 42.0, 9), _cell_centred(10.0, 40.0, 12)
    lat_out, lon_out = _cell_centred(60.0, 42.0, 4), _cell_centred(10.0, 40.0, 5)
    rm = Remap(lat, lon, lat_out, lon_out, weights="none")
    assert rm.shape_out == (4, 5) and rm.wy.shape[1] == 3 and rm.wx.shape[1] == 4
    assert np.array_equal(rm.iy0, [0, 2, 4, 6]) and np.array_equal(rm.ny, [3, 3, 3, 3])
    assert np.array_equal(rm.jx0, [0, 2, 4, 7, 9]) and np.array_equal(rm.nx, [3, 3, 4, 3, 3])
    assert np.abs(rm.wy[0, :3] - [2.0, 2.0, 0.5]).max() <= 1e-12 and np.abs(rm.wx[2] - [0.5, 2.5, 2.5, 0.5]).max() <= 1e-12
    assert np.abs(_dense(rm.iy0, rm.ny, rm.wy, 9).sum(axis=0) - 2.0).max() <= 1e-12
    assert np.abs(_dense(rm.jx0, rm.nx, rm.wx, 12).sum(axis=0) - 2.5).max() <= 1e-12
    # ascending latitudes: the same cells in the other order
    up = Remap(lat[::-1].copy(), lon, lat_out[::-1].copy(), lon_out, weights="none")
    assert np.array_equal(up.ny, rm.ny[::-1]) and np.abs(up.wy[3, :3] - [0.5, 2.0, 2.0]).max() <= 1e-12
    # a target that runs against the source: it follows what it is given
    mixed = Remap(lat, lon, lat_out[::-1].copy(), lon_out, weights="none")
    assert np.array_equal(mixed.iy0, rm.iy0[::-1]) and np.array_equal(mixed.wy, rm.wy[::-1])
    # 5 x 8 -> 9 x 16: a finer target, spans of one and two
    fine = Remap(_cell_centred(50.0, 40.0, 5), _cell_centred(0.0, 16.0, 8), _cell_centred(50.0, 40.0, 9), _cell_centred(0.0, 16.0, 16))
    assert fine.shape_out == (9, 16) and set(fine.ny) == {1, 2} and (fine.nx == 1).all()
    assert np.array_equal(fine.jx0, np.arange(16) // 2)
    X = np.random.RandomState(3).standard_normal((1, 40)).astype(np.float32)
    got = rr.remap(X, 1, 5, 8, *_tables(fine)).reshape(9, 16)
    assert np.array_equal(_bits(got[0]), _bits(np.repeat(X.reshape(5, 8)[0], 2)))    # a cell inside one source cell: that value


def test_value_errors():
    lat, lon = 90.0 - 15.0 * np.arange(13), 22.5 * np.arange(16)
    reg_lat, reg_lon = _cell_centred(60.0, 42.0, 9), _cell_centred(10.0, 40.0, 12)
    with pytest.raises(ValueError, match="not covered"):                            # a column half outside a regional source
        Remap(reg_lat, reg_lon, _cell_centred(60.0, 42.0, 4), _cell_centred(9.0, 39.0, 5))
    with pytest.raises(ValueError, match="not covered"):                            # a row beyond it
        Remap(reg_lat, reg_lon, _cell_centred(62.0, 42.0, 4), _cell_centred(10.0, 40.0, 5))
    with pytest.raises(ValueError, match="spans 65"):                               # 0.25 -> 16.25 degrees
        Remap(ERA5_LAT, ERA5_LON[:1300], 90.0 - 15.0 * np.arange(13), _cell_centred(-0.125, 324.875, 20))
    wide = Remap(ERA5_LAT, ERA5_LON[:1280], 90.0 - 15.0 * np.arange(13), _cell_centred(-0.125, 319.875, 20))
    assert wide.ny.max() == 61 and (wide.nx == 64).all()                           # the widest span that is taken
    for bad_lat in (np.array([90.0, 60.0, 45.0, 0.0, -90.0]), np.array([10.0, 10.0, 10.0])):
        with pytest.raises(ValueError, match="evenly"):
            Remap(bad_lat, lon, np.array([50.0, 40.0]), lon)
    with pytest.raises(ValueError, match="evenly"):
        Remap(lat, np.array([0.0, 90.0, 200.0, 270.0]), lat, lon)
    with pytest.raises(ValueError, match="evenly"):
        Remap(lat, lon, lat, np.array([0.0, 90.0, 200.0, 270.0]))
    with pytest.raises(ValueError, match="ascend"):
        Remap(lat, lon[::-1].copy(), lat, lon)
    with pytest.raises(ValueError, match="one-dimensional"):
        Remap(lat.reshape(1, -1), lon, lat, lon)
    with pytest.raises(ValueError, match="one-dimensional"):
        Remap(lat, lon, lat, lon.reshape(2, 8))
    with pytest.raises(ValueError, match="weights"):
        Remap(lat, lon, lat, lon, weights="cos")
    with pytest.raises(ValueError, match="min_frac"):
        Remap(lat, lon, lat, lon, min_frac=1.5)
    with pytest.raises(ValueError, match="lat_edges"):
        Remap(lat, lon, lat, lon, lat_edges=np.linspace(90, -90, 13))
    with pytest.raises(ValueError, match="divide"):
        Remap.regular(lat, lon, 7.0, 45.0)
    with pytest.raises(ValueError, match="divide"):
        Remap.regular(lat, lon, 30.0, 50.0)
    # apply checks everything before the first launch
    kern = rr.RemapDouble()
    rm = Remap.regular(lat, lon, 30, 45, kern=kern)
    X = torch.zeros((2, 2 * 13 * 16))
    for args, text in ((([X], [2, 1]), "one positive count"), (([X], 0), "one positive count"), (([X[0]], 2), "time, rows"),
                       (([X], 3), "need")):
        with pytest.raises(ValueError, match=text):
            rm.apply(*args)
    with pytest.raises(ValueError, match="out holds"):
        rm.apply([X], 2, out=[])
    with pytest.raises(ValueError, match="asked for"):
        rm.apply([X], 2, out=[torch.zeros((2, 5))])
    with pytest.raises(ValueError, match="vector"):
        rm.apply_field(X, 2)
    assert kern.calls == []


# ---------------------------------------------------------------- row shards
@pytest.mark.parametrize("world", (1, 2, 3, 7))
def test_lat_bands_give_the_global_result(world):
    lat, lon = 90.0 - 2.5 * np.arange(73), 5.0 * np.arange(72)
    lat_out, lon_out, P = 90.0 - 5.0 * np.arange(37), 15.0 * np.arange(24), 2
    kern = rr.RemapDouble()
    whole = Remap(lat, lon, lat_out, lon_out, kern=kern)
    fine = (250.0 + 30.0 * np.random.RandomState(5).standard_normal((2, P, 73, 72))).astype(np.float32)
    want = whole.apply([torch.from_numpy(fine.reshape(2, -1))], P)[0].numpy().reshape(2, P, 37, 24)
    parts, bands = [], [remap_lat_band(lat, lat_out, r, world) for r in range(world)]
    assert bands[0][0][0] == 0 and bands[-1][0][1] == 37 and all(a[0][1] == b[0][0] for a, b in zip(bands[:-1], bands[1:]))
    assert all(a[1][1] > b[1][0] for a, b in zip(bands[:-1], bands[1:]))            # neighbours share the rows a boundary cuts
    for (I0, I1), (i0, i1), edges, edges_out in bands:
        assert edges.shape == (i1 - i0 + 1,) and edges_out.shape == (I1 - I0 + 1,)
        rm = Remap(lat[i0:i1], lon, lat_out[I0:I1], lon_out, lat_edges=edges, lat_edges_out=edges_out, kern=kern)
        n = int(whole.ny[I0:I1].max())
        assert np.array_equal(rm.iy0 + i0, whole.iy0[I0:I1]) and np.array_equal(rm.ny, whole.ny[I0:I1])
        assert np.array_equal(rm.wy.view(np.uint64), whole.wy[I0:I1, :n].view(np.uint64))
        block = np.ascontiguousarray(fine[:, :, i0:i1]).reshape(2, -1)
        parts.append(rm.apply([torch.from_numpy(block)], P)[0].numpy().reshape(2, P, I1 - I0, 24))
    assert np.array_equal(_bits(np.concatenate(parts, axis=2)), _bits(want))
    with pytest.raises(ValueError, match="ranks"):
        remap_lat_band(lat, lat_out, 0, 38)
    with pytest.raises(ValueError):
        remap_lat_band(lat, lat_out, world, world)


# ---------------------------------------------------------------- through the class: round trips and the chain
def test_apply_through_the_host_double_and_round_trips(tmp_path):
    lat, lon = 90.0 - 15.0 * np.arange(13), 22.5 * np.arange(16)
    kern = rr.RemapDouble()
    rm = Remap.regular(lat, lon, 30, 45, skipna=True, min_frac=0.4, kern=kern)
    rs = np.random.RandomState(7)
    host = [(250.0 + 30.0 * rs.standard_normal((3, 2 * 208))).astype(np.float32),
            np.concatenate([(250.0 + 30.0 * rs.standard_normal((3, 208))).astype(np.float32), np.full((3, 3), np.nan, np.float32)], axis=1)]
    host[0][1, 40:44] = np.nan
    X = [torch.from_numpy(h) for h in host]
    Y = rm.apply(X, [2, 1])
    assert kern.calls == [((3, 416), 2, (7, 3), (8, 3)), ((3, 211), 1, (7, 3), (8, 3))]
    for y, h, p in zip(Y, host, (2, 1)):
        want = rr.remap(h, p, 13, 16, *_tables(rm), skipna=True, min_frac=0.4)
        assert y.shape == (3, rm.rows_out(p)) and np.array_equal(_bits(y.numpy()), _bits(want))
    out = [torch.zeros((3, rm.rows_out(2))), torch.zeros((3, rm.rows_out(1)))]
    Y2 = rm.apply(iter(X), (2, 1), out=out)
    assert all(a is b for a, b in zip(Y2, out)) and all(np.array_equal(_bits(a.numpy()), _bits(b.numpy())) for a, b in zip(Y, Y2))
    f = rm.apply_field(X[1][0], 1)
    assert f.shape == (rm.rows_out(1),) and np.array_equal(_bits(f.numpy()), _bits(Y[1][0].numpy()))
    ds = rm.to_dataset()
    assert ds["remap_wy"].dims == ("latitude_out", "span_y") and ds["remap_wx"].dims == ("longitude_out", "span_x")
    path = str(tmp_path / "remap.nc")
    rm.to_netcdf(path)
    for back in (Remap.from_dataset(ds, kern), Remap.from_netcdf(path, kern), Remap.from_dataset(io_netcdf.open_dataset(path), kern)):
        assert (back.kind, back.skipna, back.min_frac) == ("band", True, 0.4)
        for a, b in zip(_tables(back), _tables(rm)):
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
        assert np.array_equal(back.latitude, lat) and np.array_equal(back.longitude_out, rm.longitude_out)
        for a, b in zip(back.apply(X, [2, 1]), Y):
            assert np.array_equal(_bits(a.numpy()), _bits(b.numpy()))


def test_the_chain_behind_it_takes_the_blocks_as_they_are():
    """Remap.apply -> Climatology.fit and svd_snapshots, without a reshape in between."""
    from kernel_double import CpuKernelDouble
    from test_climatology import ClimDouble

    from dmd_era5_amd.climatology import Climatology
    from dmd_era5_amd.svd import svd_snapshots

    lat, lon = 90.0 - 15.0 * np.arange(13), 22.5 * np.arange(16)
    rm = Remap.regular(lat, lon, 30, 45, kern=rr.RemapDouble())
    rs = np.random.RandomState(11)
    T = 48
    X = [torch.from_numpy((rs.standard_normal((T, p * 208)) + 5.0 * np.sin(np.arange(T) * 2 * np.pi / 24)[:, None]).astype(np.float32))
         for p in (2, 1)]
    Y = rm.apply(X, [2, 1])
    times = np.datetime64("2020-03-01T00", "h") + np.arange(T) * np.timedelta64(1, "h")
    clim = Climatology.fit(Y, times, "hour", kern=ClimDouble())
    assert [tuple(m.shape) for m in clim.mean] == [(24, 2 * 56), (24, 56)]
    res = svd_snapshots(Y, 3, kern=CpuKernelDouble())
    assert res.s.shape == (3,)
    full = np.concatenate([y.numpy() for y in Y], axis=1).astype(np.float64)
    assert np.allclose(res.s.numpy(), np.linalg.svd(full, compute_uv=False)[:3], rtol=1e-4)
