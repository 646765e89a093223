"""K18 through the package on the GPU: fit -> remove_ -> svd -> DmdForecast -> write_forecast_slice(climatology=) on a
35 x 71 grid with 2 variables and 96 hourly snapshots, kind = "hour"."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
NLAT, NLON, NVAR, T = 35, 71, 2, 96
PLANE = NLAT * NLON
M = NVAR * PLANE
SPLIT = [(0, 2000), (2000, M)]                                  # cuts through the first variable
NAMES = ["temperature", "u_component_of_wind"]
K = 6


def _snapshots():
    """A diurnal cycle per grid point on top of a level, three damped oscillations and a little noise."""
    rs = np.random.RandomState(7)
    h = np.arange(T, dtype=np.float64)
    level = np.concatenate([250.0 + 30.0 * rs.rand(PLANE), 8.0 * rs.standard_normal(PLANE)])
    amp, phase = 1.0 + 4.0 * rs.rand(M), 2 * np.pi * rs.rand(M)
    cycle = amp[None, :] * np.cos(2 * np.pi * h[:, None] / 24.0 + phase[None, :])
    half = np.array([-0.004 + 0.11j, -0.01 + 0.31j, -0.002 + 0.05j])
    modes = rs.standard_normal((3, M)) + 1j * rs.standard_normal((3, M))
    dyn = 2.0 * (np.exp(np.outer(h, half)) @ modes).real
    return (level[None, :] + cycle + dyn + 0.01 * rs.standard_normal((T, M))).astype(np.float32)


def test_fit_remove_svd_forecast_and_write_with_a_climatology(svd_base_config, project_root, monkeypatch):
    from dmd_era5_amd import bopdmd as bop
    from dmd_era5_amd import era5_svd, hdf5_lite
    from dmd_era5_amd import svd as dsvd
    from dmd_era5_amd.climatology import Climatology
    from dmd_era5_amd.config_parser import config_parser
    from dmd_era5_amd.forecast import DmdForecast, expand_blocks, pack_blocks

    if not hdf5_lite.available():
        pytest.skip("libhdf5 not found")
    monkeypatch.setenv("DMDX_NETCDF_BACKEND", "hdf5")
    X = torch.from_numpy(_snapshots()).to(DEV)
    Xb = [X[:, a:b].contiguous() for a, b in SPLIT]
    times = np.datetime64("2019-01-01T00", "h") + np.arange(T) * np.timedelta64(1, "h")

    clim = Climatology.fit(Xb, times, "hour")
    assert clim.counts.tolist() == [4] * 24 and [tuple(m.shape) for m in clim.mean] == [(24, b - a) for a, b in SPLIT]
    grouped = X.cpu().numpy().astype(np.float64).reshape(4, 24, M).mean(axis=0)
    assert np.abs(torch.cat(clim.mean, dim=1).cpu().numpy() - grouped).max() <= 1e-4
    clim.remove_(Xb, times)
    assert float(torch.cat(Xb, dim=1).abs().max()) < 100.0     # the levels (250 K) are gone

    res = dsvd.svd_snapshots(Xb, K)
    H = bop.reduced_coordinates(res.s, res.Vh)
    hours = torch.arange(T, dtype=torch.float64, device=DEV)
    dmd = bop.optdmd(H.to(torch.complex128).to(DEV), hours, K, tol=1e-8, maxiter=40)
    Ub = [res.Ut[:, a:b] for a, b in SPLIT]
    f = DmdForecast(Ub, dmd)

    Tf = 24
    tt = np.arange(90.0, 90.0 + Tf)
    valid = times[0] + tt.astype(np.int64) * np.timedelta64(1, "h")
    cfg = dict(svd_base_config, start_datetime="2019-01-04T18", end_datetime="2019-01-05T17",
               variables=",".join(NAMES), levels="1000")
    p = config_parser(cfg, "era5-svd")
    grid = dict(levels=[1000], latitude=np.linspace(60.0, 26.0, NLAT), longitude=np.linspace(0.0, 17.5, NLON))
    out = era5_svd.write_forecast_slice(p["era5_slice_path"], f, tt, valid, NAMES, **grid, slab=7, climatology=clim,
                                        attrs={"source_path": p["source_path"]})
    ds, _ = era5_svd.retrieve_era5_slice(p)
    assert ds is not None
    Ct = f.coefficients(torch.from_numpy(tt))[0]
    want = (torch.cat(expand_blocks(Ub, Ct), dim=1) + torch.cat(clim.at(valid), dim=1)).cpu().numpy()
    full = torch.cat(f.fields(torch.from_numpy(tt), climatology=clim, times=valid), dim=1).cpu().numpy()
    assert np.array_equal(full.view(np.uint32), want.view(np.uint32))
    for g, name in enumerate(NAMES):
        pk = out["packing"][name]
        w = want[:, g * PLANE:(g + 1) * PLANE].reshape(Tf, 1, NLAT, NLON)
        got = np.asarray(ds[name].values)
        assert got.shape == w.shape and (out["filled"][name], out["saturated"][name]) == (0, 0)
        assert np.abs(got.astype(np.float64) - w).max() <= pk.scale_factor

    # without a climatology: today's path, the file bytes of pack_blocks
    plain = str(project_root / "plain.nc")
    out0 = era5_svd.write_forecast_slice(plain, f, tt, valid, NAMES, **grid, slab=7)
    groups = [torch.arange(a, b) // PLANE for a, b in SPLIT]
    ref = pack_blocks(Ub, Ct, groups=groups, delay_block=None, n_groups=NVAR)
    codes = torch.cat(ref["codes"], dim=1).cpu().numpy()
    r = hdf5_lite.Reader(plain)
    for g, name in enumerate(NAMES):
        assert (out0["packing"][name].scale_factor, out0["packing"][name].add_offset) == \
            (ref["packing"][g].scale_factor, ref["packing"][g].add_offset)
        assert np.array_equal(r.read(name), codes[:, g * PLANE:(g + 1) * PLANE].reshape(Tf, 1, NLAT, NLON))
    r.close()
