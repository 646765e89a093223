"""The packed ingest on the GPU: int16 codes travel to HBM and K14 unpacks them there.

One field on a 3-level 35 x 71 grid (2485 points per level: no multiple of 4), 41 snapshots, stored
twice by the project's own writer: as int16 codes with scale_factor / add_offset / _FillValue /
missing_value, and as the decoded float32 values (tests/unpack_ref.py).  Whatever route the two files
take through the ingest, the same float32 matrix must arrive in HBM, bit for bit.
"""
import numpy as np
import pytest
import torch

import unpack_ref as ur

pytestmark = pytest.mark.gpu

FILL, MISSING = -32767, 12345
NT, NLEV, NLAT, NLON = 41, 3, 35, 71
VARS = ("temperature", "u_component_of_wind")


def _fields():
    """Mock fields with three planted space-time patterns (a separated spectrum), as float64, and noise well
    above the packing step everywhere (the mock temperature is 0 at the poles: rows that are constant after
    quantisation would have no standard deviation to scale by)."""
    from dmd_era5_amd.create_mock_data import create_mock_era5

    full = create_mock_era5("2019-01-01T00", "2019-01-02T16", list(VARS), [1000, 850, 500], seed=21, dtype=np.float32)
    assert full[VARS[0]].shape[0] == NT
    t = np.arange(NT, dtype=np.float64)[:, None, None, None]
    lat = np.radians(full.coords["latitude"].values[:NLAT])[None, None, :, None]
    lon = np.radians(full.coords["longitude"].values[:NLON])[None, None, None, :]
    out, rs = {}, np.random.RandomState(5)
    for v, name in enumerate(VARS):
        f = full[name].values[:, :, :NLAT, :NLON].astype(np.float64) + rs.standard_normal((NT, 3, NLAT, NLON))
        f = f + 60 * np.sin(2 * np.pi * t / 24) * np.cos(lat) * np.cos(lon + v) + 35 * np.cos(2 * np.pi * t / 11) * np.sin(2 * lat) * np.sin(2 * lon)
        out[name] = f + 20 * (t / NT) ** 2 * np.cos(3 * lon) * np.ones_like(lat)
    return full, out


def _datasets(fill_at=()):
    """-> (packed Dataset, decoded float32 Dataset)."""
    from dmd_era5_amd.labeled import Coord, DataArray, Dataset

    full, fields = _fields()
    cds = {"time": full.coords["time"], "level": full.coords["level"],
           "latitude": Coord("latitude", full.coords["latitude"].values[:NLAT]),
           "longitude": Coord("longitude", full.coords["longitude"].values[:NLON])}
    packed, plain = Dataset(coords=cds, attrs=dict(full.attrs)), Dataset(coords=cds, attrs=dict(full.attrs))
    for name, f in fields.items():
        lo, hi = float(f.min()), float(f.max())
        sf, ao = (hi - lo) / 65000.0, (hi + lo) / 2.0
        q = ur.pack(f, sf, ao)
        q[(q == FILL) | (q == MISSING)] = 0
        for i, idx in enumerate(x[1:] for x in fill_at if x[0] == name):
            q[idx] = FILL if i == 0 else MISSING
        attrs = dict(full[name].attrs, scale_factor=np.float64(sf), add_offset=np.float64(ao),
                     _FillValue=np.int16(FILL), missing_value=np.int16(MISSING))
        packed[name] = DataArray(q, full[name].dims, cds, attrs)
        plain[name] = DataArray(ur.decode(q, sf, ao, (FILL, MISSING)), full[name].dims, cds, dict(full[name].attrs))
    return packed, plain


@pytest.fixture
def small_slabs(monkeypatch):
    """Every variable file-backed, several slabs per variable on both routes."""
    from dmd_era5_amd import era5_svd, hdf5_lite, io_netcdf

    if not hdf5_lite.available():
        pytest.fail("libhdf5 not found: the packed route reads HDF5 slices")
    monkeypatch.setenv("DMDX_NETCDF_BACKEND", "hdf5")
    monkeypatch.setattr(io_netcdf, "LAZY_BYTES", 1000)
    monkeypatch.setattr(era5_svd, "SLAB_BYTES", 9 * NLEV * NLAT * NLON * 4)


@pytest.fixture
def files(tmp_path, small_slabs):
    from dmd_era5_amd import io_netcdf

    packed, plain = _datasets()
    pp, pf = str(tmp_path / "packed.nc"), str(tmp_path / "plain.nc")
    io_netcdf.to_netcdf(packed, pp)
    io_netcdf.to_netcdf(plain, pf)
    return io_netcdf.open_dataset(pp), io_netcdf.open_dataset(pf)


class _Counting:
    """The HIP kernel provider with its K14 launches counted (nothing else changed)."""

    def __init__(self, kern):
        self._kern, self.unpacks = kern, 0

    def __getattr__(self, name):
        return getattr(self._kern, name)

    def unpack_i16_(self, *a, **k):
        self.unpacks += 1
        return self._kern.unpack_i16_(*a, **k)


@pytest.mark.parametrize("pad4", [False, True], ids=["tight", "pad4"])
@pytest.mark.parametrize("take", ["contiguous", "stride3", "irregular"])
@pytest.mark.parametrize("levels", ["all", "subset"])
@pytest.mark.parametrize("band", [None, (5, 23)], ids=["whole", "band"])
def test_upload_variable_gives_the_same_row_blocks_from_both_files(files, band, levels, take, pad4):
    from dmd_era5_amd import svd as dsvd
    from dmd_era5_amd.era5_svd import _upload_variable
    from dmd_era5_amd.kernels import default_kernels

    dsp, dsf = files
    kern = _Counting(default_kernels())
    dev = torch.device("cuda", torch.cuda.current_device())
    level_idx = np.arange(NLEV) if levels == "all" else np.array([2, 1])
    tk = {"contiguous": np.arange(3, 36), "stride3": np.arange(1, 41, 3),
          "irregular": np.array([0, 1, 2, 4, 7, 8, 15, 16, 23, 40])}[take]
    name = VARS[0]
    assert dsp[name].lazy.dtype == np.int16 and dsf[name].lazy.dtype == np.float32
    sp, sf_ = {"mean": [], "std": []}, {"mean": [], "std": []}
    bp, mp, nbp = _upload_variable(dsp[name], level_idx, tk, dev, kern, False, False, sp, band, pad4)
    bf, mf, nbf = _upload_variable(dsf[name], level_idx, tk, dev, kern, False, False, sf_, band, pad4)
    torch.cuda.synchronize()
    nlat = NLAT if band is None else band[1] - band[0]
    assert mp == mf == len(level_idx) * nlat * NLON and len(bp) == len(bf) == len(dsvd.split_rows(mp))
    for a, b in zip(bp, bf):
        assert a.shape == b.shape and a.shape[0] == len(tk)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))          # pad rows included
    if pad4:
        assert sum(int(b.shape[1]) for b in bp) % 4 == 0 and sum(int(b.shape[1]) for b in bp) - mp == (-mp) % 4
    # the device route was taken for every arithmetic progression, the host decode for the rest
    nslabs = kern.unpacks // len(bp)
    assert (kern.unpacks > 0) == (take != "irregular") and kern.unpacks % len(bp) == 0
    assert int(sp["fills"][0][1]) == 0 and sp["fills"][0][0] == name and "fills" not in sf_
    # bytes moved: 4 per selected value from the float32 file; the packed call moves the codes of the level range it
    # reads (here exactly the selected levels) of the selected snapshots only, 2 per value -- also with a stride
    assert nbf == 4 * len(tk) * mp
    assert nbp == (nbf // 2 if take != "irregular" else nbf)             # (irregular: decoded on the host, moved as float32)
    if band is None and levels == "all" and take == "contiguous":
        assert nslabs > 1                                                    # (the slab loop and its two buffers are exercised)


def _main_cfg(base, svd_type, scale):
    return dict(base, start_datetime="2019-01-01T00", end_datetime="2019-01-02T16", variables=",".join(VARS),
                levels="1000,850,500", svd_type=svd_type, mean_center=True, scale=scale, delay_embedding=2,
                n_components=3, save_data_matrix=False, svd_seed=0)


def _main_on(root, monkeypatch, ds, cfg):
    from dmd_era5_amd import io_netcdf
    from dmd_era5_amd.config_parser import config_parser
    from dmd_era5_amd.create_mock_data import add_download_attributes
    from dmd_era5_amd.era5_svd import main

    root.mkdir(exist_ok=True)
    monkeypatch.setenv("DMD_ERA5_ROOT", str(root))
    p = config_parser(cfg, "era5-svd")
    io_netcdf.to_netcdf(add_download_attributes(ds, p), p["era5_slice_path"])
    res, _, _ = main(cfg, write_to_netcdf=True)
    back = io_netcdf.open_dataset(p["save_path"])
    return res, back


@pytest.mark.parametrize("svd_type, scale", [("standard", False), ("randomized", False), ("standard", True)])
def test_main_on_the_packed_file_agrees_with_the_float32_file(svd_base_config, tmp_path, monkeypatch, small_slabs,
                                                               svd_type, scale):
    """Tolerances: those of test_gpu_pipeline.py::test_main_streams_a_slice_that_does_not_fit, two routes of one
    computation (here the same float32 matrix reaches the SVD, so the results are normally identical)."""
    packed, plain = _datasets()
    cfg = _main_cfg(svd_base_config, svd_type, scale)
    a, a_file = _main_on(tmp_path / "plain", monkeypatch, plain, cfg)
    b, b_file = _main_on(tmp_path / "packed", monkeypatch, packed, cfg)
    assert sorted(a.data_vars) == sorted(b.data_vars)
    assert b["U"].values.dtype == a["U"].values.dtype == np.float32 and b["s"].values.dtype == np.float32
    assert np.allclose(b["s"].values, a["s"].values, rtol=1e-6 if svd_type == "standard" else 1e-5)
    assert np.abs(b["U"].values - a["U"].values).max() < 1e-4 * np.abs(a["U"].values).max()
    assert np.abs(b["V"].values - a["V"].values).max() < 1e-5
    assert np.abs(b_file["U"].values - a_file["U"].values).max() < 1e-4 * np.abs(a_file["U"].values).max()  # the written U
    assert np.array_equal(b_file["U"].values, b["U"].values)
    assert np.array_equal(b["X_mean"].values, a["X_mean"].values)
    if scale:
        assert np.allclose(b["X_std"].values, a["X_std"].values, rtol=1e-6)
    gap = np.min(np.abs(np.diff(a["s"].values))) / a["s"].values[0]
    assert gap > 0.01                                                         # (the vectors are comparable one by one)


def test_fill_codes_stop_the_run_before_any_svd_kernel(svd_base_config, tmp_path, monkeypatch, small_slabs):
    from dmd_era5_amd import io_netcdf
    from dmd_era5_amd.config_parser import config_parser
    from dmd_era5_amd.era5_svd import _device_pipeline, main
    from dmd_era5_amd.kernels import default_kernels

    fills = [(VARS[1], 0, 0, 0, 0), (VARS[1], 17, 2, 34, 70), (VARS[1], 40, 1, 11, 3)]
    packed, _ = _datasets(fills)
    path = str(tmp_path / "packed.nc")
    io_netcdf.to_netcdf(packed, path)
    cfg = _main_cfg(svd_base_config, "standard", False)
    p = config_parser(cfg, "era5-svd")
    kern = default_kernels()
    kern.events = []
    try:
        with pytest.raises(ValueError, match=r"u_component_of_wind: 3 missing values"):
            _device_pipeline(io_netcdf.open_dataset(path), p, None, kern, torch.device("cuda", torch.cuda.current_device()))
        torch.cuda.synchronize()
        names = [e[0] for e in kern.events]
    finally:
        kern.events = None
    assert "unpack_i16" in names and not any(n.startswith(("syrk", "gemm", "skinny")) for n in names), names
    # and through main(): the reference's wrapping of whatever the SVD stage raises
    from dmd_era5_amd.create_mock_data import add_download_attributes

    monkeypatch.setenv("DMD_ERA5_ROOT", str(tmp_path / "root"))
    p = config_parser(cfg, "era5-svd")
    io_netcdf.to_netcdf(add_download_attributes(packed, p), p["era5_slice_path"])
    with pytest.raises(Exception, match=r"u_component_of_wind: 3 missing values") as ei:
        main(cfg, write_to_netcdf=False)
    assert isinstance(ei.value.__cause__, ValueError)
