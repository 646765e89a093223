"""CF packing (int16 + scale_factor / add_offset / _FillValue / missing_value) on the host side:
the reader decodes it as ``xr.open_dataset`` does for the reference, the ingest's host branch
hands the decoded values to the pipeline, and missing values stop the run on every rank.

Packed fixtures are made with the project's own writer (``to_netcdf`` stores arrays as given); the
decode is compared bit for bit with tests/unpack_ref.py.
"""
import os
import socket
import sys
from datetime import timedelta

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import unpack_ref as ur
from kernel_double import CpuKernelDouble

FILL, MISSING = -32767, 12345
PACK_ATTRS = ("scale_factor", "add_offset", "_FillValue", "missing_value")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _mock(seed=4, stop="2019-01-02"):
    from dmd_era5_amd.create_mock_data import create_mock_era5

    return create_mock_era5("2019-01-01", stop, ["temperature", "u_component_of_wind"], [1000, 850, 500],
                            seed=seed, dtype=np.float32)


def _packed_pair(ds, fill_at=()):
    """(packed Dataset, decoded fp32 Dataset, codes per variable) of a mock slice.  ``fill_at``:
    indices (variable name, t, level, lat, lon) that get the fill code (first) / missing_value (others)."""
    from dmd_era5_amd.labeled import DataArray, Dataset

    packed, plain, codes = Dataset(coords=ds.coords, attrs=dict(ds.attrs)), Dataset(coords=ds.coords, attrs=dict(ds.attrs)), {}
    for v, name in enumerate(ds.data_vars):
        f = ds[name].values.astype(np.float64)
        lo, hi = float(f.min()), float(f.max())                # a packing of its own per variable, as a packer
        sf, ao = (hi - lo) / 65000.0, (hi + lo) / 2.0          # chooses it: the data spread over the 16 bits
        q = ur.pack(f, sf, ao)
        q[(q == FILL) | (q == MISSING)] = 0
        for i, idx in enumerate(x[1:] for x in fill_at if x[0] == name):
            q[idx] = FILL if i == 0 else MISSING
        codes[name] = (q, sf, ao)
        # (np.float64: scipy's NetCDF-3 writer stores a Python float as a 32-bit attribute)
        attrs = dict(ds[name].attrs, scale_factor=np.float64(sf), add_offset=np.float64(ao), _FillValue=np.int16(FILL), missing_value=np.int16(MISSING))
        packed[name] = DataArray(q, ds[name].dims, ds.coords, attrs)
        plain[name] = DataArray(ur.decode(q, sf, ao, (FILL, MISSING)), ds[name].dims, ds.coords, dict(ds[name].attrs))
    return packed, plain, codes


def _write(ds, path, fmt):
    from dmd_era5_amd import hdf5_lite, io_netcdf

    if fmt == "hdf5":
        if not hdf5_lite.available():
            pytest.fail("libhdf5 not found: the project's own HDF5 binding is what these cases are about")
        io_netcdf._write_hdf5(ds, path)
    else:
        io_netcdf._write_scipy(ds, path)
    return path


@pytest.fixture(autouse=True)
def _hdf5_backend(monkeypatch):
    monkeypatch.setenv("DMDX_NETCDF_BACKEND", "hdf5")


# ------------------------------------------------------------------ the reader
@pytest.mark.parametrize("fmt", ["hdf5", "netcdf3"])
def test_packed_variables_are_decoded_on_open(tmp_path, fmt):
    from dmd_era5_amd import io_netcdf

    fills = [("temperature", 0, 0, 0, 0), ("temperature", 3, 2, 5, 7), ("u_component_of_wind", 1, 1, 1, 1)]
    packed, plain, codes = _packed_pair(_mock(), fills)
    got = io_netcdf.open_dataset(_write(packed, str(tmp_path / "packed.nc"), fmt))
    for name, (q, sf, ao) in codes.items():
        x = got[name].values
        assert x.dtype == np.float32 and got[name].dtype == np.float32
        assert np.array_equal(_bits(x), _bits(ur.decode(q, sf, ao, (FILL, MISSING))))
        assert np.array_equal(np.isnan(x), (q == FILL) | (q == MISSING))
        assert int(np.isnan(x).sum()) == sum(f[0] == name for f in fills)
        assert not set(PACK_ATTRS) & set(got[name].attrs)          # the result file must not claim to be packed
        assert got[name].encoding["scale_factor"] == sf and int(got[name].encoding["_FillValue"]) == FILL
    assert np.array_equal(got.coords["level"].values, packed.coords["level"].values)


def test_lazy_packed_variable_keeps_the_file_dtype_for_slab_reads(tmp_path, monkeypatch):
    from dmd_era5_amd import io_netcdf

    packed, plain, codes = _packed_pair(_mock(), [("temperature", 2, 1, 3, 4)])
    path = _write(packed, str(tmp_path / "packed.nc"), "hdf5")
    monkeypatch.setattr(io_netcdf, "LAZY_BYTES", 1000)
    got = io_netcdf.open_dataset(path)
    q, sf, ao = codes["temperature"]
    lazy = got["temperature"].lazy
    assert lazy is not None and lazy.dtype == np.int16 and got["temperature"].dtype == np.float32
    assert (lazy.packing.scale_factor, lazy.packing.add_offset, lazy.packing.fills) == (sf, ao, (FILL, MISSING))
    out = np.empty((3,) + q.shape[1:], dtype=np.int16)
    assert lazy.read_slab(2, 5, out) is out and np.array_equal(out, q[2:5])
    box = np.empty((2, 2, 5, 9), dtype=np.int16)
    lazy.read_box((1, 1, 3, 4), box.shape, box)
    assert np.array_equal(box, q[1:3, 1:3, 3:8, 4:13])
    assert np.array_equal(_bits(np.asarray(lazy)), _bits(ur.decode(q, sf, ao, (FILL, MISSING))))
    x = got["temperature"].values                                      # loads and decodes
    assert x.dtype == np.float32 and got["temperature"].lazy is None
    assert np.array_equal(_bits(x), _bits(ur.decode(q, sf, ao, (FILL, MISSING))))
    assert not set(PACK_ATTRS) & set(got["temperature"].attrs)


@pytest.mark.parametrize("fmt", ["hdf5", "netcdf3"])
def test_other_integer_widths_and_float_fill_values(tmp_path, fmt):
    from dmd_era5_amd import io_netcdf
    from dmd_era5_amd.labeled import DataArray, Dataset

    ds = _mock()
    f = ds["temperature"].values
    q32 = np.rint(f.astype(np.float64) * 1000).astype(np.int32)
    q32[0, 0, 0, 1] = -2 ** 31 + 1
    fl = f.copy()
    fl[1, 2, 3, 4] = np.float32(9.96921e36)
    out = Dataset(coords=ds.coords, attrs=dict(ds.attrs))
    out["wide"] = DataArray(q32, ds["temperature"].dims, ds.coords,
                            {"scale_factor": np.float64(1e-3), "add_offset": np.float64(250.0), "_FillValue": np.int32(-2 ** 31 + 1)})
    out["floaty"] = DataArray(fl, ds["temperature"].dims, ds.coords, {"_FillValue": np.float32(9.96921e36)})
    out["plain"] = DataArray(f, ds["temperature"].dims, ds.coords, {"units": "K"})
    got = io_netcdf.open_dataset(_write(out, str(tmp_path / "mixed.nc"), fmt))
    w = got["wide"].values
    assert w.dtype == np.float32 and np.array_equal(_bits(w), _bits(ur.decode(q32, 1e-3, 250.0, (-2 ** 31 + 1,))))
    assert np.isnan(w[0, 0, 0, 1]) and int(np.isnan(w).sum()) == 1
    x = got["floaty"].values
    assert x.dtype == np.float32 and np.isnan(x[1, 2, 3, 4]) and int(np.isnan(x).sum()) == 1
    keep = np.ones(f.shape, dtype=bool)
    keep[1, 2, 3, 4] = False
    assert np.array_equal(_bits(x[keep]), _bits(f[keep]))
    # no packing attributes: as before, bit for bit, attributes included
    assert got["plain"].values.dtype == np.float32 and np.array_equal(_bits(got["plain"].values), _bits(f))
    assert got["plain"].attrs["units"] == "K" and got["plain"].encoding == {}


def test_svd_result_file_round_trips_unchanged(tmp_path, svd_base_config, project_root):
    from dmd_era5_amd import io_netcdf
    from dmd_era5_amd.config_parser import config_parser
    from dmd_era5_amd.era5_svd import add_config_attributes, combine_svd_results
    from dmd_era5_amd.slice_tools import apply_delay_embedding, flatten_era5_variables

    p = config_parser(svd_base_config, "era5-svd")
    da = apply_delay_embedding(flatten_era5_variables(_mock()["temperature", ]), 2)
    rs = np.random.RandomState(0)
    U, s, V = rs.standard_normal((da.shape[0], 4)).astype(np.float32), np.arange(4, 0, -1).astype(np.float32), \
        rs.standard_normal((4, da.shape[1])).astype(np.float32)
    res = add_config_attributes(combine_svd_results(U, s, V, da.coords, X=da), p)
    path = str(tmp_path / "res.nc")
    io_netcdf.to_netcdf(res, path)
    back = io_netcdf.open_dataset(path)
    for name in res.data_vars:
        a, b = np.asarray(res[name].values), back[name].values
        assert a.dtype == b.dtype and np.array_equal(a, b), name
        assert getattr(back[name], "encoding", {}) == {}


# ------------------------------------------------------------------ the pipeline on the CPU kernel double
def _cfg(svd_type="standard", scale=False, levels=None, d=2):
    return {"delay_embedding": d, "mean_center": True, "scale": scale, "levels": levels,
            "delta_time": timedelta(hours=1), "n_components": 3, "svd_type": svd_type,
            "save_data_matrix": False, "svd_seed": 0}


def _pipeline(path, cfg, comm=None, lazy_bytes=1000):
    from dmd_era5_amd import era5_svd, io_netcdf
    from dmd_era5_amd import svd as dsvd

    io_netcdf.LAZY_BYTES = lazy_bytes
    era5_svd.SLAB_BYTES = 11 * 3 * 36 * 72 * 4                  # several slabs per variable
    ds = io_netcdf.open_dataset(path)
    return era5_svd._device_pipeline(ds, cfg, comm or dsvd.Comm(), kern=CpuKernelDouble(), device=torch.device("cpu"))


@pytest.fixture
def _restore_module_constants():
    from dmd_era5_amd import era5_svd, io_netcdf

    keep = io_netcdf.LAZY_BYTES, era5_svd.SLAB_BYTES
    yield
    io_netcdf.LAZY_BYTES, era5_svd.SLAB_BYTES = keep


@pytest.mark.parametrize("lazy_bytes", [1000, 1 << 40], ids=["file-backed", "eager"])
@pytest.mark.parametrize("svd_type", ["standard", "randomized"])
def test_packed_slice_without_scaling_gives_the_singular_values_of_the_decoded_one(tmp_path, svd_type, lazy_bytes,
                                                                                   _restore_module_constants):
    """scale = False: the affine map does not cancel.  Raw codes fed to the SVD (what happened before the
    reader knew about packing) give s too large by 1 / scale_factor, a factor of a few hundred here."""
    packed, plain, _ = _packed_pair(_mock(seed=8, stop="2019-01-03"))
    pp = _write(packed, str(tmp_path / "packed.nc"), "hdf5")
    pf = _write(plain, str(tmp_path / "plain.nc"), "hdf5")
    cfg = _cfg(svd_type, levels=[850, 1000])
    U, s, V, *_ = _pipeline(pp, cfg, lazy_bytes=lazy_bytes)
    U1, s1, V1, *_ = _pipeline(pf, cfg, lazy_bytes=lazy_bytes)
    assert s.dtype == s1.dtype == np.float32 and U.dtype == np.float32
    assert np.array_equal(s, s1)                                 # the same fp32 matrix reached the same kernels
    assert np.array_equal(U, U1) and np.array_equal(V, V1)


@pytest.mark.parametrize("lazy_bytes", [1000, 1 << 40], ids=["file-backed", "eager"])
@pytest.mark.parametrize("stream", [0, 1], ids=["resident", "streamed"])
def test_fill_codes_in_the_slice_raise_with_name_and_count(tmp_path, monkeypatch, stream, lazy_bytes,
                                                           _restore_module_constants):
    fills = [("u_component_of_wind", 0, 0, 0, 0), ("u_component_of_wind", 7, 2, 30, 70), ("u_component_of_wind", 24, 1, 18, 3)]
    packed, _, _ = _packed_pair(_mock(seed=8), fills)
    pp = _write(packed, str(tmp_path / "packed.nc"), "hdf5")
    if stream:
        monkeypatch.setenv("DMDX_STREAM_BYTES", str(7 * 4 * 25 * 3 * 72))
    # resident: the count of the whole selection; streamed: of the first piece that has any (7 latitude rows)
    with pytest.raises(ValueError, match=r"u_component_of_wind: %s missing values" % ("1" if stream else "3")) as ei:
        _pipeline(pp, _cfg(), lazy_bytes=lazy_bytes)
    assert "temperature" not in str(ei.value)
    # the count is that of the selected slice: one of the three sits on level 850
    with pytest.raises(ValueError, match=r"u_component_of_wind: 1 missing values"):
        _pipeline(pp, _cfg(levels=[850]), lazy_bytes=lazy_bytes)


@pytest.mark.parametrize("fill", [np.nan, 9.96921e36], ids=["nan-fill", "finite-fill"])
def test_float32_variable_with_a_fill_value_keeps_the_direct_ingest(tmp_path, fill, _restore_module_constants):
    """xarray writes ``_FillValue = NaN`` on every float variable, so the reference's own float32 slices carry
    the attribute.  Such a variable must still be read straight into the staging buffers (``read_slab`` with an
    ``out``), give the blocks and ``nbytes`` of a file without the attribute, and have its missing values counted."""
    from dmd_era5_amd import era5_svd, io_netcdf
    from dmd_era5_amd.labeled import DataArray, Dataset

    ds = _mock(seed=11)
    f = ds["temperature"].values.copy()
    holes = [(0, 0, 0, 0), (13, 2, 35, 71), (24, 1, 7, 9)]
    with_attr, without = Dataset(coords=ds.coords, attrs=dict(ds.attrs)), Dataset(coords=ds.coords, attrs=dict(ds.attrs))
    g = f.copy()
    for idx in holes:
        g[idx] = np.float32(fill)
    nan = f.copy()
    for idx in holes:
        nan[idx] = np.nan
    with_attr["temperature"] = DataArray(g, ds["temperature"].dims, ds.coords, {"units": "K", "_FillValue": np.float32(fill)})
    without["temperature"] = DataArray(nan, ds["temperature"].dims, ds.coords, {"units": "K"})
    io_netcdf.LAZY_BYTES = 1000
    era5_svd.SLAB_BYTES = 7 * 3 * 36 * 72 * 4
    out = {}
    for tag, d in (("attr", with_attr), ("plain", without)):
        da = io_netcdf.open_dataset(_write(d, str(tmp_path / (tag + ".nc")), "hdf5"))["temperature"]
        lazy, calls = da.lazy, []
        assert lazy.dtype == np.float32 and (lazy.packing is not None) == (tag == "attr")
        inner = lazy.read_slab
        lazy.read_slab = lambda a, b, out=None, _f=inner: (calls.append(out is not None), _f(a, b, out))[1]
        st = {"mean": [], "std": []}
        blocks, m_v, nb = era5_svd._upload_variable(da, np.arange(3), np.arange(25), torch.device("cpu"), CpuKernelDouble(),
                                                    False, False, st)
        out[tag] = (blocks, nb, st.get("fills"), calls)
    (ba, nba, fa, ca), (bp, nbp, fp_, cp) = out["attr"], out["plain"]
    assert ca and all(ca) and ca == cp                                   # every slab went straight into a staging buffer
    assert nba == nbp == 4 * 25 * 3 * 36 * 72
    for x, y in zip(ba, bp):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))     # NaN where the holes are, same bits elsewhere
    assert fp_ is None and fa[0][0] == "temperature" and int(fa[0][1]) == 3


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, path, cfg, q, stream_bytes=0):
    for p in (os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist

    from dmd_era5_amd import svd as dsvd

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), DMDX_NETCDF_BACKEND="hdf5",
                      DMDX_STREAM_BYTES=str(stream_bytes))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        try:
            _pipeline(path, cfg, dsvd.TorchDistComm())
            q.put((rank, "returned", ""))
        except ValueError as e:
            q.put((rank, "raised", str(e)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("stream", [0, 1], ids=["resident", "streamed"])
def test_fill_codes_in_one_band_make_both_ranks_raise(tmp_path, stream):
    """36 latitude rows over two ranks: rows 0..17 and 18..35.  Both fill codes sit in rank 1's band; rank 0
    must raise too (alone it would wait for rank 1 in the Gram all-reduce).  Streamed (pieces of 7 latitude
    rows): the ranks have no common point per piece, the NaN reaches the all-reduced Gram, every rank gets
    the same LinAlgError and the summed counts turn it into the same ValueError."""
    fills = [("temperature", 3, 0, 20, 5), ("temperature", 9, 2, 35, 71)]
    packed, _, _ = _packed_pair(_mock(seed=8), fills)
    pp = _write(packed, str(tmp_path / "packed.nc"), "hdf5")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, pp, _cfg(), q, stream * 7 * 4 * 25 * 3 * 72)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted(q.get(timeout=180) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert [g[:2] for g in got] == [(0, "raised"), (1, "raised")]
    assert all("temperature: 2 missing values" in g[2] for g in got)
