"""GPU end-to-end tests of the drop-in entry points: ``main`` (device pipeline: upload ->
K5 centre/scale -> zero-copy delay view -> SVD -> NetCDF) and ``svd_on_era5`` against the
CPU oracle restating the reference's stages on the same seeded mock slice."""
import numpy as np
import pytest

from oracle import era5_oracle as orc
from parity_utils import col_cosines

pytestmark = pytest.mark.gpu


def _write_slice(cfg, seed, dtype):
    from dmd_era5_amd import io_netcdf
    from dmd_era5_amd.config_parser import config_parser
    from dmd_era5_amd.create_mock_data import add_download_attributes, create_mock_era5

    p = config_parser(cfg, "era5-svd")
    ds = add_download_attributes(
        create_mock_era5(cfg["start_datetime"], cfg["end_datetime"], p["variables"], p["levels"],
                         seed=seed, dtype=dtype), p)
    io_netcdf.to_netcdf(ds, p["era5_slice_path"])
    return p, ds


@pytest.mark.parametrize("svd_type,scale,d", [("standard", False, 2), ("standard", True, 1),
                                              ("randomized", False, 2), ("standard", True, 3)])
def test_main_matches_oracle_pipeline(svd_base_config, project_root, svd_type, scale, d):
    from dmd_era5_amd.era5_svd import main

    cfg = dict(svd_base_config, start_datetime="2019-01-01T00", end_datetime="2019-01-03T00",
               variables="temperature,u_component_of_wind", levels="1000,850", svd_type=svd_type,
               mean_center=True, scale=scale, delay_embedding=d, n_components=6,
               save_data_matrix=True, svd_seed=0)
    p, ds = _write_slice(cfg, seed=3, dtype=np.float32)
    res, added, retrieved = main(cfg, write_to_netcdf=True)
    assert (added, retrieved) == (False, False)

    variables = {k: ds[k].values for k in p["variables"]}
    X, X_mean, X_std = orc.preprocess(variables, True, scale, d)
    Uo, so, Vo = orc.svd_standard(X.astype(np.float64), 6)
    m = X.shape[0]
    assert res["U"].shape == (m, 6) and res["V"].shape == (6, X.shape[1]) and res["s"].shape == (6,)
    assert res["U"].values.dtype == np.float32
    # the pre-processed matrix itself (K5 + embedding order) against the reference arithmetic
    assert np.allclose(res["X"].values, X, rtol=0, atol=2e-4 * (1 if scale else 30))
    # mock data are white noise beyond the first (mean-structure) components: singular values
    # cluster, so compare s tightly and the subspace via the reconstruction
    if svd_type == "standard":
        assert np.allclose(res["s"].values, so, rtol=2e-5)
    else:
        # flat (white-noise) spectrum: the randomized estimate is 1-3 % below the exact values
        # by construction, so compare with the reference algorithm
        # (oracle restatement of sklearn) run on the same Omega = RandomState(0) draw
        Ur, sr, Vr = orc.svd_randomized(X, 6, random_state=0)
        assert np.allclose(res["s"].values, sr, rtol=1e-3)
        assert np.all(res["s"].values <= so * (1 + 1e-5)) and np.all(res["s"].values >= 0.95 * so)
    if svd_type == "standard":
        rec = (res["U"].values.astype(np.float64) * res["s"].values) @ res["V"].values
        ref = (Uo * so) @ Vo
        assert np.linalg.norm(rec - ref) <= 2e-3 * np.linalg.norm(ref)
    U = res["U"].values.astype(np.float64)
    assert np.abs(U.T @ U - np.eye(6)).max() < 1e-4
    # labels and the X_mean quirk (kept only when centred and d > 1, ref era5_svd.py:400-414)
    assert np.array_equal(res.coords["delay"].values, orc.delay_labels(m // d, d))
    assert np.array_equal(res.coords["space"].values, np.arange(m))
    assert list(res.coords["original_variable"].values[[0, m // d - 1]]) == ["temperature", "u_component_of_wind"]
    if d > 1:
        # the reference's mean is an fp32 accumulation (numpy), ours fp64 rounded once:
        # they agree to the fp32 summation error of n ~ 49 values of size <= 280
        assert np.allclose(res["X_mean"].values, X_mean, rtol=1e-5, atol=2e-4)
        if scale:
            assert np.allclose(res["X_std"].values, X_std, rtol=1e-5)
    else:
        assert "X_mean" not in res
    assert res.attrs["svd_type"] == svd_type and res.attrs["delay_embedding"] == d
    # second call: the stored result is returned (ref era5_svd.py:203-208)
    again, _, _ = main(cfg, write_to_netcdf=True)
    assert np.allclose(again["s"].values, res["s"].values)
    assert again["U"].shape == res["U"].shape


@pytest.mark.parametrize("svd_type", ["standard", "randomized"])
def test_svd_on_era5_shapes_like_reference_test(svd_base_config, svd_type):
    """reference tests/test_03_era5_svd.py:153-176 (shapes), plus orthonormality."""
    from dmd_era5_amd import slice_tools as st
    from dmd_era5_amd.config_parser import config_parser
    from dmd_era5_amd.create_mock_data import create_mock_era5
    from dmd_era5_amd.era5_svd import svd_on_era5

    cfg = dict(svd_base_config, svd_type=svd_type)
    p = config_parser(cfg, "era5-svd")
    data = create_mock_era5("2019-01-01", "2019-01-02", ["temperature"], [1000], seed=9)
    da = st.apply_delay_embedding(st.flatten_era5_variables(data), p["delay_embedding"])
    U, s, V = svd_on_era5(da, p)
    n_samples, n_time = da.shape
    assert U.shape == (n_samples, 10) and s.shape == (10,) and V.shape == (10, n_time)
    assert U.dtype == np.float64                     # fp64 in -> fp64 out (fp64 arithmetic: engine._svd_fp64)
    assert np.all(np.diff(s) <= 1e-6 * s[0])
    Ur, sr, Vr = orc.svd_standard(da.values, 10)
    assert np.allclose(s[:1], sr[:1], rtol=1e-5)     # un-centred mock: one dominant component
    assert col_cosines(U[:, :1], Ur[:, :1]).min() > 1 - 1e-6
    with pytest.raises(ValueError, match="SVD type foo is not supported."):
        svd_on_era5(da, dict(p, svd_type="foo"))


def test_main_streams_a_lazy_hdf5_slice_with_resampling(svd_base_config, project_root, monkeypatch):
    """File-backed variables (HDF5 backend), level subset in a different order, 6-hourly
    nearest resampling, small staging slabs: the streaming ingest must build the same X."""
    from dmd_era5_amd import era5_svd, io_netcdf
    from dmd_era5_amd.era5_svd import main

    monkeypatch.setenv("DMDX_NETCDF_BACKEND", "hdf5")
    monkeypatch.setattr(io_netcdf, "LAZY_BYTES", 1000)
    monkeypatch.setattr(era5_svd, "SLAB_BYTES", 7 * 3 * 36 * 72 * 4)      # 7 snapshots per slab
    cfg = dict(svd_base_config, start_datetime="2019-01-01T00", end_datetime="2019-01-06T00",
               delta_time="6h", variables="temperature,v_component_of_wind", levels="850,1000",
               svd_type="standard", mean_center=True, scale=False, delay_embedding=2, n_components=5,
               save_data_matrix=True)
    wcfg = dict(cfg, delta_time="1h", levels="1000,925,850")
    from dmd_era5_amd.config_parser import config_parser
    from dmd_era5_amd.create_mock_data import add_download_attributes, create_mock_era5

    p = config_parser(cfg, "era5-svd")
    pw = config_parser(wcfg, "era5-svd")
    full = add_download_attributes(
        create_mock_era5(cfg["start_datetime"], cfg["end_datetime"], pw["variables"], pw["levels"], seed=4,
                         dtype=np.float32), pw)
    assert io_netcdf.to_netcdf(full, p["era5_slice_path"]) == "hdf5-lite"
    res, _, _ = main(cfg, write_to_netcdf=True)
    # oracle: levels [850, 1000] (requested order) of the 1000/925/850 file, every 6th hour
    variables = {k: full[k].values[::6][:, [2, 0]] for k in p["variables"]}
    X, X_mean, _ = orc.preprocess(variables, True, False, 2)
    assert res["X"].shape == X.shape == (2 * 2 * 2 * 36 * 72, 20)
    assert np.allclose(res["X"].values, X, rtol=0, atol=6e-3)
    assert np.array_equal(res.coords["level"].values[:2 * 36 * 72], np.repeat([850.0, 1000.0], 36 * 72))
    Uo, so, Vo = orc.svd_standard(X.astype(np.float64), 5)
    assert np.allclose(res["s"].values, so, rtol=2e-5)
    back = io_netcdf.open_dataset(p["save_path"])
    assert np.allclose(back["s"].values, res["s"].values)
    assert list(np.unique(back.coords["original_variable"].values)) == ["temperature", "v_component_of_wind"]


def test_main_direct_pinned_ingest_path(svd_base_config, project_root, monkeypatch):
    """fp32 file-backed variable, hourly (contiguous) snapshots, all levels: slabs are read straight
    into pinned staging buffers and copied asynchronously -- same X as the oracle."""
    from dmd_era5_amd import era5_svd, io_netcdf
    from dmd_era5_amd.era5_svd import main

    monkeypatch.setenv("DMDX_NETCDF_BACKEND", "hdf5")
    monkeypatch.setattr(io_netcdf, "LAZY_BYTES", 1000)
    monkeypatch.setattr(era5_svd, "SLAB_BYTES", 5 * 2 * 36 * 72 * 4)      # 5 snapshots per slab, 2 buffers
    cfg = dict(svd_base_config, start_datetime="2019-01-01T00", end_datetime="2019-01-02T12",
               variables="temperature", levels="1000,850", svd_type="standard", mean_center=True,
               scale=True, delay_embedding=1, n_components=4, save_data_matrix=True)
    p, ds = _write_slice(cfg, seed=12, dtype=np.float32)
    res, _, _ = main(cfg)
    X, _, _ = orc.preprocess({"temperature": ds["temperature"].values}, True, True, 1)
    assert res["X"].shape == X.shape == (2 * 36 * 72, 37)
    assert np.allclose(res["X"].values, X, rtol=0, atol=2e-4)
    _, so, _ = orc.svd_standard(X.astype(np.float64), 4)
    assert np.allclose(res["s"].values, so, rtol=2e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [1, 2])
def test_main_uncentred_temperature_matches_oracle(svd_base_config, project_root, d):
    """mean_center = False on a temperature field (values ~ 280 K): the pipeline must still return
    the SVD of the UN-centred matrix; it goes through the mean-deflated route (the plain Gram
    route loses the trailing singular values there).  Truth: oracle preprocessing + numpy fp64."""
    from dmd_era5_amd.era5_svd import main

    cfg = dict(svd_base_config, start_datetime="2019-01-01T00", end_datetime="2019-01-04T00",
               variables="temperature", levels="1000", svd_type="standard", mean_center=False, scale=False,
               delay_embedding=d, n_components=5, save_data_matrix=True)
    p, ds = _write_slice(cfg, seed=11, dtype=np.float32)
    res, _, _ = main(cfg, write_to_netcdf=False)
    X, _, _ = orc.preprocess({k: ds[k].values for k in p["variables"]}, False, False, d)
    assert np.allclose(res["X"].values, X, rtol=0, atol=1e-3)               # restored after the in-place centring
    Uo, so, Vo = orc.svd_standard(X.astype(np.float64), 5)
    assert so[0] > 100 * so[1]                                              # the mean mode dominates
    # fp32 data with s_1 / s_i ~ 220: numpy's own fp32 LAPACK answer is good to ~eps32 s_1 / s_i = 1e-5
    assert np.allclose(res["s"].values, so, rtol=1e-5)
    # the noise singular values cluster (mock data are white noise), so the rank-5 truncation is
    # compared through its error, which must be the Eckart-Young optimum, not vector by vector
    X64 = X.astype(np.float64)
    rec = (res["U"].values.astype(np.float64) * res["s"].values) @ res["V"].values
    sall = np.linalg.svd(X64, compute_uv=False)
    assert np.linalg.norm(X64 - rec) <= (1 + 1e-4) * np.sqrt((sall[5:] ** 2).sum())
    U = res["U"].values.astype(np.float64)
    assert np.abs(U.T @ U - np.eye(5)).max() < 1e-4


def test_create_mock_era5_svd_and_combine_like_the_reference_tests():
    """reference tests/test_01_create_mock_data.py:33-53 and tests/test_03_era5_svd.py:179-225:
    the mock-SVD helper's return types / shapes / coordinate keys, and the Dataset that
    combine_svd_results builds from it (with and without the data matrix) -- plus the values
    against numpy on the same seeded slice, which the reference's tests do not pin."""
    from dmd_era5_amd.create_mock_data import create_mock_era5_svd
    from dmd_era5_amd.era5_svd import combine_svd_results
    from dmd_era5_amd.labeled import DataArray, Dataset

    U, s, V, coords, X = create_mock_era5_svd(n_components=4, seed=21)
    assert all(isinstance(a, np.ndarray) for a in (U, s, V)) and isinstance(X, DataArray)
    assert U.shape[1] == 4 and s.size == 4 and V.shape[0] == 4
    assert sorted(coords.keys()) == sorted(["space", "time", "original_variable", "delay"])
    assert X.shape == (2 * 36 * 72, 24) and U.shape[0] == X.shape[0] and V.shape[1] == X.shape[1]
    sr = np.linalg.svd(X.values, compute_uv=False)[:4]
    assert np.allclose(s, sr, rtol=2e-5)

    ds = combine_svd_results(U, s, V, coords)
    assert isinstance(ds, Dataset) and sorted(ds.data_vars.keys()) == ["U", "V", "s"]
    assert sorted(ds["U"].dims) == ["components", "space"] and list(ds["s"].dims) == ["components"]
    assert sorted(ds["V"].dims) == ["components", "time"]
    assert sorted(ds["U"].coords.keys()) == sorted(["space", "components", "original_variable", "delay"])
    assert sorted(ds["s"].coords.keys()) == ["components"]
    assert sorted(ds["V"].coords.keys()) == ["components", "time"]
    dx = combine_svd_results(U, s, V, coords, X=X)
    assert sorted(dx.data_vars.keys()) == ["U", "V", "X", "s"]
    assert dx["U"].shape[0] == dx["X"].shape[0] and dx["V"].shape[1] == dx["X"].shape[1]


@pytest.mark.parametrize("ranks", ["two-over-gloo", "one-over-rccl", "four-over-gloo"])
@pytest.mark.parametrize("streamed", [False, True])
def test_main_sharded_over_two_ranks(svd_base_config, tmp_path, monkeypatch, streamed, ranks):
    """``main`` under torch.distributed.run, one process per rank, the space
    points sharded by latitude band -- here two ranks sharing the one GPU of the box over gloo
    (the driver's multi-GPU runs use RCCL).  Rank 0's result file must hold the same
    decomposition, in the same row order, as a single-process run on the same slice.
    ``streamed``: each rank additionally streams its band from the file in two passes (pieces of
    4 latitude rows), as it would for a slice larger than the HBM.
    ``one-over-rccl``: RCCL wants one GPU per rank, so on this box it can only carry a ONE-rank
    group -- DMDX_COMM_FORCE=1 makes that group issue every collective of the sharded path
    (packed Gram all-reduce, stats all-gather, broadcasts, the gather to the root) through the
    nccl backend with device tensors, which is what gloo's host staging cannot check."""
    import json
    import os
    import socket
    import subprocess
    import sys

    from dmd_era5_amd import io_netcdf
    from dmd_era5_amd.era5_svd import main

    if ranks == "four-over-gloo" and streamed:
        pytest.skip("the four-rank rehearsal (at most 6 processes may share the box's GPU, this one included) runs the resident path; "
                    "8 ranks with uneven bands: tests/test_sharded_pipeline.py (CPU, gloo)")
    here = os.path.dirname(os.path.abspath(__file__))
    cfg = dict(svd_base_config, start_datetime="2019-01-01T00", end_datetime="2019-01-03T00",
               variables="temperature,v_component_of_wind", levels="850,1000", svd_type="standard",
               mean_center=True, scale=True, delay_embedding=2, n_components=3, save_data_matrix=not streamed)
    from dmd_era5_amd.config_parser import config_parser
    from dmd_era5_amd.create_mock_data import add_download_attributes, create_mock_era5

    roots = {}
    for tag in ("one", "two"):
        roots[tag] = tmp_path / tag
        roots[tag].mkdir()
        monkeypatch.setenv("DMD_ERA5_ROOT", str(roots[tag]))
        p = config_parser(cfg, "era5-svd")
        ds = create_mock_era5(cfg["start_datetime"], cfg["end_datetime"], p["variables"], p["levels"], seed=8)
        # three planted space-time patterns above the mock's white noise, so that the leading
        # singular triplets are separated and comparable between the two runs
        t = np.arange(ds["temperature"].shape[0], dtype=np.float64)[:, None, None, None]
        lat = np.radians(ds.coords["latitude"].values)[None, None, :, None]
        lon = np.radians(ds.coords["longitude"].values)[None, None, None, :]
        for v, name in enumerate(ds.data_vars):
            f = ds[name].values
            f = f + 60 * np.sin(2 * np.pi * t / 24) * np.cos(lat) * np.cos(lon + v)
            f = f + 35 * np.cos(2 * np.pi * t / 11) * np.sin(2 * lat) * np.sin(2 * lon)
            f = f + 20 * (t / 49.0) ** 2 * np.cos(3 * lon) * np.ones_like(lat)
            ds[name].values = f.astype(np.float32)
        io_netcdf.to_netcdf(add_download_attributes(ds, p), p["era5_slice_path"])
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, DMD_ERA5_ROOT=str(roots["two"]), DMDX_DEVICE="0", DMDX_TEST_CONFIG=json.dumps(cfg))
    if ranks != "one-over-rccl":
        env["DMDX_DIST_BACKEND"] = "gloo"
    else:
        env.pop("DMDX_DIST_BACKEND", None)
        env.update(DMDX_COMM_FORCE="1", DMDX_TEST_EXPECT_BACKEND="nccl")
    if streamed:
        env["DMDX_STREAM_BYTES"] = str(4 * 4 * 49 * 2 * 72)
    nproc = {"two-over-gloo": "2", "one-over-rccl": "1", "four-over-gloo": "4"}[ranks]
    run = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", nproc,
                          "--master-addr", "127.0.0.1", "--master-port", str(port),
                          os.path.join(here, "dist_main_worker.py")],
                         env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    if ranks == "two-over-gloo":
        assert "latitude rows 0:18" in run.stdout and "latitude rows 18:36" in run.stdout
    elif ranks == "four-over-gloo":
        assert "latitude rows 0:9" in run.stdout and "latitude rows 27:36" in run.stdout
    else:
        assert "backend nccl" in run.stdout and "collectives issued" in run.stdout
    two = io_netcdf.open_dataset(p["save_path"])

    monkeypatch.setenv("DMD_ERA5_ROOT", str(roots["one"]))
    one, _, _ = main(cfg, write_to_netcdf=False)
    for name in ("U", "s", "V", "X_mean", "X_std") + (() if streamed else ("X",)):
        assert two[name].shape == one[name].shape, name
    if streamed:
        assert "X" not in two.data_vars and "streaming it in" in run.stdout
        assert np.abs(two["U"].values - one["U"].values).max() < 1e-4 * np.abs(one["U"].values).max()
    else:
        assert np.array_equal(two["X"].values, one["X"].values)            # same rows, same order
    assert np.array_equal(two["X_mean"].values, one["X_mean"].values)
    for c in ("latitude", "longitude", "level", "original_variable", "delay"):
        assert np.array_equal(two.coords[c].values, one.coords[c].values), c
    assert np.allclose(two["s"].values, one["s"].values, rtol=1e-5)
    rec2 = (two["U"].values.astype(np.float64) * two["s"].values) @ two["V"].values
    rec1 = (one["U"].values.astype(np.float64) * one["s"].values) @ one["V"].values
    assert np.linalg.norm(rec2 - rec1) <= 1e-3 * np.linalg.norm(rec1)


def test_slice_larger_than_hbm_is_refused_with_advice(svd_base_config, project_root, monkeypatch):
    """X must be resident in HBM: a slice that does not fit is refused before the upload, with the
    number of ranks that would hold it."""
    import torch

    from dmd_era5_amd.era5_svd import main

    cfg = dict(svd_base_config, start_datetime="2019-01-01T00", end_datetime="2019-01-02T00", svd_type="standard")
    _write_slice(cfg, seed=1, dtype=np.float32)
    # (the reserve next to X is sized from the problem: here two 256 MB staging slabs + 1 GiB of
    # slack + a few MB of workspaces; the allocator's cached-but-unused bytes count as free)
    monkeypatch.setattr(torch.cuda, "memory_reserved", lambda *a, **k: torch.cuda.memory_allocated())
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (2 << 30, 288 << 30))
    main(cfg)                                                     # 60 KB of X, ~1.5 GiB of reserve: fine
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (1 << 30, 288 << 30))
    monkeypatch.setenv("DMD_ERA5_ROOT", str(project_root))
    with pytest.raises(Exception, match="Error in the SVD on ERA5 process: .*does not fit.*torch.distributed.run"):
        main(dict(cfg, n_components=9))                            # (another result file: no cache hit)


@pytest.mark.parametrize("svd_type", ["standard", "randomized"])
def test_main_on_a_wide_problem(svd_base_config, project_root, svd_type):
    """Fewer space rows than snapshots (the 5-degree mock grid over 113 days of hourly data: 2592 x
    2712): sklearn transposes such inputs, LAPACK does not care; the device pipeline runs the tall
    algorithms on the transposed matrix and swaps the factors."""
    from dmd_era5_amd import io_netcdf
    from dmd_era5_amd.config_parser import config_parser
    from dmd_era5_amd.create_mock_data import add_download_attributes, create_mock_era5
    from dmd_era5_amd.era5_svd import main

    cfg = dict(svd_base_config, start_datetime="2019-01-01T00", end_datetime="2019-04-23T23", svd_type=svd_type,
               mean_center=True, scale=False, delay_embedding=1, n_components=3, save_data_matrix=True, svd_seed=0)
    p = config_parser(cfg, "era5-svd")
    ds = create_mock_era5(cfg["start_datetime"], cfg["end_datetime"], p["variables"], p["levels"], seed=12, dtype=np.float32)
    t = np.arange(ds["temperature"].shape[0], dtype=np.float64)[:, None, None, None]
    lat = np.radians(ds.coords["latitude"].values)[None, None, :, None]
    lon = np.radians(ds.coords["longitude"].values)[None, None, None, :]
    f = ds["temperature"].values.astype(np.float64)
    f = f + 60 * np.sin(2 * np.pi * t / 24) * np.cos(lat) * np.cos(lon) + 35 * np.cos(2 * np.pi * t / 11) * np.sin(2 * lat) * np.sin(2 * lon)
    f = f + 20 * (t / len(t)) ** 2 * np.cos(3 * lon) * np.ones_like(lat)
    ds["temperature"].values = f.astype(np.float32)
    io_netcdf.to_netcdf(add_download_attributes(ds, p), p["era5_slice_path"])
    res, _, _ = main(cfg, write_to_netcdf=True)
    X = res["X"].values.astype(np.float64)
    assert X.shape == (2592, 2712) and res["U"].shape == (2592, 3) and res["V"].shape == (3, 2712)
    U, s, V = (res[k].values.astype(np.float64) for k in ("U", "s", "V"))
    sref = np.linalg.svd(X, compute_uv=False)[:3]
    assert np.allclose(s, sref, rtol=1e-5 if svd_type == "standard" else 1e-4)
    assert np.abs(U.T @ U - np.eye(3)).max() < 1e-5 and np.abs(V @ V.T - np.eye(3)).max() < 1e-5
    assert np.max(np.linalg.norm(X.T @ U - V.T * s, axis=0) / s) < (1e-5 if svd_type == "standard" else 1e-3)
    assert np.all(U[np.abs(U).argmax(axis=0), np.arange(3)] > 0)              # u-based sign convention


@pytest.mark.parametrize("svd_type,d,scale,center", [("standard", 1, False, True), ("standard", 2, True, True),
                                                     ("randomized", 2, False, True), ("standard", 2, False, False)])
def test_main_streams_a_slice_that_does_not_fit(svd_base_config, tmp_path, monkeypatch, svd_type, d, scale, center):
    """A snapshot matrix larger than the free HBM is streamed from the file in passes instead of
    being refused (standard: Gram pass + projection pass; randomized: one pass per power iteration
    + two).  Forced by a piece budget of 5 latitude rows; the result must equal the resident run on
    the same slice.  ``center = False``: un-centred fields lifted by 5000 (s_1 ~ 1e3 s_2): the
    streamed standard path deflates the time mean exactly, piece by piece, as the resident one."""
    from dmd_era5_amd import io_netcdf
    from dmd_era5_amd.config_parser import config_parser
    from dmd_era5_amd.create_mock_data import add_download_attributes, create_mock_era5
    from dmd_era5_amd.era5_svd import main

    cfg = dict(svd_base_config, start_datetime="2019-01-01T00", end_datetime="2019-01-04T00",
               variables="temperature,u_component_of_wind", levels="1000,500", svd_type=svd_type,
               mean_center=center, scale=scale, delay_embedding=d, n_components=3, save_data_matrix=False, svd_seed=0)
    out = {}
    for tag in ("resident", "streamed"):
        root = tmp_path / tag
        root.mkdir()
        monkeypatch.setenv("DMD_ERA5_ROOT", str(root))
        monkeypatch.setenv("DMDX_NETCDF_BACKEND", "hdf5")
        p = config_parser(cfg, "era5-svd")
        ds = create_mock_era5(cfg["start_datetime"], cfg["end_datetime"], p["variables"], p["levels"], seed=31, dtype=np.float32)
        t = np.arange(ds["temperature"].shape[0], dtype=np.float64)[:, None, None, None]
        lat = np.radians(ds.coords["latitude"].values)[None, None, :, None]
        lon = np.radians(ds.coords["longitude"].values)[None, None, None, :]
        for v, name in enumerate(ds.data_vars):
            f = ds[name].values.astype(np.float64)
            f = f + 60 * np.sin(2 * np.pi * t / 24) * np.cos(lat) * np.cos(lon + v) + 35 * np.cos(2 * np.pi * t / 11) * np.sin(2 * lat) * np.sin(2 * lon)
            f = f + 20 * (t / len(t)) ** 2 * np.cos(3 * lon) * np.ones_like(lat)
            ds[name].values = (f + (0.0 if center else 5000.0)).astype(np.float32)
        io_netcdf.to_netcdf(add_download_attributes(ds, p), p["era5_slice_path"])
        if tag == "streamed":
            monkeypatch.setenv("DMDX_STREAM_BYTES", str(5 * 4 * 73 * 2 * 72))
        out[tag], _, _ = main(cfg, write_to_netcdf=True)
        monkeypatch.delenv("DMDX_STREAM_BYTES", raising=False)
    a, b = out["resident"], out["streamed"]
    assert sorted(a.data_vars) == sorted(b.data_vars) and "X" not in b.data_vars
    assert np.allclose(b["s"].values, a["s"].values, rtol=1e-6 if svd_type == "standard" else 1e-5)
    assert np.abs(b["U"].values - a["U"].values).max() < 1e-4 * np.abs(a["U"].values).max()
    assert np.abs(b["V"].values - a["V"].values).max() < 1e-5
    if d > 1 and center:
        assert np.array_equal(b["X_mean"].values, a["X_mean"].values)
        if scale:
            assert np.allclose(b["X_std"].values, a["X_std"].values, rtol=1e-6)
    if not center:
        assert "X_mean" not in b.data_vars and float(b["s"].values[0]) > 200 * float(b["s"].values[1])


@pytest.mark.parametrize("ranks", ["two-over-gloo", "one-over-rccl", "four-over-gloo"])
@pytest.mark.parametrize("workload", ["small", "small-randomized"])
def test_bench_two_ranks_on_one_gpu_over_gloo(workload, ranks):
    """bench.py's N > 1 path as the driver launches it (torch.distributed.run, one process per
    rank, RANK / LOCAL_RANK / WORLD_SIZE from the environment) -- rehearsed with two ranks on the
    box's one GPU over gloo (DMDX_BENCH_DEVICE / DMDX_DIST_BACKEND; RCCL needs one GPU per rank and
    is the driver's 8-GPU run).  The line must say what the ranks saw: world size, backend, one
    device entry per rank; row shards of ONE global matrix: the singular values of the 2-rank run
    are those of the stacked matrix (sqrt(2) x the planted single-shard ones, 5 %).
    ``one-over-rccl``: the same launch with ONE rank and the default backend -- the only group
    RCCL can form on a one-GPU box; DMDX_BENCH_FORCE_DIST / DMDX_COMM_FORCE make it carry every
    collective of the step (device tensors through the nccl backend)."""
    import json
    import os
    import socket
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, DMDX_BENCH_DEVICE="0")
    if ranks != "one-over-rccl":
        env["DMDX_DIST_BACKEND"] = "gloo"
    else:
        env.pop("DMDX_DIST_BACKEND", None)
        env.update(DMDX_BENCH_FORCE_DIST="1", DMDX_COMM_FORCE="1")
    extra = ["--workload", "small"]
    if workload == "small-randomized":
        env["DMDX_BENCH_SVD_TYPE"] = "randomized"
    w = {"two-over-gloo": 2, "one-over-rccl": 1, "four-over-gloo": 4}[ranks]
    run = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(w),
                          "--master-addr", "127.0.0.1", "--master-port", str(port),
                          os.path.join(root, "bench.py"), "--gpus", str(w), "--steps", "2", "--warmup", "1",
                          "--full", "--no-cpu-baseline", "--no-calibrate"] + extra,
                         env=env, capture_output=True, text=True, timeout=600, cwd=root)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, run.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == w and out["world_size"] == w and out["steps"] == 2 and out["scaling"] == "weak"
    assert out["backend"].startswith("gloo" if w >= 2 else "nccl") and [d["rank"] for d in out["devices"]] == list(range(w))
    assert all(d["device_index"] == 0 for d in out["devices"])
    assert out["value"] > 0 and out["unit"] == "GB/s" and out["config"]["m_total"] == w * out["config"]["m_per_gpu"]
    if w >= 2:
        assert "cpu_baseline" not in out and "hard_spectrum" not in out          # N = 1 only
    else:
        assert out["collectives_per_step"] > 0
    # the line explains its own collectives: wall time, calls and bytes per step by kind (round 3)
    cm = out["collective_ms"]
    assert cm and all(v["ms_per_step"] >= 0 and v["calls_per_step"] > 0 for v in cm.values())
    assert abs(sum(v["calls_per_step"] for v in cm.values()) - out["collectives_per_step"]) < 1e-9
    if workload == "small":
        assert "gram_allreduce" in cm and cm["gram_allreduce"]["bytes_per_step"] == 8 * (1024 * 1025 // 2)
    assert len(out["step_ms"]) == 2 and all(t > 0 for t in out["step_ms"])
    m, n = out["config"]["m_total"], out["config"]["n"]
    planted = 100.0 * 0.9 ** np.arange(3) * np.sqrt(float(m) * n)
    assert np.all(np.abs(np.array(out["s_head"]) / planted - 1.0) < 0.05), out["s_head"]
    if workload == "small":
        assert out["roofline"]["bound"] == "mfma" and out["roofline"]["frac"] > 0
        if w >= 2:
            assert "one packed-triangle Gram all-reduce" in out["config"]["sharding"]


def test_bench_plain_run_is_lean_and_dumps_the_same_outputs_twice(tmp_path):
    """A plain bench.py run prints the headline fields and none of what --full measures; with
    --dump-outputs it writes the SVD of its last timed step, and a second run with the same
    arguments writes the same one (the inputs are seeded)."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    runs = []
    for tag in ("a", "b"):
        run = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3",
                              "--warmup", "1", "--workload", "small", "--dump-outputs", str(tmp_path / tag)],
                             capture_output=True, text=True, timeout=600, cwd=root)
        assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
        lines = [ln for ln in run.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, run.stdout[-2000:]
        runs.append(json.loads(lines[0]))
    out = runs[0]
    assert out["steps"] == 3 and out["warmup"] == 1 and out["unit"] == "GB/s" and out["higher_is_better"] is True
    assert out["dtype"] == "f32" and out["metric"] and out["ms_per_step"] > 0
    m, n = out["config"]["m_total"], out["config"]["n"]
    assert abs(out["value"] * out["ms_per_step"] / (m * n * 4.0 / 1e6) - 1) < 1e-9
    for key in ("roofline", "step_ms", "collective_ms", "stage_ms", "kernel_ms_per_step", "calibration",
                "cpu_baseline", "hard_spectrum"):
        assert key not in out, key
    assert sorted(out["outputs"]["arrays"]) == ["U", "V", "s"]
    k = out["config"]["rank"]
    s, V, U = (np.load(tmp_path / "a" / f"{a}.npy") for a in ("s", "V", "U"))
    assert s.shape == (k,) and V.shape == (n, k) and U.shape == (m, k)
    assert s.dtype == V.dtype == np.float64 and U.dtype == np.float32
    assert np.array_equal(s[:3], np.array(out["s_head"]))
    planted = 100.0 * 0.9 ** np.arange(3) * np.sqrt(float(m) * n)
    assert np.all(np.abs(s[:3] / planted - 1.0) < 0.05)
    assert np.abs(V.T @ V - np.eye(k)).max() < 1e-6
    assert np.abs(U.T.astype(np.float64) @ U - np.eye(k)).max() < 1e-3
    s2, V2, U2 = (np.load(tmp_path / "b" / f"{a}.npy") for a in ("s", "V", "U"))
    assert np.allclose(s2, s, rtol=1e-6, atol=0)
    assert col_cosines(U2, U).min() > 1 - 1e-5 and col_cosines(V2, V).min() > 1 - 1e-5


@pytest.mark.parametrize("svd_type,center,scale,d", [("standard", True, False, 2), ("standard", True, True, 1),
                                                     ("standard", False, False, 2), ("randomized", True, False, 2)])
def test_float64_mock_slice_comes_back_with_float64_accuracy(svd_base_config, project_root, svd_type, center, scale, d):
    """BASELINE config 1 / the reference's own test inputs are float64 (create_mock_era5): such
    slices take the fp64 path -- the reference's host sequence on the mirrored slice tools, the
    Gram on the fp64 MFMA kernel (K9), the fp64 eigen stage -- and must agree with the reference's
    arithmetic (oracle.preprocess + np.linalg.svd on float64) to float64 accuracy, through
    main() and through svd_on_era5: 1e-11 on every singular value (round 1: 5e-6, fp32
    arithmetic), vectors to 1e-9 where the gaps allow.  Randomized: against the oracle's
    restatement of sklearn on the same Omega."""
    from dmd_era5_amd.era5_svd import main, svd_on_era5

    cfg = dict(svd_base_config, start_datetime="2019-01-01T00", end_datetime="2019-01-03T00",
               variables="temperature,u_component_of_wind", levels="1000,850", svd_type=svd_type,
               mean_center=center, scale=scale, delay_embedding=d, n_components=4, save_data_matrix=True, svd_seed=0)
    p, ds = _write_slice(cfg, seed=3, dtype=np.float64)
    # planted patterns so that the leading triplets are separated (the mock is white noise)
    t = np.arange(ds["temperature"].shape[0], dtype=np.float64)[:, None, None, None]
    lat = np.radians(ds.coords["latitude"].values)[None, None, :, None]
    lon = np.radians(ds.coords["longitude"].values)[None, None, None, :]
    from dmd_era5_amd import io_netcdf

    for v, name in enumerate(ds.data_vars):
        f = ds[name].values + 60 * np.sin(2 * np.pi * t / 24) * np.cos(lat) * np.cos(lon + v)
        f = f + 35 * np.cos(2 * np.pi * t / 11) * np.sin(2 * lat) * np.sin(2 * lon) + 20 * (t / 49.0) ** 2 * np.cos(3 * lon)
        ds[name].values = f
    io_netcdf.to_netcdf(ds, p["era5_slice_path"])
    res, _, _ = main(cfg, write_to_netcdf=False)
    X, X_mean, X_std = orc.preprocess({k: ds[k].values for k in p["variables"]}, center, scale, d)
    assert X.dtype == np.float64 and res["U"].values.dtype == np.float64 and res["X"].values.dtype == np.float64
    assert np.array_equal(res["X"].values, X)                       # the host sequence IS the reference's arithmetic
    if svd_type == "standard":
        Uo, so, Vo = orc.svd_standard(X, 4)
    else:
        Uo, so, Vo = orc.svd_randomized(X, 4, random_state=0)
    s, U, V = res["s"].values, res["U"].values, res["V"].values
    assert np.abs(s / so - 1).max() < (1e-11 if svd_type == "standard" else 1e-9), np.abs(s / so - 1).max()
    assert col_cosines(U[:, :3], Uo[:, :3]).min() > 1 - 1e-9 and col_cosines(V[:3].T, Vo[:3].T).min() > 1 - 1e-9
    assert np.abs(U.T @ U - np.eye(4)).max() < 1e-12
    if center and d > 1:
        assert np.array_equal(res["X_mean"].values, X_mean)
    # the function boundary the reference's own test calls (tests/test_03_era5_svd.py:164)
    from dmd_era5_amd.labeled import DataArray

    U2, s2, V2 = svd_on_era5(DataArray(X, ("space", "time")), p)
    assert U2.dtype == np.float64 and np.abs(s2 / so - 1).max() < (1e-11 if svd_type == "standard" else 1e-9)


@pytest.mark.parametrize("svd_type", ["standard", "randomized"])
def test_main_with_the_library_primer_on_a_side_thread(svd_base_config, project_root, monkeypatch, svd_type):
    """main() primes the libraries on a side thread (a toy SVD with a kernel provider and a stream
    of its own, incl. the grid-barrier kernels) while the slice is ingested -- only for slices of
    >= 1 GiB by default; DMDX_PRIME_MIN_BYTES=0 forces it here.  The decomposition must be the one
    a run without the primer returns (no test ran with priming on)."""
    from dmd_era5_amd import era5_svd
    from dmd_era5_amd.era5_svd import main

    cfg = dict(svd_base_config, start_datetime="2019-01-01T00", end_datetime="2019-01-04T00",
               variables="temperature,u_component_of_wind", levels="1000,850", svd_type=svd_type,
               mean_center=True, scale=False, delay_embedding=2, n_components=5, svd_seed=0)
    _write_slice(cfg, seed=21, dtype=np.float32)
    monkeypatch.setenv("DMDX_NO_PRIME", "1")
    off, _, _ = main(cfg)
    monkeypatch.delenv("DMDX_NO_PRIME")
    monkeypatch.setenv("DMDX_PRIME_MIN_BYTES", "0")
    era5_svd._PRIMED.clear()
    started = []
    real = era5_svd._prime_async

    def spy(device, typ):
        t = real(device, typ)
        started.append(t)
        return t

    monkeypatch.setattr(era5_svd, "_prime_async", spy)
    on, _, _ = main(cfg)
    assert started and started[0] is not None and not started[0].is_alive()
    for name in ("U", "s", "V"):
        assert np.array_equal(on[name].values, off[name].values), name


@pytest.mark.parametrize("svd_type,d,scale", [("standard", 1, False), ("standard", 2, True), ("randomized", 1, False)])
def test_main_on_a_grid_whose_point_count_is_not_a_multiple_of_four(svd_base_config, project_root, monkeypatch, svd_type, d, scale):
    """35 x 71 grid points x 2 levels = 4970 space points per variable (4970 % 4 = 2): the ingest
    appends two zero space points per variable so that the aligned kernel bodies run, and main()
    must give back exactly the rows of the reference pipeline (no trace of the padding in U, X,
    X_mean or the labels)."""
    from dmd_era5_amd import era5_svd, io_netcdf
    from dmd_era5_amd.config_parser import config_parser
    from dmd_era5_amd.create_mock_data import add_download_attributes, create_mock_era5
    from dmd_era5_amd.labeled import Coord, DataArray, Dataset

    cfg = dict(svd_base_config, start_datetime="2019-01-01T00", end_datetime="2019-01-03T00",
               variables="temperature,u_component_of_wind", levels="1000,850", svd_type=svd_type,
               mean_center=True, scale=scale, delay_embedding=d, n_components=5,
               save_data_matrix=True, svd_seed=0)
    p = config_parser(cfg, "era5-svd")
    full = create_mock_era5(cfg["start_datetime"], cfg["end_datetime"], p["variables"], p["levels"], seed=11, dtype=np.float32)
    cds = {"time": full.coords["time"], "level": full.coords["level"],
           "latitude": Coord("latitude", full.coords["latitude"].values[:35]),
           "longitude": Coord("longitude", full.coords["longitude"].values[:71])}
    ds = Dataset(coords=cds, attrs=dict(full.attrs))
    for name in p["variables"]:
        ds[name] = DataArray(np.ascontiguousarray(full[name].values[:, :, :35, :71]), full[name].dims, cds, dict(full[name].attrs))
    io_netcdf.to_netcdf(add_download_attributes(ds, p), p["era5_slice_path"])

    seen = []
    real = era5_svd._upload_variable
    monkeypatch.setattr(era5_svd, "_upload_variable",
                        lambda *a, **k: (lambda out: (seen.append([int(b.shape[1]) for b in out[0]]), out)[1])(real(*a, **k)))
    res, _, _ = era5_svd.main(cfg, write_to_netcdf=False)
    assert seen == [[4972], [4972]]                      # the blocks the kernels saw were padded

    variables = {k: ds[k].values for k in p["variables"]}
    X, X_mean, X_std = orc.preprocess(variables, True, scale, d)
    m = X.shape[0]
    assert m == d * 2 * 4970 and res["U"].shape == (m, 5) and res["X"].shape == X.shape
    assert np.allclose(res["X"].values, X, rtol=0, atol=2e-4 * (1 if scale else 30))
    if svd_type == "standard":
        Uo, so, Vo = orc.svd_standard(X.astype(np.float64), 5)
        assert np.allclose(res["s"].values, so, rtol=2e-5)
        rec = (res["U"].values.astype(np.float64) * res["s"].values) @ res["V"].values
        assert np.linalg.norm(rec - (Uo * so) @ Vo) <= 2e-3 * np.linalg.norm((Uo * so) @ Vo)
    else:
        Ur, sr, Vr = orc.svd_randomized(X, 5, random_state=0)
        assert np.allclose(res["s"].values, sr, rtol=1e-3)
    U = res["U"].values.astype(np.float64)
    assert np.abs(U.T @ U - np.eye(5)).max() < 1e-4
    assert np.array_equal(res.coords["space"].values, np.arange(m))
    if d > 1:
        assert np.allclose(res["X_mean"].values, X_mean, rtol=1e-5, atol=2e-4)
        if scale:
            assert np.allclose(res["X_std"].values, X_std, rtol=1e-5)
