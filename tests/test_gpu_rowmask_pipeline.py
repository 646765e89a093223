"""``missing = "mask"`` end to end on the GPU: ``main()`` on the HIP provider through a NETCDF4 file whose temperature
is missing over a static "land" mask -- stored as CF-packed int16 with fill codes (K14 turns them into NaN) and as
float32 with a NaN ``_FillValue`` (the direct route) --, K20 counting and zeroing the rows, and a DMD restart from
masked analyses.  35 x 71 points per level: an odd point count, so the row blocks carry ``pad4`` rows.

The reference is tests/rowmask_ref.py (masked points dropped, ``np.linalg.svd`` in fp64); tolerances and the sign
convention are those of tests/test_gpu_pipeline.py::test_main_matches_oracle_pipeline.
"""
import numpy as np
import pytest
import torch

import rowmask_ref as rr
import unpack_ref as ur
from oracle import era5_oracle as orc

pytestmark = pytest.mark.gpu

FILL = -32767
NT, NLEV, NLAT, NLON = 25, 2, 35, 71
VARS = ("temperature", "u_component_of_wind")
K = 5
PLANE = NLEV * NLAT * NLON


def _fields():
    """Mock fields with three planted space-time patterns, noise well above the packing step; the planted mask."""
    from dmd_era5_amd.create_mock_data import create_mock_era5

    full = create_mock_era5("2019-01-01T00", "2019-01-02T00", list(VARS), [1000, 850], seed=21, dtype=np.float32)
    assert full[VARS[0]].shape[0] == NT
    t = np.arange(NT, dtype=np.float64)[:, None, None, None]
    lat = np.radians(full.coords["latitude"].values[:NLAT])[None, None, :, None]
    lon = np.radians(full.coords["longitude"].values[:NLON])[None, None, None, :]
    out, rs = {}, np.random.RandomState(5)
    for v, name in enumerate(VARS):
        f = full[name].values[:, :, :NLAT, :NLON].astype(np.float64) + rs.standard_normal((NT, NLEV, NLAT, NLON))
        f = f + 60 * np.sin(2 * np.pi * t / 24) * np.cos(lat) * np.cos(lon + v) + 35 * np.cos(2 * np.pi * t / 11) * np.sin(2 * lat) * np.sin(2 * lon)
        out[name] = f + 20 * (t / NT) ** 2 * np.cos(3 * lon) * np.ones_like(lat)
    land = rs.rand(NLAT, NLON) < 0.3
    land[0, 0], land[NLAT - 1, NLON - 1], land[17, 30] = True, False, False
    # the last point of the last level (the ragged quad of the last row block), and three more, in a few snapshots
    partly = [(3, 1, NLAT - 1, NLON - 1), (NT - 1, 1, NLAT - 1, NLON - 1), (0, 1, 17, 30), (7, 0, 20, 1), (8, 0, 20, 1)]
    where = np.zeros((NT, NLEV, NLAT, NLON), dtype=bool)
    where[:, :, land] = True
    for idx in partly:
        where[idx] = True
    used = np.ones((2, NLEV, NLAT, NLON), dtype=bool)
    used[0] = ~where.any(axis=0)
    return full, out, where, used.reshape(-1)


def _datasets():
    """-> (packed int16 Dataset with fill codes, float32 Dataset with a NaN _FillValue, the decoded values of each,
    the used points)."""
    from dmd_era5_amd.labeled import Coord, DataArray, Dataset

    full, fields, where, used = _fields()
    cds = {"time": full.coords["time"], "level": full.coords["level"],
           "latitude": Coord("latitude", full.coords["latitude"].values[:NLAT]),
           "longitude": Coord("longitude", full.coords["longitude"].values[:NLON])}
    packed, plain = Dataset(coords=cds, attrs=dict(full.attrs)), Dataset(coords=cds, attrs=dict(full.attrs))
    decoded = {"packed": {}, "direct": {}}
    for name, f in fields.items():
        lo, hi = float(f.min()), float(f.max())
        sf, ao = (hi - lo) / 65000.0, (hi + lo) / 2.0
        q = ur.pack(f, sf, ao)
        q[q == FILL] = 0
        g = f.astype(np.float32)
        if name == VARS[0]:
            q[where] = FILL
            g[where] = np.nan
        packed[name] = DataArray(q, full[name].dims, cds, dict(full[name].attrs, scale_factor=np.float64(sf),
                                                                add_offset=np.float64(ao), _FillValue=np.int16(FILL)))
        plain[name] = DataArray(g, full[name].dims, cds, dict(full[name].attrs, _FillValue=np.float32(np.nan)))
        decoded["packed"][name] = ur.decode(q, sf, ao, (FILL,))
        decoded["direct"][name] = g
    return {"packed": packed, "direct": plain}, decoded, used


@pytest.fixture
def small_slabs(monkeypatch):
    """Every variable file-backed, several slabs per variable on both routes."""
    from dmd_era5_amd import era5_svd, hdf5_lite, io_netcdf

    if not hdf5_lite.available():
        pytest.fail("libhdf5 not found: the routes under test read HDF5 slices")
    monkeypatch.setenv("DMDX_NETCDF_BACKEND", "hdf5")
    monkeypatch.setattr(io_netcdf, "LAZY_BYTES", 1000)
    monkeypatch.setattr(era5_svd, "SLAB_BYTES", 9 * NLEV * NLAT * NLON * 4)


def _cfg(base, svd_type, scale, **more):
    cfg = dict(base, start_datetime="2019-01-01T00", end_datetime="2019-01-02T00", variables=",".join(VARS),
               levels="1000,850", svd_type=svd_type, mean_center=True, scale=scale, delay_embedding=2,
               n_components=K, save_data_matrix=True, svd_seed=0, missing="mask")
    cfg.update(more)
    return cfg


def _main_on(root, monkeypatch, ds, cfg):
    from dmd_era5_amd import io_netcdf
    from dmd_era5_amd.config_parser import config_parser
    from dmd_era5_amd.create_mock_data import add_download_attributes
    from dmd_era5_amd.era5_svd import main
    from dmd_era5_amd.kernels import default_kernels

    root.mkdir(exist_ok=True)
    monkeypatch.setenv("DMD_ERA5_ROOT", str(root))
    p = config_parser(cfg, "era5-svd")
    io_netcdf.to_netcdf(add_download_attributes(ds, p), p["era5_slice_path"])
    kern = default_kernels()
    kern.events = []
    try:
        res, _, _ = main(cfg, write_to_netcdf=True)
        torch.cuda.synchronize()
        launched = [e[0] for e in kern.events]
    finally:
        kern.events = None
    return res, io_netcdf.open_dataset(p["save_path"]), launched


@pytest.mark.parametrize("route", ["packed", "direct"])
@pytest.mark.parametrize("svd_type,scale", [("standard", True), ("randomized", False)])
def test_main_masks_the_land_points_on_the_hip_provider(svd_base_config, tmp_path, monkeypatch, small_slabs, route,
                                                        svd_type, scale):
    sets, decoded, want_used = _datasets()
    res, back, launched = _main_on(tmp_path / route, monkeypatch, sets[route], _cfg(svd_base_config, svd_type, scale))
    # the route under test ran, and K20 did the counting and the zeroing (X blocks, then the U blocks)
    assert ("unpack_i16" in launched) == (route == "packed")
    assert "row_missing_count" in launched and launched.count("row_mask_apply") >= 2
    M, d = want_used.size, 2
    assert PLANE % 4 != 0                                                             # pad4 was in play (per variable)
    used = np.tile(want_used, d)
    mask = np.asarray(res["space_mask"].values)
    assert mask.dtype == np.int8 and np.array_equal(mask, used.astype(np.int8))       # the planted mask, exactly
    assert res.attrs["missing"] == "mask" and res.attrs["masked_points"] == int((~want_used).sum())
    U, s, V = (np.asarray(res[k].values) for k in ("U", "s", "V"))
    assert U.shape == (d * M, K) and U.dtype == np.float32 and (U[~used] == 0).all()
    Xv = np.asarray(res["X"].values)
    assert (Xv[~used] == 0).all() and np.isfinite(Xv).all()                           # the zeros that were decomposed
    ref = rr.masked_svd(decoded[route], True, scale, d, K)
    assert np.array_equal(ref["used"], want_used)
    assert np.allclose(Xv[used], ref["X"], rtol=0, atol=2e-4 * (1 if scale else 30))
    want = (ref["U"] * ref["s"]) @ ref["V"]
    if svd_type == "standard":
        assert np.allclose(s, ref["s"], rtol=2e-5)
    else:
        Ur, sr, Vr = orc.svd_randomized(ref["X"], K, random_state=0)
        assert np.allclose(s, sr, rtol=1e-3)
        assert np.all(s <= ref["s"] * (1 + 1e-5)) and np.all(s >= 0.95 * ref["s"])
        want = (Ur * sr) @ Vr
    Uu = U[used].astype(np.float64)
    rec = (Uu * s.astype(np.float64)) @ V.astype(np.float64)
    assert np.linalg.norm(rec - want) <= 2e-3 * np.linalg.norm(want)
    assert np.abs(Uu.T @ Uu - np.eye(K)).max() < 1e-4
    assert np.all(U[np.abs(U).argmax(axis=0), np.arange(K)] > 0)                      # u-based sign convention
    Xm = np.asarray(res["X_mean"].values)
    assert np.array_equal(np.isnan(Xm), ~used)
    assert np.allclose(Xm[used], np.tile(ref["mean"], d), rtol=1e-5, atol=2e-4)
    if scale:
        Xs = np.asarray(res["X_std"].values)
        assert np.array_equal(np.isnan(Xs), ~used) and np.allclose(Xs[used], np.tile(ref["std"], d), rtol=1e-5)
    # the written file
    assert back["space_mask"].values.dtype == np.int8 and np.array_equal(back["space_mask"].values, mask)
    assert np.array_equal(back["U"].values, U) and back.attrs["missing"] == "mask"
    assert np.array_equal(np.isnan(back["X_mean"].values), ~used)


def test_reconstruction_projection_and_restart_from_masked_analyses(svd_base_config, tmp_path, monkeypatch, small_slabs):
    from dmd_era5_amd import era5_svd
    from dmd_era5_amd import forecast as fc
    from dmd_era5_amd.bopdmd import OptDMDResult
    from dmd_era5_amd.kernels import default_kernels

    sets, decoded, want_used = _datasets()
    res, back, _ = _main_on(tmp_path / "r", monkeypatch, sets["direct"],
                            _cfg(svd_base_config, "standard", True, n_components=NT - 1))
    M, d = want_used.size, 2
    used = np.tile(want_used, d)
    kern = default_kernels()
    # reconstruction: NaN exactly at the masked points, through the mean and through K20
    R = era5_svd.reconstruct_from_svd_results(back).values
    assert np.array_equal(np.isnan(R), np.repeat((~used)[:, None], R.shape[1], axis=1))
    Rs = era5_svd.reconstruct_from_svd_results(back, destandardize=False).values
    Xv = np.asarray(res["X"].values)
    assert np.array_equal(np.isnan(Rs), np.isnan(R)) and np.abs(Rs[used] - Xv[used]).max() <= 2e-4 * np.abs(Xv).max()
    # projection of the raw snapshots (NaN at the masked rows): finite, the energy of the compacted ones
    raw, _ = orc.flatten(decoded["direct"])                                           # (M, NT) fp32
    E = np.ascontiguousarray(orc.delay_embed(np.ascontiguousarray(raw), d))
    keep = E.copy()
    C = era5_svd.project_onto_svd_results(back, E)
    assert np.array_equal(rr.bits(E), rr.bits(keep)) and np.isfinite(C.values).all()
    mu, sd = (np.asarray(back[k].values, dtype=np.float64) for k in ("X_mean", "X_std"))
    Z = (E[used].astype(np.float64) - mu[used, None]) / sd[used, None]
    assert C.attrs["energy_total"] == pytest.approx(float((Z * Z).sum()), rel=1e-5)
    want = np.asarray(back["U"].values, dtype=np.float64)[used].T @ Z
    assert np.abs(C.values - want).max() <= 1e-4 * np.abs(want).max()
    # a bundle with masks: restart from masked analyses, fields with NaN at the masked points, fill codes in the pack
    dev = torch.device("cuda", torch.cuda.current_device())
    Uv = np.asarray(back["U"].values)
    spans = [(0, 3001), (3001, M)]                                                    # (an odd cut: a dword-route block)

    def t32(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)

    Ub = [t32(np.concatenate([Uv[j * M + a:j * M + b] for j in range(d)]).T) for a, b in spans]
    means, stds = ([t32(np.asarray(back[k].values)[a:b]) for a, b in spans] for k in ("X_mean", "X_std"))
    masks = [torch.from_numpy(want_used[a:b].astype(np.int8)).to(dev) for a, b in spans]
    k = int(Ub[0].shape[0])
    rs = np.random.RandomState(0)
    half = np.array([-0.05 + 1.0j, -0.2 + 2.5j])
    mh = rs.standard_normal((k, 2)) + 1j * rs.standard_normal((k, 2))
    model = OptDMDResult(eigs=torch.from_numpy(np.concatenate([half, half.conj()])),
                         modes=torch.from_numpy(np.concatenate([mh, mh.conj()], axis=1)),
                         amplitudes=torch.from_numpy(np.ones(4)), rel_error=0.0, n_iter=0, converged=True)
    f = fc.DmdForecast(Ub, model, means, stds, d, kern=kern, masks=masks)
    Xb = [t32(raw[a:b].T) for a, b in spans]
    before = [X.clone() for X in Xb]
    g = f.restart(Xb, np.arange(NT - 1.0))
    for X, X0, m in zip(Xb, before, masks):
        assert (X[:, m == 0] == 0).all()                                              # zeroed in place ...
        assert torch.equal(X[:, m != 0].view(torch.int32), X0[:, m != 0].view(torch.int32))   # ... the rest bit for bit
    assert g.masks is masks and torch.isfinite(g.result.amplitudes).all() and np.isfinite(g.result.rel_error)
    proj = f.project([X.clone() for X in before])
    assert np.abs(proj["Ct"].cpu().numpy().T - want).max() <= 1e-4 * np.abs(want).max()
    T = 4
    fields = torch.cat(g.fields(np.arange(T, dtype=np.float64)), dim=1).cpu().numpy()
    assert np.array_equal(np.isnan(fields), np.repeat((~want_used)[None], T, axis=0))
    groups = [torch.from_numpy(np.arange(a, b) // PLANE) for a, b in spans]
    packed = g.pack(np.arange(T, dtype=np.float64), groups=groups)
    codes = torch.cat(packed["codes"], dim=1).cpu().numpy()
    assert np.array_equal(codes == -32768, np.repeat((~want_used)[None], T, axis=0))
    assert [int(c[0]) for c in packed["counts"].cpu().tolist()] == [T * int((~want_used[:PLANE]).sum()), 0]
