"""Drop-in for the reference's SVD driver ``dmd_era5.era5_svd.era5_svd``
(ref: /root/reference/src/dmd_era5/era5_svd/era5_svd.py).

Same public names (``__all__`` of ref: src/dmd_era5/era5_svd/__init__.py:10-17), same
arguments, same return shapes, same exception messages:

    svd_on_era5(da, parsed_config) -> (U (m,k), s (k,), V (k,n))      ref :230-263
    combine_svd_results(U, s, V, coords, X=, X_mean=, X_std=)           ref :266-333
    add_config_attributes(ds, parsed_config)                            ref :42-66
    retrieve_era5_slice / retrieve_svd_results (working-directory branch) ref :69-227
    main(config, write_to_netcdf=False, use_dvc=False)                  ref :336-453
    python -m dmd_era5_amd.era5_svd  (and the ``dmd_era5`` alias package) ref :456-478

What differs is where the arithmetic runs: ``svd_on_era5`` hands X to the MI355X
engine (:mod:`dmd_era5_amd.engine`), and ``main`` never materialises X on the host at
all -- each variable of the slice is uploaded once as ``(time, space)`` row blocks,
centred / scaled in place by K5, delay-embedded as a zero-copy view and decomposed on
the device (the reference holds ~5 copies of X in host RAM).
DVC (``use_dvc=True``) is out of scope and raises.

Optional engine keys in the config dict (absent from the reference, defaults reproduce
its behaviour): ``svd_seed`` (int, makes "randomized" reproducible), ``n_oversamples``,
``n_iter``, and ``missing``: ``"raise"`` (the default) refuses a slice with missing values;
``"mask"`` takes every grid point that is missing (fill value, NaN, Inf) in at least one selected
snapshot out of the decomposition (K20: its rows of X are zero, so are its rows of U) and
returns it as missing: the result gains ``space_mask`` (int8 over ``space``, 1 = used) and the
attributes ``missing`` / ``masked_points``, ``X_mean`` / ``X_std`` are NaN there, and
``reconstruct_from_svd_results`` / ``write_forecast_slice`` give NaN / ``_FillValue`` at those
points.  Sea-surface temperature, missing over land in every file, needs it.
"""
from __future__ import annotations

import logging
import os
import sys
from dataclasses import dataclass
from datetime import datetime

import numpy as np

from . import io_netcdf
from .config_parser import config_parser
from .config_reader import config_reader
from .labeled import Coord, DataArray, Dataset
from .logger import log_and_print, setup_logger
from .slice_tools import (
    apply_delay_embedding,
    delay_coords,
    flatten_era5_variables,
    nearest_resample_index,
    resample_era5_dataset,
    slice_era5_dataset,
    space_coord_to_level_lat_lon,
    space_labels,
    standardize_data,
)

__all__ = [
    "svd_on_era5",
    "combine_svd_results",
    "retrieve_era5_slice",
    "retrieve_svd_results",
    "add_config_attributes",
    "main",
    "reconstruct_from_svd_results",
    "project_onto_svd_results",
    "write_forecast_slice",
]

logger = setup_logger("ERA5-SVD", "era5_svd.log")
_console = logging.StreamHandler(sys.stdout)
_console.setFormatter(logging.Formatter("%(asctime)s - %(name)s - %(levelname)s - %(message)s"))
logger.addHandler(_console)

_ENGINE_KEYS = {"svd_seed": "random_state", "n_oversamples": "n_oversamples", "n_iter": "n_iter"}


MISSING_MODES = ("raise", "mask")


def _missing_mode(config: dict) -> str:
    """The engine-only key ``missing`` of a config / parsed config; absent means "raise"."""
    mode = config.get("missing", "raise")
    if mode not in MISSING_MODES:
        raise ValueError(f'missing = {mode!r} is not supported: use "raise" (refuse a slice with missing values, '
                         'the default) or "mask" (leave the affected grid points out of the decomposition)')
    return mode


def _engine_opts(parsed_config: dict) -> dict:
    if parsed_config["svd_type"] != "randomized":
        return {}
    return {dst: parsed_config[src] for src, dst in _ENGINE_KEYS.items() if src in parsed_config}


def add_config_attributes(ds: Dataset, parsed_config: dict) -> Dataset:
    """Configuration settings as attributes of the result (ref :42-66)."""
    a = ds.attrs
    a["source_path"] = parsed_config["source_path"]
    a["n_components"] = parsed_config["n_components"]
    a["variables"] = parsed_config["variables"]
    a["levels"] = parsed_config["levels"]
    a["mean_center"] = int(parsed_config["mean_center"])
    a["scale"] = int(parsed_config["scale"])
    a["delay_embedding"] = parsed_config["delay_embedding"]
    a["svd_type"] = parsed_config["svd_type"]
    a["era5_slice_path"] = parsed_config["era5_slice_path"]
    a["date_processed"] = datetime.now().isoformat()
    a["save_data_matrix"] = int(parsed_config["save_data_matrix"])
    return ds


def _as_str_list(obj) -> list[str]:
    if isinstance(obj, str):
        return obj.split(",") if "," in obj else [obj]
    return [str(x) for x in np.atleast_1d(obj).tolist()]


def _as_int_list(obj) -> list[int]:
    arr = np.atleast_1d(obj)
    if not np.issubdtype(arr.dtype, np.integer):
        raise ValueError("Levels must be integers.")
    return [int(x) for x in arr.tolist()]


def _no_dvc(use_dvc: bool) -> None:
    if use_dvc:
        raise NotImplementedError("DVC data versioning is outside the scope of dmd_era5_amd "
                                  "(SURVEY.md section 2 row 6); call with use_dvc=False")


def retrieve_era5_slice(parsed_config: dict, use_dvc: bool = False):
    """ERA5 slice from the working directory (ref :69-154, no-DVC branch): accepted iff the
    requested variables / levels are contained in the file's and ``source_path`` matches."""
    _no_dvc(use_dvc)
    path = parsed_config["era5_slice_path"]
    if not os.path.exists(path):
        log_and_print(logger, "ERA5 slice not found in working directory.", "warning")
        return None, False
    log_and_print(logger, "ERA5 slice found in working directory.")
    ds = io_netcdf.open_dataset(path)
    want_v, want_l = parsed_config["variables"], parsed_config["levels"]
    ok = (sorted(want_v) == sorted(set(_as_str_list(ds.attrs["variables"])) & set(want_v))
          and sorted(want_l) == sorted(set(_as_int_list(ds.attrs["levels"])) & set(want_l))
          and parsed_config["source_path"] == ds.attrs["source_path"])
    if ok:
        log_and_print(logger, "ERA5 slice matches configuration.")
        return ds, False
    log_and_print(logger, "ERA5 slice does not match configuration.")
    log_and_print(logger, "ERA5 slice in working directory does not match configuration.", "warning")
    return None, False


def retrieve_svd_results(parsed_config: dict, use_dvc: bool = False):
    """Cached SVD result from the working directory (ref :157-227, no-DVC branch).  The key
    is the attribute set of ref :178-188 (svd_type is *not* part of it, as in the reference)."""
    _no_dvc(use_dvc)
    path = parsed_config["save_path"]
    if not os.path.exists(path):
        log_and_print(logger, "SVD results not found in working directory.", "warning")
        return None, False
    log_and_print(logger, "SVD results found in working directory.")
    ds = io_netcdf.open_dataset(path)
    a = ds.attrs
    ok = (parsed_config["source_path"] == a["source_path"]
          and parsed_config["n_components"] == a["n_components"]
          and parsed_config["variables"] == _as_str_list(a["variables"])
          and parsed_config["levels"] == _as_int_list(a["levels"])
          and parsed_config["mean_center"] == a["mean_center"]
          and parsed_config["scale"] == a["scale"]
          and parsed_config["delay_embedding"] == a["delay_embedding"])
    if ok:
        log_and_print(logger, "SVD results match configuration.")
        return ds, False
    log_and_print(logger, "SVD results do not match configuration.")
    log_and_print(logger, "SVD results in working directory do not match configuration.", "warning")
    return None, False


def svd_on_era5(da, parsed_config: dict):
    """Rank-``n_components`` SVD of the pre-processed slice (ref :230-263) on the MI355X.

    ``da``: anything with ``.values`` of shape (space, time) -- our DataArray or a real
    ``xr.DataArray`` -- or the ndarray itself.  Returns numpy ``(U, s, V)`` in X's dtype."""
    from .engine import svd_numpy

    X = da.values if hasattr(da, "values") else np.asarray(da)
    svd_type = parsed_config["svd_type"]
    n_components = parsed_config["n_components"]
    if svd_type == "standard":
        log_and_print(logger, "Performing standard SVD...")
    elif svd_type == "randomized":
        log_and_print(logger, "Performing randomized SVD...")
    else:
        raise ValueError(f"SVD type {svd_type} is not supported.")
    from .engine import FP64_MAX_BYTES

    if getattr(X, "dtype", None) == np.float64 and X.nbytes > FP64_MAX_BYTES:
        log_and_print(logger, "Input is float64 and larger than the fp64 path takes: the engine computes it in "
                              "fp32 on the MFMA units (the reference's ERA5 slices are float32) and returns "
                              "float64 arrays that carry ~1e-6 relative accuracy, not LAPACK's 1e-12.",
                      level="warning")
    U, s, V = svd_numpy(X, svd_type, n_components, **_engine_opts(parsed_config))
    if s.size and float(s[0]) > 0 and float(s[-1]) <= 1e-7 * float(s[0]):
        log_and_print(logger, "Singular values below 1e-7 s_1 are under the fp32 resolution of the data: their "
                              "columns of U are an arbitrary orthonormal completion (as LAPACK's are for zero "
                              "singular values), not directions of the data.", level="warning")
    log_and_print(logger, f"{svd_type.capitalize()} SVD complete.")
    return U, s, V


def combine_svd_results(U, s, V, coords, **kwargs) -> Dataset:
    """U(space, components), s(components), V(components, time) [+ X, X_mean, X_std] as
    one Dataset with the coordinates of the decomposed array (ref :266-333).  ``space_mask=`` (with
    ``masked_points=``, the number of grid points left out): the result of ``missing = "mask"`` -- one more
    variable ``space_mask`` over ``space`` (int8, 1 = used in the decomposition) and the attributes ``missing``
    and ``masked_points``; absent otherwise."""
    comp = np.arange(U.shape[1])
    row = {k: coords[k] for k in ("space", "original_variable", "delay") if k in coords}
    cds = dict(coords)
    cds["components"] = Coord("components", comp)
    ds = Dataset(coords=cds)
    ds["U"] = DataArray(U, ("space", "components"), {**row, "components": cds["components"]})
    ds["s"] = DataArray(s, ("components",), {"components": Coord("components", np.arange(s.shape[0]))})
    ds["V"] = DataArray(V, ("components", "time"),
                        {"components": Coord("components", np.arange(V.shape[0])), "time": coords["time"]})
    for key in ("X", "X_mean", "X_std"):
        if kwargs.get(key) is not None:
            ds[key] = kwargs[key]
    if kwargs.get("space_mask") is not None:
        # missing = "mask": which rows took part (1) and which were left out and are missing in every product (0)
        mask = kwargs["space_mask"]
        if not isinstance(mask, DataArray):
            mask = DataArray(np.asarray(mask).astype(np.int8), ("space",), {k: v for k, v in row.items() if k != "delay"})
        ds["space_mask"] = mask
        ds.attrs["missing"] = "mask"
        points = kwargs.get("masked_points")
        if points is None:                           # (grid points, not embedded rows: every delay block repeats them)
            d = int(np.unique(coords["delay"].values).size) if "delay" in coords else 1
            points = int((np.asarray(mask.values) == 0).sum()) // d
        ds.attrs["masked_points"] = int(points)
    return ds


def reconstruct_from_svd_results(svd_ds: Dataset, n_components: int | None = None, times=None,
                                 destandardize: bool = True, kern=None) -> DataArray:
    """The data matrix of an SVD result, regenerated from its factors: ``U[:, :r] diag(s[:r]) V[:r, times]``
    as the ``(space, time)`` DataArray the file's own ``X`` variable is (same coordinates and dtype) --
    what ``save_data_matrix = False`` left out, or its rank-r approximation.

    ``svd_ds``: the Dataset ``main()`` returns or ``retrieve_svd_results`` loads.  ``n_components``: r
    (default: all stored).  ``times``: indices into the file's time axis (default: all).
    ``destandardize``: apply ``X_std`` and ``X_mean`` when the file has them (it has them only for a
    delay embedding d > 1 -- the reference's quirk, ref :400-414 -- so for d = 1 the standardized
    matrix is what comes back either way).  fp32 results are formed by K12 on the device in row
    blocks; float64 results (the small-slice fp64 route) take the library's fp64 product.
    A result of ``missing = "mask"`` comes back with NaN at the masked points: through their NaN mean
    when the mean is applied, through K20 on the expanded block otherwise."""
    U, s, V = (np.asarray(svd_ds[k].values) for k in ("U", "s", "V"))
    k = int(s.shape[0])
    r = k if n_components is None else int(n_components)
    if not 1 <= r <= k:
        raise ValueError(f"n_components = {r} outside 1 .. {k}")
    tidx = np.arange(V.shape[1]) if times is None else np.atleast_1d(np.asarray(times, dtype=np.int64))
    names = set(svd_ds.data_vars)
    mu = np.asarray(svd_ds["X_mean"].values) if destandardize and "X_mean" in names else None
    sd = np.asarray(svd_ds["X_std"].values) if destandardize and "X_std" in names else None
    M = int(U.shape[0])
    # a result of missing = "mask": NaN at the masked points -- through the NaN of their mean where there is one
    gone = np.asarray(svd_ds["space_mask"].values) == 0 if "space_mask" in names and mu is None else None
    if U.dtype == np.float64:
        X = (U[:, :r] * s[:r]) @ V[:r][:, tidx]
        if sd is not None:
            X *= sd[:, None]
        if mu is not None:
            X += mu[:, None]
        if gone is not None:
            X[gone] = np.nan
    else:
        import torch

        from . import forecast
        from .svd import _kern, row_mask_apply_, split_rows

        kern = _kern(kern)
        dev = torch.device("cuda" if getattr(kern, "name", "") == "hip" else "cpu")
        Ct = forecast.svd_coefficients(torch.from_numpy(s[:r].astype(np.float64)),
                                       torch.from_numpy(V[:r].astype(np.float64)), torch.from_numpy(tidx)).to(dev)
        X = np.empty((M, tidx.shape[0]), dtype=U.dtype)
        for a, b in split_rows(M):
            Ut = torch.from_numpy(np.ascontiguousarray(U[a:b, :r].T.astype(np.float32, copy=False))).to(dev)
            vec = [None if v is None else [torch.from_numpy(np.ascontiguousarray(v[a:b], dtype=np.float32))] for v in (mu, sd)]
            (Xt,) = forecast.expand_blocks([Ut], Ct, vec[0], vec[1], kern=kern)
            if gone is not None:
                row_mask_apply_(kern, Xt, torch.from_numpy(gone[a:b].astype(np.int32)).to(dev), float("nan"))
            X[a:b] = Xt.T.cpu().numpy()
            del Xt, Ut
    row = {c: svd_ds.coords[c] for c in ("space", "original_variable", "delay", "time") if c in svd_ds.coords}
    if times is not None:
        tc = svd_ds.coords["time"]
        row["time"] = Coord("time", np.asarray(tc.values)[tidx])
    return DataArray(X, ("space", "time"), row)


# pinned staging of write_forecast_slice: the codes of one time slab of all variables (2 bytes per value)
FORECAST_STAGE_BYTES = 256 << 20


def write_forecast_slice(path: str, forecast, t, time, variables, levels, latitude, longitude, *, packing=None,
                         ensemble: bool = False, spread: bool = False, slab: int | None = None,
                         attrs: dict | None = None, climatology=None, trend=None, trend_extra=None) -> dict:
    """The fields of a :class:`forecast.DmdForecast` at the model times ``t`` as a NETCDF4 file in the schema of the
    input slice: one ``int16`` variable ``(time, level, latitude, longitude)`` per name with ``scale_factor``,
    ``add_offset`` (float64) and ``_FillValue`` (int16 -32768), the coordinate variables, and the global attributes
    ``retrieve_era5_slice`` keys on -- the file is a valid input slice of :func:`main`.  The codes are formed on the
    device where the field is formed (K17): no fp32 field is stored, and 2 bytes per value cross PCIe and reach the
    file.

    ``time``: the time coordinate of the file, one entry per entry of ``t`` (datetime64, or numbers stored as they
    are).  ``variables`` / ``levels`` / ``latitude`` / ``longitude``: the names and coordinates of the grid; the rows
    of the forecast's U blocks (together) follow ``flatten_era5_variables``' order -- variable, then level, latitude,
    longitude -- and one variable is one group: one ``scale_factor`` per file variable.  A forecast whose U blocks
    are delay-embedded writes delay block 0, the physical fields.
    ``packing``: None chooses ``Packing.for_range`` of every variable's finite values over ALL of ``t`` in a range
    pass of its own, which forms coefficients and partial extrema only; a dict name -> Packing (or a list in the
    order of ``variables``) is taken as it is -- the analysis file's own packing: one pass, comparable codes.
    ``ensemble=True`` writes the ensemble mean of a bagged fit, ``spread=True`` adds the K15 spread of the same
    times as ``<name>_spread`` variables (always packed by their own range).
    ``slab``: snapshots per slab of the walk along the time axis -- expand_pack into a device int16 slab, one
    device-to-host copy of the codes, ``Writer.write_slab``; by default what fits ``FORECAST_STAGE_BYTES`` of
    (pinned) staging.  ``attrs``: more global attributes (``source_path`` among them, if ``main`` is to accept the
    file for a configuration).
    ``climatology``: a :class:`climatology.Climatology` the model was fitted on the anomalies of (``time`` must then
    be datetime64).  A time slab is expanded to fp32 (K12), the climatology of its times is put back in place (K18) and
    the slab is packed as a field (K17's streaming pair): one fp32 slab is stored.  The range pass, when no packing is
    given, runs on the restored fields.  The spread has no offset and is written as without a climatology.
    ``trend``: a :class:`trend.Trend` that was removed (after the climatology) before the fit (``time`` must be
    datetime64; ``trend_extra``: its user series at ``time``, one row per entry, if it has any).  It is put back on the
    fp32 slab (K21) before the climatology, on the same route.

    Returns ``{"packing": {name: Packing}, "filled": {name: int}, "saturated": {name: int}}`` over the file's
    variables: the values that were not finite and became ``_FillValue``, and those a given packing clamped."""
    import torch

    from . import forecast as fc
    from . import hdf5_lite
    from .labeled import Packing

    if not hdf5_lite.available():
        raise RuntimeError("write_forecast_slice writes NETCDF4 / HDF5 and libhdf5 was not found (set DMDX_HDF5_LIB)")
    if spread and not ensemble:
        raise ValueError("write_forecast_slice: spread=True needs ensemble=True")
    variables = _as_str_list(variables)
    levels, lat, lon = np.atleast_1d(np.asarray(levels)), np.atleast_1d(np.asarray(latitude)), np.atleast_1d(np.asarray(longitude))
    time = np.atleast_1d(np.asarray(time))
    tt = torch.as_tensor(t, dtype=torch.float64).reshape(-1)
    T, plane = int(tt.numel()), int(levels.size * lat.size * lon.size)
    if time.shape != (T,):
        raise ValueError(f"write_forecast_slice: {time.shape[0] if time.ndim == 1 else time.shape} time labels for {T} times")
    nvar, d = len(variables), int(forecast.delay)
    Ub = list(forecast.Ublocks)
    rows = [int(U.shape[1]) // d for U in Ub]
    M = sum(rows)
    if M != nvar * plane or any(int(U.shape[1]) % d for U in Ub):
        raise ValueError(f"write_forecast_slice: the U blocks hold {M} physical rows, {nvar} variables x "
                         f"{levels.size} levels x {lat.size} x {lon.size} points are {nvar * plane}")
    starts = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    groups = [torch.from_numpy(np.arange(a, b, dtype=np.int64) // plane) for a, b in zip(starts[:-1], starts[1:])]
    if isinstance(packing, dict):
        packing = [packing[v] for v in variables]
    if ensemble:
        Ct, Dev, _ = forecast.ensemble_coefficients(tt)
    else:
        (Ct, _), Dev = forecast.coefficients(tt), None
    dev = Ub[0].device
    kern, dblock = forecast.kern, (0 if d > 1 else None)
    if slab is None:
        slab = max(1, min(T, FORECAST_STAGE_BYTES // (2 * M * (2 if spread else 1))))
    slab = int(slab)
    if slab < 1:
        raise ValueError("write_forecast_slice: slab >= 1")

    def spread_of(t0, t1):
        return fc.spread_blocks(Ub, Dev[:, t0:t1], forecast.stds, dblock, delay=d, kern=kern)

    if climatology is not None and not np.issubdtype(time.dtype, np.datetime64):
        raise ValueError("write_forecast_slice: a climatology needs datetime64 time labels")
    if trend is not None and not np.issubdtype(time.dtype, np.datetime64):
        raise ValueError("write_forecast_slice: a trend needs datetime64 time labels")
    if trend_extra is not None:
        trend_extra = np.asarray(trend_extra, dtype=np.float64).reshape(T, -1)
    offset = climatology is not None or trend is not None     # the fields pass through an fp32 slab
    fbuf = []

    def restored(t0, t1):
        """The full fields of a slab: expand, then the trend and the climatology of its times in place (the buffers
        are reused)."""
        o = [B[:t1 - t0] for B in fbuf] if fbuf else None
        F = fc.expand_blocks(Ub, Ct[t0:t1], forecast.means, forecast.stds, dblock, out=o, delay=d, kern=kern)
        if not fbuf:
            fbuf.extend(F)
        if trend is not None:
            F = trend.restore_(F, time[t0:t1], extra=None if trend_extra is None else trend_extra[t0:t1])
        return F if climatology is None else climatology.restore_(F, time[t0:t1])

    # the packings: the range pass stores coefficients and extrema only (the spread is a field: slab by slab)
    if packing is None and offset:
        state = None
        for t0 in range(0, T, slab):
            state = fc.range_field_blocks(restored(t0, min(T, t0 + slab)), groups, kern, nvar, state)
        packing = [Packing.for_range(lo, hi) for lo, hi in state[0].cpu().tolist()]
    elif packing is None:
        state = fc.range_blocks(Ub, Ct, forecast.means, forecast.stds, groups, dblock, d, kern, nvar)
        packing = [Packing.for_range(lo, hi) for lo, hi in state[0].cpu().tolist()]
    else:
        packing = fc._packings(packing, nvar, "write_forecast_slice")
    spacking = None
    if spread:
        state = None
        for t0 in range(0, T, slab):
            state = fc.range_field_blocks(spread_of(t0, min(T, t0 + slab)), groups, kern, nvar, state)
        spacking = [Packing.for_range(lo, hi) for lo, hi in state[0].cpu().tolist()]

    names = [(v, packing[g], False) for g, v in enumerate(variables)]
    if spread:
        names += [(f"{v}_spread", spacking[g], True) for g, v in enumerate(variables)]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    dims = ("time", "level", "latitude", "longitude")
    shape = (T, int(levels.size), int(lat.size), int(lon.size))
    gattrs = {"Conventions": "CF-1.6", "source_path": "dmd_era5_amd forecast", "variables": list(variables),
              "levels": [int(x) for x in levels.tolist()], "date_downloaded": datetime.now().isoformat(),
              "forecast_rank": int(Ub[0].shape[0]), "forecast_delay": d}
    with hdf5_lite.Writer(path) as w:
        if np.issubdtype(time.dtype, np.datetime64):
            w.dataset("time", np.round(io_netcdf._encode_time(time)).astype(np.int64), ("time",),
                      {"units": io_netcdf.TIME_UNITS, "calendar": "proleptic_gregorian"})
            gattrs["start_datetime"], gattrs["end_datetime"] = (str(x.astype("datetime64[s]")) for x in (time[0], time[-1]))
            if T > 1:
                gattrs["hours_delta_time"] = float((time[1] - time[0]) / np.timedelta64(1, "h"))
        else:
            w.dataset("time", time, ("time",))
        for name, vals in (("level", levels), ("latitude", lat), ("longitude", lon)):
            w.dataset(name, vals, (name,))
        for name, pk, _ in names:
            w.create(name, shape, np.int16, dims, {"scale_factor": np.float64(pk.scale_factor),
                                                   "add_offset": np.float64(pk.add_offset),
                                                   "_FillValue": np.int16(Packing.FILL_I16)})
        gattrs.update(attrs or {})
        w.attrs(None, gattrs)

        nfield = 2 if spread else 1
        dslab = torch.empty((nfield, slab, M), dtype=torch.int16, device=dev)
        stage = torch.empty((nfield, slab, M), dtype=torch.int16, pin_memory=(dev.type == "cuda"))
        counts, scounts = None, None
        for t0 in range(0, T, slab):
            t1 = min(T, t0 + slab)
            n = t1 - t0
            out = [dslab[0, :n, a:b] for a, b in zip(starts[:-1], starts[1:])]
            if offset:
                counts = fc.pack_field_blocks(restored(t0, t1), groups, packing, out, kern, nvar, counts)["counts"]
            else:
                counts = fc.pack_blocks(Ub, Ct[t0:t1], forecast.means, forecast.stds, groups, packing, dblock, d, out,
                                        kern, nvar, counts=counts)["counts"]
            if spread:
                out = [dslab[1, :n, a:b] for a, b in zip(starts[:-1], starts[1:])]
                scounts = fc.pack_field_blocks(spread_of(t0, t1), groups, spacking, out, kern, nvar, scounts)["counts"]
            stage[:, :n].copy_(dslab[:, :n])                   # the one device-to-host copy of the slab: the codes
            host = stage.numpy()
            for i, (name, _, is_spread) in enumerate(names):
                g = i % nvar
                w.write_slab(name, t0, host[int(is_spread), :n, g * plane:(g + 1) * plane].reshape((n,) + shape[1:]))
    res = {"packing": {}, "filled": {}, "saturated": {}}
    for c, sel in ((counts, False), (scounts, True)):
        if c is None:
            continue
        c = c.cpu().tolist()
        for i, (name, pk, is_spread) in enumerate(names):
            if is_spread == sel:
                res["packing"][name], res["filled"][name], res["saturated"][name] = pk, int(c[i % nvar][0]), int(c[i % nvar][1])
    return res


def project_onto_svd_results(svd_ds: Dataset, X, n_components: int | None = None, mean=None, std=None,
                             kern=None) -> DataArray:
    """The coefficients of snapshots in the basis of an SVD result, ``U[:, :r]^T ((X - mean) / std)``: the
    counterpart of :func:`reconstruct_from_svd_results` for data that were NOT part of the decomposition
    (another year on the modes of this one, new data compressed into the stored basis).  For the decomposed
    snapshots themselves it returns ``diag(s[:r]) V[:r]``.

    ``X``: a ``(space, time)`` array or DataArray on the file's space axis (for a delay embedding: the
    embedded rows), raw when ``mean`` / ``std`` are given.  ``mean`` / ``std``: per-row vectors; they default
    to the file's ``X_mean`` / ``X_std`` when it has them (only for a delay embedding d > 1 -- the
    reference's quirk, ref :400-414) and to None (no centring, no scaling) otherwise.  Returns the
    ``(components, time)`` DataArray in U's dtype, with the time coordinate of ``X`` if it has one; attrs
    ``energy_total`` = ||(X - mean) / std||_F^2 and ``captured_total`` = the part of it the r columns hold.
    fp32 results are formed by K13 on the device in row blocks, X read once; float64 ones (the small-slice
    fp64 route) take the library's fp64 product.
    A result of ``missing = "mask"`` brings its ``space_mask``: the masked rows of ``X`` (missing there too) take
    no part -- they are zeroed on the device copy, ``X`` itself is not changed -- and ``energy_total`` counts the
    used points only."""
    U = np.asarray(svd_ds["U"].values)
    k = int(U.shape[1])
    r = k if n_components is None else int(n_components)
    if not 1 <= r <= k:
        raise ValueError(f"n_components = {r} outside 1 .. {k}")
    Xv = np.asarray(X.values if hasattr(X, "values") else X)
    M = int(U.shape[0])
    if Xv.ndim != 2 or Xv.shape[0] != M:
        raise ValueError(f"X is {Xv.shape}: its space axis must have the {M} rows of U")
    names = set(svd_ds.data_vars)
    vecs = []
    for v, key in ((mean, "X_mean"), (std, "X_std")):
        if v is None and key in names:
            v = svd_ds[key]
        if v is not None:
            v = np.asarray(v.values if hasattr(v, "values") else v).reshape(-1)
            if v.shape[0] != M:
                raise ValueError(f"{key[2:]} has {v.shape[0]} entries, U has {M} rows")
        vecs.append(v)
    mu, sd = vecs
    if sd is not None and (sd == 0).any():
        raise ValueError(f"{int((sd == 0).sum())} entries of std are zero")
    T = int(Xv.shape[1])
    # a result of missing = "mask": the masked rows are missing in X too -- they count as 0, their mean / std as 0 / 1
    used = np.asarray(svd_ds["space_mask"].values) != 0 if "space_mask" in names else None
    if used is not None:
        mu = None if mu is None else np.where(used, mu, 0.0)
        sd = None if sd is None else np.where(used, sd, 1.0)
    if U.dtype == np.float64:
        Xs = Xv.astype(np.float64)
        if used is not None:
            Xs[~used] = 0.0
        if mu is not None:
            Xs = Xs - mu[:, None]
        if sd is not None:
            Xs = Xs / sd[:, None]
        C = U[:, :r].T @ Xs
        energy = float((Xs * Xs).sum())
    else:
        import torch

        from . import forecast
        from .svd import _kern, split_rows

        kern = _kern(kern)
        dev = torch.device("cuda" if getattr(kern, "name", "") == "hip" else "cpu")
        blocks = split_rows(M)

        def f32(a):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))

        def snapshots(a, b):
            x = f32(Xv[a:b].T)
            # (project_blocks zeroes the masked rows in place: on a copy of the caller's array, never on the array)
            return x.clone() if used is not None and dev.type == "cpu" else x.to(dev)

        res = forecast.project_blocks(
            (f32(U[a:b, :r].T).to(dev) for a, b in blocks), (snapshots(a, b) for a, b in blocks),
            None if mu is None else [f32(mu[a:b]) for a, b in blocks],
            None if sd is None else [f32(sd[a:b]) for a, b in blocks], kern=kern,
            masks=None if used is None else [used[a:b] for a, b in blocks])
        C = res["Ct"].T.cpu().numpy().astype(U.dtype)
        energy = res["energy_total"]
    coords = {"components": Coord("components", np.arange(r))}
    xc = getattr(X, "coords", None)
    if xc is not None and "time" in xc:
        coords["time"] = xc["time"]
    out = DataArray(np.ascontiguousarray(C), ("components", "time"), coords)
    out.attrs["energy_total"] = energy
    out.attrs["captured_total"] = float((C.astype(np.float64) ** 2).sum() / energy) if energy > 0 else float("nan")
    return out


# --------------------------------------------------------------------------------------
# main: the device pipeline
# --------------------------------------------------------------------------------------
SLAB_BYTES = 256 << 20   # host staging slab of the streaming ingest


def plan_selection(ds: Dataset, levels, delta_time):
    """Index form of ``slice_era5_dataset(ds, levels=...)`` + ``resample_era5_dataset``
    (ref era5_svd.py:385-388): which level indices and which time indices the SVD uses, and
    the resulting time coordinate -- computed from the coordinates only, so that a
    file-backed slice is never loaded whole.  Same validation / messages as slice_tools."""
    have = list(ds.coords["level"].values)
    levels = levels or have
    missing = [lv for lv in levels if lv not in have]
    if missing:
        msg = f"Requested level is not available in the dataset.Available levels: {have}"
        log_and_print(logger, msg, "error")
        raise ValueError(msg)
    level_idx = np.array([have.index(lv) for lv in levels])
    times = ds.coords["time"].values
    if len(times) < 2:
        raise ValueError("Start datetime must be before end datetime.")
    labels, take = nearest_resample_index(times, delta_time)
    return level_idx, np.asarray(levels), take, labels


def _resident_reserve_bytes(rows: int, n: int, d: int, k: int, svd_type: str, kern) -> int:
    """HBM the resident path needs NEXT TO the snapshot matrix, from the problem's own sizes (a
    fixed 12 GB used to be added: it refused small slices on small cards and under-reserved cfg3's
    rank 200): the fp64 Gram and the dense pieces of the eigen stage (standard), the partial-tile
    workspace of the batched Gram / product launch as the library itself sizes it, the m x l basis
    and the m x k result (fp32), the two pinned-slab-sized device staging buffers of the ingest,
    and 1 GiB of slack for the allocator."""
    nd = max(1, n - d + 1)
    l = min(nd, k + max(8, k // 4)) if svd_type == "standard" else min(nd, k + 20)
    out = 2 * SLAB_BYTES + (1 << 30)
    out += 4 * rows * d * (l + k)                                   # U' / Y and U
    if svd_type == "standard":
        out += 3 * 8 * n * n                                        # G, the deflated / shifted copy, K8 partials
        out += 8 * 8 * nd * 2 * l                                   # blocks of the eigen stage
    else:
        out += 4 * rows * d * l                                     # Q next to Y in the range finder
    try:
        import ctypes as C

        from .svd import split_rows

        ms = [b - a for a, b in split_rows(rows)][:16]
        arr = (C.c_int64 * len(ms))(*ms)
        if svd_type == "standard":
            out += int(kern._lib.dmdx_syrk_blocks_workspace_bytes(arr, len(ms), n))
        else:
            out += int(kern._lib.dmdx_gemm_tn_blocks_workspace_bytes(arr, len(ms), n, l))
    except Exception:
        out += 8 << 30                                              # a provider without the C ABI (tests)
    return int(out)


def lat_band(nlat: int, rank: int, world: int) -> tuple[int, int]:
    """Latitude rows [i0, i1) of rank ``rank``: the space points are sharded over the GPUs by
    latitude band (every level and variable of the band lives on the same rank), bands of
    nearly equal height."""
    if world > nlat:
        raise ValueError(f"{world} ranks for {nlat} latitude rows: use at most one rank per latitude row")
    return rank * nlat // world, (rank + 1) * nlat // world


def _take_step(take) -> int | None:
    """Step of the snapshot selection if it is an arithmetic progression (1 = contiguous), else None."""
    n = len(take)
    if n <= 1:
        return 1
    step = int(take[1]) - int(take[0])
    return step if step >= 1 and np.array_equal(take, int(take[0]) + step * np.arange(n)) else None


def _raise_on_fill_codes(found, comm, device, where: str = "the selected slice") -> None:
    """``found``: (variable name, fill codes met in the selected slice -- int or one-element device
    tensor) per variable that declares fill codes, the same list on every rank.  The reference hands
    NaN to LAPACK / sklearn, which raise; here the variable and the count are named before any SVD
    work.  The counts are summed over the ranks first, so that every rank raises (a rank that
    raised alone would leave the others waiting in their next collective)."""
    if not found:
        return
    import torch

    counts = torch.stack([c.reshape(()).to(torch.int64) if isinstance(c, torch.Tensor)
                          else torch.tensor(int(c), dtype=torch.int64, device=device) for _, c in found]).to(device)
    if comm.exchanges:
        comm.allreduce_sum_(counts, tag="fill_count_allreduce")
    totals: dict = {}
    for (name, _), c in zip(found, counts.tolist()):
        totals[name] = totals.get(name, 0) + int(c)
    bad = {k: v for k, v in totals.items() if v}
    if bad:
        what = ", ".join(f"variable {k}: {v} missing values (fill codes)" for k, v in bad.items())
        msg = (f"{what} in {where}; an SVD of data with missing values is not defined -- "
               "select levels / times without them or fill them before the decomposition"
               ' (or set missing = "mask" to leave the affected grid points out of it)')
        log_and_print(logger, msg, "error")
        raise ValueError(msg)


def _report_missing(names, counts, n: int, comm, device) -> int:
    """``missing = "mask"``: what was taken out of the decomposition.  ``counts``: per variable the int32 row
    counts of K20 (one vector per row block / piece of this rank, physical rows), the same variables on every rank;
    ``n``: the selected snapshots.  One all-reduce of [missing values, masked points, points, points that are only
    partly missing] per variable, made where ``_raise_on_fill_codes`` makes its own, so that every rank arrives; one
    log line per variable (a warning when a point with valid snapshots is dropped); if no point is left over all
    variables and ranks, every rank raises.  -> the masked points of all variables and ranks."""
    import torch

    v = torch.zeros((len(names), 4), dtype=torch.int64, device=device)
    for i, per_block in enumerate(counts):
        for c in per_block:
            on = c != 0
            v[i] += torch.stack([c.sum(dtype=torch.int64), on.sum(), torch.tensor(c.numel(), device=c.device),
                                 (on & (c < n)).sum()]).to(device)
    if comm.exchanges:
        comm.allreduce_sum_(v, tag="missing_allreduce")
    masked_all = points_all = 0
    for name, (values, masked, points, partly) in zip(names, v.tolist()):
        masked_all, points_all = masked_all + masked, points_all + points
        msg = (f"variable {name}: {values} missing values, {masked} of {points} grid points masked out of the "
               f"decomposition ({partly} of them missing in only a part of the {n} snapshots)")
        if partly:
            log_and_print(logger, "WARNING: " + msg + ": their valid snapshots are dropped with them", "warning")
        else:
            log_and_print(logger, msg)
    if masked_all == points_all:
        msg = (f"all {points_all} grid points of the selected slice have a missing value in at least one snapshot: "
               'missing = "mask" leaves nothing to decompose')
        log_and_print(logger, msg, "error")
        raise ValueError(msg)
    return int(masked_all)


def _mask_block_(kern, Xb, cnt, mu, sd) -> None:
    """The masked rows (count != 0) of a centred / scaled block become 0, their means / stds NaN."""
    from . import svd as dsvd

    dsvd.row_mask_apply_(kern, Xb, cnt, 0.0)
    for v in (mu, sd):
        if v is not None:
            v.masked_fill_(cnt != 0, float("nan"))


def _upload_packed_i16(lazy, level_idx, take, step, band, ranges, blocks, device, kern, count_fills):
    """The packed route of ``_upload_variable``: int16 codes of the file -> pinned int16 staging ->
    device slab -> one K14 launch per row block (unpack + level / band gather).
    Only the level range min(level_idx) .. max(level_idx) and the latitude band are read.  Contiguous
    snapshots are read as one span per slab; with a step the selected snapshots are read one by one
    into consecutive rows of the staging buffer (a snapshot is megabytes and contiguous in the file),
    so that what crosses the staging and PCIe is 2 bytes per selected value in either case -- a span
    with step 3 would move 6, more than the 4 of the host decode.
    -> (bytes moved, device fill-code counter or None)."""
    import torch

    packing, n = lazy.packing, len(take)
    (i0, i1), nlon = band, lazy.shape[3]
    nlat = i1 - i0
    l0, l1 = int(np.min(level_idx)), int(np.max(level_idx)) + 1
    plane = nlat * nlon
    lds = (l1 - l0) * plane
    segs = [(int(lv) - l0) * plane for lv in level_idx]
    everything = (l0, l1, i0, i1) == (0, lazy.shape[1], 0, lazy.shape[2])
    per = min(n, max(1, SLAB_BYTES // (lds * lazy.dtype.itemsize)))     # snapshots per slab
    pinned = [torch.empty((per, lds), dtype=torch.int16).pin_memory() for _ in range(2)]
    events = [None, None]
    nfill = torch.zeros(1, dtype=torch.int64, device=device) if count_fills else None
    nbytes = 0

    def read(t0, cnt, out):
        if everything:
            lazy.read_slab(t0, t0 + cnt, out)
        else:
            lazy.read_box((t0, l0, i0, 0), (cnt, l1 - l0, nlat, nlon), out)

    for it, j0 in enumerate(range(0, n, per)):
        j1 = min(n, j0 + per)
        buf = pinned[it & 1]
        if events[it & 1] is not None:
            events[it & 1].synchronize()            # the copy that last used this buffer is done
        view = buf[: j1 - j0].numpy().reshape((j1 - j0, l1 - l0, nlat, nlon))
        if step == 1:
            read(int(take[j0]), j1 - j0, view)
        else:
            for j in range(j0, j1):
                read(int(take[j]), 1, view[j - j0:j - j0 + 1])
        dev = buf[: j1 - j0].to(device, non_blocking=True)
        events[it & 1] = torch.cuda.Event()
        events[it & 1].record()
        nbytes += (j1 - j0) * lds * lazy.dtype.itemsize
        for (a, b), Xb in zip(ranges, blocks):
            kern.unpack_i16_(dev.reshape(-1), lds, 1, Xb[j0:j1, : b - a], a, plane, segs, packing.scale_factor,
                             packing.add_offset, packing.fills, nfill)
        del dev
    return nbytes, nfill


def _scatter_slab(dev, j0, j1, ranges, blocks) -> None:
    """Rows j0:j1 of every row block from a (j1 - j0, m_v) device slab."""
    for (a, b), Xb in zip(ranges, blocks):
        Xb[j0:j1, : b - a].copy_(dev[:, a:b])


def _upload_direct_f32(lazy, take, band, rows, ranges, blocks, device, count_fills):
    """The direct route of ``_upload_variable``: an fp32 file-backed variable, contiguous snapshots, every
    level.  A slab of ``rows`` snapshots is read straight into one of two pinned staging buffers and copied to
    the device asynchronously, so the next read overlaps the previous host->device copy.
    (A float32 variable that only declares a fill value -- xarray writes _FillValue = NaN on every float
    variable -- takes this route too: the fill value is replaced and the NaN counted on the device, behind the
    upload: no host pass, no host sync.)
    -> (bytes moved, device NaN counter or None)."""
    import torch

    n, (i0, i1) = len(take), band
    nlev, nlat_all, nlon = lazy.shape[1:]
    nlat = i1 - i0
    m_v = nlev * nlat * nlon
    whole = (i0, i1) == (0, nlat_all)
    on_gpu = device.type == "cuda"
    # (a NaN fill value is already what it should become)
    fills = [np.float32(f) for f in lazy.packing.fills if f == f] if count_fills and lazy.packing is not None else []
    pinned = [torch.empty((rows, m_v), dtype=torch.float32) for _ in range(2)]
    if on_gpu:
        pinned = [b.pin_memory() for b in pinned]
    events = [None, None]
    nan_count = torch.zeros((), dtype=torch.int64, device=device) if count_fills else None
    nbytes = 0
    for it, j0 in enumerate(range(0, n, rows)):
        j1 = min(n, j0 + rows)
        buf = pinned[it & 1]
        if events[it & 1] is not None:
            events[it & 1].synchronize()            # the copy that last used this buffer is done
        view = buf[: j1 - j0].numpy().reshape((j1 - j0, nlev, nlat, nlon))
        if whole:
            lazy.read_slab(int(take[j0]), int(take[j1 - 1]) + 1, view)
        else:
            lazy.read_box((int(take[j0]), 0, i0, 0), (j1 - j0, nlev, nlat, nlon), view)
        dev = buf[: j1 - j0].to(device, non_blocking=True)
        nbytes += (j1 - j0) * m_v * 4
        if count_fills:
            for f in fills:
                dev.masked_fill_(dev == f, float("nan"))
            nan_count += torch.isnan(dev).sum()
        _scatter_slab(dev, j0, j1, ranges, blocks)
        if on_gpu:
            events[it & 1] = torch.cuda.Event()
            events[it & 1].record()
        del dev
    return nbytes, nan_count


def _upload_host_decode(da, level_idx, take, band, rows, ranges, blocks, device, count_fills):
    """The host route of ``_upload_variable``: whatever the other two do not take (an in-memory variable, a
    level subset, an irregular resampling, packed values the kernel's limits exclude).  A slab of ``rows``
    snapshots is read or sliced, gathered, decoded (``labeled.Packing.decode``) and made contiguous on the
    host, then uploaded.  -> (bytes moved, device NaN counter or None)."""
    import torch

    lazy, n, (i0, i1) = da.lazy, len(take), band
    nlev_all, nlat_all, nlon = da.shape[1:]
    nlat = i1 - i0
    m_v = len(level_idx) * nlat * nlon
    whole = (i0, i1) == (0, nlat_all)
    host = None if lazy is not None else da.values
    packing = lazy.packing if lazy is not None else None
    contiguous = np.array_equal(take, np.arange(take[0], take[0] + n)) if n else True
    all_levels = len(level_idx) == nlev_all and np.array_equal(level_idx, np.arange(nlev_all))

    def read(lo, hi):
        if lazy is None:
            return host[lo:hi] if whole else host[lo:hi, :, i0:i1]
        if whole:
            return lazy.read_slab(lo, hi)
        return lazy.read_box((lo, 0, i0, 0), (hi - lo, nlev_all, nlat, nlon))

    nan_count = torch.zeros((), dtype=torch.int64, device=device) if count_fills else None
    nbytes = 0
    for j0 in range(0, n, rows):
        j1 = min(n, j0 + rows)
        if contiguous:
            slab = read(int(take[j0]), int(take[j1 - 1]) + 1)
        else:  # resampled: gather the selected snapshots
            idx = take[j0:j1]
            lo = int(idx.min())
            slab = read(lo, int(idx.max()) + 1)[idx - lo]
        if not all_levels:
            slab = slab[:, level_idx]
        if packing is not None:                 # file values -> physical ones
            slab = packing.decode(slab)
        slab = np.ascontiguousarray(slab.reshape(j1 - j0, m_v), dtype=np.float32)
        nbytes += slab.nbytes
        dev = torch.from_numpy(slab).to(device, non_blocking=False)
        if count_fills:
            nan_count += torch.isnan(dev).sum()
        _scatter_slab(dev, j0, j1, ranges, blocks)
        del dev
    return nbytes, nan_count


def _upload_variable(da: DataArray, level_idx, take, device, kern, center, scale, stats, band=None, pad4=False,
                     missing: str = "raise"):
    """One variable (time, level, lat, lon) -> centred/scaled row blocks (time, rows) in HBM.

    ``pad4``: a variable whose number of space points is not a multiple of 4 (a grid with an odd
    number of longitudes and latitudes) gets its last row block widened by 1-3 all-zero space points,
    so that every block keeps the 16-byte-aligned leading dimension the LDS-DMA / 16-byte-load bodies of
    K1 / K2 / K3 need (the register-staged bodies they otherwise fall to are 1.3-1.4x slower).  Zero
    rows change neither X^T X nor the singular values, and their rows of U are exactly zero; the
    caller drops them (returned widths are the padded ones, ``m_v`` the true count).

    Streams time slabs: file/host -> pinned staging -> device slab -> strided device copy
    into each row block, by one of three routes (``_upload_packed_i16``, ``_upload_direct_f32``,
    ``_upload_host_decode``); K5 centres / scales every block behind the last slab.
    Row order inside the variable: level slowest, longitude fastest.
    ``band`` = (i0, i1): only these latitude rows (this rank's shard); file-backed variables
    are then read as hyperslabs, so a rank touches only its own bytes of the file.

    A file-backed int16 variable with CF packing stays packed until it is in HBM: the codes of the
    span ``take[j0] .. take[j1 - 1]`` go through two pinned int16 buffers (half the bytes from the
    file, over PCIe and in the staging) and one K14 launch per row block unpacks and gathers the
    selected levels / latitude band; a regular resampling is compacted while it is read -- so
    neither ``all_levels`` nor a contiguous ``take`` is asked for.  Every other packed case is
    decoded on the host (same arithmetic) by the host route.  A variable that declares fill codes
    appends (name, number of them in the selection) to ``stats["fills"]``.

    ``missing = "mask"``: behind the last slab, whichever route ran, K20 counts the non-finite snapshots
    of every row of every block (``stats["count"]``, int32 per block), K5 runs unchanged, and the rows
    with a count become 0 in X and NaN in the means / stds; nothing goes to ``stats["fills"]``."""
    import torch

    from . import svd as dsvd

    order = [da.dims.index(x) for x in ("time", "level", "latitude", "longitude")]
    if order != [0, 1, 2, 3]:
        raise ValueError(f"variable {da.name}: expected dims (time, level, latitude, longitude), got {da.dims}")
    n = len(take)
    nlev_all, nlat_all, nlon = da.shape[1:]
    band = band if band is not None else (0, nlat_all)
    nlat = band[1] - band[0]
    m_v = len(level_idx) * nlat * nlon
    ranges = dsvd.split_rows(m_v)
    blocks = [torch.zeros((n, b - a + (-(b - a)) % 4), dtype=torch.float32, device=device) if pad4 and (b - a) % 4
              else torch.empty((n, b - a), dtype=torch.float32, device=device) for a, b in ranges]
    # the route
    lazy = da.lazy
    packing = lazy.packing if lazy is not None else None
    contiguous = np.array_equal(take, np.arange(take[0], take[0] + n)) if n else True
    all_levels = len(level_idx) == nlev_all and np.array_equal(level_idx, np.arange(nlev_all))
    direct = lazy is not None and contiguous and all_levels and lazy.dtype == np.float32 and \
        (packing is None or not packing.affine)
    step = _take_step(take)
    declared = bool(packing.fills) if packing is not None else any(
        k in getattr(da, "encoding", {}) for k in ("_FillValue", "missing_value"))
    # packed bytes travel and K14 unpacks: what the kernel's own limits allow (anything else is decoded on the host)
    unpacked = (packing is not None and lazy.dtype == np.int16 and device.type == "cuda" and hasattr(kern, "unpack_i16_")
                and step is not None and n > 0 and m_v > 0 and len(level_idx) <= 64 and len(packing.fills) <= 2
                and (int(np.max(level_idx)) - int(np.min(level_idx)) + 1) * nlat * nlon < 2 ** 31)
    rows = max(1, SLAB_BYTES // max(1, nlev_all * max(nlat, 1) * nlon * 4))     # snapshots per fp32 slab
    if unpacked:
        nbytes, found = _upload_packed_i16(lazy, level_idx, take, step, band, ranges, blocks, device, kern, declared)
    elif direct:
        nbytes, found = _upload_direct_f32(lazy, take, band, rows, ranges, blocks, device, declared)
    else:
        nbytes, found = _upload_host_decode(da, level_idx, take, band, rows, ranges, blocks, device, declared)
    mask = missing == "mask"
    if found is not None and not mask:
        stats.setdefault("fills", []).append((da.name, found))
    for (a, b), Xb in zip(ranges, blocks):
        mu = sd = None
        # (every variable is counted, whether it declares a fill value or merely holds a NaN; the pad rows are not)
        cnt = dsvd.row_missing_count(kern, Xb[:, : b - a]) if mask else None
        if center:
            # (rows are independent: a NaN spoils its own row only)
            mu, sd = kern.row_center_scale_(Xb[:, : b - a], bool(scale))   # (the zero rows stay zero: 0 / 0 otherwise)
            stats["mean"].append(mu)
            if scale:
                stats["std"].append(sd)
        if mask:
            _mask_block_(kern, Xb[:, : b - a], cnt, mu, sd)
            stats.setdefault("count", []).append(cnt)
    return blocks, m_v, nbytes


@dataclass(frozen=True, eq=False)
class _Job:
    """The shape of one ``_device_pipeline`` call: what is decomposed, how, and this rank's share of it."""
    names: list            # the variables, in the file's order
    level_idx: np.ndarray  # the selected levels as indices into the file's level axis
    levels: np.ndarray
    take: np.ndarray       # the selected snapshots as indices into the file's time axis
    time: np.ndarray       # their labels
    lats: np.ndarray
    lons: np.ndarray
    nlev: int
    nlat: int
    nlon: int
    d: int                 # delay embedding
    k: int                 # n_components
    svd_type: str
    center: bool
    scale: bool
    save_data_matrix: bool
    engine_opts: dict
    out_dtype: type        # of the returned arrays: the file's float type
    band: tuple | None     # this rank's latitude rows [i0, i1), None for a single rank
    rows_local: int        # space points of this rank (before the embedding)
    rows_global: int       # rows of the embedded matrix over all ranks
    wide: bool             # fewer rows than embedded snapshots
    can_stream: bool
    shard: str             # " (rank r of N: latitude rows i0:i1)" for the log lines, "" for a single rank
    missing: str = "raise"  # "mask": grid points with a missing value are left out of the decomposition

    @property
    def n(self) -> int:
        return len(self.take)

    @property
    def lat_rows(self) -> tuple:
        return self.band if self.band else (0, self.nlat)


def _plan_job(ds: Dataset, parsed_config: dict, comm) -> _Job:
    names = list(ds.data_vars)
    d = parsed_config["delay_embedding"]
    level_idx, levels, take, time = plan_selection(ds, parsed_config["levels"], parsed_config["delta_time"])
    log_and_print(logger, f"Dataset slicing completed successfully using levels {list(levels)}")
    log_and_print(logger, f"Resampled the dataset with time delta: {parsed_config['delta_time']}")
    lats, lons = ds.coords["latitude"].values, ds.coords["longitude"].values
    nlev, nlat, nlon = len(levels), len(lats), len(lons)
    band = lat_band(nlat, comm.rank, comm.world_size) if comm.world_size > 1 else None
    rows_global = d * len(names) * nlev * nlat * nlon
    wide = rows_global < len(take) - d + 1
    src_dtype = ds[names[0]].dtype
    return _Job(
        names=names, level_idx=level_idx, levels=levels, take=take, time=time, lats=lats, lons=lons,
        nlev=nlev, nlat=nlat, nlon=nlon, d=d, k=parsed_config["n_components"], svd_type=parsed_config["svd_type"],
        center=parsed_config["mean_center"], scale=parsed_config["scale"],
        save_data_matrix=parsed_config["save_data_matrix"], engine_opts=_engine_opts(parsed_config),
        out_dtype=src_dtype if src_dtype in (np.float32, np.float64) else np.float64,
        band=band, rows_local=len(names) * nlev * ((band[1] - band[0]) if band else nlat) * nlon,
        rows_global=rows_global, wide=wide,
        # what can be streamed from the file in passes when X does not fit: anything tall whose data
        # matrix is not asked for (un-centred standard SVD included: the exact mean deflation centres
        # the pieces as they pass; a spectrum steeper than the Gram resolves costs one more pass)
        can_stream=not wide and not parsed_config["save_data_matrix"],
        shard=f" (rank {comm.rank} of {comm.world_size}: latitude rows {band[0]}:{band[1]})" if band else "",
        missing=_missing_mode(parsed_config))


def _sync(device) -> None:
    if device.type == "cuda":
        import torch

        torch.cuda.synchronize()


# ---- residency: X in HBM, or streamed from the file in passes
def _stream_bytes_for(need: int, free: int, reserve: int, can_stream: bool, *, rows: int, n: int, rows_all: int,
                      world_size: int, others_fit: bool = True) -> int:
    """The residency decision of one rank.  ``need``: bytes of this rank's ``rows x n`` fp32 share of X plus
    ``reserve``, what the resident path allocates next to it; ``free``: free HBM; ``others_fit``: the vote of the
    ranks.  -> 0: X is resident; > 0: the bytes of X a streamed piece may take.  A slice that neither fits nor
    can be streamed is refused with the number of ranks that would hold its ``rows_all x n`` values."""
    if need <= free and others_fit:
        return 0
    if can_stream:
        return max(1 << 30, min(free // 3, 32 << 30))
    ranks = -(-4 * rows_all * n // max(free - reserve, 1 << 30))
    raise MemoryError(
        f"the snapshot matrix of this rank ({rows} x {n} fp32 = {4 * rows * n / 1e9:.1f} GB) "
        f"does not fit the {free / 1e9:.1f} GB of free HBM; shard the space points over more GPUs: "
        f"python -m torch.distributed.run --nproc-per-node N -m dmd_era5_amd.era5_svd with N >= "
        f"{max(ranks, world_size + 1)} (without save_data_matrix such a slice is streamed from the "
        "file in passes instead)")


def _all_ranks_fit(fits: bool, comm, device) -> bool:
    """One decision for all ranks: the resident and the streaming path exchange differently."""
    if not comm.exchanges:
        return fits
    import torch

    flags = comm.allgather(torch.tensor([1 if fits else 0], dtype=torch.int64, device=device))
    return all(int(f.item()) for f in flags)


def _decide_stream_bytes(job: _Job, comm, kern, device) -> int:
    """``_stream_bytes_for`` on what this device has free.  DMDX_STREAM_BYTES > 0 forces the streaming path
    (tests); off the GPU X is always resident."""
    from . import svd as dsvd

    forced = int(os.environ.get("DMDX_STREAM_BYTES", "0"))
    if forced or device.type != "cuda":
        return forced
    # X should be resident: find out before the allocator does
    reserve = _resident_reserve_bytes(job.rows_local, job.n, job.d, job.k, job.svd_type, kern)
    need = 4 * job.rows_local * job.n + reserve
    free = dsvd.free_device_bytes(device)
    return _stream_bytes_for(need, free, reserve, job.can_stream, rows=job.rows_local, n=job.n,
                             rows_all=len(job.names) * job.nlev * job.nlat * job.nlon, world_size=comm.world_size,
                             others_fit=_all_ranks_fit(need <= free, comm, device))


# ---- the streamed run
class _StreamedPieces:
    """The piece source of the streamed run.  Every call is one pass over the file: per variable and latitude
    sub-band, the centred / scaled row blocks of that piece.  The passes leave behind the row means / stds per
    (variable index, first latitude row), the fill codes met per piece, and the bytes moved (all passes)."""

    def __init__(self, ds, job: _Job, comm, kern, device, sub):
        self.ds, self.job, self.comm, self.kern, self.device, self.sub = ds, job, comm, kern, device, sub
        self.means, self.stds, self.fills, self.moved = {}, {}, {}, 0
        self.counts = {}      # missing = "mask": the K20 row counts per piece (a function of its data: every pass the same)

    def __call__(self):
        import torch

        job = self.job
        for vi, name in enumerate(job.names):
            for j0, j1 in self.sub:
                st = {"mean": [], "std": []}
                vb, _, nbytes = _upload_variable(self.ds[name], job.level_idx, job.take, self.device, self.kern,
                                                 job.center, job.scale, st, (j0, j1), missing=job.missing)
                if job.missing == "mask":
                    self.counts[(vi, j0)] = torch.cat(st["count"])
                if st.get("fills"):
                    # one rank: the piece is refused before it reaches a Gram or a product.  Several
                    # ranks: the ranks have different numbers of pieces, so there is no common point
                    # for a collective here; the counts are kept and summed once behind the SVD call,
                    # which every rank leaves at the same place (its finite checks are made on
                    # all-reduced quantities)
                    if not self.comm.exchanges:
                        _raise_on_fill_codes(st["fills"], self.comm, self.device,
                                             f"latitude rows {j0}:{j1} of the selected slice (the first piece with any)")
                    self.fills[(vi, j0)] = st["fills"][0]
                if job.center:
                    self.means[(vi, j0)] = torch.cat(st["mean"])
                if job.scale:
                    self.stds[(vi, j0)] = torch.cat(st["std"])
                self.moved += nbytes
                yield vb


def _svd_streamed(ds: Dataset, job: _Job, comm, kern, device, stream_bytes: int):
    """X does not fit: the Gram is accumulated and the projection made while latitude sub-bands of the
    variables pass through the HBM, two or three times (svd.svd_snapshots_streaming).
    -> (SvdResult with the rows in this rank's (k, d, variable, level, band, lon) order, stats);
    ``stats["moved"]``: file bytes moved over all passes."""
    import torch

    from . import svd as dsvd

    if not job.can_stream:
        raise ValueError("the streaming path needs save_data_matrix = False and a tall problem")
    names, nlev, nlon, d = job.names, job.nlev, job.nlon, job.d
    i0, i1 = job.lat_rows
    h = max(1, stream_bytes // max(1, 4 * job.n * nlev * nlon))       # latitude rows per piece
    sub = [(j, min(i1, j + h)) for j in range(i0, i1, h)]
    pieces = _StreamedPieces(ds, job, comm, kern, device, sub)
    log_and_print(logger, f"Snapshot matrix larger than the HBM: streaming it in {len(names) * len(sub)} pieces of "
                          f"<= {h} latitude rows{job.shard}")
    log_and_print(logger, f"Performing {job.svd_type} SVD...")
    failed = None
    try:
        if job.svd_type == "standard":
            Ub, s_, Vh_, sinfo = dsvd.svd_snapshots_streaming(pieces, job.k, job.rows_global, delay=d, comm=comm, kern=kern)
        else:
            Ub, s_, Vh_, sinfo = dsvd.svd_randomized_streaming(pieces, job.k, job.rows_global, job.n, delay=d, comm=comm,
                                                               kern=kern, **job.engine_opts)
    except np.linalg.LinAlgError as e:          # (raised on all-reduced quantities: by every rank or by none)
        failed = e
    except Exception as e:                      # missing = "mask" with nothing left: the report below says so
        if job.missing != "mask":
            raise
        failed = e
    declared = [nm for nm in names if any(key in getattr(ds[nm], "encoding", {}) for key in ("_FillValue", "missing_value"))]
    masked_points = None
    if job.missing == "mask":
        # (the same place as the summed fill-code check below: every rank arrives here)
        masked_points = _report_missing(names, [[pieces.counts[(vi, j0)] for j0, _ in sub if (vi, j0) in pieces.counts]
                                                for vi in range(len(names))], job.n, comm, device)
    elif comm.exchanges and declared:
        # several ranks: ONE summed check here, where every rank arrives whether the SVD raised or returned
        local = {}
        for (vi, _), (nm, c) in sorted(pieces.fills.items()):
            local[nm] = local.get(nm, 0) + int(c)
        _raise_on_fill_codes([(nm, local.get(nm, 0)) for nm in declared], comm, device)
    if failed is not None:
        raise failed
    if sinfo.get("warning"):
        log_and_print(logger, "WARNING: " + sinfo["warning"])
    kk = int(s_.numel())
    Ul = torch.empty((kk, d, len(names), nlev, i1 - i0, nlon), dtype=torch.float32, device=device)
    mean_l = torch.empty((len(names), nlev, i1 - i0, nlon), dtype=torch.float32, device=device)
    std_l = torch.empty_like(mean_l) if job.scale else None
    count_l = torch.zeros(mean_l.shape, dtype=torch.int32, device=device) if job.missing == "mask" else None
    idx = 0
    for vi in range(len(names)):
        for j0, j1 in sub:      # a piece's rows: (level, its latitude rows, longitude), embedded as k_delay * m_piece + s
            Ul[:, :, vi, :, j0 - i0:j1 - i0, :] = dsvd._assemble_rows(Ub[idx], d).reshape(kk, d, nlev, j1 - j0, nlon)
            if job.center:
                mean_l[vi, :, j0 - i0:j1 - i0, :] = pieces.means[(vi, j0)].reshape(nlev, j1 - j0, nlon)
            if job.scale:
                std_l[vi, :, j0 - i0:j1 - i0, :] = pieces.stds[(vi, j0)].reshape(nlev, j1 - j0, nlon)
            if count_l is not None:
                count_l[vi, :, j0 - i0:j1 - i0, :] = pieces.counts[(vi, j0)].reshape(nlev, j1 - j0, nlon)
            Ub[idx] = None
            idx += 1
    res = dsvd.SvdResult(Ut=Ul.reshape(kk, -1), s=s_, Vh=Vh_, info=sinfo)
    stats = {"mean": [mean_l.reshape(-1)], "std": [std_l.reshape(-1)] if job.scale else [], "moved": pieces.moved}
    if count_l is not None:
        stats["count"], stats["masked_points"] = [count_l.reshape(-1)], masked_points
        res = _mask_u_rows(res, stats["count"], d, kern)
    return res, stats


# ---- the resident run
def _ingest_resident(ds: Dataset, job: _Job, comm, kern, device):
    """Every variable of this rank's band -> centred / scaled row blocks in HBM.
    -> (blocks, true_rows, stats, bytes moved); ``true_rows``: the width of every block without the zero rows
    ``pad4`` appended.  Missing values raise here, before any SVD work -- or, with ``missing = "mask"``, are
    reported here (``stats["count"]`` per block, ``stats["masked_points"]`` over all ranks)."""
    from . import svd as dsvd

    # `python -m dmd_era5.era5_svd.era5_svd` is one process per slice: every run is a "first
    # call".  While the slice crosses PCIe (the GPU and most host threads are idle) a side
    # thread takes the SVD path once on a toy matrix, so that the dense libraries' handles and
    # the code objects of every kernel are loaded when the real matrix is resident.  Only for
    # slices of >= 1 GiB: the reference's default config (0.4 GB, scripts/bench_default_config.py)
    # ingests in 0.1-0.4 s, less than the toy run takes -- 2.62 s primed against 1.99 s.
    # (DMDX_PRIME_MIN_BYTES: tests force the primer onto small slices)
    prime_min = int(os.environ.get("DMDX_PRIME_MIN_BYTES", str(1 << 30)))
    primer = _prime_async(device, job.svd_type) if device.type == "cuda" and \
        4 * job.rows_local * job.n >= prime_min else None
    blocks, true_rows, stats, total = [], [], {"mean": [], "std": []}, 0
    per_variable = []
    for name in job.names:
        # (a tall problem on a grid whose space-point count is not a multiple of 4: 1-3 zero rows per variable)
        seen = len(stats.get("count", []))
        vb, m_v, nbytes = _upload_variable(ds[name], job.level_idx, job.take, device, kern, job.center, job.scale,
                                           stats, job.band, pad4=not job.wide, missing=job.missing)
        blocks.extend(vb)
        true_rows.extend(b - a for a, b in dsvd.split_rows(m_v))
        per_variable.append(stats.get("count", [])[seen:])
        total += nbytes
    if primer is not None:
        primer.join()
    _sync(device)
    if job.missing == "mask":
        stats["masked_points"] = _report_missing(job.names, per_variable, job.n, comm, device)
    else:
        _raise_on_fill_codes(stats.get("fills"), comm, device)
    return blocks, true_rows, stats, total


def _svd_transposed(blocks, job: _Job, comm, kern):
    """WIDE problem (fewer space rows than snapshots: a coarse mock grid over a long period).
    sklearn transposes wide inputs (extmath.py:562-566) and LAPACK does not care; here the
    tall algorithms run on E^T -- the embedded matrix is small by definition (< n^2 floats),
    so it is materialised -- and the factors swap roles."""
    import torch

    from . import svd as dsvd

    d, nd = job.d, job.n - job.d + 1
    if comm.world_size > 1:
        raise ValueError(f"{job.rows_global} space rows < {nd} snapshots: a wide problem is small, "
                         "run it as a single process (no torch.distributed)")
    Xall = torch.cat(blocks, dim=1)                                            # (n, M)
    E = torch.cat([Xall[kd:kd + nd].T for kd in range(d)], dim=0).contiguous()  # (d M, nd): row kd*M + s
    del Xall
    log_and_print(logger, f"Performing {job.svd_type} SVD...")
    if job.svd_type == "standard":
        rt = dsvd.svd_snapshots(E, job.k, flip_sign=False, kern=kern)
    else:
        rt = dsvd.svd_randomized(E, job.k, flip_sign=False, kern=kern, **job.engine_opts)
    Ut = rt.Vh.to(torch.float32)                   # (k, d M): left singular vectors of E
    Vh = rt.Ut.to(torch.float64)                   # (k, nd)
    big = Ut.abs().argmax(dim=1, keepdim=True)     # u-based sign convention (svd_flip)
    sign = torch.where(Ut.gather(1, big) < 0, -1.0, 1.0)
    res = dsvd.SvdResult(Ut=Ut * sign, s=rt.s, Vh=Vh * sign.to(torch.float64), info=dict(rt.info, wide=True))
    log_and_print(logger, f"{job.svd_type.capitalize()} SVD complete.")
    return res


def _drop_pad_rows(res, blocks, true_rows, d: int):
    """Drop the zero rows the ingest appended (their rows of U are exactly zero)
    -> (SvdResult on the true rows, the blocks as their narrow views)."""
    import torch

    from . import svd as dsvd

    Mp = sum(int(b.shape[1]) for b in blocks)
    keep, off = [], 0
    for b, r in zip(blocks, true_rows):
        keep.append(torch.arange(off, off + r, device=b.device))
        off += int(b.shape[1])
    kk = res.Ut.shape[0]
    Ut = res.Ut.reshape(kk, d, Mp).index_select(2, torch.cat(keep)).reshape(kk, -1)
    return dsvd.SvdResult(Ut=Ut, s=res.s, Vh=res.Vh, info=res.info), [b[:, :r] for b, r in zip(blocks, true_rows)]


def _mask_u_rows(res, counts, d: int, kern):
    """``missing = "mask"``: the rows of U of the masked grid points, in every delay block, are set to 0 (K20 on
    the (k, rows) blocks of U^T).  Zero rows of X give exactly zero rows of U already; this also covers the
    orthonormal completion of a rank-deficient slice, which writes into every column.  ``counts``: the int32 row
    counts of this rank's physical rows, in row order."""
    import torch

    from . import svd as dsvd

    cnt = torch.cat(list(counts))
    kk = res.Ut.shape[0]
    Ut = res.Ut.contiguous()
    per_delay = Ut.view(kk, d, -1)
    for kd in range(d):
        dsvd.row_mask_apply_(kern, per_delay[:, kd], cnt, 0.0)
    return dsvd.SvdResult(Ut=Ut, s=res.s, Vh=res.Vh, info=res.info)


def _svd_resident(blocks, true_rows, job: _Job, comm, kern, counts=None):
    """-> (SvdResult on this rank's true rows, the row blocks without their pad rows).  ``counts``: the row counts
    of ``missing = "mask"`` (``_mask_u_rows``)."""
    from . import svd as dsvd

    if job.wide:
        res = _svd_transposed(blocks, job, comm, kern)
    elif job.svd_type == "standard":
        log_and_print(logger, "Performing standard SVD...")
        res = dsvd.svd_snapshots(blocks, job.k, delay=job.d, comm=comm, kern=kern)
        if res.info.get("mean_deflated"):
            log_and_print(logger, "Un-centred data: SVD of the centred matrix + rank-one update for the time mean.")
        if res.info.get("warning"):
            log_and_print(logger, "WARNING: " + res.info["warning"])
        log_and_print(logger, "Standard SVD complete.")
    else:
        log_and_print(logger, "Performing randomized SVD...")
        res = dsvd.svd_randomized(blocks, job.k, delay=job.d, comm=comm, kern=kern, **job.engine_opts)
        log_and_print(logger, "Randomized SVD complete.")
    if any(int(b.shape[1]) != r for b, r in zip(blocks, true_rows)):
        res, blocks = _drop_pad_rows(res, blocks, true_rows, job.d)
    if counts is not None:
        res = _mask_u_rows(res, counts, job.d, kern)
    return res, blocks


# ---- the gather to rank 0's host memory
def _assemble(t, lead: tuple, job: _Job, comm) -> np.ndarray | None:
    """Rank-local (*lead, rows of this rank in (variable, level, band, lon) order) pieces ->
    the global (*lead, variable, level, latitude, longitude) host array on rank 0."""
    parts = comm.gather_to_root(t)
    if parts is None:
        return None
    grid = (len(job.names), job.nlev, job.nlat, job.nlon)
    if len(parts) == 1:
        return parts[0].numpy().reshape(lead + grid)
    out = np.empty(lead + grid, dtype=parts[0].numpy().dtype)
    for r, part in enumerate(parts):
        j0, j1 = lat_band(job.nlat, r, comm.world_size)
        out[..., j0:j1, :] = part.numpy().reshape(lead + grid[:2] + (j1 - j0, job.nlon))
    return out


def _row_vector(parts, job: _Job, comm, coords) -> DataArray | None:
    """Per-row values of the ingest (means, stds) -> the (space,) DataArray of the embedded rows on rank 0."""
    import torch

    v = _assemble(torch.cat(parts), (), job, comm)
    if v is None:
        return None
    return DataArray(np.tile(v.reshape(-1).astype(job.out_dtype), job.d), ("space",),
                     {k: coords[k] for k in ("space", "original_variable")})


def _data_matrix(blocks, job: _Job, comm, device, coords) -> DataArray | None:
    """The embedded data matrix ``save_data_matrix`` asks for, (space, time) on rank 0."""
    import torch

    from . import svd as dsvd
    from .slice_tools import _apply_delay_embedding_np

    d, n = job.d, blocks[0].shape[0]
    nt, M = n - d + 1, sum(int(b.shape[1]) for b in blocks)
    if not comm.exchanges and device.type == "cuda" and nt > 0 and \
            4 * d * M * nt + (1 << 30) <= dsvd.free_device_bytes(device):
        # one rank and room for it: the embedded matrix is laid out on the device as the file
        # wants it -- (space = k_delay * M + s, time) row-major, E[k M + s, t] = X[t + k, s] -- and
        # leaves in one copy.  (The host route below gathers the time-major blocks, embeds them
        # column-major as the reference does and lets the writer transpose 0.8 GB: 0.27 s of the
        # 0.73 s a warm main() takes on the reference's default config; this takes 0.06 s.)
        Xe = torch.empty((d, M, nt), dtype=torch.float32, device=device)
        off = 0
        for b in blocks:
            mb = int(b.shape[1])
            for kd in range(d):
                Xe[kd, off:off + mb].copy_(b[kd:kd + nt].T)
            off += mb
        return DataArray(Xe.reshape(d * M, nt).cpu().numpy().astype(job.out_dtype, copy=False), ("space", "time"), coords)
    # several ranks, or no room: concatenate on the host (a device-side cat would hold X twice in HBM)
    Xall = torch.cat(blocks, dim=1) if comm.exchanges else torch.cat([b.cpu() for b in blocks], dim=1)
    Xg = _assemble(Xall, (n,), job, comm)                # (time, variable, level, lat, lon) on rank 0
    del Xall
    if Xg is None:
        return None
    Xc = Xg.reshape(n, -1).T.astype(job.out_dtype, copy=False)
    return DataArray(_apply_delay_embedding_np(np.asfortranarray(Xc), d), ("space", "time"), coords)


def _space_mask(used, d: int, coords) -> DataArray:
    """``used``: bool over the physical grid points in row order -> ``space_mask``: int8 over the embedded
    ``space`` axis, 1 = the point took part in the decomposition."""
    return DataArray(np.tile(np.asarray(used).astype(np.int8), d), ("space",),
                     {k: coords[k] for k in ("space", "original_variable") if k in coords})


def _gather_results(res, stats, blocks, job: _Job, comm, device, extras: dict | None = None):
    """The row-sharded results -> what ``_device_pipeline`` returns: U, then the row means and stds, then X
    are gathered to rank 0 in the global row order; the other ranks get None for them and for the coords.
    ``missing = "mask"``: ``extras`` receives ``space_mask`` (rank 0; None elsewhere) and ``masked_points``."""
    kk = res.Ut.shape[0]
    Ug = _assemble(res.Ut, (kk, job.d), job, comm)       # local row order k_delay*m_loc + s_loc
    U = None if Ug is None else Ug.reshape(kk, -1).T.astype(job.out_dtype, copy=False)
    s = res.s.cpu().numpy().astype(job.out_dtype, copy=False)
    V = res.Vh.cpu().numpy().astype(job.out_dtype, copy=False)
    coords = X = X_mean = X_std = None
    if comm.rank == 0:
        one = space_labels(job.levels, job.lats, job.lons)
        coords = delay_coords(np.tile(one, (len(job.names), 1)), np.repeat(job.names, one.shape[0]), job.time, job.d)
    if job.center and job.d > 1:  # the reference keeps the mean / std only in this case (ref :400-414)
        X_mean = _row_vector(stats["mean"], job, comm, coords)
        if job.scale:
            X_std = _row_vector(stats["std"], job, comm, coords)
    if job.save_data_matrix:
        X = _data_matrix(blocks, job, comm, device, coords)
    if job.missing == "mask" and extras is not None:
        import torch

        cnt = _assemble(torch.cat(stats["count"]), (), job, comm)       # one more small gather, made by every rank
        extras["masked_points"] = stats["masked_points"]
        extras["space_mask"] = None if cnt is None else _space_mask(cnt.reshape(-1) == 0, job.d, coords)
    return U, s, V, coords, X, X_mean, X_std


def _device_pipeline(ds: Dataset, parsed_config: dict, comm=None, kern=None, device=None, extras: dict | None = None):
    """Slice -> (U, s, V, coords, X, X_mean, X_std) with X resident only in HBM.

    Row order = the reference's flatten order (variable-major, then level, latitude,
    longitude; ref slice_tools.py:311-336); embedding order k*m + s (ref :207-211).

    ``comm`` (svd.TorchDistComm, one process per GPU): the space points are sharded by latitude
    band (``lat_band``); each rank reads, centres and decomposes only its rows, the exchanges
    are the small all-reduces inside the SVD, and the row-sharded results (U, the row means,
    X if asked for) are gathered to rank 0's HOST memory in the global row order for the
    NetCDF write.  Ranks other than 0 return U = X = X_mean = X_std = None.

    ``kern`` / ``device``: the kernel provider and where the row blocks live -- the HIP kernels
    on the current GPU unless a test injects its CPU double (main() never does: without
    libdmdx.so or a GPU ``default_kernels()`` raises).

    ``extras``: a dict that receives what ``missing = "mask"`` adds to the result -- ``space_mask`` (the int8
    DataArray over ``space`` on rank 0, None elsewhere) and ``masked_points`` (over all ranks).  Masked points are
    zero rows of X and of U, NaN in X_mean / X_std; the masking happens in the ingest (``_upload_variable``).

    The stages: ``_plan_job`` (the shape of the job), ``_decide_stream_bytes`` (X resident or streamed),
    ``_svd_streamed`` or ``_ingest_resident`` + ``_svd_resident``, ``_gather_results``."""
    import time as _time

    import torch

    from . import svd as dsvd
    from .kernels import default_kernels

    comm = comm or dsvd.Comm()
    if kern is None:
        kern = default_kernels()
        device = torch.device("cuda", torch.cuda.current_device())
    job = _plan_job(ds, parsed_config, comm)
    stream_bytes = _decide_stream_bytes(job, comm, kern, device)
    t0 = _time.perf_counter()
    if stream_bytes:
        blocks = []
        res, stats = _svd_streamed(ds, job, comm, kern, device, stream_bytes)
        npass = int(res.info.get("passes_over_X", 2))
        total = stats["moved"] // npass
        _sync(device)
        dt = _time.perf_counter() - t0
        log_and_print(logger, f"{job.svd_type.capitalize()} SVD complete.")
        log_and_print(logger, f"Ingest + SVD ({npass} passes over the file): {dt:.2f} s "
                              f"({npass * total / 1e9 / max(dt, 1e-9):.1f} GB/s of file data)")
    else:
        blocks, true_rows, stats, total = _ingest_resident(ds, job, comm, kern, device)
        dt = _time.perf_counter() - t0
        log_and_print(logger, f"Ingest: {total / 1e9:.3f} GB to HBM in {dt:.2f} s ({total / 1e9 / max(dt, 1e-9):.2f} GB/s, "
                              f"{len(blocks)} row blocks, centre/scale on device){job.shard}")
        t0 = _time.perf_counter()
        res, blocks = _svd_resident(blocks, true_rows, job, comm, kern, stats.get("count"))
        _sync(device)
        dt = _time.perf_counter() - t0
        log_and_print(logger, f"SVD stage: {dt:.3f} s ({total / 1e9 / max(dt, 1e-9):.1f} GB/s of X)")
    return _gather_results(res, stats, blocks, job, comm, device, extras)


_PRIMED: set = set()


def _prime_async(device, svd_type: str):
    """Start (once per process, device and svd_type) a thread that runs the SVD path on a toy
    matrix with a kernel provider of its own: first-use costs of rocBLAS / rocSOLVER / libdmdx
    (0.3-0.8 s at cfg2 scale) overlap the ingest instead of following it.  Returns the thread, or
    None when there is nothing left to prime or DMDX_NO_PRIME=1."""
    import os
    import threading

    import torch

    key = (str(device), svd_type)
    if key in _PRIMED or os.environ.get("DMDX_NO_PRIME") == "1":
        return None
    _PRIMED.add(key)

    def work():
        try:
            from . import svd as dsvd
            from .kernels import HipKernels

            torch.cuda.set_device(device)
            k2 = HipKernels()
            # a stream of its own: the toy run (it includes the grid-barrier kernels K7L / K10) must not
            # queue in front of, or between, the ingest's copies and K5 launches on the default stream;
            # its workspaces (a few MB) belong to this provider and stream and are released below
            side = torch.cuda.Stream(device=device)
            with torch.cuda.stream(side):
                g = torch.Generator(device=device)
                g.manual_seed(0)
                toy = torch.randn((1024, 8192), device=device, dtype=torch.float32, generator=g)
                halves = [toy[:, :4096].contiguous(), toy[:, 4096:].contiguous()]
                if svd_type == "standard":
                    dsvd.svd_snapshots(halves, 12, delay=2, kern=k2)
                else:
                    dsvd.svd_randomized(halves, 12, delay=2, random_state=0, kern=k2)
                side.synchronize()
            k2.release_workspace()
        except Exception as e:      # priming is an optimisation: never fail the run for it
            logger.debug(f"library priming failed: {e}")

    t = threading.Thread(target=work, name="dmdx-prime", daemon=True)
    t.start()
    return t


def _small_float64_slice(ds: Dataset, parsed_config: dict) -> bool:
    """float64 variables whose embedded snapshot matrix is small enough for the fp64 engine path
    (the reference's mock slices: a few MB).  Real ERA5 slices are float32 and go to the device
    pipeline."""
    from .engine import FP64_MAX_BYTES

    names = list(ds.data_vars)
    if not names or any(np.dtype(ds[v].dtype) != np.float64 for v in names):
        return False
    cells = sum(int(np.prod(ds[v].shape)) for v in names)
    return 8 * cells * int(parsed_config["delay_embedding"]) <= FP64_MAX_BYTES


def _host_pipeline_fp64(ds: Dataset, parsed_config: dict, extras: dict | None = None):
    """The reference's own sequence (ref era5_svd.py:384-415) on the mirrored slice tools, for
    small float64 slices: slice -> resample -> standardize -> flatten -> delay-embed on the host
    in float64 (a few MB: not a device job), then ``svd_on_era5``, whose float64 input takes the
    engine's fp64 path (K9 Gram, fp64 eigen stage) -- so that the reference's float64 mock data
    come back with float64 accuracy (1e-12 against numpy), not fp32's 1e-6.  Returns what
    ``_device_pipeline`` returns."""
    from .slice_tools import (apply_delay_embedding, flatten_era5_variables, resample_era5_dataset,
                              slice_era5_dataset, standardize_data)

    d = parsed_config["delay_embedding"]
    ds = slice_era5_dataset(ds, levels=parsed_config["levels"])
    ds = resample_era5_dataset(ds, parsed_config["delta_time"])
    bad = None
    if _missing_mode(parsed_config) == "mask":
        # the rule of the device pipeline, in numpy: a grid point with a snapshot that is not finite is left out
        import torch

        from . import svd as dsvd

        names = list(ds.data_vars)
        cnt = np.logical_not(np.isfinite(flatten_era5_variables(ds).values)).sum(axis=1).astype(np.int32)
        per = torch.from_numpy(cnt).reshape(len(names), -1)
        masked = _report_missing(names, [[c] for c in per], int(ds.coords["time"].values.shape[0]), dsvd.Comm(),
                                 torch.device("cpu"))
        bad = cnt != 0
    ds_mean = ds_std = None
    if parsed_config["mean_center"] and parsed_config["scale"]:
        ds, ds_mean, ds_std = standardize_data(ds)
    elif parsed_config["mean_center"]:
        ds, ds_mean, ds_std = standardize_data(ds, scale=False)
    flat = flatten_era5_variables(ds)                                  # (a new array: the caller's values stay)
    if bad is not None:
        flat.values[bad] = 0.0
    da = apply_delay_embedding(flat, d)
    row = {c: da.coords[c] for c in ("space", "original_variable", "delay") if c in da.coords}

    def row_vector(stat: Dataset) -> DataArray:
        v = flatten_era5_variables(stat).values
        if bad is not None:
            v[bad] = np.nan
        return DataArray(np.tile(v, d), ("space",), row)

    da_mean = da_std = None
    if ds_mean is not None and d > 1:                                  # (the reference's d == 1 quirk: no X_mean)
        da_mean = row_vector(ds_mean)
        if ds_std is not None:
            da_std = row_vector(ds_std)
    U, s, V = svd_on_era5(da, parsed_config)
    if bad is not None:
        U[np.tile(bad, d)] = 0.0                                       # (already zero, up to an orthonormal completion)
        if extras is not None:
            extras["masked_points"], extras["space_mask"] = masked, _space_mask(~bad, d, da.coords)
    return U, s, V, da.coords, (da if parsed_config["save_data_matrix"] else None), da_mean, da_std


def _dist_comm():
    """The communicator of this process: single-rank unless it runs under
    ``python -m torch.distributed.run --nproc-per-node N -m dmd_era5_amd.era5_svd`` (one process
    per GPU, RCCL) or inside an already initialised ``torch.distributed`` job.  Returns
    (comm, created) -- ``created``: the process group was made here and is torn down by main.
    DMDX_DIST_BACKEND=gloo / DMDX_DEVICE=i: rehearsal knobs (several ranks on one GPU);
    DMDX_COMM_FORCE=1: a one-rank process group whose collectives are all issued (RCCL itself on
    a one-GPU box)."""
    import os

    import torch
    import torch.distributed as dist

    from . import svd as dsvd

    force = os.environ.get("DMDX_COMM_FORCE") == "1"
    if dist.is_available() and dist.is_initialized():
        return (dsvd.TorchDistComm() if dist.get_world_size() > 1 or force else dsvd.Comm()), False
    if int(os.environ.get("WORLD_SIZE", "1")) <= 1 and not force:
        return dsvd.Comm(), False
    if force:
        for key, val in (("RANK", "0"), ("WORLD_SIZE", "1"), ("MASTER_PORT", "29533")):
            os.environ.setdefault(key, val)
    dev = int(os.environ.get("DMDX_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(dev)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    backend = os.environ.get("DMDX_DIST_BACKEND", "nccl")
    if backend == "nccl":
        dist.init_process_group("nccl", device_id=torch.device("cuda", dev))
    else:
        dist.init_process_group(backend)
    return dsvd.TorchDistComm(), True


def main(config: dict | None = None, write_to_netcdf: bool = False, use_dvc: bool = False):
    """SVD of an ERA5 slice (ref :336-453).  Returns (results Dataset, added_to_dvc,
    retrieved_from_dvc) -- the two flags are always False here (no DVC).

    Under torch.distributed (one process per GPU) the space points are sharded over the ranks
    (``_device_pipeline``); rank 0 assembles, returns and writes the results, the other ranks
    return ``(None, False, False)`` -- unless the results were already on disk, which every
    rank finds for itself."""
    import time

    _no_dvc(use_dvc)
    t_start = time.perf_counter()
    if config is None:
        config = config_reader("era5-svd")
    parsed_config = config_parser(config, "era5-svd")
    for key in (*_ENGINE_KEYS, "missing"):
        if key in config:
            parsed_config[key] = config[key]
    masking = _missing_mode(parsed_config) == "mask"

    try:
        svd_results, _ = retrieve_svd_results(parsed_config, use_dvc)
    except Exception as e:
        msg = f"Error retrieving SVD results: {e}"
        log_and_print(logger, msg, "error")
        raise Exception(msg) from e
    if svd_results is not None:
        return svd_results, False, False

    try:
        ds, _ = retrieve_era5_slice(parsed_config, use_dvc)
        if ds is None:
            msg = ("\n                    Could not retrieve ERA5 slice from working directory.\n"
                   "                    Consider using DVC to retrieve the ERA5 slice, if available.\n"
                   "                    ")
            log_and_print(logger, msg, "error")
            raise FileNotFoundError(msg)
    except Exception as e:
        msg = f"Error retrieving ERA5 slice: {e}"
        log_and_print(logger, msg, "error")
        raise Exception(msg) from e

    t_open = time.perf_counter()
    comm, created = _dist_comm()
    try:
        ds = ds[parsed_config["variables"]]
        # slice_era5_dataset(levels=...) and resample_era5_dataset(...) happen inside, as index
        # selections applied while the slice is streamed to the device
        extras = {}
        more = {"extras": extras} if masking else {}      # (the default call is what it was)
        if comm.world_size == 1 and _small_float64_slice(ds, parsed_config):
            U, s, V, coords, X, X_mean, X_std = _host_pipeline_fp64(ds, parsed_config, **more)
        else:
            U, s, V, coords, X, X_mean, X_std = _device_pipeline(ds, parsed_config, comm, **more)
        svd_results = None
        t_pipe = time.perf_counter()
        if comm.rank == 0:
            svd_results = combine_svd_results(U, s, V, coords, X=X, X_mean=X_mean, X_std=X_std, **extras)
            svd_results = add_config_attributes(svd_results, parsed_config)
            svd_results = space_coord_to_level_lat_lon(svd_results)
    except Exception as e:
        msg = f"Error in the SVD on ERA5 process: {e}"
        log_and_print(logger, msg, "error")
        raise Exception(msg) from e
    finally:
        from .kernels import release_cached_workspaces

        release_cached_workspaces()
        if created:
            import torch.distributed as dist

            dist.destroy_process_group()

    t_done = time.perf_counter()
    if comm.rank == 0:
        log_and_print(logger, f"main(): slice found and opened in {t_open - t_start:.2f} s, ingest + SVD + gather "
                              f"{t_pipe - t_open:.2f} s, result Dataset {t_done - t_pipe:.2f} s")
    if write_to_netcdf and svd_results is not None:
        try:
            log_and_print(logger, "Writing SVD results to NetCDF...")
            io_netcdf.to_netcdf(svd_results, parsed_config["save_path"])
            log_and_print(logger, f"SVD results written to {parsed_config['save_path']} "
                                  f"({time.perf_counter() - t_done:.2f} s)")
        except Exception as e:
            msg = f"Error writing SVD results to NetCDF: {e}"
            log_and_print(logger, msg, "error")
            raise Exception(msg) from e
    return svd_results, False, False


if __name__ == "__main__":
    log_and_print(logger, "Not a Data Version Control (DVC) repository. Will not use DVC.", level="warning")
    main(write_to_netcdf=True)
