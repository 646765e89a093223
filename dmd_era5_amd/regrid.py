"""Area-weighted coarsening of the snapshots on the device (K23, csrc/coarsen.hip).

ERA5 arrives at 0.25 degrees; a DMD of the climate is usually fitted at 1 degree or coarser, and the cost of everything
here scales with the number of grid points.  Taking every n-th grid point aliases in space exactly as ``tstep`` aliases in
time; the area-weighted mean over ``fy x fx`` cells of the latitude / longitude grid does not.  This module forms the
weights of the latitude rows on the host in fp64 (:func:`lat_weights`: pure numpy) and applies ``HipKernels.coarsen`` to
the resident ``(time, rows)`` blocks: one read of X, one write of X / (fy fx), no fp64 copy.

    cz = Coarsen(latitude, longitude, 4, 4)                      # 721 x 1440 -> 180 x 360, one pole row dropped
    Yblocks = cz.apply(Xblocks, planes)                          # (T, planes_b * 180 * 360) fp32 per block
    w_rows = cz.row_weights_out(planes_b)                        # what verify_blocks / crps_blocks take on that grid

Coarsening is the first step of the chain after the ingest: ingest, *coarsen*, filter / decimate, climatology, trend,
SVD.  Its output is again a list of ``(T, rows)`` fp32 blocks in the project's flatten order (plane, latitude,
longitude) that ``TimeFilter.apply``, ``Climatology.fit``, ``Trend.fit`` and the SVD take as they are, and the coarse
``latitude_out`` / ``longitude_out`` are what ``write_forecast_slice`` and ``area_weights`` are then called with.
Coarsening commutes with the time filter in exact arithmetic (both are linear, on different axes) and is the cheaper one
to run first: the filter then reads 1 / (fy fx) of the data.  Rows are independent: row shards (latitude bands whose
boundaries fall on cell boundaries, :func:`coarse_lat_band`) coarsen their own blocks, no collective is involved.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _timeaxis as ta
from . import io_netcdf
from .labeled import Coord, DataArray, Dataset
from .svd import _kern

__all__ = ["KINDS", "lat_weights", "coarse_lat_band", "Coarsen"]

KINDS = ("cos", "band", "none")
MAX_FACTOR = 64                                                 # dmdx_coarsen_max_factor()


def _latitudes(latitude_deg, who: str) -> np.ndarray:
    lat = np.ascontiguousarray(np.asarray(latitude_deg, dtype=np.float64))
    if lat.ndim != 1 or not np.isfinite(lat).all() or (np.abs(lat) > 90.0).any():
        raise ValueError(f"{who}: latitude must be a one-dimensional array of finite degrees in [-90, 90], got {lat.shape}")
    return lat


def lat_weights(latitude_deg, kind: str = "cos") -> np.ndarray:
    """The fp64 weight of every latitude row.  ``"cos"``: ``cos(latitude)``, clipped at 0 (a pole a rounding past 90
    degrees).  ``"band"``: ``sin`` of the upper edge minus ``sin`` of the lower edge of the row, the edges being the
    midpoints between neighbouring rows, clipped to +-90 degrees -- the exact area of the row on the sphere (up to
    2 pi R^2); it needs evenly spaced latitudes, and a pole-to-pole grid sums to 2.  ``"none"``: ones."""
    lat = _latitudes(latitude_deg, "lat_weights")
    if kind not in KINDS:
        raise ValueError(f"lat_weights: kind = {kind!r}, one of {KINDS}")
    if kind == "none":
        return np.ones(lat.shape[0], dtype=np.float64)
    if kind == "cos":
        return np.maximum(np.cos(np.deg2rad(lat)), 0.0)
    n = lat.shape[0]
    if n < 2:
        raise ValueError("lat_weights: 'band' needs at least two latitude rows to know their spacing")
    d = np.diff(lat)
    step = (lat[-1] - lat[0]) / (n - 1)
    if step == 0.0 or (np.abs(d - step) > 1e-6 * abs(step)).any():
        raise ValueError("lat_weights: 'band' needs evenly spaced latitudes")
    mid = 0.5 * (lat[:-1] + lat[1:])
    edges = np.clip(np.concatenate([[lat[0] - 0.5 * step], mid, [lat[-1] + 0.5 * step]]), -90.0, 90.0)
    s = np.sin(np.deg2rad(edges))
    return np.abs(s[1:] - s[:-1])


def coarse_lat_band(nlat: int, fy: int, lat0: int, rank: int, world: int) -> tuple[int, int]:
    """Fine latitude rows [i0, i1) of rank ``rank``: the companion of ``era5_svd.lat_band`` for a grid that is coarsened.
    The ``NLAT = (nlat - lat0) // fy`` coarse rows are split into contiguous bands of nearly equal height, so every
    boundary falls on a cell boundary; over all ranks the bands cover exactly the rows ``lat0 .. lat0 + NLAT fy``.  A
    rank builds its :class:`Coarsen` from ``latitude[i0:i1]`` with ``lat0 = 0``."""
    nlat, fy, lat0, rank, world = (int(v) for v in (nlat, fy, lat0, rank, world))
    if fy < 1 or lat0 < 0 or not 0 <= rank < world:
        raise ValueError(f"coarse_lat_band: fy = {fy} < 1, lat0 = {lat0} < 0 or rank {rank} outside 0..{world - 1}")
    n_out = max(0, (nlat - lat0) // fy)
    if world > n_out:
        raise ValueError(f"{world} ranks for {n_out} coarse latitude rows: use at most one rank per coarse row")
    return lat0 + fy * (rank * n_out // world), lat0 + fy * ((rank + 1) * n_out // world)


class Coarsen:
    """The ``fy x fx`` block mean on the grid ``latitude x longitude`` (degrees; the fine coordinates of a plane, in the
    order of its rows and columns).  Cell (I, J) covers the fine rows ``lat0 + I fy ..`` and longitudes ``lon0 + J fx
    ..``: whole cells only, what lies outside them is dropped.  ``weights``: a kind of :func:`lat_weights` or an array
    of one non-negative finite weight per fine latitude row.  ``skipna``: values that are not finite are left out of
    a cell; a cell that keeps less than ``min_frac`` of its weight is NaN.  Without ``skipna`` a cell that holds a
    non-finite value is non-finite and ``min_frac`` plays no part."""

    def __init__(self, latitude, longitude, fy: int, fx: int, *, lat0: int = 0, lon0: int = 0, weights="cos",
                 skipna: bool = False, min_frac: float = 0.5, kern=None):
        self.latitude = _latitudes(latitude, "Coarsen")
        self.longitude = np.ascontiguousarray(np.asarray(longitude, dtype=np.float64))
        if self.longitude.ndim != 1 or not np.isfinite(self.longitude).all():
            raise ValueError(f"Coarsen: longitude must be a one-dimensional array of finite degrees, got {self.longitude.shape}")
        self.fy, self.fx, self.lat0, self.lon0 = int(fy), int(fx), int(lat0), int(lon0)
        if not (1 <= self.fy <= MAX_FACTOR and 1 <= self.fx <= MAX_FACTOR):
            raise ValueError(f"Coarsen: fy = {fy} or fx = {fx} outside 1..{MAX_FACTOR}")
        if self.lat0 < 0 or self.lon0 < 0:
            raise ValueError(f"Coarsen: lat0 = {lat0} or lon0 = {lon0} negative")
        nlat, nlon = self.shape_in
        self.n_lat_out, self.n_lon_out = max(0, (nlat - self.lat0) // self.fy), max(0, (nlon - self.lon0) // self.fx)
        if self.n_lat_out < 1 or self.n_lon_out < 1:
            raise ValueError(f"Coarsen: no {self.fy} x {self.fx} cell fits the {nlat} x {nlon} grid from ({self.lat0}, {self.lon0})")
        if isinstance(weights, str):
            self.kind, self.weights = weights, lat_weights(self.latitude, weights)
        else:
            w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64))
            if w.shape != (nlat,):
                raise ValueError(f"Coarsen: weights must hold one weight per latitude row ({nlat}), got {w.shape}")
            if not np.isfinite(w).all() or (w < 0.0).any():
                raise ValueError("Coarsen: a weight is negative or not finite")
            self.kind, self.weights = "array", w
        self.skipna, self.min_frac = bool(skipna), float(min_frac)
        if not 0.0 <= self.min_frac <= 1.0:
            raise ValueError(f"Coarsen: min_frac = {min_frac} outside [0, 1]")
        self.kern = kern

    # -- geometry -------------------------------------------------------------------------------------------------
    @property
    def shape_in(self) -> tuple[int, int]:
        return int(self.latitude.shape[0]), int(self.longitude.shape[0])

    @property
    def shape_out(self) -> tuple[int, int]:
        return self.n_lat_out, self.n_lon_out

    @property
    def dropped(self) -> tuple[int, int]:
        """The latitude rows and the longitudes outside the cells (before the offsets and behind the last cell)."""
        nlat, nlon = self.shape_in
        return nlat - self.n_lat_out * self.fy, nlon - self.n_lon_out * self.fx

    def _cells(self, v: np.ndarray, first: int, f: int, n: int) -> np.ndarray:
        return v[first:first + n * f].reshape(n, f)

    @property
    def latitude_out(self) -> np.ndarray:
        """The fp64 mean of the latitudes of every coarse row."""
        return self._cells(self.latitude, self.lat0, self.fy, self.n_lat_out).mean(axis=1)

    @property
    def longitude_out(self) -> np.ndarray:
        return self._cells(self.longitude, self.lon0, self.fx, self.n_lon_out).mean(axis=1)

    @property
    def weights_out(self) -> np.ndarray:
        """Per coarse latitude row the fp64 sum of the weights of its fine rows: the area weight of the coarse grid."""
        return self._cells(self.weights, self.lat0, self.fy, self.n_lat_out).sum(axis=1)

    def rows_in(self, planes: int) -> int:
        return int(planes) * self.shape_in[0] * self.shape_in[1]

    def rows_out(self, planes: int) -> int:
        return int(planes) * self.n_lat_out * self.n_lon_out

    def row_weights_out(self, planes: int) -> torch.Tensor:
        """:attr:`weights_out` repeated over the longitudes and the planes: one fp32 weight per row of a coarsened
        block of ``planes`` planes, what ``verify_blocks(weights=...)`` and ``crps_blocks`` take."""
        w = np.tile(np.repeat(self.weights_out, self.n_lon_out), int(planes))
        return torch.from_numpy(w.astype(np.float32))

    # -- apply ----------------------------------------------------------------------------------------------------
    def apply(self, Xblocks, planes, out=None) -> list:
        """The coarsened blocks: per ``(T, rows)`` fp32 block of ``Xblocks`` one launch and one ``(T, planes_b NLAT
        NLON)`` fp32 tensor -- fresh, or the view ``out[b]`` (inner stride 1, not overlapping the block).  ``planes``:
        the planes (variable x level) of every block, an int or one int per block; the rows of a block beyond
        ``planes_b nlat nlon`` are pad and are ignored, a block with fewer rows is a ValueError.  Everything is checked
        before the first launch; the weights are uploaded once per device."""
        Xblocks = list(Xblocks)
        if isinstance(planes, (int, np.integer)):
            planes = [int(planes)] * len(Xblocks)
        planes = [int(p) for p in planes]
        if len(planes) != len(Xblocks) or any(p < 1 for p in planes):
            raise ValueError(f"Coarsen.apply: {len(Xblocks)} blocks, planes = {planes}: one positive count per block")
        for b, (X, p) in enumerate(zip(Xblocks, planes)):
            if X.dim() != 2:
                raise ValueError(f"Coarsen.apply: block {b} must be (time, rows), got {tuple(X.shape)}")
            if int(X.shape[1]) < self.rows_in(p):
                raise ValueError(f"Coarsen.apply: block {b} holds {int(X.shape[1])} rows, {p} planes of "
                                 f"{self.shape_in[0]} x {self.shape_in[1]} need {self.rows_in(p)}")
        if out is not None:
            out = list(out)
            if len(out) != len(Xblocks):
                raise ValueError(f"Coarsen.apply: {len(Xblocks)} blocks, out holds {len(out)}")
            for b, (X, p, Y) in enumerate(zip(Xblocks, planes, out)):
                if tuple(Y.shape) != (int(X.shape[0]), self.rows_out(p)):
                    raise ValueError(f"Coarsen.apply: out[{b}] is {tuple(Y.shape)}, ({int(X.shape[0])}, {self.rows_out(p)}) "
                                     "asked for")
        kern = _kern(self.kern)
        w = ta.OnDevices(self.weights)
        nlat, nlon = self.shape_in
        return [kern.coarsen(X, p, nlat, nlon, w.on(X.device), self.fy, self.fx, lat0=self.lat0, lon0=self.lon0,
                             n_lat_out=self.n_lat_out, n_lon_out=self.n_lon_out, skipna=self.skipna,
                             min_frac=self.min_frac, out=None if out is None else out[b])
                for b, (X, p) in enumerate(zip(Xblocks, planes))]

    def apply_field(self, vec: torch.Tensor, planes: int) -> torch.Tensor:
        """A static per-row vector (a mean, a climatology slot) of ``planes`` planes, coarsened as one snapshot:
        ``(rows,)`` fp32 -> ``(planes NLAT NLON,)`` fp32."""
        if vec.dim() != 1:
            raise ValueError(f"Coarsen.apply_field: a (rows,) vector asked for, got {tuple(vec.shape)}")
        return self.apply([vec.reshape(1, -1)], int(planes))[0].reshape(-1)

    # -- persistence ----------------------------------------------------------------------------------------------
    def to_dataset(self) -> Dataset:
        """``coarsen_weights(latitude)`` fp64 with the fine ``latitude`` and ``longitude`` as coordinates and the
        factors, the offsets, the weight kind, ``skipna`` and ``min_frac`` (``repr`` of the fp64: an exact round trip)
        as attributes; ``io_netcdf.to_netcdf`` writes it."""
        lat, lon = Coord("latitude", self.latitude.copy()), Coord("longitude", self.longitude.copy())
        ds = Dataset(coords={"latitude": lat, "longitude": lon}, attrs={
            "fy": self.fy, "fx": self.fx, "lat0": self.lat0, "lon0": self.lon0, "weights": str(self.kind),
            "skipna": int(self.skipna), "min_frac": repr(self.min_frac)})
        ds["coarsen_weights"] = DataArray(self.weights.copy(), ("latitude",), {"latitude": lat})
        return ds

    @classmethod
    def from_dataset(cls, ds: Dataset, kern=None) -> "Coarsen":
        """The coarsening :meth:`to_dataset` stored: the weights bit for bit (a kind of :func:`lat_weights` is kept as
        the kind, and the stored array is what is applied)."""
        a = ds.attrs
        res = cls(np.asarray(ds.coords["latitude"].values, dtype=np.float64),
                  np.asarray(ds.coords["longitude"].values, dtype=np.float64), ta.attr_int(a["fy"]), ta.attr_int(a["fx"]),
                  lat0=ta.attr_int(a["lat0"]), lon0=ta.attr_int(a["lon0"]),
                  weights=np.asarray(ds["coarsen_weights"].values, dtype=np.float64), skipna=bool(ta.attr_int(a["skipna"])),
                  min_frac=float(ta.attr_str(a["min_frac"])), kern=kern)
        res.kind = ta.attr_str(a["weights"])
        return res

    def to_netcdf(self, path: str) -> str:
        return io_netcdf.to_netcdf(self.to_dataset(), path)

    @classmethod
    def from_netcdf(cls, path: str, kern=None) -> "Coarsen":
        return cls.from_dataset(io_netcdf.open_dataset(path), kern)
