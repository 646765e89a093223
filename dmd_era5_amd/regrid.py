"""Area-weighted coarsening (K23, csrc/coarsen.hip) and conservative remapping (K28, csrc/remap.hip) of the snapshots on
the device: the two operations on the space axis.

When to use which.  :class:`Coarsen` takes whole ``fy x fx`` blocks of the source grid and nothing else: it is the
fastest way down from 0.25 degrees, and the grid it gives is the project's own (721 x 1440 by 4 x 4: 180 x 360, one pole
row dropped, the first longitude at 0.375).  :class:`Remap` lands on a grid someone else also uses -- the regular
1 degree grid with both poles (181 x 360), 1.5 degrees (121 x 240), the half-cell-offset 5.625 degree grid -- where
target cells cut source cells, wrap around in longitude and end in a clipped cap at the poles.  Fields, scores and
``write_forecast_slice`` files on such a grid can be laid over another data set.  Both have the same surface and feed
the same chain.

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

    rm = Remap.regular(latitude, longitude, 1.0, 1.0)            # 721 x 1440 -> 181 x 360, poles kept, longitudes 0, 1, ..
    Yblocks = rm.apply(Xblocks, planes)                          # first-order conservative, separable
    w_rows = rm.row_weights_out(planes_b)                        # the exact areas of the target rows

The remapping is first-order conservative: a target cell is the area-weighted mean of the source cells it overlaps,
each weighted by the area of the overlap.  Both grids are regular and node-centred, so the overlap factors into a
latitude part (exact band areas, ``sin`` of the edges) and a longitude part (degrees), formed here in fp64 in pure
numpy as six small tables; ``HipKernels.remap`` applies them.  Row shards: :func:`remap_lat_band`.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _timeaxis as ta
from . import io_netcdf
from .labeled import Coord, DataArray, Dataset
from .svd import _kern

__all__ = ["KINDS", "lat_weights", "coarse_lat_band", "Coarsen", "REMAP_KINDS", "remap_lat_band", "Remap"]

KINDS = ("cos", "band", "none")
MAX_FACTOR = 64                                                 # dmdx_coarsen_max_factor()
REMAP_KINDS = ("band", "none")
MAX_SPAN = 64                                                   # dmdx_remap_max_span()
SLIVER = 1e-9                                                   # of a source cell's width: below it an overlap is rounding noise


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


# ---- K28: conservative remapping onto another regular grid -----------------------------------------------------------
def _axis(values, who: str, name: str) -> np.ndarray:
    v = np.ascontiguousarray(np.asarray(values, dtype=np.float64))
    if v.ndim != 1 or v.shape[0] < 1 or not np.isfinite(v).all():
        raise ValueError(f"{who}: {name} must be a one-dimensional array of finite degrees, got {v.shape}")
    return v


def _step(v: np.ndarray, who: str, name: str) -> float:
    """The step of evenly spaced centres (1e-6 relative), of either sign."""
    n = v.shape[0]
    if n < 2:
        raise ValueError(f"{who}: {name} needs at least two points to know its spacing")
    step = (v[-1] - v[0]) / (n - 1)
    if step == 0.0 or (np.abs(np.diff(v) - step) > 1e-6 * abs(step)).any():
        raise ValueError(f"{who}: {name} must be evenly spaced")
    return float(step)


def _lat_edges(lat: np.ndarray, who: str, name: str) -> np.ndarray:
    """The n + 1 edges of n latitude rows, as ``lat_weights(kind="band")`` forms them: the midpoints between
    neighbouring rows, the outer edges half a step beyond the first and the last row, clipped to +-90 degrees."""
    step = _step(lat, who, name)
    mid = 0.5 * (lat[:-1] + lat[1:])
    return np.clip(np.concatenate([[lat[0] - 0.5 * step], mid, [lat[-1] + 0.5 * step]]), -90.0, 90.0)


def _given_edges(edges, lat: np.ndarray, who: str, name: str) -> np.ndarray:
    e = np.ascontiguousarray(np.asarray(edges, dtype=np.float64))
    if e.shape != (lat.shape[0] + 1,) or not np.isfinite(e).all() or (np.abs(e) > 90.0).any():
        raise ValueError(f"{who}: {name} must hold {lat.shape[0] + 1} finite edges in [-90, 90], got {e.shape}")
    d = np.diff(e)
    lo, hi = np.minimum(e[:-1], e[1:]), np.maximum(e[:-1], e[1:])
    if not ((d > 0).all() or (d < 0).all()) or (lat < lo).any() or (lat > hi).any():
        raise ValueError(f"{who}: {name} must be strictly monotone with every row between its two edges")
    return e


def _area(lo: np.ndarray, hi: np.ndarray) -> np.ndarray:
    """The area of the latitude band lo .. hi (degrees) on the unit sphere, up to 2 pi."""
    return np.abs(np.sin(np.deg2rad(hi)) - np.sin(np.deg2rad(lo)))


def _overlap_tables(slo, shi, tlo, thi, period: float, weight, who: str, axis: str):
    """Per target cell ``tlo .. thi`` the source cells ``slo .. shi`` it overlaps: (first, count, w), w (nt, S) zero
    beyond the count.  An overlap below SLIVER of the source cell's width is rounding noise of the edges and is dropped;
    a target cell that the source does not cover beyond that is a ValueError.  ``period`` > 0: the source wraps (the
    walk goes on at cell 0 behind the last one), and ``first`` lies in 0 .. ns - 1."""
    ns, nt = slo.shape[0], tlo.shape[0]
    width = shi - slo
    if period > 0.0:
        k = np.floor((tlo - slo[0]) / period)
        tlo, thi = tlo - k * period, thi - k * period             # every target cell starts inside the first period
        slo, shi, width = np.concatenate([slo, slo + period]), np.concatenate([shi, shi + period]), np.concatenate([width, width])
    first, count, rows = np.zeros(nt, dtype=np.int64), np.zeros(nt, dtype=np.int64), []
    for c in range(nt):
        lo, hi = np.maximum(tlo[c], slo), np.minimum(thi[c], shi)
        idx = np.flatnonzero(hi - lo > SLIVER * width)
        covered = float((hi - lo)[idx].sum()) if idx.size else 0.0
        if idx.size == 0 or (thi[c] - tlo[c]) - covered > SLIVER * float(width.max()):
            raise ValueError(f"{who}: target {axis} {c} ({tlo[c]:.6f} .. {thi[c]:.6f} degrees) is not covered by the source grid")
        if idx[-1] - idx[0] + 1 != idx.size:
            raise ValueError(f"{who}: target {axis} {c} overlaps source cells that are not neighbours")
        if idx.size > MAX_SPAN or idx.size > ns:
            raise ValueError(f"{who}: target {axis} {c} spans {idx.size} source cells, at most {min(MAX_SPAN, ns)} can be taken")
        first[c], count[c] = idx[0] % ns, idx.size
        rows.append(weight(lo[idx], hi[idx]))
    w = np.zeros((nt, int(count.max())), dtype=np.float64)
    for c, r in enumerate(rows):
        w[c, :r.shape[0]] = r
    return first.astype(np.int32), count.astype(np.int32), w


def _lat_tables(es: np.ndarray, et: np.ndarray, kind: str, who: str):
    weight = _area if kind == "band" else (lambda lo, hi: hi - lo)
    return _overlap_tables(np.minimum(es[:-1], es[1:]), np.maximum(es[:-1], es[1:]), np.minimum(et[:-1], et[1:]),
                           np.maximum(et[:-1], et[1:]), 0.0, weight, who, "row")


def remap_lat_band(latitude, latitude_out, rank: int, world: int):
    """Rank ``rank``'s share of a remapping whose rows are sharded: ``((I0, I1), (i0, i1), edges, edges_out)``.  The
    target rows are split into contiguous bands of nearly equal height, ``[I0, I1)`` is this rank's; ``[i0, i1)`` are
    the source rows the band touches (neighbouring ranks share the rows their boundary cuts), ``edges`` the slice
    ``i0 .. i1`` of the global source edges and ``edges_out`` the slice ``I0 .. I1`` of the global target edges.  A
    rank builds its :class:`Remap` from ``latitude[i0:i1]``, ``latitude_out[I0:I1]``, ``lat_edges=edges`` and
    ``lat_edges_out=edges_out``; its tables are then the global ones bit for bit (``iy0`` shifted by ``i0``).  The
    outer edge of a band is the midpoint to a row the rank does not hold, so neither set of edges can be rebuilt from
    the slices alone."""
    who = "remap_lat_band"
    lat, lat_out = _latitudes(latitude, who), _latitudes(latitude_out, who)
    rank, world = int(rank), int(world)
    if not 0 <= rank < world:
        raise ValueError(f"{who}: rank {rank} outside 0..{world - 1}")
    if world > lat_out.shape[0]:
        raise ValueError(f"{world} ranks for {lat_out.shape[0]} target latitude rows: use at most one rank per target row")
    es, et = _lat_edges(lat, who, "latitude"), _lat_edges(lat_out, who, "latitude_out")
    iy0, ny, _ = _lat_tables(es, et, "none", who)
    n = lat_out.shape[0]
    I0, I1 = rank * n // world, (rank + 1) * n // world
    i0, i1 = int(iy0[I0:I1].min()), int((iy0[I0:I1] + ny[I0:I1]).max())
    return (I0, I1), (i0, i1), es[i0:i1 + 1].copy(), et[I0:I1 + 1].copy()


class Remap:
    """First-order conservative remapping from the regular grid ``latitude x longitude`` (degrees, node-centred, evenly
    spaced; latitude in either direction, longitude ascending) onto the regular grid ``latitude_out x longitude_out``.
    Latitude edges are the midpoints between neighbouring rows, the outer ones half a step beyond, clipped to +-90
    degrees (a clipped cap at a pole); longitude edges are centre +- half a step, and the source wraps where its
    longitudes go around the globe (``nlon * step`` is 360 degrees to 1e-6).  A target cell is the mean of the source
    cells it overlaps, weighted by the overlap: in latitude its exact area (``weights="band"``) or its degrees
    (``"none"``), in longitude its degrees.  Every target cell must be covered by the source; spans are at most 64
    source cells per axis; a target finer than the source is fine.  ``skipna`` / ``min_frac``: as :class:`Coarsen`.
    ``lat_edges`` (nlat + 1 values) and ``lat_edges_out`` (NLAT + 1) override the midpoint rule, for row shards
    (:func:`remap_lat_band`)."""

    def __init__(self, latitude, longitude, latitude_out, longitude_out, *, weights="band", skipna: bool = False,
                 min_frac: float = 0.5, lat_edges=None, lat_edges_out=None, kern=None):
        who = "Remap"
        lat, lat_out = _latitudes(latitude, who), _latitudes(latitude_out, who)
        lon, lon_out = _axis(longitude, who, "longitude"), _axis(longitude_out, who, "longitude_out")
        if lat.shape[0] < 1 or lat_out.shape[0] < 1:
            raise ValueError(f"{who}: an empty latitude axis")
        if weights not in REMAP_KINDS:
            raise ValueError(f"{who}: weights = {weights!r}, one of {REMAP_KINDS}")
        es = _lat_edges(lat, who, "latitude") if lat_edges is None else _given_edges(lat_edges, lat, who, "lat_edges")
        et = (_lat_edges(lat_out, who, "latitude_out") if lat_edges_out is None
              else _given_edges(lat_edges_out, lat_out, who, "lat_edges_out"))
        if lat_edges is not None and lat.shape[0] > 2:
            _step(lat, who, "latitude")
        if lat_edges_out is not None and lat_out.shape[0] > 2:
            _step(lat_out, who, "latitude_out")
        iy0, ny, wy = _lat_tables(es, et, weights, who)
        sx, tx = _step(lon, who, "longitude"), _step(lon_out, who, "longitude_out")
        if sx < 0.0 or tx < 0.0:
            raise ValueError(f"{who}: longitudes must ascend")
        period = 360.0 if abs(lon.shape[0] * sx - 360.0) <= 1e-6 * 360.0 else 0.0
        jx0, nx, wx = _overlap_tables(lon - 0.5 * sx, lon + 0.5 * sx, lon_out - 0.5 * tx, lon_out + 0.5 * tx, period,
                                      lambda lo, hi: hi - lo, who, "column")
        self._set(lat, lon, lat_out, lon_out, (iy0, ny, wy, jx0, nx, wx), weights, skipna, min_frac, kern)

    def _set(self, lat, lon, lat_out, lon_out, tables, kind, skipna, min_frac, kern) -> None:
        """Everything :meth:`apply` uses, validated: the tables are applied as they stand."""
        who = "Remap"
        self.latitude, self.longitude, self._lat_out, self._lon_out = lat, lon, lat_out, lon_out
        nlat, nlon, NLAT, NLON = lat.shape[0], lon.shape[0], lat_out.shape[0], lon_out.shape[0]
        iy0, ny, wy, jx0, nx, wx = tables
        iy0, ny, jx0, nx = (np.ascontiguousarray(np.asarray(v, dtype=np.int32)) for v in (iy0, ny, jx0, nx))
        wy, wx = (np.ascontiguousarray(np.asarray(v, dtype=np.float64)) for v in (wy, wx))
        for first, count, w, n, N, name in ((iy0, ny, wy, nlat, NLAT, "latitude"), (jx0, nx, wx, nlon, NLON, "longitude")):
            if first.shape != (N,) or count.shape != (N,) or w.ndim != 2 or w.shape[0] != N:
                raise ValueError(f"{who}: the {name} tables must hold {N} target cells, got {first.shape}, {count.shape}, {w.shape}")
            if not 1 <= w.shape[1] <= MAX_SPAN:
                raise ValueError(f"{who}: a {name} span of {w.shape[1]} source cells, 1..{MAX_SPAN} can be taken")
            if (count < 1).any() or (count > w.shape[1]).any() or (count > n).any() or (first < 0).any() or (first >= n).any():
                raise ValueError(f"{who}: a {name} table points outside the source grid")
            valid = np.arange(w.shape[1])[None, :] < count[:, None]
            if not np.isfinite(w[valid]).all() or (w[valid] < 0.0).any():
                raise ValueError(f"{who}: a {name} weight is negative or not finite")
        if ((iy0.astype(np.int64) + ny) > nlat).any():
            raise ValueError(f"{who}: a latitude table points outside the source grid")   # (longitudes wrap)
        self.iy0, self.ny, self.wy, self.jx0, self.nx, self.wx = iy0, ny, wy, jx0, nx, wx
        self.kind, self.skipna, self.min_frac, self.kern = str(kind), bool(skipna), float(min_frac), kern
        if not 0.0 <= self.min_frac <= 1.0:
            raise ValueError(f"{who}: min_frac = {min_frac} outside [0, 1]")

    @classmethod
    def from_tables(cls, latitude, longitude, latitude_out, longitude_out, iy0, ny, wy, jx0, nx, wx, *, weights="tables",
                    skipna: bool = False, min_frac: float = 0.5, kern=None) -> "Remap":
        """A remapping from its six tables as they are (:meth:`from_dataset`; tables of one's own)."""
        res = cls.__new__(cls)
        res._set(_latitudes(latitude, "Remap"), _axis(longitude, "Remap", "longitude"), _latitudes(latitude_out, "Remap"),
                 _axis(longitude_out, "Remap", "longitude_out"), (iy0, ny, wy, jx0, nx, wx), weights, skipna, min_frac, kern)
        return res

    @classmethod
    def blocks(cls, latitude, longitude, fy: int, fx: int, *, lat0: int = 0, lon0: int = 0, weights="cos",
               skipna: bool = False, min_frac: float = 0.5, kern=None) -> "Remap":
        """``Coarsen(latitude, longitude, fy, fx, ...)`` as a remapping: whole ``fy x fx`` blocks, the row weights of
        :func:`lat_weights` and unit longitude weights.  It gives the bits of :class:`Coarsen` (K28's contract is
        K23's term for term then); what it is for is checking and measuring one against the other."""
        cz = Coarsen(latitude, longitude, fy, fx, lat0=lat0, lon0=lon0, weights=weights, skipna=skipna, min_frac=min_frac)
        NLAT, NLON = cz.shape_out
        iy0, jx0 = cz.lat0 + cz.fy * np.arange(NLAT), cz.lon0 + cz.fx * np.arange(NLON)
        wy = cz.weights[iy0[:, None] + np.arange(cz.fy)[None, :]]
        return cls.from_tables(cz.latitude, cz.longitude, cz.latitude_out, cz.longitude_out, iy0, np.full(NLAT, cz.fy), wy, jx0,
                               np.full(NLON, cz.fx), np.ones((NLON, cz.fx)), weights=cz.kind, skipna=skipna, min_frac=min_frac,
                               kern=kern)

    @classmethod
    def regular(cls, latitude, longitude, dlat: float, dlon: float, *, poles: bool = True, lon0=None, **kw) -> "Remap":
        """The standard target of a global source: rows every ``dlat`` degrees from the source's first latitude to its
        last (``poles=True``: 721 rows at 0.25 degrees and ``dlat = 1`` give 181, both poles kept) or, with
        ``poles=False``, offset by half a cell from the source's outer edge (5.625 degrees: 32 rows from 87.1875);
        columns every ``dlon`` from ``lon0`` (default: the source's first longitude) once around the source's
        longitudes.  ``dlat`` and ``dlon`` must divide the source's extent; what else ``Remap`` takes passes through."""
        who = "Remap.regular"
        lat, lon = _latitudes(latitude, who), _axis(longitude, who, "longitude")
        dlat, dlon = float(dlat), float(dlon)
        if not (dlat > 0.0 and dlon > 0.0):
            raise ValueError(f"{who}: dlat = {dlat} and dlon = {dlon} must be positive")
        es, sx = _lat_edges(lat, who, "latitude"), _step(lon, who, "longitude")
        sign = 1.0 if lat[-1] > lat[0] else -1.0
        start, span = (lat[0], abs(lat[-1] - lat[0])) if poles else (es[0], abs(es[-1] - es[0]))
        n = int(round(span / dlat))
        if n < 1 or abs(n * dlat - span) > 1e-6 * dlat:
            raise ValueError(f"{who}: dlat = {dlat} does not divide the {span} degrees of the source's latitudes")
        lat_out = start + sign * dlat * (np.arange(n + 1) if poles else np.arange(n) + 0.5)
        m = int(round(lon.shape[0] * sx / dlon))
        if m < 1 or abs(m * dlon - lon.shape[0] * sx) > 1e-6 * dlon:
            raise ValueError(f"{who}: dlon = {dlon} does not divide the {lon.shape[0] * sx} degrees of the source's longitudes")
        lon_out = (float(lon[0]) if lon0 is None else float(lon0)) + dlon * np.arange(m)
        return cls(lat, lon, np.clip(lat_out, -90.0, 90.0), lon_out, **kw)

    # -- geometry -------------------------------------------------------------------------------------------------
    @property
    def shape_in(self) -> tuple[int, int]:
        return int(self.latitude.shape[0]), int(self.longitude.shape[0])

    @property
    def shape_out(self) -> tuple[int, int]:
        return int(self._lat_out.shape[0]), int(self._lon_out.shape[0])

    @property
    def latitude_out(self) -> np.ndarray:
        return self._lat_out

    @property
    def longitude_out(self) -> np.ndarray:
        return self._lon_out

    @property
    def weights_out(self) -> np.ndarray:
        """Per target latitude row the fp64 sum of its ``wy``: with ``"band"`` the exact area of the row."""
        valid = np.arange(self.wy.shape[1])[None, :] < self.ny[:, None]
        return np.where(valid, self.wy, 0.0).sum(axis=1)

    def rows_in(self, planes: int) -> int:
        return int(planes) * self.shape_in[0] * self.shape_in[1]

    def rows_out(self, planes: int) -> int:
        return int(planes) * self.shape_out[0] * self.shape_out[1]

    def row_weights_out(self, planes: int) -> torch.Tensor:
        """:attr:`weights_out` repeated over the longitudes and the planes: one fp32 weight per row of a remapped block
        of ``planes`` planes, what ``verify_blocks(weights=...)`` and ``crps_blocks`` take."""
        w = np.tile(np.repeat(self.weights_out, self.shape_out[1]), int(planes))
        return torch.from_numpy(w.astype(np.float32))

    # -- apply ----------------------------------------------------------------------------------------------------
    def apply(self, Xblocks, planes, out=None) -> list:
        """The remapped blocks: per ``(T, rows)`` fp32 block of ``Xblocks`` one launch and one ``(T, planes_b NLAT
        NLON)`` fp32 tensor -- fresh, or the view ``out[b]`` (inner stride 1, not overlapping the block).  ``planes``:
        an int or one int per block; the rows of a block beyond ``planes_b nlat nlon`` are pad and are ignored, a
        block with fewer rows is a ValueError.  Everything is checked before the first launch; the tables are
        uploaded once per device."""
        Xblocks = list(Xblocks)
        if isinstance(planes, (int, np.integer)):
            planes = [int(planes)] * len(Xblocks)
        planes = [int(p) for p in planes]
        if len(planes) != len(Xblocks) or any(p < 1 for p in planes):
            raise ValueError(f"Remap.apply: {len(Xblocks)} blocks, planes = {planes}: one positive count per block")
        for b, (X, p) in enumerate(zip(Xblocks, planes)):
            if X.dim() != 2:
                raise ValueError(f"Remap.apply: block {b} must be (time, rows), got {tuple(X.shape)}")
            if int(X.shape[1]) < self.rows_in(p):
                raise ValueError(f"Remap.apply: block {b} holds {int(X.shape[1])} rows, {p} planes of "
                                 f"{self.shape_in[0]} x {self.shape_in[1]} need {self.rows_in(p)}")
        if out is not None:
            out = list(out)
            if len(out) != len(Xblocks):
                raise ValueError(f"Remap.apply: {len(Xblocks)} blocks, out holds {len(out)}")
            for b, (X, p, Y) in enumerate(zip(Xblocks, planes, out)):
                if tuple(Y.shape) != (int(X.shape[0]), self.rows_out(p)):
                    raise ValueError(f"Remap.apply: out[{b}] is {tuple(Y.shape)}, ({int(X.shape[0])}, {self.rows_out(p)}) "
                                     "asked for")
        kern = _kern(self.kern)
        tables = [ta.OnDevices(t) for t in (self.iy0, self.ny, self.wy, self.jx0, self.nx, self.wx)]
        nlat, nlon = self.shape_in
        return [kern.remap(X, p, nlat, nlon, *(t.on(X.device) for t in tables), skipna=self.skipna, min_frac=self.min_frac,
                           out=None if out is None else out[b])
                for b, (X, p) in enumerate(zip(Xblocks, planes))]

    def apply_field(self, vec: torch.Tensor, planes: int) -> torch.Tensor:
        """A static per-row vector (a mean, a climatology slot) of ``planes`` planes, remapped as one snapshot:
        ``(rows,)`` fp32 -> ``(planes NLAT NLON,)`` fp32."""
        if vec.dim() != 1:
            raise ValueError(f"Remap.apply_field: a (rows,) vector asked for, got {tuple(vec.shape)}")
        return self.apply([vec.reshape(1, -1)], int(planes))[0].reshape(-1)

    # -- persistence ----------------------------------------------------------------------------------------------
    def to_dataset(self) -> Dataset:
        """The six tables as they are applied (``remap_iy0``, ``remap_ny``, ``remap_wy``, ``remap_jx0``, ``remap_nx``,
        ``remap_wx``; the indices as fp64, which holds them exactly) with the four coordinate axes, and the weight
        kind, ``skipna`` and ``min_frac`` (``repr`` of the fp64) as attributes; ``io_netcdf.to_netcdf`` writes it."""
        c = {"latitude": Coord("latitude", self.latitude.copy()), "longitude": Coord("longitude", self.longitude.copy()),
             "latitude_out": Coord("latitude_out", self._lat_out.copy()),
             "longitude_out": Coord("longitude_out", self._lon_out.copy()),
             "span_y": Coord("span_y", np.arange(self.wy.shape[1], dtype=np.float64)),
             "span_x": Coord("span_x", np.arange(self.wx.shape[1], dtype=np.float64))}
        ds = Dataset(coords=c, attrs={"weights": self.kind, "skipna": int(self.skipna), "min_frac": repr(self.min_frac)})
        for name, v, dims in (("remap_iy0", self.iy0, ("latitude_out",)), ("remap_ny", self.ny, ("latitude_out",)),
                              ("remap_wy", self.wy, ("latitude_out", "span_y")), ("remap_jx0", self.jx0, ("longitude_out",)),
                              ("remap_nx", self.nx, ("longitude_out",)), ("remap_wx", self.wx, ("longitude_out", "span_x"))):
            ds[name] = DataArray(np.asarray(v, dtype=np.float64).copy(), dims, {d: c[d] for d in dims})
        return ds

    @classmethod
    def from_dataset(cls, ds: Dataset, kern=None) -> "Remap":
        """The remapping :meth:`to_dataset` stored: the stored tables are what is applied, bit for bit."""
        a = ds.attrs

        def axis(name):
            return np.asarray(ds.coords[name].values, dtype=np.float64)

        def table(name, dtype):
            v = np.asarray(ds[name].values, dtype=np.float64)
            return v if dtype is np.float64 else np.rint(v).astype(dtype)

        return cls.from_tables(axis("latitude"), axis("longitude"), axis("latitude_out"), axis("longitude_out"),
                               table("remap_iy0", np.int32), table("remap_ny", np.int32), table("remap_wy", np.float64),
                               table("remap_jx0", np.int32), table("remap_nx", np.int32), table("remap_wx", np.float64),
                               weights=ta.attr_str(a["weights"]), skipna=bool(ta.attr_int(a["skipna"])),
                               min_frac=float(ta.attr_str(a["min_frac"])), kern=kern)

    def to_netcdf(self, path: str) -> str:
        return io_netcdf.to_netcdf(self.to_dataset(), path)

    @classmethod
    def from_netcdf(cls, path: str, kern=None) -> "Remap":
        return cls.from_dataset(io_netcdf.open_dataset(path), kern)
