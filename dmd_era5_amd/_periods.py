"""What :mod:`spells` (K27) and :mod:`extremes` (K29) share on the host: the periods of a fit, the check of the blocks
against the stamps, offsets as stamps, the area mean over row blocks, and the common half of ``to_dataset`` /
``from_dataset``.  The planes may have any number of axes before ``(P, rows)``."""
from __future__ import annotations

import numpy as np
import torch

from . import _timeaxis as ta
from .forecast import _check_weights, _group_pieces
from .labeled import Coord, DataArray, Dataset
from .svd import Comm


KINDS = ("year", "month", "season", "all")
_SEASONS = ("DJF", "MAM", "JJA", "SON")


def periods_of(times, kind: str = "year"):
    """Time stamps -> ``(bounds, labels)``: the P + 1 int32 positions that cut the snapshots into periods -- period p is
    ``times[bounds[p]:bounds[p + 1]]`` -- and a label per period (a numpy array of strings).

    ``kind``: ``"year"`` ("2001"), ``"month"`` ("2001-03"), ``"season"`` ("2001-DJF": December to February is labelled
    by the year of its January; a season cut off at either end of the series is kept as it is) or ``"all"`` (one
    period, "all").  The times must be strictly ascending, else a ValueError."""
    if kind not in KINDS:
        raise ValueError(f"periods_of: kind = {kind!r}, expected one of {KINDS}")
    t = ta.stamps(times, "periods_of")
    T = int(t.shape[0])
    if T == 0:
        raise ValueError("periods_of: no times")
    if T > 1 and not (np.diff(t.astype("datetime64[ns]").astype(np.int64)) > 0).all():
        raise ValueError("periods_of: times must be strictly ascending: a period is a run of consecutive snapshots")
    months = t.astype("datetime64[M]").astype(np.int64)             # months since 1970-01
    if kind == "all":
        key, names = np.zeros(T, dtype=np.int64), lambda k: "all"
    elif kind == "year":
        key, names = months // 12, lambda k: f"{1970 + k:04d}"
    elif kind == "month":
        key, names = months, lambda k: f"{1970 + k // 12:04d}-{k % 12 + 1:02d}"
    else:
        key = (months + 1) // 3                                      # Dec, Jan, Feb share a value; 3 key is the January
        names = lambda k: f"{1970 + (3 * k) // 12:04d}-{_SEASONS[k % 4]}"
    cuts = np.flatnonzero(np.diff(key)) + 1
    bounds = np.concatenate([[0], cuts, [T]]).astype(np.int32)
    return bounds, np.array([names(int(key[b])) for b in bounds[:-1]])


def bounds_list(bounds, who: str) -> list:
    raw = np.asarray(bounds)
    if raw.ndim != 1 or raw.size < 2 or raw.dtype.kind not in "iu":
        raise ValueError(f"{who}: bounds must be at least two integers, got {bounds!r}")
    b = [int(v) for v in raw]
    if b[0] < 0 or any(y <= x for x, y in zip(b, b[1:])):
        raise ValueError(f"{who}: bounds must be >= 0 and strictly ascending, got {b[:8]}{' ...' if len(b) > 8 else ''}")
    return b


def resolve_periods(times, period, who: str):
    """-> ``(t, bounds, labels)``: the stamps as datetime64[ns] (None without ``times``), the P + 1 int32 positions
    and the P labels.  ``period``: a kind of :func:`periods_of` (needs ``times``), or the bounds themselves."""
    t = None if times is None else ta.stamps(times, who).astype("datetime64[ns]")
    if isinstance(period, str):
        if t is None:
            raise ValueError(f"{who}: period = {period!r} needs times")
        bounds, labels = periods_of(t, period)
    else:
        bounds = np.asarray(bounds_list(period, who), dtype=np.int32)
        labels = np.array([str(p) for p in range(bounds.shape[0] - 1)])
        if t is not None and bounds[-1] > t.shape[0]:
            raise ValueError(f"{who}: the bounds end at {int(bounds[-1])}, times has {t.shape[0]}")
    return t, bounds, labels


def checked_blocks(Xblocks, t, who: str):
    """The blocks as they come, each checked against the stamps before it is read."""
    for b, X in enumerate(Xblocks):
        T = int(X.shape[0])
        if t is not None and T != t.shape[0]:
            raise ValueError(f"{who}: block {b} holds {T} snapshots, times has {t.shape[0]}")
        yield X


def ratio(num, den):
    """num / den where den > 0, NaN elsewhere."""
    return torch.where(den > 0, num / torch.where(den > 0, den, torch.ones_like(den)), torch.full_like(den, float("nan")))


def when(offsets, start, scale: int, times, who: str) -> list:
    """Offsets from the start of a period as stamps: per block ``times[start + offset * scale]`` (numpy datetime64),
    NaT where the offset is negative.  ``offsets``: per block a (..., P, rows) integer tensor; ``start``: the (P,)
    first snapshots of the periods."""
    if times is None:
        raise ValueError(f"{who}: fitted without times: only the offsets are known")
    start = np.asarray(start).astype(np.int64)[:, None]
    out = []
    for o in offsets:
        o = o.cpu().numpy().astype(np.int64)
        stamp = times[np.where(o >= 0, start + o * scale, 0)]
        stamp[o < 0] = np.datetime64("NaT")
        out.append(stamp)
    return out


def area_mean_sums(planes_valid, values, keep_extra, weights, groups, n_groups, comm, tag: str, who: str) -> dict:
    """The area-weighted mean of an index per group of rows.  Per block: ``planes_valid`` the (..., P, rows) count
    of valid snapshots or days, ``values`` the index in the same shape; a row counts where its weight is not 0, the
    count is positive and ``keep_extra(value)`` (None: everywhere) holds.  ``weights``, ``groups``, ``n_groups`` as
    :func:`baseline.baseline_scores` -> ``mean`` (G, ..., P) fp64 (NaN where no row counts), ``weight`` the sum of
    the weights and ``rows`` (int64) the number of the rows that count; ONE ``comm.allreduce_sum_`` under ``tag``."""
    comm = comm or Comm()
    weights = _check_weights(weights, who)
    rows_of = [int(nv.shape[-1]) for nv in planes_valid]
    if weights is not None and len(weights) != len(rows_of):
        raise ValueError(f"{who}: {len(weights)} weight vectors for {len(rows_of)} blocks")
    pieces, G = _group_pieces(groups, rows_of, [1] * len(rows_of), n_groups, who)
    shape = (3, G) + tuple(planes_valid[0].shape[:-1])
    # the numbers of a row: reduced on the host, in one order whatever the device
    sums = torch.zeros(shape, dtype=torch.float64)
    for b, (nv, val) in enumerate(zip(planes_valid, values)):
        w = torch.ones(rows_of[b], dtype=torch.float64) if weights is None else \
            torch.as_tensor(weights[b]).to(device="cpu", dtype=torch.float64).reshape(-1)
        if w.numel() != rows_of[b]:
            raise ValueError(f"{who}: weights[{b}] has {w.numel()} entries, the block {rows_of[b]} rows")
        val = val.cpu().to(torch.float64)
        keep = (w != 0) & (nv.cpu() > 0)
        if keep_extra is not None:
            keep = keep & keep_extra(val)
        ww = torch.where(keep, w.expand_as(val), torch.zeros_like(val))
        wv = torch.where(keep, ww * val, torch.zeros_like(val))
        for s, e, g in pieces[b]:
            sums[0, g] += wv[..., s:e].sum(dim=-1)
            sums[1, g] += ww[..., s:e].sum(dim=-1)
            sums[2, g] += keep[..., s:e].sum(dim=-1)
    sums = comm.allreduce_sum_(sums.reshape(-1).to(planes_valid[0].device), tag=tag).cpu().reshape(shape)
    return {"mean": ratio(sums[0], sums[1]), "weight": sums[1], "rows": sums[2].to(torch.int64)}


def to_dataset(var: str, planes, dtype, bounds, labels, times, coords, own_dim: str, own_vars: dict) -> Dataset:
    """``var(plane, space)``: the planes of every block flattened to (planes, rows) and joined along the rows;
    ``period_bound(bound)``; ``own_vars`` as int64 variables along ``own_dim``; the stamps as ``time_s`` /
    ``time_ns(time_index)`` (absent without times); the attribute ``period_labels``, the labels joined by commas."""
    n_planes = int(np.prod(planes[0].shape[:-1]))
    own = {name: np.asarray(v, dtype=np.int64) for name, v in own_vars.items()}
    cds = {"plane": Coord("plane", np.arange(n_planes, dtype=np.int64)),
           "bound": Coord("bound", np.arange(len(bounds), dtype=np.int64)),
           own_dim: Coord(own_dim, np.arange(len(next(iter(own.values()))), dtype=np.int64)), **ta.row_coords(coords)}
    ds = Dataset(coords=cds, attrs={"period_labels": ",".join(str(v) for v in labels)})
    row = {k: v for k, v in cds.items() if k not in ("plane", "bound", own_dim)}
    field = np.concatenate([Q.detach().cpu().numpy().reshape(n_planes, -1) for Q in planes], axis=1)
    ds[var] = DataArray(field.astype(dtype), ("plane", "space"), {"plane": cds["plane"], **row})
    ds["period_bound"] = DataArray(bounds.astype(np.int64), ("bound",), {"bound": cds["bound"]})
    for name, v in own.items():
        ds[name] = DataArray(v, (own_dim,), {own_dim: cds[own_dim]})
    if times is not None:
        ns = times.astype("datetime64[ns]").astype(np.int64)
        tc = Coord("time_index", np.arange(ns.shape[0], dtype=np.int64))
        ds.coords["time_index"] = tc
        ds["time_s"] = DataArray(ns // 10**9, ("time_index",), {"time_index": tc})
        ds["time_ns"] = DataArray(ns % 10**9, ("time_index",), {"time_index": tc})
    return ds


def from_dataset(ds: Dataset, var: str, dtype):
    """What :func:`to_dataset` stored -> ``(field, bounds, labels, times)``: the (planes, rows) field as it is."""
    field = np.ascontiguousarray(np.asarray(ds[var].values), dtype=dtype)
    bounds = np.asarray(ds["period_bound"].values).astype(np.int32).reshape(-1)
    text = ta.attr_str(ds.attrs["period_labels"]) if "period_labels" in ds.attrs else ""
    labels = np.array(text.split(",")) if text else np.array([str(p) for p in range(int(bounds.shape[0]) - 1)])
    times = None
    if "time_s" in ds:
        s = np.asarray(ds["time_s"].values).astype(np.int64).reshape(-1)
        times = (s * 10**9 + np.asarray(ds["time_ns"].values).astype(np.int64).reshape(-1)).astype("datetime64[ns]")
    return field, bounds, labels, times


class Periods:
    """What both results carry in their fields ``bounds``, ``labels``, ``times`` and ``kern``."""

    @property
    def n_periods(self) -> int:
        return int(self.bounds.shape[0]) - 1

    def period_years(self) -> np.ndarray:
        """The decimal year of the first stamp of every period, (P,) fp64 (2001.0 for 2001-01-01T00, the fraction by
        the length of its own year): the time coordinate ``MannKendall.fit`` takes.  A ValueError without ``times``."""
        if self.times is None:
            raise ValueError(f"{type(self).__name__}.period_years: fitted without times: the periods have no dates")
        t = self.times[np.asarray(self.bounds[:-1]).astype(np.int64)].astype("datetime64[ns]")
        year = t.astype("datetime64[Y]")
        start, end = year.astype("datetime64[ns]"), (year + 1).astype("datetime64[ns]")
        return 1970.0 + year.astype(np.int64) + (t - start).astype(np.int64) / (end - start).astype(np.int64)

    def _when(self, offsets: list, scale: int, who: str) -> list:
        return when(offsets, self.bounds[:-1], scale, self.times, f"{type(self).__name__}.{who}")
