"""Slot climatology of the snapshots and anomalies against it (K18, csrc/clim.hip).

K5 removes the mean of a grid point over ALL of time (the reference's ``standardize_data``).  ERA5 temperature,
geopotential and wind are dominated by the annual and the diurnal cycle, and a DMD is fitted to what is left once
they are gone: the anomalies against a climatology that depends on the hour of the day and the time of the year.
A *slot* is a class of the calendar; this module turns time stamps into slots on the host (:func:`slots_of`, pure
numpy), and the device forms the mean (and standard deviation) of every row per slot and subtracts / restores it
(``HipKernels.clim_mean`` / ``clim_std`` / ``clim_apply_``): one read of the resident ``(time, rows)`` blocks for the
mean, one read and one write for the anomalies, no fp64 copy and no gathered ``mean[slot]`` second X.

    clim = Climatology.fit(Xblocks, times, "month_hour")       # (288, rows) per block
    clim.remove_(Xblocks, times)                               # X <- X - clim[slot(t)], in place
    fields = forecast.fields(t, climatology=clim, times=valid) # the model's anomalies back to full fields

Rows are independent: row shards fit and apply their own blocks, no collective is involved.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _timeaxis as ta
from .labeled import Coord, DataArray, Dataset
from .svd import _kern

__all__ = ["KINDS", "slots_of", "Climatology"]

# kind -> number of slots
KINDS = {"hour": 24, "month_hour": 288, "dayofyear": 366, "dayofyear_hour": 8784}
_LEAP_CUM = np.array([0, 31, 60, 91, 121, 152, 182, 213, 244, 274, 305, 335], dtype=np.int64)


def _calendar(times):
    """-> (month 0..11, day of the year 0..365 in the LEAP calendar -- Feb 29 is 59, Mar 1 is 60 in every year --,
    hour 0..23) of datetime64 time stamps."""
    t = ta.stamps(times, "slots_of", TypeError)
    days = t.astype("datetime64[D]")
    months = t.astype("datetime64[M]")
    month = months.astype(np.int64) % 12
    dom = (days - months.astype("datetime64[D]")).astype(np.int64)
    hour = (t.astype("datetime64[h]") - days.astype("datetime64[h]")).astype(np.int64)
    return month, _LEAP_CUM[month] + dom, hour


def slots_of(times, kind: str, window_days: int = 0):
    """Time stamps -> the slot lists K18 takes: ``(slot, order, start, S)``.

    ``kind``: ``"hour"`` (24 slots), ``"month_hour"`` (288: month * 24 + hour), ``"dayofyear"`` (366, counted in the
    leap calendar: Feb 29 is slot 59 and exists in leap years only) or ``"dayofyear_hour"`` (8784: day * 24 + hour).
    ``slot`` (T,) int32: the snapshot's own class.  ``order`` / ``start`` (int32; ``start`` has S + 1 entries): the
    CSR list of the members -- slot s owns ``order[start[s]:start[s + 1]]``, ascending in time.
    ``window_days`` = w > 0 (the two day-of-year kinds only): slot s lists every snapshot whose day of the year is
    within w days of it, circularly over 366 (with the same hour for ``"dayofyear_hour"``): a smoother climatology
    from few years, each snapshot in 2 w + 1 slots.  ``slot`` stays the snapshot's own class."""
    if kind not in KINDS:
        raise ValueError(f"slots_of: kind = {kind!r}, expected one of {sorted(KINDS)}")
    w = int(window_days)
    if w < 0 or (w > 0 and not kind.startswith("dayofyear")):
        raise ValueError(f"slots_of: window_days = {window_days} needs a day-of-year kind and w >= 0")
    if 2 * w + 1 > 366:
        raise ValueError(f"slots_of: a window of +-{w} days covers the year more than once")
    S = KINDS[kind]
    month, doy, hour = _calendar(times)
    T = int(doy.shape[0])
    per_day = 24 if kind == "dayofyear_hour" else 1
    if kind == "hour":
        slot = hour
    elif kind == "month_hour":
        slot = month * 24 + hour
    elif kind == "dayofyear":
        slot = doy
    else:
        slot = doy * 24 + hour
    if T * (2 * w + 1) >= 2**31:
        raise ValueError(f"slots_of: {T} snapshots x {2 * w + 1} slots each do not fit an int32 list")
    if w == 0:
        key, idx = slot, np.arange(T, dtype=np.int64)
    else:
        sub = hour if per_day == 24 else 0
        off = np.arange(-w, w + 1, dtype=np.int64)
        key = (((doy[None, :] + off[:, None]) % 366) * per_day + sub).reshape(-1)
        idx = np.tile(np.arange(T, dtype=np.int64), off.shape[0])
    stamps = np.atleast_1d(np.asarray(times)).astype("datetime64[ns]").astype(np.int64)
    perm = np.lexsort((idx, stamps[idx], key))                  # by slot, then time, then index
    order = idx[perm].astype(np.int32)
    start = np.searchsorted(key[perm], np.arange(S + 1, dtype=np.int64)).astype(np.int32)
    return slot.astype(np.int32), order, start, S


QUANTILE_METHODS = ("linear", "lower", "higher")


def _probabilities(quantiles, method: str, who: str) -> tuple:
    """``quantiles`` as a tuple of 1 .. 4 floats in [0, 1] (K25 takes as many as K24 takes thresholds)."""
    qs = tuple(float(v) for v in np.atleast_1d(np.asarray(quantiles, dtype=np.float64)).reshape(-1))
    if not 1 <= len(qs) <= 4 or not all(0.0 <= v <= 1.0 for v in qs):
        raise ValueError(f"{who}: quantiles must hold 1 .. 4 values in [0, 1], got {quantiles!r}")
    if method not in QUANTILE_METHODS:
        raise ValueError(f"{who}: method = {method!r}, expected one of {QUANTILE_METHODS}")
    return qs


@dataclass
class Climatology:
    """The slot climatology of a list of row blocks: ``mean`` (and ``sd``) hold one ``(S, rows)`` fp32 tensor per
    block, ``counts`` (S,) the snapshots every slot was formed from, ``ddof`` the one of ``sd``.  With quantiles (K25):
    ``q`` the J probabilities, ``quant`` one ``(J, S, rows)`` fp32 tensor per block, ``method`` how a position between
    two members was resolved."""

    kind: str
    window_days: int
    mean: list
    sd: list | None
    counts: np.ndarray
    ddof: int = 0
    kern: object = None
    q: tuple | None = None
    quant: list | None = None
    method: str = "linear"

    @property
    def n_slots(self) -> int:
        return KINDS[self.kind]

    # -- fit ------------------------------------------------------------------------------------------------------
    @classmethod
    def fit(cls, Xblocks, times, kind: str, window_days: int = 0, with_std: bool = False, ddof: int = 0,
            kern=None, quantiles=None, method: str = "linear") -> "Climatology":
        """The climatology of the snapshots ``Xblocks`` ((T, rows) fp32 per block, any iterable consumed once) taken
        at ``times`` (T datetime64 stamps): one read of every block for the mean, one more with ``with_std``, one
        more with ``quantiles`` (1 .. 4 probabilities in [0, 1]: the empirical quantiles of every slot and row, K25;
        ``method``: ``"linear"``, ``"lower"`` or ``"higher"``, numpy's names) -- the percentile thresholds of
        :meth:`quantile_thresholds`."""
        if ddof not in (0, 1):
            raise ValueError(f"Climatology.fit: ddof = {ddof}, expected 0 or 1")
        qs = None if quantiles is None else _probabilities(quantiles, method, "Climatology.fit")
        kern = _kern(kern)
        _, order, start, S = slots_of(times, kind, window_days)
        T = int(np.atleast_1d(np.asarray(times)).shape[0])
        orders, starts, mean, sd, quant = ta.OnDevices(order), ta.OnDevices(start), [], [], []
        for b, X in enumerate(Xblocks):
            if X.shape[0] != T:
                raise ValueError(f"Climatology.fit: block {b} holds {int(X.shape[0])} snapshots, times has {T}")
            o, s = orders.on(X.device), starts.on(X.device)
            mean.append(kern.clim_mean(X, o, s))
            if with_std:
                sd.append(kern.clim_std(X, o, s, mean[-1], ddof=ddof))
            if qs is not None:
                quant.append(kern.clim_quantile(X, o, s, qs, method=method))
        return cls(kind, int(window_days), mean, sd if with_std else None, np.diff(start.astype(np.int64)), int(ddof), kern,
                   qs, quant if qs is not None else None, method if qs is not None else "linear")

    # -- apply ----------------------------------------------------------------------------------------------------
    def _labels(self, times, who: str) -> np.ndarray:
        slot = slots_of(times, self.kind)[0]
        empty = np.unique(slot[self.counts[slot] == 0])
        if empty.size:
            raise ValueError(f"Climatology.{who}: slot {int(empty[0])} of kind {self.kind!r} was fitted from no snapshot"
                             f" ({empty.size} unpopulated slots are asked for): its climatology is not defined")
        return slot

    def _apply(self, Xblocks, times, out, restore: bool, use_sd: bool, who: str) -> list:
        slot = self._labels(times, who)                           # (raises before any launch)
        Xblocks = list(Xblocks)
        if len(Xblocks) != len(self.mean):
            raise ValueError(f"Climatology.{who}: {len(Xblocks)} blocks, the climatology holds {len(self.mean)}")
        kern = _kern(self.kern)
        labels, res = ta.OnDevices(slot), []
        for b, X in enumerate(Xblocks):
            if tuple(X.shape) != (slot.shape[0], int(self.mean[b].shape[1])):
                raise ValueError(f"Climatology.{who}: block {b} is {tuple(X.shape)}, {slot.shape[0]} times and "
                                 f"{int(self.mean[b].shape[1])} rows asked for")
            sd = self.sd[b] if (use_sd and self.sd is not None) else None
            res.append(kern.clim_apply_(X, labels.on(X.device), self.mean[b], sd, restore=restore,
                                        out=None if out is None else out[b]))
        return res

    def remove_(self, Xblocks, times, out=None) -> list:
        """``X <- (X - mean[slot(t)]) [/ sd[slot(t)]]`` for the snapshots taken at ``times``, one launch per block;
        in place, or into the list ``out`` of (T, rows) fp32 views that do not overlap X.  A time whose slot was
        fitted from no snapshot is a ValueError before any launch."""
        return self._apply(Xblocks, times, out, False, True, "remove_")

    def restore_(self, Xblocks, times, out=None) -> list:
        """The inverse of :meth:`remove_`: ``X <- X [* sd] + mean`` (two roundings)."""
        return self._apply(Xblocks, times, out, True, True, "restore_")

    def at(self, times) -> list:
        """The climatology fields of ``times``: per block a (T, rows) fp32 tensor, ``mean[slot(t)]`` -- restore on
        zeros without the standard deviation."""
        T = int(np.atleast_1d(np.asarray(times)).shape[0])
        Z = [torch.zeros((T, int(M.shape[1])), dtype=torch.float32, device=M.device) for M in self.mean]
        return self._apply(Z, times, None, True, False, "at")

    # -- thresholds of an exceedance forecast (K24) ---------------------------------------------------------------
    def slots(self, times) -> np.ndarray:
        """The slot of every time as int32 labels 0 .. S - 1: the ``slot`` of ``forecast.exceed_blocks`` /
        ``exceed_prob_blocks`` for thresholds from :meth:`thresholds`.  A time whose slot was fitted from no snapshot
        is a ValueError."""
        return self._labels(times, "slots").astype(np.int32)

    def thresholds(self, z, anomaly: bool = True) -> list:
        """Climatological thresholds for every slot and row: per block a (J, S, rows) fp32 tensor, ``z[j] * sd`` with
        ``anomaly`` (for a model and an analysis the slot means were removed from, not divided by ``sd``) and
        ``mean + z[j] * sd`` otherwise, each operation rounded to fp32 -- z = 1.2816 is the upper decile of a normal
        climate.  A slot that was fitted from no snapshot has NaN thresholds (no event).  Without ``sd`` a
        ValueError."""
        if self.sd is None:
            raise ValueError("Climatology.thresholds: the climatology holds no standard deviation (fit with with_std=True)")
        zs = [float(v) for v in np.atleast_1d(np.asarray(z, dtype=np.float64))]
        if not zs or not all(np.isfinite(zs)):
            raise ValueError(f"Climatology.thresholds: z must hold at least one finite factor, got {z!r}")
        res = []
        for M, D in zip(self.mean, self.sd):
            zt = torch.tensor(zs, dtype=torch.float32, device=D.device)[:, None, None]
            th = zt * D[None]
            res.append((th if anomaly else M[None] + th).contiguous())
        return res

    def quantile_thresholds(self, anomaly: bool = False) -> list:
        """The empirical quantiles as thresholds: per block the (J, S, rows) fp32 table ``exceed_blocks`` /
        ``exceed_prob_blocks`` / ``DmdForecast.ensemble_exceedance`` take, threshold j = quantile ``q[j]`` of the
        slot.  ``anomaly``: ``quant - mean`` rounded once, for a model fitted on anomalies whose climatology was
        fitted on the full fields.  A slot that was fitted from no snapshot has NaN thresholds (no event).  Without
        quantiles a ValueError."""
        if self.quant is None:
            raise ValueError("Climatology.quantile_thresholds: the climatology holds no quantiles (fit with quantiles=)")
        if not anomaly:
            return [Q.contiguous() for Q in self.quant]
        return [(Q - M[None]).contiguous() for Q, M in zip(self.quant, self.mean)]

    # -- persistence ----------------------------------------------------------------------------------------------
    def to_dataset(self, coords=None) -> Dataset:
        """``clim_mean(slot, space)``, ``clim_std`` if there is one, ``clim_count(slot)`` and the attributes ``kind``,
        ``window_days``, ``ddof``; ``coords``: the per-row coordinates of the decomposed array (``space`` and what
        lives on it), taken over as they are.  ``io_netcdf.to_netcdf`` writes it."""
        S = self.n_slots
        cds = {"slot": Coord("slot", np.arange(S, dtype=np.int64)), **ta.row_coords(coords)}
        ds = Dataset(coords=cds, attrs={"kind": self.kind, "window_days": int(self.window_days), "ddof": int(self.ddof)})
        row = {k: v for k, v in cds.items() if k != "slot"}

        def field(blocks):
            return np.concatenate([B.detach().cpu().numpy() for B in blocks], axis=1)

        ds["clim_mean"] = DataArray(field(self.mean), ("slot", "space"), {"slot": cds["slot"], **row})
        if self.sd is not None:
            ds["clim_std"] = DataArray(field(self.sd), ("slot", "space"), {"slot": cds["slot"], **row})
        ds["clim_count"] = DataArray(np.asarray(self.counts, dtype=np.int64), ("slot",), {"slot": cds["slot"]})
        if self.quant is not None:
            qc = Coord("quantile", np.asarray(self.q, dtype=np.float64))
            ds.coords["quantile"] = qc
            ds.attrs["quantile_method"] = self.method
            ds["clim_quantile"] = DataArray(np.concatenate([B.detach().cpu().numpy() for B in self.quant], axis=2),
                                            ("quantile", "slot", "space"), {"quantile": qc, "slot": cds["slot"], **row})
        return ds

    @classmethod
    def from_dataset(cls, ds: Dataset, rows=None, device=None, kern=None) -> "Climatology":
        """The climatology :meth:`to_dataset` stored (``io_netcdf.open_dataset`` of its file).  ``rows``: the row
        counts of the blocks to cut the fields into (default: one block); ``device``: where they go (default: the
        GPU for the HIP provider)."""
        kern = _kern(kern)
        kind = ta.attr_str(ds.attrs["kind"])
        if kind not in KINDS:
            raise ValueError(f"Climatology.from_dataset: kind = {kind!r}")
        mean = np.ascontiguousarray(np.asarray(ds["clim_mean"].values), dtype=np.float32)
        S = mean.shape[0]
        if S != KINDS[kind]:
            raise ValueError(f"Climatology.from_dataset: clim_mean holds {S} slots, kind {kind!r} has {KINDS[kind]}")
        mean = ta.cut_rows(mean, rows, device, kern, "Climatology.from_dataset")
        sd = None
        if "clim_std" in ds:
            sd = ta.cut_rows(np.ascontiguousarray(np.asarray(ds["clim_std"].values), dtype=np.float32), rows, device,
                             kern, "Climatology.from_dataset")
        counts = np.asarray(ds["clim_count"].values).astype(np.int64).reshape(-1)
        qs, quant, method = None, None, "linear"
        if "clim_quantile" in ds:
            table = np.ascontiguousarray(np.asarray(ds["clim_quantile"].values), dtype=np.float32)
            J = int(table.shape[0])
            method = ta.attr_str(ds.attrs["quantile_method"])
            qs = _probabilities(np.asarray(ds.coords["quantile"].values, dtype=np.float64), method,
                                "Climatology.from_dataset")
            if table.shape[:2] != (len(qs), S):
                raise ValueError(f"Climatology.from_dataset: clim_quantile is {table.shape}, {len(qs)} quantiles of {S} "
                                 f"slots asked for")
            flat = ta.cut_rows(table.reshape(J * S, -1), rows, device, kern, "Climatology.from_dataset")
            quant = [F.reshape(J, S, -1) for F in flat]
        return cls(kind, ta.attr_int(ds.attrs["window_days"]), mean, sd, counts, ta.attr_int(ds.attrs["ddof"]), kern,
                   qs, quant, method)
