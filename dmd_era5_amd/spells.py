"""Spell and exceedance-count indices per grid point (K27, csrc/spell.hip): how often, how long and when a field lies
beyond a threshold.

``Climatology.fit(..., quantiles=(0.1, 0.9))`` gives percentile thresholds per slot of the calendar (K25).  The index a
climate user forms from them first is not a probability per snapshot but a count per YEAR and grid point: the
snapshots above the 90th percentile (TX90p / TN10p), those of them in runs of at least 6 (WSDI / CSDI), the longest
run (CDD / CWD), and where the first and the last such run of a season lie (heat-wave onset, first and last frost).
The device forms all of them for up to 4 thresholds in one read of the resident ``(time, rows)`` blocks
(``HipKernels.spells``): no (T, rows) masks, no cumulative sums with resets, no gathered copy of the thresholds.

    bounds, labels = periods_of(times, "year")
    stats = SpellStats.fit(Xblocks, times, climatology=clim, period="year", min_length=6)    # clim holds quantiles
    stats.frequency()                 # per block (J, P, rows): n_event / n_valid
    stats.spell_days()                # per block (J, P, rows): snapshots in runs of >= 6
    stats.onset(as_time=True)         # per block (J, P, rows) datetime64, NaT where there is no spell
    stats.area_mean("spell_days", weights=w, groups=g)           # (G, J, P), one collective
    frost = SpellStats.fit(Xblocks, times, thresholds=273.15, above=False, period="season")

A run never spans two periods: a spell that crosses New Year counts as two, the second with onset 0 (climdex's
default).  A snapshot that is not finite, has no slot or a NaN threshold is invalid: it is no event and ends a run.

The blocks of ``DmdForecast.fields(...)`` are ``(T, rows)`` fp32 blocks like any other, so the spells of a forecast
need no code of their own: pass the fields and their valid times.

Rows are independent: row shards fit their own blocks; :meth:`SpellStats.area_mean` makes one collective.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _timeaxis as ta
from .forecast import _check_weights, _group_pieces, _slot_labels, _threshold_tables
from .labeled import Coord, DataArray, Dataset
from .svd import Comm, _kern

__all__ = ["SEGMENT", "PLANES", "KINDS", "periods_of", "spell_blocks", "SpellStats"]

# the snapshots of a piece of the time split (HipKernels.spells); no result depends on it
SEGMENT = 512
PLANES = ("n_valid", "n_event", "n_spell", "n_in_spell", "longest", "first", "last")
KINDS = ("year", "month", "season", "all")
_SEASONS = ("DJF", "MAM", "JJA", "SON")
_INDICES = ("frequency", "spell_count", "spell_days", "longest", "onset", "end")


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


def _per_threshold(v, J, cast, who, name):
    a = [cast(x) for x in np.atleast_1d(np.asarray(v)).reshape(-1)]
    if len(a) not in (1, J):
        raise ValueError(f"{who}: {name} must be one value or one per threshold ({J}), got {v!r}")
    return tuple(a * J if len(a) == 1 else a)


def _scalar_thresholds(thresholds):
    """The thresholds as a list of floats where they are plain numbers (one for every row and slot), else None."""
    if isinstance(thresholds, (int, float, np.integer, np.floating)):
        return [float(thresholds)]
    if isinstance(thresholds, (list, tuple, np.ndarray)) and len(thresholds) and all(
            isinstance(v, (int, float, np.integer, np.floating)) for v in thresholds):
        return [float(v) for v in thresholds]
    return None


def _bounds_list(bounds, who):
    raw = np.asarray(bounds)
    if raw.ndim != 1 or raw.size < 2 or raw.dtype.kind not in "iu":
        raise ValueError(f"{who}: bounds must be at least two integers, got {bounds!r}")
    b = [int(v) for v in raw]
    if b[0] < 0 or any(y <= x for x, y in zip(b, b[1:])):
        raise ValueError(f"{who}: bounds must be >= 0 and strictly ascending, got {b[:8]}{' ...' if len(b) > 8 else ''}")
    return b


def spell_blocks(Xblocks, thresholds, bounds, min_length=1, above=True, slot=None, kern=None) -> list:
    """The planes of ``HipKernels.spells`` for every block of ``Xblocks`` ((T, rows) fp32 per block, any iterable
    consumed once): per block a (J, 7, P, rows) int32 tensor, the planes in the order of :data:`PLANES`.

    ``thresholds``: per block a (J, S, rows) or (J, rows) fp32 table (``Climatology.quantile_thresholds()``,
    ``Climatology.thresholds(z)``), or plain numbers -- one or a list of J <= 4 -- that hold for every row (frost:
    ``273.15`` with ``above=False``).  ``bounds``: the P + 1 positions of :func:`periods_of`.  ``min_length`` (>= 1)
    and ``above`` (True: the event is x > threshold, False: x < threshold; strict): one value or one per threshold.
    ``slot``: the T slot labels in 0 .. S - 1 (``Climatology.slots(times)``), None for S = 1."""
    who = "spell_blocks"
    kern = _kern(kern)
    b = _bounds_list(bounds, who)
    scal = _scalar_thresholds(thresholds)
    Xblocks = list(Xblocks) if scal is None else Xblocks
    if scal is None:
        tabs, J, S = _threshold_tables(thresholds, len(Xblocks), who)
    else:
        tabs, J, S = None, len(scal), 1
    if not 1 <= J <= 4:
        raise ValueError(f"{who}: {J} thresholds, 1 .. 4 asked for")
    ml = _per_threshold(min_length, J, int, who, "min_length")
    ab = _per_threshold(above, J, bool, who, "above")
    if min(ml) < 1:
        raise ValueError(f"{who}: min_length must be >= 1, got {min_length!r}")
    labels, out = {}, []
    for i, X in enumerate(Xblocks):
        if X.dim() != 2 or b[-1] > int(X.shape[0]):
            raise ValueError(f"{who}: block {i} is {tuple(X.shape)}, the bounds end at {b[-1]}")
        T, rows = int(X.shape[0]), int(X.shape[1])
        if scal is not None:
            thr = torch.tensor(scal, dtype=torch.float32, device=X.device)[:, None, None].expand(J, 1, rows).contiguous()
        else:
            thr = tabs[i].to(X.device).contiguous()
            if int(thr.shape[2]) != rows:
                raise ValueError(f"{who}: thresholds[{i}] holds {int(thr.shape[2])} rows, the block {rows}")
        if (X.device, T) not in labels:
            labels[X.device, T] = _slot_labels(slot, S, T, X.device, who)
        out.append(kern.spells(X, thr, b, ml, ab, slot=labels[X.device, T], seg=SEGMENT))
    return out


@dataclass
class SpellStats:
    """The spell indices of a list of row blocks: ``planes`` holds one (J, 7, P, rows) int32 tensor per block
    (:func:`spell_blocks`), ``bounds`` the P + 1 positions of the periods, ``labels`` their names, ``times`` the T
    stamps (or None), ``min_length`` and ``above`` one value per threshold."""

    planes: list
    bounds: np.ndarray
    labels: np.ndarray
    min_length: tuple
    above: tuple
    times: np.ndarray | None = None
    kern: object = None

    @classmethod
    def fit(cls, Xblocks, times, thresholds=None, period="year", min_length=1, above=True, climatology=None, slot=None,
            kern=None) -> "SpellStats":
        """One read of every block.  ``times``: the T datetime64 stamps of the snapshots, strictly ascending;
        ``period``: a kind of :func:`periods_of`, or the bounds themselves (then ``times`` may be None).
        ``thresholds``: as :func:`spell_blocks`.  With a ``climatology`` that holds quantiles ``thresholds=None``
        means ``climatology.quantile_thresholds()``, and whenever a climatology is given the slots are
        ``climatology.slots(times)``; without one ``slot`` names them."""
        who = "SpellStats.fit"
        t = None if times is None else ta.stamps(times, who).astype("datetime64[ns]")
        if isinstance(period, str):
            if t is None:
                raise ValueError(f"{who}: period = {period!r} needs times")
            bounds, labels = periods_of(t, period)
        else:
            bounds = np.asarray(_bounds_list(period, who), dtype=np.int32)
            labels = np.array([str(p) for p in range(bounds.shape[0] - 1)])
            if t is not None and bounds[-1] > t.shape[0]:
                raise ValueError(f"{who}: the bounds end at {int(bounds[-1])}, times has {t.shape[0]}")
        if climatology is not None:
            if t is None or slot is not None:
                raise ValueError(f"{who}: a climatology takes its slots from times: pass times and no slot")
            if thresholds is None:
                thresholds = climatology.quantile_thresholds()
            slot = climatology.slots(t)
        if thresholds is None:
            raise ValueError(f"{who}: no thresholds (and no climatology with quantiles to take them from)")
        kern = _kern(kern)
        seen = []

        def checked():
            for b, X in enumerate(Xblocks):
                T = int(X.shape[0])
                if t is not None and T != t.shape[0]:
                    raise ValueError(f"{who}: block {b} holds {T} snapshots, times has {t.shape[0]}")
                seen.append(T)
                yield X

        planes = spell_blocks(checked(), thresholds, bounds, min_length, above, slot, kern)
        if not planes:
            raise ValueError(f"{who}: no blocks")
        J = int(planes[0].shape[0])
        return cls(planes, bounds, labels, _per_threshold(min_length, J, int, who, "min_length"),
                   _per_threshold(above, J, bool, who, "above"), t, kern)

    # -- the indices ------------------------------------------------------------------------------------------------
    @property
    def n_thresholds(self) -> int:
        return len(self.min_length)

    @property
    def n_periods(self) -> int:
        return int(self.bounds.shape[0]) - 1

    def period_lengths(self) -> np.ndarray:
        """The snapshots of every period, (P,) int64."""
        return np.diff(self.bounds.astype(np.int64))

    def _plane(self, name: str) -> list:
        return [Q[:, PLANES.index(name)] for Q in self.planes]

    def n_valid(self) -> list:
        return self._plane("n_valid")

    def n_event(self) -> list:
        return self._plane("n_event")

    def frequency(self) -> list:
        """n_event / n_valid per block, (J, P, rows) fp64; NaN where no snapshot of the period is valid."""
        out = []
        for Q in self.planes:
            nv, ne = Q[:, 0].to(torch.float64), Q[:, 1].to(torch.float64)
            out.append(torch.where(nv > 0, ne / nv.clamp(min=1.0), torch.full_like(nv, float("nan"))))
        return out

    def spell_count(self) -> list:
        """The runs of at least ``min_length`` events, (J, P, rows) int32."""
        return self._plane("n_spell")

    def spell_days(self) -> list:
        """The snapshots in runs of at least ``min_length`` events (WSDI / CSDI in snapshots), (J, P, rows) int32."""
        return self._plane("n_in_spell")

    def longest(self) -> list:
        """The longest run of events, qualifying or not (CDD / CWD in snapshots); 0 where there is none."""
        return self._plane("longest")

    def _when(self, name: str, as_time: bool, who: str) -> list:
        off = self._plane(name)
        if not as_time:
            return off
        if self.times is None:
            raise ValueError(f"SpellStats.{who}: fitted without times: only the offsets are known")
        start = self.bounds[:-1].astype(np.int64)[None, :, None]
        out = []
        for o in off:
            o = o.cpu().numpy().astype(np.int64)
            when = self.times[np.where(o >= 0, start + o, 0)]
            when[o < 0] = np.datetime64("NaT")
            out.append(when)
        return out

    def onset(self, as_time: bool = False) -> list:
        """Where the first qualifying run of the period starts: the offset from the period's first snapshot, (J, P,
        rows) int32, -1 where there is none; ``as_time``: the stamps instead (numpy datetime64, NaT where none)."""
        return self._when("first", as_time, "onset")

    def end(self, as_time: bool = False) -> list:
        """Where the last qualifying run of the period ends (its last snapshot), as :meth:`onset`."""
        return self._when("last", as_time, "end")

    # -- over the grid --------------------------------------------------------------------------------------------
    def area_mean(self, index: str, weights=None, groups=None, comm: Comm | None = None,
                  n_groups: int | None = None) -> dict:
        """The area-weighted mean of an index per group of rows, threshold and period.  ``index``: ``"frequency"``,
        ``"spell_count"``, ``"spell_days"``, ``"longest"``, ``"onset"`` or ``"end"`` (the last two as offsets, over
        the rows that have a qualifying run).  Conventions as :func:`baseline.baseline_scores`: ``weights`` per block
        the weight of every row (None: 1), a negative or non-finite one is a ValueError; ``groups`` per block an
        integer label vector (0 .. G - 1), ``n_groups`` G for ranks that do not see the largest label.  A row counts
        for (threshold, period) if its weight is not 0, it has a valid snapshot there and, for onset / end, a spell.

        Returns ``mean`` (G, J, P) fp64 = sum w index / sum w over the rows that count (NaN where none does),
        ``weight`` (G, J, P) = that sum w, and ``rows`` (G, J, P) int64, their number.  Row shards: ONE
        ``comm.allreduce_sum_`` of the stacked sums per call."""
        who = "SpellStats.area_mean"
        if index not in _INDICES:
            raise ValueError(f"{who}: index = {index!r}, expected one of {_INDICES}")
        comm = comm or Comm()
        weights = _check_weights(weights, who)
        rows_of = [int(Q.shape[3]) for Q in self.planes]
        if weights is not None and len(weights) != len(rows_of):
            raise ValueError(f"{who}: {len(weights)} weight vectors for {len(rows_of)} blocks")
        pieces, G = _group_pieces(groups, rows_of, [1] * len(rows_of), n_groups, who)
        J, P = self.n_thresholds, self.n_periods
        values = {"frequency": self.frequency, "spell_count": self.spell_count, "spell_days": self.spell_days,
                  "longest": self.longest, "onset": self.onset, "end": self.end}[index]()
        device = self.planes[0].device if self.planes else torch.device("cpu")
        # (J, P) numbers per row: reduced on the host, in one order whatever the device
        sums = torch.zeros((3, G, J, P), dtype=torch.float64)
        for b, (Q, val) in enumerate(zip(self.planes, values)):
            w = torch.ones(rows_of[b], dtype=torch.float64) if weights is None else \
                torch.as_tensor(weights[b]).to(device="cpu", dtype=torch.float64).reshape(-1)
            if w.numel() != rows_of[b]:
                raise ValueError(f"{who}: weights[{b}] has {w.numel()} entries, the block {rows_of[b]} rows")
            val = val.cpu().to(torch.float64)
            keep = (w != 0)[None, None] & (Q[:, 0].cpu() > 0)
            if index in ("onset", "end"):
                keep = keep & (val >= 0)
            ww = torch.where(keep, w[None, None].expand_as(val), torch.zeros_like(val))
            wv = torch.where(keep, ww * val, torch.zeros_like(val))
            for s, e, g in pieces[b]:
                sums[0, g] += wv[:, :, s:e].sum(dim=2)
                sums[1, g] += ww[:, :, s:e].sum(dim=2)
                sums[2, g] += keep[:, :, s:e].sum(dim=2)
        sums = comm.allreduce_sum_(sums.reshape(-1).to(device), tag="spell_allreduce").cpu().reshape(3, G, J, P)
        W = sums[1]
        mean = torch.where(W > 0, sums[0] / torch.where(W > 0, W, torch.ones_like(W)), torch.full_like(W, float("nan")))
        return {"mean": mean, "weight": W, "rows": sums[2].to(torch.int64)}

    # -- persistence ----------------------------------------------------------------------------------------------
    def to_dataset(self, coords=None) -> Dataset:
        """``spell_planes(plane, space)`` int32 with plane = (j 7 + q) P + p, ``period_bound(bound)``,
        ``min_length(threshold)``, ``above(threshold)``, the stamps as ``time_s`` / ``time_ns(time_index)`` (whole
        seconds since 1970 and the nanoseconds beyond; absent without times) and the attribute ``period_labels``
        (the labels joined by commas); ``coords``: the per-row coordinates of the decomposed array, taken over as they
        are.  ``io_netcdf.to_netcdf`` writes it."""
        J, P = self.n_thresholds, self.n_periods
        cds = {"plane": Coord("plane", np.arange(J * len(PLANES) * P, dtype=np.int64)),
               "bound": Coord("bound", np.arange(P + 1, dtype=np.int64)),
               "threshold": Coord("threshold", np.arange(J, dtype=np.int64)), **ta.row_coords(coords)}
        ds = Dataset(coords=cds, attrs={"period_labels": ",".join(str(v) for v in self.labels)})
        row = {k: v for k, v in cds.items() if k not in ("plane", "bound", "threshold")}
        field = np.concatenate([Q.detach().cpu().numpy().reshape(J * len(PLANES) * P, -1) for Q in self.planes], axis=1)
        ds["spell_planes"] = DataArray(field.astype(np.int32), ("plane", "space"), {"plane": cds["plane"], **row})
        ds["period_bound"] = DataArray(self.bounds.astype(np.int64), ("bound",), {"bound": cds["bound"]})
        ds["min_length"] = DataArray(np.asarray(self.min_length, dtype=np.int64), ("threshold",), {"threshold": cds["threshold"]})
        ds["above"] = DataArray(np.asarray(self.above, dtype=np.int64), ("threshold",), {"threshold": cds["threshold"]})
        if self.times is not None:
            ns = self.times.astype("datetime64[ns]").astype(np.int64)
            tc = Coord("time_index", np.arange(ns.shape[0], dtype=np.int64))
            ds.coords["time_index"] = tc
            ds["time_s"] = DataArray(ns // 10**9, ("time_index",), {"time_index": tc})
            ds["time_ns"] = DataArray(ns % 10**9, ("time_index",), {"time_index": tc})
        return ds

    @classmethod
    def from_dataset(cls, ds: Dataset, rows=None, device=None, kern=None) -> "SpellStats":
        """The statistics :meth:`to_dataset` stored (``io_netcdf.open_dataset`` of its file).  ``rows``: the row counts
        of the blocks to cut the planes into (default: one block); ``device``: where they go (default: the GPU for
        the HIP provider)."""
        who = "SpellStats.from_dataset"
        kern = _kern(kern)
        field = np.ascontiguousarray(np.asarray(ds["spell_planes"].values), dtype=np.int32)
        bounds = np.asarray(ds["period_bound"].values).astype(np.int32).reshape(-1)
        ml = tuple(int(v) for v in np.asarray(ds["min_length"].values).reshape(-1))
        ab = tuple(bool(v) for v in np.asarray(ds["above"].values).reshape(-1))
        J, P = len(ml), int(bounds.shape[0]) - 1
        if field.shape[0] != J * len(PLANES) * P or len(ab) != J:
            raise ValueError(f"{who}: spell_planes holds {field.shape[0]} planes, {J} thresholds and {P} periods ask for "
                             f"{J * len(PLANES) * P}")
        text = ta.attr_str(ds.attrs["period_labels"]) if "period_labels" in ds.attrs else ""
        labels = np.array(text.split(",")) if text else np.array([str(p) for p in range(P)])
        times = None
        if "time_s" in ds:
            s = np.asarray(ds["time_s"].values).astype(np.int64).reshape(-1)
            times = (s * 10**9 + np.asarray(ds["time_ns"].values).astype(np.int64).reshape(-1)).astype("datetime64[ns]")
        flat = ta.cut_rows(field, rows, device, kern, who)
        return cls([F.reshape(J, len(PLANES), P, -1) for F in flat], bounds, labels, ml, ab, times, kern)
