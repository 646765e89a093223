"""Per-period extremes and totals of a daily statistic per grid point (K29, csrc/pstat.hip): the block maxima, minima
and totals a climate user fits a trend or a GEV to.

:mod:`spells` counts how often and how long a field lies beyond a threshold.  The other half of the standard index set
is a VALUE per year (month, season) and grid point: the snapshots of a period are grouped into days of ``group``
snapshots, every day gives one number (``inner``: sum, mean, max, min or range of its finite snapshots), a running sum
over ``window`` days never crosses a period, and per period the device forms the count, the largest and the smallest
running value with their day, the total, and the total and count beyond a per-row threshold -- in one read of the
resident ``(time, rows)`` blocks (``HipKernels.period_stats``): no reshape to days, no fp64 copy, no unfold, no mask.

    g = snapshots_per_day(times)                          # 24 for hourly stamps
    tx = PeriodStats.fit(Xblocks, times, period="year", group=g, inner="max")
    tx.maximum(); tx.when_max(as_time=True)               # TXx and the day it fell, per block (P, rows)
    Trend.fit(tx.series("maximum"), years)                # the annual series as (P, rows) fp32 blocks

    index      field                  group  inner  window  threshold        accessor
    TXx        2 m temperature        g      max    1                        maximum()
    TNn                               g      min    1                        minimum()
    TXn                               g      max    1                        minimum()
    TNx                               g      min    1                        maximum()
    DTR                               g      range  1                        mean()
    Rx1day     precipitation          g      sum    1                        maximum()
    Rx5day                            g      sum    5                        maximum()
    PRCPTOT                           g      sum    1       1 mm, inclusive  total_beyond()
    SDII                              g      sum    1       1 mm, inclusive  intensity()
    R95pTOT                           g      sum    1       95th percentile  fraction_beyond() (of the total of all days;
                                                            of wet days      over PRCPTOT of a second fit for climdex's)
    degree     temperature - base     g      mean   1       0.0              total_beyond(); heating: below=True
    days       (subtract the base first: K18's ``remove_`` of a constant climatology, or ``X - base`` on the host)

A day with fewer than ``min_count`` finite snapshots (default: all ``group`` of them) is missing: it gives no value and
breaks a window.  ``threshold`` is one number or per block a ``(rows,)`` table -- for instance one slot of
``Climatology.quantile_thresholds()``; thresholds per calendar slot are K27's (:mod:`spells`).

The blocks of ``DmdForecast.fields(...)`` are ``(T, rows)`` fp32 blocks like any other, so the extremes of a forecast
need no code of their own: pass the fields and their valid times.

Rows are independent: row shards fit their own blocks; :meth:`PeriodStats.area_mean` makes one collective.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _periods as pp
from . import _timeaxis as ta
from .labeled import Dataset
from .svd import Comm, _kern

__all__ = ["SEGMENT", "PLANES", "INNER", "snapshots_per_day", "period_stat_blocks", "PeriodStats"]

# the DAYS of a piece of the time split (HipKernels.period_stats).  The fp64 sums of the planes "total" and
# "total_beyond" are formed per piece and the pieces added in order, so these two depend on it (in their last bits);
# n, max, argmax, min, argmin and count_beyond do not.
SEGMENT = 64
PLANES = ("n", "max", "argmax", "min", "argmin", "total", "total_beyond", "count_beyond")
INNER = ("sum", "mean", "max", "min", "range")
_INDICES = ("n_valid", "maximum", "minimum", "total", "total_beyond", "count_beyond", "when_max", "when_min", "mean",
            "intensity", "fraction_beyond")
_DAY_NS = 86_400 * 10**9


def snapshots_per_day(times) -> int:
    """The snapshots of a day: 86 400 s over the constant step of the stamps (24 for hourly data, 1 for daily).  An
    irregular axis, fewer than two stamps or a step that does not divide a day is a ValueError."""
    who = "snapshots_per_day"
    t = ta.stamps(times, who).astype("datetime64[ns]").astype(np.int64)
    if t.shape[0] < 2:
        raise ValueError(f"{who}: at least two stamps give a step, got {t.shape[0]}")
    d = np.diff(t)
    if d[0] <= 0 or not (d == d[0]).all():
        raise ValueError(f"{who}: the stamps must ascend in one constant step")
    if _DAY_NS % int(d[0]) != 0:
        raise ValueError(f"{who}: a step of {int(d[0])} ns does not divide a day")
    return _DAY_NS // int(d[0])


def _settings(group, inner, window, min_count, who):
    if not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in (group, window)) or group < 1:
        raise ValueError(f"{who}: group and window must be integers >= 1, got {group!r} and {window!r}")
    if inner not in INNER:
        raise ValueError(f"{who}: inner = {inner!r}, expected one of {INNER}")
    if not 1 <= window <= 8:
        raise ValueError(f"{who}: window = {window}, 1 .. 8 asked for")
    mc = int(group) if min_count is None else min_count
    if not isinstance(mc, (int, np.integer)) or isinstance(mc, bool) or not 1 <= mc <= group:
        raise ValueError(f"{who}: min_count = {min_count!r}, an integer in 1 .. group = {group} asked for")
    return int(group), int(window), int(mc)


def _is_number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


def period_stat_blocks(Xblocks, bounds, group=1, inner="sum", window=1, min_count=None, threshold=None, below=False,
                       inclusive=False, kern=None) -> list:
    """The planes of ``HipKernels.period_stats`` for every block of ``Xblocks`` ((T, rows) fp32 per block, any iterable
    consumed once): per block an (8, P, rows) fp64 tensor, the planes in the order of :data:`PLANES`.

    ``bounds``: the P + 1 positions of :func:`spells.periods_of`.  ``group`` (>= 1): the snapshots of a day
    (:func:`snapshots_per_day`); ``inner``: one of :data:`INNER`; ``window``: 1 .. 8 days; ``min_count``: the finite
    snapshots a valid day needs, 1 .. group (None: group).  ``threshold``: None, one number for every row, or per block
    a (rows,) fp32 table; the event is value > threshold, < with ``below``, >= / <= with ``inclusive``."""
    who = "period_stat_blocks"
    kern = _kern(kern)
    b = pp.bounds_list(bounds, who)
    g, w, mc = _settings(group, inner, window, min_count, who)
    tabs = None
    if threshold is not None and not _is_number(threshold):
        Xblocks = list(Xblocks)
        tabs = list(threshold) if isinstance(threshold, (list, tuple)) else [threshold]
        if len(tabs) != len(Xblocks) or not all(isinstance(t, torch.Tensor) and t.dim() == 1 for t in tabs):
            raise ValueError(f"{who}: threshold must be a number or one (rows,) tensor per block: {len(tabs)} tables for "
                             f"{len(Xblocks)} blocks")
    out = []
    for i, X in enumerate(Xblocks):
        if X.dim() != 2 or b[-1] > int(X.shape[0]):
            raise ValueError(f"{who}: block {i} is {tuple(X.shape)}, the bounds end at {b[-1]}")
        rows = int(X.shape[1])
        if threshold is None:
            thr = None
        elif tabs is None:
            thr = torch.full((rows,), float(threshold), dtype=torch.float32, device=X.device)
        else:
            if int(tabs[i].shape[0]) != rows:
                raise ValueError(f"{who}: threshold[{i}] holds {int(tabs[i].shape[0])} rows, the block {rows}")
            thr = tabs[i].to(device=X.device, dtype=torch.float32).contiguous()
        out.append(kern.period_stats(X, b, group=g, inner=inner, window=w, min_count=mc, thr=thr, below=bool(below),
                                     inclusive=bool(inclusive), seg=SEGMENT))
    return out


@dataclass
class PeriodStats(pp.Periods):
    """The period statistics of a list of row blocks: ``planes`` holds one (8, P, rows) fp64 tensor per block
    (:func:`period_stat_blocks`), ``bounds`` the P + 1 positions of the periods, ``labels`` their names, ``times`` the
    T stamps (or None), the rest the settings of the fit."""

    planes: list
    bounds: np.ndarray
    labels: np.ndarray
    group: int
    inner: str
    window: int
    min_count: int
    below: bool = False
    inclusive: bool = False
    has_threshold: bool = False
    times: np.ndarray | None = None
    kern: object = None

    @classmethod
    def fit(cls, Xblocks, times, period="year", group=1, inner="sum", window=1, min_count=None, threshold=None,
            below=False, inclusive=False, kern=None) -> "PeriodStats":
        """One read of every block.  ``times``: the T datetime64 stamps of the snapshots, strictly ascending;
        ``period``: a kind of :func:`spells.periods_of`, or the bounds themselves (then ``times`` may be None).  The
        rest as :func:`period_stat_blocks`."""
        who = "PeriodStats.fit"
        t, bounds, labels = pp.resolve_periods(times, period, who)
        g, w, mc = _settings(group, inner, window, min_count, who)
        kern = _kern(kern)
        planes = period_stat_blocks(pp.checked_blocks(Xblocks, t, who), bounds, g, inner, w, mc, threshold, below, inclusive,
                                    kern)
        if not planes:
            raise ValueError(f"{who}: no blocks")
        return cls(planes, bounds, labels, g, inner, w, mc, bool(below), bool(inclusive), threshold is not None, t, kern)

    # -- the indices ------------------------------------------------------------------------------------------------
    def period_days(self) -> np.ndarray:
        """The days of every period, the ragged last one included, (P,) int64."""
        return -(-np.diff(self.bounds.astype(np.int64)) // self.group)

    def _plane(self, name: str) -> list:
        return [Q[PLANES.index(name)] for Q in self.planes]

    def n_valid(self) -> list:
        """The days of the period that have a value (with a window: the windows of valid days only), (P, rows) fp64."""
        return self._plane("n")

    def maximum(self) -> list:
        """The largest value of the period (TXx, Rx1day, Rx5day), NaN where there is none."""
        return self._plane("max")

    def minimum(self) -> list:
        """The smallest value of the period (TNn), NaN where there is none."""
        return self._plane("min")

    def total(self) -> list:
        """The sum of the values of the period; +0.0 where there is none."""
        return self._plane("total")

    def total_beyond(self) -> list:
        """The sum of the values beyond the threshold (PRCPTOT with 1 mm, degree days with 0); +0.0 without one."""
        return self._plane("total_beyond")

    def count_beyond(self) -> list:
        """The number of values beyond the threshold (wet days)."""
        return self._plane("count_beyond")

    def mean(self) -> list:
        """total / n (DTR), NaN where the period has no value."""
        return [pp.ratio(Q[5], Q[0]) for Q in self.planes]

    def intensity(self) -> list:
        """total_beyond / count_beyond (SDII), NaN where nothing lies beyond the threshold."""
        return [pp.ratio(Q[6], Q[7]) for Q in self.planes]

    def fraction_beyond(self) -> list:
        """total_beyond / total (R95pTOT), NaN where the total is not positive."""
        return [pp.ratio(Q[6], Q[5]) for Q in self.planes]

    def _day(self, name: str, as_time: bool, who: str) -> list:
        off = [Q.to(torch.int64) for Q in self._plane(name)]
        return self._when(off, self.group, who) if as_time else off

    def when_max(self, as_time: bool = False) -> list:
        """The day of the period on which the maximum fell (the last day of its window; the first one among equal
        maxima): the offset in days from the period's start, (P, rows) int64, -1 where there is none; ``as_time``: the
        stamp of the first snapshot of that day instead (numpy datetime64, NaT where none)."""
        return self._day("argmax", as_time, "when_max")

    def when_min(self, as_time: bool = False) -> list:
        """The day of the minimum, as :meth:`when_max`."""
        return self._day("argmin", as_time, "when_min")

    def _index(self, name: str, who: str) -> list:
        if name not in _INDICES:
            raise ValueError(f"{who}: index = {name!r}, expected one of {_INDICES}")
        return getattr(self, name)()

    def series(self, name: str) -> list:
        """An index as ``(P, rows)`` fp32 blocks -- the periods take the place of the snapshots -- so that
        ``Trend.fit`` and ``LagStats.fit`` take the annual series as they are.  ``name``: an accessor of this class
        (``"maximum"``, ``"total"``, ``"mean"``, ``"when_max"``, ...)."""
        return [v.to(torch.float32).contiguous() for v in self._index(name, "PeriodStats.series")]

    # -- over the grid --------------------------------------------------------------------------------------------
    def area_mean(self, index: str, weights=None, groups=None, comm: Comm | None = None,
                  n_groups: int | None = None) -> dict:
        """The area-weighted mean of an index per group of rows and period.  ``index``: the name of an accessor
        (``when_max`` / ``when_min`` as offsets in days).  Conventions as :meth:`spells.SpellStats.area_mean`:
        ``weights`` per block the weight of every row (None: 1), a negative or non-finite one is a ValueError;
        ``groups`` per block an integer label vector (0 .. G - 1), ``n_groups`` G for ranks that do not see the largest
        label.  A row counts for a period if its weight is not 0, the period has a value there (n > 0) and the index is
        not NaN.

        Returns ``mean`` (G, P) fp64 = sum w index / sum w over the rows that count (NaN where none does), ``weight``
        (G, P) = that sum w, and ``rows`` (G, P) int64, their number.  Row shards: ONE ``comm.allreduce_sum_`` of the
        stacked sums per call."""
        who = "PeriodStats.area_mean"
        values = self._index(index, who)
        return pp.area_mean_sums(self._plane("n"), values, lambda v: ~torch.isnan(v), weights, groups, n_groups, comm,
                                 "pstat_allreduce", who)

    # -- persistence ----------------------------------------------------------------------------------------------
    def to_dataset(self, coords=None) -> Dataset:
        """``period_planes(plane, space)`` fp64 with plane = q P + p, ``period_bound(bound)``, ``settings(setting)``
        int64 -- group, the index of inner in :data:`INNER`, window, min_count, below, inclusive, has_threshold --
        the stamps as ``time_s`` / ``time_ns(time_index)`` (whole seconds since 1970 and the nanoseconds beyond;
        absent without times) and the attribute ``period_labels`` (the labels joined by commas); ``coords``: the
        per-row coordinates of the decomposed array, taken over as they are.  ``io_netcdf.to_netcdf`` writes it."""
        sets = [self.group, INNER.index(self.inner), self.window, self.min_count, int(self.below), int(self.inclusive),
                int(self.has_threshold)]
        return pp.to_dataset("period_planes", self.planes, np.float64, self.bounds, self.labels, self.times, coords, "setting",
                             {"settings": sets})

    @classmethod
    def from_dataset(cls, ds: Dataset, rows=None, device=None, kern=None) -> "PeriodStats":
        """The statistics :meth:`to_dataset` stored (``io_netcdf.open_dataset`` of its file).  ``rows``: the row counts
        of the blocks to cut the planes into (default: one block); ``device``: where they go (default: the GPU for
        the HIP provider)."""
        who = "PeriodStats.from_dataset"
        kern = _kern(kern)
        field, bounds, labels, times = pp.from_dataset(ds, "period_planes", np.float64)
        sets = [int(v) for v in np.asarray(ds["settings"].values).reshape(-1)]
        P = int(bounds.shape[0]) - 1
        if field.shape[0] != len(PLANES) * P or len(sets) != 7 or not 0 <= sets[1] < len(INNER):
            raise ValueError(f"{who}: period_planes holds {field.shape[0]} planes, {P} periods ask for {len(PLANES) * P}; "
                             f"settings holds {len(sets)} values")
        flat = ta.cut_rows(field, rows, device, kern, who)
        return cls([F.reshape(len(PLANES), P, -1) for F in flat], bounds, labels, sets[0], INNER[sets[1]], sets[2], sets[3],
                   bool(sets[4]), bool(sets[5]), bool(sets[6]), times, kern)
