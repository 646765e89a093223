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

from . import _periods as pp
from . import _timeaxis as ta
from ._periods import KINDS, periods_of
from .forecast import _slot_labels, _threshold_tables
from .labeled import Dataset
from .svd import Comm, _kern

__all__ = ["SEGMENT", "PLANES", "KINDS", "periods_of", "spell_blocks", "SpellStats"]

# the snapshots of a piece of the time split (HipKernels.spells); no result depends on it
SEGMENT = 512
PLANES = ("n_valid", "n_event", "n_spell", "n_in_spell", "longest", "first", "last")
_INDICES = ("frequency", "spell_count", "spell_days", "longest", "onset", "end")


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
    b = pp.bounds_list(bounds, who)
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
class SpellStats(pp.Periods):
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
        t, bounds, labels = pp.resolve_periods(times, period, who)
        if climatology is not None:
            if t is None or slot is not None:
                raise ValueError(f"{who}: a climatology takes its slots from times: pass times and no slot")
            if thresholds is None:
                thresholds = climatology.quantile_thresholds()
            slot = climatology.slots(t)
        if thresholds is None:
            raise ValueError(f"{who}: no thresholds (and no climatology with quantiles to take them from)")
        kern = _kern(kern)
        planes = spell_blocks(pp.checked_blocks(Xblocks, t, who), thresholds, bounds, min_length, above, slot, kern)
        if not planes:
            raise ValueError(f"{who}: no blocks")
        J = int(planes[0].shape[0])
        return cls(planes, bounds, labels, _per_threshold(min_length, J, int, who, "min_length"),
                   _per_threshold(above, J, bool, who, "above"), t, kern)

    # -- the indices ------------------------------------------------------------------------------------------------
    @property
    def n_thresholds(self) -> int:
        return len(self.min_length)

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
        return [pp.ratio(Q[:, 1].to(torch.float64), Q[:, 0].to(torch.float64)) for Q in self.planes]

    def spell_count(self) -> list:
        """The runs of at least ``min_length`` events, (J, P, rows) int32."""
        return self._plane("n_spell")

    def spell_days(self) -> list:
        """The snapshots in runs of at least ``min_length`` events (WSDI / CSDI in snapshots), (J, P, rows) int32."""
        return self._plane("n_in_spell")

    def longest(self) -> list:
        """The longest run of events, qualifying or not (CDD / CWD in snapshots); 0 where there is none."""
        return self._plane("longest")

    def _offsets(self, name: str, as_time: bool, who: str) -> list:
        return self._when(self._plane(name), 1, who) if as_time else self._plane(name)

    def onset(self, as_time: bool = False) -> list:
        """Where the first qualifying run of the period starts: the offset from the period's first snapshot, (J, P,
        rows) int32, -1 where there is none; ``as_time``: the stamps instead (numpy datetime64, NaT where none)."""
        return self._offsets("first", as_time, "onset")

    def end(self, as_time: bool = False) -> list:
        """Where the last qualifying run of the period ends (its last snapshot), as :meth:`onset`."""
        return self._offsets("last", as_time, "end")

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
        values = getattr(self, index)()
        extra = (lambda v: v >= 0) if index in ("onset", "end") else None
        return pp.area_mean_sums(self.n_valid(), values, extra, weights, groups, n_groups, comm, "spell_allreduce", who)

    # -- persistence ----------------------------------------------------------------------------------------------
    def to_dataset(self, coords=None) -> Dataset:
        """``spell_planes(plane, space)`` int32 with plane = (j 7 + q) P + p, ``period_bound(bound)``,
        ``min_length(threshold)``, ``above(threshold)``, the stamps as ``time_s`` / ``time_ns(time_index)`` (whole
        seconds since 1970 and the nanoseconds beyond; absent without times) and the attribute ``period_labels``
        (the labels joined by commas); ``coords``: the per-row coordinates of the decomposed array, taken over as they
        are.  ``io_netcdf.to_netcdf`` writes it."""
        return pp.to_dataset("spell_planes", self.planes, np.int32, self.bounds, self.labels, self.times, coords, "threshold",
                             {"min_length": self.min_length, "above": self.above})

    @classmethod
    def from_dataset(cls, ds: Dataset, rows=None, device=None, kern=None) -> "SpellStats":
        """The statistics :meth:`to_dataset` stored (``io_netcdf.open_dataset`` of its file).  ``rows``: the row counts
        of the blocks to cut the planes into (default: one block); ``device``: where they go (default: the GPU for
        the HIP provider)."""
        who = "SpellStats.from_dataset"
        kern = _kern(kern)
        field, bounds, labels, times = pp.from_dataset(ds, "spell_planes", np.int32)
        ml = tuple(int(v) for v in np.asarray(ds["min_length"].values).reshape(-1))
        ab = tuple(bool(v) for v in np.asarray(ds["above"].values).reshape(-1))
        J, P = len(ml), int(bounds.shape[0]) - 1
        if field.shape[0] != J * len(PLANES) * P or len(ab) != J:
            raise ValueError(f"{who}: spell_planes holds {field.shape[0]} planes, {J} thresholds and {P} periods ask for "
                             f"{J * len(PLANES) * P}")
        flat = ta.cut_rows(field, rows, device, kern, who)
        return cls([F.reshape(J, len(PLANES), P, -1) for F in flat], bounds, labels, ml, ab, times, kern)
