"""Per-grid-point trend and harmonic regression of the snapshots, fitted and removed on the device (K21,
csrc/treg.hip).

The slot climatology (K18, :mod:`climatology`) takes out what repeats with the calendar.  What a multi-year ERA5
slice holds besides is a secular trend: left in the snapshot matrix it costs the DMD a near-zero eigenvalue pair,
tilts the other modes and inflates the anomaly correlation of a forecast verified against a stationary climatology.
This module regresses every grid point on a small temporal design matrix -- an intercept, a polynomial trend, annual
and diurnal harmonics, user series such as an ENSO index; p <= 8 columns -- by least squares.  The host forms the
design ``D`` (T, p) and ``W = (D^T D)^-1 D^T`` in fp64 (:func:`design`, :func:`weights`: pure numpy); the device
forms the coefficients in one read of the resident ``(time, rows)`` blocks (``HipKernels.treg_fit``) and removes or
restores the fitted part in one read and one write (``treg_apply_``): no fp64 copy of X, no stored trend field.

    trend = Trend.fit(Xblocks, times, degree=1, harmonics=2)    # (p, rows) coefficients per block
    trend.slope()                                               # the trend map, units per decade
    trend.remove_(Xblocks, times)                               # X <- X - D(t) coef, in place
    fields = forecast.fields(t, trend=trend, times=valid)       # the model's detrended anomalies back to full fields

With a climatology the order is: climatology out, then the trend; back in reverse.  Rows are independent: row shards
fit and apply their own blocks, no collective is involved.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _timeaxis as ta
from .labeled import Coord, DataArray, Dataset
from .svd import _kern

__all__ = ["SEGMENT", "MAX_TERMS", "MAX_COND", "design", "weights", "Trend"]

# the segment length of the fp64 sums of the fit: part of the arithmetic contract (a result does not depend on how
# a launch was cut), so one constant and never tuned per launch
SEGMENT = 1024
MAX_TERMS = 8
MAX_COND = 1e8
_NS_PER_DAY = 86400.0e9


def _extra(extra, T: int, who: str) -> np.ndarray:
    if extra is None:
        return np.zeros((T, 0), dtype=np.float64)
    e = np.asarray(extra, dtype=np.float64)
    e = e.reshape(-1, 1) if e.ndim == 1 else e
    if e.ndim != 2 or e.shape[0] != T:
        raise ValueError(f"{who}: extra must hold one row per time stamp ({T}), got {np.asarray(extra).shape}")
    return e


def design(times, origin, half_span_days: float, degree: int = 1, harmonics: int = 0, diurnal: int = 0,
           period_days: float = 365.2425, extra=None) -> np.ndarray:
    """The (T, p) fp64 design matrix of the datetime64 stamps ``times``.  Columns, in this order: ``1``;
    ``tau, ..., tau^degree`` with ``tau = (t - origin) / half_span_days`` (-1 .. 1 over the fitted period); the annual
    ``cos, sin`` of ``2 pi h days / period_days`` for h = 1 .. ``harmonics``, ``days`` the days since ``origin``; the
    daily ``cos, sin`` of ``2 pi h days`` for h = 1 .. ``diurnal``; the columns of ``extra`` ((T,) or (T, q): user
    series, an ENSO index).  At most 8 columns."""
    t = ta.stamps(times, "design").astype("datetime64[ns]")
    degree, harmonics, diurnal = int(degree), int(harmonics), int(diurnal)
    if degree < 0 or harmonics < 0 or diurnal < 0:
        raise ValueError(f"design: degree = {degree}, harmonics = {harmonics}, diurnal = {diurnal} must be >= 0")
    if not float(half_span_days) > 0.0 or not float(period_days) > 0.0:
        raise ValueError(f"design: half_span_days = {half_span_days} and period_days = {period_days} must be > 0")
    T = int(t.shape[0])
    ex = _extra(extra, T, "design")
    p = 1 + degree + 2 * harmonics + 2 * diurnal + ex.shape[1]
    if p > MAX_TERMS:
        raise ValueError(f"design: {p} columns (1 + degree {degree} + 2 x {harmonics} annual + 2 x {diurnal} daily + "
                         f"{ex.shape[1]} extra), at most {MAX_TERMS}")
    days = (t - np.datetime64(origin, "ns")).astype(np.int64).astype(np.float64) / _NS_PER_DAY
    tau = days / float(half_span_days)
    cols = [np.ones(T, dtype=np.float64)]
    cols += [tau ** q for q in range(1, degree + 1)]
    for h, per in [(h, float(period_days)) for h in range(1, harmonics + 1)] + [(h, 1.0) for h in range(1, diurnal + 1)]:
        ang = 2.0 * np.pi * h * days / per
        cols += [np.cos(ang), np.sin(ang)]
    return np.ascontiguousarray(np.concatenate([np.stack(cols, axis=1), ex], axis=1))


def weights(D: np.ndarray) -> np.ndarray:
    """``W = (D^T D)^-1 D^T`` (p, T) fp64 of a (T, p) design through its QR factorisation: ``R W = Q^T``.  A design
    with ``cond(D) > 1e8`` (or fewer snapshots than columns) is a ValueError."""
    D = np.asarray(D, dtype=np.float64)
    T, p = D.shape
    cond = np.linalg.cond(D) if T >= p else np.inf
    if not cond <= MAX_COND:
        raise ValueError(f"trend: the design of {T} snapshots and {p} columns has condition number {cond:.3g} > "
                         f"{MAX_COND:g}: its columns are not independent over these times")
    Q, R = np.linalg.qr(D)
    return np.ascontiguousarray(np.linalg.solve(R, Q.T))


@dataclass
class Trend:
    """The regression of a list of row blocks on a temporal design: ``coef`` holds one ``(p, rows)`` fp32 tensor per
    block, the other fields are what :func:`design` needs to form the columns at any time."""

    origin: np.datetime64
    half_span_days: float
    degree: int
    harmonics: int
    diurnal: int
    period_days: float
    n_extra: int
    coef: list
    kern: object = None

    @property
    def n_terms(self) -> int:
        return 1 + self.degree + 2 * self.harmonics + 2 * self.diurnal + self.n_extra

    def design(self, times, extra=None, who: str = "design") -> np.ndarray:
        """The model's design at ``times`` -- any times, after the fitted period included."""
        T = int(np.atleast_1d(np.asarray(times)).shape[0])
        given = 0 if extra is None else int(_extra(extra, T, f"Trend.{who}").shape[1])
        if given != self.n_extra:
            raise ValueError(f"Trend.{who}: the model was fitted with {self.n_extra} extra series, extra holds {given}: "
                             "pass the same series at these times")
        return design(times, self.origin, self.half_span_days, self.degree, self.harmonics, self.diurnal, self.period_days,
                      extra)

    # -- fit ------------------------------------------------------------------------------------------------------
    @classmethod
    def fit(cls, Xblocks, times, degree: int = 1, harmonics: int = 0, diurnal: int = 0, extra=None,
            period_days: float = 365.2425, kern=None) -> "Trend":
        """Least squares of the snapshots ``Xblocks`` ((T, rows) fp32 per block, any iterable consumed once) taken at
        ``times`` (T datetime64 stamps, evenly spaced or not) on :func:`design` with ``origin`` the mid-point of the
        fitted period and ``half_span_days`` half its length: one read of every block.  A design whose condition
        number exceeds 1e8 is a ValueError before any launch."""
        t = ta.stamps(times, "Trend.fit").astype("datetime64[ns]")
        T = int(t.shape[0])
        if T < 1:
            raise ValueError("Trend.fit: no time stamps")
        lo, hi = t.min(), t.max()
        origin = lo + (hi - lo) // 2
        half = float((hi - origin).astype(np.int64)) / _NS_PER_DAY
        half = half if half > 0.0 else 1.0
        ex = _extra(extra, T, "Trend.fit")
        D = design(t, origin, half, degree, harmonics, diurnal, period_days, extra)
        W = ta.OnDevices(weights(D))
        kern = _kern(kern)
        coef = []
        for b, X in enumerate(Xblocks):
            if X.shape[0] != T:
                raise ValueError(f"Trend.fit: block {b} holds {int(X.shape[0])} snapshots, times has {T}")
            coef.append(kern.treg_fit(X, W.on(X.device), SEGMENT))
        return cls(origin, half, int(degree), int(harmonics), int(diurnal), float(period_days), int(ex.shape[1]), coef, kern)

    # -- apply ----------------------------------------------------------------------------------------------------
    def _apply(self, Xblocks, times, extra, out, restore: bool, who: str) -> list:
        D = ta.OnDevices(self.design(times, extra, who))            # (raises before any launch)
        T = int(D.host.shape[0])
        Xblocks = list(Xblocks)
        if len(Xblocks) != len(self.coef):
            raise ValueError(f"Trend.{who}: {len(Xblocks)} blocks, the trend holds {len(self.coef)}")
        for b, X in enumerate(Xblocks):
            if tuple(X.shape) != (T, int(self.coef[b].shape[1])):
                raise ValueError(f"Trend.{who}: block {b} is {tuple(X.shape)}, {T} times and "
                                 f"{int(self.coef[b].shape[1])} rows asked for")
        kern = _kern(self.kern)
        return [kern.treg_apply_(X, D.on(X.device), self.coef[b], restore=restore, out=None if out is None else out[b])
                for b, X in enumerate(Xblocks)]

    def remove_(self, Xblocks, times, out=None, extra=None) -> list:
        """``X <- fp32(fp64(X) - D(t) coef)`` for the snapshots taken at ``times``, one launch per block; in place, or
        into the list ``out`` of (T, rows) fp32 views that do not overlap X.  A model fitted with ``extra`` needs the
        series at these times again."""
        return self._apply(Xblocks, times, extra, out, False, "remove_")

    def restore_(self, Xblocks, times, out=None, extra=None) -> list:
        """The inverse of :meth:`remove_`: ``X <- fp32(fp64(X) + D(t) coef)``; no exact round trip is promised."""
        return self._apply(Xblocks, times, extra, out, True, "restore_")

    def at(self, times, extra=None) -> list:
        """The fitted fields at ``times`` -- inside or after the fitted period: per block a (T, rows) fp32 tensor,
        restore on zeros."""
        T = int(np.atleast_1d(np.asarray(times)).shape[0])
        Z = [torch.zeros((T, int(C.shape[1])), dtype=torch.float32, device=C.device) for C in self.coef]
        return self._apply(Z, times, extra, None, True, "at")

    def slope(self, per_days: float = 3652.425) -> list:
        """The trend map: per block a (rows,) fp64 tensor, the coefficient of ``tau`` in the units of the data per
        ``per_days`` days (default: per decade).  With ``degree`` > 1 this is the slope at the mid-point."""
        if self.degree < 1:
            raise ValueError("Trend.slope: the model has no linear term (degree = 0)")
        return [C[1].to(torch.float64) * (float(per_days) / self.half_span_days) for C in self.coef]

    # -- persistence ----------------------------------------------------------------------------------------------
    def to_dataset(self, coords=None) -> Dataset:
        """``trend_coef(term, space)`` and, as attributes, every parameter of the design: ``origin`` (ISO, ns),
        ``half_span_days`` and ``period_days`` (``repr`` of the fp64: an exact round trip), ``degree``, ``harmonics``,
        ``diurnal``, ``n_extra``; ``coords``: the per-row coordinates of the decomposed array, taken over as they
        are.  ``io_netcdf.to_netcdf`` writes it."""
        cds = {"term": Coord("term", np.arange(self.n_terms, dtype=np.int64)), **ta.row_coords(coords)}
        ds = Dataset(coords=cds, attrs={
            "origin": str(np.datetime64(self.origin, "ns")), "half_span_days": repr(float(self.half_span_days)),
            "period_days": repr(float(self.period_days)), "degree": int(self.degree), "harmonics": int(self.harmonics),
            "diurnal": int(self.diurnal), "n_extra": int(self.n_extra)})
        row = {k: v for k, v in cds.items() if k != "term"}
        field = np.concatenate([C.detach().cpu().numpy() for C in self.coef], axis=1)
        ds["trend_coef"] = DataArray(field, ("term", "space"), {"term": cds["term"], **row})
        return ds

    @classmethod
    def from_dataset(cls, ds: Dataset, rows=None, device=None, kern=None) -> "Trend":
        """The trend :meth:`to_dataset` stored (``io_netcdf.open_dataset`` of its file).  ``rows``: the row counts of
        the blocks to cut the coefficients into (default: one block); ``device``: where they go (default: the GPU for
        the HIP provider)."""
        kern = _kern(kern)
        coef = np.ascontiguousarray(np.asarray(ds["trend_coef"].values), dtype=np.float32)
        p = coef.shape[0]
        blocks = ta.cut_rows(coef, rows, device, kern, "Trend.from_dataset")
        a = ds.attrs
        res = cls(np.datetime64(ta.attr_str(a["origin"]), "ns"), float(ta.attr_str(a["half_span_days"])),
                  ta.attr_int(a["degree"]), ta.attr_int(a["harmonics"]), ta.attr_int(a["diurnal"]),
                  float(ta.attr_str(a["period_days"])), ta.attr_int(a["n_extra"]), blocks, kern)
        if res.n_terms != p:
            raise ValueError(f"Trend.from_dataset: trend_coef holds {p} terms, the attributes describe {res.n_terms}")
        return res
