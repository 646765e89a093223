"""Temporal FIR filtering and decimation of the snapshots on the device (K22, csrc/tfilt.hip).

ERA5 is hourly; what a DMD of the climate is fitted to are daily means or low-pass / band-pass filtered fields.  Taking
every n-th snapshot (``nearest_resample_index``, ``tstep``) aliases everything above the new Nyquist frequency into
the band that is kept; a filter along time followed by decimation does not.  This module designs the taps on the host
in fp64 (:func:`boxcar`, :func:`lanczos_lowpass`, :func:`lanczos_bandpass`, :func:`response`: pure numpy) and applies
them to the resident ``(time, rows)`` blocks with ``HipKernels.tfilt``: a weighted sum over a sliding window of
snapshots with an output stride, valid windows only, one read of X and no fp64 copy.

    tf = TimeFilter.block_mean(times)                           # hourly -> daily means, stamped with the day
    tf = TimeFilter.lowpass(times, cutoff_days=10.0, every_days=1.0)
    Yblocks, times_out = tf.apply(Xblocks, times)               # (T_out, rows) fp32 per block

The filter is the first step of the chain: ingest, filter / decimate, climatology, trend, SVD.  Its output is again a
list of ``(T_out, rows)`` fp32 blocks that ``Climatology.fit``, ``Trend.fit`` and the SVD take as they are.  Rows are
independent: row shards filter their own blocks, no collective is involved.  A window that holds a NaN gives a NaN.
"""
from __future__ import annotations

import math

import numpy as np

from . import _timeaxis as ta
from .labeled import Coord, DataArray, Dataset
from .svd import _kern

__all__ = ["LABELS", "boxcar", "lanczos_lowpass", "lanczos_bandpass", "response", "TimeFilter"]

LABELS = ("center", "left")
_NS_PER_DAY = 86400 * 10**9


# ---- tap design ---------------------------------------------------------------------------------------------------
def boxcar(L: int) -> np.ndarray:
    """The running mean: L taps of ``1 / L``."""
    L = int(L)
    if L < 1:
        raise ValueError(f"boxcar: L = {L} < 1")
    return np.full(L, 1.0 / L, dtype=np.float64)


def lanczos_lowpass(cutoff: float, half_width: int) -> np.ndarray:
    """The Lanczos low-pass of Duchon (1979): ``w_k = sin(2 pi f_c k) / (pi k) * sinc(k / n)`` for ``|k| <= n``,
    ``w_0 = 2 f_c``, divided by their sum.  ``cutoff`` = f_c in cycles per step (0 < f_c < 0.5), ``half_width`` = n:
    ``L = 2 n + 1`` taps, symmetric to the bit.  The transition band is ``f_c -+ 1 / n`` wide: with ``f_c n = 2`` the
    response is within 1 % of 1 below it, below 1 % above it and 1 / 2 at f_c."""
    fc, n = float(cutoff), int(half_width)
    if not 0.0 < fc < 0.5:
        raise ValueError(f"lanczos_lowpass: cutoff = {cutoff} cycles per step outside (0, 0.5)")
    if n < 1:
        raise ValueError(f"lanczos_lowpass: half_width = {half_width} < 1")
    k = np.arange(1, n + 1, dtype=np.float64)
    side = np.sin(2.0 * np.pi * fc * k) / (np.pi * k) * np.sinc(k / n)
    w = np.concatenate([side[::-1], [2.0 * fc], side])
    return w / math.fsum(w)


def lanczos_bandpass(f_low: float, f_high: float, half_width: int) -> np.ndarray:
    """The difference of the two Lanczos low-passes of the same width with cut-offs ``f_high`` and ``f_low`` (cycles
    per step, ``f_low < f_high``): passes the band between them, sums to zero."""
    if not float(f_low) < float(f_high):
        raise ValueError(f"lanczos_bandpass: f_low = {f_low} must be below f_high = {f_high}")
    return lanczos_lowpass(f_high, half_width) - lanczos_lowpass(f_low, half_width)


def response(taps, freq) -> np.ndarray:
    """The amplitude response ``|sum over j of h[j] exp(-2 pi i f j)|`` of the taps at ``freq`` (cycles per step; a
    scalar or an array).  At f = 0 this is the absolute value of ``numpy.sum(taps)``."""
    h = np.asarray(taps, dtype=np.float64).reshape(-1)
    f = np.asarray(freq, dtype=np.float64)
    j = np.arange(h.shape[0], dtype=np.float64) - 0.5 * (h.shape[0] - 1)          # centred: the modulus is the same
    out = np.empty(f.size, dtype=np.float64)
    for q, fq in enumerate(f.reshape(-1)):
        ang = 2.0 * np.pi * fq * j
        out[q] = math.hypot(np.sum(h * np.cos(ang)), np.sum(h * np.sin(ang)))
    return out.reshape(f.shape)


# ---- time stamps ----------------------------------------------------------------------------------------------------
def _even_stamps(times, who: str) -> tuple[np.ndarray, int]:
    """-> (the stamps as datetime64[ns], their step in ns); anything but evenly spaced datetime64 is a ValueError."""
    t = ta.stamps(times, who).astype("datetime64[ns]")
    if t.shape[0] < 2:
        return t, 0
    d = np.diff(t.astype(np.int64))
    if d[0] <= 0 or (d != d[0]).any():
        raise ValueError(f"{who}: times must be evenly spaced and ascending (a filter along time has one step)")
    return t, int(d[0])


def _steps(days: float, step_ns: int, who: str, what: str) -> int:
    """`days` as a whole number >= 1 of steps."""
    ns = int(round(float(days) * _NS_PER_DAY))
    if step_ns <= 0:
        raise ValueError(f"{who}: at least two time stamps are needed to know the step")
    if ns < step_ns or ns % step_ns:
        raise ValueError(f"{who}: the step of the stamps ({step_ns / _NS_PER_DAY:g} days) does not divide {what} = {days:g} days")
    return ns // step_ns


class TimeFilter:
    """``taps`` (L fp64 weights, applied to snapshots u stride .. u stride + L - 1 in this order) with an output
    ``stride`` and the ``label`` of an output: ``"center"`` -- the stamp of the window's centre tap, L odd -- or
    ``"left"`` -- the window's first stamp, what a daily mean is labelled with."""

    def __init__(self, taps, stride: int = 1, label: str = "center", kern=None):
        h = np.ascontiguousarray(np.asarray(taps, dtype=np.float64))
        if h.ndim != 1 or h.shape[0] < 1 or not np.isfinite(h).all():
            raise ValueError(f"TimeFilter: taps must be a one-dimensional array of L >= 1 finite weights, got {h.shape}")
        if int(stride) < 1:
            raise ValueError(f"TimeFilter: stride = {stride} < 1")
        if label not in LABELS:
            raise ValueError(f"TimeFilter: label = {label!r}, one of {LABELS}")
        if label == "center" and h.shape[0] % 2 == 0:
            raise ValueError(f"TimeFilter: label = 'center' needs an odd number of taps, got {h.shape[0]} (label = 'left' "
                             "stamps a window with its first snapshot)")
        self.taps, self.stride, self.label, self.kern = h, int(stride), label, kern

    @property
    def n_taps(self) -> int:
        return int(self.taps.shape[0])

    def response(self, freq) -> np.ndarray:
        return response(self.taps, freq)

    def n_out(self, T: int) -> int:
        """The number of valid windows in T snapshots; fewer snapshots than taps is a ValueError."""
        T = int(T)
        if T < self.n_taps:
            raise ValueError(f"TimeFilter: {T} snapshots are fewer than the {self.n_taps} taps of one window")
        return (T - self.n_taps) // self.stride + 1

    def times_out(self, times) -> np.ndarray:
        """The stamps of the outputs for the evenly spaced datetime64 stamps ``times`` of the snapshots."""
        t, _ = _even_stamps(times, "TimeFilter.times_out")
        n = self.n_out(t.shape[0])
        first = (self.n_taps - 1) // 2 if self.label == "center" else 0
        return t[first + self.stride * np.arange(n, dtype=np.int64)]

    # -- apply ----------------------------------------------------------------------------------------------------
    def apply(self, Xblocks, times=None, out=None):
        """The filtered and decimated blocks: per (T, rows) fp32 block of ``Xblocks`` one launch and one
        ``(T_out, rows)`` fp32 tensor -- fresh, or the view ``out[b]`` (inner stride 1, not overlapping the block).
        -> (Yblocks, the stamps of the outputs or None without ``times``).  Everything is checked before the first
        launch; the taps are uploaded once per device."""
        Xblocks = list(Xblocks)
        t_out = None if times is None else self.times_out(times)
        T = None if times is None else int(np.atleast_1d(np.asarray(times)).shape[0])
        for b, X in enumerate(Xblocks):
            if X.dim() != 2:
                raise ValueError(f"TimeFilter.apply: block {b} must be (time, rows), got {tuple(X.shape)}")
            T = int(X.shape[0]) if T is None else T
            if int(X.shape[0]) != T:
                raise ValueError(f"TimeFilter.apply: block {b} holds {int(X.shape[0])} snapshots, {T} asked for")
        n = self.n_out(T) if T is not None else 0
        if out is not None:
            out = list(out)
            if len(out) != len(Xblocks):
                raise ValueError(f"TimeFilter.apply: {len(Xblocks)} blocks, out holds {len(out)}")
            for b, (X, Y) in enumerate(zip(Xblocks, out)):
                if tuple(Y.shape) != (n, int(X.shape[1])):
                    raise ValueError(f"TimeFilter.apply: out[{b}] is {tuple(Y.shape)}, ({n}, {int(X.shape[1])}) asked for")
        kern = _kern(self.kern)
        h = ta.OnDevices(self.taps)
        res = [kern.tfilt(X, h.on(X.device), self.stride, out=None if out is None else out[b])
               for b, X in enumerate(Xblocks)]
        return res, t_out

    # -- constructors in physical units ---------------------------------------------------------------------------
    @classmethod
    def block_mean(cls, times, days: float = 1.0, kern=None) -> "TimeFilter":
        """Means over consecutive periods of ``days`` days (L = stride = the steps of one period), stamped with the
        start of the period.  The step of ``times`` must divide the period and ``times[0]`` must lie on a period
        boundary (counted from 1970-01-01T00): a daily mean starts at midnight."""
        t, step = _even_stamps(times, "TimeFilter.block_mean")
        L = _steps(days, step, "TimeFilter.block_mean", "the period")
        if int(t[0].astype(np.int64)) % (L * step):
            raise ValueError(f"TimeFilter.block_mean: times[0] = {t[0]} is not on a boundary of the {days:g}-day periods: "
                             "cut the snapshots before it")
        return cls(boxcar(L), L, "left", kern)

    @classmethod
    def _lanczos(cls, who, times, short_days, long_days, width_days, every_days, kern):
        """long_days None: the low-pass at short_days; else the band between the two."""
        _, step = _even_stamps(times, who)
        slow = short_days if long_days is None else long_days
        if not 0.0 < float(short_days) <= float(slow):
            raise ValueError(f"{who}: periods of {short_days:g} and {slow:g} days: positive and short <= long asked for")
        n = _steps(2.0 * float(slow) if width_days is None else width_days, step, who, "the half width")
        stride = 1
        if every_days is not None:
            if float(every_days) > float(short_days) / 2.0:
                raise ValueError(f"{who}: every_days = {every_days:g} > {short_days:g} / 2: the decimated series must keep the "
                                 "pass band below its Nyquist frequency, or what the filter kept is aliased")
            stride = _steps(every_days, step, who, "every_days")
        f_hi = step / (float(short_days) * _NS_PER_DAY)
        if long_days is None:
            return cls(lanczos_lowpass(f_hi, n), stride, "center", kern)
        return cls(lanczos_bandpass(step / (float(long_days) * _NS_PER_DAY), f_hi, n), stride, "center", kern)

    @classmethod
    def lowpass(cls, times, cutoff_days: float, width_days: float | None = None, every_days: float | None = None,
                kern=None) -> "TimeFilter":
        """The Lanczos low-pass with its half-power point at periods of ``cutoff_days``; ``width_days`` per side
        (default ``2 cutoff_days``: f_c n = 2); ``every_days``: the spacing of the outputs, at most
        ``cutoff_days / 2``."""
        return cls._lanczos("TimeFilter.lowpass", times, cutoff_days, None, width_days, every_days, kern)

    @classmethod
    def bandpass(cls, times, short_days: float, long_days: float, width_days: float | None = None,
                 every_days: float | None = None, kern=None) -> "TimeFilter":
        """The Lanczos band-pass for periods between ``short_days`` and ``long_days`` (20 and 100: the intraseasonal
        band); ``width_days`` per side (default ``2 long_days``); ``every_days`` at most ``short_days / 2``."""
        return cls._lanczos("TimeFilter.bandpass", times, short_days, long_days, width_days, every_days, kern)

    # -- persistence ----------------------------------------------------------------------------------------------
    def to_dataset(self) -> Dataset:
        """``filter_taps(tap)`` fp64 with ``stride`` and ``label`` as attributes; ``io_netcdf.to_netcdf`` writes it."""
        tap = Coord("tap", np.arange(self.n_taps, dtype=np.int64))
        ds = Dataset(coords={"tap": tap}, attrs={"stride": int(self.stride), "label": str(self.label)})
        ds["filter_taps"] = DataArray(self.taps.copy(), ("tap",), {"tap": tap})
        return ds

    @classmethod
    def from_dataset(cls, ds: Dataset, kern=None) -> "TimeFilter":
        """The filter :meth:`to_dataset` stored (``io_netcdf.open_dataset`` of its file): the taps bit for bit."""
        taps = np.asarray(ds["filter_taps"].values, dtype=np.float64)
        return cls(taps, ta.attr_int(ds.attrs["stride"]), ta.attr_str(ds.attrs["label"]), kern)
