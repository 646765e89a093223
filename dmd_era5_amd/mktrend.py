"""The Mann-Kendall test and the Theil-Sen slope per grid point (K32, csrc/mktrend.hip): the trend of an index series as
it is reported.

:mod:`spells` and :mod:`extremes` give the standard indices as one value per year and grid point.  Annual maxima, wet-day
totals and spell lengths are skewed, full of ties and often partly missing, so their trend is not the least-squares line
of :mod:`trend` but the median of all pairwise slopes (Theil-Sen), with a rank-based confidence interval, and its
significance the Mann-Kendall test.  Per block the device forms the integer statistics of the test in one read
(``HipKernels.mk_stats``) and selects four order statistics of the N = v (v - 1) / 2 pairwise slopes of every row without
storing or sorting them (``HipKernels.sen_slopes``); the handful of fp64 operations between the two run in torch on the
``(rows,)`` vectors of the block.

    tx = PeriodStats.fit(Xblocks, times, period="year", group=g, inner="max")
    mk = MannKendall.fit(tx.series("maximum"), tx.period_years(), alpha=0.05)     # (P, rows) blocks
    mk.slope(per=10.0); mk.slope_interval(); mk.p_value(); mk.significant(fdr=True)

A point that is not finite is missing; the pairs are those of the valid points of a row.  The ranks of the interval are
those of ``scipy.stats.theilslopes``; a row with fewer than two valid points has NaN slopes.

Out of scope: the intercept; the seasonal Mann-Kendall test; pre-whitening (``variance_scale`` takes n / n_eff of
``LagStats.effective_sample_size`` instead); the false discovery rate across row shards (with a ``comm`` the caller
gathers the p-values and calls :func:`fdr_threshold`); series longer than 128 points (``Trend.fit``).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from statistics import NormalDist

import numpy as np
import torch

from . import _timeaxis as ta
from .labeled import Coord, DataArray, Dataset
from .svd import _kern

__all__ = ["PLANES", "RANKS", "MAX_POINTS", "mk_blocks", "sen_blocks", "interval_ranks", "fdr_threshold", "MannKendall"]

PLANES = ("n", "s", "ties", "tie_term")                 # the planes of HipKernels.mk_stats
RANKS = ("median_low", "median_high", "lower", "upper")  # the order statistics a fit asks sen_slopes for
MAX_POINTS = 128                                        # DMDX_MK_MAX_N; checked against the provider's mk_max_n
_DAY_NS = 86_400 * 10**9


def _coordinate(coord, who: str) -> np.ndarray:
    """``coord`` as n finite, strictly ascending fp64 numbers; datetime64 stamps become days since the first."""
    c = np.atleast_1d(np.asarray(coord))
    if c.ndim != 1 or c.shape[0] < 1:
        raise ValueError(f"{who}: coord must be a one-dimensional list of time coordinates, got {c.shape}")
    if np.issubdtype(c.dtype, np.datetime64):
        ns = ta.stamps(c, who).astype("datetime64[ns]").astype(np.int64)
        c = (ns - ns[0]) / _DAY_NS
    c = c.astype(np.float64)
    if not np.isfinite(c).all() or not (np.diff(c) > 0).all():
        raise ValueError(f"{who}: coord must be finite and strictly ascending")
    if c.shape[0] > MAX_POINTS:
        raise ValueError(f"{who}: {c.shape[0]} time points, at most {MAX_POINTS} asked for: the pairwise slopes of a "
                         f"longer series are not formed; Trend.fit takes any length")
    return c


def _provider(kern, who: str):
    kern = _kern(kern)
    if int(kern.mk_max_n) != MAX_POINTS:
        raise RuntimeError(f"{who}: the kernels take {int(kern.mk_max_n)} time points, this module {MAX_POINTS}")
    return kern


def _checked(Yblocks, n: int | None, who: str):
    for b, Y in enumerate(Yblocks):
        if Y.dim() != 2:
            raise ValueError(f"{who}: block {b} is {tuple(Y.shape)}, a (time points, rows) block asked for")
        if n is not None and int(Y.shape[0]) != n:
            raise ValueError(f"{who}: block {b} is {tuple(Y.shape)}, coord has {n} time points")
        if int(Y.shape[0]) > MAX_POINTS:
            raise ValueError(f"{who}: block {b} holds {int(Y.shape[0])} time points, at most {MAX_POINTS} asked for; "
                             f"Trend.fit takes any length")
        yield Y


def mk_blocks(Yblocks, kern=None) -> list:
    """The planes of ``HipKernels.mk_stats`` for every block of ``Yblocks`` ((n, rows) fp32 per block): per block a
    (4, rows) int32 tensor in the order of :data:`PLANES`."""
    kern = _provider(kern, "mk_blocks")
    return [kern.mk_stats(Y) for Y in _checked(Yblocks, None, "mk_blocks")]


def sen_blocks(Yblocks, coord, ranks, kern=None) -> list:
    """``HipKernels.sen_slopes`` for every block: ``ranks`` per block a (J, rows) int32 tensor -> (J, rows) fp32."""
    who = "sen_blocks"
    kern = _provider(kern, who)
    c = _coordinate(coord, who)
    Yblocks, ranks = list(Yblocks), list(ranks)
    if len(ranks) != len(Yblocks):
        raise ValueError(f"{who}: {len(ranks)} rank tables for {len(Yblocks)} blocks")
    return [kern.sen_slopes(Y, c, r) for Y, r in zip(_checked(Yblocks, c.shape[0], who), ranks)]


def _pairs(stats: torch.Tensor) -> torch.Tensor:
    v = stats[0].to(torch.int64)
    return v * (v - 1) // 2


def _variance(stats: torch.Tensor, scale) -> torch.Tensor:
    """Var(S) = (v (v - 1) (2 v + 5) - G) / 18, times ``scale``; fp64, the integers exact."""
    v = stats[0].to(torch.int64)
    num = (v * (v - 1) * (2 * v + 5) - stats[3].to(torch.int64)).to(torch.float64)
    var = num / torch.full_like(num, 18.0)     # (a tensor: a device divides by a number as a product with 1 / 18)
    return var if scale is None else var * scale


def interval_ranks(stats: torch.Tensor, alpha: float, variance_scale=None) -> torch.Tensor:
    """The four ranks of :data:`RANKS` a fit asks ``sen_slopes`` for, (4, rows) int32, from the (4, rows) planes of
    ``mk_stats``: the two middle ones, and for the 1 - ``alpha`` interval those of ``scipy.stats.theilslopes`` --
    ``max(round((N - z sigma) / 2) - 1, 0)`` and ``min(round((N + z sigma) / 2), N - 1)``, round half to even, with
    sigma^2 = Var(S) times ``variance_scale`` ((rows,) fp64 or None).  A NaN variance gives ranks outside every row
    (NaN slopes)."""
    z = -NormalDist().inv_cdf(float(alpha) / 2.0)
    N = _pairs(stats)
    Nf, zs = N.to(torch.float64), z * torch.sqrt(_variance(stats, variance_scale))
    lo = torch.clamp(torch.round((Nf - zs) / 2.0) - 1.0, min=0.0)
    hi = torch.minimum(torch.round((Nf + zs) / 2.0), Nf - 1.0)
    bad = torch.isnan(zs)
    lo = torch.where(bad, torch.full_like(lo, -1.0), lo)
    hi = torch.where(bad, torch.full_like(hi, -1.0), hi)
    return torch.stack([torch.div(N - 1, 2, rounding_mode="floor"), torch.div(N, 2, rounding_mode="floor"),
                        lo.to(torch.int64), hi.to(torch.int64)]).to(torch.int32)


def fdr_threshold(p_blocks, alpha: float) -> float:
    """Benjamini-Hochberg: the largest p_(i) with p_(i) <= (i / M) alpha over all M non-NaN p-values of the blocks of
    this process, 0.0 if there is none.  A test is significant at the false discovery rate alpha iff p <= this."""
    p = torch.cat([torch.as_tensor(b).detach().reshape(-1).to(device="cpu", dtype=torch.float64) for b in p_blocks]) \
        if len(p_blocks) else torch.zeros(0, dtype=torch.float64)
    p = torch.sort(p[~torch.isnan(p)]).values
    M = int(p.numel())
    if M == 0:
        return 0.0
    ok = p <= torch.arange(1, M + 1, dtype=torch.float64) / M * float(alpha)
    return float(p[ok].max()) if bool(ok.any()) else 0.0


@dataclass
class MannKendall:
    """The rank-based trend of a list of series blocks: ``stats`` holds one (4, rows) int32 tensor per block
    (:data:`PLANES`), ``slopes`` one (4, rows) fp32 tensor (:data:`RANKS`), ``coord`` the n time coordinates, ``alpha``
    the level of the interval, ``variance_scale`` per block the (rows,) fp64 factor of Var(S) or None."""

    stats: list
    slopes: list
    coord: np.ndarray
    alpha: float
    variance_scale: list | None = None
    kern: object = None

    @classmethod
    def fit(cls, Yblocks, coord, alpha: float = 0.05, variance_scale=None, kern=None) -> "MannKendall":
        """``Yblocks``: (n, rows) fp32 per block -- ``PeriodStats.series`` / ``SpellStats`` results as they are;
        ``coord``: n numbers (years: ``period_years()``), or datetime64 stamps taken as days since the first;
        ``alpha``: the interval covers 1 - alpha; ``variance_scale``: per block a (rows,) factor of Var(S), for instance
        n / n_eff of ``LagStats.effective_sample_size``.  Per block one ``mk_stats`` and one ``sen_slopes`` call."""
        who = "MannKendall.fit"
        c = _coordinate(coord, who)
        if not 0.0 < float(alpha) < 1.0:
            raise ValueError(f"{who}: alpha = {alpha!r}, a level inside (0, 1) asked for")
        kern = _provider(kern, who)
        Yblocks = list(Yblocks)
        if not Yblocks:
            raise ValueError(f"{who}: no blocks")
        scales = None
        if variance_scale is not None:
            scales = list(variance_scale) if isinstance(variance_scale, (list, tuple)) else [variance_scale]
            if len(scales) != len(Yblocks):
                raise ValueError(f"{who}: {len(scales)} variance scales for {len(Yblocks)} blocks")
        stats, slopes, kept = [], [], []
        for b, Y in enumerate(_checked(Yblocks, c.shape[0], who)):
            scale = None
            if scales is not None:
                scale = torch.as_tensor(scales[b]).to(device=Y.device, dtype=torch.float64).reshape(-1)
                if int(scale.shape[0]) != int(Y.shape[1]):
                    raise ValueError(f"{who}: variance_scale[{b}] holds {int(scale.shape[0])} rows, the block "
                                     f"{int(Y.shape[1])}")
                kept.append(scale)
            Q = kern.mk_stats(Y)
            stats.append(Q)
            slopes.append(kern.sen_slopes(Y, c, interval_ranks(Q, alpha, scale).contiguous()))
        return cls(stats, slopes, c, float(alpha), kept if scales is not None else None, kern)

    # -- the test ---------------------------------------------------------------------------------------------------
    def _scale(self, b: int):
        return None if self.variance_scale is None else self.variance_scale[b]

    def n_valid(self) -> list:
        """The valid points v of every row, (rows,) int32 per block."""
        return [Q[0] for Q in self.stats]

    def s(self) -> list:
        """Kendall's S, the sum over the pairs a < b of sgn(y_b - y_a)."""
        return [Q[1] for Q in self.stats]

    def variance(self) -> list:
        """Var(S) with the correction for ties, times the variance scale; fp64."""
        return [_variance(Q, self._scale(b)) for b, Q in enumerate(self.stats)]

    def z(self) -> list:
        """(S - sgn S) / sigma, the continuity-corrected normal score; NaN where sigma = 0."""
        out = []
        for Q, var in zip(self.stats, self.variance()):
            S, sigma = Q[1].to(torch.float64), torch.sqrt(var)
            safe = torch.where(sigma > 0, sigma, torch.ones_like(sigma))
            out.append(torch.where(sigma > 0, (S - torch.sign(S)) / safe, torch.full_like(sigma, float("nan"))))
        return out

    def p_value(self) -> list:
        """The two-sided p-value erfc(|Z| / sqrt 2)."""
        return [torch.special.erfc(torch.abs(Z) / torch.full_like(Z, math.sqrt(2.0))) for Z in self.z()]

    def tau_b(self) -> list:
        """Kendall's tau-b, S / sqrt(N (N - E)); NaN where every pair is tied or there is none."""
        out = []
        for Q in self.stats:
            N = _pairs(Q)
            den = (N * (N - Q[2].to(torch.int64))).to(torch.float64)
            safe = torch.where(den > 0, den, torch.ones_like(den))
            out.append(torch.where(den > 0, Q[1].to(torch.float64) / torch.sqrt(safe), torch.full_like(den, float("nan"))))
        return out

    # -- the slope --------------------------------------------------------------------------------------------------
    def slope(self, per: float = 1.0) -> list:
        """The Theil-Sen slope, the median of the pairwise slopes: the mean of the two middle ones, formed in fp64 and
        rounded once to fp32, times ``per`` (10.0: per decade of a coordinate in years).  Slopes that overflow fp32 are
        ordinary values of the kernel: a row whose two middle slopes are -Inf and +Inf has the slope NaN."""
        return [((E[0].to(torch.float64) + E[1].to(torch.float64)) * 0.5).to(torch.float32) * float(per)
                for E in self.slopes]

    def slope_interval(self, per: float = 1.0) -> tuple:
        """``(lower, upper)``: the rank-based 1 - alpha confidence interval of the slope, times ``per`` (> 0)."""
        if not float(per) > 0.0:
            raise ValueError(f"MannKendall.slope_interval: per = {per!r}, a positive factor asked for")
        return [E[2] * float(per) for E in self.slopes], [E[3] * float(per) for E in self.slopes]

    def significant(self, alpha: float | None = None, fdr: bool = False) -> list:
        """p <= alpha per row (default: the level of the fit); with ``fdr`` p <= :func:`fdr_threshold` over all rows
        of the blocks of this process (Benjamini-Hochberg).  A NaN p-value is not significant."""
        a = self.alpha if alpha is None else float(alpha)
        p = self.p_value()
        thr = fdr_threshold(p, a) if fdr else a
        return [q <= thr for q in p]

    # -- persistence ------------------------------------------------------------------------------------------------
    def to_dataset(self, coords=None) -> Dataset:
        """``mk_planes(plane, space)`` int32, ``sen_slopes(rank, space)`` fp32, ``mk_coord(point)`` fp64,
        ``variance_scale(space)`` fp64 where there is one, and the attribute ``alpha`` (``repr`` of the fp64: an exact
        round trip); ``coords``: the per-row coordinates of the decomposed array, taken over as they are.
        ``io_netcdf.to_netcdf`` writes it."""
        cds = {"plane": Coord("plane", np.arange(len(PLANES), dtype=np.int64)),
               "rank": Coord("rank", np.arange(len(RANKS), dtype=np.int64)),
               "point": Coord("point", np.arange(self.coord.shape[0], dtype=np.int64)), **ta.row_coords(coords)}
        row = {k: v for k, v in cds.items() if k not in ("plane", "rank", "point")}
        ds = Dataset(coords=cds, attrs={"alpha": repr(float(self.alpha))})
        join = lambda blocks: np.concatenate([B.detach().cpu().numpy() for B in blocks], axis=-1)
        ds["mk_planes"] = DataArray(join(self.stats).astype(np.int32), ("plane", "space"), {"plane": cds["plane"], **row})
        ds["sen_slopes"] = DataArray(join(self.slopes).astype(np.float32), ("rank", "space"), {"rank": cds["rank"], **row})
        ds["mk_coord"] = DataArray(self.coord.astype(np.float64), ("point",), {"point": cds["point"]})
        if self.variance_scale is not None:
            ds["variance_scale"] = DataArray(join(self.variance_scale).astype(np.float64), ("space",), dict(row))
        return ds

    @classmethod
    def from_dataset(cls, ds: Dataset, rows=None, device=None, kern=None) -> "MannKendall":
        """The fit :meth:`to_dataset` stored (``io_netcdf.open_dataset`` of its file).  ``rows``: the row counts of the
        blocks (default: one block); ``device``: where they go (default: the GPU for the HIP provider)."""
        who = "MannKendall.from_dataset"
        kern = _kern(kern)
        planes = np.ascontiguousarray(np.asarray(ds["mk_planes"].values), dtype=np.int32)
        slopes = np.ascontiguousarray(np.asarray(ds["sen_slopes"].values), dtype=np.float32)
        if planes.shape[0] != len(PLANES) or slopes.shape[0] != len(RANKS) or planes.shape[1] != slopes.shape[1]:
            raise ValueError(f"{who}: mk_planes is {planes.shape} and sen_slopes {slopes.shape}; ({len(PLANES)}, rows) and "
                             f"({len(RANKS)}, rows) asked for")
        scale = None
        if "variance_scale" in ds:
            sc = np.ascontiguousarray(np.asarray(ds["variance_scale"].values), dtype=np.float64).reshape(1, -1)
            scale = [s.reshape(-1) for s in ta.cut_rows(sc, rows, device, kern, who)]
        coord = np.asarray(ds["mk_coord"].values).astype(np.float64).reshape(-1)
        return cls(ta.cut_rows(planes, rows, device, kern, who), ta.cut_rows(slopes, rows, device, kern, who), coord,
                   float(ta.attr_str(ds.attrs["alpha"])), scale, kern)
