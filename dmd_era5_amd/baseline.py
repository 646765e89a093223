"""Lagged moments per grid point: autocorrelation, the persistence baselines of a forecast score and their skill (K26,
csrc/lagmom.hip).

``verify_blocks`` gives RMSE, bias and ACC of a forecast, ``crps_blocks`` the CRPS, ``exceed_blocks`` the Brier score.
A score is read against a baseline: persistence (the anomaly stays what it is), damped persistence (it decays with the
least-squares factor of its lag) and climatology (the anomaly is 0), as functions of the lead time and averaged over
ALL start times of the period.  All three follow from four sums per grid point and lag over the pairs
(d_{u - tau}, d_u), u = tau .. T - 1, of the anomalies d = x - centre:

    P = sum d_{u - tau} d_u      A = sum d_{u - tau}^2      B = sum d_u^2      n = T - tau

The device forms S = sum over all t of d_t^2, P, and the squares of the first and of the last tau snapshots (H, E) in
one read of the resident ``(time, rows)`` blocks for up to 8 lags (``HipKernels.lag_moments``): A = S - E, B = S - H.
No fp64 copy of X, no shifted views.  The same sums give the autocorrelation of every grid point and with it the
effective sample size behind a trend map (:meth:`trend.Trend.slope`): hourly data has far fewer than T independent
samples.

    stats = LagStats.fit(Xblocks, lags=(1, 6, 12, 24), centres=means, times=times)
    stats.autocorrelation()                      # per block (L, rows)
    stats.effective_sample_size()                # per block (rows,): T (1 - r1) / (1 + r1)
    base = baseline_scores(stats, weights=w, groups=g)           # (G, L) per key, one collective
    skill(verify["rmse"] ** 2, base["rmse_persistence"] ** 2)    # the forecast against persistence

Rows are independent: row shards fit their own blocks; :func:`baseline_scores` makes one collective.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _timeaxis as ta
from .forecast import _check_weights, _group_pieces
from .labeled import Coord, DataArray, Dataset
from .svd import Comm, _kern

__all__ = ["SEGMENT", "MAX_LAGS", "lag_moments_blocks", "LagStats", "baseline_scores", "skill"]

# the segment length of the fp64 sums: part of the arithmetic contract (a result does not depend on how a launch was
# cut), so one constant and never tuned per launch
SEGMENT = 1024
MAX_LAGS = 8


def _lag_list(lags, who: str) -> list:
    raw = np.atleast_1d(np.asarray(lags))
    if raw.ndim != 1 or raw.size == 0 or raw.dtype.kind not in "iu":
        raise ValueError(f"{who}: lags must be a non-empty list of integers, got {lags!r}")
    out = [int(v) for v in raw]
    if out[0] < 0 or any(b <= a for a, b in zip(out, out[1:])):
        raise ValueError(f"{who}: lags must be >= 0 and strictly ascending, got {out}")
    return out


def lag_moments_blocks(Xblocks, lags, centres=None, kern=None) -> list:
    """The planes of ``HipKernels.lag_moments`` for every block of ``Xblocks`` ((T, rows) fp32 per block, any iterable
    consumed once): per block a (1 + 3L, rows) fp64 tensor -- S, then P, H and E of every lag in the order of ``lags``
    (strictly ascending, 0 <= tau < T).  ``centres``: per block the (rows,) fp32 value the anomalies are taken about
    (None: the data are anomalies already).  More than 8 lags run in groups of 8, one read of X per group."""
    lags = _lag_list(lags, "lag_moments_blocks")
    kern = _kern(kern)
    L = len(lags)
    centres = None if centres is None else list(centres)
    out = []
    for b, X in enumerate(Xblocks):
        if X.dim() != 2 or lags[-1] >= int(X.shape[0]):
            raise ValueError(f"lag_moments_blocks: block {b} is {tuple(X.shape)}, the largest lag {lags[-1]} needs more "
                             "snapshots")
        if centres is not None and b >= len(centres):
            raise ValueError(f"lag_moments_blocks: {len(centres)} centres, block {b} has none")
        mu = None if centres is None or centres[b] is None else centres[b].to(torch.float32).contiguous()
        planes = torch.empty((1 + 3 * L, int(X.shape[1])), dtype=torch.float64, device=X.device)
        for g in range(0, L, MAX_LAGS):
            part = lags[g:g + MAX_LAGS]
            n = len(part)
            Q = kern.lag_moments(X, part, mu=mu, seg=SEGMENT)
            planes[0] = Q[0]
            for q in range(3):
                planes[1 + q * L + g:1 + q * L + g + n] = Q[1 + q * n:1 + (q + 1) * n]
        out.append(planes)
    return out


@dataclass
class LagStats:
    """The lagged moments of a list of row blocks: ``planes`` holds one (1 + 3L, rows) fp64 tensor per block
    (:func:`lag_moments_blocks`), ``T`` the snapshots, ``lags`` the lags in snapshots and ``step`` the spacing of the
    snapshots (a timedelta64, or None when no times were given)."""

    planes: list
    T: int
    lags: tuple
    step: object = None
    kern: object = None

    @classmethod
    def fit(cls, Xblocks, lags, centres=None, times=None, kern=None) -> "LagStats":
        """One read of every block per 8 lags.  ``times``: the T datetime64 stamps of the snapshots; they must be
        evenly spaced (a lag is a number of snapshots), else a ValueError before any launch; their step gives
        :meth:`leads` its units."""
        lags = _lag_list(lags, "LagStats.fit")
        step, Tt = None, None
        if times is not None:
            t = ta.stamps(times, "LagStats.fit").astype("datetime64[ns]")
            Tt = int(t.shape[0])
            if Tt > 1:
                d = np.diff(t)
                if not (d == d[0]).all() or not d[0] > np.timedelta64(0, "ns"):
                    raise ValueError("LagStats.fit: times must be evenly spaced and ascending: a lag is a number of "
                                     "snapshots")
                step = d[0]
        kern = _kern(kern)
        seen = []

        def checked():
            for b, X in enumerate(Xblocks):
                T = int(X.shape[0])
                if (Tt is not None and T != Tt) or (seen and T != seen[0]):
                    raise ValueError(f"LagStats.fit: block {b} holds {T} snapshots, "
                                     f"{'times has ' + str(Tt) if Tt is not None else 'block 0 ' + str(seen[0])}")
                seen.append(T)
                yield X

        planes = lag_moments_blocks(checked(), lags, centres, kern)
        if not planes:
            raise ValueError("LagStats.fit: no blocks")
        return cls(planes, seen[0], tuple(lags), step, kern)

    # -- the sums ---------------------------------------------------------------------------------------------------
    @property
    def n_lags(self) -> int:
        return len(self.lags)

    def _parts(self, Q):
        """S (rows,), and P, A, B (L, rows) of one block: A = S - E (the earlier members), B = S - H (the later)."""
        L = self.n_lags
        S = Q[0]
        return S, Q[1:1 + L], S[None] - Q[1 + 2 * L:1 + 3 * L], S[None] - Q[1 + L:1 + 2 * L]

    def _n(self, Q):
        return (self.T - torch.tensor(self.lags, dtype=torch.float64, device=Q.device))[:, None]

    def pairs(self) -> torch.Tensor:
        """n_l = T - tau_l: (L,) int64, the same for every row."""
        return self.T - torch.tensor(self.lags, dtype=torch.int64)

    def leads(self) -> np.ndarray:
        """The lags as lead times, (L,) timedelta64; needs ``times`` at the fit."""
        if self.step is None:
            raise ValueError("LagStats.leads: fitted without times (or with a single one): the lags have no units")
        return np.asarray(self.lags, dtype=np.int64) * self.step

    def autocovariance(self) -> list:
        """P / n."""
        return [self._parts(Q)[1] / self._n(Q) for Q in self.planes]

    def autocorrelation(self) -> list:
        """P / sqrt(A B): the correlation of the pairs about the centre."""
        out = []
        for Q in self.planes:
            _, P, A, B = self._parts(Q)
            out.append(P / torch.sqrt(A * B))
        return out

    def damping(self) -> list:
        """P / A: the least-squares alpha of d_u ~ alpha d_{u - tau}."""
        out = []
        for Q in self.planes:
            _, P, A, _ = self._parts(Q)
            out.append(P / A)
        return out

    def persistence_mse(self) -> list:
        """(A + B - 2 P) / n, the mean square of d_u - d_{u - tau}, clamped at 0."""
        out = []
        for Q in self.planes:
            _, P, A, B = self._parts(Q)
            out.append(((A + B - 2.0 * P) / self._n(Q)).clamp_(min=0.0))
        return out

    def damped_mse(self) -> list:
        """(B - P^2 / A) / n, the mean square of d_u - alpha d_{u - tau} with alpha = P / A (0 where A is 0), clamped
        at 0."""
        out = []
        for Q in self.planes:
            _, P, A, B = self._parts(Q)
            out.append(((B - _explained(P, A)) / self._n(Q)).clamp_(min=0.0))
        return out

    def climatology_mse(self) -> list:
        """B / n, the mean square of d_u itself."""
        return [self._parts(Q)[3] / self._n(Q) for Q in self.planes]

    def effective_sample_size(self) -> list:
        """T (1 - r) / (1 + r) with r the lag-1 autocorrelation: per block (rows,).  A ValueError when lag 1 was not
        fitted."""
        if 1 not in self.lags:
            raise ValueError(f"LagStats.effective_sample_size: lag 1 was not fitted (lags = {list(self.lags)})")
        l = self.lags.index(1)
        out = []
        for r in self.autocorrelation():
            out.append(self.T * (1.0 - r[l]) / (1.0 + r[l]))
        return out

    # -- persistence ----------------------------------------------------------------------------------------------
    def to_dataset(self, coords=None) -> Dataset:
        """``lag_moments(plane, space)`` fp64, ``lag(lag_index)`` and the attributes ``n_snapshots`` and ``step_ns``
        (the decimal string of the step in nanoseconds, empty without one); ``coords``: the per-row coordinates of
        the decomposed array, taken over as they are.  ``io_netcdf.to_netcdf`` writes it."""
        L = self.n_lags
        cds = {"plane": Coord("plane", np.arange(1 + 3 * L, dtype=np.int64)),
               "lag_index": Coord("lag_index", np.arange(L, dtype=np.int64)), **ta.row_coords(coords)}
        step = "" if self.step is None else str(int(self.step.astype("timedelta64[ns]").astype(np.int64)))
        ds = Dataset(coords=cds, attrs={"n_snapshots": int(self.T), "step_ns": step})
        row = {k: v for k, v in cds.items() if k not in ("plane", "lag_index")}
        field = np.concatenate([Q.detach().cpu().numpy() for Q in self.planes], axis=1)
        ds["lag_moments"] = DataArray(field, ("plane", "space"), {"plane": cds["plane"], **row})
        ds["lag"] = DataArray(np.asarray(self.lags, dtype=np.int64), ("lag_index",), {"lag_index": cds["lag_index"]})
        return ds

    @classmethod
    def from_dataset(cls, ds: Dataset, rows=None, device=None, kern=None) -> "LagStats":
        """The statistics :meth:`to_dataset` stored (``io_netcdf.open_dataset`` of its file).  ``rows``: the row counts
        of the blocks to cut the planes into (default: one block); ``device``: where they go (default: the GPU for
        the HIP provider)."""
        kern = _kern(kern)
        field = np.ascontiguousarray(np.asarray(ds["lag_moments"].values), dtype=np.float64)
        lags = tuple(int(v) for v in np.asarray(ds["lag"].values).reshape(-1))
        if field.shape[0] != 1 + 3 * len(lags):
            raise ValueError(f"LagStats.from_dataset: lag_moments holds {field.shape[0]} planes, {len(lags)} lags ask for "
                             f"{1 + 3 * len(lags)}")
        step = ta.attr_str(ds.attrs["step_ns"]) if "step_ns" in ds.attrs else ""
        return cls(ta.cut_rows(field, rows, device, kern, "LagStats.from_dataset"), ta.attr_int(ds.attrs["n_snapshots"]),
                   lags, np.timedelta64(int(step), "ns") if step.strip() else None, kern)


def _explained(P, A):
    """P^2 / A, the squares the damped persistence explains; 0 where A is 0 (no earlier member varies: alpha = 0)."""
    return torch.where(A > 0, P * P / torch.where(A > 0, A, torch.ones_like(A)), torch.zeros_like(A))


def baseline_scores(stats: LagStats, weights=None, groups=None, comm: Comm | None = None,
                    n_groups: int | None = None) -> dict:
    """The persistence, damped-persistence and climatology baselines on the grid, per group of rows and lag, averaged
    over all start times of the fitted period.  Conventions as :func:`forecast.verify_blocks`:
    ``weights``: per block the weight of every row (:func:`forecast.area_weights`; None: 1).  A row with weight 0 is
    left out, whatever it holds; a negative or non-finite weight is a ValueError before anything runs.  A row whose S
    is not finite (a NaN or Inf among its snapshots) is left out too and counted in ``masked_rows`` with the weight-0
    rows.  ``groups``: per block an integer label vector (0 .. G - 1), in any order and in several runs; ``n_groups``:
    G for ranks that do not see the largest label.

    With Q = A + B - 2 P (persistence), D = B - P^2 / A (damped persistence) and the weighted sums over the rows of a
    group, W the sum of their weights and n = T - tau, returns per group and lag (G, L)
      ``rmse_persistence`` = sqrt(sum w Q / (W n)), ``rmse_damped`` = sqrt(sum w D / (W n)),
      ``rmse_climatology`` = sqrt(sum w B / (W n)), ``acc_persistence`` = sum w P / sqrt(sum w A sum w B),
      ``skill_persistence_vs_clim`` = 1 - sum w Q / sum w B,
    the raw ``sums`` (G, 4, L) = sum w (P, A, B, D), and per group (G,) ``weight`` (of the rows that count), ``rows``
    and ``masked_rows``.  The mean squares are those of :meth:`LagStats.persistence_mse` and its companions, so
    ``skill(verify_blocks(...)["rmse"] ** 2, rmse_persistence ** 2)`` is the skill of a forecast against persistence.

    Row shards: ONE ``comm.allreduce_sum_`` of the stacked ``[sums, W, rows, masked]`` per call (on the device of the
    planes).  The planes are (1 + 3L) doubles per row: they are reduced on the host in one order whatever the device,
    and the results are small host tensors."""
    who = "baseline_scores"
    comm = comm or Comm()
    weights = _check_weights(weights, who)
    L = stats.n_lags
    rows_of = [int(Q.shape[1]) for Q in stats.planes]
    if weights is not None and len(weights) != len(rows_of):
        raise ValueError(f"{who}: {len(weights)} weight vectors for {len(rows_of)} blocks")
    pieces, G = _group_pieces(groups, rows_of, [1] * len(rows_of), n_groups, who)
    device = stats.planes[0].device if stats.planes else torch.device("cpu")
    # the planes are small ((1 + 3L) doubles per row): they are reduced on the host, in one order whatever the device
    sums = torch.zeros((G, 4, L), dtype=torch.float64)
    meta = torch.zeros((3, G), dtype=torch.float64)
    for b, Q in enumerate(stats.planes):
        S, P, A, B = stats._parts(Q.cpu())
        w = torch.ones(rows_of[b], dtype=torch.float64) if weights is None else \
            torch.as_tensor(weights[b]).to(device="cpu", dtype=torch.float64).reshape(-1)
        if w.numel() != rows_of[b]:
            raise ValueError(f"{who}: weights[{b}] has {w.numel()} entries, the block {rows_of[b]} rows")
        keep = (w != 0) & torch.isfinite(S)
        stack = torch.stack([P, A, B, B - _explained(P, A)])                      # (4, L, rows)
        stack = torch.where(keep[None, None], stack * w[None, None], torch.zeros_like(stack))
        for s, e, g in pieces[b]:
            sums[g] += stack[:, :, s:e].sum(dim=2)
            k = keep[s:e]
            meta[0, g] += float(w[s:e][k].sum())
            meta[1, g] += e - s
            meta[2, g] += (e - s) - int(k.sum())
    flat = torch.cat([sums.reshape(-1), meta.reshape(-1)]).to(device)
    flat = comm.allreduce_sum_(flat, tag="baseline_allreduce").cpu()
    sums = flat[:sums.numel()].reshape(G, 4, L)
    W, rows, masked = flat[sums.numel():].reshape(3, G)
    n = (stats.T - torch.tensor(stats.lags, dtype=torch.float64))[None]
    SP, SA, SB, SD = (sums[:, q] for q in range(4))
    SQ = (SA + SB - 2.0 * SP).clamp(min=0.0)
    Wn = W[:, None] * n
    return {"rmse_persistence": torch.sqrt(SQ / Wn), "rmse_damped": torch.sqrt(SD.clamp(min=0.0) / Wn),
            "rmse_climatology": torch.sqrt(SB / Wn), "acc_persistence": SP / torch.sqrt(SA * SB),
            "skill_persistence_vs_clim": 1.0 - SQ / SB, "sums": sums, "weight": W, "rows": rows.to(torch.int64),
            "masked_rows": masked.to(torch.int64)}


def skill(mse_model, mse_reference):
    """``1 - mse_model / mse_reference``, elementwise: 1 is a perfect forecast, 0 no better than the reference, negative
    worse.  The glue between :func:`forecast.verify_blocks` and :func:`baseline_scores`: ``mse_model`` is
    ``verify_blocks(...)["rmse"] ** 2`` at the snapshots whose lead times are the lags (``S0 / W`` of its sums),
    ``mse_reference`` is ``rmse_persistence ** 2``, ``rmse_damped ** 2`` or ``rmse_climatology ** 2`` of
    :func:`baseline_scores` with the same weights and groups -- anomalies about the same centre on both sides
    (``clims`` there, ``centres`` here)."""
    return 1.0 - mse_model / mse_reference
