"""DINEOF gap filling (Beckers & Rixen 2003; Alvera-Azcarate et al. 2005) of a field whose gaps move in time, iterated
on the device (K31, csrc/gapfill.hip): the decomposition of a gappy field, and the field with its gaps filled.

``missing = "mask"`` (K20) drops a grid point that is missing in any snapshot from every snapshot.  That is right for
land under sea-surface temperature and wrong for a moving ice edge, a satellite swath or a few bad hours.  Here the gaps
are NaN (or +-Inf) in the resident ``(T, rows)`` fp32 row blocks, and the blocks are filled IN PLACE:

    1. ``gap_mask`` per block: the packed mask W (one bit per element), the gaps per row, the fp64 sum and sum of squares
       of the present values.  Rows with fewer than ``min_valid`` present values -- or, under ``scale``, no variance --
       are MASKED ROWS: all their bits are set, mean = 0, std = 1, they end as NaN and are reported in ``row_mask``.
    2. mean = S1 / n in fp64, rounded to fp32; with ``scale`` std = sqrt(S2 / n - (S1 / n)^2); ``scale0`` is the rms of
       the standardised present values, from the same sums.
    3. The cross-validation set: ``numpy.random.default_rng(seed + rank)`` draws
       ``max(min_cv, cv_fraction * present)`` distinct present elements of the local rows that are not masked
       (:func:`draw_cv`); their raw values are kept and their bits are set in W.
    4. ``gap_standardize_``: X holds Z = (X - mean) / std with 0 at the gaps and at the CV points.
    5. For r = 1 .. ``max_rank``: repeat { rank-r SVD of Z; C = (diag(s) Vh)^T in fp32; ``gap_fill_`` on every block;
       change = sqrt(sum change_row / n_fill) } until change <= tol scale0 or ``max_iter`` iterations -- one packed
       all-reduce per iteration.  The fill is warm-started from rank r - 1.  cv_error[r] = rms(Z[cv] - truth).  r stops
       rising once the last ``patience`` errors all exceed the minimum so far.
    6. At the best r: the CV truth goes back, the CV bits are cleared, the iteration runs to convergence and its SVD is
       kept; ``gap_standardize_(back=True)``; NaN on the masked rows.

One iteration reads X once for the SVD's Gram and once for U, and ``gap_fill_`` touches X only at the gaps: no second
X-sized buffer, no boolean mask, no ``torch.where``.

    fit = dineof_blocks(blocks, max_rank=12)        # blocks now hold the filled field
    fit.svd.s, fit.svd.Vh, fit.svd.Ut               # the decomposition of the gappy field (standardised units)
    fit.rank, fit.cv_error[fit.rank], fit.expected_error

The module runs on any provider with ``gap_mask``, ``gap_standardize_`` and ``gap_fill_`` (tests/gap_ref.py has a numpy
one); like ``row_missing_count`` in :mod:`svd` it does not import HIP.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

from . import _timeaxis as ta
from . import io_netcdf
from . import svd as _svd
from .labeled import Coord, DataArray, Dataset
from .svd import Comm, SvdResult, _kern

__all__ = ["GapFill", "dineof_blocks", "draw_cv"]

def draw_cv(rng, n_rows: int, T: int, n_cv: int, present) -> np.ndarray:
    """``n_cv`` distinct present elements, as flat indices ``row * T + t`` in the order they were drawn.  Rounds of
    ``rng.integers(0, n_rows * T, 2 * need + 16)``; a round keeps, in order, what ``present(flat)`` accepts and what was
    not drawn before.  (Rejection instead of a permutation of the present elements: nothing of the size of X exists on
    the host.)"""
    got = np.empty(0, dtype=np.int64)
    for _ in range(200):
        need = n_cv - got.size
        if need <= 0:
            break
        d = rng.integers(0, n_rows * T, size=2 * need + 16, dtype=np.int64)
        d = d[np.asarray(present(d), dtype=bool)]
        both = np.concatenate([got, d])
        _, first = np.unique(both, return_index=True)
        got = both[np.sort(first)][:n_cv]
    if got.size < n_cv:
        raise ValueError(f"dineof_blocks: found {got.size} of {n_cv} cross-validation elements: too few present values")
    return got


@dataclass
class GapFill:
    """What :func:`dineof_blocks` found.  ``cv_error[r]`` and ``iterations[r]`` are indexed by the rank r = 1 .. the last
    one tried (``cv_error[0]`` is NaN, ``iterations[0]`` counts the final pass); ``converged``: the final pass met
    ``tol``.  ``n_missing``: the filled gaps (all ranks; masked rows not counted), ``n_cv``: the cross-validation
    elements (all ranks).  ``mean`` / ``std`` / ``row_mask`` per block: (rows,) fp32, fp32 and bool.  ``masks``: the W
    tensors of the final pass -- a set bit is a filled element, every bit of a masked row is set.  ``svd``: the
    :class:`svd.SvdResult` of the final pass, the decomposition of the standardised gappy field.  ``expected_error``:
    ``cv_error[rank]``, in the units of the data when ``scale`` was False and in standard deviations otherwise."""

    rank: int
    cv_error: np.ndarray
    iterations: np.ndarray
    converged: bool
    n_missing: int
    n_cv: int
    scale0: float
    tol: float
    scaled: bool
    mean: list
    std: list
    row_mask: list
    masks: list | None = field(default=None, repr=False)
    svd: SvdResult | None = field(default=None, repr=False)
    kern: object = field(default=None, repr=False)

    @property
    def expected_error(self) -> float:
        return float(self.cv_error[self.rank])

    # -- persistence ----------------------------------------------------------------------------------------------
    def to_dataset(self, coords=None) -> Dataset:
        """Everything but the masks: ``cv_error(rank)``, ``iterations(rank)``, ``mean`` / ``std`` / ``row_mask(space)``,
        ``s(mode)``, ``Vh(mode, time_index)`` and ``U(mode, space)`` of the final SVD; the scalars as attributes."""
        nr = len(self.cv_error)
        cds = {"rank": Coord("rank", np.arange(nr, dtype=np.int64))}
        cds.update(ta.row_coords(coords))
        row = {n: c for n, c in cds.items() if n != "rank"}
        ds = Dataset(coords=cds, attrs={"rank": int(self.rank), "converged": int(self.converged),
                                        "n_missing": int(self.n_missing), "n_cv": int(self.n_cv),
                                        "scale0": repr(float(self.scale0)), "tol": repr(float(self.tol)),
                                        "scaled": int(self.scaled)})
        ds["cv_error"] = DataArray(np.array(self.cv_error, dtype=np.float64), ("rank",), {"rank": cds["rank"]})
        ds["iterations"] = DataArray(np.array(self.iterations, dtype=np.int64), ("rank",), {"rank": cds["rank"]})
        for name, parts, dtype in (("mean", self.mean, np.float32), ("std", self.std, np.float32),
                                   ("row_mask", self.row_mask, np.int8)):
            ds[name] = DataArray(np.concatenate([v.detach().cpu().numpy().astype(dtype) for v in parts]), ("space",), row)
        if self.svd is not None:
            k, n = int(self.svd.Vh.shape[0]), int(self.svd.Vh.shape[1])
            mode = Coord("mode", np.arange(k, dtype=np.int64))
            tix = Coord("time_index", np.arange(n, dtype=np.int64))
            ds["s"] = DataArray(self.svd.s.detach().cpu().numpy().astype(np.float64), ("mode",), {"mode": mode})
            ds["Vh"] = DataArray(self.svd.Vh.detach().cpu().numpy().astype(np.float64), ("mode", "time_index"),
                                 {"mode": mode, "time_index": tix})
            ds["U"] = DataArray(self.svd.Ut.detach().cpu().numpy().astype(np.float32), ("mode", "space"),
                                dict(row, mode=mode))
        return ds

    @classmethod
    def from_dataset(cls, ds: Dataset, rows=None, device=None, kern=None) -> "GapFill":
        """The fit :meth:`to_dataset` stored (``masks`` is None).  ``rows``: the row counts of the blocks to cut the
        per-row vectors into (default: one block); ``device``: where they go (default: the GPU for the HIP provider)."""
        kern = _kern(kern)
        a = ds.attrs

        def cut(name, dtype):
            v = np.ascontiguousarray(np.asarray(ds[name].values), dtype=dtype).reshape(1, -1)
            return [t.reshape(-1) for t in ta.cut_rows(v, rows, device, kern, "GapFill.from_dataset")]

        mean, std = cut("mean", np.float32), cut("std", np.float32)
        row_mask = [t != 0 for t in cut("row_mask", np.int8)]
        res = None
        if "U" in ds:
            dev = mean[0].device
            res = SvdResult(Ut=torch.from_numpy(np.ascontiguousarray(np.asarray(ds["U"].values), dtype=np.float32)).to(dev),
                            s=torch.from_numpy(np.asarray(ds["s"].values, dtype=np.float64).reshape(-1).copy()).to(dev),
                            Vh=torch.from_numpy(np.ascontiguousarray(np.asarray(ds["Vh"].values), dtype=np.float64)).to(dev))
        return cls(ta.attr_int(a["rank"]), np.asarray(ds["cv_error"].values, dtype=np.float64).reshape(-1),
                   np.asarray(ds["iterations"].values, dtype=np.int64).reshape(-1), bool(ta.attr_int(a["converged"])),
                   ta.attr_int(a["n_missing"]), ta.attr_int(a["n_cv"]), float(ta.attr_str(a["scale0"])),
                   float(ta.attr_str(a["tol"])), bool(ta.attr_int(a["scaled"])), mean, std, row_mask, None, res, kern)

    def to_netcdf(self, path: str, coords=None) -> str:
        return io_netcdf.to_netcdf(self.to_dataset(coords), path)

    @classmethod
    def from_netcdf(cls, path: str, rows=None, device=None, kern=None) -> "GapFill":
        return cls.from_dataset(io_netcdf.open_dataset(path), rows, device, kern)


def _flip_bits_(W: torch.Tensor, rows: torch.Tensor, ts: torch.Tensor, on: bool) -> None:
    """Set (``on``) or clear the bits of the distinct elements (rows[j], ts[j]) in the words W (ceil(T / 32), m).  The
    bits of one word are OR-ed first (distinct elements: distinct bits, so their sum in int64), then every word is
    named once in one indexed update."""
    if rows.numel() == 0:
        return
    m = int(W.shape[1])
    word, inv = torch.unique((ts >> 5) * m + rows, return_inverse=True)
    acc = torch.zeros(word.shape[0], dtype=torch.int64, device=W.device)
    acc.index_add_(0, inv, torch.ones_like(ts) << (ts & 31))
    acc = torch.where(acc >= 1 << 31, acc - (1 << 32), acc).to(torch.int32)     # the word's bit pattern, as int32
    i, j = torch.div(word, m, rounding_mode="floor"), word % m
    W[i, j] = (W[i, j] | acc) if on else (W[i, j] & ~acc)


def _bits_at(W: torch.Tensor, rows: torch.Tensor, ts: torch.Tensor) -> torch.Tensor:
    return (W[ts >> 5, rows] >> (ts & 31)) & 1


def dineof_blocks(Xblocks, max_rank: int, *, cv_fraction: float = 0.01, min_cv: int = 30, seed: int = 0,
                  tol: float = 1e-4, max_iter: int = 100, patience: int = 2, scale: bool = False, min_valid: int = 2,
                  svd: str = "snapshots", comm: Comm | None = None, kern=None) -> GapFill:
    """Fill the non-finite elements of the resident ``(T, rows)`` fp32 row blocks ``Xblocks`` in place by DINEOF and
    return the :class:`GapFill` (the module's docstring has the algorithm).  ``max_rank``: the largest rank tried;
    ``svd``: "snapshots" (the Gram route, ``deflate_mean=False``) or "randomized" (``random_state=seed``); ``comm``: the
    row shards' communicator (:class:`svd.Comm`).  Not here: delay embedding, streamed slices."""
    kern = _kern(kern)
    comm = comm or Comm()
    blocks = list(Xblocks)
    if not blocks:
        raise ValueError("dineof_blocks: no blocks")
    T, dev = int(blocks[0].shape[0]), blocks[0].device
    for b, X in enumerate(blocks):
        if X.dim() != 2 or int(X.shape[0]) != T or X.dtype != torch.float32:
            raise ValueError(f"dineof_blocks: block {b} is {tuple(X.shape)} {X.dtype}, ({T}, rows) fp32 asked for")
    if svd not in ("snapshots", "randomized"):
        raise ValueError(f"dineof_blocks: svd = {svd!r}, 'snapshots' or 'randomized' asked for")
    max_rank, max_iter, patience = int(max_rank), int(max_iter), int(patience)
    if not 1 <= max_rank <= T or max_iter < 1 or patience < 1 or not 0.0 <= cv_fraction < 0.5:
        raise ValueError(f"dineof_blocks: max_rank = {max_rank} outside 1 .. T = {T}, max_iter = {max_iter} < 1, "
                         f"patience = {patience} < 1 or cv_fraction = {cv_fraction} outside [0, 0.5)")
    max_k = int(getattr(kern, "gap_fill_max_k", 256))
    if max_rank > max_k:
        raise ValueError(f"dineof_blocks: max_rank = {max_rank}, the fill holds at most {max_k} modes")
    nw = -(-T // 32)
    last_word = -1 if T % 32 == 0 else int(np.array((1 << (T % 32)) - 1, dtype=np.uint32).view(np.int32))

    # 1, 2: masks and moments
    masks, means, stds, row_masks, n_row = [], [], [], [], []
    ss_local = present_local = gaps_local = 0.0
    for X in blocks:
        W, nmiss, sums = kern.gap_mask(X, want_sums=True)
        n = (T - nmiss).to(torch.float64)
        ok = n >= max(int(min_valid), 1)
        n1 = torch.where(ok, n, torch.ones_like(n))
        m1 = sums[0] / n1
        var = sums[1] / n1 - m1 * m1
        if scale:
            ok = ok & (var > 0)
        mean = torch.where(ok, m1, torch.zeros_like(m1)).to(torch.float32)
        std = torch.where(ok, var.clamp_min(0).sqrt(), torch.ones_like(var)).to(torch.float32) if scale \
            else torch.ones_like(mean)
        if scale:
            ok = ok & (std > 0)                                  # (a variance that rounds to zero in fp32)
            mean, std = torch.where(ok, mean, torch.zeros_like(mean)), torch.where(ok, std, torch.ones_like(std))
        bad = ~ok
        if bool(bad.any()):
            W[:, bad] = -1
            W[nw - 1, bad] = last_word
        # the centred sum of squares of the present values of a row, in its own units (scale: its variance = 1)
        css = (sums[1] - sums[0] * m1).clamp_min(0)
        unit = torch.where(ok, var, torch.ones_like(var)) if scale else torch.ones_like(var)
        zz = torch.where(ok, css / unit, torch.zeros_like(css))
        ss_local += float(zz.sum())
        present_local += float(n[ok].sum())
        gaps_local += float((T - n[ok]).sum())
        masks.append(W), means.append(mean), stds.append(std), row_masks.append(bad), n_row.append(int(X.shape[1]))

    # 3: the cross-validation set of this rank
    edges = np.concatenate([[0], np.cumsum(n_row)]).astype(np.int64)
    n_cv_local = max(int(min_cv), int(cv_fraction * present_local)) if present_local > 0 else 0
    if n_cv_local > present_local / 2:
        raise ValueError(f"dineof_blocks: {n_cv_local} cross-validation elements of {int(present_local)} present values")
    rng = np.random.default_rng(int(seed) + int(comm.rank))

    def split(flat):
        """flat = row * T + t over the local rows -> per block (block, rows in the block, ts) as device tensors"""
        r, t = flat // T, flat % T
        blk = np.searchsorted(edges, r, side="right") - 1
        out = []
        for b in range(len(blocks)):
            sel = blk == b
            d = blocks[b].device
            out.append((np.nonzero(sel)[0], torch.from_numpy(r[sel] - edges[b]).to(d), torch.from_numpy(t[sel]).to(d)))
        return out

    def present(flat):
        keep = np.zeros(flat.shape[0], dtype=bool)
        for (pos, rows, ts), W in zip(split(flat), masks):
            if pos.size:
                keep[pos] = (_bits_at(W, rows, ts) == 0).cpu().numpy()
        return keep

    cv_flat = draw_cv(rng, int(edges[-1]), T, n_cv_local, present) if n_cv_local else np.empty(0, dtype=np.int64)
    cv = []                                                       # per block: rows, ts, the truth in standardised units
    for (pos, rows, ts), X, W, mean, std in zip(split(cv_flat), blocks, masks, means, stds):
        truth = (X[ts, rows] - mean[rows]) / std[rows]            # fp32: the bits gap_standardize_ gives
        _flip_bits_(W, rows, ts, True)
        cv.append((rows, ts, truth))

    tot = torch.tensor([ss_local, present_local, gaps_local, float(n_cv_local)], dtype=torch.float64, device=dev)
    ss, n_present, n_missing, n_cv = comm.allreduce_sum_(tot, tag="dineof_setup_allreduce").tolist()
    if not n_present >= 1:
        raise ValueError("dineof_blocks: no row with enough present values")
    scale0 = float(np.sqrt(ss / n_present))

    # 4
    for X, W, mean, std in zip(blocks, masks, means, stds):
        kern.gap_standardize_(X, W, mean, std if scale else None)

    def factor(r):
        if svd == "snapshots":
            return _svd.svd_snapshots(blocks, r, deflate_mean=False, comm=comm, kern=kern)
        return _svd.svd_randomized(blocks, r, random_state=int(seed), comm=comm, kern=kern)

    def iterate(r, n_fill):
        """-> (iterations, converged, rms at the CV set, the last SVD): fill at rank r until the gaps stop moving"""
        res, err, done = None, float("nan"), False
        for it in range(1, max_iter + 1):
            res = factor(r)
            Ct = (res.s[:, None] * res.Vh).T.to(torch.float32).contiguous()
            v = torch.zeros(2, dtype=torch.float64, device=dev)
            off = 0
            for X, W, (rows, ts, truth) in zip(blocks, masks, cv):
                rows_b = int(X.shape[1])
                change = kern.gap_fill_(res.Ut[:, off:off + rows_b], Ct.to(X.device), W, X)
                off += rows_b
                v[0] += change.sum().to(dev)
                if rows.numel():
                    e = (X[ts, rows] - truth).to(torch.float64)
                    v[1] += (e * e).sum().to(dev)
            total, cv_sse = comm.allreduce_sum_(v, tag="dineof_allreduce").tolist()
            if not np.isfinite(total):
                raise ValueError("dineof_blocks: the change of an iteration is not finite")
            err = float(np.sqrt(cv_sse / n_cv)) if n_cv else float("nan")
            if np.sqrt(total / max(n_fill, 1.0)) <= tol * scale0:
                done = True
                break
        return it, done, err, res

    # 5
    cv_error, iterations = [float("nan")], [0]
    for r in range(1, max_rank + 1):
        it, _, err, _ = iterate(r, n_missing + n_cv)
        cv_error.append(err), iterations.append(it)
        e = cv_error[1:]
        if len(e) > patience and all(x > min(e) for x in e[-patience:]):
            break
    rank = 1 + int(np.nanargmin(cv_error[1:])) if n_cv else max_rank

    # 6
    for X, W, (rows, ts, truth) in zip(blocks, masks, cv):
        if rows.numel():
            X[ts, rows] = truth
            _flip_bits_(W, rows, ts, False)
    it, converged, _, res = iterate(rank, n_missing)
    iterations[0] = it
    for X, mean, std, bad in zip(blocks, means, stds, row_masks):
        kern.gap_standardize_(X, None, mean, std if scale else None, back=True)
        if bool(bad.any()):
            _svd.row_mask_apply_(kern, X, bad.to(torch.int32), float("nan"))
    return GapFill(rank, np.asarray(cv_error), np.asarray(iterations, dtype=np.int64), converged, int(round(n_missing)),
                   int(round(n_cv)), scale0, float(tol), bool(scale), means, stds, row_masks, masks, res, kern)
