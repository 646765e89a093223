"""From the rank-k factors back to ERA5 fields: reconstruction, DMD forecast and their score.

``svd.py`` turns a slice into ``U, s, V`` and ``bopdmd.py`` fits the optimized DMD on the reduced
coordinates ``H = V S``; both stop in the coordinates of ``U``.  This module evaluates

        x(t) = mu + sigma * (U c(t))            on the grid, per row block of U,

with ``c(t)`` either the SVD coefficients ``diag(s) Vh[:, t]`` (the rank-k reconstruction of the
decomposed snapshots) or the fitted model ``Re(Phi(t) diag(b) modes^T)`` at arbitrary times (the
forecast), and scores it against real snapshots without materialising the fields: K12
(``HipKernels.expand`` / ``expand_score``, csrc/expand.hip).  The other direction -- raw snapshots that
were not part of the decomposition to their coefficients ``c = U^T ((x - mu) / sigma)`` and energy
``||(x - mu) / sigma||^2`` -- is K13 (``HipKernels.project``, csrc/project.hip): out-of-sample validation
of the basis, compression of new data, and ``DmdForecast.restart``, which re-fits the amplitudes of a
fitted model to a new state so that the forecast starts from the latest analysis.  A bagged fit
(``bopdmd(keep_trials=True)``) is an ensemble of models: :func:`ensemble_coefficients` turns it into the mean
coefficients and the scaled member deviations, K12 expands the mean and K15 (``HipKernels.spread`` /
``spread_score``, csrc/spread.hip) the spread ``|sigma| sqrt(sum_b (U d_b)^2)`` per grid point and lead time
without storing a member field; ``DmdForecast.ensemble_score`` sets that spread against the error the mean makes.
What a forecast of gridded fields is published with -- RMSE, bias and anomaly correlation, weighted by the area of
the grid cells, per variable and level, with masked points left out -- is K16 (``HipKernels.verify``,
csrc/verify.hip): :func:`area_weights`, :func:`verify_blocks` and ``DmdForecast.verify``.  And the way out of the
package: K17 (``HipKernels.expand_range`` / ``expand_pack`` / ``field_range`` / ``pack``, csrc/pack.hip) turns the
forecast into the CF-packed int16 codes an ERA5 file stores, one ``scale_factor`` / ``add_offset`` per group of rows (a
variable), where the field is formed and without storing it in fp32: :func:`pack_blocks`, :func:`pack_field_blocks` and
``DmdForecast.pack``; ``era5_svd.write_forecast_slice`` writes them.  A model fitted on the anomalies against a slot
climatology (K18, :mod:`climatology`) takes ``climatology=`` / ``times=`` in ``DmdForecast.fields`` and ``verify`` and in
``write_forecast_slice``: the climatology is put back on the expanded fields, the analysis is anomalised for the scores.
A trend and harmonic regression that was removed as well (K21, :mod:`trend`) takes ``trend=`` in the same three places
and shares ``times=``: out after the climatology, back before it.
The members of a bagged fit as an ensemble forecast -- the continuous ranked probability score, area-weighted per group,
and the rank histogram -- are K19 (``HipKernels.crps``, csrc/crps.hip): :func:`member_coefficients`,
:func:`crps_blocks` and ``DmdForecast.ensemble_crps``; no member field is stored there either.  The same members as
the probability that a field exceeds a threshold, and that probability scored -- Brier score, reliability diagram, ROC
area -- are K24 (``HipKernels.exceed_prob`` / ``exceed_score``, csrc/exceed.hip): :func:`exceed_prob_blocks`,
:func:`exceed_blocks`, ``DmdForecast.exceedance_fields`` and ``DmdForecast.ensemble_exceedance``.

Layout as everywhere in the package (kernels.py): a column-major matrix is held as its row-major
transpose -- U blocks are ``(k, rows)`` (``SvdResult.Ut``), coefficients ``Ct`` are ``(T, k)``,
fields and snapshots ``(T, rows)``.  A delay-embedded U block is ``(k, d * rows)`` with delay j in
columns ``[j * rows, (j + 1) * rows)`` (svd._assemble_rows).

The drivers that sum a score over the grid -- :func:`score_blocks`, :func:`spread_score_blocks`, :func:`verify_blocks`,
:func:`crps_blocks`, :func:`exceed_blocks` -- are one loop, :func:`_grid_sums`: U resident, X consumed block by block, the launches of a block
from :func:`_group_pieces`, one ``allreduce_sum_`` per call; a driver states its accumulators, the kernel call on one
row range and its score formulas.  :func:`project_blocks` keeps a loop of its own (it learns T and k from the first
block and writes into the snapshot blocks).

``kern=None`` means the HIP provider, as in svd.py.  A provider WITHOUT ``expand`` (the CPU kernel
double of the tests) takes the plain torch expression, as ``svd._tn`` does for K9.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .bopdmd import OptDMDResult, _phi
from .labeled import Packing
from .svd import Comm, _kern, _pitched, embed_view, free_device_bytes, row_mask_apply_

__all__ = ["svd_coefficients", "dmd_coefficients", "ensemble_coefficients", "expand_blocks", "iter_fields",
           "score_blocks", "project_blocks", "spread_blocks", "spread_score_blocks", "area_weights", "verify_blocks",
           "member_coefficients", "crps_blocks", "exceed_blocks", "exceed_prob_blocks", "pack_blocks",
           "pack_field_blocks", "range_blocks", "range_field_blocks", "mask_weights", "DmdForecast"]


# ---------------------------------------------------------------------------
# coefficients c(t), (T, k) fp32
# ---------------------------------------------------------------------------
def svd_coefficients(s: torch.Tensor, Vh: torch.Tensor, cols=None) -> torch.Tensor:
    """``(diag(s) Vh[:, cols])^T`` as (T, k) fp32: the coefficients of the rank-k reconstruction of
    the snapshots ``cols`` (all of them by default; an index tensor, list or slice)."""
    V = Vh if cols is None else Vh[:, cols]
    return (V.to(torch.float64) * s.to(torch.float64)[:, None]).T.to(torch.float32).contiguous()


def dmd_coefficients(result: OptDMDResult, t: torch.Tensor) -> tuple[torch.Tensor, float]:
    """The fitted model at the times ``t`` (inside or beyond the training window) in the coordinates
    of U: ``(Re(Phi(t) diag(b) modes^T) as (T, n_s) fp32, max|Im| / max|Re|)``.  Phi is formed in
    complex128 (on the device by dmdx_exp_basis).  The fit does not force conjugate pairs, so the
    un-projected value has an imaginary part; its relative size says how real the model is."""
    tt = torch.as_tensor(t, dtype=torch.float64, device=result.eigs.device).reshape(-1)
    re, ratio = _model64(result, tt)
    return re.to(torch.float32).contiguous(), ratio


def _model64(result: OptDMDResult, tt: torch.Tensor) -> tuple[torch.Tensor, float]:
    """The arithmetic of :func:`dmd_coefficients` up to its rounding: (Re Z (T, n_s) fp64, imag ratio)."""
    alpha = result.eigs.to(torch.complex128)
    phi = _phi(alpha, tt.to(alpha.device), torch.complex128)
    Z = (phi * result.amplitudes.to(torch.complex128)) @ result.modes.to(torch.complex128).T
    re_max = float(Z.real.abs().max()) if Z.numel() else 0.0
    im_max = float(Z.imag.abs().max()) if Z.numel() else 0.0
    ratio = im_max / re_max if re_max > 0.0 else (0.0 if im_max == 0.0 else float("inf"))
    return Z.real, ratio


def ensemble_coefficients(results, t: torch.Tensor, ddof: int = 1) -> tuple[torch.Tensor, torch.Tensor, float]:
    """An ensemble of fitted models (``OptDMDResult.trials`` of a bagged fit) at the times ``t``:
    ``(Cbar (T, k) fp32, Dev (B, T, k) fp32, imag_ratio)``.  Every member is evaluated as
    :func:`dmd_coefficients` does, in complex128; the mean over the members and the deviations are formed in
    fp64, the deviations scaled by ``1 / sqrt(B - ddof)`` and both rounded once to fp32, so that
    ``sum_b (U Dev[b])^2`` is the variance (``ddof`` as numpy's) of the member fields.  ``imag_ratio`` is the
    largest of the members'."""
    results = list(results)
    B = len(results)
    if B - ddof < 1:
        raise ValueError(f"ensemble_coefficients: {B} members with ddof = {ddof}: B - ddof must be >= 1")
    ks = {int(r.modes.shape[0]) for r in results}
    if len(ks) != 1:
        raise ValueError(f"ensemble_coefficients: the members have different numbers of coordinates {sorted(ks)}")
    dev = results[0].eigs.device
    tt = torch.as_tensor(t, dtype=torch.float64, device=dev).reshape(-1)
    Z, ratio = [], 0.0
    for r in results:
        z, q = _model64(r, tt)
        Z.append(z.to(dev))
        ratio = max(ratio, q)
    Z = torch.stack(Z)                                   # (B, T, k) fp64
    Cbar = Z.mean(dim=0)
    Dev = (Z - Cbar) / (B - ddof) ** 0.5
    return Cbar.to(torch.float32).contiguous(), Dev.to(torch.float32).contiguous(), ratio


def member_coefficients(results, t: torch.Tensor) -> tuple[torch.Tensor, float]:
    """The members of an ensemble of fitted models (``OptDMDResult.trials`` of a bagged fit) at the times ``t``:
    ``(Cm (B, T, k) fp32, imag_ratio)``.  Every member is evaluated as :func:`dmd_coefficients` does, in
    complex128, and rounded once: ``Cm[b]`` is ``dmd_coefficients(results[b], t)[0]`` bit for bit.  These are the
    members themselves (what K19 takes), not the scaled deviations of :func:`ensemble_coefficients`;
    ``imag_ratio`` is the largest of the members'."""
    results = list(results)
    if not results:
        raise ValueError("member_coefficients: no members")
    ks = {int(r.modes.shape[0]) for r in results}
    if len(ks) != 1:
        raise ValueError(f"member_coefficients: the members have different numbers of coordinates {sorted(ks)}")
    dev = results[0].eigs.device
    tt = torch.as_tensor(t, dtype=torch.float64, device=dev).reshape(-1)
    Z, ratio = [], 0.0
    for r in results:
        z, q = _model64(r, tt)
        Z.append(z.to(torch.float32).to(dev))
        ratio = max(ratio, q)
    return torch.stack(Z).contiguous(), ratio


# ---------------------------------------------------------------------------
# one block
# ---------------------------------------------------------------------------
def _affine64(Ut, Ct, mean, std):
    P = Ct.to(torch.float64) @ Ut.to(torch.float64)
    if std is not None:
        P = P * std.to(torch.float64)
    if mean is not None:
        P = P + mean.to(torch.float64)
    return P


def _expand(kern, Ut, Ct, mean, std, out=None):
    f = getattr(kern, "expand", None)
    if f is not None:
        return f(Ut, Ct, mean, std, out=out)
    P = _affine64(Ut, Ct, mean, std).to(torch.float32)
    if out is None:
        return P
    out.copy_(P)
    return out


def _expand_score(kern, Ut, Ct, Xt, mean, std, out, want_rows):
    f = getattr(kern, "expand_score", None)
    if f is not None:
        return f(Ut, Ct, Xt, mean, std, out=out, want_rows=want_rows)
    X = Xt.to(torch.float64)
    E = X - _affine64(Ut, Ct, mean, std)
    G = X if mean is None else X - mean.to(torch.float64)
    cols = torch.stack([(E * E).sum(dim=1), (G * G).sum(dim=1)])
    if out is not None:
        out += cols
        cols = out
    return cols, ((E * E).sum(dim=0) if want_rows else None)


def _verify(kern, Ut, Ct, Xt, mean, std, weight, clim, out, want_rows):
    f = getattr(kern, "verify", None)
    if f is not None:
        return f(Ut, Ct, Xt, mean, std, weight, clim, out=out, want_rows=want_rows)
    X = Xt.to(torch.float64)
    Xh = _affine64(Ut, Ct, mean, std)
    cl = clim if clim is not None else mean
    cl = 0.0 if cl is None else cl.to(torch.float64)
    e, fc, a = Xh - X, Xh - cl, X - cl
    Q = torch.stack([e * e, e, a, fc * fc, a * a, fc * a])          # (6, T, rows)
    if weight is None:
        cols = Q.sum(dim=2)
    else:                                                           # weight 0 leaves the row out: no 0 * NaN
        sel = weight != 0
        cols = (Q[:, :, sel] * weight[sel].to(torch.float64)).sum(dim=2)
    if out is not None:
        out += cols
        cols = out
    return cols, (Q.sum(dim=1) if want_rows else None)


def _crps(kern, Ut, Cm, Xt, mean, std, weight, out, hist, want_rows):
    """K19 of one row range: (cols (2, T) fp64, rows (2, m) fp64 | None, hist (B + 1,) int64); ``out`` / ``hist`` are
    added to."""
    f = getattr(kern, "crps", None)
    if f is not None:
        return f(Ut, Cm, Xt, mean, std, weight, out=out, hist=hist, want_rows=want_rows)
    B = int(Cm.shape[0])
    X = Xt.to(torch.float64)
    P = Cm.to(torch.float64) @ Ut.to(torch.float64)                 # (B, T, rows)
    if std is not None:
        P = P * std.to(torch.float64)
    if mean is not None:
        P = P + mean.to(torch.float64)
    absq = (P - X).abs().sum(dim=0)
    coef = 2.0 * torch.arange(1, B + 1, dtype=torch.float64, device=P.device) - (B + 1)
    pair = (torch.sort(P, dim=0).values * coef[:, None, None]).sum(dim=0)      # sum_{b < b'} |x_b - x_b'|
    fin = torch.isfinite(absq)
    pair = torch.where(fin, pair, torch.full_like(pair, float("nan")))
    rank = (P < X).sum(dim=0)
    Q = torch.stack([absq, pair])                                   # (2, T, rows)
    if weight is None:
        cols, sel = Q.sum(dim=2), fin
    else:                                                           # weight 0 leaves the row out: no 0 * NaN
        keep = weight != 0
        cols = (Q[:, :, keep] * weight[keep].to(torch.float64)).sum(dim=2)
        sel = fin & keep
    counts = torch.bincount(rank[sel].reshape(-1), minlength=B + 1).to(torch.int64)
    if out is not None:
        out += cols
        hist += counts
        cols, counts = out, hist
    return cols, (Q.sum(dim=1) if want_rows else None), counts


def _exceed_elements(Ut, Cm, thr, slot, above, mean, std):
    """The torch fp64 form of K24's elements: (c (J, T, rows) int64, the thresholds (J, T, rows) fp64, finite (T, rows))."""
    P = Cm.to(torch.float64) @ Ut.to(torch.float64)                 # (B, T, rows)
    if std is not None:
        P = P * std.to(torch.float64)
    if mean is not None:
        P = P + mean.to(torch.float64)
    th = (thr if thr.dim() == 3 else thr.unsqueeze(1)).to(torch.float64)
    T = int(Cm.shape[1])
    sl = torch.zeros(T, dtype=torch.long, device=th.device) if slot is None else slot.to(torch.long)
    th = th[:, sl, :]                                               # (J, T, rows)
    ev = P[None] > th[:, None] if above else P[None] < th[:, None]
    return ev.sum(dim=1), th, torch.isfinite(P).all(dim=0)


def _exceed_prob(kern, Ut, Cm, thr, slot, above, mean, std, out=None):
    """K24's probability planes of one row range: (J, T, rows) fp32."""
    f = getattr(kern, "exceed_prob", None)
    if f is not None:
        return f(Ut, Cm, thr, slot, above, mean, std, out=out)
    c, _, fin = _exceed_elements(Ut, Cm, thr, slot, above, mean, std)
    p = (c.to(torch.float64) / int(Cm.shape[0])).to(torch.float32)
    p = torch.where(fin[None], p, torch.full_like(p, float("nan")))
    if out is None:
        return p
    out.copy_(p)
    return out


def _exceed(kern, Ut, Cm, Xt, thr, slot, above, mean, std, weight, out, counts, want_rows):
    """K24's score of one row range: (cols (J, 4, T) fp64, rows (J, 4, m) fp64 | None, counts (J, 2, B + 1) int64);
    ``out`` / ``counts`` are added to."""
    f = getattr(kern, "exceed_score", None)
    if f is not None:
        return f(Ut, Cm, Xt, thr, slot, above, mean, std, weight, out=out, counts=counts, want_rows=want_rows)
    B = int(Cm.shape[0])
    c, th, fin = _exceed_elements(Ut, Cm, thr, slot, above, mean, std)
    X = Xt.to(torch.float64)
    fin = fin & torch.isfinite(X)
    o = (X[None] > th) if above else (X[None] < th)                 # (J, T, rows)
    of = o.to(torch.float64)
    p = (c.to(torch.float64) / B).to(torch.float32).to(torch.float64)
    Q = torch.stack([(p - of) ** 2, of, p, p * p], dim=1)           # (J, 4, T, rows)
    Q = torch.where(fin[None, None], Q, torch.full_like(Q, float("nan")))
    if weight is None:
        cols, sel = Q.sum(dim=3), fin
    else:                                                           # weight 0 leaves the row out: no 0 * NaN
        keep = weight != 0
        cols = (Q[:, :, :, keep] * weight[keep].to(torch.float64)).sum(dim=3)
        sel = fin & keep
    J = int(c.shape[0])
    cnt = torch.stack([torch.bincount((o[j].to(torch.long) * (B + 1) + c[j])[sel].reshape(-1), minlength=2 * (B + 1))
                       for j in range(J)]).reshape(J, 2, B + 1).to(torch.int64)
    if out is not None:
        out += cols
        counts += cnt
        cols, cnt = out, counts
    return cols, (Q.sum(dim=2) if want_rows else None), cnt


def _merge_range(P: torch.Tensor, out):
    """(range (2,) fp32, count (1,) int64) of the fp32 field P, merged into the pair ``out`` of an earlier call."""
    fin = torch.isfinite(P)
    inf = torch.tensor(float("inf"), dtype=torch.float32, device=P.device)
    mn = torch.where(fin, P, inf).amin() if P.numel() else inf
    mx = torch.where(fin, P, -inf).amax() if P.numel() else -inf
    cnt = (~fin).sum().reshape(1)
    if out is None:
        return torch.stack([mn, mx]), cnt
    rng, c = out
    rng[0], rng[1] = torch.minimum(rng[0], mn), torch.maximum(rng[1], mx)
    c += cnt
    return rng, c


def _encode_host(P: torch.Tensor, packing: Packing, out, counts):
    q, filled, saturated = packing.encode(P.detach().cpu().numpy(), counts=True)
    Q = torch.from_numpy(q).to(P.device)
    if out is not None:
        out.copy_(Q)
        Q = out
    add = torch.tensor([filled, saturated], dtype=torch.int64, device=P.device)
    if counts is None:
        return Q, add
    counts += add
    return Q, counts


def _expand_range(kern, Ut, Ct, mean, std, out):
    f = getattr(kern, "expand_range", None)
    if f is not None:
        return f(Ut, Ct, mean, std, out=out)
    return _merge_range(_expand(kern, Ut, Ct, mean, std), out)


def _expand_pack(kern, Ut, Ct, mean, std, packing, out, counts):
    f = getattr(kern, "expand_pack", None)
    if f is not None:
        return f(Ut, Ct, mean, std, packing, out=out, counts=counts)
    return _encode_host(_expand(kern, Ut, Ct, mean, std), packing, out, counts)


def _field_range(kern, Xt, out):
    f = getattr(kern, "field_range", None)
    return f(Xt, out=out) if f is not None else _merge_range(Xt, out)


def _field_pack(kern, Xt, packing, out, counts):
    f = getattr(kern, "pack", None)
    return f(Xt, packing, out=out, counts=counts) if f is not None else _encode_host(Xt, packing, out, counts)


def _project(kern, Ut, Xt, mean, std, out, want_energy=True):
    f = getattr(kern, "project", None)
    if f is not None:
        return f(Ut, Xt, mean, std, out=out, want_energy=want_energy)
    X = Xt.to(torch.float64)
    if mean is not None:
        X = X - mean.to(torch.float64)
    if std is not None:
        X = X / std.to(torch.float64)
    C = X @ Ut.to(torch.float64).T
    e = (X * X).sum(dim=1) if want_energy else None
    if out is None:
        return C, e
    out[0].add_(C)
    if want_energy:
        out[1].add_(e)
    return out


def _spread64(Ut, Dev):
    """sum_b (U d_b)^2 as (T, rows) fp64."""
    P = Dev.to(torch.float64) @ Ut.to(torch.float64)       # (B, T, rows)
    return (P * P).sum(dim=0)


def _spread(kern, Ut, Dev, std, out=None):
    f = getattr(kern, "spread", None)
    if f is not None:
        return f(Ut, Dev, std, out=out)
    S = torch.sqrt(_spread64(Ut, Dev))
    if std is not None:
        S = S * std.to(torch.float64).abs()
    S = S.to(torch.float32)
    if out is None:
        return S
    out.copy_(S)
    return out


def _spread_score(kern, Ut, Dev, std, out, want_rows):
    f = getattr(kern, "spread_score", None)
    if f is not None:
        return f(Ut, Dev, std, out=out, want_rows=want_rows)
    V = _spread64(Ut, Dev)
    if std is not None:
        V = V * std.to(torch.float64) ** 2
    var = V.sum(dim=1)
    if out is not None:
        out += var
        var = out
    return var, (V.sum(dim=0) if want_rows else None)


def _pitched_dev(kern, Dev: torch.Tensor) -> torch.Tensor:
    """The (B, T, k) deviations with every k-vector on a 16-byte boundary, ONCE for all row blocks (the image
    HipKernels.spread hands to K15 as it is)."""
    if getattr(kern, "pitch", None) is None:
        return Dev
    B, T, k = Dev.shape
    if Dev.is_contiguous() and k % 4 == 0 and Dev.data_ptr() % 16 == 0:
        return Dev
    Dp = torch.zeros((B, T, (k + 3) // 4 * 4), dtype=Dev.dtype, device=Dev.device)
    Dp[:, :, :k] = Dev
    return Dp[:, :, :k]


def _vec(v, b, reps, device):
    """Block b of a list of per-row vectors (or None) as fp32 on ``device``, repeated for every delay.  An entry with
    three dimensions is a table (..., rows) per row -- K24's thresholds -- and keeps its shape: the rows are its last
    axis."""
    if v is None:
        return None
    x = torch.as_tensor(v[b]).to(device=device, dtype=torch.float32)
    if x.dim() == 3:
        return (x.repeat(1, 1, reps) if reps > 1 else x).contiguous()
    x = x.reshape(-1)
    return (x.repeat(reps) if reps > 1 else x).contiguous()


def _block_rows(Ub, delay, delay_block):
    """The (k, rows) view of a U block that is expanded, and how often its mean / std repeat."""
    if delay_block is None:
        return Ub, delay
    if not 0 <= delay_block < delay or Ub.shape[1] % delay:
        raise ValueError(f"delay_block = {delay_block} outside 0 .. {delay - 1}, or a U block whose "
                         f"{Ub.shape[1]} rows are no multiple of the delay {delay}")
    mb = Ub.shape[1] // delay
    return Ub[:, delay_block * mb:(delay_block + 1) * mb], 1


# ---------------------------------------------------------------------------
# lists of row blocks
# ---------------------------------------------------------------------------
def expand_blocks(Ublocks, Ct: torch.Tensor, means=None, stds=None, delay_block: int | None = None,
                  out=None, delay: int = 1, kern=None) -> list[torch.Tensor]:
    """The fields of every row block: a list of (T, rows) fp32 tensors, ``mean + std * (U c)``.

    ``means`` / ``stds``: lists of per-row vectors of the PHYSICAL rows of every block (None: 0 / 1).
    ``delay``: the delay embedding U was computed with (d * rows columns per block);
    ``delay_block = j`` expands the rows of delay j only -- ``delay_block=0`` gives the physical
    fields at the times of ``Ct`` -- None all d * rows of them.
    ``out``: a list of (T, rows) fp32 views to write into.
    Refuses (MemoryError, bytes stated) when the result does not fit the free device memory: use
    :func:`iter_fields` then."""
    kern = _kern(kern)
    Ublocks = list(Ublocks)
    views = [_block_rows(U, delay, delay_block) for U in Ublocks]
    T = int(Ct.shape[0])
    if out is None:
        need = 4 * T * sum(int(U.shape[1]) for U, _ in views)
        dev = Ublocks[0].device
        if dev.type == "cuda":
            free = free_device_bytes(dev)
            if need > free:
                raise MemoryError(f"expand_blocks: the fields need {need} bytes ({T} snapshots x "
                                  f"{need // (4 * max(T, 1))} rows, fp32) and {free} bytes of device memory are "
                                  "free; expand time chunks with iter_fields(..., chunk=)")
    Cp = _pitched(kern, Ct)
    res = []
    for b, (U, reps) in enumerate(views):
        res.append(_expand(kern, U, Cp, _vec(means, b, reps, U.device), _vec(stds, b, reps, U.device),
                           out=None if out is None else out[b]))
    return res


def iter_fields(Ublocks, Ct: torch.Tensor, means=None, stds=None, delay_block: int | None = None,
                delay: int = 1, chunk: int = 256, kern=None):
    """Time-chunked :func:`expand_blocks`: yields ``(t0, t1, blocks)`` with the fields of the
    coefficients ``Ct[t0:t1]``; every chunk reuses the buffers of the one before (copy what you keep)."""
    if chunk < 1:
        raise ValueError("iter_fields: chunk >= 1")
    Ublocks = list(Ublocks)
    bufs = None
    T = int(Ct.shape[0])
    for t0 in range(0, T, chunk):
        t1 = min(T, t0 + chunk)
        o = None if bufs is None else [B[:t1 - t0] for B in bufs]
        blocks = expand_blocks(Ublocks, Ct[t0:t1], means, stds, delay_block, out=o, delay=delay, kern=kern)
        if bufs is None:
            bufs = blocks
        yield t0, t1, blocks


def _check_weights(weights, who):
    """The per-block row weights as a list (or None); a negative or non-finite one is refused, before any launch."""
    if weights is None:
        return None
    weights = list(weights)
    for b, v in enumerate(weights):
        x = torch.as_tensor(v).to(torch.float64)
        bad = int((~torch.isfinite(x) | (x < 0)).sum())
        if bad:
            raise ValueError(f"{who}: {bad} weights of block {b} are negative or not finite (a row is left "
                             "out with the weight 0)")
    return weights


def _block_vecs(vecs: dict, b, reps, mb, device, who) -> dict:
    """Block b of every named list of per-row vectors (:func:`_vec`), each of them as long as the block's mb
    physical rows."""
    out = {}
    for name, v in vecs.items():
        out[name] = x = _vec(v, b, reps, device)
        if x is not None and (x.shape[-1] if x.dim() == 3 else x.numel()) != reps * mb:
            raise ValueError(f"{who}: {name}[{b}] has {(x.shape[-1] if x.dim() == 3 else x.numel()) // reps} entries, the "
                             f"block {mb} rows")
    return out


def _grid_sums(who, tag, comm, Ublocks, Xblocks, T, delay, device, vecs: dict, zeros, launch, groups=None,
               n_groups=None, want_rows=False):
    """The loop of the drivers that sum a score over the grid (:func:`score_blocks`, :func:`spread_score_blocks`,
    :func:`verify_blocks`, :func:`crps_blocks`): the blocks in order, the launches of a block in the order of
    :func:`_group_pieces` (run-major, delay-minor), ONE ``comm.allreduce_sum_`` (``tag``) of everything summed.

    ``Ublocks`` is resident (a list is made of it); ``Xblocks`` -- None for a score without snapshots -- is consumed
    once, in order, one block alive at a time, and its embedded view must be (T, d * rows).  ``vecs``: name ->
    list of per-row vectors of the physical rows (or of three-dimensional tables with the rows last), or None
    (``means``, ``stds``, ...).  A ``weights`` entry makes the
    score a weighted one: it is validated (:func:`_check_weights`), and the sum of the weights W -- per run on the
    host in fp64, times the delay -- and the rows with weight 0 travel with the row count.
    ``zeros(G, device)`` -> the tuple of zero accumulators (made at the first block, or on ``device`` by a rank
    without blocks); ``launch(acc, U, E, v, g)`` adds one row range of group g to them -- ``v``: name -> that range of
    the block's vectors -- and returns its row sums (..., rows of the range) or None.

    -> (the accumulators after the collective, the counts (rows,) or (W, rows, masked rows), each (G,), the list of
    the local blocks' row sums)."""
    comm = comm or Comm()
    weighted = "weights" in vecs
    if weighted:
        vecs = {**vecs, "weights": _check_weights(vecs["weights"], who)}
    Ublocks = list(Ublocks)
    for b, U in enumerate(Ublocks):
        if U.shape[1] % delay:
            raise ValueError(f"{who}: the {int(U.shape[1])} rows of U block {b} are no multiple of the delay {delay}")
    rows_of = [int(U.shape[1]) // delay for U in Ublocks]
    pieces, G = _group_pieces(groups, rows_of, [delay] * len(rows_of), n_groups, who)
    acc, meta, row_sums = None, torch.zeros((3, G), dtype=torch.float64), []
    Xs = [None] * len(Ublocks) if Xblocks is None else Xblocks
    for b, (U, X) in enumerate(zip(Ublocks, Xs, strict=True)):         # (a streamed X that ends early is an error)
        E = None if X is None else embed_view(X, delay)
        if E is not None and E.shape != (T, U.shape[1]):
            raise ValueError(f"{who}: block {b} of X is {tuple(E.shape)} (delay {delay}), U and the coefficients ask "
                             f"for {(T, int(U.shape[1]))}")
        mb = rows_of[b]
        if acc is None:
            acc = zeros(G, U.device)
        v = _block_vecs(vecs, b, delay, mb, U.device, who)
        w = v.get("weights")
        wcpu = None if w is None else w[:mb].to(device="cpu", dtype=torch.float64)
        for s, e, g in ([(0, mb, 0)] if groups is None else pieces[b][::delay]):   # the runs: the launches of delay 0
            ww = None if wcpu is None else wcpu[s:e]
            meta[0, g] += delay * (float(e - s) if ww is None else float(ww.sum()))
            meta[1, g] += delay * (e - s)
            meta[2, g] += 0 if ww is None else delay * int((ww == 0).sum())
        R = None
        for s, e, g in pieces[b]:
            r = launch(acc, U[:, s:e], None if E is None else E[:, s:e],
                       {name: None if x is None else x[..., s:e] for name, x in v.items()}, g)
            if want_rows:
                if R is None:
                    R = r.new_zeros(r.shape[:-1] + (delay * mb,))
                R[..., s:e] = r
        if want_rows:
            row_sums.append(R)
    if acc is None:        # a rank without blocks still takes part in the collective
        acc = zeros(G, device)
    flat = torch.cat([a.reshape(-1).to(torch.float64) for a in acc]
                     + [(meta if weighted else meta[1]).reshape(-1).to(acc[0].device)])
    flat = comm.allreduce_sum_(flat, tag=tag)
    parts = flat.split([a.numel() for a in acc] + [flat.numel() - sum(a.numel() for a in acc)])
    return [p.reshape(a.shape) for p, a in zip(parts, acc)], parts[-1].reshape(-1, G), row_sums


def score_blocks(Ublocks, Ct: torch.Tensor, Xblocks, means=None, stds=None, delay: int = 1,
                 comm: Comm | None = None, want_rows: bool = False, kern=None) -> dict:
    """How well ``mean + std * (U c)`` matches the snapshots, without storing it.

    ``Xblocks``: the (n, rows) snapshot blocks that belong to ``Ublocks`` (any iterable, consumed
    once in order: a streamed X accumulates block after block); with ``delay`` d > 1 the
    zero-copy embedded view (n - d + 1, d * rows) of every block is scored, and ``Ct`` has
    n - d + 1 rows.  Returns per snapshot ``sse``, ``ref`` (= sum_i (x - mean)^2), ``rel_error`` =
    sqrt(sse / ref) and ``rmse``, the totals ``sse_total``, ``ref_total``, ``rel_error_total``,
    ``rmse_total``, ``rows`` (global), and with ``want_rows`` the list ``row_rmse`` of per-row RMSE
    vectors of the local blocks.

    Row shards: ONE ``comm.allreduce_sum_`` of the stacked per-snapshot vectors per call, whatever
    the number of local blocks (ranks hold different numbers of them)."""
    kern = _kern(kern)
    T = int(Ct.shape[0])
    Cp = _pitched(kern, Ct)
    (cols,), counts, row_sse = _grid_sums(
        "score_blocks", "score_allreduce", comm, Ublocks, Xblocks, T, delay, Ct.device, {"means": means, "stds": stds},
        lambda G, dev: (torch.zeros((2, T), dtype=torch.float64, device=dev),),
        lambda acc, U, E, v, g: _expand_score(kern, U, Cp, E, v["means"], v["stds"], acc[0], want_rows)[1],
        want_rows=want_rows)
    sse, ref, rows = cols[0], cols[1], float(counts[0, 0])
    sse_total, ref_total = sse.sum(), ref.sum()
    res = {
        "sse": sse, "ref": ref, "rel_error": torch.sqrt(sse / ref), "rmse": torch.sqrt(sse / rows),
        "sse_total": float(sse_total), "ref_total": float(ref_total),
        "rel_error_total": float(torch.sqrt(sse_total / ref_total)),
        "rmse_total": float(torch.sqrt(sse_total / (rows * T))), "rows": int(rows),
    }
    if want_rows:
        res["row_rmse"] = [torch.sqrt(r / T) for r in row_sse]
    return res


def spread_blocks(Ublocks, Dev: torch.Tensor, stds=None, delay_block: int | None = None, out=None, delay: int = 1,
                  kern=None) -> list[torch.Tensor]:
    """The ensemble spread of every row block: a list of (T, rows) fp32 tensors
    ``|std| * sqrt(sum_b (U Dev[b])^2)`` -- with ``Dev`` of :func:`ensemble_coefficients` the standard deviation
    over the members of the fields ``mean + std * (U c_b)``, per grid point and time (K15; no member field is
    stored).  ``stds``, ``delay``, ``delay_block`` and ``out`` as in :func:`expand_blocks`; a spread has no mean."""
    kern = _kern(kern)
    Dp = _pitched_dev(kern, Dev)
    res = []
    for b, U in enumerate(Ublocks):
        Ub, reps = _block_rows(U, delay, delay_block)
        res.append(_spread(kern, Ub, Dp, _vec(stds, b, reps, Ub.device), out=None if out is None else out[b]))
    return res


def spread_score_blocks(Ublocks, Dev: torch.Tensor, stds=None, delay: int = 1, comm: Comm | None = None,
                        want_rows: bool = False, kern=None) -> dict:
    """The ensemble spread summed over the grid, without storing it: per snapshot ``var`` = sum_i S[i, t]^2 and
    ``spread`` = sqrt(var / rows) (the RMS spread, the counterpart of ``rmse`` of :func:`score_blocks`), the
    totals ``var_total`` and ``spread_total`` = sqrt(var_total / (rows T)), ``rows`` (global), and with
    ``want_rows`` the list ``row_spread`` of per-row RMS spread vectors of the local blocks.  With a delay d
    all d * rows rows of every block are summed, as :func:`score_blocks` scores them.

    Row shards: ONE ``comm.allreduce_sum_`` of the stacked ``[var, rows]`` per call, whatever the number of
    local blocks.  A rank without blocks still takes part."""
    kern = _kern(kern)
    T = int(Dev.shape[1])
    Dp = _pitched_dev(kern, Dev)
    (var,), counts, row_var = _grid_sums(
        "spread_score_blocks", "spread_allreduce", comm, Ublocks, None, T, delay, Dev.device, {"stds": stds},
        lambda G, dev: (torch.zeros(T, dtype=torch.float64, device=dev),),
        lambda acc, U, E, v, g: _spread_score(kern, U, Dp, v["stds"], acc[0], want_rows)[1],
        want_rows=want_rows)
    rows = float(counts[0, 0])
    var_total = var.sum()
    res = {"var": var, "spread": torch.sqrt(var / rows), "var_total": float(var_total),
           "spread_total": float(torch.sqrt(var_total / (rows * T))), "rows": int(rows)}
    if want_rows:
        res["row_spread"] = [torch.sqrt(r / T) for r in row_var]
    return res


def area_weights(latitude_deg) -> torch.Tensor:
    """The area weight of every row of a regular latitude / longitude grid: ``cos(latitude)``, formed in fp64,
    clamped at 0 (a latitude a rounding past a pole) and rounded to fp32.  ``latitude_deg``: the latitude of
    every ROW in degrees (for a (lat, lon) plane ``lat.repeat_interleave(n_lon)``), any array-like.
    The normalisation is irrelevant: every score of :func:`verify_blocks` divides by the sum of the weights."""
    lat = torch.as_tensor(latitude_deg, dtype=torch.float64).reshape(-1)
    return torch.cos(torch.deg2rad(lat)).clamp_(min=0.0).to(torch.float32)


def _runs(labels) -> list[tuple[int, int, int]]:
    """A label vector cut into its runs: [(first row, one past the last row, label)]."""
    lab = torch.as_tensor(labels).reshape(-1).cpu()
    if lab.numel() == 0:
        return []
    if lab.dtype.is_floating_point or lab.dtype == torch.bool:
        raise ValueError(f"verify_blocks: group labels must be integers, got {lab.dtype}")
    cut = (torch.nonzero(lab[1:] != lab[:-1]).reshape(-1) + 1).tolist()
    edges = [0] + cut + [int(lab.numel())]
    return [(a, b, int(lab[a])) for a, b in zip(edges[:-1], edges[1:])]


def verify_blocks(Ublocks, Ct: torch.Tensor, Xblocks, means=None, stds=None, weights=None, clims=None, groups=None,
                  delay: int = 1, comm: Comm | None = None, want_rows: bool = False, kern=None,
                  n_groups: int | None = None) -> dict:
    """The verification of ``mean + std * (U c)`` (the forecast) against the snapshots ``Xblocks`` (the analysis)
    on the grid, without storing the fields (K16): weighted RMSE, bias and anomaly correlation per group of rows.

    ``Xblocks``, ``means``, ``stds``, ``delay`` as in :func:`score_blocks`.
    ``weights``: per block the weight of every PHYSICAL row (:func:`area_weights`; None: 1), repeated for every
    delay like ``means``.  A row with weight 0 is left out, whatever it holds -- the NaN a ``_FillValue`` became,
    the land points of a sea-surface field.  A negative or non-finite weight is a ValueError before any launch.
    ``clims``: per block the climatology of every physical row (None: the mean, and 0 without one); anomalies are
    taken against it.  With ``clims`` = the initial analysis the anomaly ``x - clim`` is the error of the
    persistence forecast: ``sqrt(S4 / W)`` is its RMSE and ``skill_vs_clim`` = 1 - S0 / S4 the skill against it.
    ``groups``: per block an integer label vector (0 .. G - 1) over the physical rows -- one variable at one level
    is one group.  The labels need not be sorted; a group may come in several runs and may be absent from a block
    or a rank (every run is one launch on a row range).  None: one group.  ``n_groups``: G, for ranks that do not
    see the largest label (all ranks must agree); by default the largest local label + 1.

    With e = forecast - analysis, f = forecast - clim, a = analysis - clim, the sums S0 .. S5 = sum w (e^2, e, a,
    f^2, a^2, f a) over the rows of a group and W = the sum of its weights, returns per group and snapshot (G, T)
      ``rmse`` = sqrt(S0 / W), ``bias`` = S1 / W, ``acc`` = S5 / sqrt(S3 S4), ``activity`` = sqrt(S3 / S4),
      ``acc_centred`` = (S5 - Sf S2 / W) / sqrt((S3 - Sf^2 / W) (S4 - S2^2 / W)) with Sf = S1 + S2 (the weighted
      means of f and a removed), ``skill_vs_clim`` = 1 - S0 / S4,
    the same over all snapshots as ``*_total`` (G,), the raw ``sums`` (G, 6, T), ``weight`` (G,) (W: the fp64 sum
    of the weights that are not 0, times the delay), ``rows`` and ``masked_rows`` (G,) (rows of the embedding, as
    :func:`score_blocks` counts them), and with ``want_rows`` the lists ``row_rmse``, ``row_bias``, ``row_acc`` of
    per-row vectors of the local blocks: the scores over time of every grid point (unweighted: a weight per row
    cancels).

    Row shards: ONE ``comm.allreduce_sum_`` of the stacked ``[sums, W, rows, masked]`` per call, whatever the
    number of local blocks and groups.  A rank without blocks still takes part."""
    kern = _kern(kern)
    T = int(Ct.shape[0])
    Cp = _pitched(kern, Ct)
    (sums,), (W, rows, masked), row_sums = _grid_sums(
        "verify_blocks", "verify_allreduce", comm, Ublocks, Xblocks, T, delay, Ct.device,
        {"means": means, "stds": stds, "weights": weights, "clims": clims},
        lambda G, dev: (torch.zeros((G, 6, T), dtype=torch.float64, device=dev),),
        lambda acc, U, E, v, g: _verify(kern, U, Cp, E, v["means"], v["stds"], v["weights"], v["clims"], acc[0][g],
                                        want_rows)[1],
        groups, n_groups, want_rows)

    def scores(S, Wn):
        S0, S1, S2, S3, S4, S5 = (S[:, q] for q in range(6))
        Sf = S1 + S2
        return {"rmse": torch.sqrt(S0 / Wn), "bias": S1 / Wn, "acc": S5 / torch.sqrt(S3 * S4),
                "acc_centred": (S5 - Sf * S2 / Wn) / torch.sqrt((S3 - Sf * Sf / Wn) * (S4 - S2 * S2 / Wn)),
                "activity": torch.sqrt(S3 / S4), "skill_vs_clim": 1.0 - S0 / S4}

    res = scores(sums, W[:, None])
    res.update({f"{key}_total": v for key, v in scores(sums.sum(dim=2), W * T).items()})
    res.update(sums=sums, weight=W, rows=rows.to(torch.int64), masked_rows=masked.to(torch.int64))
    if want_rows:
        res["row_rmse"] = [torch.sqrt(R[0] / T) for R in row_sums]
        res["row_bias"] = [R[1] / T for R in row_sums]
        res["row_acc"] = [R[5] / torch.sqrt(R[3] * R[4]) for R in row_sums]
    return res


def crps_blocks(Ublocks, Cm: torch.Tensor, Xblocks, means=None, stds=None, weights=None, groups=None, delay: int = 1,
                comm: Comm | None = None, want_rows: bool = False, fair: bool = True, kern=None,
                n_groups: int | None = None) -> dict:
    """The continuous ranked probability score and the rank histogram of the B member forecasts
    ``mean + std * (U c_b)`` against the snapshots ``Xblocks`` (the analysis) on the grid, without storing a member
    field (K19).  ``Cm``: (B, T, k) fp32, :func:`member_coefficients`.

    ``Xblocks``, ``means``, ``stds``, ``weights``, ``groups``, ``delay``, ``n_groups`` exactly as in
    :func:`verify_blocks`: a row with weight 0 is left out whatever it holds, a negative or non-finite weight is a
    ValueError before any launch, a group may come in several runs and be absent from a block or a rank.

    With S0 = sum w sum_b |x_b - y|, S1 = sum w sum_{b < b'} |x_b - x_b'| over the rows of a group and W = the sum of
    its weights, returns per group and snapshot (G, T)
      ``crps`` = S0 / (B W) - S1 / (B (B - 1) W) (``fair=True``: the estimator that is unbiased for a finite
      ensemble; B < 2 is a ValueError) or S0 / (B W) - S1 / (B^2 W) (``fair=False``: the CRPS of the empirical
      distribution of the members; with B = 1 the weighted mean absolute error),
      ``member_mae`` = S0 / (B W), the mean absolute error of a member, and
      ``member_distance`` = 2 S1 / (B (B - 1) W), the mean distance between two different members (NaN for B = 1),
    the same over all snapshots as ``*_total`` (G,), the raw ``sums`` (G, 2, T), ``rank_hist`` (G, B + 1) int64 (how
    many selected, finite elements had r members below the analysis; flat for a calibrated ensemble), ``weight``
    (G,), ``rows`` and ``masked_rows`` (G,) as :func:`verify_blocks`, and with ``want_rows`` the list ``row_crps``
    of per-row vectors of the local blocks: the CRPS over time of every grid point (unweighted).

    Row shards: ONE ``comm.allreduce_sum_`` of the stacked ``[sums, hist, W, rows, masked]`` per call.  A rank
    without blocks still takes part.  The counts travel as fp64: exact below 2^53 per bin."""
    kern = _kern(kern)
    if Cm.dim() != 3:
        raise ValueError(f"crps_blocks: Cm must be (B, T, k), got {tuple(Cm.shape)}")
    B, T = int(Cm.shape[0]), int(Cm.shape[1])
    if fair and B < 2:
        raise ValueError(f"crps_blocks: the fair estimator needs B >= 2 members, got {B} (pass fair=False)")
    Cp = _pitched_dev(kern, Cm)
    (sums, rank_hist), (W, rows, masked), row_sums = _grid_sums(
        "crps_blocks", "crps_allreduce", comm, Ublocks, Xblocks, T, delay, Cm.device,
        {"means": means, "stds": stds, "weights": weights},
        lambda G, dev: (torch.zeros((G, 2, T), dtype=torch.float64, device=dev),
                        torch.zeros((G, B + 1), dtype=torch.int64, device=dev)),
        lambda acc, U, E, v, g: _crps(kern, U, Cp, E, v["means"], v["stds"], v["weights"], acc[0][g], acc[1][g],
                                      want_rows)[1],
        groups, n_groups, want_rows)
    rank_hist = rank_hist.round().to(torch.int64)          # (the counts travelled as fp64)
    npairs = float(B * (B - 1))

    def scores(S, Wn):
        S0, S1 = S[:, 0], S[:, 1]
        mae = S0 / (B * Wn)
        dist = 2.0 * S1 / (npairs * Wn) if B > 1 else torch.full_like(mae, float("nan"))
        crps = mae - S1 / ((npairs if fair else float(B * B)) * Wn)
        return {"crps": crps, "member_mae": mae, "member_distance": dist}

    res = scores(sums, W[:, None])
    res.update({f"{key}_total": v for key, v in scores(sums.sum(dim=2), W * T).items()})
    res.update(sums=sums, rank_hist=rank_hist, weight=W, rows=rows.to(torch.int64), masked_rows=masked.to(torch.int64))
    if want_rows:
        div = npairs if fair else float(B * B)
        res["row_crps"] = [R[0] / (B * T) - R[1] / (div * T) for R in row_sums]
    return res


def _threshold_tables(thresholds, nblocks, who):
    """The per-block threshold tables as (J, S, rows) fp32 (a (J, rows) table has one slot) -> (tables, J, S).  A
    rank without blocks has no table to learn J from and passes the number J itself."""
    if isinstance(thresholds, int):
        if nblocks or thresholds < 1:
            raise ValueError(f"{who}: thresholds = {thresholds}: the number J >= 1 stands for the tables only where there "
                             "are no blocks")
        return [], int(thresholds), 1
    tabs = [torch.as_tensor(t).to(torch.float32) for t in thresholds]
    tabs = [t.unsqueeze(1) if t.dim() == 2 else t for t in tabs]
    if len(tabs) != nblocks:
        raise ValueError(f"{who}: {len(tabs)} threshold tables for {nblocks} blocks")
    if any(t.dim() != 3 or t.shape[:2] != tabs[0].shape[:2] or t.shape[0] < 1 or t.shape[1] < 1 for t in tabs):
        raise ValueError(f"{who}: every threshold table must be (J, S, rows) or (J, rows) with the same J >= 1 and S >= 1, "
                         f"got {[tuple(t.shape) for t in tabs]}")
    if not tabs:
        raise ValueError(f"{who}: no threshold table: a rank without blocks passes the number of thresholds J")
    return tabs, int(tabs[0].shape[0]), int(tabs[0].shape[1])


def _slot_labels(slot, S, T, device, who):
    """The slot of every snapshot as device int32, or None for one slot; labels outside 0 .. S - 1 are a ValueError."""
    if slot is None:
        if S != 1:
            raise ValueError(f"{who}: the thresholds have {S} slots, so slot must name one per snapshot")
        return None
    sl = torch.as_tensor(slot).reshape(-1).cpu()
    if sl.dtype.is_floating_point or sl.numel() != T or int(sl.min()) < 0 or int(sl.max()) >= S:
        raise ValueError(f"{who}: slot must hold {T} integer labels in 0 .. {S - 1}")
    return sl.to(device=device, dtype=torch.int32).contiguous()


def exceed_prob_blocks(Ublocks, Cm: torch.Tensor, thresholds, slot=None, above: bool = True, means=None, stds=None,
                       delay_block: int | None = None, out=None, delay: int = 1, kern=None) -> list[torch.Tensor]:
    """The exceedance probability of every row block: a list of (J, T, rows) fp32 tensors, the share of the B member
    fields ``mean + std * (U Cm[b])`` above (``above=False``: below) threshold j -- per grid point and time (K24; no
    member field is stored).  NaN where a member is not finite.  ``thresholds``: per block a (J, S, rows) or (J, rows)
    table over the PHYSICAL rows (``Climatology.thresholds``), ``slot``: the slot 0 .. S - 1 of every snapshot of
    ``Cm`` (None with one slot).  The comparison is strict: a member that equals the threshold is no event.
    ``means``, ``stds``, ``delay``, ``delay_block`` as in :func:`expand_blocks`; ``out``: a list of contiguous
    (J, T, rows) fp32 tensors to write into.  ``[P[j] for P in result]`` is an ``Xblocks`` of
    :func:`pack_field_blocks`."""
    kern = _kern(kern)
    Ublocks = list(Ublocks)
    tabs, J, S = _threshold_tables(thresholds, len(Ublocks), "exceed_prob_blocks")
    Cp = _pitched_dev(kern, Cm)
    sl = _slot_labels(slot, S, int(Cm.shape[1]), Cm.device, "exceed_prob_blocks")
    res = []
    for b, U in enumerate(Ublocks):
        Ub, reps = _block_rows(U, delay, delay_block)
        th = tabs[b].to(Ub.device)
        th = (th.repeat(1, 1, reps) if reps > 1 else th).contiguous()
        if th.shape[2] != Ub.shape[1]:
            raise ValueError(f"exceed_prob_blocks: thresholds[{b}] has {int(tabs[b].shape[2])} rows, the block "
                             f"{int(Ub.shape[1]) // reps}")
        res.append(_exceed_prob(kern, Ub, Cp, th, sl, above, _vec(means, b, reps, Ub.device),
                                _vec(stds, b, reps, Ub.device), out=None if out is None else out[b]))
    return res


def exceed_blocks(Ublocks, Cm: torch.Tensor, Xblocks, thresholds, slot=None, above: bool = True, means=None, stds=None,
                  weights=None, groups=None, delay: int = 1, comm: Comm | None = None, want_rows: bool = False, kern=None,
                  n_groups: int | None = None) -> dict:
    """The exceedance probability p = (members beyond the threshold) / B of the B member forecasts
    ``mean + std * (U c_b)`` scored against the snapshots ``Xblocks`` (the analysis) on the grid, without storing a
    member field (K24): Brier score, reliability diagram and ROC area, per group of rows and threshold.

    ``Cm``: (B, T, k) fp32, :func:`member_coefficients`.  ``thresholds``: per block a (J, S, rows) or (J, rows) table
    over the PHYSICAL rows (``Climatology.thresholds``), repeated for every delay like ``means`` (a rank without
    blocks passes the number J instead: the collective needs it); ``slot``: the slot 0 .. S - 1 of every (embedded)
    snapshot, None with one slot; ``above``: the event is value > threshold, otherwise value < threshold -- strict, a
    tie is no event, a NaN threshold gives none.  ``Xblocks``, ``means``, ``stds``, ``weights``, ``groups``,
    ``delay``, ``n_groups`` exactly as in :func:`verify_blocks`.

    With o the outcome (1 where the analysis is in the event), S0 .. S3 = sum w ((p - o)^2, o, p, p^2) over the rows
    of a group and W = the sum of its weights, returns per group, threshold and snapshot (G, J, T)
      ``brier`` = S0 / W, ``brier_fair`` = S0 / W - (S2 - S3) / ((B - 1) W) (Ferro's correction for the ensemble
      size: unbiased for the score of the underlying probability; NaN for B = 1), ``base_rate`` = S1 / W,
      ``forecast_rate`` = S2 / W, ``brier_skill`` = 1 - brier / (base_rate (1 - base_rate)),
    the same over all snapshots as ``*_total`` (G, J), and from the counts N[o, c] of selected, finite elements with
    outcome o and c members in the event (``counts`` (G, J, 2, B + 1) int64, unweighted):
      ``bin_counts`` = N_c = N[0, c] + N[1, c] and ``reliability`` = N[1, c] / N_c (G, J, B + 1): the observed
      frequency where c / B was forecast (NaN for an empty bin),
      ``reliability_term`` = sum_c N_c (c / B - O_c / N_c)^2 / N, ``resolution_term`` = sum_c N_c (O_c / N_c - O / N)^2
      / N and ``uncertainty`` = (O / N) (1 - O / N) (G, J): Murphy's decomposition, Brier = reliability - resolution +
      uncertainty for unit weights,
      ``roc_area`` (G, J): the area under the hit rate against the false alarm rate of the B + 1 decisions "at least
      c members", joined by trapezoids from (0, 0) to (1, 1) (NaN unless both outcomes occur),
    the raw ``sums`` (G, J, 4, T), ``weight`` (G,), ``rows`` and ``masked_rows`` (G,) as :func:`verify_blocks`, and
    with ``want_rows`` the list ``row_brier`` of (J, rows) tensors of the local blocks: the Brier score over time of
    every grid point (unweighted).

    Row shards: ONE ``comm.allreduce_sum_`` of the stacked ``[sums, counts, W, rows, masked]`` per call.  A rank
    without blocks still takes part.  The counts travel as fp64: exact below 2^53 per bin."""
    kern = _kern(kern)
    if Cm.dim() != 3:
        raise ValueError(f"exceed_blocks: Cm must be (B, T, k), got {tuple(Cm.shape)}")
    B, T = int(Cm.shape[0]), int(Cm.shape[1])
    Ublocks = list(Ublocks)
    tabs, J, S = _threshold_tables(thresholds, len(Ublocks), "exceed_blocks")
    sl = _slot_labels(slot, S, T, Cm.device, "exceed_blocks") if Ublocks else None
    Cp = _pitched_dev(kern, Cm)
    vecs = {"means": means, "stds": stds, "weights": weights, "thresholds": tabs}

    def launch(acc, U, E, v, g):        # (the row range of the table is copied once: the kernel takes a dense one)
        return _exceed(kern, U, Cp, E, v["thresholds"].contiguous(), sl, above, v["means"], v["stds"], v["weights"],
                       acc[0][g], acc[1][g], want_rows)[1]

    (sums, counts), (W, rows, masked), row_sums = _grid_sums(
        "exceed_blocks", "exceed_allreduce", comm, Ublocks, Xblocks, T, delay, Cm.device, vecs,
        lambda G, dev: (torch.zeros((G, J, 4, T), dtype=torch.float64, device=dev),
                        torch.zeros((G, J, 2, B + 1), dtype=torch.int64, device=dev)),
        launch, groups, n_groups, want_rows)
    counts = counts.round().to(torch.int64)          # (the counts travelled as fp64)

    def scores(Sm, Wn):
        S0, S1, S2, S3 = (Sm[:, :, q] for q in range(4))
        brier, base = S0 / Wn, S1 / Wn
        fair = brier - (S2 - S3) / ((B - 1) * Wn) if B > 1 else torch.full_like(brier, float("nan"))
        return {"brier": brier, "brier_fair": fair, "base_rate": base, "forecast_rate": S2 / Wn,
                "brier_skill": 1.0 - brier / (base * (1.0 - base))}

    res = scores(sums, W[:, None, None])
    res.update({f"{key}_total": v for key, v in scores(sums.sum(dim=3), (W * T)[:, None]).items()})
    N = counts.to(torch.float64)
    Nc, Oc = N.sum(dim=2), N[:, :, 1]
    Ntot, freq = Nc.sum(dim=2), Oc / Nc                                  # (an empty bin: 0 / 0 = NaN)
    obar = Oc.sum(dim=2) / Ntot
    f0 = torch.where(Nc > 0, freq, torch.zeros_like(freq))
    pc = torch.arange(B + 1, dtype=torch.float64, device=N.device) / B
    z = torch.zeros(N.shape[:2] + (1,), dtype=torch.float64, device=N.device)
    far = torch.cat([z, torch.cumsum(N[:, :, 0].flip(2), dim=2) / N[:, :, 0].sum(dim=2, keepdim=True)], dim=2)
    hit = torch.cat([z, torch.cumsum(N[:, :, 1].flip(2), dim=2) / N[:, :, 1].sum(dim=2, keepdim=True)], dim=2)
    res.update(reliability=freq, bin_counts=Nc.to(torch.int64),
               reliability_term=(Nc * (pc - f0) ** 2).sum(dim=2) / Ntot,
               resolution_term=(Nc * (f0 - obar[:, :, None]) ** 2).sum(dim=2) / Ntot,
               uncertainty=obar * (1.0 - obar),
               roc_area=(0.5 * (hit[:, :, 1:] + hit[:, :, :-1]) * (far[:, :, 1:] - far[:, :, :-1])).sum(dim=2),
               sums=sums, counts=counts, weight=W, rows=rows.to(torch.int64), masked_rows=masked.to(torch.int64))
    if want_rows:
        res["row_brier"] = [R[:, 0] / T for R in row_sums]
    return res


def _group_pieces(groups, rows, reps, n_groups, who):
    """-> (pieces, G): per block the list of (first row, one past the last row, group) of its launches.  ``rows``:
    the physical rows of every block, each label vector repeated for the ``reps`` delays of its block."""
    if groups is None:
        return [[(0, r * j, 0)] for r, j in zip(rows, reps)], (1 if n_groups is None else int(n_groups))
    runs = [_runs(g) for g in groups]
    if len(runs) != len(rows):
        raise ValueError(f"{who}: {len(runs)} label vectors for {len(rows)} blocks")
    labels = [g for r in runs for _, _, g in r]
    if labels and min(labels) < 0:
        raise ValueError(f"{who}: group labels must be >= 0")
    G = max(labels) + 1 if labels else 1
    if n_groups is not None:
        if G > n_groups and labels:
            raise ValueError(f"{who}: label {G - 1} with n_groups = {n_groups}")
        G = int(n_groups)
    for b, (r, mb) in enumerate(zip(runs, rows)):
        if sum(e - s for s, e, _ in r) != mb:
            raise ValueError(f"{who}: groups[{b}] has {sum(e - s for s, e, _ in r)} labels, the block {mb} rows")
    return [[(j * mb + s, j * mb + e, g) for s, e, g in r for j in range(reps_b)]
            for r, mb, reps_b in zip(runs, rows, reps)], G


def _range_pieces(pieces, G, device, range_fn, state=None):
    """The range pass over the launches ``pieces``, merged into ``state`` = (range (G, 2) fp32, count (G, 1) int64)
    device tensors of an earlier pass (time slabs); nothing is synchronised."""
    if state is None:
        state = (torch.tensor([[float("inf"), float("-inf")]] * G, dtype=torch.float32, device=device),
                 torch.zeros((G, 1), dtype=torch.int64, device=device))
    rng, cnt = state
    for b, ps in enumerate(pieces):
        for s, e, g in ps:
            range_fn(b, s, e, (rng[g], cnt[g]))
    return state


def _packings(packing, G, who):
    if isinstance(packing, Packing):
        return [packing] * G
    packing = list(packing)
    if len(packing) != G or not all(isinstance(p, Packing) for p in packing):
        raise ValueError(f"{who}: {len(packing)} packings for {G} groups (a Packing, or a list of one per group)")
    return packing


def _pack_pieces(pieces, G, shapes, device, packing, out, range_fn, pack_fn, who, counts=None):
    """The two passes of :func:`pack_blocks` / :func:`pack_field_blocks` over the launches ``pieces``.  ``counts``: a
    (G, 2) int64 device tensor of an earlier call to add to (time slabs); the result then holds its running sums."""
    rng = None
    if packing is None:
        rng = _range_pieces(pieces, G, device, range_fn)[0].cpu()      # the one synchronisation of the range pass
        packing = [Packing.for_range(lo, hi) for lo, hi in rng.tolist()]
    else:
        packing = _packings(packing, G, who)
    if out is not None:
        out = list(out)
        for b, shp in enumerate(shapes):
            if tuple(out[b].shape) != shp or out[b].dtype != torch.int16:
                raise ValueError(f"{who}: out[{b}] must be a {shp} int16 tensor, got {out[b].dtype} {tuple(out[b].shape)}")
    codes = out if out is not None else [torch.empty(shp, dtype=torch.int16, device=device) for shp in shapes]
    if counts is None:
        counts = torch.zeros((G, 2), dtype=torch.int64, device=device)
    for b, ps in enumerate(pieces):
        for s, e, g in ps:
            pack_fn(b, s, e, packing[g], codes[b][:, s:e], counts[g])
    host = counts.cpu()
    return {"codes": codes, "packing": packing, "range": rng, "filled": host[:, 0].clone(),
            "saturated": host[:, 1].clone(), "counts": counts}


def _expand_setup(kern, Ublocks, Ct, means, stds, groups, delay_block, delay, n_groups, who):
    views = [_block_rows(U, delay, delay_block) for U in Ublocks]
    rows = [int(U.shape[1]) // reps for U, reps in views]
    pieces, G = _group_pieces(groups, rows, [reps for _, reps in views], n_groups, who)
    Cp = _pitched(kern, Ct)
    vecs = [(_vec(means, b, reps, U.device), _vec(stds, b, reps, U.device)) for b, (U, reps) in enumerate(views)]
    for b, ((U, _), (mean, std)) in enumerate(zip(views, vecs)):
        for name, v in (("means", mean), ("stds", std)):
            if v is not None and v.numel() != U.shape[1]:
                raise ValueError(f"{who}: {name}[{b}] does not match the {int(U.shape[1])} rows of the block")
    cut = (lambda v, s, e: None if v is None else v[s:e])
    args = (lambda b, s, e: (views[b][0][:, s:e], Cp, cut(vecs[b][0], s, e), cut(vecs[b][1], s, e)))
    return views, pieces, G, args


def range_blocks(Ublocks, Ct: torch.Tensor, means=None, stds=None, groups=None, delay_block: int | None = 0,
                 delay: int = 1, kern=None, n_groups: int | None = None, state=None):
    """The range pass of :func:`pack_blocks` on its own: -> ``state`` = (range (G, 2) fp32, count (G, 1) int64) device
    tensors -- minimum / maximum of the finite values of ``mean + std * (U c)`` and the number of non-finite ones
    per group, no field stored -- merged into the ``state`` of an earlier call (chunks of the time axis).  Nothing is
    synchronised; ``Packing.for_range(*state[0][g].tolist())`` is the packing of group g."""
    kern = _kern(kern)
    Ublocks = list(Ublocks)
    _, pieces, G, args = _expand_setup(kern, Ublocks, Ct, means, stds, groups, delay_block, delay, n_groups, "range_blocks")
    dev = Ublocks[0].device if Ublocks else Ct.device
    return _range_pieces(pieces, G, dev, lambda b, s, e, o: _expand_range(kern, *args(b, s, e), o), state)


def pack_blocks(Ublocks, Ct: torch.Tensor, means=None, stds=None, groups=None, packing=None,
                delay_block: int | None = 0, delay: int = 1, out=None, kern=None, n_groups: int | None = None,
                comm: Comm | None = None, counts=None) -> dict:
    """The fields ``mean + std * (U c)`` of every row block as CF-packed int16 codes, one packing per group of rows,
    the fp32 fields never stored (K17).

    ``means``, ``stds``, ``delay``, ``delay_block`` as in :func:`expand_blocks` (``delay_block=0``, the default, packs
    the physical fields).  ``groups`` as in :func:`verify_blocks`: per block an integer label vector over the
    physical rows -- one variable of the file is one group; a group may come in several runs and may be absent
    from a block (every run is one launch on a row range).  None: one group.  ``n_groups``: G.
    ``packing``: None runs a range pass first (the coefficients are expanded twice, nothing is stored) and packs
    group g with ``Packing.for_range`` of its finite values; a :class:`Packing` or a list of G of them is taken as
    it is and the range pass is skipped -- the forecast written with the analysis file's own ``scale_factor`` /
    ``add_offset``: one pass, directly comparable codes, and ``saturated`` says what did not fit.
    ``out``: per block a (T, rows) int16 view to write into (any row stride: a time slab of a staging buffer).

    Returns ``codes`` (per block a (T, rows) int16 device tensor, or the views of ``out``), ``packing`` (a list of
    G), ``range`` ((G, 2) fp32 minimum / maximum of the finite values; None with a given packing), ``filled`` and
    ``saturated`` ((G,) int64: the non-finite values, which became the fill code -32768, and the values the clamp
    to -32767 .. 32767 caught) and ``counts`` (the (G, 2) int64 device tensor behind the two; handed back in as
    ``counts=`` by a caller that walks the time axis in slabs, it keeps running sums).

    Row shards: the range of a group is a minimum / maximum over all ranks and ``Comm`` has no such collective:
    with a ``comm`` of more than one rank pass the ``packing``; ``filled`` / ``saturated`` are this rank's."""
    kern = _kern(kern)
    if comm is not None and comm.world_size > 1 and packing is None:
        raise ValueError("pack_blocks: the range pass is single-process; with a comm of more than one rank pass the "
                         "packing (a Packing per group)")
    Ublocks = list(Ublocks)
    T = int(Ct.shape[0])
    views, pieces, G, args = _expand_setup(kern, Ublocks, Ct, means, stds, groups, delay_block, delay, n_groups,
                                           "pack_blocks")
    dev = Ublocks[0].device if Ublocks else Ct.device
    shapes = [(T, int(U.shape[1])) for U, _ in views]
    return _pack_pieces(pieces, G, shapes, dev, packing, out,
                        lambda b, s, e, o: _expand_range(kern, *args(b, s, e), o),
                        lambda b, s, e, pk, o, c: _expand_pack(kern, *args(b, s, e), pk, o, c), "pack_blocks", counts)


def pack_field_blocks(Xblocks, groups=None, packing=None, out=None, kern=None, n_groups: int | None = None,
                      counts=None) -> dict:
    """:func:`pack_blocks` of fields that exist: ``Xblocks`` a list of (T, rows) fp32 tensors -- the K15 spread, an
    ensemble mean, real snapshots.  ``groups``, ``packing``, ``out``, ``n_groups`` and the result as there."""
    kern = _kern(kern)
    Xblocks = list(Xblocks)
    pieces, G = _group_pieces(groups, [int(X.shape[1]) for X in Xblocks], [1] * len(Xblocks), n_groups,
                              "pack_field_blocks")

    def range_fn(b, s, e, o):
        _field_range(kern, Xblocks[b][:, s:e], o)

    def pack_fn(b, s, e, pk, o, c):
        _field_pack(kern, Xblocks[b][:, s:e], pk, o, c)

    shapes = [tuple(int(n) for n in X.shape) for X in Xblocks]
    dev = Xblocks[0].device if Xblocks else torch.device("cpu")
    return _pack_pieces(pieces, G, shapes, dev, packing, out, range_fn, pack_fn, "pack_field_blocks", counts)


def range_field_blocks(Xblocks, groups=None, kern=None, n_groups: int | None = None, state=None):
    """:func:`range_blocks` of fields that exist (``Xblocks`` as in :func:`pack_field_blocks`)."""
    kern = _kern(kern)
    Xblocks = list(Xblocks)
    pieces, G = _group_pieces(groups, [int(X.shape[1]) for X in Xblocks], [1] * len(Xblocks), n_groups,
                              "range_field_blocks")
    dev = Xblocks[0].device if Xblocks else torch.device("cpu")
    return _range_pieces(pieces, G, dev, lambda b, s, e, o: _field_range(kern, Xblocks[b][:, s:e], o), state)


def _masked_count(masks, b, device) -> torch.Tensor:
    """Block b of a list of ``space_mask`` vectors (1 = used, 0 = masked) as the int32 count K20 takes: != 0 at the
    masked rows."""
    return (torch.as_tensor(masks[b]).to(device).reshape(-1) == 0).to(torch.int32).contiguous()


def mask_weights(weights, masks) -> list:
    """The per-block row weights of :func:`verify_blocks` / :func:`crps_blocks` with the masked grid points left
    out: ``weights`` (per block the weight of every physical row; None: all ones) with 0 where ``masks`` (per block
    the ``space_mask`` of its physical rows, 1 = used in the decomposition) is 0.  A row with weight 0 is selected
    out of every score, whatever it holds -- the NaN that the mean of a masked point is."""
    out = []
    for b, m in enumerate(masks):
        used = torch.as_tensor(m).reshape(-1) != 0
        w = torch.ones(used.shape, dtype=torch.float32, device=used.device) if weights is None else \
            torch.as_tensor(weights[b]).to(device=used.device, dtype=torch.float32).reshape(-1)
        if w.shape != used.shape:
            raise ValueError(f"mask_weights: block {b} has {w.numel()} weights and {used.numel()} mask entries")
        out.append(torch.where(used, w, torch.zeros_like(w)))
    return out


def project_blocks(Ublocks, Xblocks, means=None, stds=None, delay: int = 1, comm: Comm | None = None, kern=None,
                   shape: tuple[int, int] | None = None, masks=None) -> dict:
    """The coefficients of raw snapshots in the basis U: ``c_t = U^T ((x_t - mean) / std)``, X read once and
    no standardised copy made (K13).  The snapshots need not be the ones U was computed from.

    ``Xblocks``: the (n, rows) snapshot blocks that belong to ``Ublocks`` (any iterable, consumed once in
    order); with ``delay`` d > 1 the zero-copy embedded view (n - d + 1, d * rows) of every block is
    projected.  ``means`` / ``stds``: lists of per-row vectors of the PHYSICAL rows of every block (None:
    0 / 1), repeated for every delay; a std with a zero entry is refused (ValueError) before any launch.
    ``masks``: per block the ``space_mask`` of its physical rows (1 = used, 0 = masked: the result of
    ``missing = "mask"``).  The masked rows are missing in the new snapshots as well: they are SET TO 0 IN PLACE in
    the blocks handed in (K20; rows that are used are not touched), and their mean / std entries -- NaN in such a
    result -- are taken as 0 / 1, so that K13 never sees a NaN and the energy counts the used points only.
    Returns ``Ct`` (T, k) fp64, per snapshot ``energy`` = ||(x - mean) / std||^2 and ``captured`` =
    ||c_t||^2 / energy_t, the totals ``captured_total`` = sum ||c||^2 / sum energy and ``energy_total``, and
    ``rows`` (global).

    ``1 - captured`` is a difference of two sums of m terms each and resolves nothing below ~1e-7: the
    accurate out-of-sample residual is ``score_blocks(Ublocks, Ct.float(), Xblocks, ...)``, which sums the
    squared residuals themselves.

    Row shards: ONE ``comm.allreduce_sum_`` of the stacked ``[Ct, energy, rows]`` per call, whatever the
    number of local blocks.  A rank without blocks still takes part; it cannot know the sizes and states
    them as ``shape = (T, k)``."""
    kern = _kern(kern)
    comm = comm or Comm()
    if stds is not None:
        zeros = sum(int((torch.as_tensor(v) == 0).sum()) for v in stds)
        if zeros:
            raise ValueError(f"project_blocks: {zeros} entries of std are zero: (x - mean) / std is not defined for "
                             "those rows (constant rows are kept out of the decomposition)")
    acc, rows_local, T, k, dev = None, 0, None, None, None
    for b, (U, X) in enumerate(zip(Ublocks, Xblocks, strict=True)):   # (a streamed X that ends early is an error)
        E = embed_view(X, delay)
        if T is None:
            T, k, dev = int(E.shape[0]), int(U.shape[0]), U.device
            if shape is not None and tuple(shape) != (T, k):
                raise ValueError(f"project_blocks: shape = {tuple(shape)} stated, the blocks give {(T, k)}")
        if E.shape != (T, U.shape[1]) or U.shape[0] != k:
            raise ValueError(f"project_blocks: block {b} of X is {tuple(E.shape)} (delay {delay}) and of U "
                             f"{tuple(U.shape)}; {(T, int(U.shape[1]))} and {(k, int(U.shape[1]))} asked for")
        mu, sd = _block_vecs({"means": means, "stds": stds}, b, delay, int(U.shape[1]) // delay, U.device,
                             "project_blocks").values()
        if masks is not None:
            cnt = _masked_count(masks, b, X.device)
            row_mask_apply_(kern, X, cnt, 0.0)                         # (the physical block: every delay sees the zeros)
            on = (cnt != 0).to(U.device).repeat(delay)
            mu = None if mu is None else mu.masked_fill(on, 0.0)
            sd = None if sd is None else sd.masked_fill(on, 1.0)
        acc = _project(kern, U, E, mu, sd, acc)
        rows_local += int(U.shape[1])
    if acc is None:        # a rank without blocks still takes part in the collective
        if shape is None:
            raise ValueError("project_blocks: no blocks and no shape = (T, k)")
        T, k = int(shape[0]), int(shape[1])
        dev = torch.device("cuda" if getattr(kern, "name", "") == "hip" else "cpu")
        acc = (torch.zeros((T, k), dtype=torch.float64, device=dev), torch.zeros(T, dtype=torch.float64, device=dev))
    Ct, energy = acc
    flat = torch.cat([Ct.reshape(-1), energy, torch.tensor([float(rows_local)], dtype=torch.float64, device=Ct.device)])
    flat = comm.allreduce_sum_(flat, tag="project_allreduce")
    Ct, energy, rows = flat[:T * k].reshape(T, k), flat[T * k:T * k + T], float(flat[T * k + T])
    c2 = (Ct * Ct).sum(dim=1)
    e_total = energy.sum()
    return {"Ct": Ct, "energy": energy, "captured": c2 / energy, "captured_total": float(c2.sum() / e_total),
            "energy_total": float(e_total), "rows": int(rows)}


def _climatology_args(climatology, times, who: str, trend=None) -> None:
    if trend is None and (climatology is None) != (times is None):
        raise ValueError(f"{who}: climatology and times go together (the datetime64 stamps say which slot a "
                         "snapshot takes)")
    if trend is not None and times is None:
        raise ValueError(f"{who}: trend and times go together (the datetime64 stamps are what the design is formed at)")


# ---------------------------------------------------------------------------
# the bundle a user holds
# ---------------------------------------------------------------------------
@dataclass
class DmdForecast:
    """U blocks + pre-processing + a fitted optimized DMD: fields and scores at any times.

    ``Ublocks``: (k, d * rows) blocks of the left singular vectors; ``means`` / ``stds``: per-row
    vectors of the physical rows of every block, or None; ``delay``: d; ``result``: the
    :class:`OptDMDResult` fitted on ``reduced_coordinates(s, Vh)``; ``s`` / ``Vh``: the SVD factors
    (only :meth:`reconstruct_svd` needs them); ``masks``: per block the ``space_mask`` of its physical rows (the
    result of ``missing = "mask"``; 1 = used), which :meth:`project` and :meth:`restart` hand to
    :func:`project_blocks`, or None."""

    Ublocks: list
    result: OptDMDResult | None = None
    means: list | None = None
    stds: list | None = None
    delay: int = 1
    s: torch.Tensor | None = None
    Vh: torch.Tensor | None = None
    kern: object = None
    masks: list | None = None

    def coefficients(self, t) -> tuple[torch.Tensor, float]:
        if self.result is None:
            raise ValueError("DmdForecast: no fitted DMD result")
        Ct, imag = dmd_coefficients(self.result, t)
        k = int(self.Ublocks[0].shape[0])
        if Ct.shape[1] != k:
            raise ValueError(f"DmdForecast: the DMD was fitted on {Ct.shape[1]} coordinates, U has {k} columns")
        return Ct.to(self.Ublocks[0].device), imag

    def fields(self, t, delay_block: int | None = 0, out=None, climatology=None, times=None, trend=None,
               trend_extra=None) -> list[torch.Tensor]:
        """The model's fields at the times ``t``: (len(t), rows) per block; ``delay_block=0`` (the
        default) the physical rows, None all d * rows of the embedding.
        ``climatology``: a :class:`climatology.Climatology` the model was fitted on the anomalies of; its fields at
        ``times`` (the datetime64 stamps of ``t``) are put back in place (K18), so that full fields come out.
        ``trend``: a :class:`trend.Trend` that was removed (after the climatology) before the fit; it is evaluated at
        the same ``times`` (``trend_extra``: its user series there, if it has any) and put back in place (K21) before
        the climatology."""
        if self.delay == 1:
            delay_block = None
        _climatology_args(climatology, times, "DmdForecast.fields", trend)
        if (climatology is not None or trend is not None) and delay_block is None and self.delay > 1:
            raise ValueError("DmdForecast.fields: a climatology or a trend lives on the physical rows; pass a delay_block")
        res = expand_blocks(self.Ublocks, self.coefficients(t)[0], self.means, self.stds, delay_block, out=out,
                            delay=self.delay, kern=self.kern)
        if trend is not None:
            trend.restore_(res, times, extra=trend_extra)
        if climatology is not None:
            climatology.restore_(res, times)
        return res

    def score(self, Xblocks, t, comm: Comm | None = None, want_rows: bool = False) -> dict:
        """:func:`score_blocks` of the model at the times ``t`` of the snapshots ``Xblocks`` (with a
        delay d the blocks hold len(t) + d - 1 snapshots); ``imag_ratio`` is added to the result."""
        Ct, imag = self.coefficients(t)
        res = score_blocks(self.Ublocks, Ct, Xblocks, self.means, self.stds, self.delay, comm, want_rows, self.kern)
        res["imag_ratio"] = imag
        return res

    def verify(self, Xblocks, t, weights=None, clims=None, groups=None, comm: Comm | None = None,
               want_rows: bool = False, ensemble: bool = False, n_groups: int | None = None, climatology=None,
               times=None, trend=None, trend_extra=None) -> dict:
        """:func:`verify_blocks` of the model at the times ``t`` against the snapshots ``Xblocks`` (with a delay d
        the blocks hold len(t) + d - 1 snapshots): weighted RMSE, bias and anomaly correlation per group.
        ``ensemble=True`` verifies the ensemble mean of a bagged fit (``Cbar`` of :meth:`ensemble_coefficients`).
        ``climatology``: a :class:`climatology.Climatology` the model was fitted on the anomalies of.  The analysis
        is anomalised against it into a scratch copy per block (``times``: the datetime64 stamps of the snapshots of
        ``Xblocks``) and ``clims`` becomes zero: forecast and analysis are both anomalies against the time-dependent
        climatology, which is what the anomaly correlation is defined with.  ``clims`` and ``climatology`` together
        are refused.  ``trend``: a :class:`trend.Trend` that was removed before the fit (``trend_extra``: its user
        series at ``times``): the analysis is detrended in the same scratch copy, after the climatology, and ``clims``
        becomes zero; ``clims`` and ``trend`` together are refused as well.  ``imag_ratio`` is added to the result."""
        _climatology_args(climatology, times, "DmdForecast.verify", trend)
        if climatology is not None or trend is not None:
            if clims is not None:
                raise ValueError("DmdForecast.verify: clims and climatology are two definitions of the anomaly; pass one"
                                 if trend is None else
                                 "DmdForecast.verify: clims and trend are two definitions of the anomaly; pass one")
            Xblocks = list(Xblocks)
            scratch = [torch.empty(tuple(X.shape), dtype=X.dtype, device=X.device) for X in Xblocks]
            if climatology is not None:
                Xblocks = climatology.remove_(Xblocks, times, out=scratch)
            if trend is not None:
                Xblocks = trend.remove_(Xblocks, times, out=None if climatology is not None else scratch,
                                        extra=trend_extra)
            clims = [torch.zeros(int(X.shape[1]), dtype=torch.float32, device=X.device) for X in Xblocks]
        if ensemble:
            Ct, _, imag = self.ensemble_coefficients(t)
        else:
            Ct, imag = self.coefficients(t)
        res = verify_blocks(self.Ublocks, Ct, Xblocks, self.means, self.stds, weights, clims, groups, self.delay, comm,
                            want_rows, self.kern, n_groups)
        res["imag_ratio"] = imag
        return res

    def pack(self, t, groups=None, packing=None, delay_block: int | None = 0, out=None, ensemble: bool = False,
             spread: bool = False, spread_packing=None, spread_out=None, n_groups: int | None = None,
             comm: Comm | None = None) -> dict:
        """:func:`pack_blocks` of the model at the times ``t``: the fields as CF-packed int16 codes, one packing per
        group, no fp32 field stored.  ``ensemble=True`` packs the ensemble mean of a bagged fit (``Cbar`` of
        :meth:`ensemble_coefficients`); with ``spread=True`` the K15 spread of the same times is formed and packed too
        (:func:`pack_field_blocks`, ``spread_packing`` / ``spread_out`` as ``packing`` / ``out``) and returned under
        ``"spread"``.  ``imag_ratio`` is added to the result."""
        if spread and not ensemble:
            raise ValueError("DmdForecast.pack: spread=True needs ensemble=True")
        if self.delay == 1:
            delay_block = None
        if ensemble:
            Ct, Dev, imag = self.ensemble_coefficients(t)
        else:
            Ct, imag = self.coefficients(t)
        res = pack_blocks(self.Ublocks, Ct, self.means, self.stds, groups, packing, delay_block, self.delay, out,
                          self.kern, n_groups, comm)
        res["imag_ratio"] = imag
        if spread:
            if comm is not None and comm.world_size > 1 and spread_packing is None:
                raise ValueError("DmdForecast.pack: with a comm of more than one rank pass spread_packing")
            S = spread_blocks(self.Ublocks, Dev, self.stds, delay_block, delay=self.delay, kern=self.kern)
            if groups is not None and delay_block is None and self.delay > 1:
                groups = [torch.as_tensor(g).reshape(-1).repeat(self.delay) for g in groups]
            res["spread"] = pack_field_blocks(S, groups, spread_packing, spread_out, self.kern, n_groups)
        return res

    def ensemble_coefficients(self, t, ddof: int = 1) -> tuple[torch.Tensor, torch.Tensor, float]:
        """:func:`ensemble_coefficients` of the trials of a bagged fit, on the device of the U blocks."""
        trials = None if self.result is None else getattr(self.result, "trials", None)
        if not trials:
            raise ValueError("DmdForecast: the result holds no trials; fit with bopdmd(..., num_trials > 0, "
                             "keep_trials=True)")
        Cbar, Dev, imag = ensemble_coefficients(trials, t, ddof)
        k = int(self.Ublocks[0].shape[0])
        if Cbar.shape[1] != k:
            raise ValueError(f"DmdForecast: the trials were fitted on {Cbar.shape[1]} coordinates, U has {k} columns")
        dev = self.Ublocks[0].device
        return Cbar.to(dev), Dev.to(dev), imag

    def ensemble_fields(self, t, delay_block: int | None = 0, out=None) -> tuple[list[torch.Tensor], list[torch.Tensor]]:
        """``(mean_blocks, spread_blocks)`` of the bagged fit's trials at the times ``t``: the fields of the
        ensemble-mean coefficients (K12) and the standard deviation (ddof 1) of the member fields per grid
        point and time (K15), (len(t), rows) per block each.  ``out``: a pair of lists of views to write
        into."""
        Cbar, Dev, _ = self.ensemble_coefficients(t)
        if self.delay == 1:
            delay_block = None
        om, osp = (None, None) if out is None else out
        mean = expand_blocks(self.Ublocks, Cbar, self.means, self.stds, delay_block, out=om, delay=self.delay,
                             kern=self.kern)
        spread = spread_blocks(self.Ublocks, Dev, self.stds, delay_block, out=osp, delay=self.delay, kern=self.kern)
        return mean, spread

    def ensemble_score(self, Xblocks, t, comm: Comm | None = None, want_rows: bool = False) -> dict:
        """:func:`score_blocks` of the ENSEMBLE MEAN of the trials against the snapshots ``Xblocks`` at the times
        ``t``, plus the ensemble's ``spread`` / ``spread_total`` (:func:`spread_score_blocks`; ``var``,
        ``var_total`` and with ``want_rows`` ``row_spread`` too) and how they compare: ``spread_skill`` =
        spread / rmse per snapshot and ``spread_skill_total``.  A well calibrated ensemble has a ratio near 1;
        below 1 it is over-confident.  Two launches per block and two collectives."""
        Cbar, Dev, imag = self.ensemble_coefficients(t)
        res = score_blocks(self.Ublocks, Cbar, Xblocks, self.means, self.stds, self.delay, comm, want_rows, self.kern)
        sp = spread_score_blocks(self.Ublocks, Dev, self.stds, self.delay, comm, want_rows, self.kern)
        res["imag_ratio"] = imag
        for key in ("var", "spread", "var_total", "spread_total"):
            res[key] = sp[key]
        if want_rows:
            res["row_spread"] = sp["row_spread"]
        res["spread_skill"] = sp["spread"] / res["rmse"]
        res["spread_skill_total"] = sp["spread_total"] / res["rmse_total"] if res["rmse_total"] > 0.0 else float("inf")
        return res

    def member_coefficients(self, t) -> tuple[torch.Tensor, float]:
        """:func:`member_coefficients` of the trials of a bagged fit, on the device of the U blocks."""
        trials = None if self.result is None else getattr(self.result, "trials", None)
        if not trials:
            raise ValueError("DmdForecast: the result holds no trials; fit with bopdmd(..., num_trials > 0, "
                             "keep_trials=True)")
        Cm, imag = member_coefficients(trials, t)
        k = int(self.Ublocks[0].shape[0])
        if Cm.shape[2] != k:
            raise ValueError(f"DmdForecast: the trials were fitted on {Cm.shape[2]} coordinates, U has {k} columns")
        return Cm.to(self.Ublocks[0].device), imag

    def ensemble_crps(self, Xblocks, t, weights=None, groups=None, comm: Comm | None = None, want_rows: bool = False,
                      fair: bool = True, n_groups: int | None = None) -> dict:
        """:func:`crps_blocks` of the trials of a bagged fit, as an ensemble forecast, against the snapshots
        ``Xblocks`` at the times ``t`` (with a delay d the blocks hold len(t) + d - 1 snapshots): the area-weighted
        CRPS per group and the rank histogram, one launch per block and group run, one collective.
        The CRPS is translation invariant -- it depends on differences of members and analysis only -- so a model
        fitted on anomalies is verified against the anomalised analysis (``Climatology.remove_``) and the score is
        the score of the full fields: there is no ``climatology=`` argument.  ``imag_ratio`` is added to the
        result."""
        Cm, imag = self.member_coefficients(t)
        res = crps_blocks(self.Ublocks, Cm, Xblocks, self.means, self.stds, weights, groups, self.delay, comm, want_rows,
                          fair, self.kern, n_groups)
        res["imag_ratio"] = imag
        return res

    def ensemble_exceedance(self, Xblocks, t, thresholds, slot=None, above: bool = True, weights=None, groups=None,
                            comm: Comm | None = None, want_rows: bool = False, n_groups: int | None = None) -> dict:
        """:func:`exceed_blocks` of the trials of a bagged fit, as an ensemble forecast, against the snapshots
        ``Xblocks`` at the times ``t`` (with a delay d the blocks hold len(t) + d - 1 snapshots): the Brier score of
        the exceedance probability per group and threshold, the reliability diagram and the ROC area, one launch per
        block and group run, one collective.  ``thresholds`` / ``slot``: per block the (J, S, rows) table and the slot
        of every time (``Climatology.thresholds`` / ``Climatology.slots``); a model fitted on anomalies takes
        thresholds of the anomalies (``anomaly=True``) and the anomalised analysis.  ``imag_ratio`` is added to the
        result."""
        Cm, imag = self.member_coefficients(t)
        res = exceed_blocks(self.Ublocks, Cm, Xblocks, thresholds, slot, above, self.means, self.stds, weights, groups,
                            self.delay, comm, want_rows, self.kern, n_groups)
        res["imag_ratio"] = imag
        return res

    def exceedance_fields(self, t, thresholds, slot=None, above: bool = True, delay_block: int | None = 0,
                          out=None) -> list[torch.Tensor]:
        """:func:`exceed_prob_blocks` of the trials of a bagged fit at the times ``t``: per block the (J, T, rows)
        fp32 probability that the forecast field is beyond threshold j, the physical rows by default
        (``delay_block`` as in :meth:`fields`)."""
        Cm, _ = self.member_coefficients(t)
        if self.delay == 1:
            delay_block = None
        return exceed_prob_blocks(self.Ublocks, Cm, thresholds, slot, above, self.means, self.stds, delay_block, out,
                                  self.delay, self.kern)

    def reconstruct_svd(self, n_components: int | None = None, cols=None, delay_block: int | None = 0,
                        out=None) -> list[torch.Tensor]:
        """The rank-``n_components`` SVD reconstruction of the decomposed snapshots ``cols``."""
        if self.s is None or self.Vh is None:
            raise ValueError("DmdForecast.reconstruct_svd needs s and Vh")
        k = int(self.s.numel()) if n_components is None else int(n_components)
        if not 1 <= k <= int(self.s.numel()):
            raise ValueError(f"n_components = {k} outside 1 .. {int(self.s.numel())}")
        Ct = svd_coefficients(self.s[:k], self.Vh[:k], cols).to(self.Ublocks[0].device)
        if self.delay == 1:
            delay_block = None
        return expand_blocks([U[:k] for U in self.Ublocks], Ct, self.means, self.stds, delay_block, out=out,
                             delay=self.delay, kern=self.kern)

    def project(self, Xblocks, comm: Comm | None = None, n_snapshots: int | None = None) -> dict:
        """:func:`project_blocks` of raw snapshots (with a delay d the blocks hold T + d - 1 of them) on this
        bundle's U, means, stds and masks (with masks the masked rows of ``Xblocks`` are set to 0 in place).
        ``n_snapshots``: T, for a rank without blocks."""
        shape = None
        if n_snapshots is not None:
            k = int(self.Ublocks[0].shape[0]) if len(self.Ublocks) else int(self.result.modes.shape[0])
            shape = (int(n_snapshots), k)
        return project_blocks(self.Ublocks, Xblocks, self.means, self.stds, self.delay, comm, self.kern, shape=shape,
                              masks=self.masks)

    def restart(self, Xblocks, t, comm: Comm | None = None, rcond: float = 1e-12) -> "DmdForecast":
        """The fitted model re-started from new snapshots: the amplitudes are re-fitted to the coefficients
        of ``Xblocks`` (raw snapshots at the times ``t``, which need not belong to the training window; one
        snapshot is enough when k >= r), the eigenvalues and the mode shapes are kept:

                b = argmin_b || Phi(t) diag(b) modes^T - C ||_F      over complex b,   C = project(Xblocks).

        Its normal equations are r x r, ``N = (Phi^H Phi) o (modes^H modes)`` and ``rhs_j = (Phi^H C
        conj(modes))_jj``, solved in complex128 through the Hermitian eigen-decomposition of N; directions
        below ``rcond * lambda_max`` (a duplicated eigenvalue, a window too short to tell two apart) are
        dropped and counted in ``info["restart_dropped"]``.  The phase of b_j moves into ``modes[:, j]``:
        ``amplitudes`` stays real and >= 0.  Returns a new bundle sharing ``Ublocks``, ``means`` and ``stds``
        whose result carries the ``rel_error`` of the window fit, ``info["restarted_at"]`` (first and last
        time of the window), ``info["restart_window"]`` (T) and ``info["captured"]`` (how much of the new
        snapshots the basis holds)."""
        if self.result is None:
            raise ValueError("DmdForecast.restart: no fitted DMD result")
        res = self.result
        alpha = res.eigs.to(torch.complex128)
        tt = torch.as_tensor(t, dtype=torch.float64, device=alpha.device).reshape(-1)
        W = res.modes.to(torch.complex128)
        k, r, T = int(W.shape[0]), int(alpha.numel()), int(tt.numel())
        if T * k < r:
            raise ValueError(f"DmdForecast.restart: {T} snapshots x {k} coordinates cannot determine {r} amplitudes")
        proj = project_blocks(self.Ublocks, Xblocks, self.means, self.stds, self.delay, comm, self.kern, shape=(T, k),
                              masks=self.masks)
        C = proj["Ct"].to(device=alpha.device, dtype=torch.complex128)
        phi = _phi(alpha, tt, torch.complex128)
        N = (phi.conj().T @ phi) * (W.conj().T @ W)
        rhs = torch.einsum("tj,tc,cj->j", phi.conj(), C, W.conj())
        lam, Q = torch.linalg.eigh(0.5 * (N + N.conj().T))
        keep = lam > rcond * lam[-1]
        Qk = Q[:, keep]
        b = Qk @ ((Qk.conj().T @ rhs) / lam[keep])
        amp = b.abs()
        phase = torch.where(amp > 0, b / torch.where(amp > 0, amp, torch.ones_like(amp)).to(b.dtype),
                            torch.ones_like(b))
        fit = (phi * b) @ W.T
        nc = float(torch.linalg.norm(C))
        rel = float(torch.linalg.norm(fit - C)) / nc if nc > 0.0 else 0.0
        info = dict(res.info)
        info.update(restart_dropped=int(r - int(keep.sum())), restarted_at=(float(tt[0]), float(tt[-1])),
                    restart_window=T, captured=proj["captured_total"])
        new = OptDMDResult(eigs=res.eigs, modes=(W * phase).to(res.modes.dtype), amplitudes=amp.to(res.amplitudes.dtype),
                           rel_error=rel, n_iter=0, converged=True, eigs_std=res.eigs_std, info=info)
        return DmdForecast(self.Ublocks, new, self.means, self.stds, self.delay, self.s, self.Vh, self.kern, self.masks)
