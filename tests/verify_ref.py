"""numpy double of K16 (dmdx_verify_f32) and the error bounds its tests use.

TEST INFRASTRUCTURE, like tests/expand_ref.py: fp64 arithmetic on the fp32 inputs.  Matrices are the LOGICAL
column-major ones of include/dmdx.h: U (m, k), C (k, T), X (m, T), mu / sigma / w / clim (m,) or None.

The quantities, with xhat = mu + sigma (U C), e = xhat - x, f = xhat - clim, a = x - clim (clim = mu, or 0, when
it is not given):   0: e^2   1: e   2: a   3: f^2   4: a^2   5: f a.
Column sums run over the rows with w != 0 -- a SELECTION, so that a masked row may hold NaN -- and carry the
weight; row sums run over t and carry none.

Bounds (u = 2^-24, derived, not measured).  expand_ref.element_bound is the error of the fp32 xhat.  The fp32
e, f, a differ from the exact ones by at most
  delta_e = element + u |x|          (the error of xhat and the rounding of the difference, as in expand_ref)
  delta_f = element + u |xhat - clim|
  delta_a = u |x - clim|             (both operands are inputs: one rounding)
and a quantity q formed from them from the exact one by at most
  squares   2 |e| delta + delta^2             products  |f| delta_a + |a| delta_f + delta_f delta_a
  linear    delta.
Every term is then rounded once (u |q|), multiplied by the weight (one more u |w q|) and summed in fp32 over at
most R terms in some order ((R - 1) u sum |w q|), fp64 beyond (its 2^-53 terms are far below u):
  |d col_q| <= sum_i w_i |dq| + (R + 3) u sum_i w_i |q|       R = DMDX_VERIFY_FP32_ROWS = 128
  |d row_q| <= sum_t |dq| + (R + 3) u sum_t |q|               R = 16 (the fp32 part of a row sum)
The scores are ratios of these sums; score_bounds propagates the sum bounds through them by intervals.
"""
import numpy as np

import expand_ref as er

U24 = 2.0 ** -24
FP32_ROWS = 128           # DMDX_VERIFY_FP32_ROWS of include/dmdx.h
FP32_COLS = 16
NQ = 6


def _parts(U, C, X, mu, sigma, clim):
    Xh = er.expand64(U, C, mu, sigma)
    x = X.astype(np.float64)
    cl = clim if clim is not None else mu
    cl = 0.0 if cl is None else cl.astype(np.float64)[:, None]
    return Xh - x, Xh - cl, x - cl, x


def _quantities(e, f, a):
    return np.stack([e * e, e, a, f * f, a * a, f * a])            # (6, m, T)


def _weighted_cols(Q, w):
    if w is None:
        return Q.sum(axis=1)
    sel = w != 0
    return (Q[:, sel, :] * w.astype(np.float64)[sel][None, :, None]).sum(axis=1)


def verify64(U, C, X, mu=None, sigma=None, w=None, clim=None):
    """-> (col (6, T), row (6, m)) in fp64; rows with w == 0 are selected out of col."""
    with np.errstate(all="ignore"):
        e, f, a, _ = _parts(U, C, X, mu, sigma, clim)
        Q = _quantities(e, f, a)
        return _weighted_cols(Q, w), Q.sum(axis=2)


def verify_bounds(U, C, X, mu=None, sigma=None, w=None, clim=None):
    """-> bounds of (col (6, T), row (6, m)), the shapes of verify64.  Masked rows must hold finite values here
    (their row bounds are computed too)."""
    e, f, a, x = _parts(U, C, X, mu, sigma, clim)
    el = er.element_bound(U, C, mu, sigma)
    e, f, a = np.abs(e), np.abs(f), np.abs(a)
    de, df, da = el + U24 * np.abs(x), el + U24 * f, U24 * a
    dQ = np.stack([2.0 * e * de + de * de, de, da, 2.0 * f * df + df * df, 2.0 * a * da + da * da,
                   f * da + a * df + df * da])
    Qa = np.abs(_quantities(e, f, a))
    col = _weighted_cols(dQ, w) + (FP32_ROWS + 3) * U24 * _weighted_cols(Qa, w)
    row = dQ.sum(axis=2) + (FP32_COLS + 3) * U24 * Qa.sum(axis=2)
    return col, row


def scores(S, W):
    """The scores of forecast.verify_blocks from sums S (..., 6, T) or (..., 6) [axis -2 or -1 = quantity] and W."""
    S0, S1, S2, S3, S4, S5 = S
    Sf = S1 + S2
    return {"rmse": np.sqrt(S0 / W), "bias": S1 / W, "acc": S5 / np.sqrt(S3 * S4),
            "acc_centred": (S5 - Sf * S2 / W) / np.sqrt((S3 - Sf * Sf / W) * (S4 - S2 * S2 / W)),
            "activity": np.sqrt(S3 / S4), "skill_vs_clim": 1.0 - S0 / S4}


def _ratio_bound(N, dN, A, dA, B, dB):
    """|N' / sqrt(A' B') - N / sqrt(A B)| for |N' - N| <= dN, ...; inf where A - dA or B - dB is not positive."""
    lo = (A - dA) * (B - dB)
    ok = (A - dA > 0) & (B - dB > 0)
    with np.errstate(all="ignore"):
        inv_lo = np.where(ok, 1.0 / np.sqrt(np.where(ok, lo, 1.0)), np.inf)
        return dN * inv_lo + np.abs(N) * (inv_lo - 1.0 / np.sqrt(A * B))


def score_bounds(S, dS, W):
    """Bounds of scores(S, W) when every sum may be off by dS (same shapes, quantity first); W is exact up to
    fp64 rounding.  rmse, activity by intervals; bias linearly; the correlations through _ratio_bound, the centred
    one after propagating dS into its three centred sums."""
    S0, S1, S2, S3, S4, S5 = S
    d0, d1, d2, d3, d4, d5 = dS
    with np.errstate(all="ignore"):
        rm = np.sqrt(S0 / W)
        rmse = np.maximum(np.sqrt((S0 + d0) / W) - rm, rm - np.sqrt(np.maximum(S0 - d0, 0.0) / W))
        Sf, df = S1 + S2, d1 + d2
        N, dN = S5 - Sf * S2 / W, d5 + (np.abs(Sf) * d2 + np.abs(S2) * df + df * d2) / W
        A, dA = S3 - Sf * Sf / W, d3 + (2.0 * np.abs(Sf) * df + df * df) / W
        B, dB = S4 - S2 * S2 / W, d4 + (2.0 * np.abs(S2) * d2 + d2 * d2) / W
        act = np.sqrt(S3 / S4)
        ok = S4 - d4 > 0
        act_b = np.where(ok, np.maximum(np.sqrt((S3 + d3) / np.where(ok, S4 - d4, 1.0)) - act,
                                        act - np.sqrt(np.maximum(S3 - d3, 0.0) / (S4 + d4))), np.inf)
        skill = np.where(ok, d0 / np.where(ok, S4 - d4, 1.0) + S0 * (1.0 / np.where(ok, S4 - d4, 1.0) - 1.0 / S4), np.inf)
    return {"rmse": rmse, "bias": d1 / W, "acc": _ratio_bound(S5, d5, S3, d3, S4, d4),
            "acc_centred": _ratio_bound(N, dN, A, dA, B, dB), "activity": act_b, "skill_vs_clim": skill}


class VerifyDouble:
    """K16's method of a kernel provider on the CPU, for the host-layer tests: numpy fp64 through verify64 above
    (independent of forecast.py's torch fallback), mixed into tests/kernel_double.CpuKernelDouble."""

    verify_max_k = 256

    def verify(self, Ut, Ct, Xt, mean=None, std=None, weight=None, clim=None, out=None, want_rows=False):
        import torch

        def _np(t):
            return None if t is None else t.detach().cpu().numpy()

        col, row = verify64(_np(Ut).T, _np(Ct).T, _np(Xt).T, _np(mean), _np(std), _np(weight), _np(clim))
        cols = torch.from_numpy(col)
        if out is not None:
            out += cols
            cols = out
        return cols, (torch.from_numpy(row) if want_rows else None)
