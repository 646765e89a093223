"""numpy double of K19 (dmdx_crps_f32) and the error bounds its tests use.

TEST INFRASTRUCTURE, like tests/verify_ref.py: fp64 arithmetic on the fp32 inputs.  Matrices are the LOGICAL
column-major ones of include/dmdx.h: U (m, k), C (k, B T) with column b T + t = member b at snapshot t, X (m, T),
mu / sigma / w (m,) or None.

Per element, with x_b = mu + sigma (U C_b) and y = X[i, t]:
  abs = sum_b |x_b - y|      pair = sum_{b < b'} |x_b - x_b'| (NaN where abs is not finite: the kernel's convention)
  rank = #{b : x_b < y}
Column sums run over the rows with w != 0 -- a SELECTION -- and carry the weight; row sums run over t and carry
none; hist counts the ranks of the selected elements with a finite abs.

Bounds (u = 2^-24, derived, not measured).  delta_b = expand_ref.element_bound of member b is the error of the fp32
field x_b.  A computed term of abs differs from the exact one by at most
  delta_b + u (|x_b - y| + delta_b)                  (the error of x_b and the rounding of the difference)
and one of pair by at most
  delta_b + delta_b' + u (|x_b - x_b'| + delta_b + delta_b').
Every term is non-negative, so an fp32 sum of n computed terms in ANY order is off by at most g(n - 1) times their sum,
g(j) = j u / (1 - j u): n = B for abs and n = B (B - 1) / 2 for pair, the longest fp32 chain csrc/crps.hip states
(ONE chain per element).  With E the sum of the term errors and Q the exact quantity
  dq = E + g(n - 1) (Q + E).
Above that the column / row form of verify_ref: the quantity is multiplied by the weight and summed in fp32 over at
most R terms, fp64 beyond:
  |d col_q| <= sum_i w_i dq + (R + 3) u sum_i w_i (q + dq)      R = DMDX_CRPS_FP32_ROWS = 128
  |d row_q| <= sum_t dq + (R + 3) u sum_t (q + dq)              R = 16 (the fp32 part of a row sum)
"""
import numpy as np

import expand_ref as er

U24 = 2.0 ** -24
FP32_ROWS = 128           # DMDX_CRPS_FP32_ROWS of include/dmdx.h
FP32_COLS = 16
NQ = 2
MEMBER_BLOCK = 8          # DMDX_CRPS_MEMBER_BLOCK (k > 128); DMDX_CRPS_MEMBER_BLOCK_SMALL_K = 2 * MEMBER_BLOCK below
MAX_B = 256               # DMDX_CRPS_MAX_B


def pair_chain(B):
    """The longest fp32 chain the kernel forms for `pair`: one accumulator per element over all pairs."""
    return B * (B - 1) // 2


def members64(U, C, T, B, mu=None, sigma=None):
    """-> (B, m, T) fp64 member fields."""
    return np.stack([er.expand64(U, C[:, b * T:(b + 1) * T], mu, sigma) for b in range(B)])


def quantities64(P, X):
    """-> (abs (m, T), pair (m, T), rank (m, T) int64) of the member fields P (B, m, T) against X."""
    B = P.shape[0]
    x = X.astype(np.float64)
    absq = np.zeros(x.shape)
    pair = np.zeros(x.shape)
    for b in range(B):
        absq += np.abs(P[b] - x)
        if b + 1 < B:
            pair += np.abs(P[b][None] - P[b + 1:]).sum(axis=0)
    pair = np.where(np.isfinite(absq), pair, np.nan)
    return absq, pair, (P < x).sum(axis=0).astype(np.int64)


def _weighted_cols(Q, w):
    if w is None:
        return Q.sum(axis=1)
    sel = w != 0
    return (Q[:, sel, :] * w.astype(np.float64)[sel][None, :, None]).sum(axis=1)


def crps64(U, C, T, B, X, mu=None, sigma=None, w=None):
    """-> (col (2, T), row (2, m), hist (B + 1,) int64) in fp64; rows with w == 0 are selected out of col and hist."""
    with np.errstate(all="ignore"):
        absq, pair, rank = quantities64(members64(U, C, T, B, mu, sigma), X)
        Q = np.stack([absq, pair])
        sel = np.isfinite(absq)
        if w is not None:
            sel &= (w != 0)[:, None]
        hist = np.bincount(rank[sel], minlength=B + 1).astype(np.int64)
        return _weighted_cols(Q, w), Q.sum(axis=2), hist


def _gamma(j):
    return j * U24 / (1.0 - j * U24) if j > 0 else 0.0


def crps_bounds(U, C, T, B, X, mu=None, sigma=None, w=None):
    """-> bounds of (col (2, T), row (2, m)), the shapes of crps64.  Every operand must be finite here."""
    P = members64(U, C, T, B, mu, sigma)
    d = np.stack([er.element_bound(U, C[:, b * T:(b + 1) * T], mu, sigma) for b in range(B)])
    x = X.astype(np.float64)
    absq, pair, _ = quantities64(P, X)
    Ea = np.zeros(x.shape)
    Ep = np.zeros(x.shape)
    for b in range(B):
        Ea += d[b] + U24 * (np.abs(P[b] - x) + d[b])
        if b + 1 < B:
            dd = d[b][None] + d[b + 1:]
            Ep += (dd + U24 * (np.abs(P[b][None] - P[b + 1:]) + dd)).sum(axis=0)
    Q = np.stack([absq, pair])
    dQ = np.stack([Ea + _gamma(B - 1) * (absq + Ea), Ep + _gamma(pair_chain(B) - 1) * (pair + Ep)])
    col = _weighted_cols(dQ, w) + (FP32_ROWS + 3) * U24 * _weighted_cols(Q + dQ, w)
    row = dQ.sum(axis=2) + (FP32_COLS + 3) * U24 * (Q + dQ).sum(axis=2)
    return col, row


def scores(S, W, B, fair=True):
    """The scores of forecast.crps_blocks from sums S (2, ...) and W."""
    S0, S1 = S
    with np.errstate(all="ignore"):
        mae = S0 / (B * W)
        div = B * (B - 1) if fair else B * B
        return {"crps": mae - S1 / (div * W), "member_mae": mae,
                "member_distance": 2.0 * S1 / (B * (B - 1) * W) if B > 1 else np.full_like(mae, np.nan)}


def score_bounds(dS, W, B, fair=True):
    """Bounds of scores(S, W, B) when the sums may be off by dS: the scores are linear in the sums."""
    d0, d1 = dS
    div = B * (B - 1) if fair else B * B
    return {"crps": d0 / (B * W) + d1 / (div * W), "member_mae": d0 / (B * W),
            "member_distance": 2.0 * d1 / (B * (B - 1) * W) if B > 1 else np.zeros_like(d0)}


class CrpsDouble:
    """K19's method of a kernel provider on the CPU, for the host-layer tests: numpy fp64 through crps64 above
    (independent of forecast.py's torch fallback), mixed into tests/kernel_double.CpuKernelDouble."""

    crps_max_k = 256
    crps_max_members = MAX_B

    def crps(self, Ut, Cm, Xt, mean=None, std=None, weight=None, out=None, hist=None, want_rows=False):
        import torch

        def _np(t):
            return None if t is None else t.detach().cpu().numpy()

        B, T, k = Cm.shape
        C = _np(Cm).reshape(B * T, k).T
        col, row, counts = crps64(_np(Ut).T, C, T, B, _np(Xt).T, _np(mean), _np(std), _np(weight))
        cols, counts = torch.from_numpy(col), torch.from_numpy(counts)
        assert (out is None) == (hist is None)
        if out is not None:
            out += cols
            hist += counts
            cols, counts = out, hist
        return cols, (torch.from_numpy(row) if want_rows else None), counts
