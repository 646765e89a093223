"""numpy doubles of K12 (dmdx_expand_f32 / dmdx_expand_score_f32) and the error bounds its tests use.

TEST INFRASTRUCTURE, like tests/kernel_double.py: fp64 arithmetic on the fp32 inputs.  Matrices are
the LOGICAL column-major ones of include/dmdx.h: U (m, k), C (k, T), X (m, T), mu / sigma (m,) or None.

Bounds (u = 2^-24, derived, not measured):
  element   |dXhat[i, t]| <= (k + 2) u (|sigma_i| sum_j |u_ij| |c_jt| + |mu_i|)
            one fp32 chain of length k in any order, then the rounding of sigma * acc and of + mu;
  score     the fp32 residual differs from the exact e = x - xhat by at most
            delta = element bound + u |x| (the error of xhat plus the rounding of the difference), so
            |d sse| <= sum (2 |e| delta + delta^2) + (R + 2) u sse
            with R = DMDX_EXPAND_FP32_ROWS = 128: squares rounded once, at most R of them summed in fp32
            in any order, fp64 beyond (its 2^-53 terms are far below u).  The same form holds for the row
            sums (16-term fp32 sums) and, with delta = u |x - mu|, for ref_col.
"""
import numpy as np

U24 = 2.0 ** -24
FP32_ROWS = 128           # DMDX_EXPAND_FP32_ROWS of include/dmdx.h


def expand64(U, C, mu=None, sigma=None):
    P = U.astype(np.float64) @ C.astype(np.float64)
    if sigma is not None:
        P = sigma.astype(np.float64)[:, None] * P
    if mu is not None:
        P = P + mu.astype(np.float64)[:, None]
    return P


def element_bound(U, C, mu=None, sigma=None):
    k = U.shape[1]
    A = np.abs(U).astype(np.float64) @ np.abs(C).astype(np.float64)
    if sigma is not None:
        A = np.abs(sigma).astype(np.float64)[:, None] * A
    if mu is not None:
        A = A + np.abs(mu).astype(np.float64)[:, None]
    return (k + 2) * U24 * A


def score64(U, C, X, mu=None, sigma=None):
    """-> (sse_col (T,), ref_col (T,), sse_row (m,)) in fp64."""
    E = X.astype(np.float64) - expand64(U, C, mu, sigma)
    G = X.astype(np.float64) - (0.0 if mu is None else mu.astype(np.float64)[:, None])
    return (E * E).sum(axis=0), (G * G).sum(axis=0), (E * E).sum(axis=1)


def score_bounds(U, C, X, mu=None, sigma=None):
    """-> bounds of (sse_col, ref_col, sse_row), same shapes as score64."""
    X64 = X.astype(np.float64)
    E = np.abs(X64 - expand64(U, C, mu, sigma))
    delta = element_bound(U, C, mu, sigma) + U24 * np.abs(X64)
    per = 2.0 * E * delta + delta * delta
    G = np.abs(X64 - (0.0 if mu is None else mu.astype(np.float64)[:, None]))
    dg = U24 * G
    perg = 2.0 * G * dg + dg * dg
    tail = (FP32_ROWS + 2) * U24
    return (per.sum(axis=0) + tail * (E * E).sum(axis=0), perg.sum(axis=0) + tail * (G * G).sum(axis=0),
            per.sum(axis=1) + tail * (E * E).sum(axis=1))


class ExpandDouble:
    """The two K12 methods of a kernel provider on the CPU, for the host-layer tests: numpy fp64 through
    expand64 / score64 above (independent of forecast.py's torch fallback), mixed into
    tests/kernel_double.CpuKernelDouble by the tests that need a provider WITH expand."""

    expand_max_k = 256

    @staticmethod
    def _np(t):
        return None if t is None else t.detach().cpu().numpy()

    def expand(self, Ut, Ct, mean=None, std=None, out=None):
        import torch

        P = expand64(self._np(Ut).T, self._np(Ct).T, self._np(mean), self._np(std))
        P = torch.from_numpy(np.ascontiguousarray(P.T.astype(np.float32)))
        if out is None:
            return P
        out.copy_(P)
        return out

    def expand_score(self, Ut, Ct, Xt, mean=None, std=None, out=None, want_rows=False):
        import torch

        sse, ref, row = score64(self._np(Ut).T, self._np(Ct).T, self._np(Xt).T, self._np(mean), self._np(std))
        cols = torch.from_numpy(np.stack([sse, ref]))
        if out is not None:
            out += cols
            cols = out
        return cols, (torch.from_numpy(row) if want_rows else None)
