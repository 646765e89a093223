"""numpy doubles of K15 (dmdx_spread_f32 / dmdx_spread_score_f32) and the error bounds its tests use.

TEST INFRASTRUCTURE, like tests/expand_ref.py: fp64 arithmetic on the fp32 inputs.  Matrices are the LOGICAL
column-major ones of include/dmdx.h: U (m, k), D (k, B T) with column b T + t = member b at snapshot t,
sigma (m,) or None.

Bounds (u = 2^-24, derived, not measured).  P_b = U D_b is the exact member field, V = sum_b P_b^2, S = |sigma| sqrt(V).
  chain     the kernel's P_b is one fp32 chain of length k in any order:
                |dP_b| <= delta_b = (k + 1) u sum_j |u_ij| |d_bj|
  V         the squares of the computed P_b differ from the exact ones by 2 |P_b| delta_b + delta_b^2; each is
            rounded once and the B of them are added in fp32 one after the other (at most B + 1 roundings on
            any term, whether the multiply-add is fused or not):
                |dV| <= sum_b (2 |P_b| delta_b + delta_b^2) + (B + 1) u V
  S         sqrt(V + dV) - sqrt(V) = dV / (sqrt(V + dV) + sqrt(V)), which is at most |dV| / sqrt(V) and at most
            sqrt(|dV|) (the second one carries V = 0: identical members); then the correctly rounded root and
            the rounding of |sigma| * root:
                |dS| <= |sigma| min(|dV| / sqrt(V), sqrt(|dV|)) + 2 u S
  sums      w = sigma^2 V with sigma^2 and the product rounded once each, at most R = DMDX_SPREAD_FP32_ROWS = 128
            of them summed in fp32 in any order, fp64 beyond (its 2^-53 terms are far below u) -- the form of
            expand_ref.score_bounds:
                |d var| <= sum sigma^2 |dV| + (R + 2) u sum sigma^2 V
            for the column sums; the row sums are 16-term fp32 sums and keep the same form.
"""
import numpy as np

U24 = 2.0 ** -24
FP32_ROWS = 128           # DMDX_SPREAD_FP32_ROWS of include/dmdx.h


def _members(U, D, T, B):
    """P (B, m, T) fp64 and A = |U| |D| of the same shape."""
    k = U.shape[1]
    assert D.shape == (k, B * T), (D.shape, k, B, T)
    U64, D64 = U.astype(np.float64), D.astype(np.float64)
    P = np.stack([U64 @ D64[:, b * T:(b + 1) * T] for b in range(B)])
    A = np.stack([np.abs(U64) @ np.abs(D64[:, b * T:(b + 1) * T]) for b in range(B)])
    return P, A


def variance64(U, D, T, B):
    """V (m, T) = sum_b (U D_b)^2 in fp64."""
    P, _ = _members(U, D, T, B)
    return (P * P).sum(axis=0)


def spread64(U, D, T, B, sigma=None):
    S = np.sqrt(variance64(U, D, T, B))
    if sigma is not None:
        S = np.abs(sigma.astype(np.float64))[:, None] * S
    return S


def spread_score64(U, D, T, B, sigma=None):
    """-> (var_col (T,), var_row (m,)) in fp64."""
    W = variance64(U, D, T, B)
    if sigma is not None:
        W = sigma.astype(np.float64)[:, None] ** 2 * W
    return W.sum(axis=0), W.sum(axis=1)


def variance_bound(U, D, T, B):
    """-> (V, |dV| bound), both (m, T)."""
    k = U.shape[1]
    P, A = _members(U, D, T, B)
    delta = (k + 1) * U24 * A
    V = (P * P).sum(axis=0)
    return V, (2.0 * np.abs(P) * delta + delta * delta).sum(axis=0) + (B + 1) * U24 * V


def spread_bound(U, D, T, B, sigma=None):
    V, dV = variance_bound(U, D, T, B)
    root = np.sqrt(V)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.minimum(np.where(V > 0, dV / root, np.inf), np.sqrt(dV))
    if sigma is not None:
        s = np.abs(sigma.astype(np.float64))[:, None]
        d, root = s * d, s * root
    return d + 2.0 * U24 * root


def spread_score_bounds(U, D, T, B, sigma=None):
    """-> bounds of (var_col, var_row), same shapes as spread_score64."""
    V, dV = variance_bound(U, D, T, B)
    if sigma is not None:
        s2 = sigma.astype(np.float64)[:, None] ** 2
        V, dV = s2 * V, s2 * dV
    tail = (FP32_ROWS + 2) * U24
    return dV.sum(axis=0) + tail * V.sum(axis=0), dV.sum(axis=1) + tail * V.sum(axis=1)


def dev_matrix(Dev):
    """The logical D (k, B T) of a (B, T, k) deviation array."""
    B, T, k = Dev.shape
    return np.ascontiguousarray(Dev.reshape(B * T, k).T)


class SpreadDouble:
    """The two K15 methods of a kernel provider on the CPU, for the host-layer tests: numpy fp64 through
    spread64 / spread_score64 above (independent of forecast.py's torch fallback), mixed into
    tests/kernel_double.CpuKernelDouble by the tests that need a provider WITH spread."""

    spread_max_k = 256

    @staticmethod
    def _np(t):
        return None if t is None else t.detach().cpu().numpy()

    def spread(self, Ut, Dev, std=None, out=None):
        import torch

        B, T, _ = Dev.shape
        S = spread64(self._np(Ut).T, dev_matrix(self._np(Dev)), T, B, self._np(std))
        S = torch.from_numpy(np.ascontiguousarray(S.T.astype(np.float32)))
        if out is None:
            return S
        out.copy_(S)
        return out

    def spread_score(self, Ut, Dev, std=None, out=None, want_rows=False):
        import torch

        B, T, _ = Dev.shape
        col, row = spread_score64(self._np(Ut).T, dev_matrix(self._np(Dev)), T, B, self._np(std))
        var = torch.from_numpy(col)
        if out is not None:
            out += var
            var = out
        return var, (torch.from_numpy(row) if want_rows else None)
