"""numpy doubles of K13 (dmdx_project_f32) and the error bounds its tests use.

TEST INFRASTRUCTURE, like tests/expand_ref.py: fp64 arithmetic on the fp32 inputs.  Matrices are the
LOGICAL column-major ones of include/dmdx.h: U (m, k), X (m, T), mu / sigma (m,) or None; the result
C is (k, T), the energy (T,).

Bounds (u = 2^-24, derived, not measured).  xd is the exact fp64 (x - mu) / sigma, xt the kernel's
fp32 value, R = DMDX_PROJECT_FP32_ROWS the longest fp32 chain, B the number of fp32 chain results that
are summed in fp32 before the sums turn fp64 (0 here: every chain is stored as it is and the row ranges
are added in fp64):
  C        |dC[j, t]|   <= (R + B + 4) u sum_i |U_ij| |xd_it|
           xt carries two roundings (the subtraction, the correctly rounded division): |xt - xd| <=
           (2 u + u^2) |xd|; every product is rounded once: u; a sum of at most R terms in ANY order (the MFMA
           chain, whatever the matrix core does inside a step) loses at most (R - 1) u of sum |terms| to first
           order, and B more when B such results meet in fp32.  Together (R + B + 2) u, the second-order terms
           ((R u)^2 / 2 = u / 2 at R = 4096) and the 2^-53 of the fp64 sums stay below the remaining 2 u.
  energy   |denergy_t|  <= (R + B + 6) u sum_i xd_it^2
           the square doubles the two roundings of xt (4 u) and is rounded once (u); the sum of at most R of
           them as above: (R + B + 4) u, 2 u left for the second-order terms.
"""
import numpy as np

U24 = 2.0 ** -24
FP32_ROWS = 4096          # DMDX_PROJECT_FP32_ROWS of include/dmdx.h
CHAINS_IN_FP32 = 0        # B


def standardized64(X, mu=None, sigma=None):
    """The exact (x - mu) / sigma of the fp32 inputs, (m, T) fp64."""
    Z = X.astype(np.float64)
    if mu is not None:
        Z = Z - mu.astype(np.float64)[:, None]
    if sigma is not None:
        Z = Z / sigma.astype(np.float64)[:, None]
    return Z


def project64(U, X, mu=None, sigma=None):
    """-> C (k, T) fp64."""
    return U.astype(np.float64).T @ standardized64(X, mu, sigma)


def energy64(X, mu=None, sigma=None):
    """-> (T,) fp64."""
    Z = standardized64(X, mu, sigma)
    return (Z * Z).sum(axis=0)


def project_bound(U, X, mu=None, sigma=None):
    return (FP32_ROWS + CHAINS_IN_FP32 + 4) * U24 * (np.abs(U).astype(np.float64).T @ np.abs(standardized64(X, mu, sigma)))


def energy_bound(X, mu=None, sigma=None):
    return (FP32_ROWS + CHAINS_IN_FP32 + 6) * U24 * energy64(X, mu, sigma)


class ProjectDouble:
    """The K13 method of a kernel provider on the CPU, for the host-layer tests: numpy fp64 through
    project64 / energy64 above (independent of forecast.py's torch fallback), mixed into
    tests/kernel_double.CpuKernelDouble by the tests that need a provider WITH project."""

    project_max_k = 256

    @staticmethod
    def _np(t):
        return None if t is None else t.detach().cpu().numpy()

    def project(self, Ut, Xt, mean=None, std=None, out=None, want_energy=True):
        import torch

        U, X, mu, sd = self._np(Ut).T, self._np(Xt).T, self._np(mean), self._np(std)
        C = torch.from_numpy(np.ascontiguousarray(project64(U, X, mu, sd).T))
        e = torch.from_numpy(energy64(X, mu, sd)) if want_energy else None
        if out is None:
            return C, e
        out[0].add_(C)
        if want_energy:
            out[1].add_(e)
        return out
