"""numpy doubles of K30 (dmdx_varimax_step_f32, dmdx_row_norms_f32), the error bounds its tests use, the orthomax
iteration on top of any step function, the closed-form k = 2 varimax angle and a provider double for the host layer.

TEST INFRASTRUCTURE, like tests/kernel_double.py.  Matrices are the LOGICAL column-major ones of include/dmdx.h:
U (m, k), R (k, k), w (m,) or None.

Bounds (u = 2^-24, derived, not measured), with a = fl(U w), Labs = |a| |R|:
  L      one fp32 chain of k products: |dL| <= k u Labs (to first order; the slack below covers the rest)
  G      a L^3: three factors of L (3 k u), one rounding for w, two for the powers, one for the product inside the
         MFMA chain of at most 4096 rows: (4096 + 3 k + 8) u |a|^T Labs^3
  q      L^2: 2 k u, w, one power, the chain: (4096 + 2 k + 6) u colsum(Labs^2)
  f      L^4: 4 k u, w, three roundings of the powers, the chain: (4096 + 4 k + 8) u colsum(Labs^4)
The fp64 sums across row ranges add 2^-53 terms, far below the spare units.
"""
import numpy as np

U24 = 2.0 ** -24
FP32_ROWS = 4096          # DMDX_VARIMAX_FP32_ROWS of include/dmdx.h
MAX_K = 64


def weighted(U, w=None):
    """a = fl(U w) in fp32, or U."""
    U = np.asarray(U, dtype=np.float32)
    return U if w is None else (U * np.asarray(w, dtype=np.float32)[:, None]).astype(np.float32)


def step64(U, R, w=None):
    """-> (G (k, k), q (k,), f (k,)) in fp64, the formulas of include/dmdx.h on the fp32 inputs."""
    a = weighted(U, w).astype(np.float64)
    L = a @ np.asarray(R).astype(np.float64)          # (the kernel's R is fp32; the fp64 iteration hands over fp64)
    L2 = L * L
    return a.T @ (L2 * L), L2.sum(axis=0), (L2 * L2).sum(axis=0)


def step_bounds(U, R, w=None):
    """-> the bounds of (G, q, f), same shapes as step64."""
    k = np.asarray(R).shape[0]
    a = np.abs(weighted(U, w).astype(np.float64))
    L = a @ np.abs(np.asarray(R, dtype=np.float32).astype(np.float64))
    L2 = L * L
    return ((FP32_ROWS + 3 * k + 8) * U24 * (a.T @ (L2 * L)), (FP32_ROWS + 2 * k + 6) * U24 * L2.sum(axis=0),
            (FP32_ROWS + 4 * k + 8) * U24 * (L2 * L2).sum(axis=0))


def step32(U, R, w=None):
    """The float32 restatement: every product and every sum inside a range of FP32_ROWS rows in np.float32, fp64
    across the ranges.  Same unit roundoff as the kernel, another summation order."""
    a = weighted(U, w)
    R = np.asarray(R, dtype=np.float32)
    k = R.shape[0]
    G, q, f = np.zeros((k, k)), np.zeros(k), np.zeros(k)
    for r0 in range(0, a.shape[0], FP32_ROWS):
        ab = a[r0:r0 + FP32_ROWS]
        L = (ab @ R).astype(np.float32)
        L2 = (L * L).astype(np.float32)
        G += (ab.T @ (L2 * L).astype(np.float32)).astype(np.float32)
        q += L2.sum(axis=0, dtype=np.float32)
        f += (L2 * L2).astype(np.float32).sum(axis=0, dtype=np.float32)
    return G, q, f


def row_norms(U, cscale=None):
    """h[i] = fp32(sqrt(sum_j fp64(fl(U[i, j] cscale[j]))^2)), j ascending, squares rounded before they are added."""
    U = np.asarray(U, dtype=np.float32)
    a = U if cscale is None else (U * np.asarray(cscale, dtype=np.float32)[None, :]).astype(np.float32)
    acc = np.zeros(U.shape[0], dtype=np.float64)
    for j in range(U.shape[1]):
        d = a[:, j].astype(np.float64)
        acc = acc + d * d
    return np.sqrt(acc).astype(np.float32)


def orthomax(U, s=None, gamma=1.0, normalize=True, max_iter=100, tol=1e-6, step=step64, n_rows=None, round_R=True):
    """The iteration of dmd_era5_amd/rotation.py written down once more, on one (m, k) fp32 matrix and any step
    function: the kernel never sees s (it gets diag(s) R in fp32, the host scales G) and gets w = 1 / h.
    -> dict(R, iterations, converged, criterion, variance, loadings) with the columns ordered and signed as the
    product orders and signs them; ``loadings`` = U diag(s) R in fp64.  ``round_R`` false keeps diag(s) R in fp64 (a
    step function that takes it): the iteration in exact-to-fp64 arithmetic, without the 2^-24 the product's R carries."""
    U = np.asarray(U, dtype=np.float32)
    m_rows, k = U.shape
    sv = np.ones(k) if s is None else np.asarray(s, dtype=np.float64)
    m = float(m_rows if n_rows is None else n_rows)
    w = None
    if normalize:
        h = row_norms(U, None if s is None else sv.astype(np.float32))
        w = np.where(h > 0, np.float32(1) / np.where(h > 0, h, np.float32(1)), np.float32(0)).astype(np.float32)
    a = weighted(U, w).astype(np.float64)
    AtA = sv[:, None] * (a.T @ a) * sv[None, :]
    U64 = U.astype(np.float64)
    plain = sv[:, None] * (U64.T @ U64) * sv[None, :]

    def sums(R):
        G, q, f = step(U, (sv[:, None] * R).astype(np.float32) if round_R else sv[:, None] * R, w)
        return sv[:, None] * G, q, float((f / m - gamma * (q / m) ** 2).sum())

    R, d_old, crit, converged, it = np.eye(k), 0.0, [], False, 0
    for it in range(1, max_iter + 1):
        G, q, c = sums(R)
        crit.append(c)
        u, sig, vh = np.linalg.svd(G - (gamma / m) * (AtA @ R) * q[None, :])
        R, d = u @ vh, float(sig.sum())
        if tol > 0 and it > 1 and d - d_old <= tol * d:
            converged = True
            break
        d_old = d
    crit.append(sums(R)[2])
    variance = np.einsum("jc,jl,lc->c", R, plain, R)
    order = np.argsort(-variance, kind="stable")
    R, variance = R[:, order], variance[order]
    R = R * np.where(R[np.abs(R).argmax(axis=0), np.arange(k)] < 0, -1.0, 1.0)[None, :]
    return dict(R=R, iterations=it, converged=converged, criterion=np.asarray(crit), variance=variance,
                loadings=(U64 * sv[None, :]) @ R)


def varimax_angle_k2(A):
    """The closed-form raw varimax angle of two columns (Kaiser 1958): the rotation
    x' = x cos(phi) + y sin(phi), y' = -x sin(phi) + y cos(phi) maximises the criterion; phi is defined modulo pi / 2."""
    x, y = np.asarray(A, dtype=np.float64).T
    m = x.shape[0]
    u, v = x * x - y * y, 2.0 * x * y
    num = 2.0 * (u * v).sum() - 2.0 * u.sum() * v.sum() / m
    den = (u * u - v * v).sum() - (u.sum() ** 2 - v.sum() ** 2) / m
    return 0.25 * np.arctan2(num, den)


def structured(rng, m, k, noise=0.02, dtype=np.float32):
    """Loadings with simple structure (each row loads on one factor, plus noise) times a random orthogonal matrix:
    -> (A (m, k), the simple loadings (m, k), the orthogonal matrix Q with A = simple Q^T)."""
    simple = np.zeros((m, k))
    simple[np.arange(m), rng.integers(0, k, m)] = rng.uniform(0.5, 1.5, m) * rng.choice([-1.0, 1.0], m)
    simple += noise * rng.standard_normal((m, k))
    Q = np.linalg.qr(rng.standard_normal((k, k)))[0]
    return (simple @ Q.T).astype(dtype), simple, Q


def match_columns(L, want):
    """L with its columns permuted and signed to match ``want`` (greedy on |L^T want|, enough for simple structure)."""
    C = np.asarray(L).T @ np.asarray(want)
    k = C.shape[0]
    out = np.zeros_like(np.asarray(L, dtype=np.float64))
    free = list(range(k))
    for c in np.argsort(-np.abs(C).max(axis=0)):
        j = max(free, key=lambda i: abs(C[i, c]))
        free.remove(j)
        out[:, c] = np.sign(C[j, c]) * np.asarray(L)[:, j]
    return out


class VarimaxDouble:
    """The K30 methods of a kernel provider on the CPU, for the host-layer tests: numpy fp64 through step64 and
    row_norms above, mixed into tests/kernel_double.CpuKernelDouble (and expand_ref.ExpandDouble) by the tests."""

    varimax_max_k = MAX_K

    @staticmethod
    def _np(t):
        return None if t is None else t.detach().cpu().numpy()

    def varimax_step(self, Ut, Rt, w=None, out=None, want_f=True):
        import torch

        G, q, f = step64(self._np(Ut).T, self._np(Rt).T, self._np(w))
        res = [torch.from_numpy(np.ascontiguousarray(G.T)), torch.from_numpy(q), torch.from_numpy(f) if want_f else None]
        if out is not None:
            for o, r in zip(out, res):
                if o is not None:
                    o += r
            return tuple(out)
        return tuple(res)

    def row_norms(self, Ut, cscale=None, out=None):
        import torch

        h = torch.from_numpy(row_norms(self._np(Ut).T, self._np(cscale)))
        if out is None:
            return h
        out.copy_(h)
        return out
