"""numpy definitions of K31 (dmdx_gap_mask_f32, dmdx_gap_standardize_f32, dmdx_gap_fill_f32), a plain fp64 DINEOF, and
the CPU double of the three provider methods.

TEST INFRASTRUCTURE, like tests/kernel_double.py.  Matrices are the LOGICAL column-major ones of include/dmdx.h:
X (m, T), U (m, k), C (k, T), mu / sigma (m,) or None; the mask W is (ceil(T / 32), m) uint32, W[tw, i] bit b <=> element
(i, 32 tw + b) is a gap.

Bound of change_row (u = 2^-24, derived, not measured).  The kernel forms, per set bit, d^ = fl(new - old) = d (1 + e1),
q^ = fl(d^ d^) = d^2 (1 + e1)^2 (1 + e2), adds the at most 16 values of a lane in a tile in fp32 -- a value goes through
at most 15 rounded additions (the first one adds to 0) -- and everything beyond in fp64 (fewer than 2^27 additions of
2^-53 each: below u / 4).  All terms are >= 0, so the relative errors carry over to the sum:
    |change_row - sum (new - old)^2| <= ((1 + u)^18 - 1 + u / 4) sum (new - old)^2 <= 19 u sum (new - old)^2
with `new` the STORED fp32 value (values in the normal range: no underflow of the squares).
"""
import numpy as np

from kernel_double import CpuKernelDouble

U24 = 2.0 ** -24
SEGMENT = 1024            # dmdx_gap_mask_segment()
CHANGE_C = 19             # the c of the bound above


def gap_bits(X):
    """True where the exponent bits are all ones (NaN of any payload, +-Inf)."""
    b = np.ascontiguousarray(X, dtype=np.float32).view(np.uint32)
    return (b & np.uint32(0x7F800000)) == np.uint32(0x7F800000)


def pack_bits(G):
    """A boolean (m, T) gap matrix -> W (ceil(T / 32), m) uint32; the bits from T on are 0."""
    m, T = G.shape
    nw = -(-T // 32)
    P = np.zeros((m, nw * 32), dtype=np.uint64)
    P[:, :T] = G
    w = (P.reshape(m, nw, 32) << np.arange(32, dtype=np.uint64)[None, None, :]).sum(axis=2)
    return np.ascontiguousarray(w.T.astype(np.uint32))


def unpack_bits(W, T):
    """W (nw, m) uint32 -> boolean (m, T); the bits from T on are dropped."""
    W = np.asarray(W).astype(np.uint32)
    nw, m = W.shape
    B = (W.T[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & np.uint32(1)
    return B.reshape(m, nw * 32)[:, :T].astype(bool)


def mask(X):
    """-> (W, nmiss int32 (m,), sums fp64 (2, m)): per segment of 1024 snapshots one fp64 chain in ascending t from
    +0.0 (a gap adds +0.0), the segment results added in ascending order from +0.0."""
    X = np.asarray(X, dtype=np.float32)
    m, T = X.shape
    G = gap_bits(X)
    with np.errstate(invalid="ignore"):                    # (signalling NaN payloads among the gaps)
        V = np.where(G, 0.0, X.astype(np.float64))
    tot = np.zeros((2, m))
    for a in range(0, T, SEGMENT):
        acc = np.zeros((2, m))
        for t in range(a, min(T, a + SEGMENT)):
            acc[0] = acc[0] + V[:, t]
            acc[1] = acc[1] + V[:, t] * V[:, t]
        tot = tot + acc
    return pack_bits(G), G.sum(axis=1).astype(np.int32), tot


def standardize(X, W=None, mu=None, sigma=None):
    """fl(fl(x - mu) / sigma), +0.0 where the bit is set: every operation rounded to fp32."""
    X = np.asarray(X, dtype=np.float32)
    with np.errstate(all="ignore"):
        Z = X if mu is None else (X - np.asarray(mu, dtype=np.float32)[:, None]).astype(np.float32)
        if sigma is not None:
            Z = (Z / np.asarray(sigma, dtype=np.float32)[:, None]).astype(np.float32)
    if W is not None:
        Z = np.where(unpack_bits(W, X.shape[1]), np.float32(0), Z)
    return Z.astype(np.float32)


def standardize_back(Z, mu=None, sigma=None):
    """fl(fl(z sigma) + mu): two roundings."""
    Z = np.asarray(Z, dtype=np.float32)
    with np.errstate(all="ignore"):
        P = Z if sigma is None else (Z * np.asarray(sigma, dtype=np.float32)[:, None]).astype(np.float32)
        if mu is not None:
            P = (P + np.asarray(mu, dtype=np.float32)[:, None]).astype(np.float32)
    return P.astype(np.float32)


def fill64(U, C, mu=None, sigma=None):
    """K12's field in fp64 (expand_ref.expand64)."""
    P = U.astype(np.float64) @ C.astype(np.float64)
    if sigma is not None:
        P = sigma.astype(np.float64)[:, None] * P
    if mu is not None:
        P = P + mu.astype(np.float64)[:, None]
    return P


def change64(new32, old32, G):
    """sum_t bit (new - old)^2 in fp64 from the fp32 values -> (m,)."""
    with np.errstate(all="ignore"):
        d = np.where(G, new32.astype(np.float64) - old32.astype(np.float64), 0.0)
    return (d * d).sum(axis=1)


def change_bound(exact):
    return CHANGE_C * U24 * exact


# ---------------------------------------------------------------- the synthetic field of the end-to-end tests
def synthetic(seed=0, m=300, T=96):
    """-> (truth (m, T) fp64 without noise, X (m, T) fp32 with noise 0.05 and NaN at the gaps).  Per-row offset ~ 280,
    three temporal modes (periods 24, 37, 11; amplitudes 3, 2, 1.2) with smooth spatial patterns.  Gaps: 8 % scattered,
    one box of 80 rows x 30 snapshots, 30 rows half missing, one snapshot missing everywhere, one row missing
    everywhere."""
    rng = np.random.default_rng(7000 + seed)
    i = np.arange(m)[:, None] / m
    t = np.arange(T)[None, :]
    truth = 280.0 + 5.0 * np.sin(2 * np.pi * i * 1.5 + 0.3) + 0.0 * t
    for period, amp, wave, ph in ((24, 3.0, 1.0, 0.2), (37, 2.0, 2.0, 1.1), (11, 1.2, 3.0, 2.3)):
        truth = truth + amp * np.cos(2 * np.pi * wave * i + ph) * np.cos(2 * np.pi * t / period + 3 * ph)
    X = (truth + 0.05 * rng.standard_normal((m, T))).astype(np.float32)
    G = rng.random((m, T)) < 0.08
    G[m // 3:m // 3 + 4 * m // 15, 5 * T // 12:5 * T // 12 + 5 * T // 16] = True     # (300 x 96: rows 100 .. 179, 40 .. 69)
    half = rng.choice(np.setdiff1d(np.arange(m), [17]), m // 10, replace=False)
    for r in half:
        G[r, rng.choice(T, T // 2, replace=False)] = True
    G[:, 55 * T // 96] = True
    G[17, :] = True
    X[G] = np.nan
    return truth, X


# ---------------------------------------------------------------- DINEOF in fp64, steps 1 - 6 of dmd_era5_amd/gapfill.py
def draw_cv(rng, n_rows, T, n_cv, P):
    """n_cv distinct present elements (P: boolean (n_rows, T)) as flat indices row * T + t: rounds of
    rng.integers(0, n_rows T, 2 need + 16), keeping in order what is present and new."""
    got = []
    seen = set()
    for _ in range(200):
        need = n_cv - len(got)
        if need <= 0:
            break
        for f in rng.integers(0, n_rows * T, size=2 * need + 16, dtype=np.int64).tolist():
            if P.reshape(-1)[f] and f not in seen:
                seen.add(f)
                got.append(f)
        got = got[:n_cv]
        seen = set(got)
    assert len(got) == n_cv
    return np.asarray(got, dtype=np.int64)


def _one_blas_thread():
    try:
        import threadpoolctl

        return threadpoolctl.threadpool_limits(limits=1, user_api="blas")
    except ImportError:
        import contextlib

        return contextlib.nullcontext()


def dineof64(X, max_rank, cv_fraction=0.01, min_cv=30, seed=0, tol=1e-4, max_iter=100, patience=2, scale=False,
             min_valid=2):
    """The reference: np.linalg.svd in fp64 on the fp32 standardised start.  -> dict with rank, cv_error (index = rank,
    [0] NaN), iterations ([0] the final pass), converged, filled (m, T) fp64 in raw units (NaN rows masked), row_mask,
    cv (flat indices), mean, std, scale0, Z (the final standardised field) and s, U, Vh of the final pass."""
    X = np.asarray(X, dtype=np.float32)
    m, T = X.shape
    W, nmiss, sums = mask(X)
    G = unpack_bits(W, T)
    n = (T - nmiss).astype(np.float64)
    ok = n >= max(min_valid, 1)
    n1 = np.where(ok, n, 1.0)
    m1 = sums[0] / n1
    var = sums[1] / n1 - m1 * m1
    if scale:
        ok &= var > 0
    mean = np.where(ok, m1, 0.0).astype(np.float32)
    std = np.where(ok, np.sqrt(np.maximum(var, 0)), 1.0).astype(np.float32) if scale else np.ones(m, dtype=np.float32)
    if scale:
        ok &= std > 0
        mean, std = np.where(ok, mean, np.float32(0)), np.where(ok, std, np.float32(1))
    G[~ok] = True
    css = np.maximum(sums[1] - sums[0] * m1, 0)
    zz = np.where(ok, css / (np.where(ok, var, 1.0) if scale else 1.0), 0.0)
    present = float(n[ok].sum())
    n_missing = float((T - n[ok]).sum())
    scale0 = float(np.sqrt(zz.sum() / present))
    n_cv = max(int(min_cv), int(cv_fraction * present))
    cv = draw_cv(np.random.default_rng(seed), m, T, n_cv, ~G)
    ci, ct = cv // T, cv % T
    with np.errstate(all="ignore"):
        truth = ((X[ci, ct] - mean[ci]) / std[ci]).astype(np.float32).astype(np.float64)
    Gcv = G.copy()
    Gcv[ci, ct] = True
    Z = standardize(X, pack_bits(Gcv), mean, std if scale else None).astype(np.float64)

    def iterate(Z, r, Gm, n_fill):
        done, err, it, f = False, np.nan, 0, None
        for it in range(1, max_iter + 1):
            with _one_blas_thread():                         # (a 300 x 96 SVD on many threads is 100 times slower)
                u, s, vh = np.linalg.svd(Z, full_matrices=False)
            f = (u[:, :r], s[:r], vh[:r])
            R = (u[:, :r] * s[:r]) @ vh[:r]
            change = float(((R - Z)[Gm] ** 2).sum())
            Z[Gm] = R[Gm]
            err = float(np.sqrt(((Z[ci, ct] - truth) ** 2).sum() / n_cv))
            if np.sqrt(change / max(n_fill, 1.0)) <= tol * scale0:
                done = True
                break
        return it, done, err, f

    cv_error, iterations = [np.nan], [0]
    for r in range(1, max_rank + 1):
        it, _, err, _ = iterate(Z, r, Gcv, n_missing + n_cv)
        cv_error.append(err), iterations.append(it)
        e = cv_error[1:]
        if len(e) > patience and all(x > min(e) for x in e[-patience:]):
            break
    rank = 1 + int(np.argmin(cv_error[1:]))
    Z[ci, ct] = truth
    it, converged, _, (u, s, vh) = iterate(Z, rank, G, n_missing)
    iterations[0] = it
    filled = Z * std.astype(np.float64)[:, None] + mean.astype(np.float64)[:, None]
    filled[~ok] = np.nan
    return dict(rank=rank, cv_error=np.asarray(cv_error), iterations=np.asarray(iterations), converged=converged,
                filled=filled, row_mask=~ok, cv=cv, mean=mean, std=std, scale0=scale0, Z=Z, U=u, s=s, Vh=vh,
                n_missing=int(n_missing), n_cv=n_cv, gaps=G)


# ---------------------------------------------------------------- the provider methods on the CPU
class GapKernelDouble(CpuKernelDouble):
    """CpuKernelDouble + the three K31 methods of HipKernels, computed by the definitions above (the fill in fp64,
    rounded once)."""

    name = "cpu-double+gap"
    gap_fill_max_k = 256
    gap_mask_segment = SEGMENT

    @staticmethod
    def _np(t):
        return None if t is None else t.detach().cpu().numpy()

    def gap_mask(self, Xt, want_sums=True, split=True):
        import torch

        W, nmiss, sums = mask(self._np(Xt).T)
        return (torch.from_numpy(W.view(np.int32).copy()), torch.from_numpy(nmiss),
                torch.from_numpy(sums) if want_sums else None)

    def gap_standardize_(self, Xt, W, mean, std, back=False):
        import torch

        X = self._np(Xt).T
        if back:
            Z = standardize_back(X, self._np(mean), self._np(std))
        else:
            Z = standardize(X, None if W is None else self._np(W).view(np.uint32), self._np(mean), self._np(std))
        Xt.copy_(torch.from_numpy(np.ascontiguousarray(Z.T)))
        return Xt

    def gap_fill_(self, Ut, Ct, W, Xt, mean=None, std=None, want_change=True):
        import torch

        T = int(Xt.shape[0])
        G = unpack_bits(self._np(W).view(np.uint32), T)
        new = fill64(self._np(Ut).T, self._np(Ct).T, self._np(mean), self._np(std)).astype(np.float32)
        old = self._np(Xt).T
        change = change64(new, old, G) if want_change else None
        Xt.copy_(torch.from_numpy(np.ascontiguousarray(np.where(G, new, old).T)))
        return None if change is None else torch.from_numpy(change)
