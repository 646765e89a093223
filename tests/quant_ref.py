"""Host definition of K25 (csrc/cquant.hip) in numpy: the empirical quantiles of the snapshots per slot.

This file IS the arithmetic contract the kernel is held to bit for bit (tests/test_gpu_quantile.py); the kernel is
never its own reference.  Matrices are (rows, snapshots) host arrays, the C ABI's logical view; the result is
(J, S, rows).  The lists are taken as ``clim_ref.slot_lists`` takes them.

Per (slot, row): the n counted members are sorted by the order-preserving key of their bit pattern u (``~u`` if the
sign bit is set, ``u | 0x80000000`` otherwise: -Inf < ... < -0.0 < +0.0 < denormals < ... < +Inf, a total order);
``h = float64(q) * float64(n - 1)`` rounded once, ``lo = floor(h)``, ``g = h - floor(h)``; "lower" sets g = 0, "higher"
takes ``lo = ceil(h)`` and g = 0.  With g == 0 the result is x_(lo) with its bits; otherwise, in fp64 and each step
rounded, ``d = b - a``, ``p = d * g``, ``r = a + p`` with a = x_(lo), b = x_(lo + 1), then one rounding to fp32.  No
counted member: the quiet NaN 0x7FC00000; a NaN among the members of (slot, row): the same NaN for every quantile.
"""
import numpy as np

from clim_ref import QUIET_NAN, slot_lists

METHODS = {"linear": 0, "lower": 1, "higher": 2}


def keys(x):
    """fp32 -> the uint32 keys whose unsigned order is the contract's order."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def unkeys(k):
    k = np.ascontiguousarray(k, dtype=np.uint32)
    u = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
    return u.view(np.float32)


def position(q, n, method):
    """-> (lo, g) of quantile q among n >= 1 sorted members."""
    h = np.float64(q) * np.float64(n - 1)
    fl = np.floor(h)
    if method == "linear":
        return int(fl), np.float64(h - fl)
    if method == "lower":
        return int(fl), np.float64(0.0)
    if method == "higher":
        return int(np.ceil(h)), np.float64(0.0)
    raise ValueError(f"method = {method!r}")


def of_members(Xs, q, method="linear"):
    """(rows, n) fp32 members -> (J, rows) fp32."""
    Xs = np.asarray(Xs, dtype=np.float32)
    m, n = Xs.shape
    qs = [float(v) for v in np.atleast_1d(np.asarray(q, dtype=np.float64))]
    out = np.empty((len(qs), m), dtype=np.float32)
    if n == 0:
        out[:] = QUIET_NAN
        return out
    srt = unkeys(np.sort(keys(Xs), axis=1)).reshape(m, n)
    bad = np.isnan(Xs).any(axis=1)
    with np.errstate(all="ignore"):
        for j, qv in enumerate(qs):
            lo, g = position(qv, n, method)
            if g == 0.0:
                out[j] = srt[:, lo]
            else:
                a, b = srt[:, lo].astype(np.float64), srt[:, lo + 1].astype(np.float64)
                d = b - a
                p = d * g
                r = a + p
                out[j] = r.astype(np.float32)
            out[j, bad] = QUIET_NAN
    return out


def quantile(X, order, start, q, method="linear"):
    """(J, S, m) fp32: the quantiles q of every row over the counted members of every slot."""
    X = np.asarray(X, dtype=np.float32)
    m, T = X.shape
    S = len(start) - 1
    J = len(np.atleast_1d(np.asarray(q)))
    out = np.empty((J, S, m), dtype=np.float32)
    for s in range(S):
        ts = slot_lists(order, start, s, T)
        out[:, s, :] = of_members(X[:, ts].reshape(m, len(ts)), q, method)
    return out
