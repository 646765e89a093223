"""Host definition of K18 (csrc/clim.hip) in numpy: the slot mean, the slot standard deviation and the apply step.

This file IS the arithmetic contract the kernel is held to bit for bit (tests/test_gpu_clim.py); the kernel is never
its own reference.  Matrices are (rows, snapshots) host arrays, the C ABI's logical view; ``mean`` / ``sd`` are
(S, rows).  The lists are taken as the kernel takes them: ``start`` clamped to [0, n_order], an entry of ``order``
outside [0, T) skipped and not counted, a label outside [0, S) leaving its snapshot alone.
"""
import numpy as np

QUIET_NAN = np.array([0x7FC00000], dtype=np.uint32).view(np.float32)[0]


def slot_lists(order, start, s, T):
    """The counted snapshot indices of slot s, in the order of the list."""
    order, start = np.asarray(order, dtype=np.int64), np.asarray(start, dtype=np.int64)
    n = order.shape[0]
    a = min(max(int(start[s]), 0), n)
    b = min(max(int(start[s + 1]), a), n)
    return [int(t) for t in order[a:b] if 0 <= t < T]


def counts(order, start, T):
    S = len(start) - 1
    return np.array([len(slot_lists(order, start, s, T)) for s in range(S)], dtype=np.int64)


def mean(X, order, start):
    """(S, m) fp32: acc = +0.0 (fp64); acc += float64(X[:, t]) for t in the list, in its order; fp32(acc / n)."""
    X = np.asarray(X, dtype=np.float32)
    m, T = X.shape
    S = len(start) - 1
    out = np.empty((S, m), dtype=np.float32)
    with np.errstate(all="ignore"):
        for s in range(S):
            ts = slot_lists(order, start, s, T)
            acc = np.zeros(m, dtype=np.float64)
            for t in ts:                                     # the sequential loop over the list
                acc += X[:, t].astype(np.float64)
            out[s] = (acc / np.float64(len(ts))).astype(np.float32) if ts else QUIET_NAN
    return out


def std(X, order, start, mu, ddof=0):
    """(S, m) fp32: d = float64(x) - float64(mean); q = d * d (a product of its own); acc += q; then
    fp32(sqrt(acc / (n - ddof))) with numpy's correctly rounded fp64 root."""
    X, mu = np.asarray(X, dtype=np.float32), np.asarray(mu, dtype=np.float32)
    m, T = X.shape
    S = len(start) - 1
    out = np.empty((S, m), dtype=np.float32)
    with np.errstate(all="ignore"):
        for s in range(S):
            ts = slot_lists(order, start, s, T)
            acc = np.zeros(m, dtype=np.float64)
            mu64 = mu[s].astype(np.float64)
            for t in ts:
                d = X[:, t].astype(np.float64) - mu64
                q = d * d
                acc += q
            n = len(ts) - int(ddof)
            out[s] = np.sqrt(acc / np.float64(n)).astype(np.float32) if n > 0 else QUIET_NAN
    return out


def apply(X, slot, mu, sd=None, restore=False):
    """(m, T) fp32, every step in fp32: ``(x - mean) [/ sd]``, or ``x [* sd] + mean`` with two roundings; the
    snapshots whose label is outside [0, S) are copies of X."""
    X = np.asarray(X, dtype=np.float32)
    mu = np.asarray(mu, dtype=np.float32)
    S = mu.shape[0]
    Y = X.copy()
    with np.errstate(all="ignore"):
        for t, s in enumerate(np.asarray(slot, dtype=np.int64).tolist()):
            if not 0 <= s < S:
                continue
            x = X[:, t]
            if restore:
                y = x if sd is None else (x * np.asarray(sd[s], dtype=np.float32)).astype(np.float32)
                y = (y + mu[s]).astype(np.float32)
            else:
                y = (x - mu[s]).astype(np.float32)
                if sd is not None:
                    y = (y / np.asarray(sd[s], dtype=np.float32)).astype(np.float32)
            Y[:, t] = y
    return Y
