"""Host definition of K29 (csrc/pstat.hip) in numpy: per-period extremes and totals of a daily statistic of every row.

This file IS the contract the kernel is held to bit for bit (tests/test_gpu_pstat.py); the kernel is never its own
reference.  :func:`period_stats` is a plain loop over the snapshots of a period -- vectorised over the rows only, every
fp64 operation in the order include/dmdx.h (K29) states, none of them fused.  X is a (rows, snapshots) host array, the C
ABI's logical view; ``thr`` a (rows,) fp32 vector or None.

    day k of period p   the snapshots [b_p + k g, min(b_p + (k + 1) g, b_{p+1})); c_k of them are finite (bit pattern);
                        valid iff c_k >= min_count
    d_k                 sum / mean / max / min / range of the finite snapshots, fp64, ascending t, strict compares
    r_k                 d_{k-w+1} + ... + d_k in that order, exists iff all w days are valid (never across a period)
    e_k                 r_k exists and r_k > h (< with below, >= / <= with inclusive), h = fp64(thr[i]) not NaN

    plane 0 n   1 max   2 argmax   3 min   4 argmin   5 total   6 event total   7 event count
    planes 5 and 6 are segsums: per piece of ``seg`` days acc = +0.0; acc = acc + v; then tot = tot + acc.

:func:`period_stats_by_pieces` restates the same results the way the split form of the kernel reaches them -- every
piece scanned on its own after the w - 1 days before it, a record per piece, merged in order -- and
tests/test_extremes.py holds the two against each other.
"""
import numpy as np
import torch

NQ = 8
INNER = ("sum", "mean", "max", "min", "range")
N, MAX, ARGMAX, MIN, ARGMIN, TOTAL, ETOTAL, ECOUNT = range(8)


def finite_bits(X):
    return (np.ascontiguousarray(X, dtype=np.float32).view(np.uint32) & 0x7F800000) != 0x7F800000


def _inner(inner):
    return INNER[inner] if isinstance(inner, (int, np.integer)) else str(inner)


def _check(bounds, T, group, inner, window, min_count, seg):
    b = [int(v) for v in np.asarray(bounds).reshape(-1)]
    assert len(b) >= 2 and b[0] >= 0 and b[-1] <= T and all(x < y for x, y in zip(b, b[1:])), b
    assert group >= 1 and _inner(inner) in INNER and 1 <= window <= 8 and seg >= 1
    mc = group if min_count is None else int(min_count)
    assert 1 <= mc <= group
    return b, mc


def day_values(X, lo, hi, group, inner, min_count, first_day=0):
    """The days first_day .. D - 1 of the period [lo, hi) of the (m, T) fp32 matrix X -> (d, ok): (m, D - first_day)
    fp64 day values (NaN where the day is not valid) and their validity."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    inner = _inner(inner)
    m = X.shape[0]
    D = -(-(hi - lo) // group)
    d = np.full((m, D - first_day), np.nan)
    ok = np.zeros((m, D - first_day), dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(first_day, D):
            s = np.zeros(m)
            c = np.zeros(m, dtype=np.int64)
            top, bot = np.zeros(m, dtype=np.float32), np.zeros(m, dtype=np.float32)
            for t in range(lo + k * group, min(lo + (k + 1) * group, hi)):
                x = X[:, t]
                fin = finite_bits(x)
                s = np.where(fin, s + x.astype(np.float64), s)
                top = np.where(fin & ((c == 0) | (x > top)), x, top)
                bot = np.where(fin & ((c == 0) | (x < bot)), x, bot)
                c = c + fin
            if inner == "sum":
                v = s
            elif inner == "mean":
                v = s / c.astype(np.float64)
            elif inner == "max":
                v = top.astype(np.float64)
            elif inner == "min":
                v = bot.astype(np.float64)
            else:
                v = top.astype(np.float64) - bot.astype(np.float64)
            ok[:, k - first_day] = c >= min_count
            d[:, k - first_day] = np.where(ok[:, k - first_day], v, np.nan)
    return d, ok


def running(d, ok, window):
    """-> (r, rk): r_k = d_{k-w+1} + ... + d_k in ascending order where all w days are valid (NaN elsewhere)."""
    m, D = d.shape
    r = np.full((m, D), np.nan)
    rk = np.zeros((m, D), dtype=bool)
    for k in range(window - 1, D):
        rk[:, k] = ok[:, k - window + 1:k + 1].all(axis=1)
        acc = d[:, k - window + 1].copy()
        for u in range(k - window + 2, k + 1):
            acc = acc + d[:, u]
        r[:, k] = np.where(rk[:, k], acc, np.nan)
    return r, rk


def events(r, rk, thr, below=False, inclusive=False):
    """The events e_k (m, D) of the running values."""
    if thr is None:
        return np.zeros_like(rk)
    h = np.asarray(thr, dtype=np.float32).astype(np.float64)[:, None]
    with np.errstate(invalid="ignore"):
        if below:
            cmp = (r <= h) if inclusive else (r < h)
        else:
            cmp = (r >= h) if inclusive else (r > h)
    return rk & ~np.isnan(h) & cmp


def tally(r, rk, ev, seg, k0=0):
    """The 8 planes (8, m) of the running values of the days k0, k0 + 1, ... of one period, the pieces cut from the
    first of them.  The plain loop."""
    m, D = r.shape
    q = np.zeros((NQ, m))
    q[[MAX, MIN]], q[[ARGMAX, ARGMIN]] = np.nan, -1.0
    for s0 in range(0, D, seg):
        acc, eacc = np.zeros(m), np.zeros(m)
        for k in range(s0, min(s0 + seg, D)):
            on, v = rk[:, k], r[:, k]
            with np.errstate(invalid="ignore"):
                up = on & ((q[N] == 0) | (v > q[MAX]))
                dn = on & ((q[N] == 0) | (v < q[MIN]))
            q[MAX], q[ARGMAX] = np.where(up, v, q[MAX]), np.where(up, k0 + k, q[ARGMAX])
            q[MIN], q[ARGMIN] = np.where(dn, v, q[MIN]), np.where(dn, k0 + k, q[ARGMIN])
            q[N] += on
            acc = np.where(on, acc + v, acc)
            eacc = np.where(ev[:, k], eacc + v, eacc)
            q[ECOUNT] += ev[:, k]
        q[TOTAL] = q[TOTAL] + acc
        q[ETOTAL] = q[ETOTAL] + eacc
    return q


def running_of_periods(X, bounds, group=1, inner="sum", window=1, min_count=None):
    """Per period (r, rk): everything of the result that does not depend on thr and seg."""
    b, mc = _check(bounds, np.shape(X)[1], group, inner, window, min_count, 1)
    return [running(*day_values(X, lo, hi, group, inner, mc), window) for lo, hi in zip(b[:-1], b[1:])]


def planes_of(runs, thr=None, below=False, inclusive=False, seg=64):
    """(8, P, m) fp64 from :func:`running_of_periods`."""
    return np.stack([tally(r, rk, events(r, rk, thr, below, inclusive), seg) for r, rk in runs], axis=1)


def period_stats(X, bounds, group=1, inner="sum", window=1, min_count=None, thr=None, below=False, inclusive=False, seg=64):
    """(8, P, m) fp64 of the (m, T) fp32 matrix X."""
    _check(bounds, np.shape(X)[1], group, inner, window, min_count, seg)
    return planes_of(running_of_periods(X, bounds, group, inner, window, min_count), thr, below, inclusive, seg)


# ---------------------------------------------------------------- the same through pieces and an ordered merge
def merge_records(records):
    """The 8 planes (8, m) of a period from the records (8, m) of its pieces, in ascending order: counts added, a
    strict compare for the extremes (the earlier piece wins a tie), tot = tot + acc from +0.0."""
    m = records[0].shape[1]
    q = np.zeros((NQ, m))
    q[[MAX, MIN]], q[[ARGMAX, ARGMIN]] = np.nan, -1.0
    for rec in records:
        has = rec[N] > 0
        with np.errstate(invalid="ignore"):
            up = has & ((q[N] == 0) | (rec[MAX] > q[MAX]))
            dn = has & ((q[N] == 0) | (rec[MIN] < q[MIN]))
        q[MAX], q[ARGMAX] = np.where(up, rec[MAX], q[MAX]), np.where(up, rec[ARGMAX], q[ARGMAX])
        q[MIN], q[ARGMIN] = np.where(dn, rec[MIN], q[MIN]), np.where(dn, rec[ARGMIN], q[ARGMIN])
        q[N] += rec[N]
        q[TOTAL] = q[TOTAL] + rec[TOTAL]
        q[ETOTAL] = q[ETOTAL] + rec[ETOTAL]
        q[ECOUNT] += rec[ECOUNT]
    return q


def period_stats_by_pieces(X, bounds, group=1, inner="sum", window=1, min_count=None, thr=None, below=False,
                           inclusive=False, seg=64):
    """:func:`period_stats` through records of pieces of ``seg`` days: every piece reads X from the w - 1 days before
    its start (inside its period) and knows nothing of the pieces before it."""
    b, mc = _check(bounds, np.shape(X)[1], group, inner, window, min_count, seg)
    out = []
    for lo, hi in zip(b[:-1], b[1:]):
        D = -(-(hi - lo) // group)
        recs = []
        for k0 in range(0, D, seg):
            k1, first = min(k0 + seg, D), max(0, k0 - (window - 1))
            end = min(lo + k1 * group, hi)
            d, ok = day_values(X, lo, end, group, inner, mc, first_day=first)
            r, rk = running(d, ok, window)
            r, rk = r[:, k0 - first:], rk[:, k0 - first:]              # the days before the piece only fill the ring
            recs.append(tally(r, rk, events(r, rk, thr, below, inclusive), seg, k0=k0))
        out.append(merge_records(recs))
    return np.stack(out, axis=1)


def n_pieces(bounds, group, seg):
    b = [int(v) for v in bounds]
    return sum(-(-(-(-(y - x) // group)) // seg) for x, y in zip(b[:-1], b[1:]))


class PstatDouble:
    """A kernel double: ``period_stats`` of HipKernels on CPU tensors, computed by :func:`period_stats`."""

    name = "cpu-double+pstat"
    period_stats_max_window = 8
    period_stats_max_periods = 128
    pstat_calls = 0

    def period_stats(self, Xt, bounds, group=1, inner="sum", window=1, min_count=None, thr=None, below=False,
                     inclusive=False, seg=64, out=None):
        type(self).pstat_calls += 1
        Q = torch.from_numpy(period_stats(Xt.numpy().T, bounds, group, inner, window, min_count,
                                          None if thr is None else thr.numpy(), below, inclusive, seg))
        if out is None:
            return Q
        out.copy_(Q)
        return out
