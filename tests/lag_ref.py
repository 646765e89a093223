"""Host definition of K26 (csrc/lagmom.hip) in numpy: the segmented lagged second moments of every row.

This file IS the arithmetic contract the kernel is held to bit for bit (tests/test_gpu_lagmom.py); the kernel is never
its own reference.  X is a (rows, snapshots) host array, the C ABI's logical view, ``mu`` (rows,) fp32 or None.  numpy's
fp64 ``-``, ``*`` and ``+`` on arrays are one IEEE operation per element and never fused.

    d_t  = float64(x_t) - float64(mu)        one rounded subtraction; with mu None d_t = float64(x_t), no operation
    sq_t = d_t * d_t
    pr_u = d_{u - tau} * d_u                 indexed by the LATER snapshot u in [tau, T)

``segsum(v, I)``: time is cut into [0, seg), [seg, 2 seg), ...; per segment acc = +0.0, then acc = acc + v_t for t in I
and the segment, ascending; tot = +0.0, then tot = tot + acc for EVERY segment in ascending order.

    plane 0           S   = segsum(sq, [0, T))
    plane 1 + l       P_l = segsum(pr, [tau_l, T))
    plane 1 + L + l   H_l = segsum(sq, [0, tau_l))          the head the later members of the pairs miss
    plane 1 + 2L + l  E_l = segsum(sq, [T - tau_l, T))      the tail the earlier members miss
"""
import numpy as np
import torch


def segsum(v, lo, hi, seg, T):
    """(m,) fp64: the segmented sum of the columns lo .. hi - 1 of v (m, T) -- v[:, t] is the term of snapshot t."""
    tot = np.zeros(v.shape[0], dtype=np.float64)
    for a in range(0, T, seg):
        acc = np.zeros(v.shape[0], dtype=np.float64)
        for t in range(max(a, lo), min(a + seg, T, hi)):          # the sequential chain of a segment
            acc = acc + v[:, t]
        tot = tot + acc
    return tot


def moments(X, lags, mu=None, seg=1024):
    """(1 + 3L, m) fp64 planes of the (m, T) fp32 matrix X."""
    X = np.asarray(X, dtype=np.float32)
    m, T = X.shape
    lags = [int(v) for v in lags]
    L, seg = len(lags), int(seg)
    assert 1 <= L <= 8 and seg >= 1 and all(0 <= v < T for v in lags) and all(a < b for a, b in zip(lags, lags[1:]))
    out = np.empty((1 + 3 * L, m), dtype=np.float64)
    with np.errstate(all="ignore"):
        d = X.astype(np.float64)
        if mu is not None:
            d = d - np.asarray(mu, dtype=np.float32).astype(np.float64)[:, None]
        sq = d * d
        out[0] = segsum(sq, 0, T, seg, T)
        for l, tau in enumerate(lags):
            pr = np.zeros_like(d)
            pr[:, tau:] = d[:, :T - tau] * d[:, tau:]
            out[1 + l] = segsum(pr, tau, T, seg, T)
            out[1 + L + l] = segsum(sq, 0, tau, seg, T)
            out[1 + 2 * L + l] = segsum(sq, T - tau, T, seg, T)
    return out


class LagDouble:
    """A kernel double: ``lag_moments`` of HipKernels on CPU tensors, computed by :func:`moments`."""

    name = "cpu-double+lag"
    lag_max_lags = 8
    lag_ring = 16
    lag_calls = 0

    def lag_moments(self, Xt, lags, mu=None, seg=1024, out=None, ring=True):
        type(self).lag_calls += 1
        P = torch.from_numpy(moments(Xt.numpy().T, lags, None if mu is None else mu.numpy(), seg))
        if out is None:
            return P
        out.copy_(P)
        return out
