"""Host definition of K21 (csrc/treg.hip) in numpy: the segmented fit and the apply step.

This file IS the arithmetic contract the kernel is held to bit for bit (tests/test_gpu_treg.py); the kernel is never
its own reference.  Matrices are (rows, snapshots) host arrays, the C ABI's logical view; ``W`` is (p, T) fp64, ``D``
(T, p) fp64, ``coef`` (p, rows) fp32.  numpy's fp64 ``*`` and ``+`` on arrays are one IEEE operation per element and
never fused: every product below is rounded on its own.
"""
import numpy as np


def w_of(D):
    """W = (D^T D)^-1 D^T (p, T) of a (T, p) fp64 design through its QR factorisation: R W = Q^T."""
    Q, R = np.linalg.qr(np.asarray(D, dtype=np.float64))
    return np.ascontiguousarray(np.linalg.solve(R, Q.T))


def fit(X, W, seg):
    """(p, m) fp32.  Time is cut into [0, seg), [seg, 2 seg), ...; per segment acc = +0.0, then for t ascending
    q = float64(X[:, t]) * W[j, t] and acc = acc + q; tot = +0.0, then tot = tot + acc per segment in ascending order;
    coef[j] = float32(tot)."""
    X = np.asarray(X, dtype=np.float32)
    W = np.asarray(W, dtype=np.float64)
    m, T = X.shape
    p = W.shape[0]
    seg = int(seg)
    assert W.shape[1] >= T and seg >= 1
    X64 = X.astype(np.float64)
    out = np.empty((p, m), dtype=np.float32)
    with np.errstate(all="ignore"):
        for j in range(p):
            tot = np.zeros(m, dtype=np.float64)
            for a in range(0, T, seg):
                acc = np.zeros(m, dtype=np.float64)
                for t in range(a, min(a + seg, T)):             # the sequential chain of a segment
                    q = X64[:, t] * W[j, t]
                    acc = acc + q
                tot = tot + acc
            out[j] = tot.astype(np.float32)
    return out


def fitted(coef, D):
    """(m, T) fp64: f = +0.0, then f = f + float64(coef[j]) * D[t, j] for j ascending (product rounded, then the
    add)."""
    coef = np.asarray(coef, dtype=np.float32).astype(np.float64)
    D = np.asarray(D, dtype=np.float64)
    T, p = D.shape
    f = np.zeros((coef.shape[1], T), dtype=np.float64)
    with np.errstate(all="ignore"):
        for j in range(p):
            q = coef[j][:, None] * D[:, j][None, :]
            f = f + q
    return f


def apply(X, D, coef, restore=False):
    """(m, T) fp32: float32(float64(x) - f), or with ``restore`` float32(float64(x) + f): one rounding."""
    X64 = np.asarray(X, dtype=np.float32).astype(np.float64)
    f = fitted(coef, D)
    with np.errstate(all="ignore"):
        return ((X64 + f) if restore else (X64 - f)).astype(np.float32)
