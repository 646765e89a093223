"""Host definition of K22 (csrc/tfilt.hip) in numpy: a FIR filter along time with an output stride, valid windows only.

This file IS the arithmetic contract the kernel is held to bit for bit (tests/test_gpu_tfilt.py); the kernel is never
its own reference.  Matrices are (rows, snapshots) host arrays, the C ABI's logical view; ``h`` is (L,) fp64.  numpy's
fp64 ``*`` and ``+`` on arrays are one IEEE operation per element and never fused: every product below is rounded on
its own.
"""
import numpy as np


def n_out(T, L, stride=1):
    """The number of valid windows of L taps, `stride` apart, in T snapshots."""
    T, L, stride = int(T), int(L), int(stride)
    return 0 if T < L else (T - L) // stride + 1


def tfilt(X, h, stride=1, T_out=None):
    """(m, T_out) fp32.  Per output u: acc = +0.0 (fp64), then for j = 0 .. L - 1 ascending
    q = float64(X[:, u stride + j]) * h[j] and acc = acc + q; Y[:, u] = float32(acc).  ``T_out``: fewer outputs than
    the snapshots allow (the trailing ones are then not looked at)."""
    X = np.asarray(X, dtype=np.float32)
    h = np.asarray(h, dtype=np.float64)
    m, T = X.shape
    L, stride = int(h.shape[0]), int(stride)
    assert h.ndim == 1 and L >= 1 and stride >= 1
    T_out = n_out(T, L, stride) if T_out is None else int(T_out)
    assert T_out >= 0 and (T_out == 0 or (T_out - 1) * stride + L <= T)
    X64 = X.astype(np.float64)
    acc = np.zeros((m, T_out), dtype=np.float64)
    with np.errstate(all="ignore"):
        for j in range(L):                                      # the sequential chain, for all outputs at once
            q = X64[:, j:j + (T_out - 1) * stride + 1:stride] * h[j] if T_out else acc
            acc = acc + q
        return acc.astype(np.float32)
