"""Host definition of K28 (csrc/remap.hip) in numpy: first-order conservative remapping onto another regular latitude /
longitude grid, separable in the two axes, from six tables.

This file IS the arithmetic contract the kernel is held to bit for bit (tests/test_gpu_remap.py); the kernel is never
its own reference.  Snapshots are ``(T, rows)`` host arrays as in tests/coarsen_ref.py: plane p of a snapshot starts at
``p * ldp``, latitude row i and longitude j of a plane sit at ``i * nlon + j``.  Target row I overlaps the ``ny[I]``
source rows from ``iy0[I]`` on with the weights ``wy[I, a]``; target column J overlaps the ``nx[J]`` source columns
``(jx0[J] + b) mod nlon`` with the weights ``wx[J, b]``.  Entries of wy and wx beyond the count are never looked at:
they may hold anything.  numpy's fp64 ``*``, ``+`` and ``/`` on arrays are one IEEE operation per element and never
fused: every product below is rounded on its own.  The walk is vectorised over the cells, with explicit loops over a
and b, both ascending: the order of the chain.  A cell whose count is below a or b is left as it is (``np.where``).
"""
import numpy as np
import torch

from coarsen_ref import QUIET_NAN_BITS, finite_bits

MAX_SPAN = 64


def block_tables(w, fy, fx, NLAT, NLON, lat0=0, lon0=0):
    """The tables of K23's ``fy x fx`` blocks: wx = 1.0, wy[I, a] = w[lat0 + I fy + a]."""
    w = np.asarray(w, dtype=np.float64)
    iy0 = (lat0 + fy * np.arange(NLAT)).astype(np.int32)
    jx0 = (lon0 + fx * np.arange(NLON)).astype(np.int32)
    wy = w[iy0[:, None].astype(np.int64) + np.arange(fy)[None, :]].reshape(NLAT, fy)
    return (iy0, np.full(NLAT, fy, dtype=np.int32), np.ascontiguousarray(wy), jx0, np.full(NLON, fx, dtype=np.int32),
            np.ones((NLON, fx), dtype=np.float64))


def remap(X, planes, nlat, nlon, iy0, ny, wy, jx0, nx, wx, *, ldp=None, skipna=False, min_frac=0.0):
    """(T, planes * NLAT * NLON) fp32 from X (T, rows >= (planes - 1) ldp + nlat nlon) fp32 and the six tables.

    Per snapshot, plane and cell (I, J):  num = den = full = +0.0;  for a ascending, i = iy0[I] + a:  r = c = f = +0.0;
    for b ascending, j = (jx0[J] + b) mod nlon, u = wx[J, b], x = X[.., i, j]:  if (not skipna or finite(x)):
    r = r + u * float64(x), c = c + u;  f = f + u;   num = num + wy[I, a] * r;  den = den + wy[I, a] * c;
    full = full + wy[I, a] * f.   Y = quiet NaN (0x7fc00000) where den == 0 or den < min_frac * full, else
    float32(num / den)."""
    X = np.asarray(X, dtype=np.float32)
    iy0, ny, jx0, nx = (np.asarray(v, dtype=np.int64) for v in (iy0, ny, jx0, nx))
    wy, wx = np.asarray(wy, dtype=np.float64), np.asarray(wx, dtype=np.float64)
    T = X.shape[0]
    planes, nlat, nlon = int(planes), int(nlat), int(nlon)
    ldp = nlat * nlon if ldp is None else int(ldp)
    NLAT, NLON = iy0.shape[0], jx0.shape[0]
    assert wy.ndim == 2 and wx.ndim == 2 and wy.shape[0] == NLAT and wx.shape[0] == NLON
    assert 1 <= wy.shape[1] <= MAX_SPAN and 1 <= wx.shape[1] <= MAX_SPAN and ny.shape == (NLAT,) and nx.shape == (NLON,)
    assert (ny >= 0).all() and (ny <= wy.shape[1]).all() and (nx >= 0).all() and (nx <= wx.shape[1]).all()
    assert (iy0 >= 0).all() and (iy0 + ny <= nlat).all() and ldp >= nlat * nlon
    assert X.ndim == 2 and (planes == 0 or X.shape[1] >= (planes - 1) * ldp + nlat * nlon)
    assert 0.0 <= float(min_frac) <= 1.0
    fine = np.empty((T, planes, nlat, nlon), dtype=np.float32)
    for p in range(planes):
        fine[:, p] = X[:, p * ldp:p * ldp + nlat * nlon].reshape(T, nlat, nlon)
    shape = (T, planes, NLAT, NLON)
    num, den, full = (np.zeros(shape, dtype=np.float64) for _ in range(3))
    with np.errstate(all="ignore"):
        for a in range(int(ny.max()) if NLAT else 0):
            in_a = (a < ny).reshape(1, 1, NLAT, 1)
            rows = np.minimum(iy0 + a, nlat - 1)                                  # (beyond the count: any row, never used)
            wa = wy[:, min(a, wy.shape[1] - 1)].reshape(1, 1, NLAT, 1)
            r, c, f = (np.zeros(shape, dtype=np.float64) for _ in range(3))
            for b in range(int(nx.max()) if NLON else 0):
                in_b = (b < nx).reshape(1, 1, 1, NLON)
                cols = (jx0 + b) % nlon
                u = wx[:, min(b, wx.shape[1] - 1)].reshape(1, 1, 1, NLON)
                x = fine[:, :, rows][:, :, :, cols]
                ok = in_b & (finite_bits(x) if skipna else True)
                r = np.where(ok, r + u * np.where(ok, x, np.float32(0)).astype(np.float64), r)
                c = np.where(ok, c + u, c)
                f = np.where(in_b, f + u, f)
            num = np.where(in_a, num + wa * r, num)
            den = np.where(in_a, den + wa * c, den)
            full = np.where(in_a, full + wa * f, full)
        least = np.float64(min_frac) * full
        bad = (den == 0.0) | (den < least)
        y = (num / den).astype(np.float32)
    y = np.where(bad, np.array([QUIET_NAN_BITS], dtype=np.uint32).view(np.float32)[0], y).astype(np.float32)
    return y.reshape(T, planes * NLAT * NLON)


class RemapDouble:
    """``HipKernels.remap`` on CPU tensors through the definition above: what ``regrid.Remap`` needs of a provider."""

    name = "host"

    def __init__(self):
        self.calls = []

    def remap(self, Xt, planes, nlat, nlon, iy0, ny, wy, jx0, nx, wx, *, ldp=None, skipna=False, min_frac=0.0, out=None,
              ldq=None):
        self.calls.append((tuple(Xt.shape), int(planes), tuple(wy.shape), tuple(wx.shape)))
        y = remap(Xt.numpy(), planes, nlat, nlon, iy0.numpy(), ny.numpy(), wy.numpy(), jx0.numpy(), nx.numpy(), wx.numpy(),
                  ldp=ldp, skipna=skipna, min_frac=min_frac)
        cells = int(wy.shape[0]) * int(wx.shape[0])
        ldq = cells if ldq is None else int(ldq)
        rows = (int(planes) - 1) * ldq + cells if planes else 0
        Y = torch.zeros((Xt.shape[0], rows), dtype=torch.float32) if out is None else out
        for p in range(int(planes)):
            Y[:, p * ldq:p * ldq + cells] = torch.from_numpy(y[:, p * cells:(p + 1) * cells])
        return Y
