"""Host definition of K23 (csrc/coarsen.hip) in numpy: the area-weighted block mean over fy x fx cells of the latitude /
longitude grid, whole cells only.

This file IS the arithmetic contract the kernel is held to bit for bit (tests/test_gpu_coarsen.py); the kernel is never
its own reference.  Snapshots are ``(T, rows)`` host arrays, the package's image of a row block: plane p of a snapshot
starts at ``p * ldp``, latitude row i and longitude j of a plane sit at ``i * nlon + j``.  numpy's fp64 ``*``, ``+`` and
``/`` on arrays are one IEEE operation per element and never fused: every product below is rounded on its own.  The
walk is vectorised over the cells, with explicit loops over a (the fine rows of a cell) and b (its longitudes), both
ascending: the order of the chain.
"""
import numpy as np
import torch

QUIET_NAN_BITS = 0x7FC00000
MAX_FACTOR = 64


def finite_bits(x):
    """K20's test on the bit pattern: an exponent of all ones is not finite."""
    return (np.asarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0x7F800000)) != np.uint32(0x7F800000)


def n_cells(n, f, first=0):
    """Whole cells of f points in n points from ``first`` on."""
    return max(0, (int(n) - int(first)) // int(f))


def coarsen(X, planes, nlat, nlon, w, fy, fx, *, ldp=None, lat0=0, lon0=0, n_lat_out=None, n_lon_out=None, skipna=False,
            min_frac=0.0):
    """(T, planes * NLAT * NLON) fp32 from X (T, rows >= (planes - 1) ldp + nlat nlon) fp32 and w (nlat,) fp64.

    Per snapshot, plane and cell (I, J):  num = den = full = +0.0;  for a ascending, i = lat0 + I fy + a:  r = +0.0,
    c = 0;  for b ascending: x = X[.., i, lon0 + J fx + b], if (not skipna or finite(x)): r = r + float64(x), c += 1;
    num = num + w[i] * r;  den = den + w[i] * float64(c);  full = full + w[i] * float64(fx).
    Y = quiet NaN (0x7fc00000) where den == 0 or den < min_frac * full, else float32(num / den)."""
    X = np.asarray(X, dtype=np.float32)
    w = np.asarray(w, dtype=np.float64)
    T = X.shape[0]
    planes, nlat, nlon, fy, fx, lat0, lon0 = (int(v) for v in (planes, nlat, nlon, fy, fx, lat0, lon0))
    ldp = nlat * nlon if ldp is None else int(ldp)
    NLAT = n_cells(nlat, fy, lat0) if n_lat_out is None else int(n_lat_out)
    NLON = n_cells(nlon, fx, lon0) if n_lon_out is None else int(n_lon_out)
    assert 1 <= fy <= MAX_FACTOR and 1 <= fx <= MAX_FACTOR and lat0 >= 0 and lon0 >= 0
    assert lat0 + NLAT * fy <= nlat and lon0 + NLON * fx <= nlon and ldp >= nlat * nlon and w.shape == (nlat,)
    assert X.ndim == 2 and (planes == 0 or X.shape[1] >= (planes - 1) * ldp + nlat * nlon)
    assert 0.0 <= float(min_frac) <= 1.0
    # the planes as (T, P, nlat, nlon) without their pads
    fine = np.empty((T, planes, nlat, nlon), dtype=np.float32)
    for p in range(planes):
        fine[:, p] = X[:, p * ldp:p * ldp + nlat * nlon].reshape(T, nlat, nlon)
    shape = (T, planes, NLAT, NLON)
    num, den, full = (np.zeros(shape, dtype=np.float64) for _ in range(3))
    dfx = np.float64(fx)
    with np.errstate(all="ignore"):
        for a in range(fy):
            rows = slice(lat0 + a, lat0 + a + (NLAT - 1) * fy + 1, fy) if NLAT else slice(0, 0)
            wi = w[rows].reshape(1, 1, NLAT, 1)
            r = np.zeros(shape, dtype=np.float64)
            c = np.zeros(shape, dtype=np.float64)
            for b in range(fx):
                cols = slice(lon0 + b, lon0 + b + (NLON - 1) * fx + 1, fx) if NLON else slice(0, 0)
                x = fine[:, :, rows, cols]
                if skipna:
                    ok = finite_bits(x)
                    r = np.where(ok, r + np.where(ok, x, np.float32(0)).astype(np.float64), r)
                    c = np.where(ok, c + 1.0, c)
                else:
                    r = r + x.astype(np.float64)
                    c = c + 1.0
            num = num + wi * r
            den = den + wi * c
            full = full + wi * dfx
        least = np.float64(min_frac) * full
        bad = (den == 0.0) | (den < least)
        y = (num / den).astype(np.float32)
    y = np.where(bad, np.array([QUIET_NAN_BITS], dtype=np.uint32).view(np.float32)[0], y).astype(np.float32)
    return y.reshape(T, planes * NLAT * NLON)


class CoarsenDouble:
    """``HipKernels.coarsen`` on CPU tensors through the definition above: what ``regrid.Coarsen`` needs of a provider."""

    name = "host"

    def __init__(self):
        self.calls = []

    def coarsen(self, Xt, planes, nlat, nlon, w, fy, fx, *, ldp=None, lat0=0, lon0=0, n_lat_out=None, n_lon_out=None,
                skipna=False, min_frac=0.0, out=None, ldq=None):
        self.calls.append((tuple(Xt.shape), int(planes), int(fy), int(fx)))
        NLAT = n_cells(nlat, fy, lat0) if n_lat_out is None else int(n_lat_out)
        NLON = n_cells(nlon, fx, lon0) if n_lon_out is None else int(n_lon_out)
        y = coarsen(Xt.numpy(), planes, nlat, nlon, w.numpy(), fy, fx, ldp=ldp, lat0=lat0, lon0=lon0, n_lat_out=NLAT,
                    n_lon_out=NLON, skipna=skipna, min_frac=min_frac)
        cells = NLAT * NLON
        ldq = cells if ldq is None else int(ldq)
        rows = (int(planes) - 1) * ldq + cells if planes else 0
        Y = torch.zeros((Xt.shape[0], rows), dtype=torch.float32) if out is None else out
        for p in range(int(planes)):
            Y[:, p * ldq:p * ldq + cells] = torch.from_numpy(y[:, p * cells:(p + 1) * cells])
        return Y
