"""dmd_era5_amd/regrid.py on the device: Coarsen.apply over a list of row blocks against tests/coarsen_ref.py bit for
bit, the weights of the coarse grid in the scores of verify_blocks, and a coarsened field through svd_snapshots."""
import numpy as np
import pytest
import torch

import coarsen_ref as cr
from dmd_era5_amd.regrid import Coarsen

pytestmark = pytest.mark.gpu

DEV = "cuda"
NLAT, NLON = 13, 24
LAT, LON = np.linspace(60.0, -60.0, NLAT), np.arange(NLON) * 15.0


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32).view(np.uint32)


def _blocks(T, planes, pad=0, seed=0):
    rs = np.random.RandomState(seed)
    host = [(250.0 + 30.0 * rs.standard_normal((T, p * NLAT * NLON + pad))).astype(np.float32) for p in planes]
    return host, [torch.from_numpy(h).to(DEV) for h in host]


@pytest.mark.parametrize("fy,fx", ((4, 4), (3, 5)))
def test_apply_on_two_blocks(fy, fx):
    T, planes = 5, [2, 1]
    host, X = _blocks(T, planes, pad=3)                                          # 3 rows of pad behind the planes
    for skipna in (False, True):
        if skipna:
            for h, x in zip(host, X):
                h[:, ::7] = np.nan
                x[:, ::7] = float("nan")
        cz = Coarsen(LAT, LON, fy, fx, lat0=1, weights="band", skipna=skipna, min_frac=0.5)
        want = [cr.coarsen(h, p, NLAT, NLON, cz.weights, fy, fx, lat0=1, skipna=skipna, min_frac=0.5) for h, p in zip(host, planes)]
        Y = cz.apply(X, planes)
        for y, w_, p in zip(Y, want, planes):
            assert y.shape == (T, cz.rows_out(p)) and y.dtype == torch.float32 and y.is_contiguous()
            assert np.array_equal(_bits(y), w_.view(np.uint32))
        # into views with a row stride; a generator of blocks
        bufs = [torch.full((T, cz.rows_out(p) + 3), 7.0, dtype=torch.float32, device=DEV) for p in planes]
        out = [b[:, :cz.rows_out(p)] for b, p in zip(bufs, planes)]
        Y2 = cz.apply((x for x in X), planes, out=out)
        for y, o, b, w_, p in zip(Y2, out, bufs, want, planes):
            assert y.data_ptr() == o.data_ptr()
            assert np.array_equal(_bits(o), w_.view(np.uint32)) and bool((b[:, cz.rows_out(p):] == 7.0).all())
        for x, h in zip(X, host):
            assert np.array_equal(_bits(x), h.view(np.uint32))                   # the input is left alone
        # a static field: one snapshot
        f = cz.apply_field(X[1][2], 1)
        assert f.shape == (cz.rows_out(1),) and np.array_equal(_bits(f), want[1][2].view(np.uint32))
    with pytest.raises(ValueError, match="block 1 holds"):
        cz.apply([X[0], X[1][:, :NLAT * NLON - 1]], planes)


def test_wrapper_checks_and_timing_record():
    from dmd_era5_amd._lib import DmdxError
    from dmd_era5_amd.kernels import HipKernels

    kern = HipKernels()
    assert kern.coarsen_max_factor == 64
    X = torch.zeros((3, 2 * NLAT * NLON), dtype=torch.float32, device=DEV)
    w = torch.ones(NLAT, dtype=torch.float64, device=DEV)
    for bad in (lambda: kern.coarsen(X, 2, NLAT, NLON, w.float(), 4, 4), lambda: kern.coarsen(X, 2, NLAT, NLON, w.cpu(), 4, 4),
                lambda: kern.coarsen(X, 2, NLAT, NLON, w[:-1], 4, 4), lambda: kern.coarsen(X, 2, NLAT, NLON, w, 0, 4),
                lambda: kern.coarsen(X, 2, NLAT, NLON, w, 4, 65), lambda: kern.coarsen(X.double(), 2, NLAT, NLON, w, 4, 4),
                lambda: kern.coarsen(X, 3, NLAT, NLON, w, 4, 4),                 # a third plane the block does not hold
                lambda: kern.coarsen(X, 2, NLAT, NLON, w, 4, 4, n_lat_out=4),    # cells that do not fit: refused by the library
                lambda: kern.coarsen(X, 2, NLAT, NLON, w, 4, 4, ldq=17),
                lambda: kern.coarsen(X, 2, NLAT, NLON, w, 4, 4, min_frac=2.0),
                lambda: kern.coarsen(X, 2, NLAT, NLON, w, 4, 4, out=torch.zeros((3, 35), dtype=torch.float32, device=DEV)),
                lambda: kern.coarsen(X, 2, NLAT, NLON, w, 4, 4, out=X[:, :36])):  # overlap: refused by the library
        with pytest.raises(DmdxError):
            bad()
    kern.events = []
    Y = kern.coarsen(X, 2, NLAT, NLON, w, 4, 4, ldq=20)
    assert Y.shape == (3, 38) and bool((Y[:, :18] == 0).all()) and bool((Y[:, 20:] == 0).all())
    assert [(n, s) for n, s, _, _ in kern.events] == [("coarsen", (2, NLAT, NLON, 3, 4, 4))]


def test_coarse_weights_in_the_scores():
    """A forecast on the coarse grid that is the analysis plus a bias: constant -> verify_blocks returns it; one value
    per coarse latitude -> the mean under ``row_weights_out``, which differs from the unweighted one.  The fields are of
    size one, so the fp32 forecast and its error are good to a few 2^-24: 1e-5 is far above that and far below the
    difference between the two means."""
    from dmd_era5_amd.forecast import verify_blocks

    T, P, fy, fx = 6, 2, 4, 4
    rs = np.random.RandomState(3)
    X = torch.from_numpy(rs.standard_normal((T, P * NLAT * NLON)).astype(np.float32)).to(DEV)
    cz = Coarsen(LAT, LON, fy, fx, weights="cos")
    Y = cz.apply([X], P)[0]
    rows = cz.rows_out(P)
    w = cz.row_weights_out(P).to(DEV)
    assert w.shape == (rows,)
    Ct = torch.eye(T, dtype=torch.float32, device=DEV)                           # U c = snapshot t of the analysis itself
    ones = torch.ones(rows, dtype=torch.float32, device=DEV)
    res = verify_blocks([Y], Ct, [Y], means=[0.75 * ones], stds=[ones], weights=[w])
    assert np.abs(res["bias"].cpu().numpy() - 0.75).max() <= 1e-5
    assert abs(float(res["weight"][0]) - float(cz.row_weights_out(P).double().sum())) <= 1e-9 * float(res["weight"][0])
    per_lat = np.array([2.0, -1.0, 0.5])
    assert cz.shape_out == (3, 6)
    bias = torch.from_numpy(np.tile(np.repeat(per_lat, 6), P).astype(np.float32)).to(DEV)
    res = verify_blocks([Y], Ct, [Y], means=[bias], stds=[ones], weights=[w])
    w64 = cz.weights_out.astype(np.float32).astype(np.float64)
    want = float((w64 * per_lat).sum() / w64.sum())
    assert abs(want - per_lat.mean()) > 1e-2
    assert np.abs(res["bias"].cpu().numpy() - want).max() <= 1e-5


def test_svd_of_a_coarsened_field():
    """A rank-3 field that is constant inside every 4 x 4 cell: coarsening gives the cell values back (a weighted mean
    of equal values, good to an ulp), and svd_snapshots of the coarse blocks returns the singular values of the coarse
    matrix formed on the host, to the relative tolerance tests/test_gpu_pipeline.py holds the same solver to."""
    from dmd_era5_amd.svd import svd_snapshots

    T, P, fy, fx, nlat, nlon = 40, 2, 4, 4, 33, 48                               # 8 x 12 cells, one latitude row dropped
    rs = np.random.RandomState(9)
    cells = P * 8 * 12
    coarse = (rs.standard_normal((T, 3)) * np.array([5.0, 3.0, 2.0])) @ rs.standard_normal((3, cells))
    coarse = coarse.astype(np.float32)
    fine = np.zeros((T, P, nlat, nlon), dtype=np.float32)
    fine[:, :, :32, :] = np.repeat(np.repeat(coarse.reshape(T, P, 8, 12), fy, axis=2), fx, axis=3)
    fine[:, :, 32, :] = 1e6                                                      # the dropped row: never looked at
    cz = Coarsen(np.linspace(80.0, -80.0, nlat), np.arange(nlon) * 7.5, fy, fx)
    assert cz.shape_out == (8, 12) and cz.dropped == (1, 0)
    Y = cz.apply([torch.from_numpy(fine.reshape(T, -1)).to(DEV)], P)[0]
    got = Y.cpu().numpy()
    assert np.abs(got.view(np.int32).astype(np.int64) - coarse.view(np.int32).astype(np.int64)).max() <= 1
    res = svd_snapshots([Y], 3)
    want = np.linalg.svd(got.astype(np.float64), compute_uv=False)[:3]
    assert np.allclose(res.s.cpu().numpy(), want, rtol=2e-5)
