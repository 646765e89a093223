"""The quantile climatology on the GPU: Climatology.fit(quantiles=) through the HIP provider (K25) against
tests/quant_ref.py bit for bit, its threshold table through exceed_prob_blocks (K24), and the NetCDF round trip."""
import numpy as np
import pytest
import torch

import quant_ref as qr

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROWS = (1300, 1185)                      # a 35 x 71 grid in two row blocks
QS = (0.1, 0.9)


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def fit():
    """One year of 6-hourly fields with an annual cycle and skewed noise (squares: not normal), the
    day-of-year climatology with a +-2-day window: 366 slots of about 20 members each, Feb 29 from its neighbours."""
    from dmd_era5_amd.climatology import Climatology, slots_of
    from dmd_era5_amd.kernels import default_kernels

    rs = np.random.RandomState(25)
    times = np.datetime64("2021-01-01T00", "h") + np.arange(1460) * np.timedelta64(6, "h")
    T = times.shape[0]
    day = np.arange(T) / 4.0
    cyc = 10.0 * np.sin(2 * np.pi * day / 365.0)[:, None]
    X = [(280.0 + cyc + rs.standard_normal((T, mb)) ** 2).astype(np.float32) for mb in ROWS]
    kern = default_kernels()
    clim = Climatology.fit([torch.from_numpy(x).to(DEV) for x in X], times, "dayofyear", window_days=2, with_std=True,
                           quantiles=QS, kern=kern)
    _, order, start, S = slots_of(times, "dayofyear", 2)
    ref = [qr.quantile(x.T, order, start, QS) for x in X]
    return dict(clim=clim, ref=ref, times=times, kern=kern, S=S, counts=np.diff(start))


def test_fit_with_quantiles_equals_the_host_definition(fit):
    clim = fit["clim"]
    assert clim.q == QS and clim.method == "linear" and fit["S"] == 366 and (fit["counts"] >= 16).all()
    for b, mb in enumerate(ROWS):
        assert clim.quant[b].shape == (2, 366, mb) and clim.quant[b].is_cuda and clim.quant[b].dtype == torch.float32
        assert np.array_equal(_bits(clim.quant[b]), _bits(fit["ref"][b]))
        q = clim.quant[b].cpu().numpy()
        mu = clim.mean[b].cpu().numpy()
        assert (q[0] < q[1]).all()
        # the skewed noise: the upper decile lies further from the mean than the lower one
        assert (q[1] - mu).mean() > 1.2 * (mu - q[0]).mean()
    an = clim.quantile_thresholds(anomaly=True)
    for b in range(2):
        want = fit["ref"][b] - clim.mean[b].cpu().numpy()[None]
        assert np.array_equal(_bits(an[b]), _bits(want))


def test_the_table_drives_the_exceedance_kernel(fit):
    from dmd_era5_amd.forecast import exceed_prob_blocks

    clim, kern = fit["clim"], fit["kern"]
    rs = np.random.RandomState(7)
    k, B, Tn = 4, 5, 6
    valid = np.datetime64("2024-02-27T00", "h") + np.arange(Tn) * np.timedelta64(12, "h")    # across a Feb 29
    lab = clim.slots(valid)
    assert lab.tolist() == [57, 57, 58, 58, 59, 59]
    Ub = [torch.from_numpy(rs.standard_normal((k, mb)).astype(np.float32)).to(DEV) for mb in ROWS]
    Cm = torch.from_numpy((2.0 * rs.standard_normal((B, Tn, k))).astype(np.float32)).to(DEV)
    means = [M[58].contiguous() for M in clim.mean]
    got = exceed_prob_blocks(Ub, Cm, clim.quantile_thresholds(), lab, True, means, kern=kern)
    host = [torch.from_numpy(r).to(DEV) for r in fit["ref"]]
    want = exceed_prob_blocks(Ub, Cm, host, lab, True, means, kern=kern)
    for p, q, mb in zip(got, want, ROWS):
        assert p.shape == (2, Tn, mb) and torch.equal(p, q)
        assert bool((p[0] >= p[1]).all()) and 0.0 < float(p[1].mean()) < float(p[0].mean()) < 1.0


def test_dataset_round_trip_on_the_device(fit, tmp_path):
    from dmd_era5_amd import io_netcdf
    from dmd_era5_amd.climatology import Climatology

    clim = fit["clim"]
    path = str(tmp_path / "clim_q.nc")
    io_netcdf.to_netcdf(clim.to_dataset(), path)
    back = Climatology.from_dataset(io_netcdf.open_dataset(path), rows=ROWS, kern=fit["kern"])
    assert back.q == QS and back.method == "linear" and back.window_days == 2
    for b in range(2):
        assert back.quant[b].is_cuda and torch.equal(back.quant[b], clim.quant[b])
        assert torch.equal(back.quantile_thresholds(anomaly=True)[b], clim.quantile_thresholds(anomaly=True)[b])
