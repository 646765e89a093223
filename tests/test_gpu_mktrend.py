"""``MannKendall.fit`` on the device against the same fit on the CPU double of tests/mk_ref.py, at n = 85 with two blocks
of 700 and 33 rows: the integer planes, the four ranks and the slopes are equal in every bit (sqrt and the products
between the two kernels are IEEE fp64 on both sides), p and Z agree to a relative 1e-12 (fp64 erfc on both sides), and
a fit survives the file round trip."""
import numpy as np
import pytest
import torch

import mk_ref as mr
from dmd_era5_amd import io_netcdf, mktrend
from dmd_era5_amd.mktrend import MannKendall

pytestmark = pytest.mark.gpu

DEV = "cuda"
N, ROWS = 85, (700, 33)


def _blocks():
    """Annual-maximum-like series: a grid of 1/8 (ties), a trend per row, gaps, some rows nearly or fully empty."""
    rs = np.random.RandomState(85)
    out = []
    for rows in ROWS:
        y = rs.gumbel(size=(N, rows)) * 2.0 + rs.uniform(-0.03, 0.05, size=rows) * np.arange(N)[:, None]
        y = (np.round(y * 8) / 8).astype(np.float32)
        y[rs.rand(N, rows) < rs.choice([0.0, 0.05, 0.4], size=rows)] = np.nan
        y[:, 3] = np.nan
        y[5:, 4] = np.nan
        y[:5, 4] = (1.0, 3.0, 2.0, 5.0, 4.0)
        y[:, 6] = 1.5
        out.append(y)
    return out


@pytest.fixture(scope="module")
def both():
    years = 1940.0 + np.arange(N)
    host = [torch.from_numpy(y) for y in _blocks()]
    scale = [torch.from_numpy(np.random.RandomState(b).uniform(1.0, 3.0, size=r)) for b, r in enumerate(ROWS)]
    from dmd_era5_amd.kernels import default_kernels

    kern = default_kernels()
    fits = {}
    for name, vs in (("plain", None), ("scaled", scale)):
        ref = MannKendall.fit(host, years, alpha=0.05, variance_scale=vs, kern=mr.MkDouble())
        dev = MannKendall.fit([y.to(DEV) for y in host], years, alpha=0.05, kern=kern,
                              variance_scale=None if vs is None else [s.to(DEV) for s in vs])
        fits[name] = (ref, dev)
    return fits


@pytest.mark.parametrize("name", ["plain", "scaled"])
def test_the_fit_on_the_device_is_the_fit_on_the_double(both, name):
    ref, dev = both[name]
    for b in range(2):
        assert dev.stats[b].is_cuda and torch.equal(dev.stats[b].cpu(), ref.stats[b])
        scale = [None if f.variance_scale is None else f.variance_scale[b] for f in (ref, dev)]
        ranks = [mktrend.interval_ranks(f.stats[b], 0.05, s) for f, s in zip((ref, dev), scale)]
        assert torch.equal(ranks[1].cpu(), ranks[0])
        assert torch.equal(dev.slopes[b].cpu().view(torch.int32), ref.slopes[b].view(torch.int32))
        assert torch.equal(dev.variance()[b].cpu(), ref.variance()[b])
        for got, want in ((dev.z()[b].cpu(), ref.z()[b]), (dev.p_value()[b].cpu(), ref.p_value()[b]),
                          (dev.tau_b()[b].cpu(), ref.tau_b()[b])):
            assert torch.equal(torch.isnan(got), torch.isnan(want))
            ok = ~torch.isnan(want)
            assert bool((torch.abs(got[ok] - want[ok]) <= 1e-12 * torch.abs(want[ok])).all())
        assert torch.equal(dev.slope(per=10.0)[b].cpu().view(torch.int32), ref.slope(per=10.0)[b].view(torch.int32))
    # the inputs hold the cases: empty rows, all-tied rows, significant and insignificant ones
    v = torch.cat(ref.n_valid())
    p = torch.cat(ref.p_value())
    assert int((v == 0).sum()) == 2 and int((v == 5).sum()) == 2 and int((v == N).sum()) > 50 and int((v < N).sum()) > 300
    assert int(torch.isnan(p).sum()) >= 4 and int((p <= 0.05).sum()) > 50 and int((p > 0.05).sum()) > 50
    assert [s.cpu().tolist() for s in dev.significant(fdr=True)] == [s.tolist() for s in ref.significant(fdr=True)]


def test_one_file_round_trip(both, tmp_path):
    _, dev = both["scaled"]
    path = str(tmp_path / "mk.nc")
    io_netcdf.to_netcdf(dev.to_dataset(), path)
    back = MannKendall.from_dataset(io_netcdf.open_dataset(path), rows=ROWS)
    for b in range(2):
        assert back.stats[b].is_cuda and torch.equal(back.stats[b], dev.stats[b])
        assert torch.equal(back.slopes[b].view(torch.int32), dev.slopes[b].view(torch.int32))
        assert torch.equal(back.variance_scale[b], dev.variance_scale[b])
        assert torch.allclose(back.p_value()[b], dev.p_value()[b], rtol=0.0, atol=0.0, equal_nan=True)   # (NaN: empty rows)
    assert back.alpha == dev.alpha and np.array_equal(back.coord, dev.coord)
