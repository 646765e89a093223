"""dmd_era5_amd.mktrend on the CPU double of tests/mk_ref.py: the ranks and the statistics against scipy
(``theilslopes``, ``kendalltau``), Z and p against the closed formulas on hand-made series, the variance scale, the
Benjamini-Hochberg threshold, ``period_years`` and the file round trip."""
import math
from statistics import NormalDist

import numpy as np
import pytest
import scipy.stats
import torch

import mk_ref as mr
from dmd_era5_amd import io_netcdf, mktrend
from dmd_era5_amd.mktrend import MannKendall, fdr_threshold, mk_blocks, sen_blocks

ALPHA = 0.1
SIZES = list(range(5, 40))
ROWS = 12                                   # series per length: 420 in all


def _series(n, rows, rs):
    """(rows, n) fp32 with heavy ties (a grid of 4 .. 9 levels plus a trend), NaNs, and n irregular coordinates."""
    levels = rs.randint(4, 10, size=(rows, 1))
    y = np.floor(rs.rand(rows, n) * levels + rs.uniform(-0.08, 0.12, size=(rows, 1)) * np.arange(n))
    y = (y * rs.choice([0.25, 1.0, 3.0], size=(rows, 1))).astype(np.float32)
    gaps = rs.rand(rows, n) < rs.choice([0.0, 0.1, 0.3], size=(rows, 1))
    gaps[:, :3] = False                     # at least three valid points
    y[gaps] = np.nan
    t = np.cumsum(rs.choice([0.5, 1.0, 1.0, 2.0, 3.25], size=n))
    return y, t


@pytest.fixture(scope="module")
def fits():
    """-> [(y (rows, n), t, MannKendall)] for every length, fitted once."""
    rs = np.random.RandomState(7)
    out = []
    for n in SIZES:
        y, t = _series(n, ROWS, rs)
        mk = MannKendall.fit([torch.from_numpy(np.ascontiguousarray(y.T))], t, alpha=ALPHA, kern=mr.MkDouble())
        out.append((y, t, mk))
    return out


def _ulp32(x):
    return float(np.spacing(np.abs(np.float32(x))))


def test_the_slopes_are_those_of_scipy(fits):
    odd = even = tied = gappy = 0
    for y, t, mk in fits:
        slope, (low, high) = mk.slope()[0].numpy(), [v[0].numpy() for v in mk.slope_interval()]
        for i in range(y.shape[0]):
            ok = np.isfinite(y[i])
            yi, ti = y[i][ok].astype(np.float64), t[ok]
            v = int(ok.sum())
            N = v * (v - 1) // 2
            ref = scipy.stats.theilslopes(yi, ti, alpha=1.0 - ALPHA)
            assert np.float32(ref[2]) == low[i] and np.float32(ref[3]) == high[i], (y.shape[1], i, ref, low[i], high[i])
            if N % 2:
                assert np.float32(ref[0]) == slope[i], (y.shape[1], i)
                odd += 1
            else:
                assert abs(float(np.float32(ref[0])) - float(slope[i])) <= _ulp32(ref[0]), (y.shape[1], i)
                even += 1
            tied += len(np.unique(yi)) < v
            gappy += v < y.shape[1]
    assert odd >= 50 and even >= 50 and tied >= 200 and gappy >= 100, (odd, even, tied, gappy)


def test_tau_b_is_that_of_scipy(fits):
    for y, t, mk in fits:
        tau = mk.tau_b()[0].numpy()
        for i in range(y.shape[0]):
            ok = np.isfinite(y[i])
            ref = scipy.stats.kendalltau(t[ok], y[i][ok].astype(np.float64)).statistic
            assert abs(tau[i] - ref) <= 1e-12, (y.shape[1], i, tau[i], ref)


def test_the_planes_of_a_fit_are_those_of_the_block_drivers(fits):
    y, t, mk = fits[10]
    Yt = torch.from_numpy(np.ascontiguousarray(y.T))
    Q = mk_blocks([Yt], kern=mr.MkDouble())[0]
    assert torch.equal(Q, mk.stats[0]) and Q.dtype == torch.int32 and tuple(Q.shape) == (4, ROWS)
    v = Q[0].to(torch.int64)
    N = v * (v - 1) // 2
    E = sen_blocks([Yt], t, [torch.stack([(N - 1) // 2, N // 2]).to(torch.int32)], kern=mr.MkDouble())[0]
    assert torch.equal(E.view(torch.int32), mk.slopes[0][:2].view(torch.int32))
    assert [torch.equal(a, b) for a, b in zip(mk.n_valid() + mk.s(), [Q[0], Q[1]])] == [True, True]


def _fit_rows(rows, t=None, **kw):
    y = np.array(rows, dtype=np.float32)
    t = np.arange(y.shape[1], dtype=np.float64) if t is None else t
    return MannKendall.fit([torch.from_numpy(np.ascontiguousarray(y.T))], t, kern=mr.MkDouble(), **kw)


def test_z_and_p_on_hand_made_series():
    nan = float("nan")
    n = 10
    up = [float(k * k) for k in range(n)]
    rows = [up, up[::-1], [3.0] * n, [nan] * n, [nan] * 4 + [2.0] + [nan] * 5, [nan, 1.0] + [nan] * 6 + [4.0, nan],
            [1.0, 1.0, 2.0, 2.0, 2.0, 3.0, nan, nan, nan, nan]]
    mk = _fit_rows(rows, alpha=0.05)
    v, S, E, G = (mk.stats[0][q].tolist() for q in range(4))
    assert v == [10, 10, 10, 0, 1, 2, 6]
    assert S == [45, -45, 0, 0, 0, 1, 15 - 4]
    assert E == [0, 0, 45, 0, 0, 0, 1 + 3]
    assert G == [0, 0, 10 * 9 * 25, 0, 0, 0, 2 * 1 * 9 + 3 * 2 * 11]
    var = mk.variance()[0].tolist()
    assert var == [125.0, 125.0, 0.0, 0.0, 0.0, 1.0, (6 * 5 * 17 - 84) / 18.0]
    z, p, tau = mk.z()[0].tolist(), mk.p_value()[0].tolist(), mk.tau_b()[0].tolist()
    z0 = 44.0 / math.sqrt(125.0)
    assert z[0] == pytest.approx(z0, rel=1e-15) and z[1] == pytest.approx(-z0, rel=1e-15)
    assert p[0] == pytest.approx(math.erfc(z0 / math.sqrt(2.0)), rel=1e-13) and p[1] == p[0]
    assert tau[0] == 1.0 and tau[1] == -1.0
    for i in (2, 3, 4):                                            # sigma = 0: all equal, no point, one point
        assert math.isnan(z[i]) and math.isnan(p[i]) and math.isnan(tau[i]), i
    assert z[5] == 0.0 and p[5] == 1.0 and tau[5] == 1.0          # two points: S = 1, sigma = 1
    z6 = 10.0 / math.sqrt(var[6])
    assert z[6] == pytest.approx(z6, rel=1e-15) and p[6] == pytest.approx(math.erfc(z6 / math.sqrt(2.0)), rel=1e-13)
    assert tau[6] == pytest.approx(11.0 / math.sqrt(15.0 * 11.0), rel=1e-15)
    slope = mk.slope()[0].tolist()
    lo, hi = (w[0].tolist() for w in mk.slope_interval())
    assert slope[2] == 0.0 and lo[2] == 0.0 and hi[2] == 0.0
    for i in (3, 4):
        assert math.isnan(slope[i]) and math.isnan(lo[i]) and math.isnan(hi[i])
    assert slope[5] == lo[5] == hi[5] == np.float32(3.0 / 7.0)    # the one slope of the two points
    assert mk.slope(per=10.0)[0].tolist()[5] == np.float32(3.0 / 7.0) * np.float32(10.0)
    assert mk.slope()[0].dtype == torch.float32
    sig = mk.significant()[0].tolist()
    assert sig == [True, True, False, False, False, False, p[6] <= 0.05]
    assert mk.significant(alpha=1e-9)[0].tolist() == [False] * 7


def test_the_ranks_are_the_formulas():
    rs = np.random.RandomState(3)
    y, t = _series(31, 40, rs)
    mk = MannKendall.fit([torch.from_numpy(np.ascontiguousarray(y.T))], t, alpha=0.2, kern=mr.MkDouble())
    z = -NormalDist().inv_cdf(0.1)
    keys, N = mr.slope_keys(y, t)
    want = []
    for i in range(40):
        v, G = int(mk.stats[0][0, i]), int(mk.stats[0][3, i])
        sigma = math.sqrt((v * (v - 1) * (2 * v + 5) - G) / 18.0)
        n = int(N[i])
        want.append([(n - 1) // 2, n // 2, max(round((n - z * sigma) / 2.0) - 1, 0), min(round((n + z * sigma) / 2.0), n - 1)])
    assert mktrend.interval_ranks(mk.stats[0], 0.2).tolist() == np.array(want).T.tolist()
    bits = mr.select(keys, N, np.array(want).T)
    assert np.array_equal(mk.slopes[0].numpy().view(np.uint32), bits)


def test_variance_scale():
    rs = np.random.RandomState(5)
    y, t = _series(25, 30, rs)
    Yt = torch.from_numpy(np.ascontiguousarray(y.T))
    scale = torch.from_numpy(rs.uniform(1.0, 4.0, size=30))
    plain = MannKendall.fit([Yt], t, kern=mr.MkDouble())
    wide = MannKendall.fit([Yt], t, variance_scale=[scale], kern=mr.MkDouble())
    assert torch.equal(wide.variance()[0], plain.variance()[0] * scale)
    s = plain.stats[0][1].to(torch.float64)
    zw = (s - torch.sign(s)) / torch.sqrt(wide.variance()[0])
    assert torch.allclose(wide.z()[0], zw, rtol=1e-15, atol=0.0)
    assert bool((wide.p_value()[0] >= plain.p_value()[0]).all())
    (lo0, hi0), (lo1, hi1) = ([w[0] for w in f.slope_interval()] for f in (plain, wide))
    assert bool((lo1 <= lo0).all()) and bool((hi1 >= hi0).all()) and bool((lo1 < lo0).any())
    assert torch.equal(wide.slope()[0], plain.slope()[0])
    with pytest.raises(ValueError, match="variance_scale"):
        MannKendall.fit([Yt], t, variance_scale=[scale[:-1]], kern=mr.MkDouble())
    with pytest.raises(ValueError, match="variance scales"):
        MannKendall.fit([Yt], t, variance_scale=[scale, scale], kern=mr.MkDouble())


def _bh(p, alpha):
    p = np.sort(p[~np.isnan(p)])
    ok = p <= np.arange(1, p.size + 1) / max(p.size, 1) * alpha
    return float(p[ok].max()) if ok.any() else 0.0


def test_fdr_threshold():
    rs = np.random.RandomState(11)
    p = np.concatenate([rs.rand(300), rs.rand(60) * 1e-3, [np.nan] * 7])
    rs.shuffle(p)
    blocks = [torch.from_numpy(p[:100]), torch.from_numpy(p[100:])]
    for alpha in (0.01, 0.05, 0.2, 1.0):
        assert fdr_threshold(blocks, alpha) == _bh(p, alpha)
    assert 0.0 < fdr_threshold(blocks, 0.05) < 0.05
    assert fdr_threshold([torch.tensor([0.5, 0.9, float("nan")])], 0.05) == 0.0
    assert fdr_threshold([torch.tensor([float("nan")])], 0.05) == 0.0 and fdr_threshold([], 0.05) == 0.0
    y, t = _series(30, 50, np.random.RandomState(2))
    mk = MannKendall.fit([torch.from_numpy(np.ascontiguousarray(y[:20].T)), torch.from_numpy(np.ascontiguousarray(y[20:].T))],
                         t, kern=mr.MkDouble())
    pv = mk.p_value()
    thr = _bh(np.concatenate([q.numpy() for q in pv]), 0.05)
    assert [s.tolist() for s in mk.significant(fdr=True)] == [(q <= thr).tolist() for q in pv]
    assert sum(int(s.sum()) for s in mk.significant(fdr=True)) <= sum(int(s.sum()) for s in mk.significant())


def test_period_years():
    import pstat_ref as pr
    from dmd_era5_amd.extremes import PeriodStats

    times = np.arange(np.datetime64("2000-07-02T00"), np.datetime64("2003-03-01T00"), np.timedelta64(12, "h"))
    X = torch.from_numpy(np.random.RandomState(0).rand(times.shape[0], 3).astype(np.float32))
    ps = PeriodStats.fit([X], times, period="year", group=2, inner="max", kern=pr.PstatDouble())
    years = ps.period_years()
    assert years.dtype == np.float64 and years.tolist() == [2000.5, 2001.0, 2002.0, 2003.0]   # 183 of 366 days
    mk = MannKendall.fit(ps.series("maximum"), years, kern=mr.MkDouble())
    assert mk.n_valid()[0].tolist() == [4, 4, 4]
    months = PeriodStats.fit([X], times, period="month", group=2, inner="max", kern=pr.PstatDouble()).period_years()
    assert months[1] == 2000.0 + (31 + 29 + 31 + 30 + 31 + 30 + 31) / 366.0 and months[6] == 2001.0
    bare = PeriodStats.fit([X], None, period=[0, 10, 20], group=2, inner="max", kern=pr.PstatDouble())
    with pytest.raises(ValueError, match="period_years"):
        bare.period_years()


def test_datetime_coordinates_are_days_since_the_first():
    y, _ = _series(12, 6, np.random.RandomState(4))
    Yt = torch.from_numpy(np.ascontiguousarray(y.T))
    days = np.array([0, 1, 2, 4, 8, 9, 10, 20, 21, 22, 30, 31.5])
    stamps = np.datetime64("2001-03-01T00") + (days * 24).astype("timedelta64[h]")
    a = MannKendall.fit([Yt], stamps, kern=mr.MkDouble())
    b = MannKendall.fit([Yt], days, kern=mr.MkDouble())
    assert np.array_equal(a.coord, days) and torch.equal(a.slopes[0].view(torch.int32), b.slopes[0].view(torch.int32))


def test_dataset_round_trip_through_a_file(tmp_path):
    rs = np.random.RandomState(9)
    y, t = _series(20, 11, rs)
    blocks = [torch.from_numpy(np.ascontiguousarray(y[:7].T)), torch.from_numpy(np.ascontiguousarray(y[7:].T))]
    scale = [torch.from_numpy(rs.uniform(1.0, 2.0, size=7)), torch.from_numpy(rs.uniform(1.0, 2.0, size=4))]
    for vs in (None, scale):
        mk = MannKendall.fit(blocks, t, alpha=0.1, variance_scale=vs, kern=mr.MkDouble())
        path = str(tmp_path / f"mk_{vs is None}.nc")
        io_netcdf.to_netcdf(mk.to_dataset(), path)
        back = MannKendall.from_dataset(io_netcdf.open_dataset(path), rows=[7, 4], kern=mr.MkDouble())
        assert back.alpha == 0.1 and np.array_equal(back.coord, t) and (back.variance_scale is None) == (vs is None)
        for b in range(2):
            assert back.stats[b].dtype == torch.int32 and torch.equal(back.stats[b], mk.stats[b])
            assert torch.equal(back.slopes[b].view(torch.int32), mk.slopes[b].view(torch.int32))
            assert torch.equal(back.p_value()[b], mk.p_value()[b])
            if vs is not None:
                assert torch.equal(back.variance_scale[b], vs[b])
        one = MannKendall.from_dataset(io_netcdf.open_dataset(path), kern=mr.MkDouble())
        assert tuple(one.stats[0].shape) == (4, 11)
        with pytest.raises(ValueError, match="rows"):
            MannKendall.from_dataset(io_netcdf.open_dataset(path), rows=[7, 5], kern=mr.MkDouble())


def test_errors():
    Y = torch.zeros((129, 4), dtype=torch.float32)
    with pytest.raises(ValueError, match="Trend.fit"):
        MannKendall.fit([Y], np.arange(129.0), kern=mr.MkDouble())
    with pytest.raises(ValueError, match="Trend.fit"):
        mk_blocks([Y], kern=mr.MkDouble())
    Y = torch.zeros((10, 4), dtype=torch.float32)
    with pytest.raises(ValueError, match="block 1"):
        MannKendall.fit([Y, Y[:9]], np.arange(10.0), kern=mr.MkDouble())
    with pytest.raises(ValueError, match="ascending"):
        MannKendall.fit([Y], np.array([0.0, 1, 2, 3, 3, 5, 6, 7, 8, 9]), kern=mr.MkDouble())
    with pytest.raises(ValueError, match="ascending"):
        MannKendall.fit([Y], np.array([0.0, 1, 2, 3, np.nan, 5, 6, 7, 8, 9]), kern=mr.MkDouble())
    with pytest.raises(ValueError, match="alpha"):
        MannKendall.fit([Y], np.arange(10.0), alpha=1.0, kern=mr.MkDouble())
    with pytest.raises(ValueError, match="no blocks"):
        MannKendall.fit([], np.arange(10.0), kern=mr.MkDouble())
    with pytest.raises(ValueError, match="rank tables"):
        sen_blocks([Y], np.arange(10.0), [], kern=mr.MkDouble())
    with pytest.raises(ValueError, match="positive"):
        MannKendall.fit([Y], np.arange(10.0), kern=mr.MkDouble()).slope_interval(per=-1.0)
    with pytest.raises(ValueError, match=r"\(time points, rows\) block"):
        mk_blocks([torch.zeros(10, dtype=torch.float32)], kern=mr.MkDouble())
    assert mktrend.MAX_POINTS == mr.MkDouble.mk_max_n == 128

    class Longer(mr.MkDouble):
        mk_max_n = 256

    with pytest.raises(RuntimeError, match="256 time points"):
        MannKendall.fit([Y], np.arange(10.0), kern=Longer())


def test_the_alias_package_names_the_same_objects():
    import dmd_era5.mktrend as alias

    assert alias.MannKendall is MannKendall and alias.fdr_threshold is fdr_threshold
    assert set(alias.__all__) == set(mktrend.__all__)
