"""The host layer of K27 on the HIP provider: SpellStats.fit on device blocks equals the same call on the kernel double
of tests/spell_ref.py, element for element -- with percentile thresholds from a Climatology (K25) across a year
boundary, with more periods than one launch takes, and on the blocks of a DmdForecast."""
import numpy as np
import pytest
import torch

import spell_ref as sr
from spell_ref import SpellDouble

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROWS = (515, 1029)


def _t(a, dtype=torch.float32, device="cpu"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(device)


@pytest.fixture(scope="module")
def hip():
    from dmd_era5_amd.kernels import default_kernels

    return default_kernels()


def _on_host(clim):
    from dmd_era5_amd.climatology import Climatology

    return Climatology(clim.kind, clim.window_days, [M.cpu() for M in clim.mean], None, clim.counts, clim.ddof, None, clim.q,
                       [Q.cpu() for Q in clim.quant], clim.method)


def _same_stats(a, b):
    assert a.bounds.tolist() == b.bounds.tolist() and a.labels.tolist() == b.labels.tolist()
    for P, Q in zip(a.planes, b.planes):
        assert P.is_cuda and P.dtype == torch.int32 and torch.equal(P.cpu(), Q)


def test_fit_with_percentile_thresholds_across_a_year_boundary_equals_the_kernel_double(hip):
    from dmd_era5_amd.climatology import Climatology
    from dmd_era5_amd.spells import SpellStats

    rs = np.random.RandomState(27)
    T = 96
    times = np.datetime64("2020-12-30T00", "h") + np.arange(T) * np.timedelta64(1, "h")
    X = [(280.0 + 3.0 * rs.standard_normal((T, mb)).cumsum(axis=0) / np.sqrt(np.arange(1, T + 1))[:, None]).astype(np.float32)
         for mb in ROWS]
    X[0][7, 3], X[1][50, 11], X[1][95, 0] = np.nan, np.inf, -np.inf
    Xd = [_t(x, device=DEV) for x in X]
    clim = Climatology.fit(Xd, times, "hour", quantiles=(0.25, 0.75), kern=hip)
    w = [(0.1 + rs.rand(mb)).astype(np.float32) for mb in ROWS]
    w[0][5] = 0.0
    lab = [np.sort(rs.randint(0, 3, mb)) for mb in ROWS]
    kw = dict(above=(False, True), min_length=(2, 3))
    got = SpellStats.fit(Xd, times, climatology=clim, kern=hip, **kw)
    want = SpellStats.fit([_t(x) for x in X], times, climatology=_on_host(clim), kern=SpellDouble(), **kw)
    _same_stats(got, want)
    assert got.bounds.tolist() == [0, 48, 96] and got.labels.tolist() == ["2020", "2021"]
    n_spell = torch.cat([q.cpu() for q in got.spell_count()], dim=2)
    assert int(n_spell.min()) == 0 and int(n_spell.max()) >= 2                   # the series do have spells, and rows without
    for name in ("frequency", "spell_count", "spell_days", "longest", "onset", "end"):
        for g, h in zip(getattr(got, name)(), getattr(want, name)()):
            assert torch.equal(g.cpu(), h) or (name == "frequency" and np.array_equal(g.cpu().numpy(), h.numpy(), equal_nan=True))
        a = got.area_mean(name, weights=[_t(v, device=DEV) for v in w], groups=[_t(v, torch.int64) for v in lab])
        b = want.area_mean(name, weights=[_t(v) for v in w], groups=[_t(v, torch.int64) for v in lab])
        for key in ("mean", "weight", "rows"):
            assert np.array_equal(a[key].numpy(), b[key].numpy(), equal_nan=True), (name, key)
    for g, h in zip(got.onset(as_time=True), want.onset(as_time=True)):
        assert np.array_equal(g, h, equal_nan=True)


def test_more_periods_than_one_launch_takes_and_an_out_tensor(hip):
    from dmd_era5_amd._lib import DmdxError
    from dmd_era5_amd.spells import SpellStats, periods_of

    rs = np.random.RandomState(3)
    T, mb = 24 * 150, 131                                          # 150 days of hourly data: 150 periods of 24
    x = rs.standard_normal((T, mb)).astype(np.float32).cumsum(axis=0)
    x -= x.mean(axis=0)
    bounds = np.arange(0, T + 1, 24)
    assert len(bounds) - 1 > hip.spell_max_periods
    got = SpellStats.fit([_t(x, device=DEV)], None, thresholds=[0.0, 1.0], period=bounds, min_length=(3, 1), kern=hip)
    want = sr.spells(x.T, np.array([0.0, 1.0], dtype=np.float32)[:, None, None] * np.ones((2, 1, mb), dtype=np.float32), bounds,
                     [3, 1], True)
    assert np.array_equal(got.planes[0].cpu().numpy(), want)
    days = np.datetime64("2021-01-01T00", "h") + np.arange(T) * np.timedelta64(1, "h")
    assert periods_of(days, "month")[0].tolist() == [0, 744, 1416, 2160, 2880, 3600]
    # the wrapper: out is written in place, every seg gives the same values, bad arguments are refused before a launch
    X, thr = _t(x, device=DEV), torch.zeros((1, mb), device=DEV)
    out = torch.full((1, 7, 2, mb), -7, dtype=torch.int32, device=DEV)
    base = hip.spells(X, thr, [0, 1000, T], 2, True)
    for seg in (1, 100, 512, T):
        assert hip.spells(X, thr, [0, 1000, T], 2, True, seg=seg, out=out).data_ptr() == out.data_ptr() and torch.equal(out, base)
    out.fill_(-7)
    for bad in (dict(bounds=[0, 1000, T + 1]), dict(bounds=[5, 5, 9]), dict(bounds=[0, 1000, 2 ** 32 + 5]), dict(min_len=0),
                dict(min_len=(1, 2)), dict(above=(True, False)), dict(seg=0), dict(bounds=[0, T]),
                dict(slot=torch.zeros(T - 1, dtype=torch.int32, device=DEV))):
        a = dict(bounds=[0, 1000, T], min_len=1, above=True, slot=None, seg=512)
        a.update(bad)
        with pytest.raises(DmdxError):
            hip.spells(X, thr, a["bounds"], a["min_len"], a["above"], slot=a["slot"], seg=a["seg"], out=out)
    assert bool((out == -7).all())


def test_the_spells_of_a_forecast_are_the_spells_of_its_fields(hip):
    """The blocks of DmdForecast.fields are (T, rows) fp32 blocks like any other: the reference runs on the downloaded
    fields."""
    from dmd_era5_amd import bopdmd as bop
    from dmd_era5_amd.forecast import DmdForecast
    from dmd_era5_amd.spells import SpellStats

    t = np.linspace(0, 6, 120)
    half = np.array([-0.05 + 2.0j, -0.1 + 5.0j])
    alpha = np.concatenate([half, half.conj()])
    rs = np.random.RandomState(2)
    mh = rs.standard_normal((2, 4)) + 1j * rs.standard_normal((2, 4))
    H = (np.exp(np.outer(t, alpha)) @ np.concatenate([mh, mh.conj()])).real
    res = bop.optdmd(torch.from_numpy(H).to(torch.complex128).to(DEV), torch.from_numpy(t).to(DEV), 4, tol=1e-10, maxiter=60)
    Q = np.linalg.qr(rs.standard_normal((700, 4)))[0].astype(np.float32)
    blocks = [(0, 300), (300, 700)]
    f = DmdForecast([_t(Q[a:b].T, device=DEV) for a, b in blocks], res)
    n = 72
    fields = f.fields(torch.from_numpy(np.linspace(0, 9, n)).to(DEV))
    times = np.datetime64("2021-02-27T12", "h") + np.arange(n) * np.timedelta64(1, "h")      # into March: two seasons
    kw = dict(thresholds=[0.05, -0.05], above=(True, False), min_length=(3, 2), period="season")
    got = SpellStats.fit(fields, times, kern=hip, **kw)
    want = SpellStats.fit([F.cpu() for F in fields], times, kern=SpellDouble(), **kw)
    _same_stats(got, want)
    assert got.labels.tolist() == ["2021-DJF", "2021-MAM"] and got.bounds.tolist() == [0, 36, 72]
    days = torch.cat([q.cpu() for q in got.spell_days()], dim=2)
    assert int(days.max()) >= 3                                     # the oscillating modes do cross the thresholds
