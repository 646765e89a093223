"""K21 through the package on the GPU: Trend.fit / remove_ / restore_ / at through HipKernels bit for bit against
tests/treg_ref.py, the wrappers' argument checks, and DmdForecast.fields(trend=) against the same call on the CPU
double."""
import dataclasses

import numpy as np
import pytest
import torch

import expand_ref as er
import treg_ref as tr

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROWS = (1029, 515)
T = 61


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    ok = (_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))
    assert got.shape == want.shape and ok.all(), f"{what}: {int((~ok).sum())} of {ok.size} elements differ"


def _times(n=T, start="2019-01-01T00", step_h=150):
    """Uneven: every 150 hours, with every fifth stamp 7 hours late -- 380 days in all."""
    return np.datetime64(start, "h") + (np.arange(n) * step_h + 7 * (np.arange(n) % 5 == 4)) * np.timedelta64(1, "h")


def _snapshots(seed=7):
    rs = np.random.RandomState(seed)
    times = _times()
    days = (times - times[0]).astype(np.float64) / 24.0
    X = []
    for mb in ROWS:
        level, slope, amp = 250.0 + 30.0 * rs.rand(mb), rs.standard_normal(mb), 5.0 * rs.rand(mb)
        X.append((level[None, :] + slope[None, :] * (days / 190.0 - 1.0)[:, None]
                  + amp[None, :] * np.cos(2 * np.pi * days / 365.2425)[:, None] + 0.3 * rs.standard_normal((T, mb)))
                 .astype(np.float32))
    return times, X


def test_fit_remove_restore_at_bit_for_bit():
    from dmd_era5_amd.trend import SEGMENT, Trend, weights

    times, X = _snapshots()
    Xd = [torch.from_numpy(x).to(DEV) for x in X]
    trend = Trend.fit(Xd, times, degree=1, harmonics=1)
    assert trend.kern.name == "hip" and trend.n_terms == 4
    D = trend.design(times)
    W = tr.w_of(D)
    assert np.array_equal(W, weights(D))
    coef = [tr.fit(x.T, W, SEGMENT) for x in X]
    for b in range(2):
        assert trend.coef[b].is_cuda and tuple(trend.coef[b].shape) == (4, ROWS[b])
        _same(trend.coef[b], coef[b], f"fit block {b}")
    out = [torch.full_like(x, 7.0) for x in Xd]
    res = trend.remove_(Xd, times, out=out)
    assert all(r is o for r, o in zip(res, out)) and all(torch.equal(a, torch.from_numpy(b).to(DEV)) for a, b in zip(Xd, X))
    trend.remove_(Xd, times)
    for b in range(2):
        _same(Xd[b], tr.apply(X[b].T, D, coef[b]).T, f"remove_ block {b}")
        assert torch.equal(Xd[b], out[b]) and float(Xd[b].abs().max()) < 3.0          # level, trend and cycle are gone
    trend.restore_(Xd, times)
    for b in range(2):
        _same(Xd[b], tr.apply(tr.apply(X[b].T, D, coef[b]), D, coef[b], restore=True).T, f"restore_ block {b}")
    later = _times(23, "2027-05-01T03", 31)
    F = trend.at(later)
    D2 = trend.design(later)
    for b in range(2):
        assert tuple(F[b].shape) == (23, ROWS[b])
        _same(F[b], tr.fitted(coef[b], D2).astype(np.float32).T, f"at block {b}")
    (s0, s1) = trend.slope()
    assert s0.dtype == torch.float64 and torch.equal(s0, trend.coef[0][1].double() * (3652.425 / trend.half_span_days))
    assert tuple(s1.shape) == (ROWS[1],)


def test_hip_kernels_wrappers():
    """HipKernels.treg_fit / treg_apply_ on strided views, both forms of the fit, and their argument checks."""
    from dmd_era5_amd import _lib
    from dmd_era5_amd.kernels import HipKernels, default_kernels

    kern = default_kernels()
    assert kern.treg_max_p == 8
    m, p, seg = 50, 3, 16
    rs = np.random.RandomState(41)
    X = (250.0 + 30.0 * rs.standard_normal((m, T))).astype(np.float32)
    D = np.ascontiguousarray(np.stack([np.ones(T), np.linspace(-1, 1, T), np.cos(np.arange(T) / 5.0)], axis=1))
    W = tr.w_of(D)
    buf = torch.zeros((T, m + 6), dtype=torch.float32, device=DEV)
    Xt = buf[:, 1:1 + m]
    Xt.copy_(torch.from_numpy(np.ascontiguousarray(X.T)))
    Wd, Dd = torch.from_numpy(W).to(DEV), torch.from_numpy(D).to(DEV)
    want = tr.fit(X, W, seg)
    coef = kern.treg_fit(Xt, Wd, seg)
    _same(coef, want, "treg_fit")
    walk = HipKernels()
    walk.treg_split = False
    _same(walk.treg_fit(Xt, Wd, seg), want, "treg_fit, one lane per row walking the segments")
    wide = torch.full((p, m + 3), 9.0, dtype=torch.float32, device=DEV)
    assert kern.treg_fit(Xt, Wd, seg, out=wide[:, :m]).data_ptr() == wide.data_ptr()
    _same(wide[:, :m], want, "treg_fit out=")
    assert bool((wide[:, m:] == 9.0).all())
    Y = kern.treg_apply_(Xt, Dd, wide[:, :m], out=torch.empty((T, m), dtype=torch.float32, device=DEV))
    _same(Y, tr.apply(X, D, want).T, "treg_apply_ out=")
    assert kern.treg_apply_(Xt, Dd, coef, restore=True) is Xt
    _same(Xt, tr.apply(X, D, want, restore=True).T, "treg_apply_ in place")
    assert bool((buf[:, 0] == 0).all()) and bool((buf[:, 1 + m:] == 0).all())
    for bad in (lambda: kern.treg_fit(Xt, Wd.float(), seg), lambda: kern.treg_fit(Xt.double(), Wd, seg),
                lambda: kern.treg_fit(Xt, Wd[:, :-1], seg), lambda: kern.treg_fit(Xt, Wd, 0),
                lambda: kern.treg_fit(Xt, torch.zeros((9, T), dtype=torch.float64, device=DEV), seg),
                lambda: kern.treg_fit(Xt.cpu(), Wd, seg), lambda: kern.treg_fit(Xt, Wd.cpu(), seg),
                lambda: kern.treg_fit(Xt, Wd, seg, out=wide[:, :m - 1]), lambda: kern.treg_apply_(Xt, Dd[:-1], coef),
                lambda: kern.treg_apply_(Xt, Dd, coef[:, :-1]), lambda: kern.treg_apply_(Xt, Dd, coef[:-1]),
                lambda: kern.treg_apply_(Xt, Dd.float(), coef), lambda: kern.treg_apply_(Xt, Dd, coef, out=Xt[:, 1:]),
                lambda: kern.treg_apply_(Xt, Dd, coef, out=buf[:, 2:2 + m])):
        with pytest.raises(_lib.DmdxError):
            bad()


def test_forecast_fields_with_a_trend_against_the_cpu_double():
    from test_ensemble import _members
    from test_trend import TrendDouble

    from dmd_era5_amd.bopdmd import OptDMDResult
    from dmd_era5_amd.forecast import DmdForecast
    from dmd_era5_amd.trend import Trend

    class Double(TrendDouble, er.ExpandDouble):
        name = "cpu-double+expand+treg"

    times, X = _snapshots(9)
    rs = np.random.RandomState(3)
    k = 7
    base = _members(1, k, seed=2)[0]
    res = OptDMDResult(eigs=base.eigs, modes=base.modes, amplitudes=base.amplitudes, rel_error=0.0, n_iter=0, converged=True)
    U = [rs.standard_normal((k, mb)).astype(np.float32) for mb in ROWS]
    mu = [rs.standard_normal(mb).astype(np.float32) for mb in ROWS]
    sd = [(0.5 + rs.rand(mb)).astype(np.float32) for mb in ROWS]
    trend = Trend.fit([torch.from_numpy(x).to(DEV) for x in X], times, degree=1, harmonics=1)
    cpu_trend = dataclasses.replace(trend, coef=[c.cpu() for c in trend.coef], kern=Double())

    def t_(a, dev):
        return torch.from_numpy(a).to(dev)

    f_dev = DmdForecast([t_(u, DEV) for u in U], res, [t_(v, DEV) for v in mu], [t_(v, DEV) for v in sd])
    f_cpu = DmdForecast([t_(u, "cpu") for u in U], res, [t_(v, "cpu") for v in mu], [t_(v, "cpu") for v in sd], kern=Double())
    tt = torch.from_numpy(np.linspace(0.0, 2.0, 19))
    valid = _times(19, "2020-02-20T00", 17)
    plain = f_dev.fields(tt)
    full = f_dev.fields(tt, trend=trend, times=valid)
    want = f_cpu.fields(tt, trend=cpu_trend, times=valid)
    D = trend.design(valid)
    Cm = f_cpu.coefficients(tt)[0].numpy().T
    for b in range(2):
        coef = trend.coef[b].cpu().numpy()
        # on the device: K12's field, then K21's restore of it, to the bit
        _same(full[b], tr.apply(plain[b].cpu().numpy().T, D, coef, restore=True).T, f"fields(trend=) block {b}")
        # against the double: K12's element bound on the field that goes in (the double rounds its fp64 field once
        # more: half an ulp), carried through fp64(x) + f unchanged, and one rounding to fp32 on either side
        x64 = er.expand64(U[b].T, Cm, mu[b], sd[b])
        into = er.element_bound(U[b].T, Cm, mu[b], sd[b]) + 2.0 ** -24 * np.abs(x64)
        y = want[b].numpy().T.astype(np.float64)
        bound = into + 2.0 ** -23 * (np.abs(y) + into)
        assert (np.abs(full[b].cpu().numpy().T.astype(np.float64) - y) <= bound).all()
        assert np.abs(y - x64).max() > 100.0                     # the level came back
    with pytest.raises(ValueError, match="go together"):
        f_dev.fields(tt, trend=trend)
