"""The host layer of K26 on the HIP provider: LagStats.fit + baseline_scores equal what the kernel double of
tests/lag_ref.py gives, bit for bit, and a forecast scored by verify_blocks combines with the baselines through
skill()."""
import numpy as np
import pytest
import torch

from lag_ref import LagDouble

pytestmark = pytest.mark.gpu

ROWS = (1029, 517)
G = 3


def _t(a, dtype=torch.float32, device="cpu"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(device)


@pytest.fixture(scope="module")
def hip():
    from dmd_era5_amd.kernels import default_kernels

    return default_kernels()


def _case(T, seed=0):
    rs = np.random.RandomState(seed)
    X = [(rs.standard_normal((T, mb)).cumsum(axis=0) * 2.0 ** rs.uniform(-6, 6, (1, mb))).astype(np.float32) for mb in ROWS]
    mu = [x.mean(axis=0).astype(np.float32) for x in X]
    w = [(0.1 + rs.rand(mb)).astype(np.float32) for mb in ROWS]
    lab = [rs.randint(0, G, mb) for mb in ROWS]
    w[0][5], w[1][7] = 0.0, 0.0
    X[0][3, 11], X[1][T - 1, 2] = np.nan, np.inf
    return X, mu, w, lab


def test_fit_and_scores_equal_the_kernel_double_bit_for_bit(hip):
    from dmd_era5_amd.baseline import SEGMENT, LagStats, baseline_scores

    T = SEGMENT + 76                                              # two segments: the split form
    lags = (0, 1, hip.lag_ring, hip.lag_ring + 8)
    X, mu, w, lab = _case(T)
    times = np.datetime64("2020-01-01", "h") + np.arange(T) * np.timedelta64(1, "h")
    res = {}
    for name, kern, dev in (("hip", hip, "cuda"), ("double", LagDouble(), "cpu")):
        stats = LagStats.fit([_t(x, device=dev) for x in X], lags, centres=[_t(v, device=dev) for v in mu], times=times,
                             kern=kern)
        res[name] = stats, baseline_scores(stats, weights=[_t(v, device=dev) for v in w],
                                           groups=[_t(v, torch.int64) for v in lab])
    (sh, bh), (sd, bd) = res["hip"], res["double"]
    for P, Q in zip(sh.planes, sd.planes):
        assert P.is_cuda and P.dtype == torch.float64
        got, want = P.cpu().numpy(), Q.numpy()
        ok = (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))
        assert ok.all(), f"{int((~ok).sum())} plane elements differ"
    assert int(bh["masked_rows"].sum()) == 4 and bh["rows"].tolist() == bd["rows"].tolist()
    for key, v in bd.items():
        got = bh[key].cpu().numpy()
        assert np.isfinite(got).all() and np.array_equal(got.view(np.uint64 if got.dtype == np.float64 else np.int64),
                                                         v.numpy().view(np.uint64 if got.dtype == np.float64 else np.int64)), key
    n_eff = sh.effective_sample_size()
    assert n_eff[0].shape == (ROWS[0],) and float(n_eff[0][0]) < T / 10         # a random walk: r1 close to 1


def test_the_wrapper_refuses_lags_the_int32_table_would_wrap(hip):
    from dmd_era5_amd._lib import DmdxError

    T = 40
    X = _t(np.random.RandomState(1).standard_normal((T, 9)), device="cuda")
    out = torch.full((4, 9), -7.0, dtype=torch.float64, device="cuda")
    for bad in ((2 ** 32 + 1,), (1, 2 ** 32 + 2), (-(2 ** 32) + 1,), (T,), (1, T), (-1,), (2, 1), (1, 1)):
        with pytest.raises(DmdxError, match="strictly ascending with 0 <= tau < T = 40"):
            hip.lag_moments(X, bad, out=out if len(bad) == 1 else None)
    assert bool((out == -7.0).all())                              # refused before a launch
    assert hip.lag_moments(X, (T - 1,), out=out).data_ptr() == out.data_ptr() and bool((out != -7.0).all())


def test_a_verified_forecast_against_the_baselines_through_skill(hip):
    from dmd_era5_amd.baseline import LagStats, baseline_scores, skill
    from dmd_era5_amd.forecast import verify_blocks

    T, k, lags = 48, 5, (1, 2, 6)
    rs = np.random.RandomState(4)
    U = [rs.standard_normal((k, mb)).astype(np.float32) / np.sqrt(k) for mb in ROWS]
    t = np.arange(T)[:, None]
    C = (np.cos(t * np.linspace(0.1, 0.5, k)[None]) * np.exp(-0.01 * t)).astype(np.float32)
    clim = [(3.0 * rs.standard_normal(mb)).astype(np.float32) for mb in ROWS]
    X = [(c[None] + C @ u + 0.2 * rs.standard_normal((T, mb))).astype(np.float32) for c, u, mb in zip(clim, U, ROWS)]
    w = [(0.1 + rs.rand(mb)).astype(np.float32) for mb in ROWS]
    lab = [np.sort(rs.randint(0, G, mb)) for mb in ROWS]
    dev = lambda vs, dt=torch.float32: [_t(v, dt, "cuda") for v in vs]
    Xd, wd, cd, gd = dev(X), dev(w), dev(clim), [_t(v, torch.int64) for v in lab]
    ver = verify_blocks(dev(U), _t(C, device="cuda"), Xd, means=cd, weights=wd, clims=cd, groups=gd, kern=hip)
    base = baseline_scores(LagStats.fit(Xd, lags, centres=cd, kern=hip), weights=wd, groups=gd)
    assert ver["rmse"].shape == (G, T) and base["rmse_persistence"].shape == (G, len(lags))
    # both sides take anomalies about the same centre with the same weights: the mean square of the analysis anomaly
    # over the snapshots u >= tau (S4 / W of verify_blocks, fp32 anomalies summed in fp64) is the climatology baseline
    S4, W = ver["sums"][:, 4].cpu().numpy(), ver["weight"].cpu().numpy()
    for l, tau in enumerate(lags):
        want = S4[:, tau:].mean(axis=1) / W
        assert np.allclose(base["rmse_climatology"][:, l].cpu().numpy() ** 2, want, rtol=1e-5, atol=0), tau
    mse = ver["rmse"].cpu()[:, list(lags)] ** 2                          # the forecast at the leads tau from its start
    for key in ("rmse_persistence", "rmse_damped", "rmse_climatology"):
        s = skill(mse, base[key] ** 2)
        assert s.shape == (G, len(lags)) and torch.equal(s, 1.0 - mse / base[key] ** 2)
        assert bool((s > 0).all()), key                            # the planted model beats every baseline
    assert bool((base["rmse_damped"] <= base["rmse_persistence"]).all())
