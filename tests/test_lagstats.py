"""Host side of K26 without a GPU: tests/lag_ref.py (the definition the kernel is held to) against a direct evaluation
over the exact pairs, and baseline.LagStats / baseline_scores / skill on the kernel double lag_ref.LagDouble against
plain numpy; the refusals of the new C entry point, which need no GPU.

Error bound used throughout.  Each of S, H, E and P is a recursive fp64 sum of at most T terms (in segments, then over
the segments: at most T + 1 additions touch a term) of products rounded once, and every |term| of P is at most the mean
of two terms of S: each carries at most (T + 1) 2^-53 S.  Q = A + B - 2 P = 2 S - E - H - 2 P weighs them with 6; the
rest of 8 T 2^-53 S covers the final roundings.
"""
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import lag_ref as lr
from lag_ref import LagDouble
from test_crps import TwoRanks

U53 = 2.0 ** -53
T0 = 37


def _era(m, T=T0, seed=0):
    rs = np.random.RandomState(seed + m)
    X = (250.0 + 30.0 * rs.standard_normal((m, T))).astype(np.float32)
    return X, X.mean(axis=1).astype(np.float32)


def _wide(m, T=T0, seed=0):
    rs = np.random.RandomState(seed + 7 * m)
    return (rs.standard_normal((m, T)) * 2.0 ** rs.uniform(-12, 12, (m, T))).astype(np.float32)


def _parts(planes, L):
    S = planes[0]
    return S, planes[1:1 + L], S[None] - planes[1 + 2 * L:1 + 3 * L], S[None] - planes[1 + L:1 + 2 * L]


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


# ---------------------------------------------------------------- the reference itself
def test_reference_on_era_like_data_equals_the_exact_sums():
    """250 + 30 N about its fp32 mean: d has at most 24 bits on a grid of 2^-16, every product and every partial sum is
    exact in fp64, so S, P, A and B are the exact sums whatever the partition."""
    X, mu = _era(5)
    lags = (0, 1, 5, 16, T0 - 1)
    L = len(lags)
    d = X.astype(np.float64) - mu.astype(np.float64)[:, None]
    for seg in (8, T0, 1024):
        S, P, A, B = _parts(lr.moments(X, lags, mu, seg), L)
        for i in range(X.shape[0]):
            assert S[i] == math.fsum(v * v for v in d[i])
            for l, tau in enumerate(lags):
                pairs = [(d[i, u - tau], d[i, u]) for u in range(tau, T0)]
                assert P[l, i] == math.fsum(a * b for a, b in pairs), (seg, i, tau)
                assert A[l, i] == math.fsum(a * a for a, _ in pairs), (seg, i, tau)
                assert B[l, i] == math.fsum(b * b for _, b in pairs), (seg, i, tau)


@pytest.mark.parametrize("with_mu", [False, True])
def test_reference_on_wide_range_data_is_within_the_summation_bound(with_mu):
    """x = N(0, 1) 2^U(-12, 12): the sums round, and Q = A + B - 2 P from the planes stays within 8 T 2^-53 S of the
    sum of (d_u - d_{u - tau})^2 over the exact pairs, evaluated in rational arithmetic."""
    m = 6
    X = _wide(m)
    mu = np.random.RandomState(3).standard_normal(m).astype(np.float32) if with_mu else None
    lags = (0, 1, 7, 8, 9, 20, T0 - 1)
    L = len(lags)
    d = X.astype(np.float64) - (0.0 if mu is None else mu.astype(np.float64)[:, None])
    worst = 0.0
    for seg in (1, 8, T0):
        S, P, A, B = _parts(lr.moments(X, lags, mu, seg), L)
        for i in range(m):
            f = [Fraction(float(v)) for v in d[i]]
            for l, tau in enumerate(lags):
                Q = sum(((f[u] - f[u - tau]) ** 2 for u in range(tau, T0)), Fraction(0))
                err = abs(Fraction(float(A[l, i] + B[l, i] - 2.0 * P[l, i])) - Q)
                bound = Fraction(8 * T0 * U53 * float(S[i]))
                worst = max(worst, float(err / bound))
                assert err <= bound, (seg, i, tau, float(err), float(bound))
    print(f"worst |Q_derived - Q| / bound = {worst:.4f}")


def test_reference_partition_matters_on_wide_range_data_only():
    X = _wide(33)
    a, b = lr.moments(X, (1, 9, 20), None, 8), lr.moments(X, (1, 9, 20), None, T0)
    for lo, hi in ((0, 1), (1, 4), (4, 7), (7, 10)):                       # S, P, H, E
        assert (a[lo:hi].view(np.uint64) != b[lo:hi].view(np.uint64)).any()
    Xe, mu = _era(33)
    assert np.array_equal(lr.moments(Xe, (1, 9, 20), mu, 8).view(np.uint64), lr.moments(Xe, (1, 9, 20), mu, T0).view(np.uint64))


def test_reference_value_rules():
    X = _wide(4)
    X[1] = 0.0
    X[2, 3] = np.nan
    lags = (0, 2, 5)
    Q = lr.moments(X, lags, None, 8)
    assert (Q[:, 1].view(np.uint64) == 0).all()                              # +0.0 in every plane of the zero row
    clean = lr.moments(_wide(4), lags, None, 8)
    assert np.array_equal(Q[:, [0, 3]].view(np.uint64), clean[:, [0, 3]].view(np.uint64))
    # t = 3 is in S, every P, H of tau = 5 (the head [0, 5)) and no tail (T - 5 = 32 > 3)
    want = np.zeros(10, dtype=bool)
    want[[0, 1, 2, 3, 6]] = True
    assert np.array_equal(np.isnan(Q[:, 2]), want)


# ---------------------------------------------------------------- LagStats against plain numpy
def _ramp_blocks(T=50, rows=(9, 4), seed=1):
    """x_t = t N: the head is small and the tail large, so A (earlier members) and B (later) differ widely."""
    rs = np.random.RandomState(seed)
    t = np.arange(1, T + 1, dtype=np.float64)[:, None]
    return [(t * rs.standard_normal((T, mb))).astype(np.float32) for mb in rows]


def _plain(X, mu, lags):
    """name -> (L, rows) fp64 by the textbook formulas on shifted views; X (T, rows)."""
    d = X.astype(np.float64) - (0.0 if mu is None else mu.astype(np.float64)[None, :])
    T = d.shape[0]
    out = {k: [] for k in ("P", "A", "B", "n")}
    for tau in lags:
        e, later = d[:T - tau], d[tau:]
        out["P"].append((e * later).sum(axis=0))
        out["A"].append((e * e).sum(axis=0))
        out["B"].append((later * later).sum(axis=0))
        out["n"].append(np.full(d.shape[1], T - tau, dtype=np.float64))
    out = {k: np.stack(v) for k, v in out.items()}
    out["S"] = (d * d).sum(axis=0)
    return out


def test_every_method_against_its_definition():
    from dmd_era5_amd.baseline import SEGMENT, LagStats

    T, lags = 50, (0, 1, 3, 10, 49)
    X = _ramp_blocks(T)
    rs = np.random.RandomState(2)
    mus = [rs.standard_normal(x.shape[1]).astype(np.float32) for x in X]
    times = np.datetime64("2020-01-01T00", "h") + np.arange(T) * np.timedelta64(6, "h")
    stats = LagStats.fit([_t(x) for x in X], lags, centres=[_t(mu) for mu in mus], times=times, kern=LagDouble())
    assert SEGMENT == 1024 and stats.T == T and stats.lags == lags and stats.pairs().tolist() == [50, 49, 47, 40, 1]
    assert stats.step == np.timedelta64(6, "h") and np.array_equal(stats.leads(), np.array(lags) * np.timedelta64(6, "h"))
    got = {name: getattr(stats, name)() for name in ("autocovariance", "autocorrelation", "damping", "persistence_mse",
                                                     "damped_mse", "climatology_mse")}
    for b, (x, mu) in enumerate(zip(X, mus)):
        assert np.array_equal(stats.planes[b].numpy().view(np.uint64), lr.moments(x.T, lags, mu, 1024).view(np.uint64))
        w = _plain(x, mu, lags)
        P, A, B, n, S = w["P"], w["A"], w["B"], w["n"], w["S"]
        eps = 8 * T * U53 * S[None]                                            # on a sum (module docstring)
        assert (np.abs(A[2] - B[2]) > 1e6 * eps[0]).all()                      # head and tail differ: a swap shows
        want = {"autocovariance": (P / n, eps / n), "climatology_mse": (B / n, eps / n),
                "persistence_mse": ((A + B - 2 * P) / n, eps / n), "damped_mse": ((B - P * P / A) / n, 3 * eps / n),
                # a ratio of two sums of the size of S: first order in the relative errors eps / A, eps / B
                "autocorrelation": (P / np.sqrt(A * B), 2 * eps / np.minimum(A, B)), "damping": (P / A, 2 * eps / A)}
        for name, (val, tol) in want.items():
            g = got[name][b].numpy()
            assert g.shape == val.shape and g.dtype == np.float64, name
            assert (np.abs(g - val) <= tol).all(), (name, b, np.abs(g - val).max())
        # the wrong direction is far outside the tolerance
        assert (np.abs(got["damping"][b].numpy()[2] - P[2] / B[2]) > 1e3 * (2 * eps[0] / A[2])).all()
        assert np.allclose(got["autocorrelation"][b].numpy()[0], 1.0, rtol=0, atol=1e-14)   # lag 0


def _binding_rows(T=T0, seed=11):
    """(T, 6) fp32, taken as anomalies (no centre), on which damped persistence nearly or exactly equals one of the
    other two.  In exact arithmetic persistence - damped = (A - P)^2 / (A n) and climatology - damped = P^2 / (A n).
      0  a constant: A = P = B, alpha = 1 exactly, damped = persistence = 0
      1  a level of 1000 with a few fp32 ulps of noise: alpha = 1 to 1e-8, persistence - damped far below the bound
      2  a random walk: alpha close to 1 at lag 1, the gap small against the scores but above the bound
      3  (1, 0, -1, 0) 1000: P = 0 exactly at the odd lags (damped = climatology), P = -A at lag 2 (damped = 0)
      4  the same with a few 2^-14 of noise: P tiny and not 0 at the odd lags, climatology - damped far below the bound
      5  white noise: P small against A at every lag, the gap above the bound"""
    rs = np.random.RandomState(seed)
    t = np.arange(T)
    wave = 1000.0 * np.array([1.0, 0.0, -1.0, 0.0])[t % 4]
    cols = [np.full(T, 1000.0), 1000.0 + 2.0 ** -14 * rs.randint(-3, 4, T), rs.standard_normal(T).cumsum(), wave,
            wave + 2.0 ** -14 * rs.randint(-3, 4, T), rs.standard_normal(T)]
    return np.stack(cols, axis=1).astype(np.float32)


def test_damped_persistence_is_never_worse_than_the_other_two():
    """damped_mse <= min(persistence_mse, climatology_mse) + 8 T 2^-53 S / n per row and lag (the bound of the module
    docstring on a sum, over n for a mean square), on the wide-range and the ERA-like data and on rows where the
    inequality binds: there the exact gap is inside the bound, so only the bound lets the computed values pass."""
    from dmd_era5_amd.baseline import LagStats

    T, lags = T0, (1, 2, 9, 30)
    bind = _binding_rows(T)
    X = [_wide(40).T.copy(), _era(25)[0].T.copy(), bind]
    stats = LagStats.fit([_t(x) for x in X], lags, centres=[None, _t(_era(25)[1]), None], kern=LagDouble())
    n = (T - np.array(lags, dtype=np.float64))[:, None]
    tols = []
    for Q, dm, pm, cm in zip(stats.planes, stats.damped_mse(), stats.persistence_mse(), stats.climatology_mse()):
        tol = 8 * T * U53 * Q[0].numpy()[None] / n
        tols.append(tol)
        assert (dm.numpy() >= 0).all() and (pm.numpy() >= 0).all()
        assert (dm.numpy() <= np.minimum(pm.numpy(), cm.numpy()) + tol).all()
    # the binding rows do bind: the gaps over the exact pairs, in rational arithmetic, against the bound
    gap_p, gap_c = np.empty((len(lags), bind.shape[1])), np.empty((len(lags), bind.shape[1]))
    for i in range(bind.shape[1]):
        f = [Fraction(float(v)) for v in bind[:, i]]
        for l, tau in enumerate(lags):
            P = sum((f[u - tau] * f[u] for u in range(tau, T)), Fraction(0))
            A = sum((f[u - tau] ** 2 for u in range(tau, T)), Fraction(0))
            gap_p[l, i], gap_c[l, i] = float((A - P) ** 2 / A / (T - tau)), float(P ** 2 / A / (T - tau))
    tol, odd = tols[2], [0, 2]                                                  # lags 1 and 9
    assert (gap_p[:, 0] == 0).all() and (gap_p[:, 1] > 0).all() and (gap_p[:, 1] < tol[:, 1]).all()          # alpha = 1
    assert (gap_c[odd, 3] == 0).all() and (gap_c[odd, 4] > 0).all() and (gap_c[odd, 4] < tol[odd, 4]).all()  # P = 0
    assert (gap_p[0, 2] > tol[0, 2]) and (gap_c[:, 5] > tol[:, 5]).all()                     # and rows that do not bind
    dm, pm, cm = stats.damped_mse()[2].numpy(), stats.persistence_mse()[2].numpy(), stats.climatology_mse()[2].numpy()
    assert np.array_equal(dm[:, 0], pm[:, 0]) and (dm[:, 0] == 0).all()
    assert np.array_equal(dm[odd, 3], cm[odd, 3]) and (dm[1, 3] == 0) and (cm[1, 3] > 0)
    assert (np.abs(dm[:, 1] - pm[:, 1]) <= tol[:, 1]).all() and (np.abs(dm[odd, 4] - cm[odd, 4]) <= tol[odd, 4]).all()


def test_effective_sample_size_of_a_planted_ar1():
    from dmd_era5_amd.baseline import LagStats

    phi, T, m = 0.8, 4000, 3
    rs = np.random.RandomState(20)
    e = rs.standard_normal((T, m))
    x = np.empty((T, m))
    x[0] = e[0] / math.sqrt(1 - phi * phi)
    for t in range(1, T):
        x[t] = phi * x[t - 1] + e[t]
    stats = LagStats.fit([_t(x)], (1, 2), kern=LagDouble())
    (r,), (neff,) = stats.autocorrelation(), stats.effective_sample_size()
    r1 = r[0].numpy()
    print("r1 =", r1)
    assert (np.abs(r1 - phi) <= 5 * math.sqrt((1 - phi * phi) / T)).all()
    assert neff.shape == (m,) and np.array_equal(neff.numpy(), T * (1.0 - r1) / (1.0 + r1))
    assert (neff.numpy() < T / 5).all()                                       # (1 - 0.8) / (1 + 0.8) = 1 / 9


def test_errors_and_more_than_eight_lags():
    from dmd_era5_amd.baseline import LagStats, lag_moments_blocks

    X = [_t(x) for x in _ramp_blocks(40)]
    times = np.datetime64("2020-01-01", "h") + np.arange(40) * np.timedelta64(1, "h")
    LagDouble.lag_calls = 0
    with pytest.raises(ValueError, match="evenly spaced"):
        LagStats.fit(X, (1,), times=np.concatenate([times[:20], times[20:] + np.timedelta64(1, "h")]), kern=LagDouble())
    with pytest.raises(ValueError, match="datetime64"):
        LagStats.fit(X, (1,), times=np.arange(40), kern=LagDouble())
    with pytest.raises(ValueError, match="block 0 holds 40 snapshots, times has 39"):
        LagStats.fit(X, (1,), times=times[:39], kern=LagDouble())
    for bad in ((), (2, 1), (1, 1), (-1, 2), (1.5,)):
        with pytest.raises(ValueError, match="lags"):
            LagStats.fit(X, bad, kern=LagDouble())
    with pytest.raises(ValueError, match="largest lag 40"):
        LagStats.fit(X, (1, 40), kern=LagDouble())
    assert LagDouble.lag_calls == 0                                           # all before any launch
    with pytest.raises(ValueError, match="block 1 holds 39"):
        LagStats.fit([X[0], X[1][:39]], (1,), kern=LagDouble())
    with pytest.raises(ValueError, match="lag 1 was not fitted"):
        LagStats.fit(X, (0, 2), kern=LagDouble()).effective_sample_size()
    with pytest.raises(ValueError, match="no units"):
        LagStats.fit(X, (1,), kern=LagDouble()).leads()
    # eleven lags: two launches per block, the planes of each group in their places
    lags = (0, 1, 2, 3, 5, 8, 13, 21, 22, 30, 39)
    LagDouble.lag_calls = 0
    planes = lag_moments_blocks(X, lags, kern=LagDouble())
    assert LagDouble.lag_calls == 2 * len(X)
    L = len(lags)
    for Q, x in zip(planes, X):
        first, second = lr.moments(x.numpy().T, lags[:8], None, 1024), lr.moments(x.numpy().T, lags[8:], None, 1024)
        Q = Q.numpy()
        assert Q.shape == (1 + 3 * L, x.shape[1])
        assert np.array_equal(Q[0], first[0]) and np.array_equal(Q[0], second[0])
        for q in range(3):
            assert np.array_equal(Q[1 + q * L:1 + q * L + 8], first[1 + q * 8:1 + (q + 1) * 8])
            assert np.array_equal(Q[1 + q * L + 8:1 + (q + 1) * L], second[1 + q * 3:1 + (q + 1) * 3])


# ---------------------------------------------------------------- baseline_scores
ROWS = (70, 100, 70)
G = 4


def _grid(seed=5, T=60):
    rs = np.random.RandomState(seed)
    M = sum(ROWS)
    t = np.arange(T)[:, None]
    X = (rs.standard_normal((T, M)).cumsum(axis=0) * 0.5 + np.sin(t / 5.0) * rs.standard_normal(M)[None]).astype(np.float32)
    w = (0.1 + rs.rand(M)).astype(np.float32)
    lab = rs.randint(0, G, M)                                                 # unsorted: every group in many runs
    lab[ROWS[0] + ROWS[1]:][lab[ROWS[0] + ROWS[1]:] == 3] = 2                 # group 3 is absent from the last block
    nan_rows = [5, 100, 200]
    w[rs.choice(np.setdiff1d(np.arange(M), nan_rows), 9, replace=False)] = 0.0
    X[7, nan_rows[0]], X[0, nan_rows[1]], X[T - 1, nan_rows[2]] = np.nan, np.inf, np.nan
    zero_and_nan = int(np.flatnonzero(w == 0)[0])
    X[3, zero_and_nan] = np.nan                                               # counted once
    edges = np.cumsum((0,) + ROWS)
    cut = lambda v: [v[..., a:b] for a, b in zip(edges[:-1], edges[1:])]
    return X, w, lab, cut


def _baseline_numpy(X, w, lab, lags, Gn):
    T = X.shape[0]
    p = _plain(X, None, lags)
    keep = (w != 0) & np.isfinite(p["S"])
    out = {k: np.zeros((Gn, len(lags))) for k in ("rmse_persistence", "rmse_damped", "rmse_climatology", "acc_persistence",
                                                   "skill_persistence_vs_clim")}
    meta = np.zeros((3, Gn))
    n = T - np.array(lags, dtype=np.float64)
    for g in range(Gn):
        sel = keep & (lab == g)
        ww = w[sel].astype(np.float64)[None]
        P, A, B = (p[k][:, sel] for k in "PAB")
        W = ww.sum()
        sQ, sB = (ww * (A + B - 2 * P)).sum(axis=1), (ww * B).sum(axis=1)
        out["rmse_persistence"][g] = np.sqrt(sQ / (W * n))
        out["rmse_damped"][g] = np.sqrt((ww * (B - P * P / A)).sum(axis=1) / (W * n))
        out["rmse_climatology"][g] = np.sqrt(sB / (W * n))
        out["acc_persistence"][g] = (ww * P).sum(axis=1) / np.sqrt((ww * A).sum(axis=1) * sB)
        out["skill_persistence_vs_clim"][g] = 1 - sQ / sB
        meta[:, g] = W, (lab == g).sum(), ((lab == g) & ~keep).sum()
    return out, meta


def test_baseline_scores_against_the_weighted_numpy_expressions():
    from dmd_era5_amd.baseline import LagStats, baseline_scores

    X, w, lab, cut = _grid()
    lags = (1, 2, 6, 24)
    stats = LagStats.fit([_t(x) for x in cut(X)], lags, kern=LagDouble())
    res = baseline_scores(stats, weights=[_t(v) for v in cut(w)], groups=[_t(v, torch.int64) for v in cut(lab)])
    want, meta = _baseline_numpy(X, w, lab, lags, G)
    for key, v in want.items():
        assert res[key].shape == (G, len(lags)) and np.isfinite(res[key].numpy()).all(), key
        assert np.allclose(res[key].numpy(), v, rtol=1e-11, atol=1e-12), key      # sums of 60 x 240 terms in fp64
    assert res["sums"].shape == (G, 4, len(lags))
    assert np.allclose(res["weight"].numpy(), meta[0], rtol=1e-14)
    assert res["rows"].tolist() == meta[1].tolist() and res["masked_rows"].tolist() == meta[2].tolist()
    assert int(res["masked_rows"].sum()) == 9 + 3                               # the weight-0 rows and the three others
    assert ((res["rmse_damped"] <= res["rmse_persistence"] + 1e-12) & (res["rmse_damped"] <= res["rmse_climatology"] + 1e-12)).all()
    # one group, no weights: every row counts 1
    one = baseline_scores(stats)
    w1, _ = _baseline_numpy(X, np.ones_like(w), np.zeros_like(lab), lags, 1)
    assert np.allclose(one["rmse_persistence"].numpy(), w1["rmse_persistence"], rtol=1e-11)
    assert one["rows"].tolist() == [sum(ROWS)] and one["masked_rows"].tolist() == [4]
    for bad in (-1.0, np.nan, np.inf):
        wb = [_t(v).clone() for v in cut(w)]
        wb[1][3] = bad
        with pytest.raises(ValueError, match="weights of block 1"):
            baseline_scores(stats, weights=wb)
    with pytest.raises(ValueError, match="label 3 with n_groups"):
        baseline_scores(stats, groups=[_t(v, torch.int64) for v in cut(lab)], n_groups=3)
    with pytest.raises(ValueError, match="2 weight vectors"):
        baseline_scores(stats, weights=[_t(v) for v in cut(w)][:2])


def test_two_row_shards_one_collective():
    from dmd_era5_amd.baseline import LagStats, baseline_scores

    X, w, lab, cut = _grid()
    lags = (1, 6)
    Xb, wb, gb = [_t(x) for x in cut(X)], [_t(v) for v in cut(w)], [_t(v, torch.int64) for v in cut(lab)]
    one = baseline_scores(LagStats.fit(Xb, lags, kern=LagDouble()), weights=wb, groups=gb)
    c1 = TwoRanks()
    baseline_scores(LagStats.fit(Xb[2:], lags, kern=LagDouble()), weights=wb[2:], groups=gb[2:], comm=c1, n_groups=G)
    assert c1.tags == ["baseline_allreduce"]
    c0 = TwoRanks(other=c1.sent)
    res = baseline_scores(LagStats.fit(Xb[:2], lags, kern=LagDouble()), weights=wb[:2], groups=gb[:2], comm=c0, n_groups=G)
    assert c0.tags == ["baseline_allreduce"]
    for key in ("sums", "weight", "rmse_persistence", "rmse_damped", "rmse_climatology", "acc_persistence",
                "skill_persistence_vs_clim"):
        assert torch.allclose(res[key], one[key], rtol=1e-13, atol=1e-15), key
    assert torch.equal(res["rows"], one["rows"]) and torch.equal(res["masked_rows"], one["masked_rows"])


def test_skill_is_one_minus_the_ratio():
    from dmd_era5_amd.baseline import skill

    a, b = torch.tensor([[1.0, 4.0], [0.0, 9.0]], dtype=torch.float64), torch.tensor([[2.0, 4.0], [5.0, 3.0]], dtype=torch.float64)
    assert torch.equal(skill(a, b), torch.tensor([[0.5, 0.0], [1.0, -2.0]], dtype=torch.float64))
    assert np.array_equal(skill(np.array([1.0, 3.0]), np.array([4.0, 4.0])), np.array([0.75, 0.25]))


# ---------------------------------------------------------------- persistence, alias, C entry point
@pytest.mark.skipif(not __import__("dmd_era5_amd.hdf5_lite", fromlist=["x"]).available(), reason="libhdf5 not found")
def test_dataset_round_trip_through_a_file(tmp_path):
    from dmd_era5_amd import io_netcdf
    from dmd_era5_amd.baseline import LagStats
    from dmd_era5_amd.labeled import Coord

    rows = (9, 4)
    X = [_t(x) for x in _ramp_blocks(40, rows)]
    times = np.datetime64("2020-01-01", "h") + np.arange(40) * np.timedelta64(3, "h")
    stats = LagStats.fit(X, (0, 1, 8), times=times, kern=LagDouble())
    M = sum(rows)
    coords = {"space": Coord("space", np.arange(M, dtype=np.int64)), "latitude": Coord("space", np.linspace(-60.0, 60.0, M)),
              "time": Coord("time", times)}
    ds = stats.to_dataset(coords)
    assert ds["lag_moments"].dims == ("plane", "space") and ds["lag_moments"].shape == (10, M) and "time" not in ds.coords
    path = str(tmp_path / "lagstats.nc")
    io_netcdf.to_netcdf(ds, path)
    back = LagStats.from_dataset(io_netcdf.open_dataset(path), rows=rows, device="cpu", kern=LagDouble())
    assert (back.T, back.lags, back.step) == (40, (0, 1, 8), np.timedelta64(3, "h"))
    for P, Q in zip(back.planes, stats.planes):
        assert P.dtype == torch.float64 and np.array_equal(P.numpy().view(np.uint64), Q.numpy().view(np.uint64))
    assert all(torch.equal(a, b) for a, b in zip(back.autocorrelation(), stats.autocorrelation()))
    one = LagStats.from_dataset(io_netcdf.open_dataset(path), device="cpu", kern=LagDouble())
    assert len(one.planes) == 1 and one.planes[0].shape == (10, M)
    plain = LagStats.fit(X, (1,), kern=LagDouble())
    other = str(tmp_path / "plain.nc")
    io_netcdf.to_netcdf(plain.to_dataset(), other)
    assert LagStats.from_dataset(io_netcdf.open_dataset(other), device="cpu", kern=LagDouble()).step is None
    with pytest.raises(ValueError, match="rows sum"):
        LagStats.from_dataset(io_netcdf.open_dataset(path), rows=(3, 4), device="cpu", kern=LagDouble())


def test_alias_package_re_exports_the_module():
    import dmd_era5.baseline as alias
    import dmd_era5_amd.baseline as mod

    assert alias.LagStats is mod.LagStats and alias.skill is mod.skill and set(alias.__all__) == set(mod.__all__)


def test_argument_errors_of_the_entry_point_are_reported_without_a_gpu():
    import ctypes

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists(os.path.join(root, "dmd_era5_amd", "libdmdx.so")):
        import __graft_entry__

        __graft_entry__.build()
    from dmd_era5_amd import _lib

    lib = _lib.load()
    assert (lib.dmdx_lag_moments_max_lags(), lib.dmdx_version()) == (8, 110) and lib.dmdx_lag_moments_ring() in (8, 16, 32)
    one = 0x1000                # a non-null aligned address that is never used: every call below is refused before a launch
    lags = (ctypes.c_int32 * 9)(0, 1, 2, 5, 8, 9, 10, 20, 30)
    good = dict(X=one, m=10, T=37, ldx=12, mu=None, lags=lags, L=3, seg=8, out=one + 0x10000, ldo=10, flags=0, ws=None, wsb=0,
                stream=None)

    def call(**over):
        a = dict(good)
        a.update(over)
        return lib.dmdx_lag_moments_f32(*a.values())

    bad = [dict(L=0), dict(L=9), dict(L=-1), dict(lags=None), dict(lags=(ctypes.c_int32 * 3)(0, 2, 2)),
           dict(lags=(ctypes.c_int32 * 3)(2, 1, 5)), dict(lags=(ctypes.c_int32 * 3)(-1, 1, 5)),
           dict(lags=(ctypes.c_int32 * 3)(0, 1, 37)), dict(seg=0), dict(seg=-3), dict(seg=2 ** 31), dict(ldo=9), dict(ldx=9),
           dict(out=one + 0x10004), dict(X=one + 2), dict(mu=one + 1), dict(flags=2), dict(flags=3), dict(flags=-2),
           dict(X=None), dict(out=None), dict(m=-1), dict(T=-1), dict(m=2 ** 31, ldx=2 ** 31, ldo=2 ** 31),
           dict(ws=one + 0x100004, wsb=1 << 30), dict(ws=one + 0x100000, wsb=5 * 4 * 10 * 8 - 1), dict(out=one + 8)]
    for over in bad:
        assert call(**over) == -1000, over
        assert b"lag_moments" in lib.dmdx_last_error()
    assert lib.dmdx_lag_moments_workspace_bytes(10, 37, 3, 8) == 5 * 4 * 10 * 8
    for args in ((10, 37, 0, 8), (10, 37, 9, 8), (10, 37, 3, 0), (-1, 37, 3, 8), (2 ** 31, 37, 3, 8)):
        assert lib.dmdx_lag_moments_workspace_bytes(*args) == 0
    # empty shapes pass the checks and launch nothing: null X and out are allowed then
    assert call(m=0, X=None, out=None) == 0 and call(T=0, X=None, out=None) == 0
