"""The CRPS layer on the GPU: DmdForecast.ensemble_crps through the HIP provider (K19) against tests/crps_ref.py,
within its bounds propagated to the scores."""
import numpy as np
import pytest
import torch

import crps_ref as cr
from test_ensemble import _members

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _t(a, device="cpu"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32).to(device)


@pytest.fixture(scope="module")
def fit():
    """m = 1003 physical rows in two blocks, delay 2 (U blocks of 2 x rows), k = 12, T = 40, B = 11 (one full member
    block and a partial one), two groups in many runs, some masked rows with NaN in the analysis; the bag of
    tests/test_gpu_ensemble.py.  -> (results fair / plain, the reference's per-group sums, bounds, W, members)."""
    from dmd_era5_amd.bopdmd import OptDMDResult
    from dmd_era5_amd.forecast import DmdForecast, member_coefficients
    from dmd_era5_amd.kernels import default_kernels

    rs = np.random.RandomState(19)
    rows, k, T, B, d, G = (500, 503), 12, 40, 11, 2, 2
    members = _members(B, k, seed=8)
    res = OptDMDResult(eigs=members[0].eigs, modes=members[0].modes, amplitudes=members[0].amplitudes, rel_error=0.0,
                       n_iter=0, converged=True, trials=members)
    Ub = [(rs.standard_normal((k, d * mb)) / np.sqrt(mb)).astype(np.float32) for mb in rows]
    mu = [rs.standard_normal(mb).astype(np.float32) for mb in rows]
    sd = [(0.5 + rs.rand(mb)).astype(np.float32) for mb in rows]
    w = [(0.1 + rs.rand(mb)).astype(np.float32) for mb in rows]
    lab = [rs.randint(0, G, mb) for mb in rows]
    X = [(m_[None] + rs.standard_normal((T + d - 1, mb)) * 0.02).astype(np.float32) for mb, m_ in zip(rows, mu)]
    for b in range(2):
        gone = rs.choice(rows[b], 17, replace=False)
        w[b][gone] = 0.0
        X[b][:, gone] = np.nan
    t = torch.from_numpy(np.linspace(0.0, 4.0, T))
    f = DmdForecast([_t(u, DEV) for u in Ub], res, [_t(v, DEV) for v in mu], [_t(v, DEV) for v in sd], delay=d,
                    kern=default_kernels())
    kw = dict(weights=[_t(v, DEV) for v in w], groups=[torch.from_numpy(v) for v in lab])
    Xd = [_t(x, DEV) for x in X]
    got = {fair: f.ensemble_crps(Xd, t, fair=fair, want_rows=fair, **kw) for fair in (True, False)}
    Cm, imag = member_coefficients(members, t)
    C = Cm.numpy().reshape(B * T, k).T
    S, dS, W, H = np.zeros((G, 2, T)), np.zeros((G, 2, T)), np.zeros(G), np.zeros((G, B + 1), dtype=np.int64)
    rowsums = []
    for b, mb in enumerate(rows):                                         # all d * rows rows of a block are scored
        m2, s2, w2, l2 = (np.tile(v[b], d) for v in (mu, sd, w, lab))
        E = np.stack([X[b][j:j + T].T for j in range(d)]).reshape(d * mb, T)
        with np.errstate(all="ignore"):
            rowsums.append(cr.crps64(Ub[b].T, C, T, B, E, m2, s2, None)[1])
        for g in range(G):
            s = (l2 == g) & (w2 != 0)
            args = (Ub[b].T[s], C, T, B, E[s], m2[s], s2[s], w2[s])
            col, _, hist = cr.crps64(*args)
            S[g] += col
            dS[g] += cr.crps_bounds(*args)[0]
            H[g] += hist
            W[g] += w2[s].astype(np.float64).sum()
    # the counts exactly: the fp32 member fields of K12 against the analysis, per group
    H32 = np.zeros((G, B + 1), dtype=np.int64)
    for b, mb in enumerate(rows):
        E = torch.stack([Xd[b][j:j + T] for j in range(d)], dim=1).reshape(T, d * mb)
        m2, s2 = f.means[b].repeat(d), f.stds[b].repeat(d)
        below = sum((f.kern.expand(f.Ublocks[b], Cm[j].to(DEV), m2, s2) < E).to(torch.int64) for j in range(B))
        w2, l2 = np.tile(w[b], d), np.tile(lab[b], d)
        below = below.cpu().numpy()
        for g in range(G):
            H32[g] += np.bincount(below[:, (l2 == g) & (w2 != 0)].ravel(), minlength=B + 1)
    return dict(got=got, H32=H32, S=S, dS=dS, W=W, H=H, B=B, T=T, imag=imag, rowsums=rowsums, w=w, d=d, rows=rows)


def test_ensemble_crps_matches_the_reference(fit):
    B, T = fit["B"], fit["T"]
    for fair in (True, False):
        res = fit["got"][fair]
        assert res["imag_ratio"] == fit["imag"]
        sums = res["sums"].cpu().numpy()
        assert (np.abs(sums - fit["S"]) <= fit["dS"]).all()
        assert np.allclose(res["weight"].cpu().numpy(), fit["W"], rtol=1e-14)
        assert int(res["masked_rows"].sum()) == 2 * 17 * fit["d"] and int(res["rows"].sum()) == fit["d"] * sum(fit["rows"])
        # the counts: every selected element is in a bin, and the bins are those of the fp32 fields of K12
        hist = res["rank_hist"].cpu().numpy()
        assert np.array_equal(hist.sum(axis=1), fit["H"].sum(axis=1))
        assert np.array_equal(hist, fit["H32"])
        for g in range(len(fit["W"])):
            want = cr.scores(fit["S"][g], fit["W"][g], B, fair)
            bound = cr.score_bounds(fit["dS"][g], fit["W"][g], B, fair)
            tw = cr.scores(fit["S"][g].sum(axis=1), fit["W"][g] * T, B, fair)
            tb = cr.score_bounds(fit["dS"][g].sum(axis=1), fit["W"][g] * T, B, fair)
            for key in ("crps", "member_mae", "member_distance"):
                v = res[key][g].cpu().numpy()
                assert (np.abs(v - want[key]) <= bound[key] + 1e-13 * np.abs(want[key])).all(), (key, g, fair)
                assert abs(float(res[key + "_total"][g]) - tw[key]) <= tb[key] + 1e-13 * abs(tw[key]), (key, g, fair)
                # what keeps the comparison honest: the bound resolves the score to a hundredth of itself
                assert (bound[key] <= 1e-2 * np.abs(want[key])).all(), (key, g)
    rc = fit["got"][True]["row_crps"]
    assert len(rc) == 2
    for b, (got, row) in enumerate(zip(rc, fit["rowsums"])):
        live = np.tile(fit["w"][b], fit["d"]) != 0
        want = row[0] / (B * T) - row[1] / (B * (B - 1) * T)
        g = got.cpu().numpy()
        assert np.isnan(g[~live]).all() and np.allclose(g[live], want[live], rtol=1e-4, atol=1e-7)


def test_plain_crps_is_at_most_the_member_error(fit):
    """CRPS = E|x - y| - E|x - x'| / 2 <= E|x - y| for the empirical distribution of the members, and >= 0; the fair
    estimator takes more off.  Both hold for the computed sums as well: every term that is taken off is >= 0."""
    plain, fair = fit["got"][False], fit["got"][True]
    assert bool((plain["crps"] <= plain["member_mae"]).all()) and bool((plain["crps_total"] <= plain["member_mae_total"]).all())
    assert bool((fair["crps"] <= plain["crps"]).all())
    assert torch.equal(fair["sums"], plain["sums"]) and torch.equal(fair["rank_hist"], plain["rank_hist"])
    assert bool((plain["crps"] > 0).all())
