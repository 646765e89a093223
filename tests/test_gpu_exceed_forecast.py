"""The exceedance layer on the GPU: DmdForecast.ensemble_exceedance / exceedance_fields through the HIP provider (K24)
against forecast.exceed_blocks of the numpy double (tests/exceed_ref.py) on the same inputs, within the summation
bounds, and the probability fields through pack_field_blocks and back."""
import numpy as np
import pytest
import torch

import exceed_ref as xr
import expand_ref as er
from test_ensemble import _members
from test_exceed import DoubleWithExceed

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _t(a, device="cpu"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32).to(device)


@pytest.fixture(scope="module")
def fit():
    """503 physical rows in two blocks, delay 2 (U blocks of 2 x rows), k = 12, T = 40, B = 11, two groups in many
    runs, some masked rows with NaN in the analysis, J = 2 thresholds in S = 3 slots at the lower and the upper third
    of the members' values; the bag is perturbed by 0.4 (the members disagree on more than a tenth of the elements), the
    analysis is one more model of the bag plus noise, so both outcomes occur."""
    from dmd_era5_amd.bopdmd import OptDMDResult
    from dmd_era5_amd.forecast import DmdForecast, exceed_blocks, member_coefficients
    from dmd_era5_amd.kernels import default_kernels

    rs = np.random.RandomState(24)
    rows, k, T, B, d, G, J, S = (300, 203), 12, 40, 11, 2, 2, 2, 3
    members = _members(B + 1, k, seed=8, eps=0.4)
    truth, members = members[B], members[:B]
    res = OptDMDResult(eigs=members[0].eigs, modes=members[0].modes, amplitudes=members[0].amplitudes, rel_error=0.0,
                       n_iter=0, converged=True, trials=members)
    Ub = [(rs.standard_normal((k, d * mb)) / np.sqrt(mb)).astype(np.float32) for mb in rows]
    mu = [rs.standard_normal(mb).astype(np.float32) for mb in rows]
    sd = [(0.5 + rs.rand(mb)).astype(np.float32) for mb in rows]
    w = [(0.1 + rs.rand(mb)).astype(np.float32) for mb in rows]
    lab = [rs.randint(0, G, mb) for mb in rows]
    t = torch.from_numpy(np.linspace(0.0, 4.0, T + d - 1))
    Cm, imag = member_coefficients(members, t[:T])
    Ctruth = member_coefficients([truth], t)[0][0].numpy().astype(np.float64)            # (T + d - 1, k)
    slot = rs.randint(0, S, T).astype(np.int32)
    X, thr = [], []
    for b, mb in enumerate(rows):
        dev = np.stack([Cm[j].numpy().astype(np.float64) @ Ub[b][:, :mb] for j in range(B)])   # (B, T, mb), in units of sd
        lo, hi = np.quantile(dev, [1 / 3, 2 / 3])
        noise = 0.3 * dev.std() * rs.standard_normal((T + d - 1, mb))
        X.append((mu[b] + sd[b] * (Ctruth @ Ub[b][:, :mb] + noise)).astype(np.float32))
        thr.append(np.stack([mu[b] + sd[b] * q * (1.0 + 0.1 * rs.standard_normal((S, mb))) for q in (lo, hi)]).astype(np.float32))
        gone = rs.choice(mb, 17, replace=False)
        w[b][gone] = 0.0
        X[b][:, gone] = np.nan
    groups = [torch.from_numpy(v) for v in lab]
    f = DmdForecast([_t(u, DEV) for u in Ub], res, [_t(v, DEV) for v in mu], [_t(v, DEV) for v in sd], delay=d,
                    kern=default_kernels())
    thd = [_t(v, DEV) for v in thr]
    got = f.ensemble_exceedance([_t(x, DEV) for x in X], t[:T], thd, slot, weights=[_t(v, DEV) for v in w], groups=groups,
                                want_rows=True)
    want = exceed_blocks([_t(u) for u in Ub], Cm, [_t(x) for x in X], [_t(v) for v in thr], slot, True, [_t(v) for v in mu],
                         [_t(v) for v in sd], [_t(v) for v in w], groups, d, want_rows=True, kern=DoubleWithExceed())
    # the summation bounds of the double's own elements per group, and the elements whose count the fp32 fields of the
    # kernel may see differently: a member within its error of a threshold
    C = Cm.numpy().reshape(B * T, k).T
    dS, near = np.zeros((G, J, 4, T)), np.zeros((G, J, T))
    for b, mb in enumerate(rows):
        m2, s2, w2, l2 = (np.tile(v[b], d) for v in (mu, sd, w, lab))
        E = np.stack([X[b][j:j + T].T for j in range(d)]).reshape(d * mb, T)
        th2 = np.tile(thr[b], (1, 1, d)).reshape(J * S, d * mb).T.copy()                     # (d mb, J S)
        U = Ub[b].T
        F64 = np.stack([er.expand64(U, C[:, j * T:(j + 1) * T], m2, s2) for j in range(B)])
        err = np.stack([er.element_bound(U, C[:, j * T:(j + 1) * T], m2, s2) for j in range(B)])
        the = xr.thresholds_of(th2, J, S, T, slot).astype(np.float64)                        # (J, d mb, T)
        close = (np.abs(F64[None] - the[:, None]) <= err[None]).any(axis=1)
        for g in range(G):
            s = (l2 == g) & (w2 != 0)
            dS[g] += xr.score_bounds(F64[:, s].astype(np.float32), E[s], th2[s], J, S, slot, True, w2[s])[0]
            near[g] += (close[:, s] * w2[s][None, :, None]).sum(axis=1)
    return dict(f=f, t=t[:T], thd=thd, slot=slot, got=got, want=want, dS=dS, near=near, imag=imag, B=B, T=T, G=G, J=J,
                rows=rows, d=d)


def test_ensemble_exceedance_matches_exceed_blocks_of_the_double(fit):
    got, want, B, T = fit["got"], fit["want"], fit["B"], fit["T"]
    assert got["imag_ratio"] == fit["imag"] and set(got) == set(want) | {"imag_ratio"}
    sums, ref = got["sums"].cpu().numpy(), want["sums"].numpy()
    assert sums.shape == (fit["G"], fit["J"], 4, T)
    # a count that differs by one moves p by 1 / B and a quantity by less than 2 / B
    slack = fit["dS"] + (2.0 / B) * fit["near"][:, :, None, :]
    assert (np.abs(sums - ref) <= slack + 1e-13 * np.abs(ref)).all()
    assert torch.equal(got["weight"].cpu(), want["weight"]) and torch.equal(got["rows"].cpu(), want["rows"])
    assert torch.equal(got["masked_rows"].cpu(), want["masked_rows"]) and int(got["masked_rows"].sum()) == 2 * 17 * fit["d"]
    cnt, cref = got["counts"].cpu().numpy(), want["counts"].numpy()
    assert np.array_equal(cnt.sum(axis=(2, 3)), cref.sum(axis=(2, 3)))
    for g in range(fit["G"]):
        for j in range(fit["J"]):
            if fit["near"][g, j].sum() == 0:
                assert np.array_equal(cnt[g, j], cref[g, j]), (g, j)
            else:
                assert np.abs(cnt[g, j] - cref[g, j]).sum() <= 2 * np.count_nonzero(fit["near"][g, j]) * max(fit["rows"]), (g, j)
    # what keeps the comparison honest: both outcomes and mixed counts are there, the bound resolves the score
    assert (cref[:, :, :, 1:B].sum(axis=(2, 3)) > 0.1 * cref.sum(axis=(2, 3))).all() and (cref.sum(axis=3) > 0).all()
    assert (fit["dS"][:, :, 0] <= 1e-3 * ref[:, :, 0]).all()
    # the scores of every (group, threshold) whose counts are settled: no member within its error of a threshold
    settled = [(g, j) for g in range(fit["G"]) for j in range(fit["J"]) if fit["near"][g, j].sum() == 0]
    assert len(settled) >= 1
    for g, j in settled:
        for key in ("brier", "brier_fair", "base_rate", "forecast_rate", "brier_skill"):
            for suffix in ("", "_total"):
                a, b = got[key + suffix][g, j].cpu().numpy(), want[key + suffix][g, j].numpy()
                assert np.allclose(a, b, rtol=1e-4, atol=1e-6), (key + suffix, g, j)
        for key in ("reliability", "bin_counts", "reliability_term", "resolution_term", "uncertainty", "roc_area"):
            a, b = got[key][g, j].cpu().numpy(), want[key][g, j].numpy()
            assert np.allclose(a, b, rtol=1e-12, atol=1e-14, equal_nan=True), (key, g, j)
    if len(settled) == fit["G"] * fit["J"]:
        for a, b in zip(got["row_brier"], want["row_brier"]):
            assert np.allclose(a.cpu().numpy(), b.numpy(), rtol=1e-4, atol=1e-7, equal_nan=True)
    assert bool((got["roc_area"] > 0.5).all())


def test_exceedance_fields_are_the_planes_of_the_kernel_and_pack(fit):
    """The (J, T, rows) fields of the physical rows are exceed_prob_blocks of the trials; multiples of 1 / B in
    [0, 1]; each threshold's fields go through pack_field_blocks and come back within half a code."""
    from dmd_era5_amd.forecast import exceed_prob_blocks, member_coefficients, pack_field_blocks

    f, B = fit["f"], fit["B"]
    P = f.exceedance_fields(fit["t"], fit["thd"], fit["slot"])
    Cm = member_coefficients(f.result.trials, fit["t"])[0].to(DEV)
    full = exceed_prob_blocks(f.Ublocks, Cm, fit["thd"], fit["slot"], True, f.means, f.stds, delay=fit["d"], kern=f.kern)
    for p, q, mb in zip(P, full, fit["rows"]):
        assert p.shape == (fit["J"], fit["T"], mb) and p.dtype == torch.float32
        assert torch.equal(p, q[:, :, :mb])
        c = p.cpu().numpy().astype(np.float64) * B
        assert np.abs(c - np.rint(c)).max() < 1e-5 and c.min() >= 0 and c.max() <= B
        assert np.array_equal(p.cpu().numpy(), (np.rint(c) / B).astype(np.float32))
    for j in range(fit["J"]):
        packed = pack_field_blocks([p[j] for p in P], kern=f.kern)
        pk = packed["packing"][0]
        assert int(packed["filled"][0]) == 0 and int(packed["saturated"][0]) == 0
        for p, codes in zip(P, packed["codes"]):
            back = pk.decode(codes.cpu().numpy())
            assert np.abs(back - p[j].cpu().numpy()).max() <= 0.5 * pk.scale_factor * (1 + 1e-6) + 1e-7
