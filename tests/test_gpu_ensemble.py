"""The ensemble layer on the GPU: DmdForecast.ensemble_fields / ensemble_score through the HIP provider (K12 for
the mean, K15 for the spread) against the CPU kernel double, within the bounds of tests/expand_ref.py and
tests/spread_ref.py."""
import numpy as np
import pytest
import torch

import expand_ref as er
import spread_ref as sr
from test_ensemble import DoubleWithSpread, _members

pytestmark = pytest.mark.gpu
DEV = "cuda"
U24 = 2.0 ** -24


def _t(a, device="cpu"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32).to(device)


def test_ensemble_fields_and_score_match_the_double():
    """m = 1003 physical rows in two blocks, delay 2 (U blocks of 2 x rows), k = 12, T = 40, B = 6."""
    from dmd_era5_amd.bopdmd import OptDMDResult
    from dmd_era5_amd.forecast import DmdForecast, ensemble_coefficients
    from dmd_era5_amd.kernels import default_kernels

    rs = np.random.RandomState(15)
    rows, k, T, B, d = (500, 503), 12, 40, 6, 2
    members = _members(B, k, seed=8)
    res = OptDMDResult(eigs=members[0].eigs, modes=members[0].modes, amplitudes=members[0].amplitudes, rel_error=0.0,
                       n_iter=0, converged=True, trials=members)
    Ub = [(rs.standard_normal((k, d * mb)) / np.sqrt(mb)).astype(np.float32) for mb in rows]
    mu = [rs.standard_normal(mb).astype(np.float32) for mb in rows]
    sd = [(0.5 + rs.rand(mb)).astype(np.float32) for mb in rows]
    t = torch.from_numpy(np.linspace(0.0, 4.0, T))
    Cbar, Dev, _ = ensemble_coefficients(members, t)
    Cm, D = Cbar.numpy().T, sr.dev_matrix(Dev.numpy())
    # snapshots: T + d - 1 of them per block, the ensemble mean's physical field plus noise
    X = [(rs.standard_normal((T + d - 1, mb)) * 0.1).astype(np.float32) for mb in rows]

    def bundle(device, kern):
        return DmdForecast([_t(u, device) for u in Ub], res, [_t(v, device) for v in mu], [_t(v, device) for v in sd],
                           delay=d, kern=kern)

    hip, cpu = bundle(DEV, default_kernels()), bundle("cpu", DoubleWithSpread())
    (mh, sh), (mc, sc) = hip.ensemble_fields(t), cpu.ensemble_fields(t)
    for b, mb in enumerate(rows):
        U0 = Ub[b][:, :mb].T                                              # delay block 0: the physical rows
        assert mh[b].shape == sh[b].shape == (T, mb)
        want_m, want_s = mc[b].numpy().T.astype(np.float64), sc[b].numpy().T.astype(np.float64)
        # the double is fp64 rounded once to fp32: u relative on top of the kernel's bound against fp64
        assert (np.abs(mh[b].cpu().numpy().T - want_m) <= er.element_bound(U0, Cm, mu[b], sd[b]) + U24 * np.abs(want_m)).all()
        assert (np.abs(sh[b].cpu().numpy().T - want_s) <= sr.spread_bound(U0, D, T, B, sd[b]) + U24 * want_s).all()
        assert not bool(torch.signbit(sh[b]).any())

    rh = hip.ensemble_score([_t(x, DEV) for x in X], t, want_rows=True)
    rc = cpu.ensemble_score([_t(x) for x in X], t, want_rows=True)
    dv, ds = np.zeros(T), np.zeros(T)
    for b, mb in enumerate(rows):                                         # all d * rows rows of a block are scored
        m2, s2 = np.tile(mu[b], d), np.tile(sd[b], d)
        E = np.stack([X[b][j:j + T].T for j in range(d)]).reshape(d * mb, T)
        dv += sr.spread_score_bounds(Ub[b].T, D, T, B, s2)[0]
        ds += er.score_bounds(Ub[b].T, Cm, E, m2, s2)[0]
        brow = sr.spread_score_bounds(Ub[b].T, D, T, B, s2)[1]
        got, want = (r["row_spread"][b].cpu().numpy().astype(np.float64) ** 2 * T for r in (rh, rc))
        assert (np.abs(got - want) <= brow + 1e-13 * want).all()
    var_h, var_c, sse_h, sse_c = (r[key].cpu().numpy() for key in ("var", "sse") for r in (rh, rc))
    assert (np.abs(var_h - var_c) <= dv).all() and (np.abs(sse_h - sse_c) <= ds).all()
    assert abs(rh["var_total"] - rc["var_total"]) <= dv.sum() and abs(rh["sse_total"] - rc["sse_total"]) <= ds.sum()
    assert rh["rows"] == rc["rows"] == d * sum(rows)
    lo, hi = np.sqrt((var_c - dv) / (sse_c + ds)), np.sqrt((var_c + dv) / (sse_c - ds))
    skill = rh["spread_skill"].cpu().numpy()
    assert (lo * (1 - 1e-14) <= skill).all() and (skill <= hi * (1 + 1e-14)).all()
    lo_t = np.sqrt((rc["var_total"] - dv.sum()) / (rc["sse_total"] + ds.sum()))
    hi_t = np.sqrt((rc["var_total"] + dv.sum()) / (rc["sse_total"] - ds.sum()))
    assert lo_t * (1 - 1e-14) <= rh["spread_skill_total"] <= hi_t * (1 + 1e-14)
    assert abs(rh["spread_skill_total"] - rc["spread_skill_total"]) < 1e-4 * rc["spread_skill_total"]


def test_wrappers_match_the_double():
    """HipKernels.spread / spread_score with a contiguous Dev whose k = 5 vectors are not on 16-byte boundaries
    (re-pitched like Ct of K12) and with the pitched image forecast.py hands over, out= views with a row stride,
    accumulation into ``out`` and the per-row sums."""
    from dmd_era5_amd.forecast import _pitched_dev
    from dmd_era5_amd.kernels import default_kernels

    KERN = default_kernels()
    rs = np.random.RandomState(16)
    m, k, T, B = 333, 5, 41, 7
    U = rs.standard_normal((m, k)).astype(np.float32)
    Dev = rs.standard_normal((B, T, k)).astype(np.float32)
    sd = ((0.5 + rs.rand(m)) * rs.choice([-1.0, 1.0], m)).astype(np.float32)
    D = sr.dev_matrix(Dev)
    Ut, Dt, st = _t(U.T, DEV), _t(Dev, DEV), _t(sd, DEV)
    assert KERN.spread_max_k == 256
    got = KERN.spread(Ut, Dt, st)
    assert got.shape == (T, m)
    assert (np.abs(got.cpu().numpy().T - sr.spread64(U, D, T, B, sd)) <= sr.spread_bound(U, D, T, B, sd)).all()
    Dp = _pitched_dev(KERN, Dt)
    assert Dp.stride() == (T * 8, 8, 1) and torch.equal(KERN.spread(Ut, Dp, st), got)
    big = torch.full((T, m + 7), -7.0, device=DEV)
    KERN.spread(Ut, Dt, st, out=big[:, 3:3 + m])
    assert torch.equal(big[:, 3:3 + m], got) and bool((big[:, :3] == -7).all()) and bool((big[:, 3 + m:] == -7).all())
    var, rows = KERN.spread_score(Ut, Dt, st, want_rows=True)
    want, bounds = sr.spread_score64(U, D, T, B, sd), sr.spread_score_bounds(U, D, T, B, sd)
    for g, w, b in zip((var, rows), want, bounds):
        assert (np.abs(g.cpu().numpy() - w) <= b).all()
    again, none = KERN.spread_score(Ut, Dp, st, out=var.clone())
    assert none is None and torch.equal(again, 2 * var)
    with pytest.raises(Exception):
        KERN.spread(Ut, _t(np.zeros((B, T, k + 1), dtype=np.float32), DEV))
    with pytest.raises(Exception):
        KERN.spread_score(Ut, Dt, st, out=torch.zeros(T + 1, dtype=torch.float64, device=DEV))
