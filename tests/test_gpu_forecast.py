"""The host layer above K12 on the GPU: HipKernels.expand / expand_score, forecast.py and
era5_svd.reconstruct_from_svd_results through the HIP ``main``."""
import numpy as np
import pytest
import torch

import expand_ref as er

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def KERN():
    from dmd_era5_amd.kernels import default_kernels

    return default_kernels()


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def test_wrappers_match_the_double(KERN):
    """expand / expand_score with an unpitched Ct (k = 5: re-pitched like W of K2), out= views with a
    row stride, accumulation into ``out`` and the per-row sums."""
    rs = np.random.RandomState(0)
    m, k, T = 333, 5, 41
    U, Cm = rs.standard_normal((m, k)).astype(np.float32), rs.standard_normal((k, T)).astype(np.float32)
    mu, sd = rs.standard_normal(m).astype(np.float32), (0.5 + rs.rand(m)).astype(np.float32)
    X = (er.expand64(U, Cm, mu, sd) + rs.standard_normal((m, T))).astype(np.float32)
    Ut, Ct, Xt = _t(U.T), _t(Cm.T), _t(X.T)
    got = KERN.expand(Ut, Ct, _t(mu), _t(sd))
    assert got.shape == (T, m)
    assert (np.abs(got.cpu().numpy().T - er.expand64(U, Cm, mu, sd)) <= er.element_bound(U, Cm, mu, sd)).all()
    big = torch.full((T, m + 7), -7.0, device=DEV)
    KERN.expand(Ut, Ct, _t(mu), _t(sd), out=big[:, 3:3 + m])
    assert torch.equal(big[:, 3:3 + m], got) and bool((big[:, :3] == -7).all()) and bool((big[:, 3 + m:] == -7).all())
    cols, rows = KERN.expand_score(Ut, Ct, Xt, _t(mu), _t(sd), want_rows=True)
    want, bounds = er.score64(U, Cm, X, mu, sd), er.score_bounds(U, Cm, X, mu, sd)
    for g, w, b in zip((cols[0], cols[1], rows), want, bounds):
        assert (np.abs(g.cpu().numpy() - w) <= b).all()
    again, none = KERN.expand_score(Ut, Ct, Xt, _t(mu), _t(sd), out=cols.clone())
    assert none is None and torch.equal(again, 2 * cols)
    with pytest.raises(Exception):
        KERN.expand(Ut, _t(np.zeros((T, k + 1), dtype=np.float32)))


def test_score_blocks_after_svd_snapshots_reproduces_the_truncation_error(KERN):
    """5000 x 96, rank 10: total sse = ||X||^2 - sum s_i^2 within the score bound of the kernel (no other
    allowance: sse 107122.67 against 107100.29, a difference of 22.4 under a bound of 28.95 on an MI355X),
    and per snapshot against fp64 of the same factors within the same bound."""
    from dmd_era5_amd import svd as dsvd
    from dmd_era5_amd.forecast import score_blocks, svd_coefficients

    rs = np.random.RandomState(1)
    m, n, r = 5000, 96, 10
    X = (rs.standard_normal((m, r)) @ (np.diag(np.linspace(30, 3, r)) @ rs.standard_normal((r, n)))
         + 0.5 * rs.standard_normal((m, n))).astype(np.float32)
    Xt = _t(X.T)
    res = dsvd.svd_snapshots(Xt, r)
    Ct = svd_coefficients(res.s, res.Vh).to(DEV)
    blocks = [(0, 2000), (2000, 5000)]
    sc = score_blocks([res.Ut[:, a:b] for a, b in blocks], Ct, [Xt[:, a:b] for a, b in blocks], want_rows=True)
    n2 = float((X.astype(np.float64) ** 2).sum())
    s = res.s.cpu().numpy()
    U, Cm = res.Ut.cpu().numpy().T, Ct.cpu().numpy().T
    bound = er.score_bounds(U, Cm, X)[0].sum()
    assert abs(sc["sse_total"] - (n2 - (s ** 2).sum())) <= bound
    want = er.score64(U, Cm, X)
    assert np.abs(sc["sse"].cpu().numpy() - want[0]).max() <= er.score_bounds(U, Cm, X)[0].max()
    assert abs(sc["ref_total"] - n2) <= 131 * 2.0 ** -24 * n2
    assert sc["rows"] == m and torch.cat(sc["row_rmse"]).shape == (m,)


def test_dmd_forecast_fields_equal_expand_of_the_coefficients(KERN):
    from dmd_era5_amd import bopdmd as bop
    from dmd_era5_amd.forecast import DmdForecast, dmd_coefficients

    t = np.linspace(0, 6, 200)
    half = np.array([-0.1 + 2.0j, -0.5 + 5.0j, -0.02 + 0.7j])
    alpha = np.concatenate([half, half.conj()])
    rs = np.random.RandomState(2)
    mh = rs.standard_normal((3, 6)) + 1j * rs.standard_normal((3, 6))
    H = (np.exp(np.outer(t, alpha)) @ np.concatenate([mh, mh.conj()])).real
    res = bop.optdmd(torch.from_numpy(H).to(torch.complex128).to(DEV), torch.from_numpy(t).to(DEV), 6, tol=1e-10, maxiter=60)
    Q = np.linalg.qr(rs.standard_normal((700, 6)))[0].astype(np.float32)
    mu = rs.standard_normal(700).astype(np.float32)
    blocks = [(0, 300), (300, 700)]
    f = DmdForecast([_t(Q[a:b].T) for a, b in blocks], res, means=[_t(mu[a:b]) for a, b in blocks])
    tt = torch.from_numpy(np.linspace(0, 8, 77)).to(DEV)                      # past the window as well
    fields = f.fields(tt)
    C, imag = dmd_coefficients(res, tt)
    assert imag < 1e-6
    for (a, b), F in zip(blocks, fields):
        assert torch.equal(F, KERN.expand(_t(Q[a:b].T), C, _t(mu[a:b])))
    truth = (np.exp(np.outer(tt.cpu().numpy(), alpha)) @ np.concatenate([mh, mh.conj()])).real @ Q.T.astype(np.float64) + mu
    got = torch.cat(fields, dim=1).cpu().numpy()
    assert np.abs(got - truth).max() < 1e-4 * np.abs(truth).max()
    sc = f.score([_t(truth[:, a:b].astype(np.float32)) for a, b in blocks], tt)
    assert sc["rel_error_total"] < 1e-4


@pytest.mark.parametrize("d,scale", [(2, True), (1, True)])
def test_reconstruct_from_svd_results_through_main(svd_base_config, project_root, d, scale):
    from dmd_era5_amd import io_netcdf
    from dmd_era5_amd.config_parser import config_parser
    from dmd_era5_amd.create_mock_data import add_download_attributes, create_mock_era5
    from dmd_era5_amd.era5_svd import main, reconstruct_from_svd_results

    nt = 13 - d + 1
    cfg = dict(svd_base_config, start_datetime="2019-01-01T00", end_datetime="2019-01-01T12", variables="temperature",
               levels="1000,850", svd_type="standard", mean_center=True, scale=scale, delay_embedding=d,
               n_components=nt, save_data_matrix=True, svd_seed=0)
    p = config_parser(cfg, "era5-svd")
    ds = add_download_attributes(create_mock_era5(cfg["start_datetime"], cfg["end_datetime"], p["variables"], p["levels"],
                                                  seed=3, dtype=np.float32), p)
    io_netcdf.to_netcdf(ds, p["era5_slice_path"])
    res, _, _ = main(cfg, write_to_netcdf=False)
    Xv = np.asarray(res["X"].values)
    R = reconstruct_from_svd_results(res, destandardize=False)
    assert R.values.dtype == Xv.dtype and R.values.shape == Xv.shape and R.dims == res["X"].dims
    assert np.abs(R.values - Xv).max() <= 2e-4 * np.abs(Xv).max()
    R = reconstruct_from_svd_results(res)
    want = Xv.astype(np.float64)
    if "X_std" in res.data_vars:
        want = want * np.asarray(res["X_std"].values)[:, None]
    if "X_mean" in res.data_vars:
        want = want + np.asarray(res["X_mean"].values)[:, None]
    assert ("X_mean" in res.data_vars) == (d > 1)
    assert np.abs(R.values - want).max() <= 2e-4 * np.abs(want).max()


def test_expand_blocks_refuses_what_does_not_fit_and_states_the_bytes(KERN, monkeypatch):
    from dmd_era5_amd.forecast import expand_blocks, iter_fields

    Ub = [torch.ones((3, 1000), device=DEV), torch.ones((3, 500), device=DEV)]
    Ct = torch.ones((40, 3), device=DEV)
    need = 4 * 40 * 1500
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (need - 1, 1 << 40))
    monkeypatch.setattr(torch.cuda, "memory_reserved", lambda *a, **k: 0)
    monkeypatch.setattr(torch.cuda, "memory_allocated", lambda *a, **k: 0)
    with pytest.raises(MemoryError, match=str(need)):
        expand_blocks(Ub, Ct)
    # cached-but-unused allocator memory counts as free
    monkeypatch.setattr(torch.cuda, "memory_reserved", lambda *a, **k: 10)
    monkeypatch.setattr(torch.cuda, "memory_allocated", lambda *a, **k: 9)
    assert [tuple(b.shape) for b in expand_blocks(Ub, Ct)] == [(40, 1000), (40, 500)]
    # buffers of the caller are not counted; time chunks fit
    monkeypatch.setattr(torch.cuda, "memory_reserved", lambda *a, **k: 0)
    out = [torch.empty((40, 1000), device=DEV), torch.empty((40, 500), device=DEV)]
    assert bool((expand_blocks(Ub, Ct, out=out)[1] == 3).all())
    assert sum(t1 - t0 for t0, t1, _ in iter_fields(Ub, Ct, chunk=20)) == 40


def test_reconstruct_regenerates_the_matrix_a_result_file_left_out(svd_base_config, project_root):
    """save_data_matrix = False: the file holds no X; the Dataset retrieve_svd_results loads gives it back."""
    from dmd_era5_amd import io_netcdf
    from dmd_era5_amd.config_parser import config_parser
    from dmd_era5_amd.create_mock_data import add_download_attributes, create_mock_era5
    from dmd_era5_amd.era5_svd import main, reconstruct_from_svd_results, retrieve_svd_results

    cfg = dict(svd_base_config, start_datetime="2019-01-01T00", end_datetime="2019-01-01T12", variables="temperature",
               levels="1000,850", svd_type="standard", mean_center=True, scale=True, delay_embedding=2,
               n_components=12, save_data_matrix=True, svd_seed=0)
    p = config_parser(cfg, "era5-svd")
    ds = add_download_attributes(create_mock_era5(cfg["start_datetime"], cfg["end_datetime"], p["variables"], p["levels"],
                                                  seed=3, dtype=np.float32), p)
    io_netcdf.to_netcdf(ds, p["era5_slice_path"])
    with_x, _, _ = main(cfg, write_to_netcdf=False)
    Xv = np.asarray(with_x["X"].values)
    cfg2 = dict(cfg, save_data_matrix=False)
    main(cfg2, write_to_netcdf=True)
    loaded, _ = retrieve_svd_results(config_parser(cfg2, "era5-svd"))
    assert loaded is not None and "X" not in loaded.data_vars
    R = reconstruct_from_svd_results(loaded, destandardize=False)
    assert R.values.shape == Xv.shape and R.values.dtype == Xv.dtype
    assert np.abs(R.values - Xv).max() <= 2e-4 * np.abs(Xv).max()
