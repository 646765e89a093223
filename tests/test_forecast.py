"""CPU tests of dmd_era5_amd.forecast and era5_svd.reconstruct_from_svd_results: the host layer above
K12, through the torch fallback (a provider without ``expand``) and a numpy-style double of the two
kernels (tests/expand_ref.ExpandDouble), plus the argument checks of the C entry points."""
import itertools
import os
import socket
import sys
from datetime import timedelta

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from expand_ref import ExpandDouble
from kernel_double import CpuKernelDouble

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = 2.0 ** -24


class DoubleWithExpand(ExpandDouble, CpuKernelDouble):
    name = "cpu-double+expand"


PROVIDERS = [CpuKernelDouble, DoubleWithExpand]        # torch fallback / kernel double


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


# ---------------------------------------------------------------- coefficients
def test_svd_coefficients():
    from dmd_era5_amd.forecast import svd_coefficients

    rs = np.random.RandomState(0)
    s, Vh = np.sort(rs.rand(5))[::-1].copy(), rs.standard_normal((5, 17))
    C = svd_coefficients(_t(s, torch.float64), _t(Vh, torch.float64))
    assert C.dtype == torch.float32 and C.shape == (17, 5) and C.is_contiguous()
    assert np.array_equal(C.numpy(), (s[:, None] * Vh).T.astype(np.float32))
    cols = [3, 0, 16]
    assert np.array_equal(svd_coefficients(_t(s, torch.float64), _t(Vh, torch.float64), cols).numpy(),
                          (s[:, None] * Vh[:, cols]).T.astype(np.float32))


def _planted_real(t, n_s=8, seed=0):
    """A REAL signal of damped oscillations: conjugate pairs of eigenvalues with conjugate modes."""
    rs = np.random.RandomState(seed)
    half = np.array([-0.1 + 2.0j, -0.5 + 5.0j, -0.02 + 0.7j])
    alpha = np.concatenate([half, half.conj()])
    mh = rs.standard_normal((3, n_s)) + 1j * rs.standard_normal((3, n_s))
    modes = np.concatenate([mh, mh.conj()])
    H = np.exp(np.outer(t, alpha)) @ modes
    assert np.abs(H.imag).max() < 1e-12
    return H.real, alpha, modes


def test_dmd_coefficients_inside_and_beyond_the_window():
    from dmd_era5_amd import bopdmd as bop
    from dmd_era5_amd.forecast import dmd_coefficients

    t = np.linspace(0, 6, 300)
    H, alpha, modes = _planted_real(t)
    res = bop.optdmd(torch.from_numpy(H).to(torch.complex128), torch.from_numpy(t), 6, tol=1e-11, maxiter=60)
    assert res.rel_error < 1e-8
    t2 = np.concatenate([t[::7], np.linspace(6.0, 9.0, 40)])           # inside and past the training window
    C, imag = dmd_coefficients(res, torch.from_numpy(t2))
    a, b, W = res.eigs.numpy(), res.amplitudes.numpy(), res.modes.numpy()
    Z = (np.exp(np.outer(t2, a)) * b) @ W.T                              # direct complex128 evaluation
    assert C.dtype == torch.float32 and C.shape == (len(t2), H.shape[1])
    assert np.array_equal(C.numpy(), Z.real.astype(np.float32)) or \
        np.abs(C.numpy() - Z.real).max() <= 4 * EPS32 * np.abs(Z.real).max()
    assert imag == pytest.approx(np.abs(Z.imag).max() / np.abs(Z.real).max(), rel=1e-6, abs=1e-15)
    assert imag < 1e-6                                                   # a real signal: a (nearly) real model
    truth = (np.exp(np.outer(t2, alpha)) @ modes).real
    assert np.abs(C.numpy() - truth).max() < 1e-5 * np.abs(truth).max()
    # a model that is NOT real says so
    res.modes = res.modes * torch.tensor(1j, dtype=res.modes.dtype)
    assert dmd_coefficients(res, torch.from_numpy(t2))[1] > 0.1


# ---------------------------------------------------------------- score identities
@pytest.mark.parametrize("provider", PROVIDERS)
def test_score_identity_with_numpy_svd(provider):
    """sse(rank r) = ||X||^2 - sum_{i <= r} s_i^2, per snapshot ||x_t||^2 - ||S_r v_t||^2, 0 at full rank."""
    from dmd_era5_amd.forecast import score_blocks, svd_coefficients

    rs = np.random.RandomState(1)
    X = rs.standard_normal((60, 24)).astype(np.float32)
    U, s, Vh = np.linalg.svd(X.astype(np.float64), full_matrices=False)
    Xt = _t(X.T)
    blocks = [(0, 28), (28, 60)]
    n2 = float((X.astype(np.float64) ** 2).sum())
    tol = 64 * EPS32 * n2                                               # U, C and X rounded to fp32 (k <= 24 terms)
    for r in (1, 5, 24):
        Ub = [_t(U[a:b, :r].T) for a, b in blocks]
        Ct = svd_coefficients(_t(s[:r], torch.float64), _t(Vh[:r], torch.float64))
        res = score_blocks(Ub, Ct, [Xt[:, a:b] for a, b in blocks], kern=provider(), want_rows=True)
        assert res["rows"] == 60
        assert abs(res["sse_total"] - (n2 - (s[:r] ** 2).sum())) <= tol
        assert abs(res["ref_total"] - n2) <= tol
        want_t = (X.astype(np.float64) ** 2).sum(axis=0) - ((s[:r, None] * Vh[:r]) ** 2).sum(axis=0)
        assert np.abs(res["sse"].numpy() - want_t).max() <= tol / 4
        assert np.allclose(res["rmse"].numpy(), np.sqrt(np.maximum(res["sse"].numpy(), 0) / 60))
        row = torch.cat(res["row_rmse"]).numpy()
        E = X - (U[:, :r] * s[:r]) @ Vh[:r]
        assert np.abs(row ** 2 * 24 - (E ** 2).sum(axis=1)).max() <= tol / 4
    assert res["rel_error_total"] < 1e-6 and float(res["rel_error"].max()) < 1e-5     # full rank


@pytest.mark.parametrize("provider", PROVIDERS)
def test_expand_blocks_means_stds_delay_and_blocks(provider):
    from dmd_era5_amd.forecast import expand_blocks, iter_fields, score_blocks

    rs = np.random.RandomState(2)
    d, k, T = 2, 4, 9
    rows = [5, 8, 3]
    Ub = [rs.standard_normal((k, d * mb)).astype(np.float32) for mb in rows]
    Ct = rs.standard_normal((T, k)).astype(np.float32)
    mu = [rs.standard_normal(mb).astype(np.float32) for mb in rows]
    sd = [(0.5 + rs.rand(mb)).astype(np.float32) for mb in rows]
    args = ([_t(u) for u in Ub], _t(Ct), [_t(v) for v in mu], [_t(v) for v in sd])
    K = provider()
    for j in (0, 1, None):
        got = expand_blocks(*args, delay_block=j, delay=d, kern=K)
        for b, mb in enumerate(rows):
            Uj = Ub[b] if j is None else Ub[b][:, j * mb:(j + 1) * mb]
            reps = d if j is None else 1
            want = np.tile(mu[b], reps) + np.tile(sd[b], reps) * (Ct.astype(np.float64) @ Uj.astype(np.float64))
            assert got[b].shape == want.shape and got[b].dtype == torch.float32
            assert np.abs(got[b].numpy() - want).max() <= (k + 2) * EPS32 * 20
    plain = expand_blocks(args[0], args[1], kern=K)                      # no means, no delay split
    assert np.abs(plain[1].numpy() - Ct.astype(np.float64) @ Ub[1].astype(np.float64)).max() <= (k + 2) * EPS32 * 20
    # time chunks give the same fields
    whole = expand_blocks(*args, delay_block=0, delay=d, kern=K)
    seen = 0
    for t0, t1, blk in iter_fields(*args, delay_block=0, delay=d, chunk=4, kern=K):
        for b in range(len(rows)):
            assert torch.equal(blk[b], whole[b][t0:t1])
        seen += t1 - t0
    assert seen == T
    with pytest.raises(ValueError):
        expand_blocks(*args, delay_block=2, delay=d, kern=K)
    # a delay-embedded score: snapshots (T + d - 1, mb), the embedded view against all d * mb rows
    Xb = [_t(rs.standard_normal((T + d - 1, mb)).astype(np.float32)) for mb in rows]
    res = score_blocks(args[0], args[1], Xb, args[2], args[3], delay=d, kern=K)
    sse = np.zeros(T)
    for b, mb in enumerate(rows):
        E = np.concatenate([Xb[b].numpy()[kd:kd + T] for kd in range(d)], axis=1).astype(np.float64)
        P = np.tile(mu[b], d) + np.tile(sd[b], d) * (Ct.astype(np.float64) @ Ub[b].astype(np.float64))
        sse += ((E - P) ** 2).sum(axis=1)
    assert np.allclose(res["sse"].numpy(), sse, rtol=1e-5) and res["rows"] == d * sum(rows)


def test_dmd_forecast_bundle():
    from dmd_era5_amd import bopdmd as bop
    from dmd_era5_amd.forecast import DmdForecast, dmd_coefficients, expand_blocks

    t = np.linspace(0, 6, 200)
    H, _, _ = _planted_real(t, n_s=6)
    rs = np.random.RandomState(3)
    Q = np.linalg.qr(rs.standard_normal((40, 6)))[0].astype(np.float32)          # U: 40 rows, 6 columns
    mu = rs.standard_normal(40).astype(np.float32)
    X = (H @ Q.T.astype(np.float64) + mu).astype(np.float32)                      # (time, space)
    res = bop.optdmd(torch.from_numpy(H).to(torch.complex128), torch.from_numpy(t), 6, tol=1e-10, maxiter=60)
    blocks = [(0, 16), (16, 40)]
    K = DoubleWithExpand()
    f = DmdForecast([_t(Q[a:b].T) for a, b in blocks], res, means=[_t(mu[a:b]) for a, b in blocks], kern=K)
    fields = f.fields(torch.from_numpy(t))
    C, _ = dmd_coefficients(res, torch.from_numpy(t))
    want = expand_blocks(f.Ublocks, C, f.means, None, kern=K)
    assert all(torch.equal(a, b) for a, b in zip(fields, want))
    assert np.abs(torch.cat(fields, dim=1).numpy() - X).max() < 1e-4 * np.abs(X).max()
    sc = f.score([_t(X[:, a:b]) for a, b in blocks], torch.from_numpy(t))
    assert sc["rel_error_total"] < 1e-4 and sc["imag_ratio"] < 1e-6
    with pytest.raises(ValueError):
        f.reconstruct_svd()


# ---------------------------------------------------------------- row shards over gloo
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _shard_problem():
    rs = np.random.RandomState(4)
    rows = [7, 4, 9, 5, 6]                       # rank 0 holds blocks 0 .. 2, rank 1 blocks 3, 4 (uneven)
    k, T = 3, 11
    Ub = [rs.standard_normal((k, mb)).astype(np.float32) for mb in rows]
    Xb = [rs.standard_normal((T, mb)).astype(np.float32) for mb in rows]
    Ct = rs.standard_normal((T, k)).astype(np.float32)
    return Ub, Xb, Ct


def _counting(base):
    class Counting(base):
        calls = 0

        def allreduce_sum_(self, t, tag="allreduce"):
            type(self).calls += 1
            return super().allreduce_sum_(t, tag=tag)

    return Counting


def _shard_worker(rank, world, port, q):
    for p in (os.path.dirname(os.path.abspath(__file__)), ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist

    from dmd_era5_amd import svd as dsvd
    from dmd_era5_amd.forecast import score_blocks

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        Ub, Xb, Ct = _shard_problem()
        mine = [0, 1, 2] if rank == 0 else [3, 4]
        comm = _counting(dsvd.TorchDistComm)()
        res = score_blocks([_t(Ub[b]) for b in mine], _t(Ct), [_t(Xb[b]) for b in mine], comm=comm,
                           kern=DoubleWithExpand())
        q.put((rank, type(comm).calls, res["sse"].numpy(), res["ref"].numpy(), res["rows"], res["rmse_total"]))
    finally:
        dist.destroy_process_group()


def test_row_shards_sum_with_one_collective():
    from dmd_era5_amd import svd as dsvd
    from dmd_era5_amd.forecast import score_blocks

    Ub, Xb, Ct = _shard_problem()
    single_comm = _counting(dsvd.Comm)()
    one = score_blocks([_t(u) for u in Ub], _t(Ct), [_t(x) for x in Xb], comm=single_comm, kern=DoubleWithExpand())
    assert type(single_comm).calls == 1
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_shard_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=180) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, calls, sse, ref, rows, rmse in got:
        assert calls == 1, "one collective per call, whatever the number of local blocks"
        assert rows == one["rows"] == 31
        assert np.allclose(sse, one["sse"].numpy(), rtol=1e-13) and np.allclose(ref, one["ref"].numpy(), rtol=1e-13)
        assert rmse == pytest.approx(one["rmse_total"], rel=1e-13)


# ---------------------------------------------------------------- the result file's data matrix
@pytest.mark.parametrize("d,center,scale", [(1, False, False), (1, True, True), (2, False, False), (2, True, False),
                                            (2, True, True)])
def test_reconstruct_from_svd_results_returns_the_data_matrix(d, center, scale):
    from dmd_era5_amd import era5_svd
    from dmd_era5_amd import svd as dsvd
    from dmd_era5_amd.create_mock_data import create_mock_era5

    ds = create_mock_era5("2019-01-01", "2019-01-01T11", ["temperature"], [1000, 850], seed=3, dtype=np.float32)
    nt = 12 - d + 1
    cfg = {"delay_embedding": d, "mean_center": center, "scale": scale, "levels": [1000, 850],
           "delta_time": timedelta(hours=1), "n_components": nt, "svd_type": "standard", "save_data_matrix": True,
           "svd_seed": 0}
    K = DoubleWithExpand()
    U, s, V, coords, X, Xm, Xs = era5_svd._device_pipeline(ds, cfg, dsvd.Comm(), kern=K, device=torch.device("cpu"))
    out = era5_svd.combine_svd_results(U, s, V, coords, X=X, X_mean=Xm, X_std=Xs)      # what main() returns
    assert ("X_mean" in out.data_vars) == (center and d > 1)                           # the reference's d = 1 quirk
    Xv = np.asarray(out["X"].values)
    tol = 2e-4 * np.abs(Xv).max()
    for kern in (K, CpuKernelDouble()):
        R = era5_svd.reconstruct_from_svd_results(out, destandardize=False, kern=kern)
        assert R.dims == out["X"].dims and R.values.dtype == Xv.dtype and R.values.shape == Xv.shape
        assert np.array_equal(R.coords["time"].values, out["X"].coords["time"].values)
        assert np.array_equal(R.coords["space"].values, out["X"].coords["space"].values)
        assert np.abs(R.values - Xv).max() <= tol
    R = era5_svd.reconstruct_from_svd_results(out, kern=K)
    want = Xv.astype(np.float64)
    if "X_std" in out.data_vars:
        want = want * np.asarray(out["X_std"].values)[:, None]
    if "X_mean" in out.data_vars:
        want = want + np.asarray(out["X_mean"].values)[:, None]
    assert np.abs(R.values - want).max() <= 2e-4 * np.abs(want).max()
    # fewer components, some snapshots: the truncated product, labelled with those times
    R2 = era5_svd.reconstruct_from_svd_results(out, n_components=3, times=[4, 1], destandardize=False, kern=K)
    want2 = (np.asarray(U, dtype=np.float64)[:, :3] * np.asarray(s, dtype=np.float64)[:3]) @ np.asarray(V, dtype=np.float64)[:3][:, [4, 1]]
    assert R2.values.shape == (Xv.shape[0], 2) and np.abs(R2.values - want2).max() <= 1e-5 * np.abs(want2).max()
    assert np.array_equal(R2.coords["time"].values, np.asarray(out["X"].coords["time"].values)[[4, 1]])
    with pytest.raises(ValueError):
        era5_svd.reconstruct_from_svd_results(out, n_components=nt + 1, kern=K)


def test_reconstruct_from_main_and_from_a_result_file_without_x(svd_base_config, project_root, monkeypatch):
    """main() itself (its device pipeline handed the kernel double), with save_data_matrix = False and a
    written result file: the Dataset retrieve_svd_results loads has no X, and the function gives it back."""
    from dmd_era5_amd import era5_svd, io_netcdf
    from dmd_era5_amd.config_parser import config_parser
    from dmd_era5_amd.create_mock_data import add_download_attributes, create_mock_era5

    K = DoubleWithExpand()
    pipeline = era5_svd._device_pipeline
    monkeypatch.setattr(era5_svd, "_device_pipeline",
                        lambda ds, cfg, comm: pipeline(ds, cfg, comm, kern=K, device=torch.device("cpu")))
    cfg = dict(svd_base_config, start_datetime="2019-01-01T00", end_datetime="2019-01-01T12", variables="temperature",
               levels="1000,850", svd_type="standard", mean_center=True, scale=True, delay_embedding=2,
               n_components=12, save_data_matrix=True, svd_seed=0)
    p = config_parser(cfg, "era5-svd")
    ds = add_download_attributes(create_mock_era5(cfg["start_datetime"], cfg["end_datetime"], p["variables"], p["levels"],
                                                  seed=3, dtype=np.float32), p)
    io_netcdf.to_netcdf(ds, p["era5_slice_path"])
    with_x, _, _ = era5_svd.main(cfg, write_to_netcdf=False)
    Xv = np.asarray(with_x["X"].values)
    R = era5_svd.reconstruct_from_svd_results(with_x, destandardize=False, kern=K)
    assert np.abs(R.values - Xv).max() <= 2e-4 * np.abs(Xv).max()
    cfg2 = dict(cfg, save_data_matrix=False)
    era5_svd.main(cfg2, write_to_netcdf=True)
    loaded, _ = era5_svd.retrieve_svd_results(config_parser(cfg2, "era5-svd"))
    assert loaded is not None and "X" not in loaded.data_vars and "X_mean" in loaded.data_vars
    R = era5_svd.reconstruct_from_svd_results(loaded, destandardize=False, kern=K)
    assert R.values.shape == Xv.shape and R.values.dtype == Xv.dtype
    assert np.abs(R.values - Xv).max() <= 2e-4 * np.abs(Xv).max()
    R = era5_svd.reconstruct_from_svd_results(loaded, kern=K)
    want = Xv * np.asarray(loaded["X_std"].values)[:, None] + np.asarray(loaded["X_mean"].values)[:, None]
    assert np.abs(R.values - want).max() <= 2e-4 * np.abs(want).max()


def test_score_blocks_refuses_lists_of_different_length():
    from dmd_era5_amd.forecast import score_blocks

    U = [torch.ones((2, 5)), torch.ones((2, 4))]
    with pytest.raises(ValueError):
        score_blocks(U, torch.ones((3, 2)), [torch.ones((3, 5))], kern=DoubleWithExpand())


def test_alias_package_exports_the_new_names():
    import dmd_era5.era5_svd as alias
    import dmd_era5.forecast as alias_fc
    from dmd_era5_amd import era5_svd, forecast

    assert alias.reconstruct_from_svd_results is era5_svd.reconstruct_from_svd_results
    assert "reconstruct_from_svd_results" in alias.__all__
    for name in forecast.__all__:
        assert getattr(alias_fc, name) is getattr(forecast, name)


# ---------------------------------------------------------------- C ABI without a GPU
@pytest.fixture(scope="module")
def lib():
    from dmd_era5_amd import _lib

    return _lib.load()


def test_expand_argument_errors_without_a_gpu(lib):
    inv, wsp = -1000, -1001
    kmax = lib.dmdx_expand_max_k()
    assert kmax >= 256
    p = 4096                                     # a non-null address: every call is refused before it is used
    ok = dict(U=p, m=10, k=3, ldu=10, C=p, ldc=3, T=5, mu=None, sigma=None, out=p, ldo=10)

    def expand(**o):
        a = {**ok, **o}
        return lib.dmdx_expand_f32(a["U"], a["m"], a["k"], a["ldu"], a["C"], a["ldc"], a["T"], a["mu"], a["sigma"], a["out"],
                                   a["ldo"], None)

    def score(ws=p, wsb=1 << 30, sse=p, **o):
        a = {**ok, **o}
        return lib.dmdx_expand_score_f32(a["U"], a["m"], a["k"], a["ldu"], a["C"], a["ldc"], a["T"], a["mu"], a["sigma"],
                                         a["out"], a["ldo"], sse, None, None, 0, ws, wsb, None)

    for f in (expand, score):
        for o in (dict(U=None), dict(C=None), dict(out=None), dict(k=0), dict(k=kmax + 1), dict(ldu=9), dict(ldc=2),
                  dict(m=0), dict(T=0), dict(m=2 ** 31, ldu=2 ** 31)):
            assert f(**o) == inv, (f.__name__, o)
            assert lib.dmdx_last_error()
    assert expand(ldo=9) == inv
    assert b"null" in (expand(U=None), lib.dmdx_last_error())[1]
    assert score(sse=None) == inv
    need = lib.dmdx_expand_score_workspace_bytes(10, 3, 5)
    assert score(wsb=need - 1) == wsp and score(ws=None) == wsp
    assert b"workspace" in lib.dmdx_last_error()


def test_expand_workspace_planner_on_degenerate_shapes(lib):
    for m, k, T in itertools.product([1, 3, 63], repeat=3):
        assert lib.dmdx_expand_score_workspace_bytes(m, k, T) > 0
    # one row block x T x 2 fp32 + the row partials: linear in both, far below X itself
    big = lib.dmdx_expand_score_workspace_bytes(129780, 50, 8760)
    assert 0 < big < 129780 * 8760 * 4 // 20
