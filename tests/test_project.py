"""CPU tests of the host layer above K13: forecast.project_blocks, DmdForecast.project / restart and
era5_svd.project_onto_svd_results, through the torch fallback (a provider without ``project``) and a numpy
double of the kernel (tests/project_ref.ProjectDouble), plus the argument checks of the C entry point."""
import itertools
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import project_ref as pr
from expand_ref import ExpandDouble
from kernel_double import CpuKernelDouble

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class DoubleWithProject(pr.ProjectDouble, ExpandDouble, CpuKernelDouble):
    name = "cpu-double+project"


PROVIDERS = [CpuKernelDouble, DoubleWithProject]        # torch fallback / kernel double


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


# ---------------------------------------------------------------- project_blocks
def _block_problem(seed=2, d=2, k=4, T=9, rows=(5, 8, 3)):
    rs = np.random.RandomState(seed)
    Ub = [rs.standard_normal((k, d * mb)).astype(np.float32) for mb in rows]
    Xb = [(280.0 + 10.0 * rs.standard_normal((T + d - 1, mb))).astype(np.float32) for mb in rows]
    mu = [(280.0 + rs.standard_normal(mb)).astype(np.float32) for mb in rows]
    sd = [(5.0 + 10.0 * rs.rand(mb)).astype(np.float32) for mb in rows]
    return Ub, Xb, mu, sd


def _embedded(X, d, T):
    """(T, d * mb) fp64 of a (T + d - 1, mb) block."""
    return np.concatenate([X[j:j + T] for j in range(d)], axis=1).astype(np.float64)


@pytest.mark.parametrize("provider", PROVIDERS)
def test_project_blocks_means_stds_delay_and_blocks(provider):
    from dmd_era5_amd.forecast import project_blocks

    d, k, T, rows = 2, 4, 9, (5, 8, 3)
    Ub, Xb, mu, sd = _block_problem(d=d, k=k, T=T, rows=rows)
    K = provider()
    for use_mu, use_sd in itertools.product((False, True), repeat=2):
        C, e = np.zeros((T, k)), np.zeros(T)
        for b, mb in enumerate(rows):
            Z = _embedded(Xb[b], d, T)
            if use_mu:
                Z = Z - np.tile(mu[b], d)
            if use_sd:
                Z = Z / np.tile(sd[b], d)
            C += Z @ Ub[b].astype(np.float64).T
            e += (Z * Z).sum(axis=1)
        res = project_blocks([_t(u) for u in Ub], iter([_t(x) for x in Xb]), [_t(v) for v in mu] if use_mu else None,
                             [_t(v) for v in sd] if use_sd else None, delay=d, kern=K)
        assert res["Ct"].shape == (T, k) and res["Ct"].dtype == torch.float64 and res["energy"].shape == (T,)
        assert np.allclose(res["Ct"].numpy(), C, rtol=1e-12, atol=1e-12 * np.abs(C).max())
        assert np.allclose(res["energy"].numpy(), e, rtol=1e-12)
        assert np.allclose(res["captured"].numpy(), (C * C).sum(axis=1) / e, rtol=1e-12)
        assert res["captured_total"] == pytest.approx((C * C).sum() / e.sum(), rel=1e-12)
        assert res["energy_total"] == pytest.approx(e.sum(), rel=1e-12)
        assert res["rows"] == d * sum(rows)
    # an orthonormal basis captures at most everything, and all of what lies in its span
    rs = np.random.RandomState(5)
    Q = np.linalg.qr(rs.standard_normal((30, 6)))[0]
    inside = (Q @ rs.standard_normal((6, 7))).T
    res = project_blocks([_t(Q[:12].T), _t(Q[12:].T)], [_t(inside[:, :12]), _t(inside[:, 12:])], kern=K)
    assert np.abs(res["captured"].numpy() - 1.0).max() < 1e-5 and abs(res["captured_total"] - 1.0) < 1e-5


@pytest.mark.parametrize("provider", PROVIDERS)
def test_project_blocks_refusals(provider):
    from dmd_era5_amd.forecast import project_blocks

    Ub, Xb, mu, sd = _block_problem()
    K = provider()
    sd[1][2] = 0.0
    sd[2][0] = 0.0

    class Tripwire(provider):
        def project(self, *a, **k):
            raise AssertionError("launched")

        def gemm_tn(self, *a, **k):
            raise AssertionError("launched")

    with pytest.raises(ValueError, match="2 entries"):      # before any launch
        project_blocks([_t(u) for u in Ub], [_t(x) for x in Xb], [_t(v) for v in mu], [_t(v) for v in sd], delay=2,
                       kern=Tripwire())
    with pytest.raises(ValueError):                         # lists of different length
        project_blocks([_t(u) for u in Ub], [_t(x) for x in Xb[:2]], delay=2, kern=K)
    with pytest.raises(ValueError):                         # a block of another shape
        project_blocks([_t(u) for u in Ub], [_t(Xb[0]), _t(Xb[1][:, :7]), _t(Xb[2])], delay=2, kern=K)
    with pytest.raises(ValueError):                         # another number of snapshots
        project_blocks([_t(u) for u in Ub], [_t(Xb[0]), _t(Xb[1][:-1]), _t(Xb[2])], delay=2, kern=K)
    with pytest.raises(ValueError):                         # nothing to learn the sizes from
        project_blocks([], [], kern=K)
    res = project_blocks([], [], kern=K, shape=(4, 3))
    assert res["Ct"].shape == (4, 3) and res["rows"] == 0 and not bool(res["Ct"].any())


# ---------------------------------------------------------------- row shards over gloo
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _counting(base):
    class Counting(base):
        calls = 0
        tags = []

        def allreduce_sum_(self, t, tag="allreduce"):
            type(self).calls += 1
            type(self).tags.append(tag)
            return super().allreduce_sum_(t, tag=tag)

    return Counting


SPLITS = {"uneven": ([0, 1, 2], [3, 4]), "empty": ([0, 1, 2, 3, 4], [])}


def _shard_problem():
    return _block_problem(seed=4, d=1, k=3, T=11, rows=(7, 4, 9, 5, 6))


def _shard_worker(rank, world, port, q):
    for p in (os.path.dirname(os.path.abspath(__file__)), ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist

    from dmd_era5_amd import svd as dsvd
    from dmd_era5_amd.forecast import project_blocks

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        Ub, Xb, mu, sd = _shard_problem()
        for name, split in SPLITS.items():
            mine = split[rank]
            comm = _counting(dsvd.TorchDistComm)()
            res = project_blocks([_t(Ub[b]) for b in mine], [_t(Xb[b]) for b in mine], [_t(mu[b]) for b in mine],
                                 [_t(sd[b]) for b in mine], comm=comm, kern=DoubleWithProject(), shape=(11, 3))
            q.put((name, rank, type(comm).calls, list(type(comm).tags), res["Ct"].numpy(), res["energy"].numpy(),
                   res["rows"], res["captured_total"]))
    finally:
        dist.destroy_process_group()


def test_row_shards_sum_with_one_collective():
    from dmd_era5_amd import svd as dsvd
    from dmd_era5_amd.forecast import project_blocks

    Ub, Xb, mu, sd = _shard_problem()
    single = _counting(dsvd.Comm)()
    one = project_blocks([_t(u) for u in Ub], [_t(x) for x in Xb], [_t(v) for v in mu], [_t(v) for v in sd], comm=single,
                         kern=DoubleWithProject())
    assert type(single).calls == 1 and type(single).tags == ["project_allreduce"]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_shard_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=180) for _ in range(2 * len(SPLITS))]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted((g[0], g[1]) for g in got) == sorted((n, r) for n in SPLITS for r in range(2))
    for name, rank, calls, tags, Ct, energy, rows, cap in got:
        assert calls == 1 and tags == ["project_allreduce"], "one collective per call, whatever the number of local blocks"
        assert rows == one["rows"] == 31
        assert np.allclose(Ct, one["Ct"].numpy(), rtol=1e-12, atol=1e-12 * float(one["Ct"].abs().max()))
        assert np.allclose(energy, one["energy"].numpy(), rtol=1e-13)
        assert cap == pytest.approx(one["captured_total"], rel=1e-12)


# ---------------------------------------------------------------- restart
def _planted(k, r, seed, pairs=True):
    """Eigenvalues, unit-norm modes (k, r) and complex amplitudes of a model Phi diag(b) modes^T."""
    rs = np.random.RandomState(seed)
    if pairs:
        half = np.array([-0.1 + 2.0j, -0.5 + 5.0j, -0.02 + 0.7j])[:r // 2]
        alpha = np.concatenate([half, half.conj()])
        mh = rs.standard_normal((k, r // 2)) + 1j * rs.standard_normal((k, r // 2))
        W = np.concatenate([mh, mh.conj()], axis=1)
        bh = rs.standard_normal(r // 2) + 1j * rs.standard_normal(r // 2)
        b = np.concatenate([bh, bh.conj()])
    else:
        alpha = -0.3 * rs.rand(r) + 1j * (0.5 + 4.0 * rs.rand(r))
        W = rs.standard_normal((k, r)) + 1j * rs.standard_normal((k, r))
        b = rs.standard_normal(r) + 1j * rs.standard_normal(r)
    W = W / np.linalg.norm(W, axis=0)
    return alpha, W, b


def _bundle(alpha, W, amp, Q, mu=None, sd=None, kern=None, blocks=((0, 16), (16, 40))):
    from dmd_era5_amd.bopdmd import OptDMDResult
    from dmd_era5_amd.forecast import DmdForecast

    res = OptDMDResult(eigs=torch.from_numpy(alpha), modes=torch.from_numpy(W), amplitudes=torch.from_numpy(amp),
                       rel_error=0.0, n_iter=3, converged=True, info={"kept": 1})
    return DmdForecast([_t(Q[a:b].T) for a, b in blocks], res, means=None if mu is None else [_t(mu[a:b]) for a, b in blocks],
                       stds=None if sd is None else [_t(sd[a:b]) for a, b in blocks], kern=kern)


@pytest.mark.parametrize("tname", ["uniform", "uneven", "single"])
def test_restart_is_exact_on_a_planted_model(tname):
    """C = Phi(t) diag(b) modes^T handed over as it is (U = the identity in fp64 through the kernel double, so that
    nothing but the r x r solve is between the planted b and the result): 1e-10 in complex128."""
    k, r = 8, 6
    alpha, W, b = _planted(k, r, seed=7, pairs=False)
    t = {"uniform": np.linspace(10.0, 12.0, 25), "uneven": np.sort(10.0 + 3.0 * np.random.RandomState(8).rand(17)),
         "single": np.array([11.5])}[tname]                                     # T = 1: k = 8 >= r = 6
    C = (np.exp(np.outer(t, alpha)) * b) @ W.T                                   # complex (T, k)
    f = _bundle(alpha, W, np.ones(r), np.eye(k), kern=DoubleWithProject(), blocks=((0, 3), (3, 8)))
    # the snapshots are real; give the real part and compare with the fit of the real part's own minimiser below
    g = f.restart([torch.from_numpy(C.real[:, :3].copy()), torch.from_numpy(C.real[:, 3:].copy())], torch.from_numpy(t))
    assert g.result.info["restart_dropped"] == 0 and g.result.info["kept"] == 1
    assert g.result.info["restarted_at"] == (float(t[0]), float(t[-1])) and g.result.info["restart_window"] == len(t)
    assert g.Ublocks is f.Ublocks and torch.equal(g.result.eigs, f.result.eigs)
    amp, modes = g.result.amplitudes.numpy(), g.result.modes.numpy()
    assert amp.dtype == np.float64 and (amp >= 0).all()
    assert np.allclose(np.linalg.norm(modes, axis=0), 1.0, atol=1e-12)
    # the minimiser of || Phi diag(b) W^T - Re C ||_F by a dense least-squares solve of the (T k) x r system
    A = np.stack([np.outer(np.exp(alpha[j] * t), W[:, j]).reshape(-1) for j in range(r)], axis=1)
    bref = np.linalg.lstsq(A, C.real.reshape(-1).astype(np.complex128), rcond=None)[0]
    phase = modes[0] / W[0]
    assert np.abs(np.abs(phase) - 1.0).max() < 1e-12
    assert np.abs(amp * phase - bref).max() <= 1e-10 * np.abs(bref).max()
    fit = (np.exp(np.outer(t, alpha)) * bref) @ W.T
    assert g.result.rel_error == pytest.approx(np.linalg.norm(fit - C.real) / np.linalg.norm(C.real), abs=1e-10)
    # handed the COMPLEX coefficients' generator exactly: a conjugate-pair model is real and b comes back
    alpha, W, b = _planted(k, r, seed=9, pairs=True)
    C = (np.exp(np.outer(t, alpha)) * b) @ W.T
    assert np.abs(C.imag).max() < 1e-12
    f = _bundle(alpha, W, np.ones(r), np.eye(k), kern=DoubleWithProject(), blocks=((0, 3), (3, 8)))
    g = f.restart([torch.from_numpy(C.real[:, :3].copy()), torch.from_numpy(C.real[:, 3:].copy())], torch.from_numpy(t))
    got = g.result.amplitudes.numpy() * (g.result.modes.numpy()[0] / W[0])
    assert np.abs(got - b).max() <= 1e-10 * np.abs(b).max()
    assert g.result.rel_error < 1e-10 and g.result.info["captured"] == pytest.approx(1.0, abs=1e-12)


def test_restart_through_fields_means_and_stds():
    """Raw fields mu + sd * (Q c) of a new state, projected with the bundle's means and stds (fp32 inputs): the
    forecast continues the new state."""
    from dmd_era5_amd.forecast import dmd_coefficients

    k, r = 6, 6
    alpha, W, b = _planted(k, r, seed=11)
    rs = np.random.RandomState(12)
    Q = np.linalg.qr(rs.standard_normal((40, k)))[0].astype(np.float32)
    mu, sd = (280.0 + rs.standard_normal(40)).astype(np.float32), (5.0 + 10.0 * rs.rand(40)).astype(np.float32)
    t = np.linspace(20.0, 21.0, 12)
    t2 = np.linspace(21.0, 23.0, 9)
    truth = lambda tt: ((np.exp(np.outer(tt, alpha)) * b) @ W.T).real                      # noqa: E731
    X = (mu + sd * (truth(t) @ Q.T.astype(np.float64))).astype(np.float32)
    for K in (DoubleWithProject(), CpuKernelDouble()):
        f = _bundle(alpha, W, np.ones(r), Q, mu, sd, kern=K)
        g = f.restart([_t(X[:, :16]), _t(X[:, 16:])], t)
        assert g.means is f.means and g.stds is f.stds
        C2, imag = dmd_coefficients(g.result, torch.from_numpy(t2))
        scale = np.abs(truth(t2)).max()
        # X is rounded to fp32 near 300: 2^-24 * 340 / 5 = 4e-6 per standardised element, sqrt(40) of that per
        # coefficient (unit columns of Q): 2.6e-5; 20 x for the least-squares fit and the fp32 result
        assert np.abs(C2.numpy() - truth(t2)).max() <= 20 * 2.6e-5 * max(scale, 1.0)
        assert imag < 1e-4
        assert g.result.rel_error < 1e-4 and abs(g.result.info["captured"] - 1.0) < 1e-4
    # the thin projection method gives the same coefficients as the function
    from dmd_era5_amd.forecast import project_blocks

    p1 = f.project([_t(X[:, :16]), _t(X[:, 16:])])
    p2 = project_blocks(f.Ublocks, [_t(X[:, :16]), _t(X[:, 16:])], f.means, f.stds, kern=CpuKernelDouble())
    assert torch.equal(p1["Ct"], p2["Ct"]) and torch.equal(p1["energy"], p2["energy"])


def test_restart_refuses_an_underdetermined_window_and_counts_dropped_directions():
    k, r = 4, 6
    alpha, W, b = _planted(k, r, seed=13, pairs=False)
    f = _bundle(alpha, W, np.ones(r), np.eye(k), kern=DoubleWithProject(), blocks=((0, 4),))
    with pytest.raises(ValueError, match="4 coordinates"):
        f.restart([torch.zeros((1, 4), dtype=torch.float64)], np.array([1.0]))             # T k = 4 < r = 6
    # a duplicated eigenvalue (with its mode): N is singular in exactly one direction; the minimum-norm solution
    # splits the amplitude evenly and reproduces the window
    alpha2, W2 = np.concatenate([alpha, alpha[:1]]), np.concatenate([W, W[:, :1]], axis=1)
    t = np.linspace(0.0, 2.0, 15)
    C = ((np.exp(np.outer(t, alpha)) * b) @ W.T).real
    f = _bundle(alpha2, W2, np.ones(r + 1), np.eye(k), kern=DoubleWithProject(), blocks=((0, 4),))
    g = f.restart([torch.from_numpy(C)], t)
    assert g.result.info["restart_dropped"] == 1
    amp = g.result.amplitudes.numpy()
    assert amp[0] == pytest.approx(amp[-1], rel=1e-9)
    f0 = _bundle(alpha, W, np.ones(r), np.eye(k), kern=DoubleWithProject(), blocks=((0, 4),))
    g0 = f0.restart([torch.from_numpy(C)], t)
    assert g0.result.info["restart_dropped"] == 0
    assert g.result.rel_error == pytest.approx(g0.result.rel_error, abs=1e-9)
    assert 2 * amp[0] == pytest.approx(g0.result.amplitudes.numpy()[0], rel=1e-8)
    with pytest.raises(ValueError):
        from dmd_era5_amd.forecast import DmdForecast

        DmdForecast([torch.eye(4)]).restart([torch.zeros((1, 4))], np.array([1.0]))


# ---------------------------------------------------------------- the result file's basis
def _synthetic_result(dtype, with_stats, seed=21, M=37, n=12, r=5):
    from dmd_era5_amd.era5_svd import combine_svd_results
    from dmd_era5_amd.labeled import Coord, DataArray

    rs = np.random.RandomState(seed)
    U = np.linalg.qr(rs.standard_normal((M, r)))[0]
    V = np.linalg.qr(rs.standard_normal((n, r)))[0].T
    s = np.linspace(9.0, 1.0, r)
    coords = {"space": Coord("space", np.arange(M)), "time": Coord("time", np.arange(100, 100 + n))}
    kw = {}
    if with_stats:
        kw["X_mean"] = DataArray((280.0 + rs.standard_normal(M)).astype(dtype), ("space",), {"space": coords["space"]})
        kw["X_std"] = DataArray((5.0 + 10.0 * rs.rand(M)).astype(dtype), ("space",), {"space": coords["space"]})
    return combine_svd_results(U.astype(dtype), s.astype(dtype), V.astype(dtype), coords, **kw), (U, s, V)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("with_stats", [False, True])
def test_project_onto_svd_results_inverts_reconstruct(dtype, with_stats):
    from dmd_era5_amd import era5_svd
    from dmd_era5_amd.labeled import Coord, DataArray

    ds, (U, s, V) = _synthetic_result(dtype, with_stats)
    sV = s[:, None] * V
    tol = (1e-12 if dtype == np.float64 else 2e-4) * np.abs(sV).max()
    for K in (DoubleWithProject(), CpuKernelDouble()):
        X = era5_svd.reconstruct_from_svd_results(ds, kern=K)              # de-standardised when the file has the stats
        C = era5_svd.project_onto_svd_results(ds, X, kern=K)               # ... which are the defaults here as well
        assert C.dims == ("components", "time") and C.values.dtype == dtype and C.values.shape == sV.shape
        assert np.array_equal(C.coords["time"].values, ds.coords["time"].values)
        assert np.array_equal(C.coords["components"].values, np.arange(5))
        assert np.abs(C.values - sV).max() <= tol
        assert C.attrs["captured_total"] == pytest.approx(1.0, abs=1e-5)
        assert C.attrs["energy_total"] == pytest.approx((s ** 2).sum(), rel=1e-4)
    # fewer components; a plain array has no time coordinate; explicit mean / std win over the file's
    C3 = era5_svd.project_onto_svd_results(ds, X.values, n_components=3, kern=K)
    assert C3.values.shape == (3, 12) and "time" not in C3.coords and np.abs(C3.values - sV[:3]).max() <= tol
    assert C3.attrs["captured_total"] == pytest.approx((s[:3] ** 2).sum() / (s ** 2).sum(), abs=1e-4)
    Xs = era5_svd.reconstruct_from_svd_results(ds, destandardize=False, kern=K)
    M = U.shape[0]
    C1 = era5_svd.project_onto_svd_results(ds, Xs, mean=np.zeros(M, dtype=dtype), std=np.ones(M, dtype=dtype), kern=K)
    assert np.abs(C1.values - sV).max() <= tol
    # new snapshots, not part of the decomposition: against the plain fp64 expression
    rs = np.random.RandomState(22)
    Xn = (280.0 + 10.0 * rs.standard_normal((M, 4))).astype(dtype)
    da = DataArray(Xn, ("space", "time"), {"time": Coord("time", np.arange(4))})
    Z = Xn.astype(np.float64)
    if with_stats:
        Z = (Z - ds["X_mean"].values.astype(np.float64)[:, None]) / ds["X_std"].values.astype(np.float64)[:, None]
    want = ds["U"].values.astype(np.float64).T @ Z
    Cn = era5_svd.project_onto_svd_results(ds, da, kern=K)
    assert np.abs(Cn.values - want).max() <= (1e-12 if dtype == np.float64 else 1e-5) * np.abs(want).max()
    assert Cn.attrs["energy_total"] == pytest.approx((Z * Z).sum(), rel=1e-6)
    assert np.array_equal(Cn.coords["time"].values, np.arange(4))
    with pytest.raises(ValueError, match="space"):
        era5_svd.project_onto_svd_results(ds, Xn[:-1], kern=K)
    with pytest.raises(ValueError):
        era5_svd.project_onto_svd_results(ds, Xn, n_components=6, kern=K)
    with pytest.raises(ValueError, match="zero"):
        era5_svd.project_onto_svd_results(ds, Xn, std=np.zeros(M, dtype=dtype), kern=K)


def test_alias_package_exports_project():
    import dmd_era5.era5_svd as alias
    import dmd_era5.forecast as alias_fc
    from dmd_era5_amd import era5_svd, forecast

    assert alias.project_onto_svd_results is era5_svd.project_onto_svd_results
    assert "project_onto_svd_results" in alias.__all__ and "project_onto_svd_results" in era5_svd.__all__
    assert "project_blocks" in forecast.__all__ and alias_fc.project_blocks is forecast.project_blocks
    assert hasattr(forecast.DmdForecast, "project") and hasattr(forecast.DmdForecast, "restart")


# ---------------------------------------------------------------- C ABI without a GPU
@pytest.fixture(scope="module")
def lib():
    from dmd_era5_amd import _lib

    return _lib.load()


def test_project_argument_errors_without_a_gpu(lib):
    inv, wsp = -1000, -1001
    kmax = lib.dmdx_project_max_k()
    assert kmax == 256
    p = 4096                                     # a non-null address: every call is refused before it is used
    ok = dict(U=p, m=10, k=3, ldu=10, X=p, ldx=10, T=5, mu=None, sigma=None, C=p, ldc=3, energy=p, ws=p, wsb=1 << 30)

    def project(**o):
        a = {**ok, **o}
        return lib.dmdx_project_f32(a["U"], a["m"], a["k"], a["ldu"], a["X"], a["ldx"], a["T"], a["mu"], a["sigma"], a["C"],
                                    a["ldc"], a["energy"], 0, a["ws"], a["wsb"], None)

    for o in (dict(U=None), dict(X=None), dict(C=None), dict(k=0), dict(k=kmax + 1), dict(ldu=9), dict(ldc=2), dict(ldx=0),
              dict(m=0), dict(T=0), dict(m=2 ** 31, ldu=2 ** 31), dict(T=2 ** 31), dict(ldu=2 ** 31), dict(ldx=2 ** 31),
              dict(ldc=2 ** 31)):
        assert project(**o) == inv, o
        assert b"project" in lib.dmdx_last_error(), o
    assert b"null" in (project(U=None), lib.dmdx_last_error())[1]
    need = lib.dmdx_project_workspace_bytes(10, 3, 5)
    assert project(wsb=need - 1) == wsp and b"project" in lib.dmdx_last_error() and b"workspace" in lib.dmdx_last_error()
    assert project(ws=None) == wsp
    # rows > ldx is the delay view, not an error: such a call gets as far as the workspace check
    assert project(ldx=4, wsb=need - 1) == wsp


def test_project_workspace_planner_on_degenerate_shapes(lib):
    for m, k, T in itertools.product([1, 3, 63], repeat=3):
        assert lib.dmdx_project_workspace_bytes(m, k, T) > 0
    assert lib.dmdx_project_workspace_bytes(0, 3, 5) == lib.dmdx_project_workspace_bytes(3, 3, 0) == 16
    # one fp32 slot per (row range of at most 4096 rows, k, T): far below X itself for a cfg2 row block, and the
    # energy slots on top
    big = lib.dmdx_project_workspace_bytes(129780, 50, 8760)
    ranges = -(-129780 // 4096)
    assert big == 16 + ranges * 50 * 8760 * 4 + ranges * 8760 * 4
    assert big < 129780 * 8760 * 4 // 50
    # few snapshots: the row range shrinks (to no less than 256 rows) so that the launch still fills the chip
    small = lib.dmdx_project_workspace_bytes(129780, 50, 24)
    assert small == 16 + -(-129780 // 256) * (50 * 24 * 4 + 24 * 4)
