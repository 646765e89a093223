"""CPU tests of the verification layer above K16: forecast.area_weights, verify_blocks and DmdForecast.verify,
through the torch fallback (a provider without ``verify``) and the numpy double of the kernel
(tests/verify_ref.VerifyDouble), against a direct numpy evaluation with the bounds of tests/verify_ref.py."""
import functools
import multiprocessing as mp
import os
import socket
import sys

import numpy as np
import pytest
import torch

import expand_ref as er
import verify_ref as vr
from expand_ref import ExpandDouble
from kernel_double import CpuKernelDouble
from verify_ref import VerifyDouble


class DoubleWithVerify(VerifyDouble, ExpandDouble, CpuKernelDouble):
    name = "cpu-double+expand+verify"


PROVIDERS = [CpuKernelDouble, DoubleWithVerify]        # torch fallback / kernel double
KEYS = ("rmse", "bias", "acc", "acc_centred", "activity", "skill_vs_clim")
NV, NL, NLAT, NLON = 2, 3, 5, 8
PLANE = NLAT * NLON
M = NV * NL * PLANE
SPLIT = (70, 100, 70)                                  # row blocks that cut through the groups of 40 rows
K, T = 6, 9


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


@functools.lru_cache(maxsize=None)
def grid_problem(delay, labels="sorted"):
    """A 2-variable x 3-level x 5 x 8 grid in three row blocks: per block U (k, d rows), X (T + d - 1, rows), and
    per physical row mean, std, weight (cos(lat), a few masked points whose X is NaN), clim and group label."""
    rs = np.random.RandomState(160 + delay)
    lat = np.repeat(np.linspace(-80.0, 80.0, NLAT), NLON)
    from dmd_era5_amd.forecast import area_weights

    w = np.tile(area_weights(lat).numpy(), NV * NL)
    if labels == "sorted":
        lab = np.arange(M) // PLANE
    else:           # unsorted, many short runs; group 3 is absent from the last block
        lab = rs.randint(0, 5, M)
        lab[SPLIT[0] + SPLIT[1]:][lab[SPLIT[0] + SPLIT[1]:] == 3] = 4
        lab[:PLANE] = 4 - np.arange(PLANE) % 5
    masked = rs.choice(M, 11, replace=False)
    w[masked] = 0.0
    mu = (3.0 * rs.standard_normal(M)).astype(np.float32)
    sd = (0.5 + rs.rand(M)).astype(np.float32)
    clim = (mu + rs.standard_normal(M)).astype(np.float32)
    C = rs.standard_normal((T, K)).astype(np.float32)
    edges = np.cumsum((0,) + SPLIT)
    blocks = []
    for a, b in zip(edges[:-1], edges[1:]):
        mb = b - a
        U = rs.standard_normal((K, delay * mb)).astype(np.float32)
        # the snapshots whose embedding is close to the model: delay 0's rows for the first T, the last delay's beyond
        Xh = er.expand64(U.T, C.T, np.tile(mu[a:b], delay), np.tile(sd[a:b], delay))       # (d mb, T)
        X = np.empty((T + delay - 1, mb))
        X[:T] = Xh[:mb].T
        for j in range(1, delay):
            X[T - 1 + j] = Xh[j * mb:(j + 1) * mb, T - 1]
        X = (X + 0.7 * rs.standard_normal(X.shape)).astype(np.float32)
        X[:, w[a:b] == 0] = np.nan
        blocks.append(dict(U=U, X=X, mu=mu[a:b], sd=sd[a:b], w=w[a:b].astype(np.float32), clim=clim[a:b], lab=lab[a:b]))
    return C, blocks


def embedded(blocks, delay):
    """The rows the kernel sees, all blocks stacked: U (R, k), X (R, T), the per-row vectors and labels."""
    out = {key: [] for key in ("U", "X", "mu", "sd", "w", "clim", "lab")}
    for B in blocks:
        mb, Tn = B["X"].shape[1], B["X"].shape[0] - delay + 1
        out["U"].append(B["U"].T)
        out["X"].append(np.concatenate([B["X"][j:j + Tn].T for j in range(delay)], axis=0))
        for key in ("mu", "sd", "w", "clim", "lab"):
            out[key].append(np.tile(B[key], delay))
        assert out["X"][-1].shape == (delay * mb, Tn)
    return {key: np.concatenate(v) for key, v in out.items()}


def call_blocks(C, blocks, delay, kern, **kw):
    from dmd_era5_amd.forecast import verify_blocks

    lists = {name: [_t(B[key]) for B in blocks] for name, key in (("means", "mu"), ("stds", "sd"), ("weights", "w"),
                                                                  ("clims", "clim"))}
    lists.update(kw)
    groups = lists.pop("groups", [torch.from_numpy(B["lab"].astype(np.int64)) for B in blocks])
    return verify_blocks([_t(B["U"]) for B in blocks], _t(C), [_t(B["X"]) for B in blocks], groups=groups, delay=delay,
                         kern=kern, **lists)


def reference(C, blocks, delay, G):
    """Per group: (col64 (6, T), its bound, W, rows, masked rows)."""
    E = embedded(blocks, delay)
    out = []
    for g in range(G):
        s = E["lab"] == g
        args = (E["U"][s], C.T, E["X"][s], E["mu"][s], E["sd"][s], E["w"][s], E["clim"][s])
        with np.errstate(all="ignore"):
            col = vr.verify64(*args)[0]
            bound = vr.verify_bounds(*args)[0]
        ww = E["w"][s].astype(np.float64)
        out.append((col, bound, ww[ww != 0].sum(), int(s.sum()), int((ww == 0).sum())))
    return out


def compare(res, ref, slack=1e-13):
    for g, (col, bound, W, rows, masked) in enumerate(ref):
        got = res["sums"][g].numpy()
        assert np.isfinite(got).all()
        assert (np.abs(got - col) <= bound).all(), g
        assert float(res["weight"][g]) == pytest.approx(W, rel=1e-14)
        assert int(res["rows"][g]) == rows and int(res["masked_rows"][g]) == masked
        want, sb = vr.scores(col, W), vr.score_bounds(col, bound, W)
        # what keeps the comparison honest: the reference itself resolves the correlation to 1e-4
        assert (sb["acc"] <= 1e-4).all() and (sb["acc_centred"] <= 1e-4).all(), (g, sb["acc"].max())
        Tn = col.shape[1]
        tw, tb = vr.scores(col.sum(axis=1), W * Tn), vr.score_bounds(col.sum(axis=1), bound.sum(axis=1), W * Tn)
        for key in KEYS:
            err = np.abs(res[key][g].numpy() - want[key])
            assert (err <= sb[key] + slack * (1.0 + np.abs(want[key]))).all(), (key, g)
            assert abs(float(res[key + "_total"][g]) - tw[key]) <= tb[key] + slack * (1.0 + abs(tw[key])), (key, g)


# ---------------------------------------------------------------- the grid
@pytest.mark.parametrize("provider", PROVIDERS)
@pytest.mark.parametrize("delay", [1, 2])
def test_verify_blocks_on_a_grid_of_variables_and_levels(provider, delay):
    C, blocks = grid_problem(delay)
    res = call_blocks(C, blocks, delay, provider(), want_rows=True)
    assert res["sums"].shape == (NV * NL, 6, T) and res["rmse"].shape == (NV * NL, T)
    assert int(res["masked_rows"].sum()) == 11 * delay and int(res["rows"].sum()) == M * delay
    compare(res, reference(C, blocks, delay, NV * NL))
    # temporal scores per grid point: the plain row sums of every block, NaN where the data are
    assert len(res["row_rmse"]) == len(res["row_bias"]) == len(res["row_acc"]) == 3
    for B, rm, rb, ra in zip(blocks, res["row_rmse"], res["row_bias"], res["row_acc"]):
        E = embedded([B], delay)
        with np.errstate(all="ignore"):
            row = vr.verify64(E["U"], C.T, E["X"], E["mu"], E["sd"], None, E["clim"])[1]
        fin = E["w"] != 0
        assert np.isnan(rm.numpy()[~fin]).all() and np.isfinite(rm.numpy()[fin]).all()
        assert np.allclose(rm.numpy()[fin], np.sqrt(row[0][fin] / T), rtol=1e-5)
        assert np.allclose(rb.numpy()[fin], row[1][fin] / T, rtol=1e-4, atol=1e-6)
        assert np.allclose(ra.numpy()[fin], row[5][fin] / np.sqrt(row[3][fin] * row[4][fin]), rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("provider", PROVIDERS)
def test_unsorted_labels_and_a_group_absent_from_a_block(provider):
    C, blocks = grid_problem(2, "unsorted")
    assert 3 not in blocks[2]["lab"] and 3 in blocks[0]["lab"]
    assert (np.diff(blocks[0]["lab"]) != 0).sum() > 20                     # many runs
    res = call_blocks(C, blocks, 2, provider())
    assert res["sums"].shape[0] == 5
    compare(res, reference(C, blocks, 2, 5))
    # groups=None: one group, one launch per block; equal to all labels 0
    one = call_blocks(C, blocks, 2, provider(), groups=None)
    zero = call_blocks(C, blocks, 2, provider(), groups=[torch.zeros(len(B["lab"]), dtype=torch.int64) for B in blocks])
    assert one["sums"].shape == (1, 6, T)
    assert torch.allclose(one["sums"], zero["sums"], rtol=1e-12, atol=1e-10)
    assert torch.allclose(one["sums"][0], res["sums"].sum(dim=0), rtol=1e-12, atol=1e-12)
    # a stated number of groups: the extra ones are empty
    more = call_blocks(C, blocks, 2, provider(), n_groups=7)
    assert more["sums"].shape == (7, 6, T) and float(more["weight"][6]) == 0.0 and int(more["rows"][5]) == 0
    assert torch.equal(more["sums"][:5], res["sums"])
    with pytest.raises(ValueError, match="n_groups"):
        call_blocks(C, blocks, 2, provider(), n_groups=3)


# ---------------------------------------------------------------- known answers
def _known(kind, provider):
    """One group, one block, X built from the forecast: -> (result, reference sums, bound, W)."""
    rs = np.random.RandomState(161)
    m = 150
    U = rs.standard_normal((K, m)).astype(np.float32)
    C = rs.standard_normal((T, K)).astype(np.float32)
    mu = (3.0 * rs.standard_normal(m)).astype(np.float32)
    sd = (0.5 + rs.rand(m)).astype(np.float32)
    clim = (mu + rs.standard_normal(m)).astype(np.float32)
    w = (0.1 + rs.rand(m)).astype(np.float32)
    Xh = er.expand64(U.T, C.T, mu, sd)
    X = {"perfect": Xh, "mirror": 2.0 * clim.astype(np.float64)[:, None] - Xh, "offset": Xh - 1.25}[kind].astype(np.float32)
    B = dict(U=U, X=X.T.copy(), mu=mu, sd=sd, w=w, clim=clim, lab=np.zeros(m, dtype=np.int64))
    res = call_blocks(C, [B], 1, provider())
    args = (U.T, C.T, X, mu, sd, w, clim)
    return res, vr.verify64(*args)[0], vr.verify_bounds(*args)[0], w.astype(np.float64).sum()


@pytest.mark.parametrize("provider", PROVIDERS)
@pytest.mark.parametrize("kind,key,value", [("perfect", "rmse", 0.0), ("perfect", "acc", 1.0), ("mirror", "acc", -1.0),
                                            ("offset", "bias", 1.25), ("offset", "acc_centred", 1.0)])
def test_known_answers(provider, kind, key, value):
    """A perfect forecast, f - clim = -(x - clim), a constant offset: the known score within the propagated bound
    (plus what rounding X to fp32 moves the fp64 reference itself away from it)."""
    res, col, bound, W = _known(kind, provider)
    want, sb = vr.scores(col, W)[key], vr.score_bounds(col, bound, W)[key]
    assert (np.abs(want - value) <= 2e-6).all()
    assert np.isfinite(sb).all() and (sb <= 1e-4).all()
    got = res[key][0].numpy()
    assert (np.abs(got - want) <= sb + 1e-13).all()
    assert (np.abs(got - value) <= sb + np.abs(want - value) + 1e-13).all()


@pytest.mark.parametrize("provider", PROVIDERS)
def test_the_first_snapshot_as_climatology_gives_persistence(provider):
    C, blocks = grid_problem(1)
    blocks = [dict(B, clim=np.where(np.isnan(B["X"][0]), 0.0, B["X"][0]).astype(np.float32)) for B in blocks]
    res = call_blocks(C, blocks, 1, provider())
    E = embedded(blocks, 1)
    for g in range(NV * NL):
        s = (E["lab"] == g) & (E["w"] != 0)
        x, w = E["X"][s].astype(np.float64), E["w"][s].astype(np.float64)
        pers = np.sqrt((w[:, None] * (x - x[:, :1]) ** 2).sum(axis=0) / w.sum())
        got = torch.sqrt(res["sums"][g, 4] / res["weight"][g]).numpy()
        assert got[0] == 0.0 and np.allclose(got, pers, rtol=1e-6, atol=0.0)
        skill = 1.0 - res["sums"][g, 0] / res["sums"][g, 4]
        assert torch.equal(res["skill_vs_clim"][g][1:], skill[1:])
        assert np.allclose(res["rmse"][g].numpy()[1:], pers[1:] * np.sqrt(1.0 - skill.numpy()[1:]), rtol=1e-6)


@pytest.mark.parametrize("bad", [-0.5, np.nan, np.inf])
def test_bad_weights_are_refused_before_any_launch(bad):
    class Never(DoubleWithVerify):
        def verify(self, *a, **k):
            raise AssertionError("launched")

    C, blocks = grid_problem(1)
    w = [_t(B["w"]) for B in blocks]
    w[2] = w[2].clone()
    w[2][5] = bad
    with pytest.raises(ValueError, match="weights of block 2"):
        call_blocks(C, blocks, 1, Never(), weights=w)


def test_area_weights():
    from dmd_era5_amd.forecast import area_weights

    w = area_weights([90.0, -90.0, 0.0, 60.0, -60.0, 90.0000001])
    assert w.dtype == torch.float32 and w.shape == (6,)
    assert float(w[2]) == 1.0 and float(w[3]) == 0.5 and float(w[4]) == 0.5
    assert 0.0 <= float(w[0]) <= 1e-16 and 0.0 <= float(w[1]) <= 1e-16 and float(w[5]) == 0.0
    lat = np.linspace(90, -90, 721)
    got = area_weights(np.repeat(lat, 3)).numpy()
    assert np.array_equal(got, np.repeat(np.maximum(np.cos(np.deg2rad(lat)), 0.0).astype(np.float32), 3))


# ---------------------------------------------------------------- row shards
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _owner(world):
    """Which rank holds which of the three blocks; rank 1 never holds one."""
    return {2: (0, 0, 0), 3: (0, 0, 2)}[world]


def _worker(rank, world, port, q):
    for p in (os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist

    from dmd_era5_amd import svd as dsvd

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        C, blocks = grid_problem(2, "unsorted")
        mine = [B for B, r in zip(blocks, _owner(world)) if r == rank]
        comm = dsvd.TorchDistComm()
        comm.start_timing()
        res = call_blocks(C, mine, 2, DoubleWithVerify(), comm=comm, n_groups=5)
        timed = comm.stop_timing()
        q.put((rank, len(mine), {k: v["calls"] for k, v in timed.items()},
               {k: v.numpy() for k, v in res.items() if isinstance(v, torch.Tensor)}))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_row_shards_with_an_empty_rank_equal_the_single_process(world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    C, blocks = grid_problem(2, "unsorted")
    one = call_blocks(C, blocks, 2, DoubleWithVerify())
    assert sorted(n for _, n, _, _ in got) == sorted(_owner(world).count(r) for r in range(world))
    assert any(n == 0 for _, n, _, _ in got)
    for rank, n, calls, res in got:
        assert calls == {"verify_allreduce": 1}, (rank, calls)
        for key in ("sums", "weight") + KEYS + tuple(k + "_total" for k in KEYS):
            assert np.allclose(res[key], one[key].numpy(), rtol=1e-12, atol=1e-13), (rank, key)
        assert np.array_equal(res["rows"], one["rows"].numpy()) and np.array_equal(res["masked_rows"], one["masked_rows"].numpy())


# ---------------------------------------------------------------- DmdForecast
@pytest.mark.parametrize("provider", PROVIDERS)
def test_forecast_verify_of_the_model_and_of_the_ensemble_mean(provider):
    from test_ensemble import _bundle, _members

    from dmd_era5_amd.forecast import verify_blocks

    rs = np.random.RandomState(162)
    members = _members(5, 7, seed=6)
    f, Ub, mu, sd = _bundle(members, provider, rs)
    t = torch.from_numpy(np.linspace(0.0, 3.0, 12))
    rows = [u.shape[1] for u in Ub]
    X = [_t(rs.standard_normal((12, mb)).astype(np.float32) + m_) for mb, m_ in zip(rows, mu)]
    w = [_t((0.1 + rs.rand(mb)).astype(np.float32)) for mb in rows]
    w[0][3] = 0.0
    groups = [torch.arange(mb) % 2 for mb in rows]
    Cbar, _, imag = f.ensemble_coefficients(t)
    res = f.verify(X, t, weights=w, groups=groups, ensemble=True, want_rows=True)
    want = verify_blocks(f.Ublocks, Cbar, X, f.means, f.stds, w, None, groups, kern=f.kern, want_rows=True)
    assert res["imag_ratio"] == imag and set(res) == set(want) | {"imag_ratio"}
    for key, v in want.items():
        if isinstance(v, list):
            assert all(torch.equal(a, b) for a, b in zip(res[key], v)), key
        else:
            assert torch.equal(res[key], v), key
    assert res["sums"].shape == (2, 6, 12) and int(res["masked_rows"].sum()) == 1
    single = f.verify(X, t, weights=w, groups=groups)
    Ct, imag1 = f.coefficients(t)
    want1 = verify_blocks(f.Ublocks, Ct, X, f.means, f.stds, w, None, groups, kern=f.kern)
    assert single["imag_ratio"] == imag1 and torch.equal(single["sums"], want1["sums"])
    assert not torch.equal(single["sums"], res["sums"])
