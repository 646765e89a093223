"""CPU tests of the layer above K19: tests/crps_ref.py itself, forecast.member_coefficients and crps_blocks through
the torch fallback (a provider without ``crps``) and through the numpy double of the kernel (crps_ref.CrpsDouble),
against a direct numpy evaluation."""
import functools

import numpy as np
import pytest
import torch

import crps_ref as cr
import expand_ref as er
from crps_ref import CrpsDouble
from expand_ref import ExpandDouble
from kernel_double import CpuKernelDouble


class DoubleWithCrps(CrpsDouble, ExpandDouble, CpuKernelDouble):
    name = "cpu-double+expand+crps"


PROVIDERS = [CpuKernelDouble, DoubleWithCrps]          # torch fallback / kernel double
KEYS = ("crps", "member_mae", "member_distance")
M, SPLIT, K, T, B, G = 240, (70, 100, 70), 6, 9, 5, 5


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def test_the_pair_sum_of_the_reference_is_the_sorted_form():
    """sum_{b < b'} |x_b - x_b'| = sum_i (2 i - B - 1) x_(i), i = 1 .. B over the sorted members: an independent form
    of what crps64 adds pair by pair."""
    rs = np.random.RandomState(190)
    for Bn in (1, 2, 3, 8, 9, 33):
        m, k, Tn = 37, 5, 11
        U = rs.standard_normal((m, k)).astype(np.float32)
        C = rs.standard_normal((k, Bn * Tn)).astype(np.float32)
        mu = rs.standard_normal(m).astype(np.float32)
        sd = (0.5 + rs.rand(m)).astype(np.float32)
        X = rs.standard_normal((m, Tn)).astype(np.float32)
        P = cr.members64(U, C, Tn, Bn, mu, sd)
        _, pair, rank = cr.quantities64(P, X)
        coef = 2.0 * np.arange(1, Bn + 1) - Bn - 1
        want = (np.sort(P, axis=0) * coef[:, None, None]).sum(axis=0)
        assert np.allclose(pair, want, rtol=1e-12, atol=1e-12)
        assert rank.min() >= 0 and rank.max() <= Bn
        col, row, hist = cr.crps64(U, C, Tn, Bn, X, mu, sd, None)
        assert hist.sum() == m * Tn and hist.shape == (Bn + 1,)
        assert np.allclose(col[1], want.sum(axis=0)) and np.allclose(row[1], want.sum(axis=1))


@functools.lru_cache(maxsize=None)
def problem(delay, Bn=B):
    """Three row blocks of M rows in all: per block U (k, d rows), X (T + d - 1, rows), per physical row mean, std,
    weight (some 0, with NaN in X there) and an unsorted group label; group 3 is absent from the last block."""
    rs = np.random.RandomState(191 + delay)
    lab = rs.randint(0, G, M)
    lab[SPLIT[0] + SPLIT[1]:][lab[SPLIT[0] + SPLIT[1]:] == 3] = 4
    w = (0.1 + rs.rand(M)).astype(np.float32)
    w[rs.choice(M, 11, replace=False)] = 0.0
    mu = (3.0 * rs.standard_normal(M)).astype(np.float32)
    sd = (0.5 + rs.rand(M)).astype(np.float32)
    Cm = (rs.standard_normal((1, T, K)) + 0.3 * rs.standard_normal((Bn, T, K))).astype(np.float32)
    edges = np.cumsum((0,) + SPLIT)
    blocks = []
    for a, b in zip(edges[:-1], edges[1:]):
        mb = b - a
        U = rs.standard_normal((K, delay * mb)).astype(np.float32)
        X = (np.tile(mu[a:b], (T + delay - 1, 1)) + rs.standard_normal((T + delay - 1, mb))).astype(np.float32)
        X[:, w[a:b] == 0] = np.nan
        blocks.append(dict(U=U, X=X, mu=mu[a:b], sd=sd[a:b], w=w[a:b], lab=lab[a:b]))
    return Cm, blocks


def embedded(blocks, delay):
    out = {key: [] for key in ("U", "X", "mu", "sd", "w", "lab")}
    for Bk in blocks:
        Tn = Bk["X"].shape[0] - delay + 1
        out["U"].append(Bk["U"].T)
        out["X"].append(np.concatenate([Bk["X"][j:j + Tn].T for j in range(delay)], axis=0))
        for key in ("mu", "sd", "w", "lab"):
            out[key].append(np.tile(Bk[key], delay))
    return {key: np.concatenate(v) for key, v in out.items()}


def call_blocks(Cm, blocks, delay, kern, **kw):
    from dmd_era5_amd.forecast import crps_blocks

    lists = {name: [_t(Bk[key]) for Bk in blocks] for name, key in (("means", "mu"), ("stds", "sd"), ("weights", "w"))}
    lists.update(kw)
    groups = lists.pop("groups", [torch.from_numpy(Bk["lab"].astype(np.int64)) for Bk in blocks])
    return crps_blocks([_t(Bk["U"]) for Bk in blocks], _t(Cm), [_t(Bk["X"]) for Bk in blocks], groups=groups, delay=delay,
                       kern=kern, **lists)


def reference(Cm, blocks, delay, Gn):
    E = embedded(blocks, delay)
    Bn, Tn, k = Cm.shape
    C = Cm.reshape(Bn * Tn, k).T
    out = []
    for g in range(Gn):
        s = E["lab"] == g
        col, _, hist = cr.crps64(E["U"][s], C, Tn, Bn, E["X"][s], E["mu"][s], E["sd"][s], E["w"][s])
        ww = E["w"][s].astype(np.float64)
        out.append((col, hist, ww[ww != 0].sum(), int(s.sum()), int((ww == 0).sum())))
    return out


def compare(res, ref, Bn, fair=True):
    for g, (col, hist, W, rows, masked) in enumerate(ref):
        got = res["sums"][g].numpy()
        assert np.isfinite(got).all()
        # both sides are fp64 here: agreement to rounding, far inside the fp32 bound of the kernel
        assert np.allclose(got, col, rtol=1e-11, atol=1e-11), g
        assert np.array_equal(res["rank_hist"][g].numpy(), hist), g
        assert float(res["weight"][g]) == pytest.approx(W, rel=1e-14)
        assert int(res["rows"][g]) == rows and int(res["masked_rows"][g]) == masked
        want = cr.scores(col, W, Bn, fair)
        tot = cr.scores(col.sum(axis=1), W * col.shape[1], Bn, fair)
        for key in KEYS:
            assert np.allclose(res[key][g].numpy(), want[key], rtol=1e-10, atol=1e-12, equal_nan=True), (key, g)
            assert np.allclose(float(res[key + "_total"][g]), tot[key], rtol=1e-10, atol=1e-12, equal_nan=True), (key, g)


@pytest.mark.parametrize("provider", PROVIDERS)
@pytest.mark.parametrize("delay", [1, 2])
@pytest.mark.parametrize("fair", [True, False])
def test_crps_blocks_with_groups_in_runs_masked_rows_and_a_delay(provider, delay, fair):
    Cm, blocks = problem(delay)
    assert (np.diff(blocks[0]["lab"]) != 0).sum() > 20 and 3 not in blocks[2]["lab"]
    res = call_blocks(Cm, blocks, delay, provider(), want_rows=True, fair=fair)
    assert res["sums"].shape == (G, 2, T) and res["crps"].shape == (G, T) and res["rank_hist"].shape == (G, B + 1)
    assert res["rank_hist"].dtype == torch.int64
    assert int(res["masked_rows"].sum()) == 11 * delay and int(res["rows"].sum()) == M * delay
    assert int(res["rank_hist"].sum()) == (M - 11) * delay * T
    compare(res, reference(Cm, blocks, delay, G), B, fair)
    assert len(res["row_crps"]) == 3
    Bn, Tn, k = Cm.shape
    for Bk, rc in zip(blocks, res["row_crps"]):
        E = embedded([Bk], delay)
        with np.errstate(all="ignore"):
            row = cr.crps64(E["U"], Cm.reshape(Bn * Tn, k).T, Tn, Bn, E["X"], E["mu"], E["sd"], None)[1]
        fin = E["w"] != 0
        want = row[0] / (Bn * Tn) - row[1] / ((Bn * (Bn - 1) if fair else Bn * Bn) * Tn)
        assert np.isnan(rc.numpy()[~fin]).all()
        assert np.allclose(rc.numpy()[fin], want[fin], rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("provider", PROVIDERS)
def test_plain_is_not_below_fair_and_not_above_the_member_error(provider):
    Cm, blocks = problem(1)
    fair = call_blocks(Cm, blocks, 1, provider(), fair=True)
    plain = call_blocks(Cm, blocks, 1, provider(), fair=False)
    assert torch.equal(fair["sums"], plain["sums"]) and torch.equal(fair["rank_hist"], plain["rank_hist"])
    assert bool((fair["crps"] <= plain["crps"]).all()) and bool((plain["crps"] <= plain["member_mae"]).all())
    assert bool((plain["crps"] >= 0).all())


@pytest.mark.parametrize("provider", PROVIDERS)
def test_one_group_and_a_stated_number_of_groups(provider):
    Cm, blocks = problem(2)
    res = call_blocks(Cm, blocks, 2, provider())
    one = call_blocks(Cm, blocks, 2, provider(), groups=None)
    assert one["sums"].shape == (1, 2, T)
    assert torch.allclose(one["sums"][0], res["sums"].sum(dim=0), rtol=1e-12, atol=1e-12)
    assert torch.equal(one["rank_hist"][0], res["rank_hist"].sum(dim=0))
    more = call_blocks(Cm, blocks, 2, provider(), n_groups=7)
    assert more["sums"].shape == (7, 2, T) and float(more["weight"][6]) == 0.0 and int(more["rank_hist"][5].sum()) == 0
    assert torch.equal(more["sums"][:G], res["sums"])
    with pytest.raises(ValueError, match="n_groups"):
        call_blocks(Cm, blocks, 2, provider(), n_groups=3)


class TwoRanks:
    """A two-rank Comm double: the all-reduce adds what the other rank would contribute and counts the collectives."""

    world_size, rank, exchanges, timed = 2, 0, True, None

    def __init__(self, other=None):
        self.other, self.tags, self.sent = other, [], None

    def allreduce_sum_(self, t, tag="allreduce"):
        self.tags.append(tag)
        self.sent = t.clone()
        if self.other is not None:
            t += self.other
        return t


@pytest.mark.parametrize("provider", PROVIDERS)
def test_two_ranks_one_collective_and_a_rank_that_misses_a_label(provider):
    """Rank 1 holds the last block only, which has no row of group 3, and says n_groups; rank 0 the other two.  Each
    issues ONE collective; the sum is the single-process result.  A rank without blocks takes part as well."""
    Cm, blocks = problem(2)
    one = call_blocks(Cm, blocks, 2, provider())
    c1 = TwoRanks()
    call_blocks(Cm, blocks[2:], 2, provider(), comm=c1, n_groups=G)
    assert c1.tags == ["crps_allreduce"]
    c0 = TwoRanks(other=c1.sent)
    res = call_blocks(Cm, blocks[:2], 2, provider(), comm=c0, n_groups=G)
    assert c0.tags == ["crps_allreduce"]
    for key in ("sums", "weight") + KEYS + tuple(k + "_total" for k in KEYS):
        assert torch.allclose(res[key], one[key], rtol=1e-12, atol=1e-13, equal_nan=True), key
    for key in ("rank_hist", "rows", "masked_rows"):
        assert torch.equal(res[key], one[key]), key
    empty = TwoRanks(other=c0.sent + c1.sent)
    res = call_blocks(Cm, [], 2, provider(), comm=empty, n_groups=G, groups=[], means=[], stds=[], weights=[])
    assert empty.tags == ["crps_allreduce"] and float(empty.sent.abs().sum()) == 0.0
    assert torch.equal(res["rank_hist"], one["rank_hist"])


@pytest.mark.parametrize("provider", PROVIDERS)
def test_one_member_plain_is_the_weighted_mean_absolute_error_and_fair_raises(provider):
    Cm, blocks = problem(1, 1)
    assert Cm.shape[0] == 1
    res = call_blocks(Cm, blocks, 1, provider(), fair=False)
    E = embedded(blocks, 1)
    Xh = er.expand64(E["U"], Cm[0].T, E["mu"], E["sd"])
    for g in range(G):
        s = (E["lab"] == g) & (E["w"] != 0)
        w = E["w"][s].astype(np.float64)
        mae = (w[:, None] * np.abs(Xh[s] - E["X"][s])).sum(axis=0) / w.sum()
        assert np.allclose(res["crps"][g].numpy(), mae, rtol=1e-12)
        assert torch.equal(res["crps"][g], res["member_mae"][g]) and bool(torch.isnan(res["member_distance"][g]).all())
        assert float(res["sums"][g, 1].abs().sum()) == 0.0
    with pytest.raises(ValueError, match="fair"):
        call_blocks(Cm, blocks, 1, provider(), fair=True)


@pytest.mark.parametrize("bad", [-0.5, np.nan, np.inf])
def test_bad_weights_are_refused_before_any_launch(bad):
    class Never(DoubleWithCrps):
        def crps(self, *a, **k):
            raise AssertionError("launched")

    Cm, blocks = problem(1)
    w = [_t(Bk["w"]) for Bk in blocks]
    w[2] = w[2].clone()
    w[2][5] = bad
    with pytest.raises(ValueError, match="weights of block 2"):
        call_blocks(Cm, blocks, 1, Never(), weights=w)


def test_a_streamed_x_is_consumed_block_by_block():
    """``Xblocks`` as a generator: when the launches of block b run, block b + 1 has not been asked for (a streamed X
    has one block alive at a time), and the result is the one of the list."""
    from dmd_era5_amd.forecast import crps_blocks

    rs = np.random.RandomState(193)
    rows, Bn, Tn, k = (5, 7, 4), 3, 4, 2
    Ub = [_t(rs.standard_normal((k, mb)).astype(np.float32)) for mb in rows]
    Xb = [_t(rs.standard_normal((Tn, mb)).astype(np.float32)) for mb in rows]
    Cm = _t(rs.standard_normal((Bn, Tn, k)).astype(np.float32))
    groups = [torch.arange(mb) % 2 for mb in rows]                   # runs of one row: several launches per block
    yielded, seen = [], []

    def stream():
        for b, X in enumerate(Xb):
            yielded.append(b)
            yield X

    class Watching(DoubleWithCrps):
        def crps(self, Ut, *a, **kw):
            seen.append((len(yielded), int(Ut.shape[1])))
            return super().crps(Ut, *a, **kw)

    got = crps_blocks(Ub, Cm, stream(), groups=groups, kern=Watching(), want_rows=True)
    assert [n for n, _ in seen] == [b + 1 for b, mb in enumerate(rows) for _ in range(mb)]
    assert yielded == [0, 1, 2]
    want = crps_blocks(Ub, Cm, Xb, groups=groups, kern=DoubleWithCrps(), want_rows=True)
    assert set(got) == set(want)
    for key, v in want.items():
        if isinstance(v, list):
            assert len(got[key]) == len(v) and all(torch.equal(a, b) for a, b in zip(got[key], v)), key
        else:
            assert torch.equal(got[key], v), key


def test_member_coefficients_are_the_members_bit_for_bit():
    from test_ensemble import _members

    from dmd_era5_amd.forecast import dmd_coefficients, member_coefficients

    members = _members(5, 7, seed=6)
    t = torch.from_numpy(np.linspace(0.0, 3.0, 12))
    Cm, imag = member_coefficients(members, t)
    assert Cm.dtype == torch.float32 and Cm.shape[:2] == (5, 12) and Cm.is_contiguous()
    ratios = []
    for b, r in enumerate(members):
        c, q = dmd_coefficients(r, t)
        ratios.append(q)
        assert torch.equal(Cm[b].view(torch.int32), c.view(torch.int32)), b
    assert imag == max(ratios)
    with pytest.raises(ValueError, match="no members"):
        member_coefficients([], t)


@pytest.mark.parametrize("provider", PROVIDERS)
def test_forecast_ensemble_crps_is_crps_blocks_of_the_trials(provider):
    from test_ensemble import _bundle, _members

    from dmd_era5_amd.forecast import crps_blocks, member_coefficients

    rs = np.random.RandomState(192)
    members = _members(5, 7, seed=6)
    f, Ub, mu, sd = _bundle(members, provider, rs)
    t = torch.from_numpy(np.linspace(0.0, 3.0, 12))
    rows = [u.shape[1] for u in Ub]
    X = [_t(rs.standard_normal((12, mb)).astype(np.float32) + m_) for mb, m_ in zip(rows, mu)]
    w = [_t((0.1 + rs.rand(mb)).astype(np.float32)) for mb in rows]
    w[0][3] = 0.0
    groups = [torch.arange(mb) % 2 for mb in rows]
    res = f.ensemble_crps(X, t, weights=w, groups=groups, want_rows=True)
    Cm, imag = member_coefficients(f.result.trials, t)
    want = crps_blocks(f.Ublocks, Cm, X, f.means, f.stds, w, groups, kern=f.kern, want_rows=True)
    assert res["imag_ratio"] == imag and set(res) == set(want) | {"imag_ratio"}
    for key, v in want.items():
        if isinstance(v, list):
            assert all(torch.equal(a, b) for a, b in zip(res[key], v)), key
        else:
            assert torch.equal(res[key], v, ) or bool(torch.isnan(v).all()), key
    assert res["sums"].shape == (2, 2, 12) and int(res["masked_rows"].sum()) == 1
    assert int(res["rank_hist"].sum()) == (sum(rows) - 1) * 12
    plain = f.ensemble_crps(X, t, weights=w, groups=groups, fair=False)
    assert bool((plain["crps"] <= plain["member_mae"]).all())
