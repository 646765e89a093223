"""CPU tests of the layer above K24: tests/exceed_ref.py itself, forecast.exceed_blocks / exceed_prob_blocks through
the torch fallback (a provider without ``exceed_score``) and through the numpy double of the kernel
(exceed_ref.ExceedDouble), against a direct numpy evaluation; Climatology.thresholds / slots; the refusals of the new
C entry points, which need no GPU."""
import functools
import itertools
import os

import numpy as np
import pytest
import torch

import exceed_ref as xr
import expand_ref as er
from exceed_ref import ExceedDouble
from expand_ref import ExpandDouble
from kernel_double import CpuKernelDouble
from test_crps import TwoRanks


class DoubleWithExceed(ExceedDouble, ExpandDouble, CpuKernelDouble):
    name = "cpu-double+expand+exceed"


PROVIDERS = [CpuKernelDouble, DoubleWithExceed]          # torch fallback / kernel double
KEYS = ("brier", "brier_fair", "base_rate", "forecast_rate", "brier_skill")
M, SPLIT, K, T, B, G, J, S = 240, (70, 100, 70), 6, 9, 5, 5, 3, 3
Z = (-0.8, 0.0, 0.9)


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


@functools.lru_cache(maxsize=None)
def problem(delay, Bn=B):
    """Three row blocks of M rows in all: per block U (k, d rows), X (T + d - 1, rows), per physical row mean, std,
    weight (some 0, with NaN in X there), an unsorted group label and a (J, S, rows) threshold table; group 3 is
    absent from the last block.  The analysis is a member-like field plus noise, the thresholds sit at Z standard
    deviations of the fields around the mean, so both outcomes and every count occur."""
    rs = np.random.RandomState(241 + delay)
    lab = rs.randint(0, G, M)
    lab[SPLIT[0] + SPLIT[1]:][lab[SPLIT[0] + SPLIT[1]:] == 3] = 4
    w = (0.1 + rs.rand(M)).astype(np.float32)
    w[rs.choice(M, 11, replace=False)] = 0.0
    mu = (3.0 * rs.standard_normal(M)).astype(np.float32)
    sd = (0.5 + rs.rand(M)).astype(np.float32)
    C0 = rs.standard_normal((1, T, K))
    Cm = (C0 + 0.5 * rs.standard_normal((Bn, T, K))).astype(np.float32)
    slot = rs.randint(0, S, T).astype(np.int32)
    edges = np.cumsum((0,) + SPLIT)
    blocks = []
    for a, b in zip(edges[:-1], edges[1:]):
        mb = b - a
        U = rs.standard_normal((K, delay * mb)).astype(np.float32)
        X = np.empty((T + delay - 1, mb), dtype=np.float32)
        truth = (C0[0] + 0.5 * rs.standard_normal((T, K))) @ U            # (T, d rows)
        for j in range(delay):
            X[j:j + T] = mu[a:b] + sd[a:b] * truth[:, j * mb:(j + 1) * mb]   # (overlapping delays: the last one stays)
        X[:, w[a:b] == 0] = np.nan
        thr = np.stack([mu[a:b] + z * sd[a:b] * np.sqrt(K) * (1.0 + 0.1 * rs.standard_normal((S, mb))) for z in Z])
        blocks.append(dict(U=U, X=X, mu=mu[a:b], sd=sd[a:b], w=w[a:b], lab=lab[a:b], thr=thr.astype(np.float32)))
    return Cm, slot, blocks


def embedded(blocks, delay):
    out = {key: [] for key in ("U", "X", "mu", "sd", "w", "lab", "thr")}
    for Bk in blocks:
        Tn = Bk["X"].shape[0] - delay + 1
        out["U"].append(Bk["U"].T)
        out["X"].append(np.concatenate([Bk["X"][j:j + Tn].T for j in range(delay)], axis=0))
        for key in ("mu", "sd", "w", "lab"):
            out[key].append(np.tile(Bk[key], delay))
        out["thr"].append(np.tile(Bk["thr"], (1, 1, delay)).transpose(2, 0, 1))       # (d rows, J, S)
    return {key: np.concatenate(v) for key, v in out.items()}


def call_blocks(Cm, slot, blocks, delay, kern, above=True, **kw):
    from dmd_era5_amd.forecast import exceed_blocks

    lists = {name: [_t(Bk[key]) for Bk in blocks] for name, key in (("means", "mu"), ("stds", "sd"), ("weights", "w"))}
    lists.update(kw)
    groups = lists.pop("groups", [torch.from_numpy(Bk["lab"].astype(np.int64)) for Bk in blocks])
    thresholds = lists.pop("thresholds", [_t(Bk["thr"]) for Bk in blocks])
    return exceed_blocks([_t(Bk["U"]) for Bk in blocks], _t(Cm), [_t(Bk["X"]) for Bk in blocks], thresholds, slot, above,
                         groups=groups, delay=delay, kern=kern, **lists)


def direct(E, Cm, slot, above, rounded, sel_rows, weighted=True):
    """The sums, counts and row sums of the embedded rows ``sel_rows``, element by element in numpy: the fields in
    fp64 (``rounded``: rounded to fp32, what the kernel double sees), p = fp32(c / B), the quantities and sums fp64."""
    Bn, Tn, k = Cm.shape
    U, mu, sd = E["U"][sel_rows], E["mu"][sel_rows], E["sd"][sel_rows]
    F = np.stack([er.expand64(U, Cm[b].T, mu, sd) for b in range(Bn)])
    if rounded:
        F = F.astype(np.float32)
    th = E["thr"][sel_rows][:, :, slot].transpose(1, 0, 2)                # (J, rows, T)
    X = E["X"][sel_rows]
    cmp = np.greater if above else np.less
    with np.errstate(invalid="ignore"):
        c = cmp(F[:, None], th[None]).sum(axis=0)
        o = cmp(X[None], th)
    p = (c / Bn).astype(np.float32).astype(np.float64)
    fin = np.isfinite(X) & np.isfinite(F).all(axis=0)
    Q = np.stack([(p - o) ** 2, o.astype(np.float64), p, p * p], axis=1)  # (J, 4, rows, T)
    Q = np.where(fin[None, None], Q, np.nan)
    w = E["w"][sel_rows].astype(np.float64) if weighted else np.ones(len(U))
    keep = w != 0
    col = (Q[:, :, keep] * w[keep][None, None, :, None]).sum(axis=2)
    cnt = np.zeros((th.shape[0], 2, Bn + 1), dtype=np.int64)
    live = fin & keep[:, None]
    for j in range(th.shape[0]):
        np.add.at(cnt[j], (o[j][live].astype(int), c[j][live]), 1)
    return col, cnt, Q.sum(axis=3), w[keep].sum(), len(U), int((~keep).sum())


def compare(res, E, Cm, slot, above, rounded, Gn, Bn):
    tol = dict(rtol=1e-6, atol=1e-9) if rounded else dict(rtol=1e-11, atol=1e-11)     # fl32(d d), fl32(w q) in the double
    for g in range(Gn):
        col, cnt, _, W, rows, masked = direct(E, Cm, slot, above, rounded, E["lab"] == g)
        got = res["sums"][g].numpy()
        assert np.isfinite(got).all()
        assert np.allclose(got, col, **tol), g
        assert np.array_equal(res["counts"][g].numpy(), cnt), g
        assert float(res["weight"][g]) == pytest.approx(W, rel=1e-14)
        assert int(res["rows"][g]) == rows and int(res["masked_rows"][g]) == masked
        want, tot = xr.scores(col, W, Bn), xr.scores(col.sum(axis=2, keepdims=True), W * col.shape[2], Bn)
        for key in KEYS:
            assert np.allclose(res[key][g].numpy(), want[key], rtol=1e-5, atol=1e-8, equal_nan=True), (key, g)
            assert np.allclose(res[key + "_total"][g].numpy(), tot[key][:, 0], rtol=1e-5, atol=1e-8, equal_nan=True), (key, g)
        Nc = cnt.sum(axis=1)
        assert np.array_equal(res["bin_counts"][g].numpy(), Nc)
        with np.errstate(all="ignore"):
            assert np.allclose(res["reliability"][g].numpy(), cnt[:, 1] / Nc, equal_nan=True)
        rel, reso, unc = xr.murphy(cnt)
        for key, v in (("reliability_term", rel), ("resolution_term", reso), ("uncertainty", unc), ("roc_area", xr.roc_area(cnt))):
            assert np.allclose(res[key][g].numpy(), v, rtol=1e-12, atol=1e-14), (key, g)


@pytest.mark.parametrize("provider", PROVIDERS)
@pytest.mark.parametrize("delay", [1, 2])
@pytest.mark.parametrize("above", [True, False])
def test_exceed_blocks_with_groups_in_runs_masked_rows_and_a_delay(provider, delay, above):
    Cm, slot, blocks = problem(delay)
    assert (np.diff(blocks[0]["lab"]) != 0).sum() > 20 and 3 not in blocks[2]["lab"]
    res = call_blocks(Cm, slot, blocks, delay, provider(), above, want_rows=True)
    assert res["sums"].shape == (G, J, 4, T) and res["brier"].shape == (G, J, T) and res["counts"].shape == (G, J, 2, B + 1)
    assert res["counts"].dtype == torch.int64 and res["brier_total"].shape == (G, J) and res["roc_area"].shape == (G, J)
    assert int(res["masked_rows"].sum()) == 11 * delay and int(res["rows"].sum()) == M * delay
    assert (res["counts"].sum(dim=(0, 2, 3)) == (M - 11) * delay * T).all()
    # the problem can tell a constant answer apart: both outcomes, and counts strictly between 0 and B
    assert bool((res["counts"][:, :, :, 1:B].sum(dim=(0, 2, 3)) > 0.1 * (M - 11) * delay * T).all())
    assert bool((res["counts"].sum(dim=(0, 3)) > 0).all())
    rounded = provider is DoubleWithExceed
    E = embedded(blocks, delay)
    compare(res, E, Cm, slot, above, rounded, G, B)
    assert len(res["row_brier"]) == 3
    for Bk, rb in zip(blocks, res["row_brier"]):
        Eb = embedded([Bk], delay)
        rows = direct(Eb, Cm, slot, above, rounded, np.ones(len(Eb["U"]), dtype=bool))[2]
        fin = Eb["w"] != 0
        assert rb.shape == (J, len(fin)) and np.isnan(rb.numpy()[:, ~fin]).all()
        # (the double forms d d in fp32, as the kernel does)
        assert np.allclose(rb.numpy()[:, fin], rows[:, 0][:, fin] / T, rtol=1e-6 if rounded else 1e-10, atol=1e-12)


@pytest.mark.parametrize("provider", PROVIDERS)
def test_one_group_a_stated_number_of_groups_and_one_slot(provider):
    Cm, slot, blocks = problem(2)
    res = call_blocks(Cm, slot, blocks, 2, provider())
    one = call_blocks(Cm, slot, blocks, 2, provider(), groups=None)
    assert one["sums"].shape == (1, J, 4, T)
    assert torch.allclose(one["sums"][0], res["sums"].sum(dim=0), rtol=1e-12, atol=1e-12)
    assert torch.equal(one["counts"][0], res["counts"].sum(dim=0))
    more = call_blocks(Cm, slot, blocks, 2, provider(), n_groups=7)
    assert more["sums"].shape == (7, J, 4, T) and float(more["weight"][6]) == 0.0 and int(more["counts"][5].sum()) == 0
    assert torch.equal(more["sums"][:G], res["sums"])
    # a (J, rows) table is one slot and wants no labels: the result of the (J, 1, rows) table with every label 0
    flat = call_blocks(Cm, None, blocks, 2, provider(), thresholds=[_t(Bk["thr"][:, 1]) for Bk in blocks])
    same = call_blocks(Cm, np.zeros(T, dtype=np.int64), blocks, 2, provider(), thresholds=[_t(Bk["thr"][:, 1:2]) for Bk in blocks])
    assert torch.equal(flat["sums"], same["sums"]) and torch.equal(flat["counts"], same["counts"])


@pytest.mark.parametrize("provider", PROVIDERS)
def test_two_ranks_one_collective_and_a_rank_without_blocks(provider):
    """Rank 1 holds the last block only, which has no row of group 3, and says n_groups; rank 0 the other two.  Each
    issues ONE collective; the sum is the single-process result.  A rank without blocks says J and takes part."""
    Cm, slot, blocks = problem(2)
    one = call_blocks(Cm, slot, blocks, 2, provider())
    c1 = TwoRanks()
    call_blocks(Cm, slot, blocks[2:], 2, provider(), comm=c1, n_groups=G)
    assert c1.tags == ["exceed_allreduce"]
    c0 = TwoRanks(other=c1.sent)
    res = call_blocks(Cm, slot, blocks[:2], 2, provider(), comm=c0, n_groups=G)
    assert c0.tags == ["exceed_allreduce"]
    for key in ("sums", "weight", "roc_area", "reliability_term") + KEYS + tuple(k + "_total" for k in KEYS):
        assert torch.allclose(res[key], one[key], rtol=1e-12, atol=1e-13, equal_nan=True), key
    for key in ("counts", "bin_counts", "rows", "masked_rows"):
        assert torch.equal(res[key], one[key]), key
    empty = TwoRanks(other=c0.sent + c1.sent)
    res = call_blocks(Cm, slot, [], 2, provider(), comm=empty, n_groups=G, groups=[], means=[], stds=[], weights=[],
                      thresholds=J)
    assert empty.tags == ["exceed_allreduce"] and float(empty.sent.abs().sum()) == 0.0
    assert torch.equal(res["counts"], one["counts"])


@pytest.mark.parametrize("provider", PROVIDERS)
def test_unit_weights_the_counts_rebuild_the_brier_score_and_its_decomposition(provider):
    """With unit weights every element is in one bin (o, c) and contributes (c / B - o)^2: the Brier score is a sum
    over the bins, and Murphy's reliability - resolution + uncertainty equals it."""
    Cm, slot, blocks = problem(1)
    clean = [dict(Bk, X=np.where(np.isnan(Bk["X"]), Bk["mu"], Bk["X"]).astype(np.float32)) for Bk in blocks]
    res = call_blocks(Cm, slot, clean, 1, provider(), weights=None)
    N = res["counts"].to(torch.float64)
    pc = (torch.arange(B + 1, dtype=torch.float64) / B).to(torch.float32).to(torch.float64)
    rebuilt = (N[:, :, 0] * pc ** 2 + N[:, :, 1] * (pc - 1.0) ** 2).sum(dim=2) / N.sum(dim=(2, 3))
    assert torch.allclose(rebuilt, res["brier_total"], rtol=1e-6, atol=1e-12)
    murphy = res["reliability_term"] - res["resolution_term"] + res["uncertainty"]
    assert torch.allclose(murphy, res["brier_total"], rtol=1e-6, atol=1e-9)
    assert torch.allclose(N[:, :, 1].sum(dim=2) / N.sum(dim=(2, 3)), res["base_rate_total"], rtol=1e-6)
    assert bool((res["roc_area"] > 0.5).all())            # members around the truth: better than no skill


def planted(pi, Bn):
    """Every pattern of Bn members in / out of the event times both outcomes, one element each, weighted with its
    probability under independent Bernoulli(pi) members and outcome: the weighted sums ARE the expectations."""
    pats = np.array(list(itertools.product((0.0, 1.0), repeat=Bn)), dtype=np.float32)       # (2^Bn, Bn)
    n = len(pats)
    members = np.concatenate([pats, pats])                                                     # (2 n, Bn)
    outcome = np.concatenate([np.zeros(n), np.ones(n)]).astype(np.float32)
    c = members.sum(axis=1)
    w = pi ** c * (1 - pi) ** (Bn - c) * np.where(outcome == 1, pi, 1 - pi)
    return members, outcome, w.astype(np.float64)


@pytest.mark.parametrize("provider", PROVIDERS)
@pytest.mark.parametrize("pi", [0.5, 0.25])
def test_the_fair_brier_score_is_unbiased_for_a_bernoulli_ensemble(provider, pi):
    """Members and outcome independent Bernoulli(pi): the probability forecast pi has the Brier score pi (1 - pi); the
    ensemble's p = c / B has it in expectation plus pi (1 - pi) / B, and the fair score removes exactly that.  The
    expectation is the weighted sum over all 2^B patterns and both outcomes, not a sample."""
    from dmd_era5_amd.forecast import exceed_blocks

    Bn = 4
    members, outcome, w = planted(pi, Bn)
    n = len(outcome)
    U = _t(np.eye(n, dtype=np.float32))                                    # (k, rows): the field of member b is Cm[b]
    Cm = _t(members.T.reshape(Bn, 1, n))
    X = _t(outcome.reshape(1, n))
    thr = [_t(np.full((1, n), 0.5, dtype=np.float32))]
    assert w.sum() == pytest.approx(1.0, rel=1e-12)
    res = exceed_blocks([U], Cm, [X], thr, weights=[_t(w.astype(np.float32))], kern=provider())
    assert float(res["brier_fair_total"][0, 0]) == pytest.approx(pi * (1 - pi), rel=1e-6)
    assert float(res["brier_total"][0, 0]) == pytest.approx(pi * (1 - pi) * (1 + 1 / Bn), rel=1e-6)
    assert float(res["base_rate_total"][0, 0]) == pytest.approx(pi, rel=1e-6)
    assert float(res["forecast_rate_total"][0, 0]) == pytest.approx(pi, rel=1e-6)
    one = exceed_blocks([U], Cm[:1], [X], thr, kern=provider())
    assert bool(torch.isnan(one["brier_fair"]).all()) and bool(torch.isfinite(one["brier"]).all())


@pytest.mark.parametrize("provider", PROVIDERS)
def test_the_roc_area_of_a_perfect_and_of_a_constant_forecast(provider):
    from dmd_era5_amd.forecast import exceed_blocks

    n, Bn = 12, 3
    outcome = (np.arange(n) % 3 == 0).astype(np.float32)
    U, X = _t(np.eye(n, dtype=np.float32)), _t(outcome.reshape(1, n))
    thr = [_t(np.full((1, n), 0.5, dtype=np.float32))]
    perfect = exceed_blocks([U], _t(np.tile(outcome, (Bn, 1, 1))), [X], thr, kern=provider())
    assert float(perfect["roc_area"][0, 0]) == 1.0 and float(perfect["brier_total"][0, 0]) == 0.0
    assert float(perfect["resolution_term"][0, 0]) == pytest.approx(float(perfect["uncertainty"][0, 0]), rel=1e-14)
    const = np.zeros((Bn, 1, n), dtype=np.float32)
    const[0] = 1.0                                                         # c = 1 everywhere
    constant = exceed_blocks([U], _t(const), [X], thr, kern=provider())
    assert float(constant["roc_area"][0, 0]) == 0.5 and float(constant["resolution_term"][0, 0]) == 0.0
    assert xr.roc_area(np.array([[4, 0, 0, 0], [0, 0, 0, 2]])) == 1.0 and xr.roc_area(np.array([[0, 5, 0], [0, 3, 0]])) == 0.5
    # below: the event is X < 0.5, the members that are 0 are in it
    below = exceed_blocks([U], _t(np.tile(outcome, (Bn, 1, 1))), [X], thr, above=False, kern=provider())
    assert float(below["roc_area"][0, 0]) == 1.0 and float(below["base_rate_total"][0, 0]) == pytest.approx(2 / 3)
    # a tie is no event in either direction
    tie = [_t(outcome.reshape(1, n).copy())]
    for above in (True, False):
        r = exceed_blocks([U], _t(np.tile(outcome, (Bn, 1, 1))), [X], tie, above=above, kern=provider())
        assert int(r["counts"][0, 0, 0, 0]) == n and float(r["brier_total"][0, 0]) == 0.0


@pytest.mark.parametrize("provider", PROVIDERS)
def test_prob_blocks_the_delay_blocks_and_the_forecast_methods(provider):
    from test_ensemble import _bundle, _members

    from dmd_era5_amd.forecast import exceed_blocks, exceed_prob_blocks, member_coefficients

    Cm, slot, blocks = problem(2)
    Ub, th = [_t(Bk["U"]) for Bk in blocks], [_t(Bk["thr"]) for Bk in blocks]
    mu, sd = [_t(Bk["mu"]) for Bk in blocks], [_t(Bk["sd"]) for Bk in blocks]
    P = exceed_prob_blocks(Ub, _t(Cm), th, slot, True, mu, sd, delay=2, kern=provider())
    P1 = exceed_prob_blocks(Ub, _t(Cm), th, slot, True, mu, sd, delay_block=1, delay=2, kern=provider())
    E = embedded(blocks, 2)
    at = 0
    for Bk, p, p1 in zip(blocks, P, P1):
        mb = len(Bk["mu"])
        rows = np.zeros(len(E["U"]), dtype=bool)
        rows[at:at + 2 * mb] = True
        at += 2 * mb
        F = np.stack([er.expand64(E["U"][rows], Cm[b].T, E["mu"][rows], E["sd"][rows]) for b in range(B)])
        if provider is DoubleWithExceed:
            F = F.astype(np.float32)
        c = (F[:, None] > E["thr"][rows][:, :, slot].transpose(1, 0, 2)[None]).sum(axis=0)
        assert p.shape == (J, T, 2 * mb) and p.dtype == torch.float32 and p1.shape == (J, T, mb)
        assert np.array_equal(p.numpy(), (c / B).astype(np.float32).transpose(0, 2, 1))
        assert torch.equal(p1, p[:, :, mb:])
    out = [torch.empty_like(p) for p in P]
    again = exceed_prob_blocks(Ub, _t(Cm), th, slot, True, mu, sd, out=out, delay=2, kern=provider())
    assert all(a is o and torch.equal(a, p) for a, o, p in zip(again, out, P))
    # the forecast bundle: the trials of a bagged fit
    rs = np.random.RandomState(242)
    members = _members(5, 7, seed=6)
    f, Ubs, mus, sds = _bundle(members, provider, rs)
    t = torch.from_numpy(np.linspace(0.0, 3.0, 12))
    rws = [u.shape[1] for u in Ubs]
    Xb = [_t(rs.standard_normal((12, mb)).astype(np.float32) + m_) for mb, m_ in zip(rws, mus)]
    w = [_t((0.1 + rs.rand(mb)).astype(np.float32)) for mb in rws]
    w[0][3] = 0.0
    groups = [torch.arange(mb) % 2 for mb in rws]
    thr = [_t(np.stack([m_ + z * s_ for z in (-0.5, 0.5)]).astype(np.float32)) for m_, s_ in zip(mus, sds)]
    res = f.ensemble_exceedance(Xb, t, thr, weights=w, groups=groups, want_rows=True)
    Cm5, imag = member_coefficients(f.result.trials, t)
    want = exceed_blocks(f.Ublocks, Cm5, Xb, thr, None, True, f.means, f.stds, w, groups, kern=f.kern, want_rows=True)
    assert res["imag_ratio"] == imag and set(res) == set(want) | {"imag_ratio"}
    for key, v in want.items():
        if isinstance(v, list):
            assert all(torch.equal(a, b, ) for a, b in zip(res[key], v)), key
        else:
            assert torch.equal(torch.nan_to_num(res[key].to(torch.float64), nan=-7.0),
                               torch.nan_to_num(v.to(torch.float64), nan=-7.0)), key
    fields = f.exceedance_fields(t, thr)
    wantf = exceed_prob_blocks(f.Ublocks, Cm5, thr, None, True, f.means, f.stds, kern=f.kern)
    assert all(torch.equal(a, b) and a.shape == (2, 12, mb) for a, b, mb in zip(fields, wantf, rws))


def test_wrapper_refusals():
    Cm, slot, blocks = problem(1)
    kern = DoubleWithExceed()

    class Never(DoubleWithExceed):
        def exceed_score(self, *a, **k):
            raise AssertionError("launched")

    with pytest.raises(ValueError, match="threshold tables for 3 blocks"):
        call_blocks(Cm, slot, blocks, 1, kern, thresholds=[_t(Bk["thr"]) for Bk in blocks[:2]])
    with pytest.raises(ValueError, match="integer labels in 0 .. 2"):
        call_blocks(Cm, slot + 1, blocks, 1, Never())
    with pytest.raises(ValueError, match="integer labels"):
        call_blocks(Cm, slot[:-1], blocks, 1, Never())
    with pytest.raises(ValueError, match="slot must name one"):
        call_blocks(Cm, None, blocks, 1, Never())
    with pytest.raises(ValueError, match="same J"):
        call_blocks(Cm, slot, blocks, 1, Never(), thresholds=[_t(Bk["thr"][:1 + (n == 0)]) for n, Bk in enumerate(blocks)])
    with pytest.raises(ValueError, match="has 69 entries"):
        call_blocks(Cm, slot, blocks, 1, Never(), thresholds=[_t(Bk["thr"][:, :, :69 if n == 0 else None]) for n, Bk in enumerate(blocks)])
    with pytest.raises(ValueError, match="no blocks"):
        call_blocks(Cm, slot, blocks, 1, Never(), thresholds=J)
    with pytest.raises(ValueError, match="Cm must be"):
        call_blocks(Cm[0], slot, blocks, 1, Never())
    w = [_t(Bk["w"]) for Bk in blocks]
    w[2] = w[2].clone()
    w[2][5] = -0.5
    with pytest.raises(ValueError, match="weights of block 2"):
        call_blocks(Cm, slot, blocks, 1, Never(), weights=w)


# ---------------------------------------------------------------- Climatology.thresholds / slots
def test_climatology_thresholds_and_slots():
    from dmd_era5_amd.climatology import Climatology

    rs = np.random.RandomState(243)
    rows, Sn = (5, 3), 24
    mean = [_t(rs.standard_normal((Sn, mb)).astype(np.float32)) for mb in rows]
    sd = [_t((0.5 + rs.rand(Sn, mb)).astype(np.float32)) for mb in rows]
    counts = np.full(Sn, 4)
    counts[7] = 0
    clim = Climatology("hour", 0, mean, sd, counts)
    z = (-1.0, 0.0, 1.2816)
    an, full = clim.thresholds(z), clim.thresholds(z, anomaly=False)
    for b, mb in enumerate(rows):
        assert an[b].shape == full[b].shape == (3, Sn, mb) and an[b].dtype == torch.float32 and an[b].is_contiguous()
        for j, zj in enumerate(z):
            zs = sd[b].numpy() * np.float32(zj)
            assert np.array_equal(an[b][j].numpy(), zs) and np.array_equal(full[b][j].numpy(), mean[b].numpy() + zs)
    assert clim.thresholds(0.5)[0].shape == (1, Sn, 5)
    times = np.array(["2001-03-04T05", "2001-03-04T23", "2002-01-01T00"], dtype="datetime64[h]")
    lab = clim.slots(times)
    assert lab.dtype == np.int32 and lab.tolist() == [5, 23, 0]
    with pytest.raises(ValueError, match="slot 7"):
        clim.slots(np.array(["2001-03-04T07"], dtype="datetime64[h]"))
    with pytest.raises(ValueError, match="standard deviation"):
        Climatology("hour", 0, mean, None, counts).thresholds(z)
    with pytest.raises(ValueError, match="finite"):
        clim.thresholds([np.nan])
    # thresholds and labels are what exceed_blocks takes
    from dmd_era5_amd.forecast import exceed_prob_blocks

    Ub = [_t(rs.standard_normal((2, mb)).astype(np.float32)) for mb in rows]
    Cm = _t(rs.standard_normal((4, 3, 2)).astype(np.float32))
    P = exceed_prob_blocks(Ub, Cm, an, lab, kern=DoubleWithExceed())
    assert [tuple(p.shape) for p in P] == [(3, 3, 5), (3, 3, 3)]


# ---------------------------------------------------------------- the reference and the C entry points
def test_c_over_b_in_fp32_is_the_nearest_for_every_pair():
    """fp32(fp64(c) / B) -- one fp64 division, one rounding to fp32 -- is the correctly rounded fp32 quotient for all
    0 <= c <= B <= 256 (no double rounding: the quotient of two 9-bit integers is never that close to a tie), and an
    exact comparison against the two neighbours in integers confirms it."""
    from fractions import Fraction

    for Bn in range(1, 257):
        c = np.arange(Bn + 1)
        p = (c.astype(np.float64) / Bn).astype(np.float32)
        assert np.array_equal(p, c.astype(np.float32) / np.float32(Bn))
        assert p[0] == 0.0 and p[Bn] == 1.0 and (np.diff(p) > 0).all()
    for Bn in (3, 7, 100, 127, 255, 256):
        for c in range(Bn + 1):
            p = np.float32(np.float64(c) / Bn)
            exact = Fraction(c, Bn)
            err = abs(Fraction(float(p)) - exact)
            for q in (np.nextafter(p, np.float32(2)), np.nextafter(p, np.float32(-1))):
                assert err <= abs(Fraction(float(q)) - exact)


def test_the_reference_counts_sums_and_scores_agree_with_each_other():
    rs = np.random.RandomState(244)
    Bn, m, Tn, Jn, Sn = 7, 23, 11, 2, 3
    F = rs.standard_normal((Bn, m, Tn)).astype(np.float32)
    X = rs.standard_normal((m, Tn)).astype(np.float32)
    thr = (0.5 * rs.standard_normal((m, Jn * Sn))).astype(np.float32)
    thr[3, 4] = np.nan
    slot = rs.randint(0, Sn, Tn)
    w = rs.rand(m).astype(np.float32)
    w[5] = 0.0
    X[5, 2] = np.nan
    X[9, 1] = np.inf
    for above in (True, False):
        col, row, cnt = xr.score(F, X, thr, Jn, Sn, slot, above, w)
        assert cnt.shape == (Jn, 2, Bn + 1) and (cnt.sum(axis=(1, 2)) == (m - 1) * Tn - 1).all()
        assert np.isnan(col[:, :, 1]).all() and np.isfinite(np.delete(col, 1, axis=2)).all()
        assert np.isnan(row[:, :, [5, 9]]).all() and np.isfinite(np.delete(row, [5, 9], axis=2)).all()
        bc, br = xr.score_bounds(F, np.where(np.isfinite(X), X, 0).astype(np.float32), thr, Jn, Sn, slot, above, w)
        assert (bc >= 0).all() and (br >= 0).all() and bc.max() < 1e-4
        P = xr.prob(F, thr, Jn, Sn, slot, above)
        assert P.dtype == np.float32 and P.min() >= 0 and P.max() <= 1
    both = xr.prob(F, thr, Jn, Sn, slot, True) + xr.prob(F, thr, Jn, Sn, slot, False)
    th = xr.thresholds_of(thr, Jn, Sn, Tn, slot)
    assert np.allclose(both[~np.isnan(th)], 1.0, atol=1e-6) and (both[np.isnan(th)] == 0).all()


def test_argument_errors_of_the_new_entry_points_are_reported_without_a_gpu():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists(os.path.join(root, "dmd_era5_amd", "libdmdx.so")):
        import __graft_entry__

        __graft_entry__.build()
    from dmd_era5_amd import _lib

    lib = _lib.load()
    assert (lib.dmdx_exceed_max_k(), lib.dmdx_exceed_max_members(), lib.dmdx_exceed_max_thresholds()) == (256, 256, 4)
    one = 0x1000                # a non-null address that is never used: every call below is refused before a launch
    prob = dict(U=one, m=10, k=3, ldu=10, C=one, ldc=3, T=5, B=4, mu=None, sigma=None, thr=one, ldthr=10, J=2, S=3,
                slot=None, above=1, P=one, ldp=10, pstride=50, stream=None)
    score = dict(prob, X=one, ldx=10, w=None, col=one, ldcol=5, row=None, ldrow=0, cnt=None, accumulate=0, ws=one,
                 wsb=1 << 30)
    for key in ("P", "ldp", "pstride", "stream"):
        del score[key]
    score["stream"] = None

    def call(f, args, **over):
        a = dict(args)
        a.update(over)
        return f(*a.values())

    shared = [dict(U=None), dict(C=None), dict(thr=None), dict(k=0), dict(k=257), dict(B=0), dict(B=257), dict(J=0), dict(J=5),
              dict(S=0), dict(ldthr=9), dict(ldu=9), dict(ldc=2), dict(m=0), dict(T=0), dict(J=2, S=2 ** 30), dict(T=2 ** 30),
              dict(m=2 ** 31, ldu=2 ** 31, ldthr=2 ** 31)]
    for over in shared + [dict(P=None), dict(ldp=9), dict(pstride=49)]:
        assert call(lib.dmdx_exceed_prob_f32, prob, **over) == -1000, over
        assert b"dmdx_exceed_prob_f32" in lib.dmdx_last_error()
    for over in shared + [dict(X=None), dict(col=None), dict(ldx=0), dict(ldcol=4), dict(row=one, ldrow=9)]:
        assert call(lib.dmdx_exceed_score_f32, score, **over) == -1000, over
        assert b"dmdx_exceed_score_f32" in lib.dmdx_last_error()
    assert call(lib.dmdx_exceed_score_f32, score, ws=None) == -1001 and call(lib.dmdx_exceed_score_f32, score, wsb=8) == -1001
    assert b"workspace" in lib.dmdx_last_error()
    need = lib.dmdx_exceed_score_workspace_bytes(1003, 37, 300, 5, 3)
    assert need > lib.dmdx_exceed_score_workspace_bytes(1003, 37, 300, 5, 1) > 16
    assert need - lib.dmdx_exceed_score_workspace_bytes(1003, 37, 300, 4, 3) == 8 * 10 * 2 * 3 * 8   # a bin per workgroup
    for bad in ((0, 3, 5, 4, 2), (10, 3, 0, 4, 2), (10, 3, 5, 0, 2), (10, 3, 5, 257, 2), (10, 3, 5, 4, 0), (10, 3, 5, 4, 5),
                (2 ** 31, 3, 5, 4, 2)):
        assert lib.dmdx_exceed_score_workspace_bytes(*bad) == 16
