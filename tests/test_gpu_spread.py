"""K15 on the GPU through the ctypes table: dmdx_spread_f32 and dmdx_spread_score_f32.

Shapes (parity with numpy fp64 of the same fp32 inputs, bounds of tests/spread_ref.py), memory (operands inside
NaN-canary guard zones, exact 0xFF workspaces: tests/memguard.py), values (the B = 1 identity with K12, exact
integers, member addressing, planted NaN / Inf, power-of-two scaling).  Every operand of every case lives in a
guarded allocation, so each parity case is a memory-edge case as well.
"""
import itertools

import numpy as np
import pytest
import torch

import memguard as mg
import spread_ref as sr

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DEV = "cuda"
E_INVALID, E_WORKSPACE = -1000, -1001

MS = [1, 31, 33, 127, 129, 257]
TS = [1, 15, 33, 65]
BS = [1, 2, 3, 8, 33]
LAYOUTS = [0, 1, 2, 3]
ENTRIES = ["spread", "score"]


@pytest.fixture(scope="module")
def L():
    from dmd_era5_amd.kernels import default_kernels

    return default_kernels()._lib


def _ks(L):
    return [1, 15, 16, 17, 64, 65, 129, 225, int(L.dmdx_spread_max_k())]


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Case:
    """Guarded operands of one call.  layout: 0 tight, 1 padded leading dimensions (multiples of 4), 2 odd
    leading dimensions and bases 1 .. 3 elements past a 16-byte boundary, 3 as 1 without sigma (the layouts of
    test_gpu_expand.Case).  D is the logical (k, B T) matrix."""

    def __init__(self, m, k, T, B, layout, U, D, sigma=None):
        self.m, self.k, self.T, self.B = m, k, T, B
        pad = {0: 0, 1: 4, 2: 3, 3: 8}[layout]
        off = (lambda j: (1 + j) % 4 if layout == 2 else 0)
        self.U, self.D, self.sigma = U, D, sigma
        self.gU = mg.Guarded(m, k, m + pad, F32, off(0), DEV).fill(U).snapshot()
        self.gD = mg.Guarded(k, B * T, k + pad, F32, off(1), DEV).fill(D).snapshot()
        self.gsg = None if sigma is None else mg.Guarded(m, 1, m, F32, off(0), DEV).fill(sigma).snapshot()
        self.gS = mg.Guarded(m, T, m + pad, F32, off(2), DEV)
        self.gcol = mg.Guarded(T, 1, T, F64, 0, DEV)
        self.grow = mg.Guarded(m, 1, m, F64, 0, DEV)

    def inputs(self):
        return [g for g in (self.gU, self.gD, self.gsg) if g is not None]

    def check_inputs(self):
        for g in self.inputs():
            g.check_untouched("input")
            g.check_unchanged("input")

    def _args(self, over):
        a = dict(U=self.gU.ptr, m=self.m, k=self.k, ldu=self.gU.ld, D=self.gD.ptr, ldd=self.gD.ld, T=self.T, B=self.B,
                 sigma=None if self.gsg is None else self.gsg.ptr)
        a.update(over)
        return a

    def spread(self, L, **over):
        a = self._args({**dict(S=self.gS.ptr, lds=self.gS.ld), **over})
        rc = L.dmdx_spread_f32(a["U"], a["m"], a["k"], a["ldu"], a["D"], a["ldd"], a["T"], a["B"], a["sigma"], a["S"],
                               a["lds"], _stream())
        torch.cuda.synchronize()
        return rc

    def score(self, L, accumulate=0, rows=True, ws=None, **over):
        need = L.dmdx_spread_score_workspace_bytes(self.m, self.k, self.T, self.B)
        assert need > 0
        self.ws = mg.exact_workspace(need, DEV) if ws is None else ws
        a = self._args({**dict(col=self.gcol.ptr, wsp=self.ws.ptr, wsb=self.ws.nbytes), **over})
        rc = L.dmdx_spread_score_f32(a["U"], a["m"], a["k"], a["ldu"], a["D"], a["ldd"], a["T"], a["B"], a["sigma"],
                                     a["col"], self.grow.ptr if rows else None, accumulate, a["wsp"], a["wsb"], _stream())
        torch.cuda.synchronize()
        return rc

    def s(self):
        return self.gS.logical()

    def sums(self):
        return self.gcol.logical()[:, 0], self.grow.logical()[:, 0]


def rand_case(rng, m, k, T, B, layout):
    U = rng.standard_normal((m, k)).astype(np.float32)
    D = rng.standard_normal((k, B * T)).astype(np.float32)
    sigma = None
    if layout != 3:   # both signs: the spread takes |sigma|
        sigma = ((0.5 + rng.random(m)) * rng.choice([-1.0, 1.0], m)).astype(np.float32)
    return Case(m, k, T, B, layout, U, D, sigma)


def parity_shapes(L):
    """A pairwise-covering sample of (m, k, T, B, layout): greedily, the combination that covers the most pairs of
    values not seen together yet, until every pair of every two lists has been.  Deterministic, ~60 cases."""
    lists = [MS, _ks(L), TS, BS, LAYOUTS]
    todo = {(a, x, b, y) for a, b in itertools.combinations(range(5), 2) for x in lists[a] for y in lists[b]}
    cands = list(itertools.product(*lists))
    out = []
    while todo:
        def gain(c):
            return sum((a, c[a], b, c[b]) in todo for a, b in itertools.combinations(range(5), 2))
        best = max(cands, key=gain)
        todo -= {(a, best[a], b, best[b]) for a, b in itertools.combinations(range(5), 2)}
        out.append(best)
    assert len(out) <= 90
    return out


def check_spread(L, c):
    assert c.spread(L) == 0, L.dmdx_last_error()
    c.gS.check_fully_written("S")
    c.gS.check_untouched("S")
    c.check_inputs()
    got = c.s()
    assert not np.signbit(got).any()
    err = np.abs(got.astype(np.float64) - sr.spread64(c.U, c.D, c.T, c.B, c.sigma))
    bound = sr.spread_bound(c.U, c.D, c.T, c.B, c.sigma)
    assert (err <= bound).all(), (c.m, c.k, c.T, c.B, float((err / np.maximum(bound, 1e-300)).max()))


def check_score(L, c, variant=0):
    """variant 0: both outputs; 1: then once more with accumulate (var_col doubles bit for bit, var_row is
    overwritten with the same bits); 2: without var_row (it keeps the canary)."""
    rows = variant != 2
    assert c.score(L, rows=rows) == 0, L.dmdx_last_error()
    c.gcol.check_fully_written("var_col")
    for g, name in ((c.gcol, "var_col"), (c.grow, "var_row")):
        g.check_untouched(name)
    if rows:
        c.grow.check_fully_written("var_row")
    else:
        assert bool((c.grow.ibuf == c.grow.canary).all())
    c.ws.check_untouched()
    c.check_inputs()
    want = sr.spread_score64(c.U, c.D, c.T, c.B, c.sigma)
    bounds = sr.spread_score_bounds(c.U, c.D, c.T, c.B, c.sigma)
    for g, w, b, name in list(zip(c.sums(), want, bounds, ("var_col", "var_row")))[:2 if rows else 1]:
        assert (np.abs(g - w) <= b).all(), (name, c.m, c.k, c.T, c.B, float((np.abs(g - w) / np.maximum(b, 1e-300)).max()))
    if variant == 1:
        first = [a.copy() for a in c.sums()]
        assert c.score(L, accumulate=1) == 0, L.dmdx_last_error()
        assert np.array_equal(c.sums()[0], 2.0 * first[0])
        assert np.array_equal(c.sums()[1].view(np.int64), first[1].view(np.int64))
        c.ws.check_untouched()
        c.gcol.check_untouched("var_col")


@pytest.mark.parametrize("entry", ENTRIES)
def test_parity_over_the_shape_edges(L, entry):
    rng = np.random.default_rng(1501)
    for n, (m, k, T, B, layout) in enumerate(parity_shapes(L)):
        c = rand_case(rng, m, k, T, B, layout)
        if entry == "spread":
            check_spread(L, c)
        else:
            check_score(L, c, n % 3)


@pytest.mark.parametrize("entry", ENTRIES)
def test_several_workgroups_and_time_splits(L, entry):
    """m past one row block with T past one tile: the T split, the partial slots of several row blocks and both
    reduce kernels take part (2100 rows = 17 row blocks, 5 tiles)."""
    rng = np.random.default_rng(1502)
    for n, (m, k, T, B, layout) in enumerate(((2100, 37, 131, 5, 2), (777, 200, 97, 3, 1))):
        c = rand_case(rng, m, k, T, B, layout)
        if entry == "spread":
            check_spread(L, c)
        else:
            check_score(L, c, 1)


# ---------------------------------------------------------------- B = 1: K12's chain
@pytest.mark.parametrize("k", [50, 129, 255])
def test_one_member_is_the_absolute_value_of_expand(L, k):
    """sqrt(fl(a^2)) = |a| exactly for normal magnitudes, so with B = 1 S is bit for bit |Xhat| of
    dmdx_expand_f32(U, D, NULL, sigma): the k order of the chain is K12's (layout 2: no alignment anywhere)."""
    rng = np.random.default_rng(1503)
    m, T = 200, 45
    c = rand_case(rng, m, k, T, 1, 2)
    assert c.spread(L) == 0, L.dmdx_last_error()
    gX = mg.Guarded(m, T, m + 3, F32, 3, DEV)
    rc = L.dmdx_expand_f32(c.gU.ptr, m, k, c.gU.ld, c.gD.ptr, c.gD.ld, T, None, c.gsg.ptr, gX.ptr, gX.ld, _stream())
    torch.cuda.synchronize()
    assert rc == 0, L.dmdx_last_error()
    assert np.array_equal(c.s().view(np.int32), np.abs(gX.logical()).view(np.int32))


# ---------------------------------------------------------------- exact integers
def int_case(rng, m, k, T, layout, a_u, a_e):
    """Integer U in [-a_u, a_u] and E in [-a_e, a_e], D = [3 E | 4 E] (B = 2), sigma in {1/2, 1, 2} with both signs:
    P_0 = 3 U E, P_1 = 4 U E, V = 25 (U E)^2 and S = 5 |sigma| |U E|, every intermediate an integer (a multiple of
    1/4 in the sums) below 2^24."""
    U = rng.integers(-a_u, a_u + 1, (m, k)).astype(np.float32)
    E = rng.integers(-a_e, a_e + 1, (k, T)).astype(np.float32)
    sigma = (rng.choice([0.5, 1.0, 2.0], m) * rng.choice([-1.0, 1.0], m)).astype(np.float32)
    P = (U.astype(np.int64) @ E.astype(np.int64))
    assert 4 * k * a_u * a_e < 2 ** 24 and 25 * (P ** 2).max() < 2 ** 24
    c = Case(m, k, T, 2, layout, U, np.concatenate([3 * E, 4 * E], axis=1), sigma)
    W4 = (4 * sigma.astype(np.float64) ** 2).astype(np.int64)[:, None] * 25 * P ** 2      # 4 sigma^2 V, integers
    # the fp32 part of the column sums runs over the 128 rows of a workgroup, of the row sums over a 32-column tile
    assert np.add.reduceat(W4, np.arange(0, m, sr.FP32_ROWS), axis=0).max() < 2 ** 24
    assert np.add.reduceat(W4, np.arange(0, T, 32), axis=1).max() < 2 ** 24
    c.want = (5.0 * np.abs(sigma.astype(np.float64))[:, None] * np.abs(P), W4.sum(axis=0) / 4.0, W4.sum(axis=1) / 4.0)
    return c


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("shape", [(131, 17, 77, 2, 2, 2), (1003, 50, 70, 1, 1, 1), (3000, 200, 70, 0, 1, 1),
                                   (40000, 7, 300, 2, 2, 2)])
def test_exact_integers(L, entry, shape):
    """Bit-exact against integer arithmetic, up to 313 workgroup rows with two tiles per workgroup and a T split
    (40000 x 300): a member that is dropped, repeated or read from the wrong column offset, or a dropped or
    doubled row or snapshot, changes the answer by a non-zero integer."""
    c = int_case(np.random.default_rng(1504), *shape)
    S, col, row = c.want
    if entry == "spread":
        assert c.spread(L) == 0, L.dmdx_last_error()
        assert np.array_equal(c.s().astype(np.float64), S) and not np.signbit(c.s()).any()
        c.gS.check_untouched("S")
    else:
        assert c.score(L) == 0, L.dmdx_last_error()
        got = c.sums()
        assert np.array_equal(got[0], col), "var_col"
        assert np.array_equal(got[1], row), "var_row"
        c.ws.check_untouched()


def test_member_addressing(L):
    """B = 3 with member 1 all zeros and members 0 and 2 distinct, T no multiple of the tile: an off-by-one in
    b T + t moves a zero column into a member or a member column out of it.  Integers: V = P_0^2 + P_2^2 exactly,
    S its correctly rounded root."""
    rng = np.random.default_rng(1505)
    m, k, T = 150, 23, 45
    U = rng.integers(-2, 3, (m, k)).astype(np.float32)
    E0, E2 = (rng.integers(-3, 4, (k, T)).astype(np.float32) for _ in range(2))
    c = Case(m, k, T, 3, 2, U, np.concatenate([E0, np.zeros_like(E0), E2], axis=1), None)
    P0, P2 = (U.astype(np.int64) @ E.astype(np.int64) for E in (E0, E2))
    V = P0 ** 2 + P2 ** 2
    assert V.max() < 2 ** 24 and V.sum(axis=0).max() < 2 ** 24
    assert c.spread(L) == 0 and c.score(L) == 0, L.dmdx_last_error()
    assert np.array_equal(c.s(), np.sqrt(V.astype(np.float32)))
    assert np.array_equal(c.sums()[0], V.sum(axis=0).astype(np.float64))
    assert np.array_equal(c.sums()[1], V.sum(axis=1).astype(np.float64))


# ---------------------------------------------------------------- NaN / Inf, scaling, reproducibility
def _cls(a):
    a = np.asarray(a, dtype=np.float64)
    return np.where(np.isnan(a), 3, np.where(np.isposinf(a), 1, np.where(np.isneginf(a), 2, 0)))


PLANTS = [("D", np.nan), ("D", np.inf), ("D", -np.inf), ("U", np.nan), ("U", np.inf), ("U_last", -np.inf),
          ("sigma", np.nan), ("sigma", np.inf), ("sigma", -np.inf)]


@pytest.mark.parametrize("entry", ENTRIES)
def test_planted_nan_and_inf(L, entry):
    """k = 37 is no multiple of the 16-column granule; "U_last" plants in the last real column of U, next to the
    zero pad.  Class of every output = numpy fp64's (never -Inf, never a sign bit on a number); outputs the element
    does not take part in keep the bits of the clean run."""
    rng = np.random.default_rng(1506)
    m, k, T, B = 150, 37, 70, 3
    base = rand_case(rng, m, k, T, B, 2)
    i0, j0, t0, b0 = 77, 11, 41, 1
    assert (base.spread(L) if entry == "spread" else base.score(L)) == 0
    with np.errstate(all="ignore"):
        for what, val in PLANTS:
            U, D, sigma = base.U.copy(), base.D.copy(), base.sigma.copy()
            if what == "U":
                U[i0, j0] = val
            elif what == "U_last":
                U[i0, k - 1] = val
            elif what == "D":
                D[j0, b0 * T + t0] = val
            else:
                sigma[i0] = val
            c = Case(m, k, T, B, 2, U, D, sigma)
            if entry == "spread":
                assert c.spread(L) == 0
                got, clean = c.s(), base.s()
                want = sr.spread64(U, D, T, B, sigma)
                assert np.array_equal(_cls(got), _cls(want)), (what, val)
                hit = np.zeros((m, T), dtype=bool)
                if what == "D":
                    hit[:, t0] = True
                else:
                    hit[i0, :] = True
                assert np.array_equal(_cls(want) != 0, hit), (what, val)
                assert np.array_equal(got.view(np.int32)[~hit], clean.view(np.int32)[~hit]), (what, val)
                assert not np.signbit(got[~np.isnan(got)]).any()
            else:
                assert c.score(L) == 0
                want = sr.spread_score64(U, D, T, B, sigma)
                for n, (g, cl, w) in enumerate(zip(c.sums(), base.sums(), want)):
                    assert np.array_equal(_cls(g), _cls(w)), (what, val, n)
                    fin = _cls(w) == 0
                    # D: var_col[t0] and every var_row; U / sigma: var_row[i0] and every var_col
                    assert (~fin).sum() == ((1 if n == 0 else m) if what == "D" else (T if n == 0 else 1))
                    assert np.array_equal(g.view(np.int64)[fin], cl.view(np.int64)[fin]), (what, val, n)


@pytest.mark.parametrize("entry", ENTRIES)
def test_power_of_two_scaling_commutes(L, entry):
    rng = np.random.default_rng(1507)
    m, k, T, B = 200, 50, 45, 4
    base = rand_case(rng, m, k, T, B, 1)
    up, dn = np.float32(2.0 ** 40), np.float32(2.0 ** -40)
    for su, sd in ((up, dn), (dn, up)):
        c = Case(m, k, T, B, 1, base.U * su, base.D * sd, base.sigma)
        if entry == "spread":
            assert base.spread(L) == 0 and c.spread(L) == 0
            assert torch.equal(c.gS.iview, base.gS.iview)
        else:
            assert base.score(L) == 0 and c.score(L) == 0
            for a, b in zip(c.sums(), base.sums()):
                assert np.array_equal(a.view(np.int64), b.view(np.int64))


def test_two_calls_give_the_same_bits(L):
    rng = np.random.default_rng(1508)
    c = rand_case(rng, 1003, 50, 131, 7, 2)
    assert c.spread(L) == 0 and c.score(L) == 0, L.dmdx_last_error()
    firsts = [g.iview.clone() for g in (c.gS, c.gcol, c.grow)]
    for g in (c.gS, c.gcol, c.grow):
        g.ibuf.fill_(g.canary)
    assert c.spread(L) == 0 and c.score(L) == 0
    for g, f in zip((c.gS, c.gcol, c.grow), firsts):
        assert torch.equal(g.iview, f)
        g.check_untouched()


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("entry", ENTRIES)
def test_refused_calls_write_nothing(L, entry):
    rng = np.random.default_rng(1509)
    c = rand_case(rng, 70, 9, 40, 3, 1)
    kmax = int(L.dmdx_spread_max_k())
    assert kmax == 256
    big = 2 ** 31
    bad = [dict(U=None), dict(D=None), dict(m=0), dict(T=0), dict(B=0), dict(m=-1), dict(B=-3), dict(k=0), dict(k=kmax + 1),
           dict(ldu=c.m - 1), dict(ldd=c.k - 1), dict(m=big, ldu=big), dict(T=big), dict(ldu=big), dict(ldd=big),
           dict(B=big // c.T + 1), dict(B=big)]
    if entry == "spread":
        bad += [dict(S=None), dict(lds=c.m - 1), dict(lds=big)]
        for over in bad:
            assert c.spread(L, **over) == E_INVALID, over
            assert L.dmdx_last_error()
    else:
        ws = mg.exact_workspace(L.dmdx_spread_score_workspace_bytes(c.m, c.k, c.T, c.B), DEV)
        bad += [dict(col=None)]
        for over in bad:
            assert c.score(L, ws=ws, **over) == E_INVALID, over
            assert L.dmdx_last_error()
        assert c.score(L, ws=ws, wsb=ws.nbytes - 1) == E_WORKSPACE
        assert L.dmdx_last_error()
        assert c.score(L, ws=ws, wsp=None) == E_WORKSPACE
        ws.check_unused()
        ws.check_untouched()
    for g in (c.gS, c.gcol, c.grow):
        assert bool((g.ibuf == g.canary).all())
    c.check_inputs()
