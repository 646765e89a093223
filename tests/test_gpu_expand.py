"""K12 on the GPU through the ctypes table: dmdx_expand_f32 and dmdx_expand_score_f32.

Shapes (parity with numpy fp64 of the same fp32 inputs, bounds of tests/expand_ref.py), memory
(operands inside NaN-canary guard zones, exact 0xFF workspaces: tests/memguard.py), values (exact
integers, planted NaN / Inf, power-of-two scaling).  Every operand of every case lives in a guarded
allocation, so each parity case is a memory-edge case as well.
"""
import itertools

import numpy as np
import pytest
import torch

import expand_ref as er
import memguard as mg

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DEV = "cuda"
E_INVALID, E_WORKSPACE = -1000, -1001

MS = [1, 3, 63, 64, 65, 127, 129, 257, 1003]
TS = [1, 2, 15, 16, 17, 33, 127, 129, 300]
ENTRIES = ["expand", "score"]


@pytest.fixture(scope="module")
def L():
    from dmd_era5_amd.kernels import default_kernels

    return default_kernels()._lib


def _ks(L):
    return [1, 2, 3, 4, 5, 31, 32, 33, 50, 64, 65, 200, int(L.dmdx_expand_max_k())]


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Case:
    """Guarded operands of one call.  layout: 0 tight, 1 padded leading dimensions (multiples of 4),
    2 odd leading dimensions and bases 1 .. 3 elements past a 16-byte boundary, 3 as 1 without mu / sigma."""

    def __init__(self, m, k, T, layout, U, Cm, mu=None, sigma=None, X=None, delay_ldx=None):
        self.m, self.k, self.T = m, k, T
        pad = {0: 0, 1: 4, 2: 3, 3: 8}[layout]
        off = (lambda j: (1 + j) % 4 if layout == 2 else 0)
        self.U, self.C, self.X, self.mu, self.sigma = U, Cm, X, mu, sigma
        self.gU = mg.Guarded(m, k, m + pad, F32, off(0), DEV).fill(U).snapshot()
        self.gC = mg.Guarded(k, T, k + pad, F32, off(1), DEV).fill(Cm).snapshot()
        self.gmu = None if mu is None else mg.Guarded(m, 1, m, F32, off(2), DEV).fill(mu).snapshot()
        self.gsg = None if sigma is None else mg.Guarded(m, 1, m, F32, off(0), DEV).fill(sigma).snapshot()
        self.gXh = mg.Guarded(m, T, m + pad, F32, off(2), DEV)
        self.gX = None
        if X is not None:
            if delay_ldx is None:
                self.gX = mg.Guarded(m, T, m + pad, F32, off(1), DEV).fill(X).snapshot()
            else:   # rows > ldx: X[i, t] = flat[i + t * ldx]
                self.gX = mg.Guarded(m, T, delay_ldx, F32, off(1), DEV)
                self.gX.fbuf[self.gX.start:self.gX.start + self.gX.region] = torch.from_numpy(delay_flat(X, delay_ldx)).to(DEV)
                self.gX.snapshot()
        self.gsse = mg.Guarded(T, 1, T, F64, 0, DEV)
        self.gref = mg.Guarded(T, 1, T, F64, 0, DEV)
        self.grow = mg.Guarded(m, 1, m, F64, 0, DEV)

    def inputs(self):
        return [g for g in (self.gU, self.gC, self.gmu, self.gsg, self.gX) if g is not None]

    def check_inputs(self):
        for g in self.inputs():
            g.check_untouched("input")
            g.check_unchanged("input")

    def expand(self, L, **over):
        a = dict(U=self.gU.ptr, m=self.m, k=self.k, ldu=self.gU.ld, C=self.gC.ptr, ldc=self.gC.ld, T=self.T,
                 mu=None if self.gmu is None else self.gmu.ptr, sigma=None if self.gsg is None else self.gsg.ptr,
                 Xhat=self.gXh.ptr, ldxh=self.gXh.ld)
        a.update(over)
        rc = L.dmdx_expand_f32(a["U"], a["m"], a["k"], a["ldu"], a["C"], a["ldc"], a["T"], a["mu"], a["sigma"], a["Xhat"],
                               a["ldxh"], _stream())
        torch.cuda.synchronize()
        return rc

    def score(self, L, accumulate=0, rows=True, ref=True, ws=None, **over):
        need = L.dmdx_expand_score_workspace_bytes(self.m, self.k, self.T)
        assert need > 0
        self.ws = mg.exact_workspace(need, DEV) if ws is None else ws
        a = dict(U=self.gU.ptr, m=self.m, k=self.k, ldu=self.gU.ld, C=self.gC.ptr, ldc=self.gC.ld, T=self.T,
                 mu=None if self.gmu is None else self.gmu.ptr, sigma=None if self.gsg is None else self.gsg.ptr,
                 X=self.gX.ptr, ldx=self.gX.ld, sse=self.gsse.ptr, wsp=self.ws.ptr, wsb=self.ws.nbytes)
        a.update(over)
        rc = L.dmdx_expand_score_f32(a["U"], a["m"], a["k"], a["ldu"], a["C"], a["ldc"], a["T"], a["mu"], a["sigma"], a["X"],
                                     a["ldx"], a["sse"], self.gref.ptr if ref else None, self.grow.ptr if rows else None,
                                     accumulate, a["wsp"], a["wsb"], _stream())
        torch.cuda.synchronize()
        return rc

    def xhat(self):
        return self.gXh.logical()

    def sums(self):
        return self.gsse.logical()[:, 0], self.gref.logical()[:, 0], self.grow.logical()[:, 0]


def delay_flat(X, ldx):
    """The flat buffer of a delay view: rows > ldx, X[i, t] = flat[i + t * ldx] must be consistent."""
    m, T = X.shape
    flat = np.zeros((T - 1) * ldx + m, dtype=np.float32)
    for t in range(T):
        flat[t * ldx:t * ldx + m] = X[:, t]
    return flat


def delay_matrix(rng, m, T, ldx):
    flat = rng.standard_normal((T - 1) * ldx + m).astype(np.float32)
    return np.stack([flat[t * ldx:t * ldx + m] for t in range(T)], axis=1)


def rand_case(rng, m, k, T, layout, score):
    U = rng.standard_normal((m, k)).astype(np.float32)
    Cm = rng.standard_normal((k, T)).astype(np.float32)
    mu = sigma = None
    if layout != 3:
        mu = (10.0 * rng.standard_normal(m)).astype(np.float32)
        sigma = (0.5 + rng.random(m)).astype(np.float32)
    X = None
    if score:
        X = (er.expand64(U, Cm, mu, sigma) + rng.standard_normal((m, T))).astype(np.float32)
    return Case(m, k, T, layout, U, Cm, mu, sigma, X)


def parity_shapes(L):
    """All (m, k) pairs and all (k, T) pairs of the edge lists, the third size and the layout cycling:
    234 cases, every value of every list with every k."""
    ks = _ks(L)
    out = []
    for (im, m), (ik, k) in itertools.product(enumerate(MS), enumerate(ks)):
        out.append((m, k, TS[(im + 2 * ik) % len(TS)], (im + ik) % 4))
    for (ik, k), (it, T) in itertools.product(enumerate(ks), enumerate(TS)):
        out.append((MS[(2 * ik + it) % len(MS)], k, T, (ik + it + 1) % 4))
    return out


def check_expand(L, c):
    assert c.expand(L) == 0, L.dmdx_last_error()
    c.gXh.check_fully_written("Xhat")
    c.gXh.check_untouched("Xhat")
    c.check_inputs()
    err = np.abs(c.xhat().astype(np.float64) - er.expand64(c.U, c.C, c.mu, c.sigma))
    bound = er.element_bound(c.U, c.C, c.mu, c.sigma)
    assert (err <= bound).all(), (c.m, c.k, c.T, float((err / np.maximum(bound, 1e-300)).max()))


def check_score(L, c):
    assert c.score(L) == 0, L.dmdx_last_error()
    for g, name in ((c.gsse, "sse_col"), (c.gref, "ref_col"), (c.grow, "sse_row")):
        g.check_fully_written(name)
        g.check_untouched(name)
    c.ws.check_untouched()
    c.check_inputs()
    got = c.sums()
    want = er.score64(c.U, c.C, c.X, c.mu, c.sigma)
    bounds = er.score_bounds(c.U, c.C, c.X, c.mu, c.sigma)
    for g, w, b, name in zip(got, want, bounds, ("sse_col", "ref_col", "sse_row")):
        assert (np.abs(g - w) <= b).all(), (name, c.m, c.k, c.T, float((np.abs(g - w) / np.maximum(b, 1e-300)).max()))


@pytest.mark.parametrize("entry", ENTRIES)
def test_parity_over_the_shape_edges(L, entry):
    rng = np.random.default_rng(1201)
    for m, k, T, layout in parity_shapes(L):
        c = rand_case(rng, m, k, T, layout, entry == "score")
        (check_expand if entry == "expand" else check_score)(L, c)


@pytest.mark.parametrize("entry", ENTRIES)
def test_several_workgroups_and_time_splits(L, entry):
    """m past one row block with T past one tile per workgroup: the T split, the partial slots of
    several row blocks and both reduce kernels take part (2100 rows = 17 row blocks, 20 tiles)."""
    rng = np.random.default_rng(1202)
    for m, k, T, layout in ((2100, 37, 611, 2), (777, 200, 97, 1)):
        c = rand_case(rng, m, k, T, layout, entry == "score")
        (check_expand if entry == "expand" else check_score)(L, c)


def test_score_of_a_delay_view_and_optional_outputs(L):
    """X with rows > ldx (the zero-copy delay view); ref_col / sse_row left out; accumulate adds."""
    rng = np.random.default_rng(1203)
    m, k, T, ldx = 300, 20, 45, 100
    U = rng.standard_normal((m, k)).astype(np.float32)
    Cm = rng.standard_normal((k, T)).astype(np.float32)
    X = delay_matrix(rng, m, T, ldx)
    c = Case(m, k, T, 0, U, Cm, None, None, X, delay_ldx=ldx)
    check_score(L, c)
    first = [a.copy() for a in c.sums()]
    # without ref_col and sse_row: they keep their bits, sse_col doubles bit for bit under accumulate
    before_ref, before_row = c.gref.iview.clone(), c.grow.iview.clone()
    assert c.score(L, accumulate=1, rows=False, ref=False) == 0, L.dmdx_last_error()
    assert torch.equal(c.gref.iview, before_ref) and torch.equal(c.grow.iview, before_row)
    assert np.array_equal(c.sums()[0], 2.0 * first[0])
    c.ws.check_untouched()


@pytest.mark.parametrize("entry", ENTRIES)
def test_refused_calls_write_nothing(L, entry):
    rng = np.random.default_rng(1204)
    c = rand_case(rng, 70, 9, 40, 1, True)
    kmax = int(L.dmdx_expand_max_k())
    bad = [dict(U=None), dict(C=None), dict(k=0), dict(k=kmax + 1), dict(ldu=c.m - 1), dict(ldc=c.k - 1), dict(m=0),
           dict(T=0), dict(ldu=2 ** 31)]
    if entry == "expand":
        bad += [dict(Xhat=None), dict(ldxh=c.m - 1), dict(ldxh=2 ** 31)]
        for over in bad:
            assert c.expand(L, **over) == E_INVALID, over
            assert L.dmdx_last_error()
    else:
        ws = mg.exact_workspace(L.dmdx_expand_score_workspace_bytes(c.m, c.k, c.T), DEV)
        bad += [dict(X=None), dict(sse=None), dict(ldx=0), dict(ldx=2 ** 31)]
        for over in bad:
            assert c.score(L, ws=ws, **over) == E_INVALID, over
        assert c.score(L, ws=ws, wsb=ws.nbytes - 1) == E_WORKSPACE
        assert c.score(L, ws=ws, wsp=None) == E_WORKSPACE
        ws.check_unused()
        ws.check_untouched()
    for g in (c.gXh, c.gsse, c.gref, c.grow):
        assert bool((g.ibuf == g.canary).all())
    c.check_inputs()


# ---------------------------------------------------------------- exact integers
def int_case(rng, m, k, T, layout):
    """U in [-2, 2], C in [-3, 3], sigma in {1, 2, 4}, integer mu, X = Xhat + d, d in [-3, 3]:
    |U C| <= 6 k <= 1200, |Xhat| <= 4800 + 50, every partial sum of every order an integer below 2^24."""
    U = rng.integers(-2, 3, (m, k)).astype(np.float32)
    Cm = rng.integers(-3, 4, (k, T)).astype(np.float32)
    mu = rng.integers(-50, 51, m).astype(np.float32)
    sigma = rng.choice([1.0, 2.0, 4.0], m).astype(np.float32)
    Xh = er.expand64(U, Cm, mu, sigma)                      # exact: integers far below 2^53
    assert np.array_equal(Xh, np.rint(Xh)) and np.abs(Xh).max() < 2 ** 24
    d = rng.integers(-3, 4, (m, T))
    X = (Xh + d).astype(np.float32)
    c = Case(m, k, T, layout, U, Cm, mu, sigma, X)
    g = (X.astype(np.int64) - mu.astype(np.int64)[:, None])
    # the fp32 part of the column sums runs over the 128 rows of a workgroup: those sums stay below 2^24
    for sq in (d * d, g * g):
        blk = np.add.reduceat(sq, np.arange(0, m, er.FP32_ROWS), axis=0)
        assert blk.max() < 2 ** 24
    c.want = (Xh.astype(np.int64), (d * d).sum(axis=0), (g * g).sum(axis=0), (d * d).sum(axis=1))
    return c


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("shape", [(131, 200, 77, 2), (1003, 50, 300, 1), (30017, 200, 70, 0), (40000, 7, 33, 2)])
def test_exact_integers(L, entry, shape):
    """Bit-exact against integer arithmetic, at m of a few 10^4 rows as well (235 / 313 workgroup rows,
    a T split, both reduce kernels): one dropped or doubled row or snapshot anywhere changes a sum by a
    non-zero integer.  Two runs give the same bits."""
    c = int_case(np.random.default_rng(1205), *shape)
    Xh, sse, ref, row = c.want
    if entry == "expand":
        assert c.expand(L) == 0, L.dmdx_last_error()
        first = c.gXh.iview.clone()
        assert np.array_equal(c.xhat().astype(np.int64), Xh) and np.array_equal(c.xhat(), Xh.astype(np.float32))
        c.gXh.ibuf.fill_(c.gXh.canary)
        assert c.expand(L) == 0
        assert torch.equal(c.gXh.iview, first)
        c.gXh.check_untouched("Xhat")
    else:
        assert c.score(L) == 0, L.dmdx_last_error()
        got = c.sums()
        for g, w, name in zip(got, (sse, ref, row), ("sse_col", "ref_col", "sse_row")):
            assert np.array_equal(g, w.astype(np.float64)), name
        firsts = [g.iview.clone() for g in (c.gsse, c.gref, c.grow)]
        assert c.score(L) == 0
        for g, f in zip((c.gsse, c.gref, c.grow), firsts):
            assert torch.equal(g.iview, f)
        c.ws.check_untouched()


# ---------------------------------------------------------------- NaN / Inf, scaling
def _cls(a):
    a = np.asarray(a, dtype=np.float64)
    return np.where(np.isnan(a), 3, np.where(np.isposinf(a), 1, np.where(np.isneginf(a), 2, 0)))


PLANTS = [("U", np.nan), ("U", np.inf), ("U_last", -np.inf), ("C", np.nan), ("C", -np.inf), ("mu", np.inf), ("mu", np.nan),
          ("X", np.nan), ("X", np.inf), ("X", -np.inf)]


@pytest.mark.parametrize("entry", ENTRIES)
def test_planted_nan_and_inf(L, entry):
    """k = 37 is no multiple of the 16-column granule; "U_last" plants in the last real column of U,
    next to the zero pad.  Class of every output = numpy fp64's; outputs the element does not take part
    in keep the bits of the clean run."""
    rng = np.random.default_rng(1206)
    m, k, T = 150, 37, 70
    base = rand_case(rng, m, k, T, 2, True)
    i0, j0, t0 = 77, 11, 41
    with np.errstate(all="ignore"):
        for what, val in PLANTS:
            if entry == "expand" and what == "X":
                continue
            U, Cm, mu, X = base.U.copy(), base.C.copy(), base.mu.copy(), base.X.copy()
            if what == "U":
                U[i0, j0] = val
            elif what == "U_last":
                U[i0, k - 1] = val
            elif what == "C":
                Cm[j0, t0] = val
            elif what == "mu":
                mu[i0] = val
            else:
                X[i0, t0] = val
            c = Case(m, k, T, 2, U, Cm, mu, base.sigma, X)
            hit_row = what in ("U", "U_last", "mu", "X")
            hit_col = what in ("C", "X")
            if entry == "expand":
                assert base.expand(L) == 0 and c.expand(L) == 0
                got, clean = c.xhat(), base.xhat()
                assert np.array_equal(_cls(got), _cls(er.expand64(U, Cm, mu, base.sigma))), (what, val)
                same = np.ones((m, T), dtype=bool)
                if hit_row:
                    same[i0, :] = False
                if hit_col:
                    same[:, t0] = False
                assert np.array_equal(got.view(np.int32)[same], clean.view(np.int32)[same]), (what, val)
            else:
                assert base.score(L) == 0 and c.score(L) == 0
                want = er.score64(U, Cm, X, mu, base.sigma)
                for n, (g, cl, w) in enumerate(zip(c.sums(), base.sums(), want)):
                    assert np.array_equal(_cls(g) != 0, _cls(w) != 0), (what, val, n)
                    assert np.array_equal(_cls(g)[_cls(g) != 3], _cls(w)[_cls(g) != 3]), (what, val, n)
                    fin = _cls(w) == 0
                    # the finite ones are the sums the element takes no part in
                    if what == "X":
                        assert (~fin).sum() == 1
                    assert np.array_equal(g.view(np.int64)[fin], cl.view(np.int64)[fin]), (what, val, n)


@pytest.mark.parametrize("entry", ENTRIES)
def test_power_of_two_scaling_commutes(L, entry):
    rng = np.random.default_rng(1207)
    m, k, T = 200, 50, 45
    base = rand_case(rng, m, k, T, 1, True)
    up, dn = np.float32(2.0 ** 40), np.float32(2.0 ** -40)
    for su, sc in ((up, dn), (dn, up)):
        c = Case(m, k, T, 1, base.U * su, base.C * sc, base.mu, base.sigma, base.X)
        if entry == "expand":
            assert base.expand(L) == 0 and c.expand(L) == 0
            assert torch.equal(c.gXh.iview, base.gXh.iview)
        else:
            assert base.score(L) == 0 and c.score(L) == 0
            for a, b in zip(c.sums(), base.sums()):
                assert np.array_equal(a.view(np.int64), b.view(np.int64))
    if entry == "expand":   # both factors down, no affine step: the result times 2^-80, bit for bit
        b0 = Case(m, k, T, 3, base.U, base.C)
        c = Case(m, k, T, 3, base.U * dn, base.C * dn)
        assert b0.expand(L) == 0 and c.expand(L) == 0
        assert np.array_equal(c.xhat().astype(np.float64), b0.xhat().astype(np.float64) * 2.0 ** -80)
