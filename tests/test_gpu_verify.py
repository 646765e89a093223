"""K16 on the GPU through the ctypes table: dmdx_verify_f32.

Shapes (parity with numpy fp64 of the same fp32 inputs, bounds of tests/verify_ref.py), memory (operands inside
NaN-canary guard zones, exact 0xFF workspaces: tests/memguard.py), values (the identity with K12, the mask as a
selection, exact integers, planted NaN / Inf, power-of-two scaling).  Every operand of every case lives in a
guarded allocation, so each parity case is a memory-edge case as well.
"""
import itertools

import numpy as np
import pytest
import torch

import expand_ref as er
import memguard as mg
import verify_ref as vr
from test_gpu_expand import delay_flat, delay_matrix

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DEV = "cuda"
E_INVALID, E_WORKSPACE = -1000, -1001
NQ = 6

MS = [1, 31, 33, 127, 129, 257]
TS = [1, 15, 33, 65]
LAYOUTS = [0, 1, 2, 3]
WMODES = ["none", "positive", "zeros"]
CLIMS = [False, True]


@pytest.fixture(scope="module")
def L():
    from dmd_era5_amd.kernels import default_kernels

    return default_kernels()._lib


def _ks(L):
    return [1, 15, 16, 17, 64, 65, 129, 225, int(L.dmdx_verify_max_k())]


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Case:
    """Guarded operands of one call.  layout: 0 tight, 1 padded leading dimensions (multiples of 4), 2 odd
    leading dimensions and bases 1 .. 3 elements past a 16-byte boundary, 3 as 1 without mu / sigma (the layouts
    of test_gpu_spread.Case).  col is the (T, 6) and row the (m, 6) column-major matrix of the header."""

    def __init__(self, m, k, T, layout, U, Cm, X, mu=None, sigma=None, w=None, clim=None, delay_ldx=None):
        self.m, self.k, self.T = m, k, T
        pad = {0: 0, 1: 4, 2: 3, 3: 8}[layout]
        off = (lambda j: (1 + j) % 4 if layout == 2 else 0)
        self.U, self.C, self.X, self.mu, self.sigma, self.w, self.clim = U, Cm, X, mu, sigma, w, clim
        vec = (lambda v, j: None if v is None else mg.Guarded(m, 1, m, F32, off(j), DEV).fill(v).snapshot())
        self.gU = mg.Guarded(m, k, m + pad, F32, off(0), DEV).fill(U).snapshot()
        self.gC = mg.Guarded(k, T, k + pad, F32, off(1), DEV).fill(Cm).snapshot()
        self.gmu, self.gsg, self.gw, self.gcl = vec(mu, 2), vec(sigma, 0), vec(w, 1), vec(clim, 2)
        if delay_ldx is None:
            self.gX = mg.Guarded(m, T, m + pad, F32, off(1), DEV).fill(X).snapshot()
        else:   # rows > ldx: X[i, t] = flat[i + t * ldx]
            self.gX = mg.Guarded(m, T, delay_ldx, F32, off(1), DEV)
            self.gX.fbuf[self.gX.start:self.gX.start + self.gX.region] = torch.from_numpy(delay_flat(X, delay_ldx)).to(DEV)
            self.gX.snapshot()
        self.gcol = mg.Guarded(T, NQ, T + pad, F64, 0, DEV)
        self.grow = mg.Guarded(m, NQ, m + pad, F64, 0, DEV)

    def inputs(self):
        return [g for g in (self.gU, self.gC, self.gmu, self.gsg, self.gw, self.gcl, self.gX) if g is not None]

    def check_inputs(self):
        for g in self.inputs():
            g.check_untouched("input")
            g.check_unchanged("input")

    def run(self, L, accumulate=0, rows=True, ws=None, **over):
        need = L.dmdx_verify_workspace_bytes(self.m, self.k, self.T)
        assert need > 0
        self.ws = mg.exact_workspace(need, DEV) if ws is None else ws
        p = (lambda g: None if g is None else g.ptr)
        a = dict(U=self.gU.ptr, m=self.m, k=self.k, ldu=self.gU.ld, C=self.gC.ptr, ldc=self.gC.ld, T=self.T, mu=p(self.gmu),
                 sigma=p(self.gsg), X=self.gX.ptr, ldx=self.gX.ld, w=p(self.gw), clim=p(self.gcl), col=self.gcol.ptr,
                 ldcol=self.gcol.ld, row=self.grow.ptr if rows else None, ldrow=self.grow.ld, wsp=self.ws.ptr,
                 wsb=self.ws.nbytes)
        a.update(over)
        rc = L.dmdx_verify_f32(a["U"], a["m"], a["k"], a["ldu"], a["C"], a["ldc"], a["T"], a["mu"], a["sigma"], a["X"],
                               a["ldx"], a["w"], a["clim"], a["col"], a["ldcol"], a["row"], a["ldrow"], accumulate,
                               a["wsp"], a["wsb"], _stream())
        torch.cuda.synchronize()
        return rc

    def sums(self):
        """-> (col (6, T), row (6, m))"""
        return self.gcol.logical().T.copy(), self.grow.logical().T.copy()

    def args(self):
        return self.U, self.C, self.X, self.mu, self.sigma, self.w, self.clim


def rand_case(rng, m, k, T, layout, wmode="positive", clim=True, delay_ldx=None):
    U = rng.standard_normal((m, k)).astype(np.float32)
    Cm = rng.standard_normal((k, T)).astype(np.float32)
    mu = sigma = None
    if layout != 3:
        mu = (10.0 * rng.standard_normal(m)).astype(np.float32)
        sigma = (0.5 + rng.random(m)).astype(np.float32)
    Xh = er.expand64(U, Cm, mu, sigma)
    if delay_ldx is None:
        X = (Xh + rng.standard_normal((m, T))).astype(np.float32)
    else:
        X = delay_matrix(rng, m, T, delay_ldx)
    w = None
    if wmode != "none":
        w = (0.05 + rng.random(m)).astype(np.float32)
        if wmode == "zeros":
            w[rng.random(m) < 0.25] = 0.0
    cl = None
    if clim:
        cl = ((0.0 if mu is None else mu) + rng.standard_normal(m)).astype(np.float32)
    return Case(m, k, T, layout, U, Cm, X, mu, sigma, w, cl, delay_ldx)


def parity_shapes(L):
    """A pairwise-covering sample of (m, k, T, layout, w mode, clim given), test_gpu_spread.parity_shapes'
    construction: greedily, the combination that covers the most pairs of values not seen together yet, until
    every pair of every two lists has been.  Deterministic, ~60 cases."""
    lists = [MS, _ks(L), TS, LAYOUTS, WMODES, CLIMS]
    n = len(lists)
    pairs = list(itertools.combinations(range(n), 2))
    todo = {(a, x, b, y) for a, b in pairs for x in lists[a] for y in lists[b]}
    cands = list(itertools.product(*lists))
    out = []
    while todo:
        best = max(cands, key=lambda c: sum((a, c[a], b, c[b]) in todo for a, b in pairs))
        todo -= {(a, best[a], b, best[b]) for a, b in pairs}
        out.append(best)
    assert len(out) <= 90
    return out


def check_verify(L, c, rows=True):
    assert c.run(L, rows=rows) == 0, L.dmdx_last_error()
    c.gcol.check_fully_written("col")
    c.gcol.check_untouched("col")
    c.grow.check_untouched("row")
    if rows:
        c.grow.check_fully_written("row")
    else:
        assert bool((c.grow.ibuf == c.grow.canary).all())
    c.ws.check_untouched()
    c.check_inputs()
    want = vr.verify64(*c.args())
    bounds = vr.verify_bounds(*c.args())
    for g, w_, b, name in list(zip(c.sums(), want, bounds, ("col", "row")))[:2 if rows else 1]:
        err = np.abs(g - w_)
        assert (err <= b).all(), (name, c.m, c.k, c.T, [float((err[q] / np.maximum(b[q], 1e-300)).max()) for q in range(NQ)])


def test_parity_over_the_shape_edges(L):
    rng = np.random.default_rng(1601)
    for n, (m, k, T, layout, wmode, clim) in enumerate(parity_shapes(L)):
        check_verify(L, rand_case(rng, m, k, T, layout, wmode, clim), rows=n % 4 != 3)


def test_several_workgroups_and_time_splits(L):
    """1003 rows = 8 row blocks, 300 snapshots = 10 tiles, one per workgroup: the T split, the partial slots of
    several row blocks and both reduce kernels take part."""
    check_verify(L, rand_case(np.random.default_rng(1602), 1003, 37, 300, 2, "zeros", True))


def test_delay_view(L):
    """X with rows > ldx (the zero-copy delay view)."""
    check_verify(L, rand_case(np.random.default_rng(1603), 300, 20, 45, 0, "zeros", True, delay_ldx=100))


def test_accumulate_adds_row_blocks(L):
    """Two row blocks into one col: within the sum of the two bounds of the sum of the two halves; the second
    call's `row` is its own."""
    rng = np.random.default_rng(1604)
    m, k, T, h = 300, 33, 70, 170
    full = rand_case(rng, m, k, T, 2, "zeros", True)
    cut = (lambda v, s: None if v is None else v[s])
    halves = [Case(s.stop - s.start, k, T, 2, full.U[s], full.C, full.X[s], cut(full.mu, s), cut(full.sigma, s),
                   cut(full.w, s), cut(full.clim, s)) for s in (slice(0, h), slice(h, m))]
    a, b = halves
    assert a.run(L) == 0, L.dmdx_last_error()
    first = a.sums()[0]
    assert b.run(L, accumulate=1, col=a.gcol.ptr, ldcol=a.gcol.ld) == 0, L.dmdx_last_error()
    a.gcol.check_untouched("col")
    assert bool((b.gcol.ibuf == b.gcol.canary).all())
    got = a.sums()[0]
    wa, wb = vr.verify64(*a.args()), vr.verify64(*b.args())
    ba, bb = vr.verify_bounds(*a.args()), vr.verify_bounds(*b.args())
    assert (np.abs(first - wa[0]) <= ba[0]).all()
    assert (np.abs(got - (wa[0] + wb[0])) <= ba[0] + bb[0]).all()
    assert (np.abs(b.sums()[1] - wb[1]) <= bb[1]).all()
    # the sum is the fp64 sum of the two calls' own results, bit for bit
    assert b.run(L) == 0
    assert np.array_equal(got, first + b.sums()[0])


# ---------------------------------------------------------------- the identity with K12
@pytest.mark.parametrize("shape", [(200, 50, 45, 2), (1003, 37, 300, 1), (257, 256, 33, 3)])
def test_without_weight_and_clim_it_is_the_k12_score(L, shape):
    """w == NULL, clim == NULL: col[0], col[4] and row[0] are sse_col, ref_col and sse_row of
    dmdx_expand_score_f32 on the same operands, bit for bit (a T split; k = max_k without mu / sigma)."""
    m, k, T, layout = shape
    if k == 256:
        assert k == int(L.dmdx_verify_max_k()) == int(L.dmdx_expand_max_k())
    c = rand_case(np.random.default_rng(1605), m, k, T, layout, "none", False)
    assert c.run(L) == 0, L.dmdx_last_error()
    gs = [mg.Guarded(n, 1, n, F64, 0, DEV) for n in (T, T, m)]
    ws = mg.exact_workspace(L.dmdx_expand_score_workspace_bytes(m, k, T), DEV)
    p = (lambda g: None if g is None else g.ptr)
    rc = L.dmdx_expand_score_f32(c.gU.ptr, m, k, c.gU.ld, c.gC.ptr, c.gC.ld, T, p(c.gmu), p(c.gsg), c.gX.ptr, c.gX.ld,
                                 gs[0].ptr, gs[1].ptr, gs[2].ptr, 0, ws.ptr, ws.nbytes, _stream())
    torch.cuda.synchronize()
    assert rc == 0, L.dmdx_last_error()
    col, row = c.sums()
    for got, g, name in ((col[0], gs[0], "sse_col"), (col[4], gs[1], "ref_col"), (row[0], gs[2], "sse_row")):
        assert np.array_equal(got.view(np.int64), g.logical()[:, 0].view(np.int64)), name


# ---------------------------------------------------------------- the mask
def _row0_finite32(U, Cm, X, mu, sigma):
    """Where numpy's row[0] is finite when the squares are formed in fp32, as the kernel forms them (1e38 squared
    is finite in fp64 and is not in fp32)."""
    with np.errstate(all="ignore"):
        e = (er.expand64(U, Cm, mu, sigma).astype(np.float32) - X).astype(np.float32)
        return np.isfinite((e * e).astype(np.float64).sum(axis=1))


@pytest.mark.parametrize("which", ["quarter", "row128", "all"])
def test_masked_rows_are_selected_out(L, which):
    """NaN, +Inf and 1e38 in the rows with w == 0 of X, U, mu, sigma and clim: every column sum keeps the bits of the
    run with ordinary values there.  "row128": m = 129 and the only masked row is the single row of the second
    workgroup; "all": every weight 0, the column sums are +0.0."""
    rng = np.random.default_rng(1606)
    m, k, T = (150, 37, 70) if which == "quarter" else (129, 20, 40)
    base = rand_case(rng, m, k, T, 2, "zeros", True)
    w = base.w.copy()
    if which == "row128":
        w = (0.05 + rng.random(m)).astype(np.float32)
        w[128] = 0.0
    elif which == "all":
        w[:] = 0.0
    masked = np.nonzero(w == 0)[0]
    assert len(masked) >= 1
    base = Case(m, k, T, 2, base.U, base.C, base.X, base.mu, base.sigma, w, base.clim)
    assert base.run(L) == 0, L.dmdx_last_error()
    col0, row0 = base.sums()
    assert np.isfinite(col0).all() and np.isfinite(row0).all()
    if which == "all":
        assert np.array_equal(col0.view(np.int64), np.zeros_like(col0).view(np.int64))      # +0.0, not -0.0
    vals = np.array([np.nan, np.inf, 1e38], dtype=np.float32)
    with np.errstate(all="ignore"):
        for what in ("X", "U", "mu", "sigma", "clim"):
            ops = dict(U=base.U.copy(), X=base.X.copy(), mu=base.mu.copy(), sigma=base.sigma.copy(), clim=base.clim.copy())
            for n, i in enumerate(masked):
                v = vals[n % 3]
                if what in ("X", "U"):
                    ops[what][i, (3 * n) % ops[what].shape[1]] = v
                else:
                    ops[what][i] = v
            c = Case(m, k, T, 2, ops["U"], base.C, ops["X"], ops["mu"], ops["sigma"], w, ops["clim"])
            assert c.run(L) == 0, L.dmdx_last_error()
            col, row = c.sums()
            assert np.array_equal(col.view(np.int64), col0.view(np.int64)), what
            fin = _row0_finite32(ops["U"], base.C, ops["X"], ops["mu"], ops["sigma"])
            assert np.array_equal(np.isfinite(row[0]), fin), what
            if what != "clim":
                assert not fin[masked].any()
            keep = np.ones(m, dtype=bool)
            keep[masked] = False
            assert np.array_equal(row[:, keep].view(np.int64), row0[:, keep].view(np.int64)), what
            c.ws.check_untouched()


# ---------------------------------------------------------------- NaN / Inf where they count
def _cls(a):
    a = np.asarray(a, dtype=np.float64)
    return np.where(np.isnan(a), 3, np.where(np.isposinf(a), 1, np.where(np.isneginf(a), 2, 0)))


PLANTS = [("X", np.nan), ("X", np.inf), ("X", -np.inf), ("U", np.nan), ("U", np.inf), ("U_last", -np.inf), ("C", np.nan),
          ("C", -np.inf), ("mu", np.inf), ("mu", np.nan), ("sigma", np.nan), ("clim", np.nan), ("clim", np.inf)]


def test_planted_nan_and_inf(L):
    """In a row that is NOT masked.  k = 37 is no multiple of the 16-column granule; "U_last" plants in the last
    real column of U, next to the zero pad.  Class of every sum = numpy fp64's; sums the element does not take
    part in keep the bits of the clean run."""
    rng = np.random.default_rng(1607)
    m, k, T = 150, 37, 70
    i0, j0, t0 = 77, 11, 41
    base = rand_case(rng, m, k, T, 2, "zeros", True)
    w = base.w.copy()
    w[i0] = 0.5
    base = Case(m, k, T, 2, base.U, base.C, base.X, base.mu, base.sigma, w, base.clim)
    assert base.run(L) == 0, L.dmdx_last_error()
    clean = base.sums()
    with np.errstate(all="ignore"):
        for what, val in PLANTS:
            o = dict(U=base.U.copy(), C=base.C.copy(), X=base.X.copy(), mu=base.mu.copy(), sigma=base.sigma.copy(),
                     clim=base.clim.copy())
            if what == "U":
                o["U"][i0, j0] = val
            elif what == "U_last":
                o["U"][i0, k - 1] = val
            elif what == "C":
                o["C"][j0, t0] = val
            elif what == "X":
                o["X"][i0, t0] = val
            else:
                o[what][i0] = val
            c = Case(m, k, T, 2, o["U"], o["C"], o["X"], o["mu"], o["sigma"], w, o["clim"])
            assert c.run(L) == 0, L.dmdx_last_error()
            want = vr.verify64(*c.args())
            hit = 0
            for n, (g, cl, w_) in enumerate(zip(c.sums(), clean, want)):
                assert np.array_equal(_cls(g) != 0, _cls(w_) != 0), (what, val, n)
                assert np.array_equal(_cls(g)[_cls(g) != 3], _cls(w_)[_cls(g) != 3]), (what, val, n)
                fin = _cls(w_) == 0
                hit += int((~fin).sum())
                assert np.array_equal(g.view(np.int64)[fin], cl.view(np.int64)[fin]), (what, val, n)
            assert hit > 0
            if what == "X":      # exactly column t0 and row i0 of the sums x enters (all but f^2)
                assert hit == 5 + 5
            if what == "clim":   # e^2 and e do not see the climatology
                assert hit == 4 * T + 4


# ---------------------------------------------------------------- exact integers
def int_case(rng, m, k, T, layout):
    """Integer U in [-2, 2], C in [-3, 3], mu, clim, sigma in {1, 2, 4}, X = Xhat + d with d in [-3, 3], w in
    {1, 2, 4}: every quantity and every partial sum of every order an integer below 2^24."""
    U = rng.integers(-2, 3, (m, k)).astype(np.float32)
    Cm = rng.integers(-3, 4, (k, T)).astype(np.float32)
    mu = rng.integers(-50, 51, m).astype(np.float32)
    sigma = rng.choice([1.0, 2.0, 4.0], m).astype(np.float32)
    clim = (mu + rng.integers(-9, 10, m)).astype(np.float32)
    w = rng.choice([1.0, 2.0, 4.0], m).astype(np.float32)
    Xh = er.expand64(U, Cm, mu, sigma)
    assert np.array_equal(Xh, np.rint(Xh)) and np.abs(Xh).max() < 2 ** 24
    X = (Xh + rng.integers(-3, 4, (m, T))).astype(np.float32)
    c = Case(m, k, T, layout, U, Cm, X, mu, sigma, w, clim)
    xh, x, cl = Xh.astype(np.int64), X.astype(np.int64), clim.astype(np.int64)[:, None]
    e, f, a = xh - x, xh - cl, x - cl
    Q = np.stack([e * e, e, a, f * f, a * a, f * a])
    WQ = Q * w.astype(np.int64)[None, :, None]
    assert np.abs(WQ).max() < 2 ** 24
    # the fp32 part of the column sums runs over the 128 rows of a workgroup, of the row sums over a 32-column tile
    assert np.add.reduceat(np.abs(WQ), np.arange(0, m, vr.FP32_ROWS), axis=1).max() < 2 ** 24
    assert np.add.reduceat(np.abs(Q), np.arange(0, T, 32), axis=2).max() < 2 ** 24
    c.want = (WQ.sum(axis=1).astype(np.float64), Q.sum(axis=2).astype(np.float64))
    return c


@pytest.mark.parametrize("shape", [(131, 17, 77, 2), (1003, 50, 300, 1), (5000, 7, 33, 0), (40000, 7, 470, 1)])
def test_exact_integers(L, shape):
    """The last shape is the smallest round one at which a workgroup walks three tiles (313 row blocks -> 5 T splits
    of 15 tiles, the last partial): the prefetch, the other LDS stage and the reuse of a slot parity all run."""
    c = int_case(np.random.default_rng(1608), *shape)
    assert c.run(L) == 0, L.dmdx_last_error()
    col, row = c.sums()
    for q in range(NQ):
        assert np.array_equal(col[q], c.want[0][q]), ("col", q)
        assert np.array_equal(row[q], c.want[1][q]), ("row", q)
    c.ws.check_untouched()


# ---------------------------------------------------------------- scaling, reproducibility
def test_power_of_two_scalings(L):
    """(2^e U, 2^-e C) changes no bit; 2^e w multiplies the column sums by exactly 2^e and leaves `row` alone."""
    rng = np.random.default_rng(1609)
    m, k, T = 200, 50, 45
    base = rand_case(rng, m, k, T, 1, "zeros", True)
    assert base.run(L) == 0, L.dmdx_last_error()
    col0, row0 = base.sums()
    up, dn = np.float32(2.0 ** 40), np.float32(2.0 ** -40)
    for su, sc in ((up, dn), (dn, up)):
        c = Case(m, k, T, 1, base.U * su, base.C * sc, base.X, base.mu, base.sigma, base.w, base.clim)
        assert c.run(L) == 0
        for a, b in zip(c.sums(), (col0, row0)):
            assert np.array_equal(a.view(np.int64), b.view(np.int64))
    for e in (5, -3):
        c = Case(m, k, T, 1, base.U, base.C, base.X, base.mu, base.sigma, base.w * np.float32(2.0 ** e), base.clim)
        assert c.run(L) == 0
        col, row = c.sums()
        assert np.array_equal(col, col0 * 2.0 ** e)
        assert np.array_equal(row.view(np.int64), row0.view(np.int64))


def test_two_calls_give_the_same_bits(L):
    c = rand_case(np.random.default_rng(1610), 1003, 50, 131, 2, "zeros", True)
    assert c.run(L) == 0, L.dmdx_last_error()
    firsts = [g.iview.clone() for g in (c.gcol, c.grow)]
    for g in (c.gcol, c.grow):
        g.ibuf.fill_(g.canary)
    assert c.run(L) == 0
    for g, f in zip((c.gcol, c.grow), firsts):
        assert torch.equal(g.iview, f)
        g.check_untouched()


# ---------------------------------------------------------------- refusals
def test_refused_calls_write_nothing(L):
    c = rand_case(np.random.default_rng(1611), 70, 9, 40, 1, "zeros", True)
    kmax = int(L.dmdx_verify_max_k())
    assert kmax == 256
    big = 2 ** 31
    ws = mg.exact_workspace(L.dmdx_verify_workspace_bytes(c.m, c.k, c.T), DEV)
    bad = [dict(k=0), dict(k=kmax + 1), dict(ldcol=c.T - 1), dict(ldrow=c.m - 1), dict(U=None), dict(C=None), dict(X=None),
           dict(col=None), dict(m=0), dict(T=0), dict(m=-1), dict(ldu=c.m - 1), dict(ldc=c.k - 1), dict(ldx=0), dict(ldx=big),
           dict(ldu=big), dict(ldc=big), dict(ldcol=big), dict(ldrow=big), dict(m=big, ldu=big), dict(T=big, ldcol=big)]
    for over in bad:
        assert c.run(L, ws=ws, **over) == E_INVALID, over
        assert L.dmdx_last_error()
    assert c.run(L, ws=ws, wsb=ws.nbytes - 1) == E_WORKSPACE
    assert L.dmdx_last_error()
    assert c.run(L, ws=ws, wsp=None) == E_WORKSPACE
    ws.check_unused()
    ws.check_untouched()
    for g in (c.gcol, c.grow):
        assert bool((g.ibuf == g.canary).all())
    c.check_inputs()
    # ldrow is not looked at without row
    assert c.run(L, rows=False, ldrow=0) == 0, L.dmdx_last_error()
