"""K19 on the GPU through the ctypes table: dmdx_crps_f32.

Shapes (parity with numpy fp64 of the same fp32 inputs, bounds of tests/crps_ref.py), memory (operands inside
NaN-canary guard zones, exact 0xFF workspaces: tests/memguard.py), values (the rank histogram as exact integers
against the fields of dmdx_expand_f32, identical and permuted members, exact integers, the mask as a selection,
planted NaN / Inf, power-of-two scaling).  Every operand of every case lives in a guarded allocation, so each parity
case is a memory-edge case as well.
"""
import itertools

import numpy as np
import pytest
import torch

import crps_ref as cr
import expand_ref as er
import memguard as mg
from test_gpu_expand import delay_flat, delay_matrix

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DEV = "cuda"
E_INVALID, E_WORKSPACE = -1000, -1001
NQ = 2
HB = cr.MEMBER_BLOCK

MS = [1, 31, 33, 127, 129, 257]
TS = [1, 15, 33, 65]
# one below, at and above every boundary of the member blocks (8 above k = 128, 16 up to it) that the largest B of the
# list reaches: 8, 16 and 32 are boundaries of the first, 16 and 32 of the second
BS = [1, 2, 3, HB - 1, HB, HB + 1, 2 * HB - 1, 2 * HB, 2 * HB + 1, 4 * HB - 1, 4 * HB, 33]
LAYOUTS = [0, 1, 2, 3]
WMODES = ["none", "positive", "zeros"]
HCANARY = 0x7EADBEEF7EADBEEF
HGUARD = 4096


@pytest.fixture(scope="module")
def L():
    from dmd_era5_amd.kernels import default_kernels

    return default_kernels()._lib


def _ks(L):
    return [1, 15, 16, 17, 64, 65, 129, 225, int(L.dmdx_crps_max_k())]


def _stream():
    return torch.cuda.current_stream().cuda_stream


class GuardedHist:
    """B + 1 int64 counts between two guard zones of a fixed bit pattern (memguard.Guarded holds floats only)."""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((2 * HGUARD + n,), HCANARY, dtype=torch.int64, device=DEV)

    @property
    def ptr(self):
        return self.buf.data_ptr() + 8 * HGUARD

    def counts(self):
        return self.buf[HGUARD:HGUARD + self.n].cpu().numpy().copy()

    def check_untouched(self):
        assert bool((self.buf[:HGUARD] == HCANARY).all()) and bool((self.buf[HGUARD + self.n:] == HCANARY).all()), "hist guard"

    def check_fully_written(self):
        assert not bool((self.buf[HGUARD:HGUARD + self.n] == HCANARY).any()), "hist not fully written"

    def check_unwritten(self):
        assert bool((self.buf == HCANARY).all()), "hist written"


class Case:
    """Guarded operands of one call.  layout: 0 tight, 1 padded leading dimensions (multiples of 4), 2 odd
    leading dimensions and bases 1 .. 3 elements past a 16-byte boundary, 3 as 1 without mu / sigma (the layouts
    of test_gpu_verify.Case).  C is the k x (B T) matrix of the header; col is the (T, 2) and row the (m, 2)
    column-major matrix."""

    def __init__(self, m, k, T, B, layout, U, Cm, X, mu=None, sigma=None, w=None, delay_ldx=None):
        self.m, self.k, self.T, self.B, self.layout = m, k, T, B, layout
        pad = {0: 0, 1: 4, 2: 3, 3: 8}[layout]
        off = (lambda j: (1 + j) % 4 if layout == 2 else 0)
        self.U, self.C, self.X, self.mu, self.sigma, self.w = U, Cm, X, mu, sigma, w
        vec = (lambda v, j: None if v is None else mg.Guarded(m, 1, m, F32, off(j), DEV).fill(v).snapshot())
        self.gU = mg.Guarded(m, k, m + pad, F32, off(0), DEV).fill(U).snapshot()
        self.gC = mg.Guarded(k, B * T, k + pad, F32, off(1), DEV).fill(Cm).snapshot()
        self.gmu, self.gsg, self.gw = vec(mu, 2), vec(sigma, 0), vec(w, 1)
        if delay_ldx is None:
            self.gX = mg.Guarded(m, T, m + pad, F32, off(1), DEV).fill(X).snapshot()
        else:   # rows > ldx: X[i, t] = flat[i + t * ldx]
            self.gX = mg.Guarded(m, T, delay_ldx, F32, off(1), DEV)
            self.gX.fbuf[self.gX.start:self.gX.start + self.gX.region] = torch.from_numpy(delay_flat(X, delay_ldx)).to(DEV)
            self.gX.snapshot()
        self.gcol = mg.Guarded(T, NQ, T + pad, F64, 0, DEV)
        self.grow = mg.Guarded(m, NQ, m + pad, F64, 0, DEV)
        self.ghist = GuardedHist(B + 1)

    def inputs(self):
        return [g for g in (self.gU, self.gC, self.gmu, self.gsg, self.gw, self.gX) if g is not None]

    def check_inputs(self):
        for g in self.inputs():
            g.check_untouched("input")
            g.check_unchanged("input")

    def run(self, L, accumulate=0, rows=True, hist=True, ws=None, **over):
        need = L.dmdx_crps_workspace_bytes(self.m, self.k, self.T, self.B)
        assert need > 0
        self.ws = mg.exact_workspace(need, DEV) if ws is None else ws
        p = (lambda g: None if g is None else g.ptr)
        a = dict(U=self.gU.ptr, m=self.m, k=self.k, ldu=self.gU.ld, C=self.gC.ptr, ldc=self.gC.ld, T=self.T, B=self.B,
                 mu=p(self.gmu), sigma=p(self.gsg), X=self.gX.ptr, ldx=self.gX.ld, w=p(self.gw), col=self.gcol.ptr,
                 ldcol=self.gcol.ld, row=self.grow.ptr if rows else None, ldrow=self.grow.ld,
                 histp=self.ghist.ptr if hist else None, wsp=self.ws.ptr, wsb=self.ws.nbytes)
        a.update(over)
        rc = L.dmdx_crps_f32(a["U"], a["m"], a["k"], a["ldu"], a["C"], a["ldc"], a["T"], a["B"], a["mu"], a["sigma"],
                             a["X"], a["ldx"], a["w"], a["col"], a["ldcol"], a["row"], a["ldrow"], a["histp"], accumulate,
                             a["wsp"], a["wsb"], _stream())
        torch.cuda.synchronize()
        return rc

    def sums(self):
        """-> (col (2, T), row (2, m))"""
        return self.gcol.logical().T.copy(), self.grow.logical().T.copy()

    def hist(self):
        return self.ghist.counts()

    def args(self):
        return self.U, self.C, self.T, self.B, self.X, self.mu, self.sigma, self.w

    def with_(self, **kw):
        o = dict(U=self.U, Cm=self.C, X=self.X, mu=self.mu, sigma=self.sigma, w=self.w)
        o.update(kw)
        return Case(self.m, self.k, self.T, self.B, self.layout, **o)

    def fields(self, L):
        """The B member fields as dmdx_expand_f32 gives them for C_b: (B, m, T) fp32."""
        out = np.empty((self.B, self.m, self.T), dtype=np.float32)
        p = (lambda g: None if g is None else g.ptr)
        g = mg.Guarded(self.m, self.T, self.m, F32, 0, DEV)
        for b in range(self.B):
            rc = L.dmdx_expand_f32(self.gU.ptr, self.m, self.k, self.gU.ld, self.gC.col_ptr(b * self.T), self.gC.ld, self.T,
                                   p(self.gmu), p(self.gsg), g.ptr, g.ld, _stream())
            torch.cuda.synchronize()
            assert rc == 0, L.dmdx_last_error()
            out[b] = g.logical()
        return out


def rand_ops(rng, m, k, T, B, layout, wmode="positive", delay_ldx=None):
    """Members around a common model, the analysis inside their range more often than not."""
    U = rng.standard_normal((m, k)).astype(np.float32)
    Cm = (np.tile(rng.standard_normal((k, T)), (1, B)) + 0.3 * rng.standard_normal((k, B * T))).astype(np.float32)
    mu = sigma = None
    if layout != 3:
        mu = (10.0 * rng.standard_normal(m)).astype(np.float32)
        sigma = (0.5 + rng.random(m)).astype(np.float32)
    if delay_ldx is None:
        b0 = int(rng.integers(B))
        X = (er.expand64(U, Cm[:, b0 * T:(b0 + 1) * T], mu, sigma) + 0.5 * rng.standard_normal((m, T))).astype(np.float32)
    else:
        X = delay_matrix(rng, m, T, delay_ldx)
    w = None
    if wmode != "none":
        w = (0.05 + rng.random(m)).astype(np.float32)
        if wmode == "zeros":
            w[rng.random(m) < 0.25] = 0.0
    return dict(U=U, Cm=Cm, X=X, mu=mu, sigma=sigma, w=w)


def rand_case(rng, m, k, T, B, layout, wmode="positive", delay_ldx=None):
    return Case(m, k, T, B, layout, delay_ldx=delay_ldx, **rand_ops(rng, m, k, T, B, layout, wmode, delay_ldx))


def parity_shapes(L):
    """A pairwise-covering sample of (m, k, T, B, layout, w mode), test_gpu_verify.parity_shapes' construction."""
    lists = [MS, _ks(L), TS, BS, LAYOUTS, WMODES]
    n = len(lists)
    pairs = list(itertools.combinations(range(n), 2))
    todo = {(a, x, b, y) for a, b in pairs for x in lists[a] for y in lists[b]}
    cands = list(itertools.product(*lists))
    out = []
    while todo:
        best = max(cands, key=lambda c: sum((a, c[a], b, c[b]) in todo for a, b in pairs))
        todo -= {(a, best[a], b, best[b]) for a, b in pairs}
        out.append(best)
    assert len(out) <= 140
    return out


def n_selected(c):
    """The number of elements that enter a bin: rows with w != 0, X and the members finite."""
    rows = c.m if c.w is None else int((c.w != 0).sum())
    return rows * c.T


def check_crps(L, c, rows=True, hist=True):
    assert c.run(L, rows=rows, hist=hist) == 0, L.dmdx_last_error()
    c.gcol.check_fully_written("col")
    c.gcol.check_untouched("col")
    c.grow.check_untouched("row")
    c.ghist.check_untouched()
    if rows:
        c.grow.check_fully_written("row")
    else:
        assert bool((c.grow.ibuf == c.grow.canary).all())
    if hist:
        c.ghist.check_fully_written()
    else:
        c.ghist.check_unwritten()
    c.ws.check_untouched()
    c.check_inputs()
    want = cr.crps64(*c.args())
    bounds = cr.crps_bounds(*c.args())
    for g, w_, b, name in list(zip(c.sums(), want, bounds, ("col", "row")))[:2 if rows else 1]:
        err = np.abs(g - w_)
        assert (err <= b).all(), (name, c.m, c.k, c.T, c.B, [float((err[q] / np.maximum(b[q], 1e-300)).max()) for q in range(NQ)])
        assert (g >= 0).all() and not np.signbit(g).any()
    if hist:
        h = c.hist()
        assert (h >= 0).all() and h.sum() == n_selected(c) == want[2].sum()
        # the fp64 ranks differ from the fp32 ones only where a member is within its error of the analysis: such an
        # element may sit in another bin (the exact counts are test_rank_histogram_is_exact's)
        P = cr.members64(c.U, c.C, c.T, c.B, c.mu, c.sigma)
        d = np.stack([er.element_bound(c.U, c.C[:, b * c.T:(b + 1) * c.T], c.mu, c.sigma) for b in range(c.B)])
        near = (np.abs(P - c.X.astype(np.float64)[None]) <= d).any(axis=0)
        if c.w is not None:
            near &= (c.w != 0)[:, None]
        assert np.abs(h - want[2]).sum() <= 2 * int(near.sum())


def test_parity_over_the_shape_edges(L):
    rng = np.random.default_rng(1901)
    assert int(L.dmdx_crps_max_members()) == cr.MAX_B >= 256 and int(L.dmdx_crps_max_k()) == 256
    for n, (m, k, T, B, layout, wmode) in enumerate(parity_shapes(L)):
        check_crps(L, rand_case(rng, m, k, T, B, layout, wmode), rows=n % 4 != 3, hist=n % 3 != 2)


def test_several_workgroups_and_time_splits(L):
    """1003 rows = 8 row blocks, 300 snapshots = 10 tiles, one per workgroup: the T split, the partial slots of
    several row blocks and the three reduce kernels take part."""
    check_crps(L, rand_case(np.random.default_rng(1902), 1003, 37, 300, 9, 2, "zeros"))


def test_delay_view(L):
    """X with rows > ldx (the zero-copy delay view)."""
    check_crps(L, rand_case(np.random.default_rng(1903), 300, 20, 45, 5, 0, "zeros", delay_ldx=100))


def test_the_largest_ensemble(L):
    """B = DMDX_CRPS_MAX_B: 32 member blocks, the last bin is bin 256 (the second bin of thread 0)."""
    rng = np.random.default_rng(1904)
    c = rand_case(rng, 70, 9, 33, cr.MAX_B, 1, "zeros")
    c = c.with_(X=(c.X + 40.0 * (rng.random(c.X.shape) < 0.1)).astype(np.float32))     # some analyses above every member
    check_crps(L, c)
    assert c.hist()[cr.MAX_B] > 0


def test_accumulate_adds_row_blocks(L):
    """Two row blocks into one col and one hist; the second call's `row` is its own."""
    rng = np.random.default_rng(1905)
    m, k, T, B, h = 300, 33, 70, 9, 170
    full = rand_case(rng, m, k, T, B, 2, "zeros")
    cut = (lambda v, s: None if v is None else v[s])
    halves = [Case(s.stop - s.start, k, T, B, 2, full.U[s], full.C, full.X[s], cut(full.mu, s), cut(full.sigma, s),
                   cut(full.w, s)) for s in (slice(0, h), slice(h, m))]
    a, b = halves
    assert a.run(L) == 0, L.dmdx_last_error()
    first, hfirst = a.sums()[0], a.hist()
    assert b.run(L, accumulate=1, col=a.gcol.ptr, ldcol=a.gcol.ld, histp=a.ghist.ptr) == 0, L.dmdx_last_error()
    a.gcol.check_untouched("col")
    a.ghist.check_untouched()
    assert bool((b.gcol.ibuf == b.gcol.canary).all())
    b.ghist.check_unwritten()
    got, hgot = a.sums()[0], a.hist()
    wa, wb = cr.crps64(*a.args()), cr.crps64(*b.args())
    ba, bb = cr.crps_bounds(*a.args()), cr.crps_bounds(*b.args())
    assert (np.abs(first - wa[0]) <= ba[0]).all()
    assert (np.abs(got - (wa[0] + wb[0])) <= ba[0] + bb[0]).all()
    assert (np.abs(b.sums()[1] - wb[1]) <= bb[1]).all()
    # the sums are the fp64 sum and the integer sum of the two calls' own results, bit for bit
    assert b.run(L) == 0
    assert np.array_equal(got, first + b.sums()[0])
    assert np.array_equal(hgot, hfirst + b.hist())
    assert hgot.sum() == n_selected(a) + n_selected(b)


# ---------------------------------------------------------------- the rank histogram, exactly
@pytest.mark.parametrize("B", [5, 33])
@pytest.mark.parametrize("shape", [(200, 50, 45, 2), (1003, 37, 300, 1), (257, 256, 33, 3)])
def test_rank_histogram_is_exact(L, shape, B):
    """hist == the counts of (field_b < X).sum(b) with field_b from dmdx_expand_f32, as integers; X is a member's
    field, bit for bit, on a tenth of the elements (exact ties: "not below"), NaN on a few, and some rows are
    masked."""
    m, k, T, layout = shape
    rng = np.random.default_rng(1906)
    c = rand_case(rng, m, k, T, B, layout, "zeros")
    F = c.fields(L)
    X = c.X.copy()
    tie = rng.random((m, T)) < 0.1
    pick = rng.integers(0, B, (m, T))
    X[tie] = np.take_along_axis(F, pick[None], axis=0)[0][tie]
    nan = rng.random((m, T)) < 0.01
    X[nan] = np.nan
    c = c.with_(X=X)
    assert c.run(L) == 0, L.dmdx_last_error()
    with np.errstate(all="ignore"):
        rank = (F < X[None]).sum(axis=0)
    live = (c.w != 0)[:, None] & ~nan
    assert tie[live].sum() > 10 and nan[(c.w != 0)].sum() >= 1
    want = np.bincount(rank[live], minlength=B + 1)
    got = c.hist()
    assert np.array_equal(got, want)
    assert got.sum() == live.sum()
    c.ghist.check_untouched()
    c.ws.check_untouched()
    # the tie convention is visible: counting ties as "below" gives another histogram
    with np.errstate(all="ignore"):
        assert not np.array_equal(np.bincount((F <= X[None]).sum(axis=0)[live], minlength=B + 1), want)


# ---------------------------------------------------------------- member identities
def int_ops(rng, m, k, T, B, identical=False):
    """Integer U in [-2, 2], C_b = C_0 + d_b with C_0 in [-3, 3] and d_b in [-1, 1], mu, sigma in {1, 2, 4},
    X = x_0 + d with d in [-3, 3], w in {1, 2, 4}: every quantity and every partial sum an integer below 2^24."""
    U = rng.integers(-2, 3, (m, k)).astype(np.float32)
    C0 = rng.integers(-3, 4, (k, T))
    Cm = np.concatenate([C0 + (0 if identical or b == 0 else rng.integers(-1, 2, (k, T))) for b in range(B)], axis=1)
    Cm = Cm.astype(np.float32)
    mu = rng.integers(-50, 51, m).astype(np.float32)
    sigma = rng.choice([1.0, 2.0, 4.0], m).astype(np.float32)
    w = rng.choice([1.0, 2.0, 4.0], m).astype(np.float32)
    X = (er.expand64(U, Cm[:, :T], mu, sigma) + rng.integers(-3, 4, (m, T))).astype(np.float32)
    return dict(U=U, Cm=Cm, X=X, mu=mu, sigma=sigma, w=w)


def int_case(rng, m, k, T, B, layout, identical=False):
    c = Case(m, k, T, B, layout, **int_ops(rng, m, k, T, B, identical))
    P = cr.members64(c.U, c.C, T, B, c.mu, c.sigma)
    assert np.array_equal(P, np.rint(P)) and np.abs(P).max() < 2 ** 24
    absq, pair, rank = cr.quantities64(P, c.X)
    Q = np.stack([absq, pair]).astype(np.int64)
    WQ = Q * c.w.astype(np.int64)[None, :, None]
    # the fp32 part of the column sums runs over the 128 rows of a workgroup, of the row sums over a 32-column tile
    assert np.add.reduceat(WQ, np.arange(0, m, cr.FP32_ROWS), axis=1).max() < 2 ** 24
    assert np.add.reduceat(Q, np.arange(0, T, 32), axis=2).max() < 2 ** 24
    c.want = (WQ.sum(axis=1).astype(np.float64), Q.sum(axis=2).astype(np.float64), np.bincount(rank.ravel(), minlength=B + 1))
    return c


@pytest.mark.parametrize("B", [3, 9])
@pytest.mark.parametrize("shape", [(131, 17, 77, 2), (1003, 50, 300, 1), (5000, 7, 33, 0)])
def test_exact_integers(L, shape, B):
    c = int_case(np.random.default_rng(1907), *shape[:3], B, shape[3])
    assert c.run(L) == 0, L.dmdx_last_error()
    col, row = c.sums()
    for q in range(NQ):
        assert np.array_equal(col[q], c.want[0][q]), ("col", q)
        assert np.array_equal(row[q], c.want[1][q]), ("row", q)
    assert np.array_equal(c.hist(), c.want[2])
    c.ws.check_untouched()


@pytest.mark.parametrize("B", [2, HB, HB + 1, 2 * HB, 2 * HB + 1, 19])
def test_identical_members(L, B):
    """pair is +0.0 exactly (bits), abs is B times the one-member result where that is exact (integers), and every
    element has rank 0 or B."""
    rng = np.random.default_rng(1908)
    m, k, T = 200, 17, 45
    c = int_case(rng, m, k, T, B, 2, identical=True)
    one = Case(m, k, T, 1, 2, c.U, c.C[:, :T], c.X, c.mu, c.sigma, c.w)
    assert c.run(L) == 0 and one.run(L) == 0, L.dmdx_last_error()
    (col, row), (col1, row1) = c.sums(), one.sums()
    for a in (col[1], row[1], col1[1], row1[1]):
        assert np.array_equal(a.view(np.int64), np.zeros_like(a).view(np.int64))         # +0.0, not -0.0
    assert np.array_equal(col[0], B * col1[0]) and np.array_equal(row[0], B * row1[0])
    h, h1 = c.hist(), one.hist()
    assert h[0] == h1[0] and h[B] == h1[1] and h.sum() == h[0] + h[B] == m * T
    # and with ordinary numbers: pair stays +0.0
    r = rand_case(rng, 150, 37, 40, 1, 2, "zeros")
    r = Case(150, 37, 40, B, 2, r.U, np.tile(r.C, (1, B)), r.X, r.mu, r.sigma, r.w)
    assert r.run(L) == 0
    for a in (r.sums()[0][1], r.sums()[1][1]):
        assert np.array_equal(a.view(np.int64), np.zeros_like(a).view(np.int64))


def test_a_permutation_of_the_members(L):
    """hist keeps its bits; the sums move within twice the bound (the order of the fp32 chains changes)."""
    rng = np.random.default_rng(1909)
    m, k, T, B = 200, 50, 45, 19
    c = rand_case(rng, m, k, T, B, 1, "zeros")
    perm = rng.permutation(B)
    Cp = np.concatenate([c.C[:, b * T:(b + 1) * T] for b in perm], axis=1)
    d = c.with_(Cm=Cp)
    assert c.run(L) == 0 and d.run(L) == 0, L.dmdx_last_error()
    assert np.array_equal(c.hist(), d.hist())
    for a, b, bound in zip(c.sums(), d.sums(), cr.crps_bounds(*c.args())):
        assert (np.abs(a - b) <= 2.0 * bound).all()
    assert not np.array_equal(c.sums()[0], d.sums()[0])


# ---------------------------------------------------------------- the mask
@pytest.mark.parametrize("which", ["quarter", "row128", "all"])
def test_masked_rows_are_selected_out(L, which):
    """NaN, +Inf and 1e38 in the rows with w == 0 of X, U, mu and sigma: col and hist keep the bits of the run with
    ordinary values there.  "row128": m = 129 and the only masked row is the single row of the second workgroup;
    "all": every weight 0, the column sums are +0.0 and the counts 0."""
    rng = np.random.default_rng(1910)
    m, k, T, B = (150, 37, 70, 9) if which == "quarter" else (129, 20, 40, 5)
    base = rand_case(rng, m, k, T, B, 2, "zeros")
    w = base.w.copy()
    if which == "row128":
        w = (0.05 + rng.random(m)).astype(np.float32)
        w[128] = 0.0
    elif which == "all":
        w[:] = 0.0
    masked = np.nonzero(w == 0)[0]
    assert len(masked) >= 1
    base = base.with_(w=w)
    assert base.run(L) == 0, L.dmdx_last_error()
    (col0, row0), hist0 = base.sums(), base.hist()
    assert np.isfinite(col0).all() and np.isfinite(row0).all() and hist0.sum() == (m - len(masked)) * T
    if which == "all":
        assert np.array_equal(col0.view(np.int64), np.zeros_like(col0).view(np.int64))      # +0.0, not -0.0
        assert not hist0.any()
    vals = np.array([np.nan, np.inf, 1e38], dtype=np.float32)
    keep = np.ones(m, dtype=bool)
    keep[masked] = False
    for what in ("X", "U", "mu", "sigma"):
        ops = dict(U=base.U.copy(), X=base.X.copy(), mu=base.mu.copy(), sigma=base.sigma.copy())
        for n, i in enumerate(masked):
            v = vals[n % 3]
            if what in ("X", "U"):
                ops[what][i, (3 * n) % ops[what].shape[1]] = v
            else:
                ops[what][i] = v
        c = base.with_(**ops)
        assert c.run(L) == 0, L.dmdx_last_error()
        col, row = c.sums()
        assert np.array_equal(col.view(np.int64), col0.view(np.int64)), what
        assert np.array_equal(c.hist(), hist0), what
        assert np.array_equal(row[:, keep].view(np.int64), row0[:, keep].view(np.int64)), what
        nanrows = masked[np.arange(len(masked)) % 3 == 0]                  # a NaN reaches the row's sums in any case
        assert not np.isfinite(row[0][nanrows]).any(), what
        c.ws.check_untouched()


# ---------------------------------------------------------------- NaN / Inf where they count
PLANTS = [("X", np.nan), ("X", np.inf), ("X", -np.inf), ("U", np.nan), ("U", np.inf), ("U_last", -np.inf), ("C", np.nan),
          ("C", -np.inf), ("mu", np.inf), ("mu", np.nan), ("sigma", np.nan)]


def test_planted_nan_and_inf(L):
    """In a row that is NOT masked.  X[i0, t0]: column t0 of both sums and row i0 of both row sums become
    non-finite, nothing else moves a bit, and the element is in no bin.  U[i0, j], mu[i0], sigma[i0]: row i0 and every
    column, T elements leave the bins.  C[j0, b0 T + t0]: column t0 and every row; the selected rows leave."""
    rng = np.random.default_rng(1911)
    m, k, T, B = 150, 37, 70, 9
    i0, j0, t0, b0 = 77, 11, 41, 4
    base = rand_case(rng, m, k, T, B, 2, "zeros")
    w = base.w.copy()
    w[i0] = 0.5
    base = base.with_(w=w)
    assert base.run(L) == 0, L.dmdx_last_error()
    clean, hclean = base.sums(), base.hist()
    F = base.fields(L)
    rank = (F < base.X[None]).sum(axis=0)
    assert np.array_equal(hclean, np.bincount(rank[w != 0].ravel(), minlength=B + 1))
    nsel = int((w != 0).sum())
    for what, val in PLANTS:
        o = dict(U=base.U.copy(), Cm=base.C.copy(), X=base.X.copy(), mu=base.mu.copy(), sigma=base.sigma.copy())
        badcol, badrow = np.zeros(T, dtype=bool), np.zeros(m, dtype=bool)
        if what in ("U", "U_last"):
            o["U"][i0, j0 if what == "U" else k - 1] = val
            badcol[:], badrow[i0], gone = True, True, rank[i0]
        elif what == "C":
            o["Cm"][j0, b0 * T + t0] = val
            badcol[t0], badrow[:], gone = True, True, rank[w != 0, t0]
        elif what == "X":
            o["X"][i0, t0] = val
            badcol[t0], badrow[i0], gone = True, True, rank[i0, t0:t0 + 1]
        else:
            o[what][i0] = val
            badcol[:], badrow[i0], gone = True, True, rank[i0]
        c = base.with_(**o)
        assert c.run(L) == 0, L.dmdx_last_error()
        col, row = c.sums()
        for q in range(NQ):
            assert np.array_equal(~np.isfinite(col[q]), badcol), (what, val, "col", q)
            assert np.array_equal(~np.isfinite(row[q]), badrow), (what, val, "row", q)
            assert np.array_equal(col[q].view(np.int64)[~badcol], clean[0][q].view(np.int64)[~badcol]), (what, val, q)
            assert np.array_equal(row[q].view(np.int64)[~badrow], clean[1][q].view(np.int64)[~badrow]), (what, val, q)
        assert np.array_equal(c.hist(), hclean - np.bincount(gone, minlength=B + 1)), (what, val)
        assert c.hist().sum() == nsel * T - len(gone)


# ---------------------------------------------------------------- scaling, reproducibility
def test_power_of_two_scaling_of_the_factors(L):
    """(2^e U, 2^-e C) changes no bit of any output."""
    rng = np.random.default_rng(1912)
    base = rand_case(rng, 200, 50, 45, 9, 1, "zeros")
    assert base.run(L) == 0, L.dmdx_last_error()
    (col0, row0), h0 = base.sums(), base.hist()
    up, dn = np.float32(2.0 ** 40), np.float32(2.0 ** -40)
    for su, sc in ((up, dn), (dn, up)):
        c = base.with_(U=base.U * su, Cm=base.C * sc)
        assert c.run(L) == 0
        for a, b in zip(c.sums(), (col0, row0)):
            assert np.array_equal(a.view(np.int64), b.view(np.int64))
        assert np.array_equal(c.hist(), h0)


def test_two_calls_give_the_same_bits(L):
    c = rand_case(np.random.default_rng(1913), 1003, 50, 131, 19, 2, "zeros")
    assert c.run(L) == 0, L.dmdx_last_error()
    firsts, h = [g.iview.clone() for g in (c.gcol, c.grow)], c.hist()
    for g in (c.gcol, c.grow):
        g.ibuf.fill_(g.canary)
    c.ghist.buf.fill_(HCANARY)
    assert c.run(L) == 0
    for g, f in zip((c.gcol, c.grow), firsts):
        assert torch.equal(g.iview, f)
        g.check_untouched()
    assert np.array_equal(c.hist(), h)


# ---------------------------------------------------------------- refusals
def test_refused_calls_write_nothing(L):
    c = rand_case(np.random.default_rng(1914), 70, 9, 40, 5, 1, "zeros")
    kmax, bmax = int(L.dmdx_crps_max_k()), int(L.dmdx_crps_max_members())
    big = 2 ** 31
    ws = mg.exact_workspace(L.dmdx_crps_workspace_bytes(c.m, c.k, c.T, c.B), DEV)
    bad = [dict(k=0), dict(k=kmax + 1), dict(B=0), dict(B=-1), dict(B=bmax + 1), dict(ldcol=c.T - 1), dict(ldrow=c.m - 1),
           dict(U=None), dict(C=None), dict(X=None), dict(col=None), dict(m=0), dict(T=0), dict(m=-1), dict(ldu=c.m - 1),
           dict(ldc=c.k - 1), dict(ldx=0), dict(ldx=big), dict(ldu=big), dict(ldc=big), dict(ldcol=big), dict(ldrow=big),
           dict(m=big, ldu=big), dict(T=big, ldcol=big), dict(T=2 ** 30, ldcol=2 ** 30)]
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
    c.ghist.check_unwritten()
    c.check_inputs()
    # the workspace does not depend on whether row and hist are given; ldrow is not looked at without row
    assert c.run(L, rows=False, hist=False, ldrow=0) == 0, L.dmdx_last_error()
    c.ghist.check_unwritten()


# ---------------------------------------------------------------- the provider method
def test_the_provider_method(L):
    """HipKernels.crps: a contiguous Cm whose k = 5 vectors are not on 16-byte boundaries and the pitched image,
    accumulation into out / hist, the per-row sums."""
    from dmd_era5_amd.forecast import _pitched_dev
    from dmd_era5_amd.kernels import default_kernels

    KERN = default_kernels()
    rng = np.random.default_rng(1915)
    m, k, T, B = 333, 5, 41, 7
    o = rand_ops(rng, m, k, T, B, 0, "zeros")
    t = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV))
    Ut, Xt, mu, sd, w = t(o["U"].T), t(o["X"].T), t(o["mu"]), t(o["sigma"]), t(o["w"])
    Cm = t(o["Cm"].T.reshape(B, T, k))
    cols, rows, hist = KERN.crps(Ut, Cm, Xt, mu, sd, w, want_rows=True)
    args = (o["U"], o["Cm"], T, B, o["X"], o["mu"], o["sigma"], o["w"])
    want, bounds = cr.crps64(*args), cr.crps_bounds(*args)
    assert cols.shape == (2, T) and rows.shape == (2, m) and hist.shape == (B + 1,) and hist.dtype == torch.int64
    for g, w_, b in zip((cols, rows), want, bounds):
        assert (np.abs(g.cpu().numpy() - w_) <= b).all()
    assert int(hist.sum()) == int((o["w"] != 0).sum()) * T
    Cp = _pitched_dev(KERN, Cm)
    assert Cp.stride() == (T * 8, 8, 1)
    again, none, h2 = KERN.crps(Ut, Cp, Xt, mu, sd, w, out=cols.clone(), hist=hist.clone())
    assert none is None and torch.equal(again, 2 * cols) and torch.equal(h2, 2 * hist)
    with pytest.raises(Exception):
        KERN.crps(Ut, Cm, Xt, mu, sd, w, out=cols.clone())
    with pytest.raises(Exception):
        KERN.crps(Ut, t(np.zeros((B, T, k + 1), dtype=np.float32)), Xt)
