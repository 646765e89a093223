"""K24 on the GPU through the ctypes table: dmdx_exceed_prob_f32 and dmdx_exceed_score_f32.

The member fields come from dmdx_expand_f32, member by member; tests/exceed_ref.py forms from them, in the kernel's
own fp32 operations, what the kernel must give: the probability planes and the counts EXACTLY, the sums within the
summation bound.  Every operand, output and workspace of every case lives in a guarded allocation (tests/memguard.py),
so each parity case is a memory-edge case as well.

Random inputs: K19's rand_ops, thresholds thr_j[i, s] = mu_i + z_j sigma_i sqrt(k) (1 + 0.1 N(0, 1)) with
z = (-1, 0, 0.5, 1.2816).  A draw is kept only if the REFERENCE says it can tell a kernel that always answers 0 or B
apart: both outcomes occur, and for B >= 5, k >= 16 every threshold has >= 10 % of its elements with 0 < c < B and an
observed rate within 5 .. 95 % (make_case asserts it on the reference alone).  Two departures from a plain assertion
on every case, both forced by the shape list: the rates are asked of cases with at least 20 elements (m = T = 1 is in
the list, and a rate of 5 % cannot be told from 0 with fewer), and make_case redraws -- at most 40 times, then it
fails -- until the reference is satisfied, since a case of a few elements shows one outcome only in many draws.
"""
import itertools

import numpy as np
import pytest
import torch

import exceed_ref as xr
import memguard as mg
from test_gpu_crps import rand_ops as member_ops
from test_gpu_expand import delay_flat

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DEV = "cuda"
E_INVALID, E_WORKSPACE = -1000, -1001
NQ = xr.NQ
Z = (-1.0, 0.0, 0.5, 1.2816)

MS = [1, 127, 128, 129, 1003]
KS = [1, 16, 17, 50, 256]
TS = [1, 31, 32, 33, 300]
BS = [1, 2, 5, 33, 256]
JS = [1, 2, 3, 4]
SS = [1, 3]
LAYOUTS = [0, 1, 2, 3]
WMODES = ["none", "positive", "zeros"]
ABOVE = [True, False]
ICANARY = 0x7EADBEEF7EADBEEF
IGUARD = 4096


@pytest.fixture(scope="module")
def L():
    from dmd_era5_amd.kernels import default_kernels

    return default_kernels()._lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


class GuardedCounts:
    """n int64 counts between two guard zones of a fixed bit pattern (memguard.Guarded holds floats only)."""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((2 * IGUARD + n,), ICANARY, dtype=torch.int64, device=DEV)

    @property
    def ptr(self):
        return self.buf.data_ptr() + 8 * IGUARD

    def counts(self):
        return self.buf[IGUARD:IGUARD + self.n].cpu().numpy().copy()

    def check_untouched(self):
        assert bool((self.buf[:IGUARD] == ICANARY).all()) and bool((self.buf[IGUARD + self.n:] == ICANARY).all()), "cnt guard"

    def check_fully_written(self):
        assert not bool((self.buf[IGUARD:IGUARD + self.n] == ICANARY).any()), "cnt not fully written"

    def check_unwritten(self):
        assert bool((self.buf == ICANARY).all()), "cnt written"


class Case:
    """Guarded operands of one call.  layout: 0 tight, 1 padded leading dimensions (multiples of 4), 2 odd leading
    dimensions and bases 1 .. 3 elements past a 16-byte boundary, 3 as 1 without mu / sigma (the layouts of
    test_gpu_crps.Case).  thr is the m x (J S) matrix of the header, slot the T labels (None: a null pointer, S = 1
    only); col is the (T, 4 J) and row the (m, 4 J) column-major matrix, P the J planes as one m x (J T) matrix."""

    def __init__(self, m, k, T, B, J, S, layout, above, U, Cm, X, thr, slot=None, mu=None, sigma=None, w=None, delay_ldx=None):
        self.m, self.k, self.T, self.B, self.J, self.S, self.layout, self.above = m, k, T, B, J, S, layout, above
        pad = {0: 0, 1: 4, 2: 3, 3: 8}[layout]
        off = (lambda j: (1 + j) % 4 if layout == 2 else 0)
        self.U, self.C, self.X, self.thr, self.slot, self.mu, self.sigma, self.w = U, Cm, X, thr, slot, mu, sigma, w
        self.delay_ldx = delay_ldx
        vec = (lambda v, j: None if v is None else mg.Guarded(m, 1, m, F32, off(j), DEV).fill(v).snapshot())
        self.gU = mg.Guarded(m, k, m + pad, F32, off(0), DEV).fill(U).snapshot()
        self.gC = mg.Guarded(k, B * T, k + pad, F32, off(1), DEV).fill(Cm).snapshot()
        self.gthr = mg.Guarded(m, J * S, m + pad, F32, off(2), DEV).fill(thr).snapshot()
        self.gmu, self.gsg, self.gw = vec(mu, 2), vec(sigma, 0), vec(w, 1)
        self.gslot = None
        if slot is not None:        # int32 labels in the integer view of a guarded fp32 column
            self.gslot = mg.Guarded(T, 1, T, F32, off(3), DEV)
            self.gslot.iview[0] = torch.from_numpy(np.asarray(slot, dtype=np.int32)).to(DEV)
            self.gslot.snapshot()
        if delay_ldx is None:
            self.gX = mg.Guarded(m, T, m + pad, F32, off(1), DEV).fill(X).snapshot()
        else:   # rows > ldx: X[i, t] = flat[i + t * ldx]
            self.gX = mg.Guarded(m, T, delay_ldx, F32, off(1), DEV)
            self.gX.fbuf[self.gX.start:self.gX.start + self.gX.region] = torch.from_numpy(delay_flat(X, delay_ldx)).to(DEV)
            self.gX.snapshot()
        self.gcol = mg.Guarded(T, NQ * J, T + pad, F64, 0, DEV)
        self.grow = mg.Guarded(m, NQ * J, m + pad, F64, 0, DEV)
        self.gcnt = GuardedCounts(2 * J * (B + 1))
        self.gP = mg.Guarded(m, J * T, m + pad, F32, off(2), DEV)

    def inputs(self):
        return [g for g in (self.gU, self.gC, self.gthr, self.gslot, self.gmu, self.gsg, self.gw, self.gX) if g is not None]

    def check_inputs(self):
        for g in self.inputs():
            g.check_untouched("input")
            g.check_unchanged("input")

    def _shared(self):
        p = (lambda g: None if g is None else g.ptr)
        return dict(U=self.gU.ptr, m=self.m, k=self.k, ldu=self.gU.ld, C=self.gC.ptr, ldc=self.gC.ld, T=self.T, B=self.B,
                    mu=p(self.gmu), sigma=p(self.gsg), thr=self.gthr.ptr, ldthr=self.gthr.ld, J=self.J, S=self.S,
                    slot=p(self.gslot), above=int(self.above))

    def run(self, L, accumulate=0, rows=True, cnt=True, ws=None, **over):
        need = L.dmdx_exceed_score_workspace_bytes(self.m, self.k, self.T, self.B, self.J)
        assert need > 0
        self.ws = mg.exact_workspace(need, DEV) if ws is None else ws
        a = self._shared()
        a.update(X=self.gX.ptr, ldx=self.gX.ld, w=None if self.gw is None else self.gw.ptr, col=self.gcol.ptr,
                 ldcol=self.gcol.ld, row=self.grow.ptr if rows else None, ldrow=self.grow.ld,
                 cntp=self.gcnt.ptr if cnt else None, wsp=self.ws.ptr, wsb=self.ws.nbytes)
        a.update(over)
        rc = L.dmdx_exceed_score_f32(a["U"], a["m"], a["k"], a["ldu"], a["C"], a["ldc"], a["T"], a["B"], a["mu"], a["sigma"],
                                     a["thr"], a["ldthr"], a["J"], a["S"], a["slot"], a["above"], a["X"], a["ldx"], a["w"],
                                     a["col"], a["ldcol"], a["row"], a["ldrow"], a["cntp"], accumulate, a["wsp"], a["wsb"],
                                     _stream())
        torch.cuda.synchronize()
        return rc

    def run_prob(self, L, **over):
        a = self._shared()
        a.update(P=self.gP.ptr, ldp=self.gP.ld, pstride=self.T * self.gP.ld)
        a.update(over)
        rc = L.dmdx_exceed_prob_f32(a["U"], a["m"], a["k"], a["ldu"], a["C"], a["ldc"], a["T"], a["B"], a["mu"], a["sigma"],
                                    a["thr"], a["ldthr"], a["J"], a["S"], a["slot"], a["above"], a["P"], a["ldp"],
                                    a["pstride"], _stream())
        torch.cuda.synchronize()
        return rc

    def sums(self):
        """-> (col (J, 4, T), row (J, 4, m))"""
        return (self.gcol.logical().T.reshape(self.J, NQ, self.T).copy(),
                self.grow.logical().T.reshape(self.J, NQ, self.m).copy())

    def counts(self):
        return self.gcnt.counts().reshape(self.J, 2, self.B + 1)

    def planes(self):
        """-> P (J, m, T)"""
        return self.gP.logical().reshape(self.m, self.J, self.T).transpose(1, 0, 2).copy()

    def with_(self, **kw):
        o = dict(U=self.U, Cm=self.C, X=self.X, thr=self.thr, slot=self.slot, mu=self.mu, sigma=self.sigma, w=self.w,
                 above=self.above)
        o.update(kw)
        above = o.pop("above")
        c = Case(self.m, self.k, self.T, self.B, self.J, self.S, self.layout, above, delay_ldx=self.delay_ldx, **o)
        return c

    def fields(self, L):
        """The B member fields as dmdx_expand_f32 gives them for C_b: (B, m, T) fp32."""
        out = np.empty((self.B, self.m, self.T), dtype=np.float32)
        p = (lambda g: None if g is None else g.ptr)
        g = mg.Guarded(self.m, self.T, self.m, F32, 0, DEV)
        for b in range(self.B):
            rc = L.dmdx_expand_f32(self.gU.ptr, self.m, self.k, self.gU.ld, self.gC.col_ptr(b * self.T), self.gC.ld, self.T,
                                   p(self.gmu), p(self.gsg), g.ptr, g.ld, _stream())
            assert rc == 0, L.dmdx_last_error()
            torch.cuda.synchronize()
            out[b] = g.logical()
        return out

    def ref_args(self, F):
        return F, self.X, self.thr, self.J, self.S, self.slot, self.above


def rand_ops(rng, m, k, T, B, J, S, layout, wmode="positive", delay_ldx=None, null_slot=False):
    o = member_ops(rng, m, k, T, B, layout, wmode, delay_ldx)
    mu = np.zeros(m) if o["mu"] is None else o["mu"].astype(np.float64)
    sg = np.ones(m) if o["sigma"] is None else o["sigma"].astype(np.float64)
    thr = np.empty((m, J * S), dtype=np.float32)
    for j in range(J):
        for s in range(S):
            thr[:, j * S + s] = mu + Z[j] * sg * np.sqrt(k) * (1.0 + 0.1 * rng.standard_normal(m))
    slot = None if (null_slot and S == 1) else rng.integers(0, S, T).astype(np.int32)
    return dict(thr=thr, slot=slot, **o)


def discriminating(c, F):
    """The condition of the module docstring, on the reference alone."""
    cc, o, _, finite = xr.elements(*c.ref_args(F))
    if not (o.any() and not o.all()):
        return False
    if c.B >= 5 and c.k >= 16 and c.m * c.T >= 20:
        for j in range(c.J):
            if ((cc[j] > 0) & (cc[j] < c.B)).mean() < 0.10 or not 0.05 <= o[j].mean() <= 0.95:
                return False
    return True


def make_case(L, rng, m, k, T, B, J, S, layout, wmode="positive", above=True, delay_ldx=None):
    """-> (case, its member fields): the first of at most 40 draws the reference finds discriminating."""
    for _ in range(40):
        c = Case(m, k, T, B, J, S, layout, above, delay_ldx=delay_ldx,
                 **rand_ops(rng, m, k, T, B, J, S, layout, wmode, delay_ldx, null_slot=layout in (0, 3)))
        F = c.fields(L)
        if discriminating(c, F):
            return c, F
    raise AssertionError(("no discriminating draw", m, k, T, B, J, S))


def parity_shapes():
    """A pairwise-covering sample of (m, k, T, B, J, S, layout, w mode, above): greedy over 300 seeded random
    candidates per step.  A single element with a single threshold cannot show both outcomes and is no candidate."""
    lists = [MS, KS, TS, BS, JS, SS, LAYOUTS, WMODES, ABOVE]
    n = len(lists)
    pairs = list(itertools.combinations(range(n), 2))
    todo = {(a, x, b, y) for a, b in pairs for x in range(len(lists[a])) for y in range(len(lists[b]))}
    rng = np.random.default_rng(2400)
    out = []
    while todo:
        cands = [tuple(int(rng.integers(len(l))) for l in lists) for _ in range(300)]
        cands = [c for c in cands if not (lists[0][c[0]] == 1 and lists[2][c[2]] == 1 and lists[4][c[4]] == 1)]
        best = max(cands, key=lambda c: sum((a, c[a], b, c[b]) in todo for a, b in pairs))
        todo -= {(a, best[a], b, best[b]) for a, b in pairs}
        out.append(tuple(l[i] for l, i in zip(lists, best)))
    assert len(out) <= 60
    return out


PARITY = parity_shapes()


def n_selected(c, finite=None):
    """The number of elements that enter the bins of one threshold."""
    sel = np.ones((c.m, c.T), dtype=bool) if finite is None else finite.copy()
    if c.w is not None:
        sel &= (c.w != 0)[:, None]
    return int(sel.sum())


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def check_exceed(L, c, F, rows=True, cnt=True, bounded=True):
    """Both entry points against the reference of the fields F: memory, P and cnt exactly, col / row in the bound."""
    assert c.run_prob(L) == 0, L.dmdx_last_error()
    c.gP.check_fully_written("P")
    c.gP.check_untouched("P")
    el = xr.elements(*c.ref_args(F))
    assert same_bits(c.planes(), xr.prob(F, c.thr, c.J, c.S, c.slot, c.above, el))
    assert c.run(L, rows=rows, cnt=cnt) == 0, L.dmdx_last_error()
    c.gcol.check_fully_written("col")
    c.gcol.check_untouched("col")
    c.grow.check_untouched("row")
    c.gcnt.check_untouched()
    if rows:
        c.grow.check_fully_written("row")
    else:
        assert bool((c.grow.ibuf == c.grow.canary).all())
    if cnt:
        c.gcnt.check_fully_written()
    else:
        c.gcnt.check_unwritten()
    c.ws.check_untouched()
    c.check_inputs()
    want = xr.score(*c.ref_args(F), c.w, el)
    if bounded:
        bounds = xr.bounds_of(*want[:2])
        for g, w_, b, name in list(zip(c.sums(), want, bounds, ("col", "row")))[:2 if rows else 1]:
            err = np.abs(g - w_)
            assert (err <= b).all(), (name, c.m, c.k, c.T, c.B, c.J, float((err / np.maximum(b, 1e-300)).max()))
            assert (g >= 0).all() and not np.signbit(g).any()
    if cnt:
        h = c.counts()
        assert np.array_equal(h, want[2])
        finite = np.isfinite(F).all(axis=0) & np.isfinite(c.X)
        assert (h >= 0).all() and (h.sum(axis=(1, 2)) == n_selected(c, finite)).all()
    return want


@pytest.mark.parametrize("n", range(len(PARITY)))
def test_parity_over_the_shape_edges(L, n):
    m, k, T, B, J, S, layout, wmode, above = PARITY[n]
    assert (int(L.dmdx_exceed_max_members()), int(L.dmdx_exceed_max_k()), int(L.dmdx_exceed_max_thresholds())) == \
        (xr.MAX_B, 256, xr.MAX_THR)
    c, F = make_case(L, np.random.default_rng(2401 + n), m, k, T, B, J, S, layout, wmode, above)
    check_exceed(L, c, F, rows=n % 4 != 3, cnt=n % 3 != 2)


def test_several_workgroups_and_time_splits(L):
    """1003 rows = 8 row blocks, 300 snapshots = 10 tiles, one per workgroup: the T split, the partial slots of
    several row blocks and the reduce kernels take part."""
    c, F = make_case(L, np.random.default_rng(2460), 1003, 37, 300, 5, 3, 3, 2, "zeros")
    assert L.dmdx_exceed_score_workspace_bytes(1003, 37, 300, 5, 3) > 8 * 10 * 2 * 3 * 6 * 8
    check_exceed(L, c, F)


def plan(m, T):
    """-> (row blocks, tiles, tiles per workgroup, T splits): plan_for of csrc/expand_tile.h, restated."""
    nrb, ntiles = -(-m // 128), -(-T // 32)
    want = max(1, min(-(-2048 // nrb), ntiles))
    tpw = -(-ntiles // want)
    return nrb, ntiles, tpw, -(-ntiles // tpw)


@pytest.mark.parametrize("B", [1, 3])
def test_several_tiles_per_workgroup(L, B):
    """16 400 rows = 129 row blocks and 530 snapshots = 17 tiles, the last one partial: 2 tiles per workgroup in 9
    T splits (the last split has one tile), which is how a production row block runs -- no smaller shape walks the
    tile loop twice (tiles x row blocks must exceed 2048).  What only a second tile does is in play: the reload of the
    thresholds and the reset of the counts and of the finite flag, the hand-over of the C stage from the last member
    of a tile to member 0 of the next, the reuse of the column slots and of the LDS counters behind one barrier per
    member (B = 1: a single barrier between two epilogues), their drain into the 64-bit counts, the row sums carried
    over tiles.  Planes and counts exactly, sums within the bound; the workspace size confirms the plan."""
    m, k, T, J, S = 16400, 5, 530, 4, 3
    nrb, ntiles, tpw, nsplit = plan(m, T)
    assert (nrb, ntiles, tpw, nsplit) == (129, 17, 2, 9)
    a16 = (lambda n: (n + 15) // 16 * 16)
    assert L.dmdx_exceed_score_workspace_bytes(m, k, T, B, J) == \
        16 + a16(nsplit * 4 * J * m * 8) + nrb * 4 * J * T * 4 + nrb * nsplit * 2 * J * (B + 1) * 8
    for shape in [(1003, 300), (1003, 131)] + [(mm, tt) for mm in MS for tt in TS]:
        assert plan(*shape)[2] == 1                 # (every other shape of this file: one tile per workgroup)
    c, F = make_case(L, np.random.default_rng(2471 + B), m, k, T, B, J, S, 2, "zeros")
    want = check_exceed(L, c, F)
    assert (want[2].sum(axis=2) > 0).all()          # every threshold sees both outcomes


def test_delay_view(L):
    """X with rows > ldx (the zero-copy delay view)."""
    c, F = make_case(L, np.random.default_rng(2461), 300, 20, 45, 5, 2, 1, 0, "zeros", delay_ldx=100)
    check_exceed(L, c, F)


def test_accumulate_adds_row_blocks(L):
    """Two row blocks into one col and one cnt; the second call's `row` is its own."""
    rng = np.random.default_rng(2462)
    m, k, T, B, J, S, h = 300, 33, 70, 9, 3, 3, 170
    full, Ff = make_case(L, rng, m, k, T, B, J, S, 2, "zeros")
    cut = (lambda v, s: None if v is None else v[s])
    a, b = [Case(s.stop - s.start, k, T, B, J, S, 2, True, full.U[s], full.C, full.X[s], full.thr[s], full.slot, cut(full.mu, s),
                 cut(full.sigma, s), cut(full.w, s)) for s in (slice(0, h), slice(h, m))]
    assert a.run(L) == 0, L.dmdx_last_error()
    first, hfirst = a.sums()[0], a.counts()
    assert b.run(L, accumulate=1, col=a.gcol.ptr, ldcol=a.gcol.ld, cntp=a.gcnt.ptr) == 0, L.dmdx_last_error()
    a.gcol.check_untouched("col")
    a.gcnt.check_untouched()
    assert bool((b.gcol.ibuf == b.gcol.canary).all())
    b.gcnt.check_unwritten()
    got, hgot = a.sums()[0], a.counts()
    # the counts are those of one call over all rows, and the sums the fp64 sum of the two calls' own results
    whole = xr.score(*full.ref_args(Ff), full.w)
    assert np.array_equal(hgot, whole[2])
    assert (np.abs(got - whole[0]) <= xr.score_bounds(*full.ref_args(Ff), full.w)[0]).all()
    assert b.run(L) == 0
    assert np.array_equal(got, first + b.sums()[0])
    assert np.array_equal(hgot, hfirst + b.counts())
    assert (np.abs(b.sums()[1] - whole[1][:, :, h:]) <= xr.score_bounds(*full.ref_args(Ff), full.w)[1][:, :, h:]).all()


# ---------------------------------------------------------------- the counts, exactly
@pytest.mark.parametrize("above", [True, False])
@pytest.mark.parametrize("shape", [(1003, 37, 300, 5, 2), (257, 256, 33, 33, 3), (131, 17, 77, 9, 1)])
def test_counts_and_planes_are_exact_with_planted_ties(L, shape, above):
    """cnt and P equal the reference of the fields of dmdx_expand_f32 as integers / bit for bit, in both directions,
    with ties planted two ways -- thr copied bit for bit from a member's field, and X equal to its threshold -- NaN in
    X and in thr on a few elements, and masked rows.  A tie is never an event: counting ties gives other counts."""
    m, k, T, B, layout = shape
    J, S = 4, 3
    rng = np.random.default_rng(2463)
    c, F = make_case(L, rng, m, k, T, B, J, S, layout, "zeros", above)
    thr, X = c.thr.copy(), c.X.copy()
    for col in range(J * S):                       # a tenth of the thresholds: a member's value at a snapshot of the slot
        ts = np.nonzero(c.slot == col % S)[0]
        rows_ = np.nonzero(rng.random(m) < 0.1)[0]
        if len(ts):
            thr[rows_, col] = F[rng.integers(0, B, len(rows_)), rows_, rng.choice(ts, len(rows_))]
    thr[rng.random(thr.shape) < 0.01] = np.nan
    th = xr.thresholds_of(thr, J, S, T, c.slot)
    tie = rng.random((m, T)) < 0.1
    X[tie] = th[rng.integers(0, J, (m, T)), np.arange(m)[:, None], np.arange(T)[None]][tie]
    X[np.isnan(X)] = 0.0
    nan = rng.random((m, T)) < 0.01
    X[nan] = np.nan
    c = c.with_(thr=thr, X=X)
    want = check_exceed(L, c, F, bounded=False)
    member_ties = int((F[:, None] == th[None]).sum())
    assert member_ties > 10 and int((X[None] == th).sum()) > 10 and nan[(c.w != 0)].sum() >= 1
    # the tie convention is visible: with >= / <= the counts are others
    cmp = np.greater_equal if above else np.less_equal
    with np.errstate(invalid="ignore"):
        loose_c = cmp(F[:, None], th[None]).sum(axis=0)
        loose_o = cmp(X[None], th)
    strict_c, strict_o, _, _ = xr.elements(*c.ref_args(F))
    assert (loose_c != strict_c).any() and (loose_o != strict_o).any()
    assert want[2].sum() == J * n_selected(c, ~nan)


def test_a_nan_threshold_gives_no_event(L):
    """Threshold 1 is NaN everywhere: c = 0 and o = 0 there, finite -- P is +0.0, every element sits in bin (0, 0),
    the sums are 0 -- and the other thresholds keep their bits."""
    rng = np.random.default_rng(2464)
    base, F = make_case(L, rng, 150, 37, 70, 9, 3, 3, 2, "zeros")
    assert base.run(L) == 0 and base.run_prob(L) == 0, L.dmdx_last_error()
    thr = base.thr.copy()
    thr[:, 3:6] = np.nan
    c = base.with_(thr=thr)
    check_exceed(L, c, F)
    P, (col, row), h = c.planes(), c.sums(), c.counts()
    assert np.array_equal(P[1].view(np.int32), np.zeros_like(P[1]).view(np.int32))
    assert not col[1].any() and not row[1].any()
    assert h[1, 0, 0] == n_selected(c) == h[1].sum()
    for j in (0, 2):
        assert same_bits(P[j], base.planes()[j]) and np.array_equal(h[j], base.counts()[j])
        assert np.array_equal(col[j].view(np.int64), base.sums()[0][j].view(np.int64))


# ---------------------------------------------------------------- the mask
def test_masked_rows_are_selected_out(L):
    """NaN, +Inf and 1e38 in the rows with w == 0 of X, U, mu, sigma and thr: col and cnt keep the bits of the run
    with ordinary values there."""
    rng = np.random.default_rng(2465)
    m, k, T, B, J, S = 150, 37, 70, 9, 2, 3
    base, _ = make_case(L, rng, m, k, T, B, J, S, 2, "zeros")
    masked = np.nonzero(base.w == 0)[0]
    assert len(masked) >= 3
    assert base.run(L) == 0, L.dmdx_last_error()
    (col0, row0), h0 = base.sums(), base.counts()
    assert np.isfinite(col0).all() and np.isfinite(row0).all() and (h0.sum(axis=(1, 2)) == (m - len(masked)) * T).all()
    vals = np.array([np.nan, np.inf, 1e38], dtype=np.float32)
    keep = np.ones(m, dtype=bool)
    keep[masked] = False
    for what in ("X", "U", "mu", "sigma", "thr"):
        ops = dict(U=base.U.copy(), X=base.X.copy(), mu=base.mu.copy(), sigma=base.sigma.copy(), thr=base.thr.copy())
        for n, i in enumerate(masked):
            v = vals[n % 3]
            if what in ("X", "U", "thr"):
                ops[what][i, (3 * n) % ops[what].shape[1]] = v
            else:
                ops[what][i] = v
        c = base.with_(**ops)
        assert c.run(L) == 0, L.dmdx_last_error()
        col, row = c.sums()
        assert np.array_equal(col.view(np.int64), col0.view(np.int64)), what
        assert np.array_equal(c.counts(), h0), what
        assert np.array_equal(row[:, :, keep].view(np.int64), row0[:, :, keep].view(np.int64)), what
        if what != "thr":
            nanrows = masked[np.arange(len(masked)) % 3 == 0]          # a NaN reaches the row's sums in any case
            assert np.isnan(row[:, :, nanrows]).all(), what
        c.ws.check_untouched()
    # every weight 0: the column sums are +0.0 and the counts 0
    c = base.with_(w=np.zeros(m, dtype=np.float32))
    assert c.run(L) == 0
    assert np.array_equal(c.sums()[0].view(np.int64), np.zeros_like(col0).view(np.int64)) and not c.counts().any()


# ---------------------------------------------------------------- NaN / Inf where they count
PLANTS = [("X", np.nan), ("X", np.inf), ("X", -np.inf), ("U", np.nan), ("U", np.inf), ("U_last", -np.inf), ("C", np.nan),
          ("C", -np.inf), ("mu", np.inf), ("sigma", np.nan)]


def test_planted_nan_and_inf(L):
    """In a row that is NOT masked.  X[i0, t0]: column t0 and row i0 of all 4 J sums become NaN, nothing else moves a
    bit, the element is in no bin, and P (which knows no X) keeps its bits.  U[i0, j], mu[i0], sigma[i0]: row i0 and
    every column; row i0 of every plane of P is NaN.  C[j0, b0 T + t0] (a member): column t0 and every row."""
    rng = np.random.default_rng(2466)
    m, k, T, B, J, S = 150, 37, 70, 9, 3, 3
    i0, j0, t0, b0 = 77, 11, 41, 4
    base, F = make_case(L, rng, m, k, T, B, J, S, 2, "zeros")
    w = base.w.copy()
    w[i0] = 0.5
    base = base.with_(w=w)
    check_exceed(L, base, F)
    clean, hclean, Pclean = base.sums(), base.counts(), base.planes()
    cc, o, _, _ = xr.elements(*base.ref_args(F))
    sel = w != 0
    for what, val in PLANTS:
        ops = dict(U=base.U.copy(), Cm=base.C.copy(), X=base.X.copy(), mu=base.mu.copy(), sigma=base.sigma.copy())
        bad = np.zeros((m, T), dtype=bool)
        if what in ("U", "U_last"):
            ops["U"][i0, j0 if what == "U" else k - 1] = val
            bad[i0, :] = True
        elif what == "C":
            ops["Cm"][j0, b0 * T + t0] = val
            bad[:, t0] = True
        elif what == "X":
            ops["X"][i0, t0] = val
            bad[i0, t0] = True
        else:
            ops[what][i0] = val
            bad[i0, :] = True
        c = base.with_(**ops)
        assert c.run(L) == 0 and c.run_prob(L) == 0, L.dmdx_last_error()
        col, row = c.sums()
        badcol, badrow = bad[sel].any(axis=0), bad.any(axis=1)
        assert np.array_equal(np.isnan(col), np.broadcast_to(badcol, col.shape)), (what, val)
        assert np.array_equal(np.isnan(row), np.broadcast_to(badrow, row.shape)), (what, val)
        assert np.array_equal(col.view(np.int64)[:, :, ~badcol], clean[0].view(np.int64)[:, :, ~badcol]), (what, val)
        assert np.array_equal(row.view(np.int64)[:, :, ~badrow], clean[1].view(np.int64)[:, :, ~badrow]), (what, val)
        gone = np.zeros_like(hclean)
        live = bad & sel[:, None]
        for j in range(J):
            np.add.at(gone[j], (o[j][live].astype(int), cc[j][live]), 1)
        assert np.array_equal(c.counts(), hclean - gone), (what, val)
        P = c.planes()
        pbad = np.zeros_like(bad) if what == "X" else bad
        assert np.array_equal(np.isnan(P), np.broadcast_to(pbad, P.shape)), (what, val)
        assert np.array_equal(P[:, ~pbad].view(np.int32), Pclean[:, ~pbad].view(np.int32)), (what, val)


# ---------------------------------------------------------------- scaling, reproducibility
def test_power_of_two_scaling_of_the_factors(L):
    """(2^e U, 2^-e C) changes no bit of any output."""
    rng = np.random.default_rng(2467)
    base, _ = make_case(L, rng, 200, 50, 45, 9, 4, 3, 1, "zeros")
    assert base.run(L) == 0 and base.run_prob(L) == 0, L.dmdx_last_error()
    (col0, row0), h0, P0 = base.sums(), base.counts(), base.planes()
    up, dn = np.float32(2.0 ** 40), np.float32(2.0 ** -40)
    for su, sc in ((up, dn), (dn, up)):
        c = base.with_(U=base.U * su, Cm=base.C * sc)
        assert c.run(L) == 0 and c.run_prob(L) == 0
        for a, b in zip(c.sums(), (col0, row0)):
            assert np.array_equal(a.view(np.int64), b.view(np.int64))
        assert np.array_equal(c.counts(), h0) and np.array_equal(c.planes().view(np.int32), P0.view(np.int32))


def test_two_calls_give_the_same_bits(L):
    c, _ = make_case(L, np.random.default_rng(2468), 1003, 50, 131, 19, 4, 3, 2, "zeros")
    assert c.run(L) == 0 and c.run_prob(L) == 0, L.dmdx_last_error()
    firsts, h = [g.iview.clone() for g in (c.gcol, c.grow, c.gP)], c.counts()
    for g in (c.gcol, c.grow, c.gP):
        g.ibuf.fill_(g.canary)
    c.gcnt.buf.fill_(ICANARY)
    assert c.run(L) == 0 and c.run_prob(L) == 0
    for g, f in zip((c.gcol, c.grow, c.gP), firsts):
        assert torch.equal(g.iview, f)
        g.check_untouched()
    assert np.array_equal(c.counts(), h)


# ---------------------------------------------------------------- refusals
def test_refused_calls_write_nothing(L):
    c, _ = make_case(L, np.random.default_rng(2469), 70, 9, 40, 5, 2, 3, 1, "zeros")
    kmax, bmax, jmax = int(L.dmdx_exceed_max_k()), int(L.dmdx_exceed_max_members()), int(L.dmdx_exceed_max_thresholds())
    big = 2 ** 31
    ws = mg.exact_workspace(L.dmdx_exceed_score_workspace_bytes(c.m, c.k, c.T, c.B, c.J), DEV)
    shared = [dict(k=0), dict(k=kmax + 1), dict(B=0), dict(B=-1), dict(B=bmax + 1), dict(U=None), dict(C=None), dict(thr=None),
              dict(J=0), dict(J=jmax + 1), dict(S=0), dict(S=-1), dict(ldthr=c.m - 1), dict(ldthr=big), dict(J=2, S=2 ** 30),
              dict(S=big), dict(m=0), dict(T=0), dict(m=-1), dict(ldu=c.m - 1), dict(ldc=c.k - 1), dict(ldu=big), dict(ldc=big),
              dict(m=big, ldu=big, ldthr=big)]
    bad = shared + [dict(ldcol=c.T - 1), dict(ldrow=c.m - 1), dict(X=None), dict(col=None), dict(ldx=0), dict(ldx=big),
                    dict(ldcol=big), dict(ldrow=big), dict(T=big, ldcol=big), dict(T=2 ** 30, ldcol=2 ** 30)]
    for over in bad:
        assert c.run(L, ws=ws, **over) == E_INVALID, over
        assert L.dmdx_last_error()
    assert c.run(L, ws=ws, wsb=ws.nbytes - 1) == E_WORKSPACE
    assert L.dmdx_last_error()
    assert c.run(L, ws=ws, wsp=None) == E_WORKSPACE
    for over in shared + [dict(P=None), dict(ldp=c.m - 1), dict(ldp=big), dict(pstride=c.T * c.gP.ld - c.gP.ld + c.m - 1),
                          dict(pstride=0), dict(T=2 ** 30)]:
        assert c.run_prob(L, **over) == E_INVALID, over
        assert L.dmdx_last_error()
    ws.check_unused()
    ws.check_untouched()
    for g in (c.gcol, c.grow, c.gP):
        assert bool((g.ibuf == g.canary).all())
    c.gcnt.check_unwritten()
    c.check_inputs()
    # the workspace does not depend on whether row and cnt are given; ldrow is not looked at without row; one plane
    # has no stride to look at
    assert c.run(L, rows=False, cnt=False, ldrow=0) == 0, L.dmdx_last_error()
    c.gcnt.check_unwritten()
    assert c.run_prob(L, J=1, pstride=0) == 0, L.dmdx_last_error()


# ---------------------------------------------------------------- the provider methods
def test_the_provider_methods(L):
    """HipKernels.exceed_prob / exceed_score: (J, S, m) and (J, m) tables, the pitched members, accumulation into
    out / counts, the per-row sums, the refusals of the wrapper."""
    from dmd_era5_amd.forecast import _pitched_dev
    from dmd_era5_amd.kernels import default_kernels

    KERN = default_kernels()
    rng = np.random.default_rng(2470)
    m, k, T, B, J, S = 333, 5, 41, 7, 3, 3
    o = rand_ops(rng, m, k, T, B, J, S, 0, "zeros")
    t = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV))
    Ut, Xt, mu, sd, w = t(o["U"].T), t(o["X"].T), t(o["mu"]), t(o["sigma"]), t(o["w"])
    Cm, slot = t(o["Cm"].T.reshape(B, T, k)), t(o["slot"])
    thr = t(o["thr"].T.reshape(J, S, m))
    F = np.stack([KERN.expand(Ut, Cm[b], mu, sd).cpu().numpy().T for b in range(B)])
    assert (KERN.exceed_max_k, KERN.exceed_max_members, KERN.exceed_max_thresholds) == (256, xr.MAX_B, xr.MAX_THR)
    for above in (True, False):
        P = KERN.exceed_prob(Ut, Cm, thr, slot, above, mu, sd)
        assert P.shape == (J, T, m) and P.dtype == F32
        assert same_bits(P.cpu().numpy().transpose(0, 2, 1), xr.prob(F, o["thr"], J, S, o["slot"], above))
        cols, rows, cnt = KERN.exceed_score(Ut, Cm, Xt, thr, slot, above, mu, sd, w, want_rows=True)
        args = (F, o["X"], o["thr"], J, S, o["slot"], above, o["w"])
        want, bounds = xr.score(*args), xr.score_bounds(*args)
        assert cols.shape == (J, 4, T) and rows.shape == (J, 4, m) and cnt.shape == (J, 2, B + 1) and cnt.dtype == torch.int64
        for g, w_, b in zip((cols, rows), want, bounds):
            assert (np.abs(g.cpu().numpy() - w_) <= b).all()
        assert np.array_equal(cnt.cpu().numpy(), want[2])
    Cp = _pitched_dev(KERN, Cm)
    again, none, c2 = KERN.exceed_score(Ut, Cp, Xt, thr, slot, False, mu, sd, w, out=cols.clone(), counts=cnt.clone())
    assert none is None and torch.equal(again, 2 * cols) and torch.equal(c2, 2 * cnt)
    out = torch.empty((J, T, m), dtype=F32, device=DEV)
    assert KERN.exceed_prob(Ut, Cp, thr, slot, False, mu, sd, out=out) is out and torch.equal(out, P)
    # one slot: a (J, m) table, no labels
    P1 = KERN.exceed_prob(Ut, Cm, thr[:, 0].contiguous(), None, True, mu, sd)
    assert same_bits(P1.cpu().numpy().transpose(0, 2, 1), xr.prob(F, o["thr"][:, ::S].copy(), J, 1, None, True))
    for call in (lambda: KERN.exceed_score(Ut, Cm, Xt, thr, slot, True, mu, sd, w, out=cols.clone()),
                 lambda: KERN.exceed_prob(Ut, Cm, thr, None),                                  # three slots, no labels
                 lambda: KERN.exceed_prob(Ut, Cm, thr, slot + 1),                              # a label outside 0 .. S - 1
                 lambda: KERN.exceed_prob(Ut, Cm, thr, slot - 1),
                 lambda: KERN.exceed_prob(Ut, Cm, thr, slot.to(torch.int64)),
                 lambda: KERN.exceed_prob(Ut, Cm, thr.double(), slot),
                 lambda: KERN.exceed_prob(Ut, Cm, torch.cat([thr, thr[:2]]), slot),            # J = 5
                 lambda: KERN.exceed_prob(Ut, Cm, thr[:, :, :-1].contiguous(), slot),
                 lambda: KERN.exceed_prob(Ut, t(np.zeros((B, T, k + 1), dtype=np.float32)), thr, slot)):
        with pytest.raises(Exception):
            call()
