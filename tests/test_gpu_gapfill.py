"""K31 on the GPU through the ctypes table: dmdx_gap_fill_f32.

What is held: at the set bits X is bit for bit what dmdx_expand_f32 stores for the same operands, at the clear bits X
keeps its bits (distinct NaN payloads are planted there: a load that took part in anything would show), change_row is
sum_t bit (new - old)^2 within the derived bound, a skipped wave or workgroup changes nothing.  Every operand lives in a
guarded allocation (tests/memguard.py), the workspace is exact.

The bound of change_row, c u sum (new - old)^2 with u = 2^-24 (tests/gap_ref.py: CHANGE_C).  `new` is the stored fp32
value, so the error of the MFMA chain is not in it.  Per set bit the kernel rounds the subtraction once and the square
once: (1 + u)^2 on d^2 from the first, (1 + u) from the second.  A lane adds its 16 values of a tile in fp32, the first
to 0: at most 15 rounded additions on any value, (1 + u)^15.  Tiles, the two lane halves and the T splits are added in
fp64: fewer than 2^27 additions of relative 2^-53, together below u / 4.  Every term is >= 0, so the relative errors
carry over to the sum: (1 + u)^18 - 1 + u / 4 < 19 u, c = 19.
"""
import itertools

import numpy as np
import pytest
import torch

import gap_ref as gr
import memguard as mg

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DEV = "cuda"
MS = [1, 31, 33, 127, 129, 300]
TS = [1, 31, 32, 33, 65, 100]
KS = [1, 7, 16, 17, 33, 64, 256]
MASKS = ["random", "single", "ones", "stray"]


@pytest.fixture(scope="module")
def L():
    from dmd_era5_amd.kernels import default_kernels

    return default_kernels()._lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def payloads(m, T):
    """A distinct quiet NaN per element (never the canary of memguard)."""
    idx = np.arange(m * T, dtype=np.uint32).reshape(m, T)
    return (np.uint32(0x7FE00000) | (idx & np.uint32(0x1FFFFF))).view(np.float32)


def make_mask(rng, kind, m, T):
    G = np.zeros((m, T), dtype=bool)
    if kind in ("random", "stray"):
        G = rng.random((m, T)) < 0.3
    elif kind == "single":
        G[rng.integers(m), rng.integers(T)] = True
    else:
        G[:] = True
    W = gr.pack_bits(G)
    if kind == "stray" and T % 32:
        W[-1] |= (rng.integers(0, 2 ** 32, m, dtype=np.uint64).astype(np.uint32) << np.uint32(T % 32))
    return G, W


class Case:
    """Guarded operands of one call.  layout: 0 tight, 1 padded leading dimensions (multiples of 4), 2 odd leading
    dimensions and bases 1 .. 3 elements past a 16-byte boundary, 3 as 1 without mu / sigma."""

    def __init__(self, m, k, T, layout, U, Cm, mu, sigma, G, W, old):
        self.m, self.k, self.T, self.G = m, k, T, G
        pad = {0: 0, 1: 4, 2: 3, 3: 8}[layout]
        off = (lambda j: (1 + j) % 4 if layout == 2 else 0)
        self.gU = mg.Guarded(m, k, m + pad, F32, off(0), DEV).fill(U).snapshot()
        self.gC = mg.Guarded(k, T, k + pad, F32, off(1), DEV).fill(Cm).snapshot()
        self.gmu = None if mu is None else mg.Guarded(m, 1, m, F32, off(2), DEV).fill(mu).snapshot()
        self.gsg = None if sigma is None else mg.Guarded(m, 1, m, F32, off(0), DEV).fill(sigma).snapshot()
        self.gW = mg.Guarded(m, W.shape[0], m + pad, F32, off(3), DEV)
        self.gW.iview.copy_(torch.from_numpy(W.view(np.int32)).to(DEV))
        self.gW.snapshot()
        # X: the old values at the set bits, a NaN payload of its own at every clear bit
        self.X0 = np.where(G, old, payloads(m, T))
        self.gX = mg.Guarded(m, T, m + pad, F32, off(2), DEV)
        self.gX.iview.copy_(torch.from_numpy(np.ascontiguousarray(self.X0.T).view(np.int32)).to(DEV))
        self.gXh = mg.Guarded(m, T, m + pad + 1, F32, 0, DEV)
        self.gch = mg.Guarded(m, 1, m, F64, 0, DEV)

    def _factors(self):
        return (self.gU.ptr, self.m, self.k, self.gU.ld, self.gC.ptr, self.gC.ld, self.T,
                None if self.gmu is None else self.gmu.ptr, None if self.gsg is None else self.gsg.ptr)

    def fill(self, L, change=True, ws=None):
        need = L.dmdx_gap_fill_workspace_bytes(self.m, self.k, self.T)
        self.ws = (mg.exact_workspace(need, DEV) if ws is None else ws) if change else None
        rc = L.dmdx_gap_fill_f32(*self._factors(), self.gW.ptr, self.gW.ld, self.gX.ptr, self.gX.ld,
                                 self.gch.ptr if change else None, self.ws.ptr if change else None,
                                 self.ws.nbytes if change else 0, _stream())
        torch.cuda.synchronize()
        return rc

    def expand(self, L):
        rc = L.dmdx_expand_f32(*self._factors(), self.gXh.ptr, self.gXh.ld, _stream())
        torch.cuda.synchronize()
        return rc

    def check(self, L, change=True):
        """Run fill and expand and hold the fill to the contract -> (X bits, change_row)."""
        assert self.fill(L, change) == 0, L.dmdx_last_error()
        assert self.expand(L) == 0, L.dmdx_last_error()
        for g, name in ((self.gX, "X"), (self.gW, "W"), (self.gU, "U"), (self.gC, "C"), (self.gmu, "mu"),
                        (self.gsg, "sigma"), (self.gch, "change_row")):
            if g is not None:
                g.check_untouched(name)
                if g not in (self.gX, self.gch):
                    g.check_unchanged(name)
        X = self.gX.logical().view(np.uint32)
        Xh = self.gXh.logical().view(np.uint32)
        what = (self.m, self.k, self.T)
        assert np.array_equal(X[self.G], Xh[self.G]), what                    # K12's field, bit for bit
        assert np.array_equal(X[~self.G], self.X0.view(np.uint32)[~self.G]), what    # untouched elsewhere
        if not change:
            return X, None
        self.ws.check_untouched()
        self.gch.check_fully_written("change_row")
        got = self.gch.logical()[:, 0]
        exact = gr.change64(X.view(np.float32), self.X0, self.G)
        ok = np.isfinite(exact)
        err, bound = np.abs(got[ok] - exact[ok]), gr.change_bound(exact[ok])
        assert (err <= bound).all(), (what, float((err / np.maximum(bound, 1e-300)).max()))
        assert not np.isfinite(got[~ok]).any(), what
        return X, got


def rand_case(rng, m, k, T, layout, kind, G=None, W=None):
    U = rng.standard_normal((m, k)).astype(np.float32)
    Cm = rng.standard_normal((k, T)).astype(np.float32)
    mu = sigma = None
    if layout != 3:
        mu = (10.0 * rng.standard_normal(m)).astype(np.float32)
        sigma = (0.5 + rng.random(m)).astype(np.float32)
    if G is None:
        G, W = make_mask(rng, kind, m, T)
    old = (gr.fill64(U, Cm, mu, sigma) + rng.standard_normal((m, T))).astype(np.float32)
    return Case(m, k, T, layout, U, Cm, mu, sigma, G, W, old)


def parity_shapes():
    """All (m, k) pairs and all (k, T) pairs of the edge lists, the third size, the layout and the mask cycling (the
    pairing of test_gpu_expand.parity_shapes)."""
    out = []
    for (im, m), (ik, k) in itertools.product(enumerate(MS), enumerate(KS)):
        out.append((m, k, TS[(im + 2 * ik) % len(TS)], (im + ik) % 4, MASKS[(im + 3 * ik) % 4]))
    for (ik, k), (it, T) in itertools.product(enumerate(KS), enumerate(TS)):
        out.append((MS[(2 * ik + it) % len(MS)], k, T, (ik + it + 1) % 4, MASKS[(ik + it) % 4]))
    return out


def test_parity_with_expand_over_the_shape_edges(L):
    assert L.dmdx_gap_fill_max_k() == L.dmdx_expand_max_k() == 256
    rng = np.random.default_rng(3111)
    for n, (m, k, T, layout, kind) in enumerate(parity_shapes()):
        rand_case(rng, m, k, T, layout, kind).check(L, change=n % 5 != 4)


def test_exact_integers(L):
    """Integer U, C, mu, sigma and X inside 2^24: every difference, square and partial sum is an integer below 2^24 in
    fp32 (|U C| <= 9 k, |d| < 700, 16 d^2 < 2^23), so change_row is the integer result bit for bit."""
    rng = np.random.default_rng(3112)
    for m, k, T, layout in ((129, 17, 100, 1), (300, 33, 65, 2), (31, 7, 33, 0)):
        U = rng.integers(-3, 4, (m, k)).astype(np.float32)
        Cm = rng.integers(-3, 4, (k, T)).astype(np.float32)
        mu = rng.integers(-5, 6, m).astype(np.float32)
        sigma = rng.integers(1, 3, m).astype(np.float32)
        G, W = make_mask(rng, "random", m, T)
        old = rng.integers(-100, 101, (m, T)).astype(np.float32)
        c = Case(m, k, T, layout, U, Cm, mu, sigma, G, W, old)
        X, got = c.check(L)
        new = gr.fill64(U, Cm, mu, sigma)
        assert np.array_equal(X.view(np.float32)[G], new[G].astype(np.float32))
        want = (np.where(G, new - old, 0.0) ** 2).sum(axis=1)
        assert np.array_equal(got, want) and not np.signbit(got).any()


def _region_mask(rng, m, T, empty_rows):
    G = rng.random((m, T)) < 0.3
    G[empty_rows] = False
    return G


@pytest.mark.parametrize("region", ["wave", "workgroup", "everywhere"])
def test_skipped_waves_and_workgroups_change_nothing(L, region):
    """m = 300 is three workgroups (rows 0 .. 127, 128 .. 255, 256 .. 299), T = 100 four tiles and four T splits.  The
    mask is empty in the rows of one wave, of one workgroup, or everywhere: X is untouched there, change_row is exactly
    +0.0 there, and the other rows equal those of a run whose mask is not empty there.  m = 100 is one workgroup."""
    for m in (300, 100):
        T, k = 100, 20
        rows = {"wave": slice(32, 64), "workgroup": slice(128, 256) if m == 300 else slice(0, m),
                "everywhere": slice(0, m)}[region]
        rng = np.random.default_rng(3113)
        G = _region_mask(rng, m, T, rows)
        a = rand_case(np.random.default_rng(3114), m, k, T, 2, None, G, gr.pack_bits(G))
        Xa, cha = a.check(L)
        empty = np.zeros(m, dtype=bool)
        empty[rows] = True
        assert np.array_equal(Xa[empty], a.X0.view(np.uint32)[empty])
        assert (cha[empty] == 0).all() and not np.signbit(cha[empty]).any()
        G2 = G.copy()
        G2[rows] = np.random.default_rng(3115).random((int(empty.sum()), T)) < 0.3
        b = rand_case(np.random.default_rng(3114), m, k, T, 2, None, G2, gr.pack_bits(G2))   # the same operands
        Xb, chb = b.check(L)
        assert np.array_equal(Xa[~empty], Xb[~empty])
        assert np.array_equal(cha[~empty].view(np.uint64), chb[~empty].view(np.uint64))


def test_several_tiles_per_workgroup_with_clustered_gaps():
    """m = 1100 (9 workgroups), T = 8200 (257 tiles): a workgroup walks two tiles, so a wave skips one tile and works in
    the next between the same barriers.  Gaps in boxes of 128 rows x 32 snapshots that do not line up with the tiles,
    through HipKernels on plain tensors; the reference is expand + torch.where on the device."""
    from dmd_era5_amd.kernels import default_kernels

    kern = default_kernels()
    rng = np.random.default_rng(3116)
    m, T, k = 1100, 8200, 20
    G = np.zeros((m, T), dtype=bool)
    for _ in range(60):
        i, t = rng.integers(0, m - 64), rng.integers(0, T - 16)
        G[i:i + 128, t:t + 32] = True
    Ut = torch.from_numpy(rng.standard_normal((k, m)).astype(np.float32)).to(DEV)
    Ct = torch.from_numpy(rng.standard_normal((T, k)).astype(np.float32)).to(DEV)
    mu = torch.from_numpy(rng.standard_normal(m).astype(np.float32)).to(DEV)
    sg = torch.from_numpy((0.5 + rng.random(m)).astype(np.float32)).to(DEV)
    X0 = torch.from_numpy(np.where(G, rng.standard_normal((m, T)).astype(np.float32), payloads(m, T)).T.copy()).to(DEV)
    Gd = torch.from_numpy(np.ascontiguousarray(G.T)).to(DEV)
    W = torch.from_numpy(gr.pack_bits(G).view(np.int32)).to(DEV)
    Xt = X0.clone()
    change = kern.gap_fill_(Ut, Ct, W, Xt, mu, sg)
    Xh = kern.expand(Ut, Ct, mu, sg)
    assert torch.equal(Xt.view(torch.int32), torch.where(Gd, Xh, X0).view(torch.int32))
    d = torch.where(Gd, Xh.double() - X0.double(), torch.zeros((), dtype=F64, device=DEV))
    exact = (d * d).sum(dim=0)
    assert bool(((change - exact).abs() <= gr.CHANGE_C * gr.U24 * exact).all())
    Xt2 = X0.clone()
    assert kern.gap_fill_(Ut, Ct, W, Xt2, mu, sg, want_change=False) is None and torch.equal(Xt2.view(torch.int32), Xt.view(torch.int32))
    change2 = kern.gap_fill_(Ut, Ct, W, X0.clone(), mu, sg)
    assert torch.equal(change2, change)                     # no atomics: the same bits again


def test_refused_calls_write_nothing(L):
    rng = np.random.default_rng(3117)
    c = rand_case(rng, 129, 7, 65, 1, "random")
    need = L.dmdx_gap_fill_workspace_bytes(c.m, c.k, c.T)
    ws = mg.exact_workspace(need, DEV)
    before = c.gX.ibuf.clone()
    short = mg.exact_workspace(need - 8, DEV)
    assert c.fill(L, ws=short) == -1001 and b"dmdx_gap_fill_f32" in L.dmdx_last_error()
    short.check_unused()
    for over in (dict(ldx=c.m - 1), dict(ldw=c.m - 1), dict(k=257)):
        a = dict(ldx=c.gX.ld, ldw=c.gW.ld, k=c.k)
        a.update(over)
        f = list(c._factors())
        f[2] = a["k"]
        rc = L.dmdx_gap_fill_f32(*f, c.gW.ptr, a["ldw"], c.gX.ptr, a["ldx"], c.gch.ptr, ws.ptr, ws.nbytes, _stream())
        torch.cuda.synchronize()
        assert rc == -1000 and b"dmdx_gap_fill_f32" in L.dmdx_last_error(), over
    ws.check_unused()
    assert torch.equal(c.gX.ibuf, before)
    assert bool((c.gch.ibuf == c.gch.canary).all())


@pytest.mark.parametrize("where", ["U", "C", "mu", "sigma", "old"])
def test_non_finite_values_reach_their_row_or_column_only(L, where):
    """The value contract: a non-finite U[i, j], mu[i] or sigma[i] reaches the set-bit elements of row i and
    change_row[i]; a non-finite C[j, t] the set-bit elements of column t and the change_row of their rows; a
    non-finite old value at a set bit change_row[i] and nothing else.  Everything else keeps the bits of the run
    without it."""
    m, k, T = 129, 17, 65
    i0, j0, t0 = 77, 16, 40
    base_rng = np.random.default_rng(3118)
    G, W = make_mask(base_rng, "random", m, T)
    G[i0, t0] = True
    W = gr.pack_bits(G)
    clean = rand_case(np.random.default_rng(3119), m, k, T, 1, None, G, W)
    Xc, chc = clean.check(L)
    for bad in (np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf)):
        c = rand_case(np.random.default_rng(3119), m, k, T, 1, None, G, W)          # the same operands
        hit = np.zeros((m, T), dtype=bool)
        if where == "old":
            c.gX.view[t0, i0] = float(bad)
            c.X0 = c.X0.copy()
            c.X0[i0, t0] = bad
        else:
            g, at = {"U": (c.gU, (j0, i0)), "C": (c.gC, (t0, j0)), "mu": (c.gmu, (0, i0)), "sigma": (c.gsg, (0, i0))}[where]
            g.view[at] = float(bad)
            g.snapshot()
            if where == "C":
                hit[:, t0] = True
            else:
                hit[i0, :] = True
        hit &= G
        X, ch = c.check(L)
        assert not np.isfinite(X.view(np.float32)[hit]).any()
        assert np.array_equal(X[~hit], Xc[~hit])
        rows = hit.any(axis=1)
        if where == "old":
            rows[i0] = True
        assert not np.isfinite(ch[rows]).any()
        assert np.array_equal(ch[~rows].view(np.uint64), chc[~rows].view(np.uint64))
