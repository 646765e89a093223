"""K30 on the GPU: dmdx_varimax_step_f32 and dmdx_row_norms_f32 through the ctypes table.

Shapes (parity with numpy fp64 of the same fp32 inputs inside the bounds of tests/varimax_ref.py), memory (every
operand of every case inside NaN-canary guard zones -- the pads of ldu, ldr and ldg hold NaN -- and an exact 0xFF
workspace: tests/memguard.py), values (exact integers, planted NaN / Inf), determinism.
"""
import numpy as np
import pytest
import torch

import memguard as mg
import varimax_ref as vr

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DEV = "cuda"
E_INVALID, E_WORKSPACE = -1000, -1001

MS = [1, 31, 32, 33, 4095, 4097, 8200]          # chunk edges; 16, 17 and 33 row ranges of 256 rows (the fill rule)
KS = [1, 2, 15, 16, 17, 32, 33, 64]             # block and pad edges
LONG_M = 512 * 4096 + 4097                      # the fill rule leaves the row ranges at their full 4096 rows


@pytest.fixture(scope="module")
def L():
    from dmd_era5_amd.kernels import default_kernels

    return default_kernels()._lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Case:
    """Guarded operands of one call.  layout: 0 tight, 1 padded leading dimensions (multiples of 4: the 16-byte
    loads), 2 odd leading dimensions and bases 1 .. 3 elements past a 16-byte boundary."""

    def __init__(self, U, R, w=None, layout=0):
        self.m, self.k = U.shape
        m, k = self.m, self.k
        pad = {0: 0, 1: 4, 2: 3}[layout]
        off = (lambda j: (1 + j) % 4 if layout == 2 else 0)
        self.U, self.R, self.w = U, R, w
        self.gU = mg.Guarded(m, k, m + pad, F32, off(0), DEV).fill(U).snapshot()
        self.gR = mg.Guarded(k, k, k + pad, F32, off(1), DEV).fill(R).snapshot()
        self.gw = None if w is None else mg.Guarded(m, 1, m, F32, off(2), DEV).fill(w).snapshot()
        self.gG = mg.Guarded(k, k, k + pad, F64, 0, DEV)
        self.gq = mg.Guarded(k, 1, k, F64, 0, DEV)
        self.gf = mg.Guarded(k, 1, k, F64, 0, DEV)
        self.ws = None

    def outputs(self):
        return (self.gG, self.gq, self.gf)

    def clear(self):
        for g in self.outputs():
            g.ibuf.fill_(g.canary)

    def check_inputs(self):
        for g in (self.gU, self.gR, self.gw):
            if g is not None:
                g.check_untouched("input")
                g.check_unchanged("input")

    def run(self, L, accumulate=0, ws=None, **over):
        need = L.dmdx_varimax_workspace_bytes(self.m, self.k)
        assert need > 0
        self.ws = mg.exact_workspace(need, DEV) if ws is None else ws
        a = dict(U=self.gU.ptr, m=self.m, k=self.k, ldu=self.gU.ld, R=self.gR.ptr, ldr=self.gR.ld,
                 w=None if self.gw is None else self.gw.ptr, G=self.gG.ptr, ldg=self.gG.ld, q=self.gq.ptr, f=self.gf.ptr,
                 accumulate=accumulate, wsp=self.ws.ptr, wsb=self.ws.nbytes)
        a.update(over)
        rc = L.dmdx_varimax_step_f32(*a.values(), _stream())
        torch.cuda.synchronize()
        return rc

    def got(self):
        return self.gG.logical(), self.gq.logical()[:, 0], self.gf.logical()[:, 0]

    def bits(self):
        return [g.iview.clone() for g in self.outputs()]


def rand_case(rng, m, k, layout, with_w):
    U = rng.standard_normal((m, k)).astype(np.float32)
    R = rng.standard_normal((k, k)).astype(np.float32)
    w = (0.5 + rng.random(m)).astype(np.float32) if with_w else None
    return Case(U, R, w, layout)


def check_values(c, got=None, tag="", factor=1.0):
    got = c.got() if got is None else got
    want, bound = vr.step64(c.U, c.R, c.w), vr.step_bounds(c.U, c.R, c.w)
    worst = [float((np.abs(g - x) / np.maximum(b, 1e-300)).max()) for g, x, b in zip(got, want, bound)]
    print(f"varimax {tag} m={c.m} k={c.k} w={c.w is not None}: err / bound  G {worst[0]:.3e}  q {worst[1]:.3e}  f {worst[2]:.3e}")
    assert max(worst) <= factor, (c.m, c.k, worst)


def check_step(L, c, tag=""):
    assert c.run(L) == 0, L.dmdx_last_error()
    for g, name in zip(c.outputs(), ("G", "q", "f")):
        g.check_fully_written(name)
        g.check_untouched(name)
    c.ws.check_untouched()
    c.check_inputs()
    check_values(c, tag=tag)


@pytest.mark.parametrize("k", KS)
def test_parity_over_the_shape_edges(L, k):
    rng = np.random.default_rng(3100 + k)
    for im, m in enumerate(MS):
        for with_w in (False, True):
            check_step(L, rand_case(rng, m, k, (im + KS.index(k) + with_w) % 3, with_w))


def test_full_length_row_ranges(L):
    """m beyond 512 x 4096: 514 row ranges of 4096 rows (32 chunks per wave), the last one of one row."""
    rng = np.random.default_rng(3101)
    check_step(L, rand_case(rng, LONG_M, 2, 1, True), tag="long")


def test_shifted_base_gives_the_bits_of_the_aligned_path(L):
    rng = np.random.default_rng(3102)
    for m, k in ((1003, 17), (4097, 50)):
        U = rng.standard_normal((m, k)).astype(np.float32)
        R = rng.standard_normal((k, k)).astype(np.float32)
        w = (0.5 + rng.random(m)).astype(np.float32)
        bits = []
        for shift in (0, 1):
            c = Case(U, R, w, 1)
            c.gU = mg.Guarded(m, k, m + 7 - (m + 3) % 4, F32, shift, DEV).fill(U).snapshot()     # ldu % 4 == 0
            c.gw = mg.Guarded(m, 1, m, F32, shift, DEV).fill(w).snapshot()
            assert c.gU.ld % 4 == 0 and (c.gU.ptr % 16 == 0) == (shift == 0)
            check_step(L, c, tag=f"shift={shift}")
            bits.append(c.bits())
        assert all(torch.equal(a, b) for a, b in zip(*bits))


def test_accumulate_over_row_blocks_and_two_identical_calls(L):
    rng = np.random.default_rng(3103)
    m, k = 3 * 4096 + 7, 50
    c = rand_case(rng, m, k, 1, True)
    check_step(L, c)
    first = c.bits()
    c.clear()
    check_step(L, c)
    assert all(torch.equal(a, b) for a, b in zip(c.bits(), first))
    cut = 6001                                        # the second block starts off a 16-byte boundary
    a = Case(c.U[:cut], c.R, c.w[:cut], 1)
    b = Case(c.U[cut:], c.R, c.w[cut:], 2)
    assert a.run(L) == 0, L.dmdx_last_error()
    assert b.run(L, accumulate=1, G=a.gG.ptr, ldg=a.gG.ld, q=a.gq.ptr, f=a.gf.ptr) == 0, L.dmdx_last_error()
    for g in a.outputs():
        g.check_fully_written()
        g.check_untouched()
    assert all(bool((g.ibuf == g.canary).all()) for g in b.outputs())
    a.ws.check_untouched()
    b.ws.check_untouched()
    check_values(c, a.got(), tag="two blocks")
    for x, y, bound in zip(a.got(), c.got(), vr.step_bounds(c.U, c.R, c.w)):
        assert (np.abs(x - y) <= 2 * bound).all()


def test_f_is_optional_and_refused_calls_write_nothing(L):
    rng = np.random.default_rng(3104)
    c = rand_case(rng, 700, 9, 1, True)
    check_step(L, c)
    full = c.bits()
    c.clear()
    assert c.run(L, f=None) == 0, L.dmdx_last_error()
    assert torch.equal(c.gG.iview, full[0]) and torch.equal(c.gq.iview, full[1]) and bool((c.gf.ibuf == c.gf.canary).all())
    c.clear()
    ws = mg.exact_workspace(L.dmdx_varimax_workspace_bytes(c.m, c.k), DEV)
    bad = [dict(U=None), dict(R=None), dict(G=None), dict(q=None), dict(k=0), dict(k=65), dict(m=0), dict(ldu=c.m - 1),
           dict(ldr=c.k - 1), dict(ldg=c.k - 1), dict(ldu=2 ** 31), dict(ldr=2 ** 31), dict(ldg=2 ** 31),
           dict(m=2 ** 31, ldu=2 ** 31)]
    for over in bad:
        assert c.run(L, ws=ws, **over) == E_INVALID, over
        assert b"dmdx_varimax_step_f32" in L.dmdx_last_error(), over
    assert c.run(L, ws=ws, wsb=ws.nbytes - 1) == E_WORKSPACE
    assert c.run(L, ws=ws, wsp=None) == E_WORKSPACE
    ws.check_unused()
    ws.check_untouched()
    assert all(bool((g.ibuf == g.canary).all()) for g in c.outputs())
    c.check_inputs()


# ---------------------------------------------------------------- exact integers
@pytest.mark.parametrize("m,k,layout,i0", [(5000, 37, 2, 4999), (5000, 64, 1, 256), (5000, 5, 0, 255)])
def test_exact_integers(L, m, k, layout, i0):
    """U in {-1, 0, 1}, R = 2 x a signed permutation, w a power of two (1, 2 or 1/2): L = +-2 a, every product and
    every partial sum of every order an integer (or a multiple of 2^-4) far below 2^24, so the result is exact --
    bit for bit the integer arithmetic.  The factor 2 tells L^3 (8 a^3) from L (2 a).  Row i0 (the last row, the
    first and the last of a row range) is planted with U = 1 and w = 2: dropped or counted twice it changes every sum."""
    rng = np.random.default_rng(3105)
    U = rng.integers(-1, 2, (m, k)).astype(np.float32)
    w = (2.0 ** rng.integers(-1, 2, m)).astype(np.float32)
    U[i0], w[i0] = 1.0, 2.0
    R = np.zeros((k, k), dtype=np.float32)
    R[rng.permutation(k), np.arange(k)] = 2.0 * rng.choice([-1.0, 1.0], k)
    a = U.astype(np.float64) * w.astype(np.float64)[:, None]               # multiples of 1/2, |a| <= 2
    Lx = a @ R.astype(np.float64)                                          # integers, |L| <= 4
    want = (a.T @ Lx ** 3, (Lx ** 2).sum(axis=0), (Lx ** 4).sum(axis=0))   # exact in fp64: < 2^21
    assert max(np.abs(x).max() for x in want) < 2 ** 21
    c = Case(U, R, w, layout)
    assert c.run(L) == 0, L.dmdx_last_error()
    for got, x in zip(c.got(), want):
        assert np.array_equal(got, x)
    first = c.bits()
    assert c.run(L) == 0
    assert all(torch.equal(x, y) for x, y in zip(c.bits(), first))
    c.ws.check_untouched()
    c.check_inputs()


# ---------------------------------------------------------------- NaN / Inf
def _cls(a):
    a = np.asarray(a, dtype=np.float64)
    return np.where(np.isnan(a), 3, np.where(np.isposinf(a), 1, np.where(np.isneginf(a), 2, 0)))


PLANTS = [("U", np.nan), ("U", np.inf), ("U", -np.inf), ("U_last", np.inf), ("w", np.nan), ("w", np.inf), ("w_last", -np.inf),
          ("R", np.nan), ("R", np.inf), ("R", -np.inf), ("R_last", np.inf)]


def test_planted_nan_and_inf(L):
    """m = 150 is no multiple of the 32-row chunk and k = 37 none of the 32-column block: the "_last" plants sit next
    to the zero rows of the last chunk and the zero columns of the pad.  U and w: every output is non-finite.  R[j, c]:
    column c of G, q[c] and f[c] are; every other output keeps the bits of the clean run.  The class of each is
    numpy fp64's."""
    rng = np.random.default_rng(3106)
    m, k = 150, 37
    base = rand_case(rng, m, k, 2, True)
    assert (base.U != 0).all() and (base.R != 0).all()
    assert base.run(L) == 0
    clean = base.got()
    i0, j0, c0 = 77, 11, 5
    with np.errstate(all="ignore"):
        for what, val in PLANTS:
            U, R, w = base.U.copy(), base.R.copy(), base.w.copy()
            same = [np.zeros((k, k), dtype=bool), np.zeros(k, dtype=bool), np.zeros(k, dtype=bool)]
            if what[0] == "U":
                i, j = (m - 1, k - 1) if what == "U_last" else (i0, j0)
                U[i, j] = val
            elif what[0] == "w":
                w[m - 1 if what == "w_last" else i0] = val
            else:
                j, c = (k - 1, k - 1) if what == "R_last" else (j0, c0)
                R[j, c] = val
                for s in same:
                    s[...] = True
                same[0][:, c] = False
                same[1][c] = same[2][c] = False
            case = Case(U, R, w, 2)
            assert case.run(L) == 0, L.dmdx_last_error()
            got, want = case.got(), vr.step64(U, R, w)
            for g, x, s, cl in zip(got, want, same, clean):
                assert np.array_equal(_cls(g), _cls(x)), (what, val)
                assert (_cls(g)[~s] != 0).all(), (what, val)
                assert np.array_equal(g.view(np.int64)[s], cl.view(np.int64)[s]), (what, val)


ONE_SIGN_PLANTS = [("U", np.inf), ("U", -np.inf), ("U", np.nan), ("U_last", np.inf), ("w", np.inf), ("w", -np.inf),
                   ("w", np.nan), ("w_last", np.inf), ("R", np.inf), ("R", -np.inf), ("R", np.nan), ("R_last", -np.inf)]


@pytest.mark.parametrize("k", [1, 33, 64])
def test_planted_inf_keeps_its_sign_next_to_the_pads(L, k):
    """U, R and w all positive, so that no sum of the fp64 evaluation meets Inf - Inf: numpy gives +Inf or -Inf, not
    NaN, wherever an Inf reaches, and the kernel must give the same class -- a 0 * Inf in a pad column or a pad row
    (k = 1 and k = 33 leave 31 pad columns, m = 150 leaves 10 pad rows; k = 64 leaves no pad column) would turn them
    into NaN.  R[j, c]: the other columns keep the bits of the clean run."""
    rng = np.random.default_rng(3109 + k)
    m = 150
    U = (0.5 + rng.random((m, k))).astype(np.float32)
    R = (0.5 + rng.random((k, k))).astype(np.float32)
    w = (0.5 + rng.random(m)).astype(np.float32)
    base = Case(U, R, w, 2)
    assert base.run(L) == 0
    clean = base.got()
    i0, j0, c0 = 77, k // 3, k // 2
    with np.errstate(all="ignore"):
        for what, val in ONE_SIGN_PLANTS:
            Up, Rp, wp = U.copy(), R.copy(), w.copy()
            same = [np.zeros((k, k), dtype=bool), np.zeros(k, dtype=bool), np.zeros(k, dtype=bool)]
            if what[0] == "U":
                i, j = (m - 1, k - 1) if what == "U_last" else (i0, j0)
                Up[i, j] = val
            elif what[0] == "w":
                wp[m - 1 if what == "w_last" else i0] = val
            else:
                j, c = (k - 1, k - 1) if what == "R_last" else (j0, c0)
                Rp[j, c] = val
                for s in same:
                    s[...] = True
                same[0][:, c] = False
                same[1][c] = same[2][c] = False
            case = Case(Up, Rp, wp, 2)
            assert case.run(L) == 0, L.dmdx_last_error()
            got, want = case.got(), vr.step64(Up, Rp, wp)
            for g, x, s, cl in zip(got, want, same, clean):
                assert np.array_equal(_cls(g), _cls(x)), (what, val, _cls(g), _cls(x))
                assert (_cls(g)[~s] != 0).all(), (what, val)
                assert np.array_equal(g.view(np.int64)[s], cl.view(np.int64)[s]), (what, val)
            if not np.isnan(val):      # the inputs do what they are for: numpy's answer is a signed Inf, nowhere a NaN
                assert all(((_cls(x) == 1) | (_cls(x) == 2))[~s].all() for x, s in zip(want, same)), (what, val)
        # without w the same plants in U and R
        for what, val in [p for p in ONE_SIGN_PLANTS if p[0][0] != "w"]:
            Up, Rp = U.copy(), R.copy()
            if what[0] == "U":
                Up[(m - 1, k - 1) if what == "U_last" else (i0, j0)] = val
            else:
                Rp[(k - 1, k - 1) if what == "R_last" else (j0, c0)] = val
            case = Case(Up, Rp, None, 1)
            assert case.run(L) == 0, L.dmdx_last_error()
            for g, x in zip(case.got(), vr.step64(Up, Rp)):
                assert np.array_equal(_cls(g), _cls(x)), (what, val)


# ---------------------------------------------------------------- row norms
@pytest.mark.parametrize("m,k,layout", [(1, 1, 0), (33, 5, 1), (1027, 50, 1), (1027, 50, 2), (4099, 64, 0), (700, 200, 2)])
def test_row_norms_bit_for_bit(L, m, k, layout):
    rng = np.random.default_rng(3107)
    U = (rng.standard_normal((m, k)) * 10.0 ** rng.integers(-3, 4, (m, 1))).astype(np.float32)
    U[m // 2] = 0.0
    cs = (0.1 + 5.0 * rng.random(k)).astype(np.float32)
    pad, off = {0: 0, 1: 4 + (-m) % 4, 2: 3}[layout], (1 if layout == 2 else 0)
    gU = mg.Guarded(m, k, m + pad, F32, off, DEV).fill(U).snapshot()
    gc = mg.Guarded(k, 1, k, F32, off, DEV).fill(cs).snapshot()
    for scale in (None, cs):
        gh = mg.Guarded(m, 1, m, F32, 0, DEV)
        rc = L.dmdx_row_norms_f32(gU.ptr, m, k, gU.ld, None if scale is None else gc.ptr, gh.ptr, _stream())
        torch.cuda.synchronize()
        assert rc == 0, L.dmdx_last_error()
        gh.check_fully_written("h")
        gh.check_untouched("h")
        assert np.array_equal(gh.logical()[:, 0].view(np.int32), vr.row_norms(U, scale).view(np.int32))
    for g in (gU, gc):
        g.check_untouched("input")
        g.check_unchanged("input")


# ---------------------------------------------------------------- the wrapper
def test_wrapper_matches_the_reference():
    from dmd_era5_amd.kernels import default_kernels

    kern = default_kernels()
    rng = np.random.default_rng(3108)
    m, k = 1111, 6
    Ubig = rng.standard_normal((k, m + 7)).astype(np.float32)
    R = rng.standard_normal((k, k)).astype(np.float32)
    w = (0.5 + rng.random(m)).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)          # noqa: E731
    Ut, U = t(Ubig)[:, 3:3 + m], Ubig[:, 3:3 + m].T
    Gt, q, f = kern.varimax_step(Ut, t(R.T), t(w))
    want, bound = vr.step64(U, R, w), vr.step_bounds(U, R, w)
    for got, x, b in zip((Gt.cpu().numpy().T, q.cpu().numpy(), f.cpu().numpy()), want, bound):
        assert (np.abs(got - x) <= b).all()
    again = kern.varimax_step(Ut, t(R.T), t(w), out=(Gt.clone(), q.clone(), f.clone()))
    assert torch.equal(again[0], 2 * Gt) and torch.equal(again[1], 2 * q) and torch.equal(again[2], 2 * f)
    G2, q2, none = kern.varimax_step(Ut, t(R.T), t(w), want_f=False)
    assert none is None and torch.equal(G2, Gt) and torch.equal(q2, q)
    assert kern.varimax_max_k == 64
    h = kern.row_norms(Ut, t(w[:k]))
    assert np.array_equal(h.cpu().numpy(), vr.row_norms(U, w[:k]))
    assert np.array_equal(kern.row_norms(Ut, out=h).cpu().numpy(), vr.row_norms(U))
    with pytest.raises(Exception):
        kern.varimax_step(Ut, t(R.T)[:, :-1], t(w))
    with pytest.raises(Exception):
        kern.varimax_step(Ut, t(R.T), t(w), out=(Gt, q, None))
