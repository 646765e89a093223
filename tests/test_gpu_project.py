"""K13 on the GPU: dmdx_project_f32 through the ctypes table, and the host layer above it.

Shapes (parity with numpy fp64 of the same fp32 inputs, bounds of tests/project_ref.py), memory (operands
inside NaN-canary guard zones, exact 0xFF workspaces: tests/memguard.py), values (exact integers, planted
NaN / Inf, power-of-two scaling, bit-equality of the standardised values with K5).  Every operand of every
case lives in a guarded allocation, so each parity case is a memory-edge case as well.
"""
import itertools

import numpy as np
import pytest
import torch

import memguard as mg
import project_ref as pr

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DEV = "cuda"
E_INVALID, E_WORKSPACE = -1000, -1001
R = pr.FP32_ROWS

MS = [1, 3, 31, 32, 33, 63, 65, 127, 129, 257, 1003, R + 33]
TS = [1, 2, 15, 16, 17, 33, 127, 129, 300]


@pytest.fixture(scope="module")
def L():
    from dmd_era5_amd.kernels import default_kernels

    return default_kernels()._lib


def _ks(L):
    return [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 50, 64, 65, 200, int(L.dmdx_project_max_k())]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def delay_flat(X, ldx):
    """The flat buffer of a delay view: rows > ldx, X[i, t] = flat[i + t * ldx] must be consistent."""
    m, T = X.shape
    flat = np.zeros((T - 1) * ldx + m, dtype=np.float32)
    for t in range(T):
        flat[t * ldx:t * ldx + m] = X[:, t]
    return flat


def delay_matrix(rng, m, T, ldx):
    flat = (280.0 + 10.0 * rng.standard_normal((T - 1) * ldx + m)).astype(np.float32)
    return np.stack([flat[t * ldx:t * ldx + m] for t in range(T)], axis=1)


class Case:
    """Guarded operands of one call.  layout: 0 tight, 1 padded leading dimensions (multiples of 4),
    2 odd leading dimensions and bases 1 .. 3 elements past a 16-byte boundary, 3 as 1 without mu / sigma."""

    def __init__(self, m, k, T, layout, U, X, mu=None, sigma=None, delay_ldx=None):
        self.m, self.k, self.T = m, k, T
        pad = {0: 0, 1: 4, 2: 3, 3: 8}[layout]
        off = (lambda j: (1 + j) % 4 if layout == 2 else 0)
        self.U, self.X, self.mu, self.sigma = U, X, mu, sigma
        self.gU = mg.Guarded(m, k, m + pad, F32, off(0), DEV).fill(U).snapshot()
        self.gmu = None if mu is None else mg.Guarded(m, 1, m, F32, off(2), DEV).fill(mu).snapshot()
        self.gsg = None if sigma is None else mg.Guarded(m, 1, m, F32, off(0), DEV).fill(sigma).snapshot()
        if delay_ldx is None:
            self.gX = mg.Guarded(m, T, m + pad, F32, off(1), DEV).fill(X).snapshot()
        else:   # rows > ldx: X[i, t] = flat[i + t * ldx]
            self.gX = mg.Guarded(m, T, delay_ldx, F32, off(1), DEV)
            self.gX.fbuf[self.gX.start:self.gX.start + self.gX.region] = torch.from_numpy(delay_flat(X, delay_ldx)).to(DEV)
            self.gX.snapshot()
        self.gC = mg.Guarded(k, T, k + pad, F64, 0, DEV)
        self.gE = mg.Guarded(T, 1, T, F64, 0, DEV)
        self.ws = None

    def inputs(self):
        return [g for g in (self.gU, self.gX, self.gmu, self.gsg) if g is not None]

    def check_inputs(self):
        for g in self.inputs():
            g.check_untouched("input")
            g.check_unchanged("input")

    def run(self, L, accumulate=0, energy=True, ws=None, mu=True, sigma=True, **over):
        need = L.dmdx_project_workspace_bytes(self.m, self.k, self.T)
        assert need > 0
        self.ws = mg.exact_workspace(need, DEV) if ws is None else ws
        a = dict(U=self.gU.ptr, m=self.m, k=self.k, ldu=self.gU.ld, X=self.gX.ptr, ldx=self.gX.ld, T=self.T,
                 mu=None if self.gmu is None or not mu else self.gmu.ptr,
                 sigma=None if self.gsg is None or not sigma else self.gsg.ptr,
                 C=self.gC.ptr, ldc=self.gC.ld, E=self.gE.ptr if energy else None, wsp=self.ws.ptr, wsb=self.ws.nbytes)
        a.update(over)
        rc = L.dmdx_project_f32(a["U"], a["m"], a["k"], a["ldu"], a["X"], a["ldx"], a["T"], a["mu"], a["sigma"], a["C"],
                                a["ldc"], a["E"], accumulate, a["wsp"], a["wsb"], _stream())
        torch.cuda.synchronize()
        return rc

    def c(self):
        return self.gC.logical()

    def e(self):
        return self.gE.logical()[:, 0]


def rand_case(rng, m, k, T, layout, delay_ldx=None):
    """Un-centred data, X = 280 + O(10), mu and sigma of that scale."""
    U = rng.standard_normal((m, k)).astype(np.float32)
    X = (280.0 + 10.0 * rng.standard_normal((m, T))).astype(np.float32) if delay_ldx is None else \
        delay_matrix(rng, m, T, delay_ldx)
    mu = sigma = None
    if layout != 3:
        mu = (280.0 + 3.0 * rng.standard_normal(m)).astype(np.float32)
        sigma = (5.0 + 10.0 * rng.random(m)).astype(np.float32)
    return Case(m, k, T, layout, U, X, mu, sigma, delay_ldx)


def parity_shapes(L):
    """All (m, k) pairs and all (k, T) pairs of the edge lists, the third size and the layout cycling: every
    value of every list meets every k and every layout."""
    ks = _ks(L)
    out = []
    for (im, m), (ik, k) in itertools.product(enumerate(MS), enumerate(ks)):
        out.append((m, k, TS[(im + 2 * ik) % len(TS)], (im + ik) % 4))
    for (ik, k), (it, T) in itertools.product(enumerate(ks), enumerate(TS)):
        out.append((MS[(2 * ik + it) % len(MS)], k, T, (ik + it + 1) % 4))
    return out


def check_values(c, mu=True, sigma=True, energy=True, tag=""):
    muv, sgv = (c.mu if mu else None), (c.sigma if sigma else None)
    errC = np.abs(c.c() - pr.project64(c.U, c.X, muv, sgv))
    bC = pr.project_bound(c.U, c.X, muv, sgv)
    worst = float((errC / np.maximum(bC, 1e-300)).max())
    if energy:
        errE = np.abs(c.e() - pr.energy64(c.X, muv, sgv))
        bE = pr.energy_bound(c.X, muv, sgv)
        worst_e = float((errE / np.maximum(bE, 1e-300)).max())
    else:
        worst_e = 0.0
    print(f"project {tag} m={c.m} k={c.k} T={c.T}: err / bound  C {worst:.3e}  energy {worst_e:.3e}")
    assert worst <= 1.0 and worst_e <= 1.0, (c.m, c.k, c.T, worst, worst_e)


def check_project(L, c):
    assert c.run(L) == 0, L.dmdx_last_error()
    for g, name in ((c.gC, "C"), (c.gE, "energy")):
        g.check_fully_written(name)
        g.check_untouched(name)
    c.ws.check_untouched()
    c.check_inputs()
    check_values(c)


def test_layout_cover():
    """Every value of each axis meets every layout in the parity list (pure bookkeeping, checked on the GPU box
    only because the list needs max_k of the library)."""
    from dmd_era5_amd import _lib

    shapes = parity_shapes(_lib.load())
    for axis, vals in ((0, MS), (1, _ks(_lib.load())), (2, TS)):
        for v in vals:
            assert {s[3] for s in shapes if s[axis] == v} == {0, 1, 2, 3}, (axis, v)


def test_parity_over_the_shape_edges(L):
    rng = np.random.default_rng(1301)
    for m, k, T, layout in parity_shapes(L):
        check_project(L, rand_case(rng, m, k, T, layout))


def test_several_units_row_ranges_and_tiles(L):
    """m = 3 R + 7 (49 row ranges: with three tiles of snapshots the fill rule shortens them to 256 rows), T = 300,
    k = 50: accumulate over two row blocks equals the single call on the stacked rows within the bound; two
    identical calls are bit-identical."""
    rng = np.random.default_rng(1302)
    m, k, T = 3 * R + 7, 50, 300
    c = rand_case(rng, m, k, T, 1)
    check_project(L, c)
    first = (c.gC.iview.clone(), c.gE.iview.clone())
    c.gC.ibuf.fill_(c.gC.canary)
    c.gE.ibuf.fill_(c.gE.canary)
    check_project(L, c)
    assert torch.equal(c.gC.iview, first[0]) and torch.equal(c.gE.iview, first[1])
    single_C, single_E = c.c(), c.e()
    cut = 6001                                        # the second block starts off a 16-byte boundary
    a = Case(cut, k, T, 1, c.U[:cut], c.X[:cut], c.mu[:cut], c.sigma[:cut])
    b = Case(m - cut, k, T, 2, c.U[cut:], c.X[cut:], c.mu[cut:], c.sigma[cut:])
    assert a.run(L) == 0, L.dmdx_last_error()
    assert b.run(L, accumulate=1, C=a.gC.ptr, ldc=a.gC.ld, E=a.gE.ptr) == 0, L.dmdx_last_error()
    for g in (a.gC, a.gE):
        g.check_fully_written()
        g.check_untouched()
    assert bool((b.gC.ibuf == b.gC.canary).all()) and bool((b.gE.ibuf == b.gE.canary).all())
    a.ws.check_untouched()
    b.ws.check_untouched()
    bC, bE = pr.project_bound(c.U, c.X, c.mu, c.sigma), pr.energy_bound(c.X, c.mu, c.sigma)
    assert (np.abs(a.c() - pr.project64(c.U, c.X, c.mu, c.sigma)) <= bC).all()
    assert (np.abs(a.e() - pr.energy64(c.X, c.mu, c.sigma)) <= bE).all()
    assert (np.abs(a.c() - single_C) <= 2 * bC).all() and (np.abs(a.e() - single_E) <= 2 * bE).all()


def test_delay_view_and_optional_operands(L):
    """X with rows > ldx (the zero-copy delay view); energy left out; every null combination of mu / sigma."""
    rng = np.random.default_rng(1303)
    m, k, T, ldx = 300, 20, 45, 100
    for layout in (0, 2):
        c = rand_case(rng, m, k, T, layout, delay_ldx=ldx + (layout == 2))
        check_project(L, c)
        for mu, sigma in ((True, False), (False, True), (False, False)):
            c.gC.ibuf.fill_(c.gC.canary)
            c.gE.ibuf.fill_(c.gE.canary)
            assert c.run(L, mu=mu, sigma=sigma) == 0, L.dmdx_last_error()
            c.gC.check_fully_written("C")
            c.gE.check_fully_written("energy")
            check_values(c, mu, sigma, tag=f"mu={mu} sigma={sigma}")
        withE = c.gC.iview.clone()
        before = c.gE.iview.clone()
        c.gC.ibuf.fill_(c.gC.canary)
        assert c.run(L, mu=False, sigma=False, energy=False) == 0, L.dmdx_last_error()
        assert torch.equal(c.gE.iview, before) and torch.equal(c.gC.iview, withE)
        c.gC.check_untouched("C")
        c.gE.check_untouched("energy")
        c.ws.check_untouched()
        c.check_inputs()


def test_refused_calls_write_nothing(L):
    rng = np.random.default_rng(1304)
    c = rand_case(rng, 70, 9, 40, 1)
    kmax = int(L.dmdx_project_max_k())
    ws = mg.exact_workspace(L.dmdx_project_workspace_bytes(c.m, c.k, c.T), DEV)
    bad = [dict(U=None), dict(X=None), dict(C=None), dict(k=0), dict(k=kmax + 1), dict(ldu=c.m - 1), dict(ldc=c.k - 1),
           dict(ldx=0), dict(m=0), dict(T=0), dict(ldu=2 ** 31), dict(ldx=2 ** 31), dict(ldc=2 ** 31),
           dict(m=2 ** 31, ldu=2 ** 31), dict(T=2 ** 31)]
    for over in bad:
        assert c.run(L, ws=ws, **over) == E_INVALID, over
        assert b"project" in L.dmdx_last_error(), over
    assert c.run(L, ws=ws, wsb=ws.nbytes - 1) == E_WORKSPACE
    assert b"project" in L.dmdx_last_error()
    assert c.run(L, ws=ws, wsp=None) == E_WORKSPACE
    ws.check_unused()
    ws.check_untouched()
    for g in (c.gC, c.gE):
        assert bool((g.ibuf == g.canary).all())
    c.check_inputs()


# ---------------------------------------------------------------- exact integers
def int_case(rng, m, k, T, layout, i0):
    """U in [-2, 2], xt in [-3, 3], sigma in {1, 2, 4}, integer mu, X = mu + sigma xt; row i0 is planted with
    U = 2 and xt = 1000 + t % 7: m a_U a_xt < 5000 * 2 * 3 + 2 * 1006 and sum xt^2 < 5000 * 9 + 1006^2, every
    partial sum of every order an integer below 2^24, X below 2^13."""
    U = rng.integers(-2, 3, (m, k)).astype(np.float32)
    Z = rng.integers(-3, 4, (m, T))
    U[i0] = 2.0
    Z[i0] = 1000 + np.arange(T) % 7
    mu = rng.integers(-300, 301, m)
    sigma = rng.choice([1, 2, 4], m)
    X = mu[:, None] + sigma[:, None] * Z
    assert np.abs(X).max() < 2 ** 13 and (np.abs(U).astype(np.int64).T @ np.abs(Z)).max() < 2 ** 24
    assert (Z * Z).sum(axis=0).max() < 2 ** 24
    c = Case(m, k, T, layout, U, X.astype(np.float32), mu.astype(np.float32), sigma.astype(np.float32))
    c.want = (U.astype(np.int64).T @ Z, (Z * Z).sum(axis=0))
    return c


@pytest.mark.parametrize("shape", [(5000, 37, 70, 2, 4999), (5000, 200, 129, 1, 256), (5000, 5, 300, 0, 255)])
def test_exact_integers(L, shape):
    """Bit-exact against integer arithmetic at m = 5000 (20 row ranges of 256 rows at these T): the planted row
    (the last one, the first of a range, the last of a range) dropped or counted twice changes every sum by
    ~2000 / ~10^6.  Two runs give the same bits."""
    c = int_case(np.random.default_rng(1305), *shape)
    assert c.run(L) == 0, L.dmdx_last_error()
    assert np.array_equal(c.c(), c.want[0].astype(np.float64)) and np.array_equal(c.e(), c.want[1].astype(np.float64))
    firsts = [g.iview.clone() for g in (c.gC, c.gE)]
    assert c.run(L) == 0
    for g, f in zip((c.gC, c.gE), firsts):
        assert torch.equal(g.iview, f)
    c.ws.check_untouched()
    c.check_inputs()


# ---------------------------------------------------------------- NaN / Inf, scaling
def _cls(a):
    a = np.asarray(a, dtype=np.float64)
    return np.where(np.isnan(a), 3, np.where(np.isposinf(a), 1, np.where(np.isneginf(a), 2, 0)))


PLANTS = [("X", np.nan), ("X", np.inf), ("X", -np.inf), ("X_last", np.inf), ("U", np.nan), ("U", np.inf), ("U_last", -np.inf),
          ("mu", np.nan), ("mu", np.inf), ("sigma", np.nan), ("sigma", np.inf), ("sigma", 0.0), ("sigma_last", 0.0)]


def test_planted_nan_and_inf(L):
    """m = 150 is no multiple of the 32-row chunk and k = 37 none of the 32-column block: "X_last" / "sigma_last"
    plant in the last row, next to the zero rows of the last chunk, "U_last" in the last real column of U, next
    to its zero pad.  Class of every output = numpy fp64's; outputs the element does not take part in keep the
    bits of the clean run."""
    rng = np.random.default_rng(1306)
    m, k, T = 150, 37, 70
    base = rand_case(rng, m, k, T, 2)
    tie = base.X == base.mu[:, None]      # ~1e-6 per element at this scale: move a drawn x = mu one ulp up
    if tie.any():
        base = Case(m, k, T, 2, base.U, np.where(tie, np.nextafter(base.X, np.float32(np.inf)), base.X), base.mu, base.sigma)
    assert (base.X != base.mu[:, None]).all() and (base.U != 0).all()
    assert base.run(L) == 0
    cleanC, cleanE = base.c(), base.e()
    i0, j0, t0 = 77, 11, 41
    with np.errstate(all="ignore"):
        for what, val in PLANTS:
            U, X, mu, sigma = base.U.copy(), base.X.copy(), base.mu.copy(), base.sigma.copy()
            i = m - 1 if what.endswith("_last") and what[0] != "U" else i0
            sameC, sameE = np.ones((k, T), dtype=bool), np.ones(T, dtype=bool)
            if what in ("X", "X_last"):
                X[i, t0] = val
                sameC[:, t0] = False
                sameE[t0] = False
            elif what in ("U", "U_last"):
                j = k - 1 if what == "U_last" else j0
                U[i, j] = val
                sameC[j, :] = False
            else:
                (mu if what == "mu" else sigma)[i] = val
                sameC[:], sameE[:] = False, False
            c = Case(m, k, T, 2, U, X, mu, sigma)
            assert c.run(L) == 0, L.dmdx_last_error()
            gotC, gotE = c.c(), c.e()
            assert np.array_equal(_cls(gotC), _cls(pr.project64(U, X, mu, sigma))), (what, val)
            assert np.array_equal(_cls(gotE), _cls(pr.energy64(X, mu, sigma))), (what, val)
            assert np.array_equal(gotC.view(np.int64)[sameC], cleanC.view(np.int64)[sameC]), (what, val)
            assert np.array_equal(gotE.view(np.int64)[sameE], cleanE.view(np.int64)[sameE]), (what, val)
            if what == "sigma" and val == np.inf:      # a row that standardises to exact zeros: everything finite
                assert (_cls(gotC) == 0).all() and (_cls(gotE) == 0).all()


def test_power_of_two_scaling_commutes(L):
    rng = np.random.default_rng(1307)
    m, k, T = 200, 50, 45
    base = rand_case(rng, m, k, T, 1)
    assert base.run(L) == 0
    for e in (20, -20):        # (2^e X, 2^e mu, 2^e sigma): the standardised values are the same bits
        f = np.float32(2.0 ** e)
        c = Case(m, k, T, 1, base.U, base.X * f, base.mu * f, base.sigma * f)
        assert c.run(L) == 0
        assert torch.equal(c.gC.iview, base.gC.iview) and torch.equal(c.gE.iview, base.gE.iview)
    for e in (40, -40):        # 2^e U: exactly 2^e C, the energy does not see U
        c = Case(m, k, T, 1, base.U * np.float32(2.0 ** e), base.X, base.mu, base.sigma)
        assert c.run(L) == 0
        assert np.array_equal(c.c(), base.c() * 2.0 ** e) and torch.equal(c.gE.iview, base.gE.iview)


def test_composition_with_k5_and_k3(L):
    """xt is bit for bit what K5 leaves in place: with U = the identity every C[j, t] is ONE product 1 * xt[j, t]
    plus exact zeros, so C equals K5's output exactly.  Then a random U: project with K5's mean and std against
    K3 (gemm_tn) on K5's output, within the sum of both bounds (K3: (min(K, 4096) / 2 + 18) 2^-24 sum |a||b|,
    include/dmdx.h)."""
    rng = np.random.default_rng(1308)
    m, T = 200, 96
    X = (280.0 + 10.0 * rng.standard_normal((m, T))).astype(np.float32)
    for layout in (1, 2):
        gK5 = mg.Guarded(m, T, m + {1: 4, 2: 3}[layout], F32, layout == 2, DEV).fill(X)
        mean, std = torch.empty(m, device=DEV), torch.empty(m, device=DEV)
        assert L.dmdx_row_center_scale_f32(gK5.ptr, m, T, gK5.ld, mean.data_ptr(), std.data_ptr(), 1, _stream()) == 0
        torch.cuda.synchronize()
        Xt = gK5.logical()                                         # K5's standardised matrix, (m, T) fp32
        mu, sd = mean.cpu().numpy(), std.cpu().numpy()
        c = Case(m, m, T, layout, np.eye(m, dtype=np.float32), X, mu, sd)
        assert c.run(L) == 0, L.dmdx_last_error()
        assert np.array_equal(c.c(), Xt.astype(np.float64))
        k = 50
        U = rng.standard_normal((m, k)).astype(np.float32)
        c = Case(m, k, T, layout, U, X, mu, sd)
        assert c.run(L) == 0, L.dmdx_last_error()
        gU, gC3 = c.gU, mg.Guarded(k, T, k, F64, 0, DEV)
        ws = mg.exact_workspace(L.dmdx_gemm_tn_workspace_bytes(m, k, T), DEV)
        assert L.dmdx_gemm_tn_f32(gU.ptr, gU.ld, gK5.ptr, gK5.ld, m, k, T, gC3.ptr, gC3.ld, None, 0, 0, ws.ptr, ws.nbytes,
                                  _stream()) == 0, L.dmdx_last_error()
        torch.cuda.synchronize()
        A = np.abs(U).astype(np.float64).T @ np.abs(Xt).astype(np.float64)
        bound = ((R + 4) + (min(m, 4096) / 2 + 18)) * pr.U24 * A
        assert (np.abs(c.c() - gC3.logical()) <= bound).all()


# ---------------------------------------------------------------- the host layer
@pytest.fixture(scope="module")
def KERN():
    from dmd_era5_amd.kernels import default_kernels

    return default_kernels()


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def test_wrapper_matches_the_double(KERN):
    """HipKernels.project: a U view with a row stride, the delay view of X, accumulation into ``out``, no energy."""
    from dmd_era5_amd.svd import embed_view

    rs = np.random.RandomState(0)
    mb, d, k, n = 111, 3, 5, 43
    m, T = d * mb, n - d + 1
    Xraw = (280.0 + 10.0 * rs.standard_normal((n, mb))).astype(np.float32)
    Ubig = rs.standard_normal((k, m + 7)).astype(np.float32)
    mu, sd = (280.0 + rs.standard_normal(m)).astype(np.float32), (5.0 + 10.0 * rs.rand(m)).astype(np.float32)
    Ut, E = _t(Ubig)[:, 3:3 + m], embed_view(_t(Xraw), d)
    assert E.shape == (T, m)
    U, X = Ubig[:, 3:3 + m].T, np.concatenate([Xraw[j:j + T] for j in range(d)], axis=1).T
    Ct, energy = KERN.project(Ut, E, _t(mu), _t(sd))
    assert Ct.shape == (T, k) and Ct.dtype == torch.float64 and energy.shape == (T,)
    assert (np.abs(Ct.cpu().numpy().T - pr.project64(U, X, mu, sd)) <= pr.project_bound(U, X, mu, sd)).all()
    assert (np.abs(energy.cpu().numpy() - pr.energy64(X, mu, sd)) <= pr.energy_bound(X, mu, sd)).all()
    dbl = pr.ProjectDouble().project(Ut, E, _t(mu), _t(sd))
    assert (np.abs(Ct.cpu().numpy() - dbl[0].numpy()) <= pr.project_bound(U, X, mu, sd).T).all()
    again = KERN.project(Ut, E, _t(mu), _t(sd), out=(Ct.clone(), energy.clone()))
    assert torch.equal(again[0], 2 * Ct) and torch.equal(again[1], 2 * energy)
    C2, none = KERN.project(Ut, E, _t(mu), _t(sd), want_energy=False)
    assert none is None and torch.equal(C2, Ct)
    assert KERN.project_max_k == 256
    with pytest.raises(Exception):
        KERN.project(Ut, E[:, :-1], _t(mu), _t(sd))
    with pytest.raises(Exception):
        KERN.project(Ut, E, _t(mu), _t(sd), out=(Ct, None))


def test_project_blocks_after_svd_snapshots_returns_s_vh(KERN):
    """2000 x 96, rank 10: U^T X of the training snapshots is diag(s) Vh.  Tolerance, per element (j, t), derived:
    the stated fp32 tolerance of the SVD, 64 eps32 s_1^2 / s_j (it bounds the eigen-residual
    S^-1 (V^T G - S^2 V^T) that U^T X - S Vh consists of when U = X V S^-1), + K13's own bound + the bound of
    the K2 product U = X (V S^-1) over n = 96 terms carried through U^T X: (n + 2) u (|X| |V| / s)^T |X|."""
    from dmd_era5_amd import svd as dsvd
    from dmd_era5_amd.forecast import project_blocks

    rs = np.random.RandomState(1)
    m, n, r = 2000, 96, 10
    X = (rs.standard_normal((m, r)) @ (np.diag(np.linspace(30, 3, r)) @ rs.standard_normal((r, n)))
         + 0.5 * rs.standard_normal((m, n))).astype(np.float32)
    Xt = _t(X.T)
    res = dsvd.svd_snapshots(Xt, r)
    blocks = [(0, 801), (801, 2000)]
    out = project_blocks([res.Ut[:, a:b] for a, b in blocks], [Xt[:, a:b] for a, b in blocks])
    s, Vh, U = res.s.cpu().numpy(), res.Vh.cpu().numpy(), res.Ut.cpu().numpy().T.astype(np.float64)
    X64 = X.astype(np.float64)
    tol = (64 * 2.0 ** -24 * s[0] ** 2 / s)[:, None] + pr.project_bound(U, X) \
        + (n + 2) * pr.U24 * ((np.abs(X64) @ np.abs(Vh.T) / s).T @ np.abs(X64))
    err = np.abs(out["Ct"].cpu().numpy().T - s[:, None] * Vh)
    print("project_blocks vs s Vh: max err / tol", float((err / tol).max()), "max err", float(err.max()))
    assert (err <= tol).all()
    energy = (X64 * X64).sum(axis=0)
    assert (np.abs(out["energy"].cpu().numpy() - energy) <= pr.energy_bound(X)).all()
    want = ((s[:, None] * Vh) ** 2).sum(axis=0) / energy
    assert np.abs(out["captured"].cpu().numpy() - want).max() <= 1e-5
    assert out["rows"] == m and abs(out["captured_total"] - (s ** 2).sum() / energy.sum()) <= 1e-5


def test_restart_continues_a_planted_signal_past_the_window(KERN):
    """Three damped oscillations (conjugate pairs) fitted on [0, 6]; a NEW state of the same dynamics -- other
    complex amplitudes -- is observed on [8, 8.5] as raw fields: restart returns its amplitudes, and the forecast
    continues it."""
    from dmd_era5_amd import bopdmd as bop
    from dmd_era5_amd.forecast import DmdForecast

    t = np.linspace(0, 6, 200)
    half = np.array([-0.1 + 2.0j, -0.5 + 5.0j, -0.02 + 0.7j])
    alpha = np.concatenate([half, half.conj()])
    rs = np.random.RandomState(2)
    mh = rs.standard_normal((3, 6)) + 1j * rs.standard_normal((3, 6))
    M = np.concatenate([mh, mh.conj()])                                  # (r, n_s): rows = modes, amplitudes inside
    H = (np.exp(np.outer(t, alpha)) @ M).real
    res = bop.optdmd(torch.from_numpy(H).to(torch.complex128).to(DEV), torch.from_numpy(t).to(DEV), 6, tol=1e-10, maxiter=60)
    assert res.rel_error < 1e-8
    Q = np.linalg.qr(rs.standard_normal((700, 6)))[0].astype(np.float32)
    mu, sd = (280.0 + rs.standard_normal(700)).astype(np.float32), (5.0 + 10.0 * rs.rand(700)).astype(np.float32)
    blocks = [(0, 300), (300, 700)]
    f = DmdForecast([_t(Q[a:b].T) for a, b in blocks], res, means=[_t(mu[a:b]) for a, b in blocks],
                    stds=[_t(sd[a:b]) for a, b in blocks])
    bh = rs.standard_normal(3) + 1j * rs.standard_normal(3)
    bnew = np.concatenate([bh, bh.conj()])
    coef = lambda tt: ((np.exp(np.outer(tt, alpha)) * bnew) @ M).real                      # noqa: E731
    field = lambda tt: (mu + sd * (coef(tt) @ Q.T.astype(np.float64))).astype(np.float32)   # noqa: E731
    tw = np.linspace(8.0, 8.5, 24)
    Xw = field(tw)
    g = f.restart([_t(Xw[:, a:b]) for a, b in blocks], tw)
    assert g.result.info["restart_dropped"] == 0 and g.result.rel_error < 1e-4
    # planted amplitudes in the result's normalisation (unit-norm modes): |b_j| ||M_j||, matched by eigenvalue
    eigs = g.result.eigs.cpu().numpy()
    amp = g.result.amplitudes.cpu().numpy()
    for j, a in enumerate(alpha):
        i = int(np.argmin(np.abs(eigs - a)))
        assert abs(eigs[i] - a) < 1e-5
        want = abs(bnew[j]) * np.linalg.norm(M[j])
        # the fields are fp32 near 300 and sigma >= 5: a standardised element is off by at most 2^-24 * 340 / 5,
        # a coefficient (unit column of Q, 700 rows) by cerr = sqrt(700) times that, the 24 x 6 window by
        # sqrt(24 * 6) cerr in the Frobenius norm; column j of the least-squares system has the norm
        # sqrt(24) exp(Re(alpha_j) t) >= sqrt(24) seen, and 4 is allowed for its conditioning
        cerr = np.sqrt(700.0) * 2.0 ** -24 * 340.0 / 5.0
        seen = np.exp(a.real * 8.5)
        print(f"restart mode {j}: amplitude {amp[i]:.9g}, planted {want:.9g}, tolerance {4 * np.sqrt(6.0) * cerr / seen:.3g}")
        assert abs(amp[i] - want) <= 4 * np.sqrt(6.0) * cerr / seen, (j, amp[i], want)
    t2 = np.linspace(8.5, 10.0, 31)
    sc = g.score([_t(field(t2)[:, a:b]) for a, b in blocks], t2)
    assert sc["rel_error_total"] < 1e-4
    old = f.score([_t(field(t2)[:, a:b]) for a, b in blocks], t2)
    assert old["rel_error_total"] > 100 * sc["rel_error_total"]         # the training window's amplitudes do not fit


@pytest.mark.parametrize("d", [1, 2])
def test_project_onto_svd_results_through_main(svd_base_config, project_root, d):
    from dmd_era5_amd import io_netcdf
    from dmd_era5_amd.config_parser import config_parser
    from dmd_era5_amd.create_mock_data import add_download_attributes, create_mock_era5
    from dmd_era5_amd.era5_svd import main, project_onto_svd_results

    nt = 13 - d + 1
    cfg = dict(svd_base_config, start_datetime="2019-01-01T00", end_datetime="2019-01-01T12", variables="temperature",
               levels="1000,850", svd_type="standard", mean_center=True, scale=True, delay_embedding=d,
               n_components=nt, save_data_matrix=True, svd_seed=0)
    p = config_parser(cfg, "era5-svd")
    ds = add_download_attributes(create_mock_era5(cfg["start_datetime"], cfg["end_datetime"], p["variables"], p["levels"],
                                                  seed=3, dtype=np.float32), p)
    io_netcdf.to_netcdf(ds, p["era5_slice_path"])
    res, _, _ = main(cfg, write_to_netcdf=False)
    Xv = np.asarray(res["X"].values)
    sV = np.asarray(res["s"].values, dtype=np.float64)[:, None] * np.asarray(res["V"].values, dtype=np.float64)
    assert ("X_mean" in res.data_vars) == (d > 1)
    if d > 1:       # the file carries the statistics: hand over the RAW embedded matrix, they are the defaults
        X = (Xv.astype(np.float64) * np.asarray(res["X_std"].values)[:, None] + np.asarray(res["X_mean"].values)[:, None])
        X = X.astype(np.float32)
    else:           # the reference's d = 1 quirk: no statistics in the file, X is the standardised matrix
        X = res["X"]
    C = project_onto_svd_results(res, X)
    assert C.dims == ("components", "time") and C.values.dtype == Xv.dtype and C.values.shape == sV.shape
    if d == 1:
        assert np.array_equal(C.coords["time"].values, res["X"].coords["time"].values)
    assert np.abs(C.values - sV).max() <= 2e-4 * np.abs(sV).max()
    assert C.attrs["captured_total"] == pytest.approx(1.0, abs=1e-4)
    C3 = project_onto_svd_results(res, X, n_components=3)
    assert np.abs(C3.values - sV[:3]).max() <= 2e-4 * np.abs(sV).max()
