"""K28 (dmdx_remap_f32) through the ctypes table: values bit for bit against tests/remap_ref.py (the host definition; the
kernel is never its own reference), the memory contract on operands from tests/memguard.py, every refusal, and the
equivalence with K23 (dmdx_coarsen_f32) on block tables.

Comparisons are made on the integer view, with the NaN rule of tests/test_gpu_coarsen.py: where the reference holds a NaN
the kernel must hold a NaN, everywhere else the bits must be equal.  Canaries sit in every element the contract says is
not read -- the plane pads, the slack of ldx, the guard zones of X -- and in every element of Y that is not written; the
entries of wy and wx beyond the counts are NaN.  With skipna off the canary of X is a NaN: a stray read shows as a NaN.
With skipna on a NaN would be skipped silently, so there it is a finite 1e30.  Every table in here describes memory that
exists: regrid.Remap is the only producer of tables and validates them on the host.
"""
import numpy as np
import pytest
import torch

import coarsen_ref as cr
import memguard as mg
import remap_ref as rr

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DEV = "cuda"
E_INVALID = -1000
FINITE_CANARY = np.array([1e30], dtype=np.float32).view(np.int32)[0]
B = 256                                                                    # DMDX_REMAP_BLOCK: the cells of one workgroup


@pytest.fixture(scope="module")
def L():
    from dmd_era5_amd.kernels import default_kernels

    return default_kernels()._lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what=""):
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ok = (_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))
    assert ok.all(), f"{what}: {int((~ok).sum())} of {ok.size} elements differ, first at {tuple(np.argwhere(~ok)[0])}"


def _ceil4(n):
    return (n + 3) // 4 * 4


def _fine(T, P, nlat, nlon, seed=0):
    rs = np.random.RandomState(seed + 3 * T + 5 * P + 7 * nlat + 11 * nlon)
    return (250.0 + 30.0 * rs.standard_normal((T, P, nlat, nlon))).astype(np.float32)


def _cell_centred(first_edge, last_edge, n):
    d = (last_edge - first_edge) / n
    return first_edge + d * (np.arange(n) + 0.5)


def _tables(rm):
    return rm.iy0, rm.ny, rm.wy, rm.jx0, rm.nx, rm.wx


def _random_tables(nlat, nlon, NLAT, NLON, SY, SX, seed, wrap=True):
    """Tables of one's own: spans of every length 1 .. S at random places (columns wrap), positive weights."""
    rs = np.random.RandomState(seed)
    ny, nx = rs.randint(1, min(SY, nlat) + 1, NLAT), rs.randint(1, min(SX, nlon) + 1, NLON)
    ny[0], nx[0] = min(SY, nlat), min(SX, nlon)
    iy0 = np.array([rs.randint(0, nlat - n + 1) for n in ny])
    jx0 = rs.randint(0, nlon, NLON) if wrap else np.array([rs.randint(0, nlon - n + 1) for n in nx])
    return (iy0.astype(np.int32), ny.astype(np.int32), rs.uniform(0.1, 1.0, (NLAT, SY)), jx0.astype(np.int32), nx.astype(np.int32),
            rs.uniform(0.1, 1.0, (NLON, SX)))


def _era_like():
    """13 x 16 around the globe -> 7 x 8 with the poles: cap rows, half cells, a column that wraps."""
    from dmd_era5_amd.regrid import Remap

    return Remap.regular(90.0 - 15.0 * np.arange(13), 22.5 * np.arange(16), 30, 45)


def _regional():
    from dmd_era5_amd.regrid import Remap

    return Remap(_cell_centred(60.0, 42.0, 9), _cell_centred(10.0, 40.0, 12), _cell_centred(60.0, 42.0, 4), _cell_centred(10.0, 40.0, 5))


def _finer():
    from dmd_era5_amd.regrid import Remap

    return Remap(_cell_centred(50.0, 40.0, 5), _cell_centred(0.0, 16.0, 8), _cell_centred(50.0, 40.0, 9), _cell_centred(0.0, 16.0, 16))


class Case:
    """The operands of one launch: guarded X and Y, the six tables with NaN beyond the counts, and the clean host image
    the reference reads."""

    def __init__(self, fine, tables, *, padx=0, pady=0, ox=0, ldxr=0, oy=0, ldyr=0, slack=0, skipna=False, min_frac=0.0):
        fine = np.ascontiguousarray(fine, dtype=np.float32)
        T, P, nlat, nlon = fine.shape
        iy0, ny, wy, jx0, nx, wx = tables
        self.tables = tuple(np.ascontiguousarray(v, dtype=np.int32) for v in (iy0, ny)) + (np.array(wy, dtype=np.float64),) + \
            tuple(np.ascontiguousarray(v, dtype=np.int32) for v in (jx0, nx)) + (np.array(wx, dtype=np.float64),)
        self.T, self.P, self.nlat, self.nlon = T, P, nlat, nlon
        self.NLAT, self.NLON, self.SY, self.SX = len(ny), len(nx), self.tables[2].shape[1], self.tables[5].shape[1]
        self.skipna, self.min_frac = bool(skipna), float(min_frac)
        self.cells = self.NLAT * self.NLON
        self.ldp, self.ldq = nlat * nlon + padx, self.cells + pady
        self.mx, self.my = (P - 1) * self.ldp + nlat * nlon, (P - 1) * self.ldq + self.cells
        self.ldx = _ceil4(self.mx) + 4 * slack + ldxr
        self.ldy = _ceil4(self.my) + 4 * slack + ldyr
        canary = FINITE_CANARY if self.skipna else np.int32(mg.CANARY32)
        self.clean = np.zeros((T, self.mx), dtype=np.float32)
        image = np.full((T, self.mx), canary, dtype=np.int32)
        for p in range(P):
            self.clean[:, p * self.ldp:p * self.ldp + nlat * nlon] = fine[:, p].reshape(T, -1)
            image[:, p * self.ldp:p * self.ldp + nlat * nlon] = fine[:, p].reshape(T, -1).view(np.int32)
        self.gX = mg.Guarded(self.mx, T, self.ldx, F32, ox, DEV)
        self.gX.ibuf.fill_(int(canary))
        self.gX.iview.copy_(torch.from_numpy(image).to(DEV))
        self.x_before = self.gX.ibuf.clone()
        # the device tables: NaN weights wherever the counts say there is nothing
        dev = [t.copy() for t in self.tables]
        dev[2][np.arange(self.SY)[None, :] >= self.tables[1][:, None]] = np.nan
        dev[5][np.arange(self.SX)[None, :] >= self.tables[4][:, None]] = np.nan
        self.dT = [torch.from_numpy(t).to(DEV) for t in dev]
        self.t_before = [t.clone() for t in self.dT]
        self.gY = mg.Guarded(self.my, T, self.ldy, F32, oy, DEV)

    def args(self, **kw):
        t = [x.data_ptr() for x in self.dT]
        a = dict(X=self.gX.ptr, T=self.T, ldx=self.ldx, P=self.P, ldp=self.ldp, nlat=self.nlat, nlon=self.nlon, iy0=t[0], ny=t[1],
                 wy=t[2], SY=self.SY, jx0=t[3], nx=t[4], wx=t[5], SX=self.SX, NLAT=self.NLAT, NLON=self.NLON,
                 skipna=int(self.skipna), min_frac=self.min_frac, Y=self.gY.ptr, ldy=self.ldy, ldq=self.ldq)
        a.update(kw)
        return a

    def want(self):
        return rr.remap(self.clean, self.P, self.nlat, self.nlon, *self.tables, ldp=self.ldp, skipna=self.skipna,
                        min_frac=self.min_frac)

    def run(self, L, what=""):
        """One launch -> Y (T, P cells), after the memory checks."""
        assert L.dmdx_remap_f32(*self.args().values(), _stream()) == 0, (what, L.dmdx_last_error())
        torch.cuda.synchronize()
        y = self.gY.iview.cpu().numpy()                                           # (T, my) int32
        logical = np.zeros(self.my, dtype=bool)
        for p in range(self.P):
            logical[p * self.ldq:p * self.ldq + self.cells] = True
        assert (y[:, logical] != np.int32(mg.CANARY32)).all(), f"{what}: a cell of Y was never written"
        assert (y[:, ~logical] == np.int32(mg.CANARY32)).all(), f"{what}: a plane pad of Y was written"
        self.gY.check_untouched(what)
        assert torch.equal(self.gX.ibuf, self.x_before), f"{what}: X or its surroundings changed"
        for now, before in zip(self.dT, self.t_before):
            assert torch.equal(now.view(torch.uint8), before.view(torch.uint8)), f"{what}: a table changed"
        return np.ascontiguousarray(y[:, logical]).view(np.float32)

    def check(self, L, what=""):
        got = self.run(L, what)
        _same(got, self.want(), what)
        return got


# ---------------------------------------------------------------- values and memory
@pytest.mark.parametrize("name,make", (("periodic 13 x 16 -> 7 x 8", _era_like), ("regional 9 x 12 -> 4 x 5", _regional),
                                       ("finer 5 x 8 -> 9 x 16", _finer)))
def test_grids_of_the_class_on_every_layout(L, name, make):
    rm = make()
    nlat, nlon = rm.shape_in
    k = 0
    for T in (1, 3, 70):
        for skipna in (False, True):
            for P, padx, pady, slack in ((1, 0, 0, 0), (3, 3, 2, 1)):
                k += 1
                fine = _fine(T, P, nlat, nlon, seed=k)
                if skipna:
                    rs = np.random.RandomState(k)
                    fine[rs.uniform(size=fine.shape) < 0.25] = np.nan
                    fine[rs.uniform(size=fine.shape) < 0.02] = np.inf
                Case(fine, _tables(rm), padx=padx, pady=pady, ox=k % 4, ldxr=k % 2, oy=(k + 1) % 4, ldyr=(k // 2) % 2, slack=slack,
                     skipna=skipna, min_frac=0.5 if skipna else 0.0).check(L, f"{name}, T {T} P {P} skipna {skipna}")


@pytest.mark.parametrize("NLON", (1, 63, 64, 65, 257))
def test_target_rows_across_waves_and_workgroups(L, NLON):
    """Rows that end inside a wave, at its end and behind it, and planes whose cells straddle workgroups; spans on both
    sides of what a lane keeps in registers (8), columns that wrap."""
    for SY, SX, NLAT, skipna in ((3, 5, 5, False), (2, 8, 3, True), (4, 9, 2, False), (1, 1, 4, True)):
        nlat, nlon = 11, 37
        fine = _fine(2, 3, nlat, nlon, seed=NLON + SX)
        if skipna:
            fine[:, :, ::3, ::5] = np.nan
        tables = _random_tables(nlat, nlon, NLAT, NLON, SY, SX, seed=NLON + 7 * SX)
        Case(fine, tables, padx=1, pady=3, ox=1, oy=2, slack=1, skipna=skipna, min_frac=0.3).check(L, f"NLON {NLON} spans {SY} x {SX}")
    assert 257 > B > 65                                                           # (257 cells of one row: two workgroups)


def test_one_cell_of_the_widest_spans(L):
    """SY = SX = 64: one cell over 64 x 64 source points, and the same spans wrapping around a grid of 64 columns."""
    fine = _fine(2, 1, 64, 64, seed=1)
    rs = np.random.RandomState(2)
    for jx0 in (0, 37):
        tables = (np.array([0]), np.array([64]), rs.uniform(0.1, 1.0, (1, 64)), np.array([jx0]), np.array([64]), rs.uniform(0.1, 1.0, (1, 64)))
        Case(fine, tables, oy=1).check(L, f"64 x 64 from column {jx0}")
    # a source grid of one column
    tables = _random_tables(5, 1, 3, 4, 2, 1, seed=3)
    Case(_fine(2, 2, 5, 1, seed=4), tables).check(L, "nlon 1")


def test_more_snapshots_than_grid_rows(L):
    """grid.y is capped at 65 535 snapshots and strided beyond: 65 537 snapshots of one cell of 2 x 2."""
    T = 65537
    fine = np.random.RandomState(4).standard_normal((T, 1, 2, 2)).astype(np.float32)
    tables = (np.array([0]), np.array([2]), np.array([[0.75, 0.5]]), np.array([1]), np.array([2]), np.array([[0.25, 1.0]]))
    Case(fine, tables).check(L, "65537 snapshots")


# ---------------------------------------------------------------- values
def test_exact_integer_means(L):
    """Integers in +-1000, weights="none", a target of twice the step aligned with the source cells: every overlap is one
    whole cell of 2 x 2.5 degrees, the sums stay far below 2^53 and the quotient lies on the grid of 1 / 4."""
    from dmd_era5_amd.regrid import Remap

    rm = Remap(_cell_centred(60.0, 44.0, 8), _cell_centred(10.0, 40.0, 12), _cell_centred(60.0, 44.0, 4), _cell_centred(10.0, 40.0, 6),
               weights="none")
    assert (rm.ny == 2).all() and (rm.nx == 2).all()
    Xi = np.random.RandomState(7).randint(-1000, 1001, (3, 2, 8, 12)).astype(np.int64)
    want = Xi.reshape(3, 2, 4, 2, 6, 2).sum(axis=(3, 5)).reshape(3, -1)
    got = Case(Xi.astype(np.float32), _tables(rm), ox=1, oy=3, padx=1, pady=2).check(L, "integers")
    assert np.array_equal(got.astype(np.float64) * 4.0, want.astype(np.float64))


def test_power_of_two_scaling_constants_and_zeros(L):
    for rm in (_era_like(), _regional(), _finer()):
        nlat, nlon = rm.shape_in
        fine = _fine(2, 2, nlat, nlon, seed=2)
        base = Case(fine, _tables(rm)).check(L, "base")
        for e in (-20, 20):
            got = Case(np.ldexp(fine, e), _tables(rm)).run(L, f"2^{e}")
            assert np.array_equal(_bits(got), _bits(np.ldexp(base, e))), e
        const = Case(np.full_like(fine, 287.654), _tables(rm)).run(L, "constant")
        assert (_bits(const) == _bits(np.float32(287.654))).all()
        zeros = np.zeros_like(fine)
        zeros[..., ::2] = -0.0
        assert (_bits(Case(zeros, _tables(rm)).run(L, "zeros")) == 0).all()
        assert (_bits(Case(-np.abs(zeros), _tables(rm)).run(L, "-0.0")) == 0).all()
        assert (_bits(Case(-np.abs(zeros), _tables(rm), skipna=True, min_frac=1.0).run(L, "-0.0, skipna")) == 0).all()


def test_nonfinite_values(L):
    """Without skipna a NaN, +Inf or -Inf reaches exactly the target cells that overlap it; with skipna it is left out;
    a cell with nothing left is 0x7fc00000; the min_frac threshold at 0, 0.5 and 1."""
    rm = _era_like()                                                            # 13 x 16 -> 7 x 8
    T, P = 2, 2
    fine = _fine(T, P, 13, 16, seed=5)
    A = np.zeros((7, 13), dtype=bool)
    Bm = np.zeros((8, 16), dtype=bool)
    for I in range(7):
        A[I, rm.iy0[I]:rm.iy0[I] + rm.ny[I]] = True
    for J in range(8):
        Bm[J, (rm.jx0[J] + np.arange(rm.nx[J])) % 16] = True
    spots = [(0, 0, 0, 0, np.nan), (0, 1, 3, 6, np.inf), (1, 0, 6, 15, -np.inf), (1, 1, 12, 8, np.nan)]
    Xn, hit = fine.copy(), np.zeros((T, P, 7, 8), dtype=bool)
    for t, p, i, j, v in spots:
        Xn[t, p, i, j] = v
        hit[t, p] |= np.outer(A[:, i], Bm[:, j])
    assert hit.sum() == 1 + 2 + 2 + 1                        # (even rows and columns lie inside one target cell, odd ones are cut)
    hit = hit.reshape(T, -1)
    clean = Case(fine, _tables(rm)).check(L, "clean")
    off = Case(Xn, _tables(rm), min_frac=1.0).check(L, "skipna off")
    assert not np.isfinite(off[hit]).any() and np.array_equal(_bits(off)[~hit], _bits(clean)[~hit])
    on = Case(Xn, _tables(rm), skipna=True, min_frac=0.5).check(L, "skipna on")
    assert np.isfinite(on).all() and np.array_equal(_bits(on)[~hit], _bits(clean)[~hit])
    assert (_bits(on)[hit] != _bits(clean)[hit]).all()
    # a whole cell gone: target (1, 2) of plane 1, snapshot 1 overlaps the source rows 1 .. 3 and columns 3 .. 5
    gone = fine.copy()
    gone[1, 1, 1:4, 3:6] = [[np.nan, np.inf, -np.inf]] * 3
    gone[0, 0, 0:2, :] = np.nan                                                  # ... and the cap row 0 of plane 0, snapshot 0
    for min_frac in (0.0, 0.5, 1.0):
        got = Case(gone, _tables(rm), skipna=True, min_frac=min_frac).check(L, f"min_frac {min_frac}").reshape(T, P, 7, 8)
        assert _bits(got[1, 1, 1, 2]) == cr.QUIET_NAN_BITS and (_bits(got[0, 0, 0]) == cr.QUIET_NAN_BITS).all()
        # the neighbours of the hole keep a part of their weight: present at 0, gone at 1
        assert np.isfinite(got[1, 1, 1, 1]) == (min_frac < 1.0) and np.isfinite(got[1, 1, 1, 3]) == (min_frac < 1.0)
        assert np.isfinite(got[0, 1]).all() and np.isfinite(got[1, 0]).all()
    # the threshold at equality, with weights that are exact: two rows of 0.5, columns of 0.25, 0.5, 0.25
    tables = (np.array([0]), np.array([2]), np.array([[0.5, 0.5]]), np.array([0]), np.array([3]), np.array([[0.25, 0.5, 0.25]]))
    x = np.array([[1.0, np.nan, 3.0], [np.nan, 5.0, np.nan]], dtype=np.float32).reshape(1, 1, 2, 3)    # kept 0.5 of 1.0
    assert np.isfinite(Case(x, tables, skipna=True, min_frac=0.5).check(L, "kept == least")).all()
    x[0, 0, 0, 0] = np.inf                                                      # kept 0.375
    assert _bits(Case(x, tables, skipna=True, min_frac=0.5).check(L, "kept < least"))[0, 0] == cr.QUIET_NAN_BITS
    assert np.isfinite(Case(x, tables, skipna=True, min_frac=0.375).check(L, "kept == least, 0.375")).all()


# ---------------------------------------------------------------- K23 on the same input
@pytest.mark.parametrize("fy,fx", ((4, 4), (2, 2), (3, 5)))
@pytest.mark.parametrize("skipna", (False, True))
def test_block_tables_give_the_bits_of_the_coarsen_kernel(L, fy, fx, skipna):
    T, P, nlat, nlon, lat0, lon0 = 3, 2, 3 * fy + 2, 70 * fx + 3, 1, 2
    NLAT, NLON = 3, 70
    fine = _fine(T, P, nlat, nlon, seed=fy + fx)
    if skipna:
        rs = np.random.RandomState(fx)
        fine[rs.uniform(size=fine.shape) < 0.2] = np.nan
        fine[rs.uniform(size=fine.shape) < 0.02] = -np.inf
    w = np.cos(np.deg2rad(np.linspace(85.0, -80.0, nlat))) + 0.01 * np.random.RandomState(nlat).uniform(size=nlat)
    c = Case(fine, rr.block_tables(w, fy, fx, NLAT, NLON, lat0, lon0), padx=2, pady=1, skipna=skipna, min_frac=0.5)
    got = c.check(L, f"blocks {fy} x {fx}")
    gW = torch.from_numpy(w).to(DEV)
    gY = mg.Guarded(c.my, T, c.ldy, F32, 0, DEV)
    rc = L.dmdx_coarsen_f32(c.gX.ptr, T, c.ldx, P, c.ldp, nlat, nlon, gW.data_ptr(), fy, fx, lat0, lon0, NLAT, NLON, int(skipna), 0.5,
                            gY.ptr, c.ldy, c.ldq, _stream())
    assert rc == 0, L.dmdx_last_error()
    torch.cuda.synchronize()
    y = gY.iview.cpu().numpy()
    k23 = np.concatenate([y[:, p * c.ldq:p * c.ldq + c.cells] for p in range(P)], axis=1).view(np.float32)
    _same(got, k23, f"K28 against K23, {fy} x {fx}")
    assert np.array_equal(np.isnan(got), np.isnan(k23))


# ---------------------------------------------------------------- refusals and empty shapes
def test_refusals_write_nothing(L):
    rm = _era_like()
    c = Case(_fine(3, 2, 13, 16), _tables(rm), padx=2, pady=1, slack=1)
    good, st, big = c.args(), _stream(), 2 ** 31
    X, Y = c.gX.ptr, c.gY.ptr
    assert int(L.dmdx_remap_max_span()) == 64 and (c.NLAT, c.NLON, c.SY, c.SX) == (7, 8, 3, 3)
    xbytes, ybytes = 4 * ((c.T - 1) * c.ldx + c.mx), 4 * ((c.T - 1) * c.ldy + c.my)
    bad = [dict(X=None), dict(Y=None), dict(iy0=None), dict(ny=None), dict(wy=None), dict(jx0=None), dict(nx=None), dict(wx=None),
           dict(T=-1), dict(P=-1), dict(nlat=-1), dict(nlon=-1), dict(NLAT=-1), dict(NLON=-1), dict(ldx=-1), dict(ldp=-1), dict(ldy=-1),
           dict(ldq=-1), dict(SY=0), dict(SX=0), dict(SY=65), dict(SX=65), dict(SY=-2),
           dict(ldp=13 * 16 - 1), dict(ldq=7 * 8 - 1), dict(ldx=c.mx - 1), dict(ldy=c.my - 1),
           dict(nlat=0, ldp=0, ldx=0), dict(nlon=0, ldp=0, ldx=0),
           dict(T=big), dict(P=big), dict(nlat=big), dict(nlon=big), dict(ldx=big), dict(ldy=big), dict(ldp=big), dict(ldq=big),
           dict(NLAT=big), dict(NLON=big), dict(T=big - 1, ldx=big - 1), dict(T=big - 1, ldy=big - 1),
           dict(min_frac=-0.1), dict(min_frac=1.0001), dict(min_frac=float("nan")),
           dict(X=X + 2), dict(Y=Y + 1), dict(Y=Y + 3), dict(iy0=good["iy0"] + 2), dict(nx=good["nx"] + 1), dict(wy=good["wy"] + 4),
           dict(wx=good["wx"] + 4),
           dict(Y=X), dict(Y=X + 16), dict(Y=X - 8), dict(Y=X + xbytes - 4), dict(Y=X - ybytes + 4)]
    for change in bad:
        assert L.dmdx_remap_f32(*{**good, **change}.values(), st) == E_INVALID, change
        assert b"remap" in L.dmdx_last_error(), change
    assert b"overlap" in L.dmdx_last_error()
    # sizes of zero: the checks, then nothing to do and nothing written
    for change in (dict(T=0), dict(P=0), dict(NLAT=0), dict(NLON=0), dict(NLAT=0, NLON=0)):
        assert L.dmdx_remap_f32(*{**good, **change}.values(), st) == 0, (change, L.dmdx_last_error())
    assert L.dmdx_remap_f32(*{**good, "T": 0, "SX": 0}.values(), st) == E_INVALID
    torch.cuda.synchronize()
    assert bool((c.gY.ibuf == c.gY.canary).all())
    assert torch.equal(c.gX.ibuf, c.x_before)
    # ... and the same arguments, unchanged, run
    c.check(L, "after the refusals")


# ---------------------------------------------------------------- through the package
def test_through_the_package():
    from dmd_era5_amd import _lib
    from dmd_era5_amd.kernels import default_kernels
    from dmd_era5_amd.regrid import Remap

    kern = default_kernels()
    rm = Remap.regular(90.0 - 15.0 * np.arange(13), 22.5 * np.arange(16), 30, 45, skipna=True, min_frac=0.4)
    rs = np.random.RandomState(9)
    host = [(250.0 + 30.0 * rs.standard_normal((3, 2 * 208))).astype(np.float32),
            np.concatenate([(250.0 + 30.0 * rs.standard_normal((3, 208))).astype(np.float32), np.full((3, 3), np.nan, np.float32)], axis=1)]
    host[0][1, 40:44] = np.nan
    X = [torch.from_numpy(h).to(DEV) for h in host]
    want = [rr.remap(h, p, 13, 16, *_tables(rm), skipna=True, min_frac=0.4) for h, p in zip(host, (2, 1))]
    Y = rm.apply(X, [2, 1])
    for y, w, p in zip(Y, want, (2, 1)):
        assert y.shape == (3, rm.rows_out(p)) and y.dtype == F32
        _same(y.cpu().numpy(), w, f"apply, {p} planes")
    # out= views with a row stride of their own, inside one allocation
    slab = torch.full((3, 2 * 56 + 56 + 10), float("nan"), device=DEV)
    out = [slab[:, :112], slab[:, 115:171]]
    Y2 = rm.apply(X, [2, 1], out=out)
    assert all(a is b for a, b in zip(Y2, out))
    for y, w in zip(Y2, want):
        _same(y.cpu().numpy(), w, "apply, out=")
    assert bool(torch.isnan(slab[:, 112:115]).all()) and bool(torch.isnan(slab[:, 171:]).all())
    f = rm.apply_field(X[1][0, :208].contiguous(), 1)
    _same(f.cpu().numpy().reshape(1, -1), want[1][:1], "apply_field")
    # HipKernels.remap itself: ldp / ldq, and what it refuses before the launch
    t = [torch.from_numpy(v).to(DEV) for v in _tables(rm)]
    Xp = torch.zeros((3, 2 * 211), device=DEV)
    Xp[:, :208], Xp[:, 211:419] = X[0][:, :208], X[0][:, 208:]
    Yp = kern.remap(Xp, 2, 13, 16, *t, ldp=211, ldq=60, skipna=True, min_frac=0.4)
    assert Yp.shape == (3, 60 + 56)
    _same(torch.cat([Yp[:, :56], Yp[:, 60:]], dim=1).cpu().numpy(), want[0], "ldp / ldq")
    for call in (lambda: kern.remap(X[0], 2, 13, 16, *t, out=X[0][:, :112]),                       # overlap
                 lambda: kern.remap(X[0].double(), 2, 13, 16, *t),                                 # dtype
                 lambda: kern.remap(X[0], 2, 13, 16, t[0], t[1], t[2].float(), t[3], t[4], t[5]),
                 lambda: kern.remap(X[0], 2, 13, 16, t[0].long(), *t[1:]),
                 lambda: kern.remap(X[0], 3, 13, 16, *t),                                          # too few rows
                 lambda: kern.remap(X[0], 2, 13, 16, *t, out=torch.zeros((3, 111), device=DEV)),
                 lambda: kern.remap(X[0], 2, 13, 16, t[0].cpu(), *t[1:])):
        with pytest.raises(_lib.DmdxError):
            call()
