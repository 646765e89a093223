"""K23 (dmdx_coarsen_f32) through the ctypes table: values bit for bit against tests/coarsen_ref.py (the host definition;
the kernel is never its own reference), the memory contract on operands from tests/memguard.py and every refusal.

Comparisons are made on the integer view, with the NaN rule of tests/test_gpu_tfilt.py: where the reference holds a NaN
the kernel must hold a NaN, everywhere else the bits must be equal.  Canaries sit in every element the contract says is
not read -- the rows before lat0 and the longitudes before lon0, the dropped trailing rows and longitudes, the plane
pads, the slack of ldx, the guard zones of X, and w outside lat0 .. lat0 + NLAT fy -- and in every element of Y that is
not written.  With skipna off the canary of X is a NaN: a stray read shows as a NaN.  With skipna on a NaN would be
skipped silently, so there it is a finite 1e30.  The kernel reads the floats of a cell's fine row with 16-byte loads
where the address of that row allows it (fx = 4, 8; at fx = 2 a lane forms four neighbouring cells, the last 1 .. 3
cells of a coarse row dword by dword, and stores the four with 16 bytes where it may) and element by element otherwise:
the offsets, leading dimensions, plane pads, grid widths and NLON of every residue mod 4 below reach every phase of
those addresses.
"""
import itertools
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import coarsen_ref as cr
import memguard as mg

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DEV = "cuda"
E_INVALID = -1000
FYS, FXS = (1, 2, 3, 4), (1, 2, 3, 4, 5, 8)
NLONS, NLATS = (1, 3, 4, 5, 9), (1, 2, 5)
FINITE_CANARY = np.array([1e30], dtype=np.float32).view(np.int32)[0]


def _kernel_geometry():
    """B: the lanes of one workgroup (DMDX_COARSEN_BLOCK of csrc/coarsen_geom.h); C2: the neighbouring cells of a coarse
    row one lane forms at fx = 2 (coarsen_cells_per_lane; one everywhere else).  Read from the source: the C ABI has no
    entry point for them."""
    src = (Path(__file__).resolve().parents[1] / "dmd_era5_amd" / "csrc" / "coarsen_geom.h").read_text()
    return (int(re.search(r"#define DMDX_COARSEN_BLOCK (\d+)", src).group(1)),
            int(re.search(r"coarsen_cells_per_lane\(int FX\) \{ return FX == 2 \? (\d+) : 1; \}", src).group(1)))


B, C2 = _kernel_geometry()


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


def _w(nlat, seed=0):
    return np.cos(np.deg2rad(np.linspace(85.0, -80.0, nlat))) + 0.01 * np.random.RandomState(seed + nlat).uniform(size=nlat)


class Case:
    """The operands of one launch: geometry, guarded X, w and Y, and the clean host image the reference reads."""

    def __init__(self, fine, w, fy, fx, *, lat0=0, lon0=0, NLAT=None, NLON=None, padx=0, pady=0, ox=0, ldxr=0, oy=0, ldyr=0,
                 slack=0, skipna=False, min_frac=0.0):
        fine = np.ascontiguousarray(fine, dtype=np.float32)
        T, P, nlat, nlon = fine.shape
        self.T, self.P, self.nlat, self.nlon, self.fy, self.fx, self.lat0, self.lon0 = T, P, nlat, nlon, fy, fx, lat0, lon0
        self.NLAT = cr.n_cells(nlat, fy, lat0) if NLAT is None else NLAT
        self.NLON = cr.n_cells(nlon, fx, lon0) if NLON is None else NLON
        self.skipna, self.min_frac = bool(skipna), float(min_frac)
        self.cells = self.NLAT * self.NLON
        self.ldp, self.ldq = nlat * nlon + padx, self.cells + pady
        self.mx, self.my = (P - 1) * self.ldp + nlat * nlon, (P - 1) * self.ldq + self.cells
        self.ldx = _ceil4(self.mx) + 4 * slack + ldxr
        self.ldy = _ceil4(self.my) + 4 * slack + ldyr
        self.w = np.asarray(w, dtype=np.float64)
        # the clean image (what the reference reads) and the device image: canaries wherever no cell is
        canary = FINITE_CANARY if self.skipna else np.int32(mg.CANARY32)
        self.clean = np.zeros((T, self.mx), dtype=np.float32)
        image = np.full((T, self.mx), canary, dtype=np.int32)
        i1, j1 = lat0 + self.NLAT * fy, lon0 + self.NLON * fx
        for p in range(P):
            self.clean[:, p * self.ldp:p * self.ldp + nlat * nlon] = fine[:, p].reshape(T, -1)
            plane = np.full((T, nlat, nlon), canary, dtype=np.int32)
            plane[:, lat0:i1, lon0:j1] = fine[:, p, lat0:i1, lon0:j1].view(np.int32)
            image[:, p * self.ldp:p * self.ldp + nlat * nlon] = plane.reshape(T, -1)
        self.gX = mg.Guarded(self.mx, T, self.ldx, F32, ox, DEV)
        self.gX.ibuf.fill_(int(canary))
        self.gX.iview.copy_(torch.from_numpy(image).to(DEV))
        self.x_before = self.gX.ibuf.clone()
        wimg = np.full(nlat, mg.CANARY64, dtype=np.int64)
        wimg[lat0:i1] = self.w[lat0:i1].view(np.int64)
        self.gW = mg.Guarded(nlat, 1, nlat, F64, 0, DEV)
        self.gW.iview.copy_(torch.from_numpy(wimg.reshape(1, -1)).to(DEV))
        self.w_before = self.gW.ibuf.clone()
        self.gY = mg.Guarded(self.my, T, self.ldy, F32, oy, DEV)

    def args(self, **kw):
        a = dict(X=self.gX.ptr, T=self.T, ldx=self.ldx, P=self.P, ldp=self.ldp, nlat=self.nlat, nlon=self.nlon, w=self.gW.ptr,
                 fy=self.fy, fx=self.fx, lat0=self.lat0, lon0=self.lon0, NLAT=self.NLAT, NLON=self.NLON, skipna=int(self.skipna),
                 min_frac=self.min_frac, Y=self.gY.ptr, ldy=self.ldy, ldq=self.ldq)
        a.update(kw)
        return a

    def want(self):
        return cr.coarsen(self.clean, self.P, self.nlat, self.nlon, self.w, self.fy, self.fx, ldp=self.ldp, lat0=self.lat0,
                          lon0=self.lon0, n_lat_out=self.NLAT, n_lon_out=self.NLON, skipna=self.skipna, min_frac=self.min_frac)

    def run(self, L, what=""):
        """One launch -> Y (T, P cells), after the memory checks."""
        assert L.dmdx_coarsen_f32(*self.args().values(), _stream()) == 0, (what, L.dmdx_last_error())
        torch.cuda.synchronize()
        y = self.gY.iview.cpu().numpy()                                           # (T, my) int32
        logical = np.zeros(self.my, dtype=bool)
        for p in range(self.P):
            logical[p * self.ldq:p * self.ldq + self.cells] = True
        assert (y[:, logical] != np.int32(mg.CANARY32)).all(), f"{what}: a cell of Y was never written"
        assert (y[:, ~logical] == np.int32(mg.CANARY32)).all(), f"{what}: a plane pad of Y was written"
        self.gY.check_untouched(what)
        assert torch.equal(self.gX.ibuf, self.x_before), f"{what}: X or its surroundings changed"
        assert torch.equal(self.gW.ibuf, self.w_before), f"{what}: w or its surroundings changed"
        return np.ascontiguousarray(y[:, logical]).view(np.float32)

    def check(self, L, what=""):
        got = self.run(L, what)
        _same(got, self.want(), what)
        return got


# ---------------------------------------------------------------- values and memory on every layout
@pytest.mark.parametrize("fy,fx", list(itertools.product(FYS, FXS)))
def test_bit_equal_on_every_layout(L, fy, fx):
    seen = {k: set() for k in ("lat0", "lon0", "trail_y", "trail_x", "P", "T", "padx", "pady", "x", "y")}
    shapes = list(itertools.product(NLATS, NLONS))
    for i, (NLAT, NLON) in enumerate(shapes + shapes):
        k = i + 7 * fy + 3 * fx
        skipna = i >= len(shapes)
        lat0, lon0 = k % 2, (0, 1, 3)[(k // 2) % 3]
        trail_y, trail_x = (k // 3) % fy, k % fx                              # dropped behind the last cell: 0 .. f - 1
        P, T = (1, 3)[(k // 2) % 2], (1, 5)[(k // 4) % 2]
        padx, pady = k % 4, (k // 4 + k) % 4
        ox, ldxr, oy, ldyr = (k // 2) % 4, k % 2, (k // 2 + 3) % 4, ((k // 2 + 3) // 4) % 2
        nlat, nlon = lat0 + NLAT * fy + trail_y, lon0 + NLON * fx + trail_x
        for key, v in (("lat0", lat0), ("lon0", lon0), ("trail_y", trail_y), ("trail_x", trail_x), ("P", P), ("T", T),
                       ("padx", padx), ("pady", pady), ("x", (ox, ldxr)), ("y", (oy, ldyr))):
            seen[key].add(v)
        fine = _fine(T, P, nlat, nlon, seed=i)
        if skipna:
            rs = np.random.RandomState(k)
            fine[rs.uniform(size=fine.shape) < 0.25] = np.nan
            fine[rs.uniform(size=fine.shape) < 0.02] = np.inf
        what = (f"{fy} x {fx}, {NLAT} x {NLON} cells from ({lat0}, {lon0}) of {nlat} x {nlon}, P {P} T {T} pads {padx} {pady} "
                f"x {ox} {ldxr} y {oy} {ldyr} skipna {skipna}")
        Case(fine, _w(nlat, i), fy, fx, lat0=lat0, lon0=lon0, NLAT=NLAT, NLON=NLON, padx=padx, pady=pady, ox=ox, ldxr=ldxr, oy=oy,
             ldyr=ldyr, slack=k % 2, skipna=skipna, min_frac=0.5 if skipna else 0.0).check(L, what)
    assert seen["lat0"] == {0, 1} and seen["lon0"] == {0, 1, 3} and seen["P"] == {1, 3} and seen["T"] == {1, 5}
    assert seen["trail_y"] == set(range(fy)) and seen["trail_x"] == set(range(fx))
    assert seen["padx"] == seen["pady"] == {0, 1, 2, 3}
    assert len(seen["x"]) == 8 and len(seen["y"]) == 8


@pytest.mark.parametrize("fx", (2, 4, 8, 3))
def test_every_pair_of_layouts(L, fx):
    """All 64 pairs of an X layout (offset 0 .. 3 past a 16-byte boundary, ldx % 4 in {0, 1}) and a Y layout, on grids of
    a width that is and is not a multiple of 4: every phase of a cell's row against the 16- and 8-byte loads."""
    fy, T, P = 2, 2, 2
    for nlon, lon0 in ((5 * fx, 0), (5 * fx + 3, 1)):
        fine, w = _fine(T, P, 7, nlon, seed=fx), _w(7, fx)
        want = None
        for ox, ldxr, oy, ldyr in itertools.product(range(4), (0, 1), range(4), (0, 1)):
            c = Case(fine, w, fy, fx, lat0=1, lon0=lon0, padx=ox % 2, pady=oy % 3, ox=ox, ldxr=ldxr, oy=oy, ldyr=ldyr)
            want = c.want() if want is None else want
            _same(c.run(L, f"fx {fx} nlon {nlon} x {ox} {ldxr} y {oy} {ldyr}"), want, f"fx {fx} nlon {nlon} x {ox} {ldxr} y {oy} {ldyr}")


def test_around_one_workgroup(L):
    """The cells of a snapshot just below, at and just above what one workgroup covers -- B cells, and C2 B at fx = 2,
    where a lane forms C2 neighbouring cells of a coarse row -- and several workgroups with planes whose cells straddle
    them."""
    for NLON in (C2 * B - 1, C2 * B, C2 * B + 1, C2 * B + C2 - 1):
        fine = _fine(2, 1, 3, 2 * NLON + 1, seed=NLON)
        Case(fine, _w(3), 1, 2, lat0=1, NLAT=1, pady=1, ox=2, oy=NLON % 4).check(L, f"1 x {NLON} cells, 1 x 2")
    for P, NLAT, NLON in ((1, 1, B - 1), (1, 1, B), (1, 1, B + 1), (3, 5, B // 4 + 1), (2, 2, B // 4)):
        for fy, fx, skipna in ((2, 4, False), (3, 3, True), (2, 2, True)):
            nlat, nlon = NLAT * fy + 1, NLON * fx + 2
            fine = _fine(2, P, nlat, nlon, seed=NLON)
            if skipna:
                fine[:, :, ::3, ::7] = np.nan
            Case(fine, _w(nlat), fy, fx, lon0=1, padx=1, pady=3, ox=1, oy=2, skipna=skipna,
                 min_frac=0.5).check(L, f"P {P}, {NLAT} x {NLON} cells, {fy} x {fx}")


def test_more_snapshots_than_grid_rows(L):
    """grid.y is capped at 65 535 snapshots and strided beyond: 65 537 snapshots of one 2 x 2 cell."""
    T = 65537
    rs = np.random.RandomState(4)
    fine = rs.standard_normal((T, 1, 2, 2)).astype(np.float32)
    got = Case(fine, [0.75, 0.5], 2, 2).run(L, "65537 snapshots")
    want = cr.coarsen(fine.reshape(T, 4), 1, 2, 2, [0.75, 0.5], 2, 2)
    assert np.array_equal(_bits(got), _bits(want))


# ---------------------------------------------------------------- values
@pytest.mark.parametrize("fy,fx", ((1, 1), (2, 2), (4, 4), (8, 8)))
def test_exact_integer_means(L, fy, fx):
    """Integers in +-1000 with unit weights and fy fx a power of two: sums below 2^16 and a quotient on the grid of 2^-6:
    exact in fp64 and in fp32, whatever the order."""
    rs = np.random.RandomState(7)
    T, P, nlat, nlon = 3, 2, 3 * fy + 1, 5 * fx + 2
    Xi = rs.randint(-1000, 1001, (T, P, nlat, nlon)).astype(np.int64)
    want = Xi[:, :, 1:, 2:].reshape(T, P, 3, fy, 5, fx).sum(axis=(3, 5)).reshape(T, -1)
    for ox, oy in ((0, 0), (1, 3)):
        c = Case(Xi.astype(np.float32), np.ones(nlat), fy, fx, lat0=1, lon0=2, ox=ox, oy=oy, padx=ox, pady=oy)
        got = c.check(L, f"integers {fy} x {fx}")
        assert np.array_equal(got.astype(np.float64) * (fy * fx), want.astype(np.float64))


def test_power_of_two_scaling_and_constants(L):
    T, P, nlat, nlon = 2, 2, 13, 24
    fine, w = _fine(T, P, nlat, nlon, seed=2), _w(nlat)
    for fy, fx in ((4, 4), (3, 5), (2, 8), (2, 2)):
        base = Case(fine, w, fy, fx, lat0=1).check(L, f"{fy} x {fx}")
        for e in (-20, 20):
            got = Case(np.ldexp(fine, e), w, fy, fx, lat0=1).run(L, f"2^{e}")
            assert np.array_equal(_bits(got), _bits(np.ldexp(base, e))), (fy, fx, e)
        const = Case(np.full_like(fine, 287.654), w, fy, fx, lat0=1).run(L, "constant")
        assert (_bits(const) == _bits(np.float32(287.654))).all()
        zeros = np.zeros_like(fine)
        zeros[..., ::2] = -0.0
        assert (_bits(Case(zeros, w, fy, fx).run(L, "zeros")) == 0).all()
        assert (_bits(Case(-np.abs(zeros), w, fy, fx).run(L, "-0.0")) == 0).all()


def test_nonfinite_values(L):
    """NaN, +Inf and -Inf reach exactly their own cell with skipna off and are skipped with skipna on; the min_frac
    threshold holds at equality; a cell with nothing left is 0x7fc00000."""
    T, P, nlat, nlon, fy, fx = 2, 2, 9, 17, 4, 4
    fine = _fine(T, P, nlat, nlon, seed=5)
    w = np.array([9.0, 1.0, 2.0, 3.0, 2.0, 1.0, 1.5, 0.5, 2.0])                # lat0 = 1: cell rows of weight 8 and 5
    spots = [(0, 0, 1, 1, np.nan), (0, 1, 3, 6, np.inf), (1, 0, 6, 12, -np.inf), (1, 1, 8, 16, np.nan), (0, 0, 0, 3, np.nan),
             (1, 1, 2, 0, np.inf)]                                               # (0, 0, 0, 3) and (1, 1, 2, 0): outside every cell
    Xn = fine.copy()
    hit = np.zeros((T, P, 2, 4), dtype=bool)
    for t, p, i, j, v in spots:
        Xn[t, p, i, j] = v
        if i >= 1 and j >= 1:
            hit[t, p, (i - 1) // fy, (j - 1) // fx] = True
    assert hit.sum() == 4
    hit = hit.reshape(T, -1)
    clean = Case(fine, w, fy, fx, lat0=1, lon0=1).check(L, "clean")
    off = Case(Xn, w, fy, fx, lat0=1, lon0=1, min_frac=1.0).check(L, "skipna off")
    assert not np.isfinite(off[hit]).any() and np.array_equal(_bits(off)[~hit], _bits(clean)[~hit])
    on = Case(Xn, w, fy, fx, lat0=1, lon0=1, skipna=True, min_frac=0.5).check(L, "skipna on")
    assert np.isfinite(on).all() and np.array_equal(_bits(on)[~hit], _bits(clean)[~hit])
    assert (_bits(on)[hit] != _bits(clean)[hit]).all()
    # the threshold at equality: in cell row 0 (weights 1, 2, 3, 2: full = 32) the rows of weight 1 and 3 go missing
    eq = fine.copy()
    eq[0, 0, 1, 1:5], eq[0, 0, 3, 1:5] = np.nan, np.inf                        # cell (0, 0): kept 16 of 32
    eq[0, 0, 1, 5:9], eq[0, 0, 3, 5:9], eq[0, 0, 2, 6] = np.nan, np.nan, np.nan   # cell (0, 1): kept 14 of 32
    eq[1, 1, 5:9, 9:13] = np.nan                                               # cell (1, 2) of plane 1: nothing left
    half = Case(eq, w, fy, fx, lat0=1, lon0=1, skipna=True, min_frac=0.5).check(L, "min_frac 0.5").reshape(T, P, 2, 4)
    assert np.isfinite(half[0, 0, 0, 0]) and _bits(half[0, 0, 0, 1]) == cr.QUIET_NAN_BITS
    assert _bits(half[1, 1, 1, 2]) == cr.QUIET_NAN_BITS
    assert np.isfinite(half).sum() == half.size - 2
    low = Case(eq, w, fy, fx, lat0=1, lon0=1, skipna=True, min_frac=14.0 / 32.0).check(L, "min_frac 14 / 32").reshape(T, P, 2, 4)
    assert np.isfinite(low[0, 0, 0, 1]) and _bits(low[1, 1, 1, 2]) == cr.QUIET_NAN_BITS
    none = Case(eq, w, fy, fx, lat0=1, lon0=1, skipna=True, min_frac=0.0).check(L, "min_frac 0").reshape(T, P, 2, 4)
    assert _bits(none[1, 1, 1, 2]) == cr.QUIET_NAN_BITS and np.isfinite(none).sum() == none.size - 1


def test_zero_weight_rows(L):
    """A cell whose rows all weigh nothing is 0 / 0: NaN in its own cells only; a zero-weight row beside others is left
    out of its cell."""
    T, P, nlat, nlon, fy, fx = 2, 1, 8, 12, 2, 4
    fine = _fine(T, P, nlat, nlon, seed=6)
    w = np.array([1.0, 2.0, 0.0, 0.0, 0.0, 3.0, 1.0, 1.0])
    for skipna in (False, True):
        got = Case(fine, w, fy, fx, skipna=skipna, min_frac=0.5).check(L, f"zero weights, skipna {skipna}").reshape(T, 4, 3)
        assert np.isnan(got[:, 1]).all() and np.isfinite(got[:, [0, 2, 3]]).all()
        assert np.array_equal(_bits(got[:, 2]), _bits(fine[:, 0, 5].reshape(T, 3, 4).astype(np.float64).sum(axis=2) * 3.0 / 12.0))


# ---------------------------------------------------------------- refusals and empty shapes
def test_refusals_write_nothing(L):
    T, P, nlat, nlon, fy, fx = 3, 2, 9, 14, 2, 4
    fine, w = _fine(T, P, nlat, nlon), _w(nlat)
    c = Case(fine, w, fy, fx, lat0=1, lon0=2, padx=2, pady=1, slack=1)
    good, st, big = c.args(), _stream(), 2 ** 31
    X, Y, W, NLAT, NLON = c.gX.ptr, c.gY.ptr, c.gW.ptr, c.NLAT, c.NLON
    assert (NLAT, NLON) == (4, 3) and int(L.dmdx_coarsen_max_factor()) == 64
    xbytes, ybytes = 4 * ((T - 1) * c.ldx + c.mx), 4 * ((T - 1) * c.ldy + c.my)
    bad = [dict(X=None), dict(w=None), dict(Y=None), dict(T=-1), dict(P=-1), dict(nlat=-1), dict(nlon=-1), dict(NLAT=-1),
           dict(NLON=-1), dict(ldx=-1), dict(ldp=-1), dict(ldy=-1), dict(ldq=-1),
           dict(fy=0), dict(fx=0), dict(fy=65), dict(fx=65), dict(fy=-2), dict(lat0=-1), dict(lon0=-1),
           dict(NLAT=5), dict(NLON=4), dict(lat0=2), dict(lon0=3), dict(lat0=nlat + 1, NLAT=0), dict(lon0=nlon + 1, NLON=0),
           dict(ldp=nlat * nlon - 1), dict(ldq=NLAT * NLON - 1), dict(ldx=c.mx - 1), dict(ldy=c.my - 1),
           dict(T=big), dict(P=big), dict(nlat=big), dict(nlon=big), dict(ldx=big), dict(ldy=big), dict(ldp=big), dict(ldq=big),
           dict(NLAT=big), dict(NLON=big), dict(T=big - 1, ldx=big - 1), dict(T=big - 1, ldy=big - 1),
           dict(min_frac=-0.1), dict(min_frac=1.0001), dict(min_frac=float("nan")),
           dict(X=X + 2), dict(Y=Y + 1), dict(Y=Y + 3), dict(w=W + 4),
           dict(Y=X), dict(Y=X + 16), dict(Y=X - 8), dict(Y=X + xbytes - 4), dict(Y=X - ybytes + 4)]
    for change in bad:
        assert L.dmdx_coarsen_f32(*{**good, **change}.values(), st) == E_INVALID, change
        assert b"coarsen" in L.dmdx_last_error(), change
    assert b"overlap" in L.dmdx_last_error()
    # sizes of zero: the checks, then nothing to do and nothing written
    for change in (dict(T=0), dict(P=0), dict(NLAT=0), dict(NLON=0), dict(NLAT=0, NLON=0)):
        assert L.dmdx_coarsen_f32(*{**good, **change}.values(), st) == 0, (change, L.dmdx_last_error())
    assert L.dmdx_coarsen_f32(*{**good, "T": 0, "fx": 0}.values(), st) == E_INVALID
    torch.cuda.synchronize()
    assert bool((c.gY.ibuf == c.gY.canary).all())
    assert torch.equal(c.gX.ibuf, c.x_before) and torch.equal(c.gW.ibuf, c.w_before)
    # ... and the same arguments, unchanged, run; so does a Y right behind the last element of X
    c.check(L, "after the refusals")
    m = nlat * nlon
    both = mg.Guarded(m, 2 * T, m, F32, 0, DEV)
    both.view[:T].copy_(torch.from_numpy(fine[:, 0].reshape(T, m)).to(DEV))
    cells = (nlat // fy) * (nlon // fx)
    gW = mg.Guarded(nlat, 1, nlat, F64, 0, DEV).fill(w).snapshot()
    rc = L.dmdx_coarsen_f32(both.ptr, T, m, 1, m, nlat, nlon, gW.ptr, fy, fx, 0, 0, nlat // fy, nlon // fx, 0, 0.0,
                            both.ptr + 4 * T * m, cells, cells, st)
    assert rc == 0, L.dmdx_last_error()
    torch.cuda.synchronize()
    both.check_untouched("X | Y")
    gW.check_untouched("w")
    gW.check_unchanged("w")
    flat = both.view.reshape(-1).cpu().numpy()
    assert np.array_equal(_bits(flat[:T * m]), _bits(fine[:, 0].reshape(-1)))
    _same(flat[T * m:T * m + T * cells].reshape(T, cells), cr.coarsen(fine[:, 0].reshape(T, m), 1, nlat, nlon, w, fy, fx),
          "Y behind X")
    assert bool((both.ibuf[both.start + T * m + T * cells:both.start + 2 * T * m] == both.canary).all())
