"""K21 (dmdx_treg_fit_f32 / dmdx_treg_apply_f32) through the ctypes table: values bit for bit against
tests/treg_ref.py (the host definition; the kernel is never its own reference), the memory contract on operands from
tests/memguard.py (NaN canaries in pads and guard zones, an exact workspace) and every refusal.

Comparisons are made on the integer view, with the NaN rule of tests/test_gpu_clim.py: where the reference holds a NaN
that arithmetic produced the kernel must hold a NaN, everywhere else the bits must be equal.  Every fit runs in both
forms -- time split over workgroups through a workspace, and one lane walking its segments -- and both must give the
reference's bits.
"""
import numpy as np
import pytest
import torch

import memguard as mg
import treg_ref as tr

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DEV = "cuda"
E_INVALID = -1000
T0 = 37
SEGS = (1, 8, 16, 37, 100)          # every snapshot a segment; a tail of 5; a tail of 5 after 2; equal to T; above T
PS = (1, 2, 5, 8)
# (X, coef) and (X, coef, Y) base offsets in floats past a 16-byte boundary: every operand sees 0 .. 3, not in step
FIT_OFFSETS = [(0, 0), (1, 2), (2, 3), (3, 1), (0, 1), (1, 0), (0, 2), (3, 3)]
APPLY_OFFSETS = [(0, 0, 0), (1, 2, 3), (2, 3, 1), (3, 1, 2), (0, 1, 0), (1, 0, 0), (0, 0, 2), (3, 3, 3)]
SHAPES = [(m, pad) for m in (1, 3, 1029, 2053) for pad in (0, 7)]


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


def _data(m, T=T0, seed=0):
    rs = np.random.RandomState(seed + m)
    return (250.0 + 30.0 * rs.standard_normal((m, T))).astype(np.float32)


def _design(T, p, seed=0):
    """A (T, p) design on uneven times: 1, tau, tau^2, one harmonic pair, then random series."""
    rs = np.random.RandomState(100 + seed + p)
    tau = np.sort(rs.uniform(-1.0, 1.0, T))
    cols = [np.ones(T), tau, tau * tau, np.cos(5.0 * tau), np.sin(5.0 * tau)] + [rs.standard_normal(T) for _ in range(3)]
    return np.ascontiguousarray(np.stack(cols[:p], axis=1))


def _w_guarded(W, pad=3):
    """W (p, T) on the device with ldw = T + pad: column j of the guarded matrix is W[j, :]."""
    p, T = W.shape
    return mg.Guarded(T, p, T + pad, F64, 0, DEV).fill(np.ascontiguousarray(W.T)).snapshot()


def _d_guarded(D, pad=3):
    """D (T, p) on the device with ldd = p + pad: column t of the guarded matrix is D[t, :]."""
    T, p = D.shape
    return mg.Guarded(p, T, p + pad, F64, 0, DEV).fill(np.ascontiguousarray(D.T)).snapshot()


def _coef(m, p, pad, off, host=None):
    """A (p, m) coefficient field: p columns of m floats, ld = m + pad; .logical().T is (p, m)."""
    g = mg.Guarded(m, p, m + pad, F32, off, DEV)
    if host is not None:
        g.fill(np.ascontiguousarray(host.T)).snapshot()
    return g


def _fit(L, gX, gW, seg, gC, split, **kw):
    """One fit; split: through an exact workspace between canaries, else workspace == NULL.  -> (rc, workspace)."""
    a = dict(X=gX.ptr, m=gX.rows, T=gX.cols, ldx=gX.ld, W=gW.ptr, p=gW.cols, ldw=gW.ld, seg=seg, coef=gC.ptr, ldc=gC.ld)
    a.update(kw)
    ws, wptr, wbytes = None, None, 0
    if split:
        wbytes = int(L.dmdx_treg_fit_workspace_bytes(a["m"], a["T"], a["p"], a["seg"]))
        nseg = -(-a["T"] // a["seg"])
        assert wbytes == nseg * a["p"] * a["m"] * 8
        ws = mg.Workspace(wbytes, DEV)
        wptr = ws.ptr
    rc = L.dmdx_treg_fit_f32(*a.values(), wptr, wbytes, _stream())
    return rc, ws


def _unwritten(g):
    return bool((g.ibuf == g.canary).all())


def _fit_checked(L, gX, gW, seg, m, p, pad, oc, what):
    """Both forms of one fit -> the (p, m) result, after the memory checks; the two forms agree to the bit."""
    res = []
    for split in (True, False):
        gC = _coef(m, p, pad, oc)
        rc, ws = _fit(L, gX, gW, seg, gC, split)
        assert rc == 0, L.dmdx_last_error()
        res.append(gC.logical().T)
        gC.check_fully_written(what)
        gC.check_untouched(what)
        if ws is not None:
            ws.check_untouched(what)
    assert np.array_equal(_bits(res[0]), _bits(res[1])), f"{what}: split and walk differ"
    return res[0]


# ---------------------------------------------------------------- fit
@pytest.mark.parametrize("m,pad", SHAPES)
def test_fit_bit_equal_on_every_layout(L, m, pad):
    X = _data(m)
    want, gWs = {}, {}
    for p in PS:
        W = tr.w_of(_design(T0, p))
        gWs[p] = _w_guarded(W)
        for seg in SEGS:
            want[seg, p] = tr.fit(X, W, seg)
    gXs = {}
    for i, (seg, p) in enumerate((seg, p) for seg in SEGS for p in PS):
        ox, oc = FIT_OFFSETS[(i + i // 8) % 8]
        if ox not in gXs:
            gXs[ox] = mg.Guarded(m, T0, m + pad, F32, ox, DEV).fill(X).snapshot()
        got = _fit_checked(L, gXs[ox], gWs[p], seg, m, p, pad, oc, f"fit seg {seg} p {p} offsets {(ox, oc)}")
        _same(got, want[seg, p], f"fit seg {seg} p {p} offsets {(ox, oc)}")
    assert sorted(gXs) == [0, 1, 2, 3]
    for g in list(gXs.values()) + list(gWs.values()):
        g.check_untouched("input")
        g.check_unchanged("input")


@pytest.mark.parametrize("pad", [0, 7])
def test_fit_several_full_segments(L, pad):
    """T = 2100 with seg = 1024: two full segments and a tail of 52 (six full groups of the unroll and four more)."""
    m, T, p = 1029, 2100, 3
    X = _data(m, T, seed=5)
    W = tr.w_of(_design(T, p, seed=1))
    want = tr.fit(X, W, 1024)
    gW = _w_guarded(W, pad=5)
    for ox, oc in ((0, 0), (1, 3)):
        gX = mg.Guarded(m, T, m + pad, F32, ox, DEV).fill(X).snapshot()
        got = _fit_checked(L, gX, gW, 1024, m, p, pad, oc, f"fit T = 2100 offsets {(ox, oc)}")
        _same(got, want, f"fit T = 2100 offsets {(ox, oc)}")
        gX.check_untouched("X")
        gX.check_unchanged("X")


def test_fit_more_segments_than_grid_rows(L):
    """T = 65 535 + 13 snapshots of 5 rows with seg = 1: 65 548 segments, grid.y of the split form is strided over
    them; the workspace holds one double per (segment, column, row)."""
    m, p, T = 5, 2, 65535 + 13
    rs = np.random.RandomState(8)
    X = (250.0 + 30.0 * rs.standard_normal((m, T))).astype(np.float32)
    W = rs.standard_normal((p, T)) / T
    want = tr.fit(X, W, 1)
    gX = mg.Guarded(m, T, m, F32, 0, DEV).fill(X).snapshot()
    gW = _w_guarded(W, pad=1)
    got = _fit_checked(L, gX, gW, 1, m, p, 0, 0, "fit with 65 548 segments")
    _same(got, want, "fit with 65 548 segments")
    for g in (gX, gW):
        g.check_untouched("input")
        g.check_unchanged("input")


def _run_fit(L, X, W, seg, split=True):
    m, T = X.shape
    gX = mg.Guarded(m, T, m, F32, 0, DEV).fill(X)
    gC = _coef(m, W.shape[0], 0, 0)
    rc, _ = _fit(L, gX, _w_guarded(W, pad=0), seg, gC, split)
    assert rc == 0, L.dmdx_last_error()
    return gC.logical().T


def test_fit_exact_values_whatever_the_order(L):
    """Integer X in +-1000 with W on the grid of 1 / 16 in +-0.5: every product and every partial sum is exact (below
    37 * 500 with 4 fraction bits: 19 bits), so every order of summation gives the fp64 matrix product exactly."""
    m, p = 37, 4
    rs = np.random.RandomState(7)
    X = rs.randint(-1000, 1001, (m, T0)).astype(np.float32)
    W = rs.randint(-8, 9, (p, T0)).astype(np.float64) / 16.0
    exact = W @ X.astype(np.float64).T
    assert np.array_equal(exact.astype(np.float32).astype(np.float64), exact)
    for seg in (1, 8, 100):
        assert np.array_equal(tr.fit(X, W, seg).astype(np.float64), exact)          # the reference, on the CPU
        for split in (True, False):
            assert np.array_equal(_run_fit(L, X, W, seg, split).astype(np.float64), exact), (seg, split)
    # zeroing one snapshot's weight changes the result by exactly that term: a snapshot dropped or taken twice at
    # a segment edge (7 | 8, 15 | 16) or at the edge of the unroll shows here
    for t0 in (0, 7, 8, 15, 16, 31, 32, 36):
        W0 = W.copy()
        W0[:, t0] = 0.0
        for split in (True, False):
            got = _run_fit(L, X, W0, 8, split).astype(np.float64)
            assert np.array_equal(exact - got, W[:, t0][:, None] * X[:, t0].astype(np.float64)[None, :]), (t0, split)


def test_fit_value_domain(L):
    m, p = 41, 5
    X = _data(m, seed=11)
    W = tr.w_of(_design(T0, p))
    clean = tr.fit(X, W, 8)
    Xn = X.copy()
    Xn[3, 9], Xn[20, 30] = np.nan, np.inf
    Xn[7, :] = 0.0
    want = tr.fit(Xn, W, 8)
    for split in (True, False):
        got = _run_fit(L, Xn, W, 8, split)
        _same(got, want, "fit with NaN / Inf")
        assert np.isnan(got[:, 3]).all() and not np.isfinite(got[:, 20]).any()
        rest = np.ones(m, dtype=bool)
        rest[[3, 7, 20]] = False
        assert np.array_equal(_bits(got[:, rest]), _bits(clean[:, rest]))            # the neighbours keep their bits
        assert (_bits(got[:, 7]) == 0).all()
        # a row of zeros (a grid point K20 masked out) under weights that are all negative: +0.0, not -0.0
        neg = _run_fit(L, Xn, -np.abs(W) - 0.25, 8, split)
        assert (_bits(neg[:, 7]) == 0).all()
    assert (_bits(tr.fit(Xn, -np.abs(W) - 0.25, 8)[:, 7]) == 0).all()


# ---------------------------------------------------------------- apply
def _apply(L, gX, gD, gC, restore, gY, **kw):
    a = dict(X=gX.ptr, m=gX.rows, T=gX.cols, ldx=gX.ld, D=gD.ptr, p=gD.rows, ldd=gD.ld, coef=gC.ptr, ldc=gC.ld,
             restore=int(restore), Y=gY.ptr, ldy=gY.ld)
    a.update(kw)
    return L.dmdx_treg_apply_f32(*a.values(), _stream())


@pytest.mark.parametrize("m,pad", SHAPES)
def test_apply_in_place_and_out_of_place(L, m, pad):
    """Every Y offset 0 .. 3 with ldy % 4 of 0 .. 3: the ragged head and tail of the aligned-store path, and a head
    shift that changes from snapshot to snapshot inside a run."""
    X = _data(m, seed=21)
    # every p with remove and with restore
    for (ox, oc, oy), p, restore in zip(APPLY_OFFSETS, PS * 2, [False, True, True, False, True, False, False, True]):
        D = _design(T0, p, seed=2)
        coef = tr.fit(X, tr.w_of(D), 16)
        want = tr.apply(X, D, coef, restore)
        gD, gC = _d_guarded(D), _coef(m, p, pad, oc, coef)
        # out of place: every logical element of Y is written
        gX = mg.Guarded(m, T0, m + pad, F32, ox, DEV).fill(X).snapshot()
        gY = mg.Guarded(m, T0, m + (0 if pad else 7) + oy % 2, F32, oy, DEV)
        assert _apply(L, gX, gD, gC, restore, gY) == 0, L.dmdx_last_error()
        got = gY.logical()
        gY.check_fully_written("Y")
        gY.check_untouched("Y")
        _same(got, want, f"apply out of place {(ox, oc, oy, p, restore)}")
        gX.check_untouched("X")
        gX.check_unchanged("X")
        # in place
        gZ = mg.Guarded(m, T0, m + pad, F32, oy, DEV).fill(X)
        assert _apply(L, gZ, gD, gC, restore, gZ) == 0, L.dmdx_last_error()
        gZ.check_untouched("X in place")
        assert np.array_equal(_bits(gZ.logical()), _bits(got))
        for g in (gD, gC):
            g.check_untouched("design / coef")
            g.check_unchanged("design / coef")


def test_apply_values_and_overlap(L):
    m, p = 41, 3
    X = _data(m, seed=31)
    D = _design(T0, p, seed=3)
    coef = tr.fit(X, tr.w_of(D), 16)
    gD, gC = _d_guarded(D, pad=0), _coef(m, p, 0, 0, coef)
    # restore(remove(X)) is the composition of the two definitions, not X
    gX = mg.Guarded(m, T0, m, F32, 0, DEV).fill(X)
    assert _apply(L, gX, gD, gC, 0, gX) == 0
    res = gX.logical()
    _same(res, tr.apply(X, D, coef), "remove")
    assert _apply(L, gX, gD, gC, 1, gX) == 0
    back = gX.logical()
    _same(back, tr.apply(tr.apply(X, D, coef), D, coef, restore=True), "restore(remove(X))")
    # against X itself only a bound holds: f is the same fp64 value both times, and each of the two roundings to
    # fp32 errs by at most half an ulp of a value below 512, 2^-16
    assert np.abs(X).max() < 512 and np.abs(back.astype(np.float64) - X).max() <= 2 * 2.0 ** -16
    # a NaN and an Inf in X reach their own element only; a NaN coefficient reaches its row
    Xn, cn = X.copy(), coef.copy()
    Xn[3, 9], Xn[20, 30], cn[1, 5] = np.nan, -np.inf, np.nan
    gXn, gCn = mg.Guarded(m, T0, m, F32, 1, DEV).fill(Xn), _coef(m, p, 0, 0, cn)
    gY = mg.Guarded(m, T0, m, F32, 2, DEV)
    assert _apply(L, gXn, gD, gCn, 0, gY) == 0
    got = gY.logical()
    _same(got, tr.apply(Xn, D, cn), "apply with NaN / Inf")
    hit = np.zeros((m, T0), dtype=bool)
    hit[3, 9] = hit[20, 30] = True
    hit[5, :] = True
    assert np.isnan(got[3, 9]) and got[20, 30] == -np.inf and np.isnan(got[5]).all()
    assert np.array_equal(_bits(got)[~hit], _bits(res)[~hit])
    # a partial overlap of X and Y is refused and nothing is written; so is Y == X with another ldy
    g = mg.Guarded(m, 2 * T0, m, F32, 0, DEV).fill(np.concatenate([X, X], axis=1)).snapshot()
    st = _stream()
    for yptr, ldy in ((g.ptr + 16, m), (g.ptr + 4 * (T0 * m - 5), m), (g.ptr, m + 1), (g.ptr - 8, m)):
        rc = L.dmdx_treg_apply_f32(g.ptr, m, T0, m, gD.ptr, p, p, gC.ptr, m, 0, yptr, ldy, st)
        assert rc == E_INVALID and b"overlap" in L.dmdx_last_error()
    rc = L.dmdx_treg_apply_f32(g.ptr, m, T0, m, gD.ptr, p, p, gC.ptr, m, 0, g.ptr + 4 * T0 * m, m, st)
    assert rc == 0                                                # the second half: disjoint, runs
    g.check_untouched("X | Y")
    both = g.logical()
    assert np.array_equal(_bits(both[:, :T0]), _bits(X))
    _same(both[:, T0:], tr.apply(X, D, coef), "apply into the neighbouring columns")


def test_apply_more_runs_than_grid_rows(L):
    """T = 8 * 65 535 + 13 snapshots of 5 rows: grid.y is strided over the runs of 8 snapshots."""
    m, p, T = 5, 2, 8 * 65535 + 13
    rs = np.random.RandomState(4)
    X = rs.standard_normal((m, T)).astype(np.float32)
    D = np.ascontiguousarray(np.stack([np.ones(T), np.linspace(-1.0, 1.0, T)], axis=1))
    coef = rs.standard_normal((p, m)).astype(np.float32)
    gX = mg.Guarded(m, T, m, F32, 0, DEV).fill(X)
    assert _apply(L, gX, _d_guarded(D, pad=0), _coef(m, p, 0, 0, coef), 0, gX) == 0, L.dmdx_last_error()
    gX.check_untouched("X")
    assert np.array_equal(_bits(gX.logical()), _bits(tr.apply(X, D, coef)))


# ---------------------------------------------------------------- refusals and empty shapes
def test_refusals_write_nothing(L):
    m, p = 12, 3
    X = _data(m)
    D = _design(T0, p)
    W = tr.w_of(D)
    coef = tr.fit(X, W, 8)
    ld, big, st = m + 2, 2**31, _stream()
    gX = mg.Guarded(m, T0, ld, F32, 0, DEV).fill(X).snapshot()
    gW, gD = _w_guarded(W), _d_guarded(D)
    gCin = _coef(m, p, 2, 0, coef)
    gC, gY = _coef(m, p, 2, 0), mg.Guarded(m, T0, ld, F32, 0, DEV)
    wbytes = int(L.dmdx_treg_fit_workspace_bytes(m, T0, p, 8))
    ws = mg.Workspace(wbytes, DEV)
    assert L.dmdx_treg_max_p() == 8
    good = dict(X=gX.ptr, m=m, T=T0, ldx=ld, W=gW.ptr, p=p, ldw=gW.ld, seg=8, coef=gC.ptr, ldc=ld, ws=ws.ptr, wbytes=wbytes)
    bad = [dict(X=None), dict(W=None), dict(coef=None), dict(m=-1), dict(T=-1), dict(ldx=m - 1), dict(ldc=m - 1),
           dict(ldw=T0 - 1), dict(p=0), dict(p=9), dict(p=-1), dict(seg=0), dict(seg=-5), dict(seg=big),
           dict(m=big, ldx=big, ldc=big), dict(T=big, ldw=big), dict(ldx=big), dict(ldc=big), dict(ldw=big),
           dict(X=gX.ptr + 2), dict(coef=gC.ptr + 1), dict(W=gW.ptr + 4), dict(ws=ws.ptr + 4), dict(wbytes=wbytes - 1)]
    for change in bad:
        for nows in ({}, dict(ws=None, wbytes=0)):
            if "ws" in change and nows or "wbytes" in change and nows:
                continue
            assert L.dmdx_treg_fit_f32(*{**good, **change, **nows}.values(), st) == E_INVALID, change
            assert L.dmdx_last_error()
    assert L.dmdx_treg_fit_workspace_bytes(m, T0, 9, 8) == 0 and L.dmdx_treg_fit_workspace_bytes(m, T0, p, 0) == 0
    good_a = dict(X=gX.ptr, m=m, T=T0, ldx=ld, D=gD.ptr, p=p, ldd=gD.ld, coef=gCin.ptr, ldc=ld, restore=0, Y=gY.ptr, ldy=ld)
    bad_a = [dict(X=None), dict(D=None), dict(coef=None), dict(Y=None), dict(m=-1), dict(T=-1), dict(ldx=m - 1),
             dict(ldc=m - 1), dict(ldy=m - 1), dict(ldd=p - 1), dict(p=0), dict(p=9), dict(m=big, ldx=big, ldc=big, ldy=big),
             dict(T=big), dict(ldx=big), dict(ldc=big), dict(ldy=big), dict(ldd=big), dict(X=gX.ptr + 2),
             dict(Y=gY.ptr + 3), dict(coef=gCin.ptr + 1), dict(D=gD.ptr + 4),
             # sizes below 2^31 each whose extent (T - 1) ld + m does not fit the overlap test: out of place, in place, one side
             dict(T=big - 1, ldx=big - 1, ldy=big - 1), dict(T=big - 1, ldx=big - 1, ldy=big - 1, Y=gX.ptr),
             dict(T=big - 1, ldx=big - 1), dict(T=big - 1, ldy=big - 1)]
    for change in bad_a:
        assert L.dmdx_treg_apply_f32(*{**good_a, **change}.values(), st) == E_INVALID, change
        assert L.dmdx_last_error()
    # sizes of zero: the checks, then nothing to do and nothing written
    for change in (dict(m=0), dict(T=0)):
        assert L.dmdx_treg_fit_f32(*{**good, **change}.values(), st) == 0
        assert L.dmdx_treg_fit_f32(*{**good, **change, "ws": None, "wbytes": 0}.values(), st) == 0
        assert L.dmdx_treg_apply_f32(*{**good_a, **change}.values(), st) == 0
    torch.cuda.synchronize()
    assert _unwritten(gC) and _unwritten(gY)
    ws.check_untouched("workspace")
    ws.check_unused("workspace")
    for g in (gX, gW, gD, gCin):
        g.check_untouched("input")
        g.check_unchanged("input")
    # ... and the same arguments, unchanged, run
    assert L.dmdx_treg_fit_f32(*good.values(), st) == 0, L.dmdx_last_error()
    _same(gC.logical().T, coef, "fit after the refusals")
