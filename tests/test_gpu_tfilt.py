"""K22 (dmdx_tfilt_f32) through the ctypes table: values bit for bit against tests/tfilt_ref.py (the host definition;
the kernel is never its own reference), the memory contract on operands from tests/memguard.py (NaN canaries in pads,
guard zones and in every snapshot no window addresses) and every refusal.

Comparisons are made on the integer view, with the NaN rule of tests/test_gpu_clim.py: where the reference holds a NaN
that arithmetic produced the kernel must hold a NaN, everywhere else the bits must be equal.  The kernel has two walks
-- a run of R outputs per lane over the union window (stride < L and ldy % 4 == 0), and one output after another --
and two ways to read X (16-byte loads, element by element): the layouts below reach every combination.
"""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import memguard as mg
import tfilt_ref as fr

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DEV = "cuda"
E_INVALID = -1000
MS = (1, 3, 4, 5, 1021, 1027)                     # below a quad, a quad, ragged quads; just below / above 1024 rows = one workgroup
TAPS = ((1, 1), (2, 1), (3, 5), (24, 24), (25, 3), (241, 1), (241, 24))
# Y: (offset in floats past a 16-byte boundary, ldy % 4); X: offset (0: 16-byte aligned with ldx % 4 == 0; else odd ldx)
Y_LAYOUTS = [(oy, r) for r in (0, 1) for oy in (0, 1, 2, 3)]
X_OFFSETS = (0, 1, 2, 3)


def _kernel_run():
    """R: the outputs a lane of the kernel holds (kRun of csrc/tfilt.hip), read from the source: the C ABI has no
    entry point for it.  This is the default of the product build (csrc/Makefile passes no -DDMDX_TFILT_RUN).  Against
    a library built with another value -- the R study of MEASUREMENTS.md -- every test here still holds, the results
    do not depend on R, but T_OUTS and the grid cap below then miss that build's R - 1 / R / R + 1 edges."""
    src = Path(__file__).resolve().parents[1] / "dmd_era5_amd" / "csrc" / "tfilt.hip"
    return int(re.search(r"#define DMDX_TFILT_RUN (\d+)", src.read_text()).group(1))


R = _kernel_run()
T_OUTS = (1, R - 1, R, R + 1, 3 * R + 2)           # the last: several runs of one lane's workgroup column


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


def _taps(Lh, seed=0):
    """Lh weights of both signs that sum to about one; nothing symmetric, so a reversed walk shows."""
    rs = np.random.RandomState(50 + seed + Lh)
    h = rs.standard_normal(Lh) + 0.5
    return h / np.abs(h).sum()


def _data(m, T, seed=0):
    rs = np.random.RandomState(seed + m + 7 * T)
    return (250.0 + 30.0 * rs.standard_normal((m, T))).astype(np.float32)


def _x_guarded(X, ox, pad=0, used=None):
    """X (m, T) on the device: ox == 0 -> 16-byte aligned with ldx % 4 == 0, else ox floats past a boundary with an
    odd ldx.  ``used``: a (T,) mask of the snapshots some window addresses; the others become canaries."""
    m, T = X.shape
    ldx = _ceil4(m) + 4 * pad if ox == 0 else (m + 2 * pad) | 1
    g = mg.Guarded(m, T, ldx, F32, ox, DEV).fill(X)
    if used is not None and not used.all():
        g.iview[torch.from_numpy(~used).to(DEV)] = mg.CANARY32
    return g.snapshot()


def _y_guarded(m, T_out, oy, r4, pad=0):
    return mg.Guarded(m, T_out, _ceil4(m) + 4 * pad + r4, F32, oy, DEV)


def _h_guarded(h):
    return mg.Guarded(len(h), 1, len(h), F64, 0, DEV).fill(np.asarray(h, dtype=np.float64)).snapshot()


def _used(T, Lh, stride, T_out):
    used = np.zeros(T, dtype=bool)
    for u in range(T_out):
        used[u * stride:u * stride + Lh] = True
    return used


def _call(L, gX, gH, stride, gY, **kw):
    a = dict(X=gX.ptr, m=gX.rows, T=gX.cols, ldx=gX.ld, h=gH.ptr, L=gH.rows, stride=stride, Y=gY.ptr, T_out=gY.cols, ldy=gY.ld)
    a.update(kw)
    return L.dmdx_tfilt_f32(*a.values(), _stream())


def _run_checked(L, X, h, stride, T_out, ox, ylay, what, pad=0):
    """One launch on guarded operands -> Y (m, T_out), after the memory checks."""
    m, T = X.shape
    gX = _x_guarded(X, ox, pad, _used(T, len(h), stride, T_out))
    gH, gY = _h_guarded(h), _y_guarded(m, T_out, *ylay, pad)
    assert _call(L, gX, gH, stride, gY) == 0, (what, L.dmdx_last_error())
    got = gY.logical()
    gY.check_fully_written(what)
    gY.check_untouched(what)
    for g in (gX, gH):
        g.check_untouched(what)
        g.check_unchanged(what)
    return got


def _run(L, X, h, stride=1, T_out=None, ox=0, ylay=(0, 0)):
    T_out = fr.n_out(X.shape[1], len(h), stride) if T_out is None else T_out
    return _run_checked(L, X, h, stride, T_out, ox, ylay, "run")


# ---------------------------------------------------------------- values and memory on every layout
@pytest.mark.parametrize("m", MS)
def test_bit_equal_on_every_layout(L, m):
    cases = [(Lh, stride, T_out, trail) for Lh, stride in TAPS for T_out in T_OUTS for trail in (0, 5)]
    if m == 5:
        cases += [(int(L.dmdx_tfilt_max_taps()), 1, R + 1, 0)]
    seen = set()
    for i, (Lh, stride, T_out, trail) in enumerate(cases):
        ylay, ox = Y_LAYOUTS[i % 8], X_OFFSETS[(i // 8 + i) % 4]
        seen.add((ylay, ox))
        T = (T_out - 1) * stride + Lh + trail                   # trail: snapshots behind the last window, never read
        X, h = _data(m, T), _taps(Lh)
        what = f"m {m} L {Lh} stride {stride} T_out {T_out} T {T} x offset {ox} y layout {ylay}"
        got = _run_checked(L, X, h, stride, T_out, ox, ylay, what, pad=i % 2)
        _same(got, fr.tfilt(X, h, stride, T_out), what)
    assert {y for y, _ in seen} == set(Y_LAYOUTS) and {x for _, x in seen} == set(X_OFFSETS)


def test_every_layout_pair_on_both_walks(L):
    """All 32 pairs of an X offset and a Y layout, on the walk over a union window and on the one over single outputs."""
    m = 1027
    for Lh, stride in ((25, 3), (24, 24)):
        T_out = R + 1
        T = (T_out - 1) * stride + Lh + 2
        X, h = _data(m, T, seed=1), _taps(Lh, seed=1)
        want = fr.tfilt(X, h, stride, T_out)
        for ox in X_OFFSETS:
            for ylay in Y_LAYOUTS:
                what = f"L {Lh} stride {stride} x offset {ox} y layout {ylay}"
                _same(_run_checked(L, X, h, stride, T_out, ox, ylay, what), want, what)


def test_more_runs_than_grid_rows(L):
    """grid.y is capped at 65 535 runs of R outputs and strided beyond: 65 535 R + 13 outputs of 4 rows, with one tap
    (single outputs) and with two (the union-window walk)."""
    m, T_out = 4, 65535 * R + 13
    for Lh in (1, 2):
        T = T_out - 1 + Lh
        rs = np.random.RandomState(8 + Lh)
        X = rs.standard_normal((m, T)).astype(np.float32)
        h = _taps(Lh, seed=2)
        got = _run_checked(L, X, h, 1, T_out, 0, (0, 0), f"{T_out} outputs, {Lh} taps")
        assert np.array_equal(_bits(got), _bits(fr.tfilt(X, h, 1, T_out)))


def test_exact_integers_whatever_the_walk(L):
    """Integer X in +-100 with taps on the grid of 2^-10 in +-1/16: every product and partial sum is exact (below
    241 * 100 * 64 < 2^21 multiples of 2^-10), so the result is the int64 sum whatever the order -- and fits fp32."""
    rs = np.random.RandomState(7)
    m = 37
    for Lh, stride in TAPS:
        T_out = 2 * R + 3
        T = (T_out - 1) * stride + Lh
        Xi = rs.randint(-100, 101, (m, T)).astype(np.int64)
        hi = rs.randint(-64, 65, Lh).astype(np.int64)
        want = np.zeros((m, T_out), dtype=np.int64)
        for j in range(Lh):
            want += Xi[:, j:j + (T_out - 1) * stride + 1:stride] * hi[j]
        X, h = Xi.astype(np.float32), hi.astype(np.float64) / 1024.0
        assert np.array_equal(fr.tfilt(X, h, stride).astype(np.float64) * 1024.0, want)          # the reference, on the CPU
        for ox, ylay in ((0, (0, 0)), (1, (3, 1)), (2, (2, 0))):
            got = _run(L, X, h, stride, T_out, ox, ylay)
            assert np.array_equal(got.astype(np.float64) * 1024.0, want), (Lh, stride, ox, ylay)
        # zeroing one tap changes every output by exactly that term: a tap dropped or taken twice shows here
        for j0 in sorted({0, Lh // 2, Lh - 1}):
            h0 = h.copy()
            h0[j0] = 0.0
            got = _run(L, X, h0, stride, T_out).astype(np.float64) * 1024.0
            assert np.array_equal(want - got, Xi[:, j0:j0 + (T_out - 1) * stride + 1:stride] * hi[j0]), (Lh, stride, j0)


def test_power_of_two_scaling(L):
    m = 41
    for Lh, stride in ((25, 3), (24, 24), (241, 1)):
        T = 3 * R * stride + Lh
        X, h = _data(m, T, seed=11), _taps(Lh, seed=3)
        base = _run(L, X, h, stride)
        for e in (-20, 7, 30):
            got = _run(L, np.ldexp(X, e), h, stride)
            assert np.array_equal(_bits(got), _bits(np.ldexp(base, e))), (Lh, stride, e)


def test_nonfinite_reaches_its_windows_only(L):
    """A NaN and an Inf at a window's edge and at a window's centre: exactly the outputs of that row whose window holds
    the snapshot are hit -- under a zero tap too (Inf * 0 is NaN) -- and every other output keeps the bits of the run
    without them.  A row of zeros gives +0.0 whatever the signs of the taps."""
    m = 41
    for Lh, stride in ((25, 3), (24, 24), (241, 24), (3, 5)):
        T_out = 2 * R + 1
        T = (T_out - 1) * stride + Lh + 3
        X, h = _data(m, T, seed=21), _taps(Lh, seed=4)
        h[Lh // 2] = 0.0
        h[0] = -abs(h[0])
        clean = _run(L, X, h, stride, T_out)
        u = R                                                     # the first output of the second run
        spots = [(3, u * stride, np.nan), (20, u * stride + Lh - 1, np.inf), (9, u * stride + Lh // 2, -np.inf),
                 (30, u * stride + Lh // 2, np.nan), (12, 0, np.inf), (13, (T_out - 1) * stride + Lh - 1, np.nan),
                 (14, T - 1, np.nan)]                             # the last one: behind every window
        Xn = X.copy()
        hit = np.zeros((m, T_out), dtype=bool)
        for i, t, v in spots:
            Xn[i, t] = v
            for w in range(T_out):
                hit[i, w] |= w * stride <= t < w * stride + Lh
        assert hit[[3, 20, 9, 30, 12, 13]].any(axis=1).all() and not hit[14].any()
        Xn[7, :] = 0.0
        got = _run(L, Xn, h, stride, T_out)
        _same(got, fr.tfilt(Xn, h, stride, T_out), f"NaN / Inf, L {Lh} stride {stride}")
        assert not np.isfinite(got[hit]).any()
        assert np.isnan(got[9, u]) and np.isnan(got[3, u])        # the Inf under the zero tap of output u
        rest = ~hit
        rest[7] = False
        assert np.array_equal(_bits(got)[rest], _bits(clean)[rest])
        assert (_bits(got[7]) == 0).all()
        neg = _run(L, Xn, -np.abs(h) - 0.25, stride, T_out)
        assert (_bits(neg[7]) == 0).all()


# ---------------------------------------------------------------- refusals and empty shapes
def test_refusals_write_nothing(L):
    m, Lh, stride, T_out = 12, 5, 3, 9
    T = (T_out - 1) * stride + Lh + 2
    X, h = _data(m, T), _taps(Lh)
    ld, big, st = m + 4, 2**31, _stream()
    gX = mg.Guarded(m, T, ld, F32, 0, DEV).fill(X).snapshot()
    gH = _h_guarded(h)
    gY = mg.Guarded(m, T_out, ld, F32, 0, DEV)
    max_taps = int(L.dmdx_tfilt_max_taps())
    assert max_taps >= 2048
    good = dict(X=gX.ptr, m=m, T=T, ldx=ld, h=gH.ptr, L=Lh, stride=stride, Y=gY.ptr, T_out=T_out, ldy=ld)
    xbytes = 4 * ((T - 1) * ld + m)
    bad = [dict(X=None), dict(h=None), dict(Y=None), dict(m=-1), dict(T=-1), dict(T_out=-1), dict(ldx=-1), dict(ldy=-1),
           dict(L=0), dict(L=-1), dict(L=max_taps + 1), dict(L=big), dict(stride=0), dict(stride=-2), dict(stride=big),
           dict(T_out=T_out + 1), dict(T=T - 3), dict(stride=stride + 1), dict(L=Lh + 3), dict(T=0), dict(T=Lh - 1, T_out=1),
           dict(ldx=m - 1), dict(ldy=m - 1), dict(m=big, ldx=big, ldy=big), dict(T=big), dict(T_out=big, T=big), dict(ldx=big),
           dict(ldy=big),
           # sizes below 2^31 each whose extent (T - 1) ldx + m, (T_out - 1) ldy + m does not fit the overlap test
           dict(T=big - 1, ldx=big - 1), dict(T=big - 1, T_out=big - 1, L=1, stride=1, ldy=big - 1), dict(X=gX.ptr + 2), dict(Y=gY.ptr + 1), dict(Y=gY.ptr + 3), dict(h=gH.ptr + 4),
           # Y inside, across the front and across the end of the address range of X (all T snapshots)
           dict(Y=gX.ptr), dict(Y=gX.ptr + 16), dict(Y=gX.ptr - 8), dict(Y=gX.ptr + xbytes - 4),
           dict(Y=gX.ptr - 4 * ((T_out - 1) * ld + m) + 4), dict(Y=gX.ptr + 4 * (T - 3) * ld)]
    for change in bad:
        assert L.dmdx_tfilt_f32(*{**good, **change}.values(), st) == E_INVALID, change
        assert L.dmdx_last_error(), change
    assert b"overlap" in L.dmdx_last_error()
    # sizes of zero: the checks, then nothing to do and nothing written
    for change in (dict(m=0), dict(T_out=0), dict(m=0, T_out=0), dict(T_out=0, T=Lh - stride)):
        assert L.dmdx_tfilt_f32(*{**good, **change}.values(), st) == 0, (change, L.dmdx_last_error())
    assert L.dmdx_tfilt_f32(*{**good, "T_out": 0, "T": Lh - stride - 1}.values(), st) == E_INVALID
    torch.cuda.synchronize()
    assert bool((gY.ibuf == gY.canary).all())
    for g in (gX, gH):
        g.check_untouched("input")
        g.check_unchanged("input")
    # ... and the same arguments, unchanged, run; so does a Y right behind the last element of X
    assert L.dmdx_tfilt_f32(*good.values(), st) == 0, L.dmdx_last_error()
    _same(gY.logical(), fr.tfilt(X, h, stride, T_out), "after the refusals")
    both = mg.Guarded(m, T + T_out, m, F32, 0, DEV)
    both.view[:T].copy_(torch.from_numpy(np.ascontiguousarray(X.T)))
    rc = L.dmdx_tfilt_f32(both.ptr, m, T, m, gH.ptr, Lh, stride, both.ptr + 4 * T * m, T_out, m, st)
    assert rc == 0, L.dmdx_last_error()
    both.check_untouched("X | Y")
    res = both.logical()
    assert np.array_equal(_bits(res[:, :T]), _bits(X))
    _same(res[:, T:], fr.tfilt(X, h, stride, T_out), "Y behind X")
