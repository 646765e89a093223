"""K26 (dmdx_lag_moments_f32) through the ctypes table: all 1 + 3L planes bit for bit against tests/lag_ref.py (the host
definition; the kernel is never its own reference), the memory contract on operands from tests/memguard.py (NaN
canaries in pads and guard zones, an exact workspace) and every refusal.

Comparisons are made on the uint64 view, with the NaN rule of tests/test_gpu_clim.py: where the reference holds a NaN
that arithmetic produced the kernel must hold a NaN, everywhere else the bits must be equal.  Every case runs in four
forms -- time split over workgroups through a workspace or one lane walking its segments, and the earlier member of a
pair from the LDS ring or loaded again (flags bit 0) -- and all four must give the reference's bits.

The value inputs are x = N(0, 1) 2^U(-12, 12): on ERA-like data (250 + 30 N about its fp32 mean) every chain is exact
in fp64 and a wrong order of summation would pass.  That the inputs tell two partitions apart is asserted on the
reference before a kernel runs.
"""
import ctypes

import numpy as np
import pytest
import torch

import lag_ref as lr
import memguard as mg

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DEV = "cuda"
E_INVALID = -1000
FORMS = [(split, flags) for split in (True, False) for flags in (0, 1)]
SHAPES = [(m, pad) for m in (1, 3, 1029, 2053) for pad in (0, 7)]
# (X, mu, out) base offsets: floats past a 16-byte boundary for X and mu, doubles for out; not in step
OFFSETS = [(0, 0, 0), (1, 2, 1), (2, 3, 0), (3, 1, 1), (0, 1, 1), (1, 0, 0), (0, 2, 0), (3, 3, 1)]


@pytest.fixture(scope="module")
def L():
    from dmd_era5_amd.kernels import default_kernels

    return default_kernels()._lib


@pytest.fixture(scope="module")
def W(L):
    w = int(L.dmdx_lag_moments_ring())
    assert w in (8, 16, 32) and L.dmdx_lag_moments_max_lags() == 8
    return w


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(got, want, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ok = (_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))
    assert ok.all(), f"{what}: {int((~ok).sum())} of {ok.size} elements differ, first at {tuple(np.argwhere(~ok)[0])}"


def _wide(m, T, seed=0):
    rs = np.random.RandomState(seed + m)
    X = (rs.standard_normal((m, T)) * 2.0 ** rs.uniform(-12, 12, (m, T))).astype(np.float32)
    return X, rs.standard_normal(m).astype(np.float32)


def _tells_partitions_apart(X, mu, lags, T):
    """The reference with seg = 8 and with seg = T differs in at least one element of each of S, P, H and E."""
    n = len(lags)
    a, b = lr.moments(X, lags, mu, 8), lr.moments(X, lags, mu, T)
    return all((_bits(a[lo:hi]) != _bits(b[lo:hi])).any() for lo, hi in ((0, 1), (1, 1 + n), (1 + n, 1 + 2 * n), (1 + 2 * n, 1 + 3 * n)))


def _t0(W):
    return max(37, W + 5)


def _lag_lists(seg, W, T):
    """Lists of 1, 2, 5 and 8 lags that together hold 0 and 1, the tier edge W - 1, W, W + 1, the segment edge seg - 1,
    seg, seg + 1, 2 seg, a lag beyond two segments and T - 1 (a single pair) -- what of them is below T."""
    c = sorted(t for t in {0, 1, W - 1, W, W + 1, seg - 1, seg, seg + 1, 2 * seg, 2 * seg + 3, T - 1} | {3, 4, 6, 10, 11}
               if 0 <= t < T)                                # (the five at the end: enough for a list of 8 whatever seg is)
    lists = [c[:8], c[-8:], c[:5], c[-5:], [c[0], c[-1]], [1, W + 1], [T - 1], [W], [0]]
    assert set(c) <= {t for li in lists for t in li} and {1, 2, 5, 8} <= {len(li) for li in lists}
    return lists


def _run(L, gX, gmu, lags, seg, gO, split, flags, **kw):
    """One call; split: through an exact workspace between canaries, else workspace == NULL.  -> (rc, workspace)."""
    n = len(lags)
    host = (ctypes.c_int32 * max(n, 1))(*lags)
    a = dict(X=gX.ptr, m=gX.rows, T=gX.cols, ldx=gX.ld, mu=None if gmu is None else gmu.ptr, lags=host, L=n, seg=seg,
             out=gO.ptr, ldo=gO.ld, flags=flags)
    a.update(kw)
    ws, wptr, wbytes = None, None, 0
    if split:
        wbytes = int(L.dmdx_lag_moments_workspace_bytes(a["m"], a["T"], a["L"], a["seg"]))
        assert wbytes == -(-a["T"] // a["seg"]) * (1 + a["L"]) * a["m"] * 8
        ws = mg.Workspace(wbytes, DEV)
        wptr = ws.ptr
    rc = L.dmdx_lag_moments_f32(*a.values(), wptr, wbytes, _stream())
    return rc, ws


def _checked(L, gX, gmu, lags, seg, m, pad, oo, what):
    """The four forms of one case -> the (1 + 3L, m) planes, after the memory checks; the forms agree to the bit."""
    res = []
    for split, flags in FORMS:
        gO = mg.Guarded(m, 1 + 3 * len(lags), m + pad, F64, oo, DEV)
        rc, ws = _run(L, gX, gmu, lags, seg, gO, split, flags)
        assert rc == 0, L.dmdx_last_error()
        res.append(gO.logical().T)
        gO.check_fully_written(what)
        gO.check_untouched(what)
        if ws is not None:
            ws.check_untouched(what)
    for r, form in zip(res[1:], FORMS[1:]):
        ok = (_bits(r) == _bits(res[0])) | (np.isnan(r) & np.isnan(res[0]))
        assert ok.all(), f"{what}: (split, flags) = {form} differs from {FORMS[0]}"
    return res[0]


def _inputs(X, mu, ox, om, pad):
    m, T = X.shape
    gX = mg.Guarded(m, T, m + pad, F32, ox, DEV).fill(X).snapshot()
    gmu = mg.Guarded(m, 1, m, F32, om, DEV).fill(mu.reshape(-1, 1)).snapshot()
    return gX, gmu


def _inputs_unchanged(*gs):
    for g in gs:
        g.check_untouched("input")
        g.check_unchanged("input")


@pytest.fixture(scope="module")
def partitions_show(W):
    """The condition of the value tests, on the reference alone: m = 33, T = T0."""
    T = _t0(W)
    X, mu = _wide(33, T)
    for centre in (None, mu):
        assert _tells_partitions_apart(X, centre, (1, W - 1, W + 1), T)
    return True


# ---------------------------------------------------------------- values and memory on every layout
@pytest.mark.parametrize("m,pad", SHAPES)
def test_bit_equal_on_every_layout_in_four_forms(L, W, partitions_show, m, pad):
    T = _t0(W)
    X, mu = _wide(m, T)
    if m >= 33:
        assert _tells_partitions_apart(X, mu, (1, W - 1, W + 1), T)
    segs = (1, 8, 16, T, 100)
    cases = [(seg, lags) for seg in segs for lags in _lag_lists(seg, W, T)]
    inputs, seen_x = {}, set()
    for i, (seg, lags) in enumerate(cases):
        ox, om, oo = OFFSETS[(i + i // 8) % 8]
        if (ox, om) not in inputs:
            inputs[ox, om] = _inputs(X, mu, ox, om, pad)
        gX, gmu = inputs[ox, om]
        seen_x.add(ox)
        centre = None if i % 3 == 0 else mu
        what = f"seg {seg} lags {lags} mu {centre is not None} offsets {(ox, om, oo)}"
        got = _checked(L, gX, None if centre is None else gmu, lags, seg, m, pad, oo, what)
        _same(got, lr.moments(X, lags, centre, seg), what)
    assert seen_x == {0, 1, 2, 3}
    _inputs_unchanged(*[g for pair in inputs.values() for g in pair])


@pytest.mark.parametrize("pad", [0, 7])
def test_more_than_eight_segments_and_a_mixed_list(L, W, pad):
    """T = 77 with seg = 8: nine full segments and a tail of 5; lags on both sides of the ring, the partner of the far
    ones several segments back."""
    m, T = 1029, 77
    X, mu = _wide(m, T, seed=3)
    lags = sorted({0, 1, 7, 8, W - 1, W, W + 1, 40})
    assert len(lags) == 8 and _tells_partitions_apart(X, mu, lags, T)
    for (ox, om, oo), centre in (((0, 0, 0), mu), ((1, 3, 1), None)):
        gX, gmu = _inputs(X, mu, ox, om, pad)
        what = f"T = 77 offsets {(ox, om, oo)}"
        got = _checked(L, gX, None if centre is None else gmu, lags, 8, m, pad, oo, what)
        _same(got, lr.moments(X, lags, centre, 8), what)
        _inputs_unchanged(gX, gmu)


def test_a_single_snapshot_and_more_segments_than_grid_rows(L, W):
    X, mu = _wide(5, 1, seed=9)
    gX, gmu = _inputs(X, mu, 0, 0, 0)
    for seg in (1, 8):
        _same(_checked(L, gX, gmu, [0], seg, 5, 3, 0, "T = 1"), lr.moments(X, [0], mu, seg), "T = 1")
    # T = 65 535 + 13 snapshots with seg = 1: grid.y of the split form is strided over 65 548 segments
    T = 65535 + 13
    X, mu = _wide(5, T, seed=10)
    gX, gmu = _inputs(X, mu, 0, 0, 0)
    _same(_checked(L, gX, gmu, [3], 1, 5, 0, 0, "65 548 segments"), lr.moments(X, [3], mu, 1), "65 548 segments")
    _inputs_unchanged(gX, gmu)


# ---------------------------------------------------------------- value domain
def test_non_finite_values_reach_their_own_planes_only(L, W, partitions_show):
    m, T = 41, _t0(W)
    X, _ = _wide(m, T, seed=11)
    lags = [0, 2, W, W + 4]
    n = len(lags)
    clean = lr.moments(X, lags, None, 8)
    for t in (1, T // 2, T - 2):                                  # the head, the middle and the tail
        Xn = X.copy()
        Xn[3, t], Xn[20, t] = np.nan, np.inf
        Xn[7:10] = 0.0
        want = lr.moments(Xn, lags, None, 8)
        # what the reference marks: S; P_l where t is the later (t >= tau_l) or the earlier (t + tau_l < T) member of a
        # pair; H_l where t < tau_l; E_l where t >= T - tau_l
        marks = np.array([True] + [t >= tau or t + tau < T for tau in lags] + [t < tau for tau in lags]
                         + [t >= T - tau for tau in lags])
        assert np.array_equal(~np.isfinite(want[:, 3]), marks) and np.array_equal(~np.isfinite(want[:, 20]), marks)
        gX = mg.Guarded(m, T, m, F32, 0, DEV).fill(Xn).snapshot()
        got = _checked(L, gX, None, lags, 8, m, 0, 0, f"NaN / Inf at t = {t}")
        _same(got, want, f"NaN / Inf at t = {t}")
        assert np.array_equal(~np.isfinite(got[:, 3]), marks) and np.array_equal(~np.isfinite(got[:, 20]), marks)
        assert np.isnan(got[marks, 3]).all() and (got[[0, 1], 20] == np.inf).all()      # S and P of lag 0
        rest = np.ones(m, dtype=bool)
        rest[[3, 7, 8, 9, 20]] = False
        assert np.array_equal(_bits(got[:, rest]), _bits(clean[:, rest]))            # the neighbours keep their bits
        assert (_bits(got[:, 7:10]) == 0).all()                                      # rows of zeros: +0.0 everywhere
        _inputs_unchanged(gX)


# ---------------------------------------------------------------- refusals and empty shapes
def test_refusals_write_nothing(L, W):
    m, T, n = 12, 37, 3
    X, mu = _wide(m, T)
    lags = [1, 5, W + 1]
    ld, big, st = m + 2, 2**31, _stream()
    gX = mg.Guarded(m, T, ld, F32, 0, DEV).fill(X).snapshot()
    gmu = mg.Guarded(m, 1, m, F32, 0, DEV).fill(mu.reshape(-1, 1)).snapshot()
    gO = mg.Guarded(m, 1 + 3 * n, ld, F64, 0, DEV)
    wbytes = int(L.dmdx_lag_moments_workspace_bytes(m, T, n, 8))
    ws = mg.Workspace(wbytes, DEV)

    def host(*v):
        return (ctypes.c_int32 * len(v))(*v)

    good = dict(X=gX.ptr, m=m, T=T, ldx=ld, mu=gmu.ptr, lags=host(*lags), L=n, seg=8, out=gO.ptr, ldo=ld, flags=0, ws=ws.ptr,
                wbytes=wbytes)
    nine = host(0, 1, 2, 3, 4, 5, 6, 7, 8)
    bad = [dict(L=0), dict(L=9, lags=nine), dict(L=-1), dict(lags=None), dict(lags=host(1, 5, 5)), dict(lags=host(5, 1, 20)),
           dict(lags=host(-1, 5, 20)), dict(lags=host(1, 5, T)), dict(lags=host(1, 5, 2**31 - 1)), dict(seg=0), dict(seg=-5),
           dict(seg=big), dict(ldo=m - 1), dict(ldx=m - 1), dict(out=gO.ptr + 4), dict(X=gX.ptr + 2), dict(mu=gmu.ptr + 1),
           dict(ws=ws.ptr + 4), dict(wbytes=wbytes - 1), dict(flags=2), dict(flags=4 | 1), dict(flags=-1), dict(X=None),
           dict(out=None), dict(m=-1), dict(T=-1), dict(m=big, ldx=big, ldo=big), dict(T=big), dict(ldx=big), dict(ldo=big),
           dict(out=gX.ptr), dict(out=gX.ptr + 8 * 5)]
    for change in bad:
        for nows in ({}, dict(ws=None, wbytes=0)):
            if ("ws" in change or "wbytes" in change) and nows:
                continue
            assert L.dmdx_lag_moments_f32(*{**good, **change, **nows}.values(), st) == E_INVALID, change
            assert b"lag_moments" in L.dmdx_last_error()
    # sizes of zero: the checks, then nothing to do and nothing written (null X and out are allowed then)
    for change in (dict(m=0), dict(T=0), dict(m=0, X=None, out=None), dict(T=0, X=None, out=None)):
        assert L.dmdx_lag_moments_f32(*{**good, **change}.values(), st) == 0, L.dmdx_last_error()
        assert L.dmdx_lag_moments_f32(*{**good, **change, "ws": None, "wbytes": 0}.values(), st) == 0
    torch.cuda.synchronize()
    assert bool((gO.ibuf == gO.canary).all())
    ws.check_untouched("workspace")
    ws.check_unused("workspace")
    _inputs_unchanged(gX, gmu)
    # ... and the same arguments, unchanged, run
    assert L.dmdx_lag_moments_f32(*good.values(), st) == 0, L.dmdx_last_error()
    _same(gO.logical().T, lr.moments(X, lags, mu, 8), "after the refusals")
    gO.check_untouched("out")
    ws.check_untouched("workspace")
