"""K29 (dmdx_period_stats_f32) through the ctypes table: all eight planes equal to tests/pstat_ref.py (the host
definition, a plain loop; the kernel is never its own reference) in every bit, the memory contract on operands from
tests/memguard.py (canaries in pads and guard zones, an exact workspace) and the refusals.

Every case runs in two forms -- time split over workgroups through a workspace with an ordered merge of the piece
records, or one lane walking the periods of its rows -- and with pieces of 1, 2, 7 and 100 days.  The partition is part
of the totals (planes 5 and 6), so the kernel at a seg is compared with the reference at the same seg; the form is part
of nothing.

Inputs: AR(1) noise (phi = 0.8) on a grid of 1/4, so that equal maxima and exact ties with the thresholds occur and
every sum of a "sum", "max", "min" or "range" case is exact; NaN, +Inf and -Inf each on about 2 % of the elements;
per-row thresholds on the same grid with some NaN; row 2 all NaN over the period [10, 50).  That the inputs hold what
can go wrong is asserted on the reference before a kernel runs.  fp32 values summed in fp64 are exact unless their
exponents spread by about 29 bits, so ordinary inputs cannot show a wrong summation order: the partition contract has
a case of its own with exponents spread over 60 bits.
"""
import ctypes

import numpy as np
import pytest
import torch

import memguard as mg
import pstat_ref as pr

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DEV = "cuda"
E_INVALID = -1000
T0 = 97
BOUNDS = [2, 9, 10, 50, 93]          # a start past 0, a period of one snapshot, an end before T
SEGS = (1, 2, 7, 100)
SHAPES = [(m, pad) for m in (1, 3, 1029, 2053) for pad in (0, 7)]
# (group, window, inner, min_count): a covering list, not the product
COMBOS = [(1, 1, "sum", 1), (1, 8, "mean", 1), (1, 2, "max", 1), (1, 5, "min", 1), (3, 1, "sum", 2), (3, 5, "mean", 1),
          (3, 2, "min", 3), (3, 8, "range", 1), (4, 2, "range", 3), (4, 1, "max", 1), (4, 8, "sum", 1), (4, 5, "mean", 4),
          (24, 1, "range", 23), (24, 2, "sum", 1), (24, 1, "mean", 24)]
FORMS = [(False, False), (True, False), (False, True), (True, True)]          # (below, inclusive)
N, MAX, ARGMAX, MIN, ARGMIN, TOTAL, ETOTAL, ECOUNT = range(8)


def test_the_list_covers_every_setting():
    assert {c[0] for c in COMBOS} == {1, 3, 4, 24} and {c[1] for c in COMBOS} == {1, 2, 5, 8}
    assert {c[2] for c in COMBOS} == set(pr.INNER)
    for g in (3, 4, 24):
        assert {c[3] for c in COMBOS if c[0] == g} == {g, g - 1, 1}


@pytest.fixture(scope="module")
def L():
    from dmd_era5_amd.kernels import default_kernels

    lib = default_kernels()._lib
    assert lib.dmdx_period_stats_max_window() == 8 and lib.dmdx_period_stats_max_periods() == 128
    return lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _i32(v):
    return (ctypes.c_int32 * len(v))(*[int(x) for x in v])


def _case(m, T=T0, seed=0):
    """-> X (m, T) fp32 and thr (m,) fp32."""
    rs = np.random.RandomState(seed + m)
    X = np.empty((m, T))
    x = rs.standard_normal(m) / 0.6
    for t in range(T):
        x = 0.8 * x + rs.standard_normal(m)
        X[:, t] = x
    X = (np.round(X * 4) / 4).astype(np.float32)
    n = max(1, m * T // 50)
    for val in (np.nan, np.inf, -np.inf):
        X[rs.randint(0, m, n), rs.randint(0, T, n)] = val
    if m >= 3:
        X[2, 10:50] = np.nan
    thr = (np.round(rs.standard_normal(m) * 4) / 4).astype(np.float32)
    thr[rs.randint(0, m, m // 50 + 1)] = np.nan
    if m >= 3:
        thr[:3] = (0.0, 0.25, 1.0)
    return X, thr


_RUNS = {}


def _runs(m, X, combo, bounds=BOUNDS, seed=0):
    """The running values of a case, computed once: everything of the reference that thr and seg are no part of."""
    key = (m, combo, tuple(bounds), seed)
    if key not in _RUNS:
        g, w, inner, mc = combo
        _RUNS[key] = pr.running_of_periods(X, bounds, g, inner, w, mc)
    return _RUNS[key]


def _what_can_go_wrong(runs, thr, window):
    """On the reference alone -> (rows with a tied maximum in a period, cells with n = 0, r_k equal to the threshold,
    cells with a window across a piece boundary at seg = 2)."""
    ties = empty = on_thr = across = 0
    with np.errstate(invalid="ignore"):
        for r, rk in runs:
            top = np.where(rk, r, -np.inf).max(axis=1) if r.shape[1] else np.full(r.shape[0], -np.inf)
            ties += int(((rk & (r == top[:, None])).sum(axis=1) > 1).sum())
            empty += int((~rk.any(axis=1)).sum())
            on_thr += int((rk & (r == thr.astype(np.float64)[:, None])).sum())
            k = np.arange(r.shape[1])
            across += int(rk[:, (k - window + 1) // 2 != k // 2].any(axis=1).sum())
    return ties, empty, on_thr, across


@pytest.fixture(scope="module")
def inputs_hold_what_can_go_wrong():
    """The condition of the value tests, on the reference alone, at m = 1029."""
    X, thr = _case(1029)
    total = np.zeros(4, dtype=np.int64)
    for combo in COMBOS:
        g, w, inner, mc = combo
        found = _what_can_go_wrong(_runs(1029, X, combo), thr, w)
        total += found
        assert found[1] >= 1, (combo, found)                        # row 2 of period [10, 50) at the least
        if g <= 4 and w <= 5 and inner != "mean":                  # periods of several days with values on the grid
            assert found[0] >= 1 and found[2] >= 1, (combo, found)
        if w > 1 and g <= 4:
            assert found[3] >= 1, (combo, found)
    assert (total >= 1).all()
    return True


class Operands:
    """The guarded inputs of one (m, pad) shape, made once per base offset."""

    def __init__(self, X, thr, pad):
        self.X, self.thr, self.pad = X, thr, pad
        self.m, self.T = X.shape
        self._x, self._t = {}, {}

    def x(self, off):
        if off not in self._x:
            self._x[off] = mg.Guarded(self.m, self.T, self.m + self.pad, F32, off, DEV).fill(self.X).snapshot()
        return self._x[off]

    def t(self, off):
        if off not in self._t:
            self._t[off] = mg.Guarded(self.m, 1, self.m + self.pad, F32, off, DEV).fill(self.thr.reshape(-1, 1)).snapshot()
        return self._t[off]

    def unchanged(self):
        for g in list(self._x.values()) + list(self._t.values()):
            g.check_untouched("input")
            g.check_unchanged("input")


def _out(m, P, pad, off):
    return mg.Guarded(m, 8 * P, m + pad, F64, off, DEV)


def _planes(gO, P):
    return gO.view.cpu().numpy().reshape(8, P, gO.rows)


def _run(L, gX, gT, combo, bounds, seg, form, gO, split, **kw):
    """One call; split: through an exact workspace between canaries, else workspace == NULL.  -> (rc, workspace)."""
    g, w, inner, mc = combo
    a = dict(X=gX.ptr, m=gX.rows, T=gX.cols, ldx=gX.ld, bounds=_i32(bounds), P=len(bounds) - 1, group=g,
             inner=pr.INNER.index(inner), window=w, min_count=mc, thr=None if gT is None else gT.ptr, seg=seg, out=gO.ptr,
             ldo=gO.ld, flags=(1 if form[0] else 0) | (2 if form[1] else 0))
    a.update(kw)
    ws, wptr, wbytes = None, None, 0
    if split:
        wbytes = int(L.dmdx_period_stats_workspace_bytes(a["m"], a["bounds"], a["P"], a["group"], a["seg"]))
        assert wbytes == pr.n_pieces(bounds, g, seg) * 8 * gX.rows * 8
        ws = mg.Workspace(wbytes, DEV)
        wptr = ws.ptr
    rc = L.dmdx_period_stats_f32(*a.values(), wptr, wbytes, _stream())
    return rc, ws


def _checked(L, gX, gT, combo, bounds, seg, form, pad, oo, what):
    """Both forms of one case -> the (8, P, m) planes, after the memory checks; the forms agree in every bit."""
    res = []
    P = len(bounds) - 1
    for split in (True, False):
        gO = _out(gX.rows, P, pad, oo)
        rc, ws = _run(L, gX, gT, combo, bounds, seg, form, gO, split)
        assert rc == 0, L.dmdx_last_error()
        res.append(_planes(gO, P))
        gO.check_fully_written(what)
        gO.check_untouched(what)
        if ws is not None:
            ws.check_untouched(what)
    _differs(res[0], res[1], f"{what}: the split form against the walk form")
    return res[0]


def _differs(got, want, what):
    """Bit for bit; NaN equals NaN."""
    g, w = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.argwhere((g.view(np.int64) != w.view(np.int64)) & ~(np.isnan(g) & np.isnan(w)))
    assert bad.size == 0, (f"{what}: {bad.shape[0]} of {w.size} elements differ, first at (q, p, row) = "
                           f"{tuple(bad[0])}: {g[tuple(bad[0])]!r} for {w[tuple(bad[0])]!r}")


# ---------------------------------------------------------------- values and memory on every layout
@pytest.mark.parametrize("m,pad", SHAPES)
def test_equal_on_every_layout_in_both_forms_for_every_seg(L, inputs_hold_what_can_go_wrong, m, pad):
    X, thr = _case(m)
    ops = Operands(X, thr, pad)
    seen, i = set(), 0
    for combo in COMBOS:
        runs = _runs(m, X, combo)
        for seg in SEGS:
            # the X of every other case starts 1 .. 3 floats past a 16-byte boundary: the dword path
            ox, ot, oo = (0 if i % 2 == 0 else (i // 2) % 3 + 1), (i // 3) % 4, i % 2
            form, with_thr = FORMS[(i // 2) % 4], i % 5 != 4
            seen.add((ox, form, with_thr))
            i += 1
            what = f"{combo} seg {seg} form {form} thr {with_thr} offsets {(ox, ot, oo)}"
            want = pr.planes_of(runs, thr if with_thr else None, form[0], form[1], seg)
            got = _checked(L, ops.x(ox), ops.t(ot) if with_thr else None, combo, BOUNDS, seg, form, pad, oo, what)
            _differs(got, want, what)
    assert {s[0] for s in seen} == {0, 1, 2, 3} and {s[1:] for s in seen} == {(f, t) for f in FORMS for t in (True, False)}
    ops.unchanged()


@pytest.mark.parametrize("pad", [0, 7])
def test_one_period_over_everything_in_days_of_24_and_all_four_comparisons(L, pad):
    m = 1029
    X, thr = _case(m, seed=3)
    ops = Operands(X, thr, pad)
    for combo, bounds in (((24, 1, "max", 20), [0, T0]), ((24, 2, "sum", 1), [0, T0]), ((1, 1, "sum", 1), [T0 - 1, T0]),
                          ((3, 2, "range", 2), [0, 1, 2, T0])):
        runs = _runs(m, X, combo, bounds, seed=3)
        for k, form in enumerate(FORMS):
            for with_thr in (True, False):
                seg = SEGS[(k + with_thr) % 4]
                what = f"{combo} bounds {bounds} form {form} thr {with_thr} seg {seg}"
                want = pr.planes_of(runs, thr if with_thr else None, form[0], form[1], seg)
                got = _checked(L, ops.x(0), ops.t(k) if with_thr else None, combo, bounds, seg, form, pad, k % 2, what)
                _differs(got, want, what)
                if not with_thr:
                    assert not got[ETOTAL:].any() and not np.signbit(got[ETOTAL:]).any()      # +0.0
    # the four forms do differ on these inputs: exact ties with the threshold occur
    runs = _runs(m, X, (3, 2, "range", 2), [0, 1, 2, T0], seed=3)
    counts = [pr.planes_of(runs, thr, b, i, 7)[ECOUNT].sum() for b, i in FORMS]
    assert counts[2] > counts[0] and counts[3] > counts[1]
    ops.unchanged()


# ---------------------------------------------------------------- the partition contract
WIDE = [(1, 1, "sum", 1), (3, 1, "sum", 3), (3, 5, "mean", 3), (4, 2, "range", 4)]


@pytest.mark.parametrize("combo", WIDE)
def test_the_partition_is_part_of_the_totals_and_the_form_is_not(L, combo):
    """standard_normal * 2^randint(-30, 31): the fp64 sum of such values depends on its order.  The reference's totals
    at seg = 2 and seg = 7 differ in at least 10 % of the 1028 cells and agree in every other plane; the kernel at
    either seg equals the reference at that seg, in both forms."""
    m = 257
    rs = np.random.RandomState(5)
    X = (rs.standard_normal((m, T0)) * np.exp2(rs.randint(-30, 31, (m, T0)))).astype(np.float32)
    g, w, inner, mc = combo
    runs = pr.running_of_periods(X, BOUNDS, g, inner, w, mc)
    want = {seg: pr.planes_of(runs, None, False, False, seg) for seg in (2, 7)}
    assert want[2][TOTAL].size == 1028
    differ = int((want[2][TOTAL] != want[7][TOTAL]).sum())
    print(f"{combo}: the totals of seg 2 and seg 7 differ in {differ} of 1028 cells")
    assert differ >= 103
    assert np.array_equal(np.delete(want[2], TOTAL, 0), np.delete(want[7], TOTAL, 0), equal_nan=True)
    ops = Operands(X, np.zeros(m, dtype=np.float32), 3)
    for seg in (2, 7):
        got = _checked(L, ops.x(0), None, combo, BOUNDS, seg, (False, False), 3, 1, f"wide {combo} seg {seg}")
        _differs(got, want[seg], f"wide {combo} seg {seg}")
    ops.unchanged()


# ---------------------------------------------------------------- the wrapper: more periods than a launch takes
def test_130_periods_through_the_wrapper(L):
    from dmd_era5_amd.kernels import default_kernels

    K = default_kernels()
    rs = np.random.RandomState(8)
    bounds = np.concatenate([[3], 3 + np.cumsum(rs.randint(1, 4, 130))]).tolist()
    m, T = 517, bounds[-1] + 2
    X, thr = _case(m, T=T, seed=5)
    assert len(bounds) - 1 == 130 > K.period_stats_max_periods and K.period_stats_max_window == 8
    Xd, td = torch.from_numpy(np.ascontiguousarray(X.T)).to(DEV), torch.from_numpy(thr).to(DEV)
    for seg in (1, 2):
        want = pr.period_stats(X, bounds, 1, "sum", 2, 1, thr, True, True, seg)
        got = K.period_stats(Xd, bounds, group=1, inner="sum", window=2, thr=td, below=True, inclusive=True, seg=seg)
        assert got.shape == (8, 130, m) and got.dtype == F64
        _differs(got.cpu().numpy(), want, f"130 periods seg {seg}")
    assert (want[N] > 0).any() and (want[N] == 0).any()


# ---------------------------------------------------------------- refusals
def test_refusals_write_nothing(L):
    m, P, seg = 12, 4, 2
    combo = (3, 2, "sum", 2)
    X, thr = _case(m)
    ops = Operands(X, thr, 2)
    gX, gT = ops.x(0), ops.t(0)
    gO = _out(m, P, 2, 0)
    b = _i32(BOUNDS)
    wbytes = int(L.dmdx_period_stats_workspace_bytes(m, b, P, 3, seg))
    assert wbytes == pr.n_pieces(BOUNDS, 3, seg) * 8 * m * 8
    ws = mg.Workspace(wbytes, DEV)
    st, big = _stream(), 2 ** 31
    good = dict(X=gX.ptr, m=m, T=T0, ldx=gX.ld, bounds=b, P=P, group=3, inner=0, window=2, min_count=2, thr=gT.ptr, seg=seg,
                out=gO.ptr, ldo=gO.ld, flags=2, ws=ws.ptr, wbytes=wbytes)
    bad = [dict(X=None), dict(out=None), dict(bounds=None), dict(P=0), dict(P=129, bounds=_i32(range(130))),
           dict(bounds=_i32([2, 9, 9, 50, 93])), dict(bounds=_i32([2, 10, 9, 50, 93])), dict(bounds=_i32([-1, 9, 10, 50, 93])),
           dict(bounds=_i32([2, 9, 10, 50, 98])), dict(group=0), dict(group=big, min_count=1), dict(inner=-1), dict(inner=5),
           dict(window=0), dict(window=9), dict(min_count=0), dict(min_count=4), dict(seg=0), dict(seg=-5), dict(seg=big),
           dict(flags=4), dict(flags=1 << 31), dict(ldx=m - 1), dict(ldo=m - 1), dict(m=-1), dict(T=-1), dict(T=big),
           dict(ldx=big), dict(ldo=big), dict(m=big, ldx=big, ldo=big), dict(X=gX.ptr + 2), dict(thr=gT.ptr + 1),
           dict(out=gO.ptr + 4), dict(ws=ws.ptr + 4), dict(wbytes=wbytes - 1), dict(out=gX.ptr), dict(out=gX.ptr + 8 * 5),
           dict(out=gT.ptr), dict(thr=gO.ptr + 8 * gO.ld)]
    for change in bad:
        for nows in ({}, dict(ws=None, wbytes=0)):
            if ("ws" in change or "wbytes" in change) and nows:
                continue
            assert L.dmdx_period_stats_f32(*{**good, **change, **nows}.values(), st) == E_INVALID, change
            assert b"period_stats" in L.dmdx_last_error()
    # no rows: the checks, then nothing to do and nothing written (null X, thr and out are allowed then)
    for change in (dict(m=0), dict(m=0, X=None, thr=None, out=None)):
        assert L.dmdx_period_stats_f32(*{**good, **change}.values(), st) == 0, L.dmdx_last_error()
        assert L.dmdx_period_stats_f32(*{**good, **change, "ws": None, "wbytes": 0}.values(), st) == 0
    torch.cuda.synchronize()
    assert bool((gO.ibuf == gO.canary).all())
    ws.check_untouched("workspace")
    ws.check_unused("workspace")
    ops.unchanged()
    # ... and the same arguments, unchanged, run
    assert L.dmdx_period_stats_f32(*good.values(), st) == 0, L.dmdx_last_error()
    _differs(_planes(gO, P), pr.period_stats(X, BOUNDS, 3, "sum", 2, 2, thr, False, True, seg), "after the refusals")
    gO.check_fully_written("out")
    gO.check_untouched("out")
    ws.check_untouched("workspace")
    ops.unchanged()
