"""K27 (dmdx_spell_f32) through the ctypes table: all seven planes equal to tests/spell_ref.py (the host definition, a
plain loop; the kernel is never its own reference), the memory contract on operands from tests/memguard.py (canaries in
pads and guard zones, an exact workspace) and every refusal.

The results are integers: every comparison is exact.  Every case runs in two forms -- time split over workgroups
through a workspace with an ordered merge of the piece records, or one lane walking the periods of its rows -- and with
pieces of 1, 4, 7, 61 and 100 snapshots: all of them must give the reference's values, so neither the form nor the
partition shows in a single bit.

Inputs: AR(1) noise (phi = 0.8) on a grid of 1/4, so runs of 1 to more than 10 events and exact ties with the
thresholds occur; thresholds near the 15th / 50th / 85th percentile on the same grid, varying with the slot; NaN, +-Inf
and NaN thresholds sprinkled in; row 0 above and row 1 below every threshold (all events / no event, by the direction
of the threshold).  That the inputs hold what the merge can get wrong is asserted on the reference before a kernel
runs.  min_len is a rotation of (1, 2, 3, 6) that depends on S, so every threshold index meets a min_len > 1.
"""
import ctypes

import numpy as np
import pytest
import torch

import memguard as mg
import spell_ref as sr

pytestmark = pytest.mark.gpu

F32 = torch.float32
DEV = "cuda"
E_INVALID = -1000
T0 = 61
BOUNDS = [2, 9, 10, 37, 58]          # a start past 0, a period of one snapshot, an end before T
SEGS = (1, 4, 7, 61, 100)
SHAPES = [(m, pad) for m in (1, 3, 1029, 2053) for pad in (0, 7)]
MASKS = {1: 0b1, 2: 0b01, 3: 0b101, 4: 0b0110}
MIN_LEN = (1, 2, 3, 6)
NV, NE, NS, NIN, LONGEST, FIRST, LAST = range(7)


@pytest.fixture(scope="module")
def L():
    from dmd_era5_amd.kernels import default_kernels

    lib = default_kernels()._lib
    assert lib.dmdx_spell_max_thresholds() == 4 and lib.dmdx_spell_max_periods() == 128
    return lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _i32(v):
    return (ctypes.c_int32 * len(v))(*[int(x) for x in v])


def _above(J):
    return [bool((MASKS[J] >> j) & 1) for j in range(J)]


def _min_len(J, S):
    r = 1 if S == 1 else 2
    return [MIN_LEN[(j + r) % 4] for j in range(J)]


def _noise(m, T, seed=0):
    rs = np.random.RandomState(seed + m)
    X = np.empty((m, T))
    x = rs.standard_normal(m) / 0.6
    for t in range(T):
        x = 0.8 * x + rs.standard_normal(m)
        X[:, t] = x
    return rs, np.round(X * 4) / 4


def _case(m, T=T0, seed=0):
    """-> X (m, T) fp32, thr (4, 5, m) fp32 (a (J, S) case takes thr[:J, :S]), slot (T,) int32 with one label out of
    range."""
    rs, X = _noise(m, T, seed)
    sd = 1 / 0.6
    level = np.array([-1.04, 0.0, 1.04, 0.0])[:, None, None] * sd          # the 15th, 50th and 85th percentile
    thr = np.round((level + 0.25 * rs.standard_normal((4, 5, 1)) + 0.25 * rs.standard_normal((4, 1, m))) * 4) / 4
    X, thr = X.astype(np.float32), thr.astype(np.float32)
    n = max(1, m * T // 100)
    for val in (np.nan, np.inf, -np.inf):
        X[rs.randint(0, m, n), rs.randint(0, T, n)] = val
    thr[rs.randint(0, 4, m // 50 + 1), rs.randint(0, 5, m // 50 + 1), rs.randint(0, m, m // 50 + 1)] = np.nan
    if m >= 3:
        X[0], X[1] = 1e6, -1e6
        thr[:, :, :2] = 0.0
    slot = ((np.arange(T) // 3) % 5).astype(np.int32)
    slot[20] = 5
    return X, thr, slot


def _slot_for(slot, S):
    """The labels of an S-slot case: folded into 0 .. S - 1, the one out of range kept out of range."""
    s = (slot % S).astype(np.int32)
    s[slot == 5] = S
    return s


def _holds_what_the_merge_can_get_wrong(X, thr, slot, J, S, bounds=BOUNDS):
    """On the reference alone, for every threshold: a run across a piece boundary at seg = 4, an event on both sides of
    a period boundary, first == -1 and first >= 0, and (where min_len > 1) an n_spell that min_len = 1 does not give."""
    above, ml = _above(J), _min_len(J, S)
    _, E = sr.valid_and_event(X, thr[:J, :S], _slot_for(slot, S), above)
    want = sr.spells(X, thr[:J, :S], bounds, ml, above, _slot_for(slot, S))
    ones = sr.spells(X, thr[:J, :S], bounds, 1, above, _slot_for(slot, S))
    cuts = [t for lo, hi in zip(bounds[:-1], bounds[1:]) for t in range(lo + 4, hi, 4)]
    s = _slot_for(slot, S)
    for j in range(J):
        assert (X[:, s < S] == thr[j, s[s < S]].T).any(), j                   # an exact tie
        assert (E[j][:, [t - 1 for t in cuts]] & E[j][:, cuts]).any(), j
        assert (E[j][:, [b - 1 for b in bounds[1:-1]]] & E[j][:, bounds[1:-1]]).any(), j
        assert (want[j, FIRST] == -1).any() and (want[j, FIRST] >= 0).any(), j
        assert ml[j] == 1 or (want[j, NS] != ones[j, NS]).any(), j
        assert want[j, LONGEST].max() >= 10 and (want[j, LONGEST] == 1).any(), j
    return want


class Operands:
    """The guarded operands of one (m, pad) shape, made once per base offset."""

    def __init__(self, X, thr, slot, pad):
        self.X, self.thr, self.slot, self.pad = X, thr, slot, pad
        self.m, self.T = X.shape
        self._x, self._t, self._s = {}, {}, {}

    def x(self, off):
        if off not in self._x:
            self._x[off] = mg.Guarded(self.m, self.T, self.m + self.pad, F32, off, DEV).fill(self.X).snapshot()
        return self._x[off]

    def t(self, J, S, off):
        if (J, S, off) not in self._t:
            g = mg.Guarded(self.m, J * S, self.m + self.pad, F32, off, DEV)
            self._t[J, S, off] = g.fill(self.thr[:J, :S].reshape(J * S, self.m).T).snapshot()
        return self._t[J, S, off]

    def s(self, S):
        if S not in self._s:
            self._s[S] = torch.from_numpy(_slot_for(self.slot, S)).to(DEV)
        return self._s[S]

    def unchanged(self):
        for g in list(self._x.values()) + list(self._t.values()):
            g.check_untouched("input")
            g.check_unchanged("input")
        for S, s in self._s.items():
            assert np.array_equal(s.cpu().numpy(), _slot_for(self.slot, S))


def _out(m, J, P, pad, off):
    return mg.Guarded(m, J * 7 * P, m + pad, F32, off, DEV)


def _planes(gO, J, P):
    return gO.iview.cpu().numpy().reshape(J, 7, P, gO.rows)


def _run(L, gX, gT, slot, J, S, mask, ml, bounds, seg, gO, split, **kw):
    """One call; split: through an exact workspace between canaries, else workspace == NULL.  -> (rc, workspace)."""
    a = dict(X=gX.ptr, m=gX.rows, T=gX.cols, ldx=gX.ld, thr=gT.ptr, ldthr=gT.ld, J=J, S=S,
             slot=None if slot is None else slot.data_ptr(), above=mask, min_len=_i32(ml), bounds=_i32(bounds),
             P=len(bounds) - 1, seg=seg, out=gO.ptr, ldo=gO.ld, flags=0)
    a.update(kw)
    ws, wptr, wbytes = None, None, 0
    if split:
        wbytes = int(L.dmdx_spell_workspace_bytes(a["m"], a["bounds"], a["P"], a["J"], a["seg"]))
        assert wbytes == sr.n_pieces(bounds, seg) * J * gX.rows * sr.WS_WORDS * 4
        ws = mg.Workspace(wbytes, DEV)
        wptr = ws.ptr
    rc = L.dmdx_spell_f32(*a.values(), wptr, wbytes, _stream())
    return rc, ws


def _checked(L, gX, gT, slot, J, S, mask, ml, bounds, seg, pad, oo, what):
    """Both forms of one case -> the (J, 7, P, m) planes, after the memory checks; the forms agree."""
    res = []
    P = len(bounds) - 1
    for split in (True, False):
        gO = _out(gX.rows, J, P, pad, oo)
        rc, ws = _run(L, gX, gT, slot, J, S, mask, ml, bounds, seg, gO, split)
        assert rc == 0, L.dmdx_last_error()
        res.append(_planes(gO, J, P))
        gO.check_fully_written(what)
        gO.check_untouched(what)
        if ws is not None:
            ws.check_untouched(what)
    assert np.array_equal(res[0], res[1]), f"{what}: the split and the walk form differ"
    return res[0]


def _differs(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, (f"{what}: {bad.shape[0]} of {want.size} elements differ, first at (j, q, p, row) = "
                           f"{tuple(bad[0])}: {got[tuple(bad[0])]} for {want[tuple(bad[0])]}")


# ---------------------------------------------------------------- values and memory on every layout
@pytest.fixture(scope="module")
def merge_cases_occur():
    """The condition of the value tests, on the reference alone, at m = 1029 and 2053 for every (J, S)."""
    for m in (1029, 2053):
        X, thr, slot = _case(m)
        for J in (1, 2, 3, 4):
            for S in (1, 5):
                _holds_what_the_merge_can_get_wrong(X, thr, slot, J, S)
    return True


@pytest.mark.parametrize("m,pad", SHAPES)
def test_equal_on_every_layout_in_both_forms_for_every_seg(L, merge_cases_occur, m, pad):
    X, thr, slot = _case(m)
    ops = Operands(X, thr, slot, pad)
    seen, i = set(), 0
    for J in (1, 2, 3, 4):
        for S in (1, 5):
            above, ml = _above(J), _min_len(J, S)
            want = sr.spells(X, thr[:J, :S], BOUNDS, ml, above, _slot_for(slot, S))
            for seg in SEGS:
                ox, ot, oo = i % 4, (i // 4 + i) % 4, (3 * i + 1) % 4
                seen.add((ox, ot, oo))
                i += 1
                what = f"J {J} S {S} seg {seg} offsets {(ox, ot, oo)}"
                got = _checked(L, ops.x(ox), ops.t(J, S, ot), ops.s(S), J, S, MASKS[J], ml, BOUNDS, seg, pad, oo, what)
                _differs(got, want, what)
    for k in range(3):
        assert {o[k] for o in seen} == {0, 1, 2, 3}
    ops.unchanged()


@pytest.mark.parametrize("pad", [0, 7])
def test_no_slot_vector_and_one_period_over_everything(L, pad):
    m = 1029
    X, thr, slot = _case(m, seed=3)
    ops = Operands(X, thr, slot, pad)
    for J, bounds, seg in ((1, [0, T0], 4), (3, [0, T0], 7), (4, [0, 1, 2, T0], 1), (2, [T0 - 1, T0], 4)):
        above, ml = _above(J), _min_len(J, 1)
        want = sr.spells(X, thr[:J, :1], bounds, ml, above, None)
        got = _checked(L, ops.x(J % 4), ops.t(J, 1, (J + 1) % 4), None, J, 1, MASKS[J], ml, bounds, seg, pad, J % 4,
                       f"no slot, J {J} bounds {bounds}")
        _differs(got, want, f"no slot, J {J} bounds {bounds}")
    ops.unchanged()


def test_128_periods_in_one_call(L):
    m, T = 517, 300
    X, thr, slot = _case(m, T=T, seed=5)
    slot[20] = 0
    rs = np.random.RandomState(8)
    bounds = np.sort(rs.choice(np.arange(T + 1), 129, replace=False)).tolist()
    ops = Operands(X, thr, slot, 3)
    want = sr.spells(X, thr[:2, :5], bounds, [2, 1], _above(2), _slot_for(slot, 5))
    for seg in (1, 2, 100):
        got = _checked(L, ops.x(0), ops.t(2, 5, 1), ops.s(5), 2, 5, MASKS[2], [2, 1], bounds, seg, 3, 2, f"128 periods seg {seg}")
        _differs(got, want, f"128 periods seg {seg}")
    ops.unchanged()


def test_more_pieces_than_grid_rows_and_a_run_of_more_than_40000(L):
    """m = 5, T = 65 548, one period, seg = 1: grid.y of the split form is strided over 65 548 pieces, and the carry of
    the merge grows over more than 40 000 of them."""
    m, T = 5, 65535 + 13
    rs, X = _noise(m, T, seed=11)
    X = X.astype(np.float32)
    X[0, 100:45000] = 1e6
    X[1, :] = 1e6
    X[2, 30000] = np.nan
    thr = np.zeros((1, 1, m), dtype=np.float32)
    want = sr.spells(X, thr, [0, T], 6, True, None)
    assert want[0, LONGEST, 0, 0] >= 44900 and want[0, :, 0, 1].tolist() == [T, T, 1, T, T, 0, T - 1]
    ops = Operands(X, thr, np.zeros(T, dtype=np.int32), 0)
    got = _checked(L, ops.x(0), ops.t(1, 1, 0), None, 1, 1, 1, [6], [0, T], 1, 0, 0, "65 548 pieces")
    _differs(got, want, "65 548 pieces")
    ops.unchanged()


# ---------------------------------------------------------------- refusals
def test_refusals_write_nothing(L):
    m, J, S, P, seg = 12, 2, 5, 4, 4
    X, thr, slot = _case(m)
    ops = Operands(X, thr, slot, 2)
    gX, gT, sl = ops.x(0), ops.t(J, S, 0), ops.s(S)
    gO = _out(m, J, P, 2, 0)
    ml = [1, 3]
    b = _i32(BOUNDS)
    wbytes = int(L.dmdx_spell_workspace_bytes(m, b, P, J, seg))
    ws = mg.Workspace(wbytes, DEV)
    st, big = _stream(), 2 ** 31
    good = dict(X=gX.ptr, m=m, T=T0, ldx=gX.ld, thr=gT.ptr, ldthr=gT.ld, J=J, S=S, slot=sl.data_ptr(), above=0b01,
                min_len=_i32(ml), bounds=b, P=P, seg=seg, out=gO.ptr, ldo=gO.ld, flags=0, ws=ws.ptr, wbytes=wbytes)
    bad = [dict(X=None), dict(thr=None), dict(out=None), dict(bounds=None), dict(min_len=None), dict(J=0), dict(J=5),
           dict(S=0), dict(S=big), dict(P=0), dict(P=129, bounds=_i32(range(130))), dict(bounds=_i32([2, 9, 9, 37, 58])),
           dict(bounds=_i32([2, 10, 9, 37, 58])), dict(bounds=_i32([-1, 9, 10, 37, 58])), dict(bounds=_i32([2, 9, 10, 37, 62])),
           dict(min_len=_i32([1, 0])), dict(min_len=_i32([-1, 3])), dict(seg=0), dict(seg=-5), dict(seg=big),
           dict(above=0b100), dict(above=0b111), dict(flags=1), dict(flags=-1), dict(ldx=m - 1), dict(ldthr=m - 1),
           dict(ldo=m - 1), dict(m=-1), dict(T=-1), dict(T=big), dict(ldx=big), dict(ldthr=big), dict(ldo=big),
           dict(m=big, ldx=big, ldthr=big, ldo=big), dict(X=gX.ptr + 2), dict(thr=gT.ptr + 1), dict(out=gO.ptr + 2),
           dict(slot=sl.data_ptr() + 2), dict(ws=ws.ptr + 2), dict(wbytes=wbytes - 1), dict(out=gX.ptr),
           dict(out=gX.ptr + 4 * 5), dict(out=gT.ptr), dict(out=gT.ptr + 4 * gT.ld)]
    for change in bad:
        for nows in ({}, dict(ws=None, wbytes=0)):
            if ("ws" in change or "wbytes" in change) and nows:
                continue
            assert L.dmdx_spell_f32(*{**good, **change, **nows}.values(), st) == E_INVALID, change
            assert b"spell" in L.dmdx_last_error()
    # no rows: the checks, then nothing to do and nothing written (null X, thr and out are allowed then)
    for change in (dict(m=0), dict(m=0, X=None, thr=None, out=None)):
        assert L.dmdx_spell_f32(*{**good, **change}.values(), st) == 0, L.dmdx_last_error()
        assert L.dmdx_spell_f32(*{**good, **change, "ws": None, "wbytes": 0}.values(), st) == 0
    torch.cuda.synchronize()
    assert bool((gO.ibuf == gO.canary).all())
    ws.check_untouched("workspace")
    ws.check_unused("workspace")
    ops.unchanged()
    # ... and the same arguments, unchanged, run
    assert L.dmdx_spell_f32(*good.values(), st) == 0, L.dmdx_last_error()
    _differs(_planes(gO, J, P), sr.spells(X, thr[:J, :S], BOUNDS, ml, [True, False], _slot_for(slot, S)), "after the refusals")
    gO.check_fully_written("out")
    gO.check_untouched("out")
    ws.check_untouched("workspace")
    ops.unchanged()
