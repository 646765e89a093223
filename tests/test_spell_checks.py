"""The argument checks of K27 (dmdx_spell_f32, dmdx_spell_workspace_bytes) through ctypes, without a GPU: they run before
HIP is touched.  Every refusal of include/dmdx.h returns DMDX_E_INVALID and names the entry point in
dmdx_last_error(); the workspace is exactly N J m DMDX_SPELL_WS_WORDS int32 with N the pieces of all periods."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1000
WS_WORDS = 9
BOUNDS = (2, 9, 10, 37, 58)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(ROOT, "dmd_era5_amd", "libdmdx.so")):
        import __graft_entry__

        __graft_entry__.build()
    from dmd_era5_amd import _lib

    return _lib.load()


def i32(*v):
    return (ctypes.c_int32 * len(v))(*v)


def test_limits_and_version(lib):
    assert (lib.dmdx_spell_max_thresholds(), lib.dmdx_spell_max_periods(), lib.dmdx_version()) == (4, 128, 110)


def test_every_refusal_returns_invalid_and_names_the_entry_point(lib):
    one = 0x10000               # non-null aligned addresses that are never used: every call below is refused before a launch
    m, T, J, S, P = 10, 61, 2, 5, 4
    X, thr, slot, out, ws = one, one + 0x100000, one + 0x200000, one + 0x300000, one + 0x400000
    good = dict(X=X, m=m, T=T, ldx=12, thr=thr, ldthr=11, J=J, S=S, slot=slot, above=0b01, min_len=i32(1, 6),
                bounds=i32(*BOUNDS), P=P, seg=4, out=out, ldo=10, flags=0, ws=None, wsb=0, stream=None)
    need = lib.dmdx_spell_workspace_bytes(m, good["bounds"], P, J, 4)
    assert need == (2 + 1 + 7 + 6) * J * m * WS_WORDS * 4

    def call(**over):
        a = dict(good)
        a.update(over)
        return lib.dmdx_spell_f32(*a.values())

    many = i32(*range(130))
    bad = [dict(X=None), dict(thr=None), dict(out=None), dict(bounds=None), dict(min_len=None),
           dict(J=0), dict(J=5), dict(J=-1), dict(S=0), dict(S=-3), dict(S=2 ** 31), dict(S=2 ** 30),      # J S >= 2^31
           dict(P=0), dict(P=129, bounds=many), dict(P=-1),
           dict(bounds=i32(2, 9, 9, 37, 58)), dict(bounds=i32(2, 9, 8, 37, 58)), dict(bounds=i32(-1, 9, 10, 37, 58)),
           dict(bounds=i32(2, 9, 10, 37, 62)), dict(bounds=i32(2, 9, 10, 37, 2 ** 31 - 1)),
           dict(min_len=i32(1, 0)), dict(min_len=i32(-2, 6)), dict(seg=0), dict(seg=-4), dict(seg=2 ** 31),
           dict(above=0b100), dict(above=0b111), dict(above=1 << 31), dict(flags=1), dict(flags=2), dict(flags=-1),
           dict(ldx=9), dict(ldthr=9), dict(ldo=9), dict(m=-1), dict(T=-1), dict(T=2 ** 31), dict(ldx=2 ** 31),
           dict(ldthr=2 ** 31), dict(ldo=2 ** 31), dict(m=2 ** 31, ldx=2 ** 31, ldthr=2 ** 31, ldo=2 ** 31),
           dict(X=X + 2), dict(thr=thr + 1), dict(out=out + 3), dict(slot=slot + 2), dict(ws=ws + 2, wsb=need),
           dict(out=X), dict(out=X + 4 * 20), dict(out=thr), dict(out=thr + 4 * 11 * 3), dict(X=out + 4 * 5),
           dict(ws=ws, wsb=need - 1), dict(ws=ws, wsb=0)]
    for over in bad:
        assert call(**over) == E_INVALID, over
        assert b"spell" in lib.dmdx_last_error(), over
    # m == 0 passes the checks and launches nothing: null X, thr and out are allowed then
    assert call(m=0) == 0 and call(m=0, X=None, thr=None, out=None) == 0
    assert call(m=0, seg=0) == E_INVALID                               # ... after the checks


@pytest.mark.parametrize("seg,pieces", [(1, 56), (4, 2 + 1 + 7 + 6), (7, 1 + 1 + 4 + 3), (100, 4)])
def test_workspace_bytes_is_the_formula(lib, seg, pieces):
    b = i32(*BOUNDS)
    assert sum(-(-(y - x) // seg) for x, y in zip(BOUNDS, BOUNDS[1:])) == pieces
    for m in (1, 3, 1029):
        for J in (1, 2, 3, 4):
            assert lib.dmdx_spell_workspace_bytes(m, b, 4, J, seg) == pieces * J * m * WS_WORDS * 4
    assert lib.dmdx_spell_workspace_bytes(0, b, 4, 1, seg) == 0
    assert lib.dmdx_spell_workspace_bytes(7, b, 2, 1, seg) == sum(-(-(y - x) // seg) for x, y in zip(BOUNDS[:2], BOUNDS[1:3])) * 7 * 36


def test_workspace_bytes_is_zero_for_what_the_call_refuses(lib):
    b = i32(*BOUNDS)
    for args in ((-1, b, 4, 1, 4), (2 ** 31, b, 4, 1, 4), (5, None, 4, 1, 4), (5, b, 0, 1, 4), (5, b, 129, 1, 4),
                 (5, b, 4, 0, 4), (5, b, 4, 5, 4), (5, b, 4, 1, 0), (5, b, 4, 1, 2 ** 31), (5, i32(2, 2, 3), 2, 1, 4),
                 (5, i32(-1, 2, 3), 2, 1, 4)):
        assert lib.dmdx_spell_workspace_bytes(*args) == 0, args
    # the largest shapes saturate instead of wrapping
    big = lib.dmdx_spell_workspace_bytes(2 ** 31 - 1, i32(0, 2 ** 31 - 1), 1, 4, 1)
    assert big == (2 ** 31 - 1) ** 2 * 4 * 36 or big == 2 ** 64 - 1
