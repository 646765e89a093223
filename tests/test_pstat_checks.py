"""The argument checks of K29 (dmdx_period_stats_f32, dmdx_period_stats_workspace_bytes) through ctypes, without a GPU:
they run before HIP is touched.  Every refusal of include/dmdx.h returns DMDX_E_INVALID and names the entry point in
dmdx_last_error(); the workspace is exactly N 8 m doubles with N the pieces of all periods, a piece being ``seg`` days
of ``group`` snapshots."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1000
BOUNDS = (2, 9, 10, 50, 93)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(ROOT, "dmd_era5_amd", "libdmdx.so")):
        import __graft_entry__

        __graft_entry__.build()
    from dmd_era5_amd import _lib

    return _lib.load()


def i32(*v):
    return (ctypes.c_int32 * len(v))(*v)


def pieces(bounds, group, seg):
    return sum(-(-(-(-(y - x) // group)) // seg) for x, y in zip(bounds, bounds[1:]))


def test_limits_and_version(lib):
    assert (lib.dmdx_period_stats_max_window(), lib.dmdx_period_stats_max_periods(), lib.dmdx_version()) == (8, 128, 110)


def test_every_refusal_returns_invalid_and_names_the_entry_point(lib):
    one = 0x10000               # non-null aligned addresses that are never used: every call below is refused before a launch
    m, T, P = 10, 97, 4
    X, thr, out, ws = one, one + 0x100000, one + 0x300000, one + 0x400000
    good = dict(X=X, m=m, T=T, ldx=12, bounds=i32(*BOUNDS), P=P, group=3, inner=0, window=2, min_count=2, thr=thr, seg=4,
                out=out, ldo=10, flags=1, ws=None, wsb=0, stream=None)
    need = lib.dmdx_period_stats_workspace_bytes(m, good["bounds"], P, 3, 4)
    assert need == (1 + 1 + 4 + 4) * 8 * m * 8            # 3, 1, 14 and 15 days in pieces of 4

    def call(**over):
        a = dict(good)
        a.update(over)
        return lib.dmdx_period_stats_f32(*a.values())

    many = i32(*range(130))
    big = 2 ** 31
    bad = [dict(X=None), dict(out=None), dict(bounds=None),
           dict(P=0), dict(P=129, bounds=many), dict(P=-1),
           dict(bounds=i32(2, 9, 9, 50, 93)), dict(bounds=i32(2, 9, 8, 50, 93)), dict(bounds=i32(-1, 9, 10, 50, 93)),
           dict(bounds=i32(2, 9, 10, 50, 98)), dict(bounds=i32(2, 9, 10, 50, 2 ** 31 - 1)),
           dict(group=0), dict(group=-3), dict(group=big, min_count=1), dict(inner=-1), dict(inner=5), dict(window=0),
           dict(window=9), dict(window=-1), dict(min_count=0), dict(min_count=4), dict(min_count=-2),
           dict(seg=0), dict(seg=-4), dict(seg=big), dict(flags=4), dict(flags=8), dict(flags=7), dict(flags=1 << 31),
           dict(ldx=9), dict(ldo=9), dict(m=-1), dict(T=-1), dict(T=big), dict(ldx=big), dict(ldo=big),
           dict(m=big, ldx=big, ldo=big),
           dict(X=X + 2), dict(thr=thr + 1), dict(out=out + 4), dict(out=out + 3), dict(ws=ws + 4, wsb=need),
           dict(out=X), dict(out=X + 8 * 20), dict(out=thr), dict(out=thr - 8 * 5), dict(X=out + 8 * 5), dict(thr=out + 8 * 40),
           dict(ws=ws, wsb=need - 1), dict(ws=ws, wsb=0)]
    for over in bad:
        assert call(**over) == E_INVALID, over
        assert b"period_stats" in lib.dmdx_last_error(), over
    # m == 0 passes the checks and launches nothing: null X, thr and out are allowed then
    assert call(m=0) == 0 and call(m=0, X=None, thr=None, out=None) == 0
    assert call(m=0, seg=0) == E_INVALID                               # ... after the checks
    assert call(m=0, window=9) == E_INVALID


@pytest.mark.parametrize("group,seg", [(1, 1), (1, 4), (3, 2), (4, 7), (24, 1), (24, 100), (1, 100), (100, 1)])
def test_workspace_bytes_is_the_formula(lib, group, seg):
    b = i32(*BOUNDS)
    n = pieces(BOUNDS, group, seg)
    for m in (1, 3, 1029):
        assert lib.dmdx_period_stats_workspace_bytes(m, b, 4, group, seg) == n * 8 * m * 8
    assert lib.dmdx_period_stats_workspace_bytes(0, b, 4, group, seg) == 0
    assert lib.dmdx_period_stats_workspace_bytes(7, b, 2, group, seg) == pieces(BOUNDS[:3], group, seg) * 7 * 64


def test_the_pieces_of_the_formula_by_hand():
    assert pieces(BOUNDS, 1, 1) == 91 and pieces(BOUNDS, 3, 2) == 2 + 1 + 7 + 8 and pieces(BOUNDS, 24, 1) == 1 + 1 + 2 + 2
    assert pieces(BOUNDS, 4, 7) == 1 + 1 + 2 + 2 and pieces(BOUNDS, 100, 1) == 4


def test_workspace_bytes_is_zero_for_what_the_call_refuses(lib):
    b = i32(*BOUNDS)
    for args in ((-1, b, 4, 1, 4), (2 ** 31, b, 4, 1, 4), (5, None, 4, 1, 4), (5, b, 0, 1, 4), (5, b, 129, 1, 4),
                 (5, b, 4, 0, 4), (5, b, 4, -1, 4), (5, b, 4, 2 ** 31, 4), (5, b, 4, 1, 0), (5, b, 4, 1, 2 ** 31),
                 (5, i32(2, 2, 3), 2, 1, 4), (5, i32(-1, 2, 3), 2, 1, 4)):
        assert lib.dmdx_period_stats_workspace_bytes(*args) == 0, args
    # the largest shapes saturate instead of wrapping
    big = lib.dmdx_period_stats_workspace_bytes(2 ** 31 - 1, i32(0, 2 ** 31 - 1), 1, 1, 1)
    assert big == 2 ** 64 - 1
