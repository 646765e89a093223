"""The argument checks of K32 (dmdx_mk_stats_f32, dmdx_sen_slopes_f32) through ctypes, without a GPU: they run before
HIP is touched.  Every refusal of include/dmdx.h returns DMDX_E_INVALID and names the entry point in
dmdx_last_error()."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1000
BIG = 2 ** 31


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(ROOT, "dmd_era5_amd", "libdmdx.so")):
        import __graft_entry__

        __graft_entry__.build()
    from dmd_era5_amd import _lib

    return _lib.load()


def f64(*v):
    return (ctypes.c_double * len(v))(*v)


def test_limits_and_version(lib):
    assert (lib.dmdx_mk_max_n(), lib.dmdx_sen_max_ranks(), lib.dmdx_version()) == (128, 4, 110)


# non-null aligned addresses that are never used: every call below is refused before a launch, or has m == 0
Y, RANK, OUT = 0x10000, 0x10000 + 0x100000, 0x10000 + 0x300000
M, N = 10, 9


def test_every_refusal_of_mk_stats(lib):
    good = dict(Y=Y, m=M, n=N, ldy=12, out=OUT, ldo=11, stream=None)

    def call(**over):
        a = dict(good)
        a.update(over)
        return lib.dmdx_mk_stats_f32(*a.values())

    bad = [dict(Y=None), dict(out=None), dict(n=0), dict(n=129), dict(n=-1), dict(n=BIG), dict(m=-1),
           dict(m=BIG, ldy=BIG, ldo=BIG), dict(ldy=BIG), dict(ldo=BIG), dict(ldy=9), dict(ldo=9),
           dict(Y=Y + 2), dict(out=OUT + 1), dict(out=OUT + 2),
           dict(out=Y), dict(out=Y + 4 * 20), dict(out=Y - 4 * 20), dict(Y=OUT + 4 * 11 * 3), dict(out=Y + 4 * (8 * 12 + 9))]
    for over in bad:
        assert call(**over) == E_INVALID, over
        assert b"mk_stats" in lib.dmdx_last_error(), over
    # out right behind the last logical element of Y, and Y right behind out: no overlap
    assert call(m=0) == 0
    assert call(m=0, out=Y + 4 * (8 * 12 + 10)) == 0
    assert call(m=0, n=129) == E_INVALID                             # ... after the checks
    assert call(m=0, Y=None) == E_INVALID


def test_every_refusal_of_sen_slopes(lib):
    tc = f64(*[1.0 * t * t for t in range(N)])
    good = dict(Y=Y, m=M, n=N, ldy=12, tc=tc, rank=RANK, ldr=10, J=4, out=OUT, ldo=11, stream=None)

    def call(**over):
        a = dict(good)
        a.update(over)
        return lib.dmdx_sen_slopes_f32(*a.values())

    def axis(t, value):
        v = [float(k) for k in range(N)]
        v[t] = value
        return f64(*v)

    inf, nan = float("inf"), float("nan")
    bad = [dict(Y=None), dict(out=None), dict(tc=None), dict(rank=None),
           dict(n=0), dict(n=129), dict(n=-1), dict(n=BIG), dict(J=0), dict(J=5), dict(J=-1), dict(m=-1),
           dict(m=BIG, ldy=BIG, ldo=BIG, ldr=BIG), dict(ldy=BIG), dict(ldo=BIG), dict(ldr=BIG),
           dict(ldy=9), dict(ldo=9), dict(ldr=9),
           dict(Y=Y + 2), dict(out=OUT + 2), dict(rank=RANK + 1), dict(tc=ctypes.c_void_p(ctypes.addressof(tc) + 4)),
           dict(tc=axis(3, nan)), dict(tc=axis(0, nan)), dict(tc=axis(8, inf)), dict(tc=axis(0, -inf)),
           dict(tc=axis(4, 3.0)), dict(tc=axis(4, 2.5)), dict(tc=axis(8, 0.0)), dict(tc=axis(1, 0.0)),
           dict(out=Y), dict(out=Y + 4 * 20), dict(Y=OUT + 4 * 11 * 3), dict(out=RANK), dict(out=RANK + 4 * 35),
           dict(rank=OUT + 4 * 11 * 3), dict(rank=OUT - 4 * 5)]
    for over in bad:
        assert call(**over) == E_INVALID, over
        assert b"sen_slopes" in lib.dmdx_last_error(), over
    assert call(m=0) == 0
    assert call(m=0, n=1, tc=f64(5.0), J=1) == 0                    # one point ascends
    assert call(m=0, tc=axis(4, 3.0)) == E_INVALID                  # ... after the checks
    assert call(m=0, J=5) == E_INVALID
    # only the n coordinates of the call are looked at
    assert call(m=0, n=4, tc=f64(0.0, 1.0, 2.0, 3.0)) == 0
