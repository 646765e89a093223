"""The host argument checks of K28 (csrc/remap_geom.h: check_remap) through libdmdx_host.so, the host-only library:
no GPU and no libdmdx.so.  dmdx_host_remap_check takes the arguments of dmdx_remap_f32 (without the stream) and returns
what that entry point returns before its first HIP call.  Every refusal of the list in include/dmdx.h, one changed
argument at a time; host memory stands in for the operands, and no call touches it."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1000
_i64, _p = C.c_int64, C.c_void_p


@pytest.fixture(scope="module")
def H():
    so = os.path.join(ROOT, "dmd_era5_amd", "libdmdx_host.so")
    if not os.path.exists(so):
        import __graft_entry__

        __graft_entry__.build()
    lib = C.CDLL(so)
    lib.dmdx_host_last_error.restype = C.c_char_p
    lib.dmdx_host_remap_max_span.restype = C.c_int
    lib.dmdx_host_remap_check.restype = C.c_int
    lib.dmdx_host_remap_check.argtypes = [_p, _i64, _i64, _i64, _i64, _i64, _i64, _p, _p, _p, C.c_int, _p, _p, _p, C.c_int, _i64,
                                          _i64, C.c_int, C.c_double, _p, _i64, _i64]
    return lib


def _good():
    """3 planes of 9 x 14 with 2 floats of pad -> 4 x 3 cells with 1 of pad, spans 3 and 5."""
    T, P, nlat, nlon, NLAT, NLON, SY, SX = 5, 3, 9, 14, 4, 3, 3, 5
    ldp, ldq = nlat * nlon + 2, NLAT * NLON + 1
    mx, my = (P - 1) * ldp + nlat * nlon, (P - 1) * ldq + NLAT * NLON
    ldx, ldy = mx + 3, my + 2
    bufs = dict(x=(C.c_float * (T * ldx + 64))(), y=(C.c_float * (T * ldy + 64))(), iy0=(C.c_int32 * NLAT)(),
                ny=(C.c_int32 * NLAT)(), wy=(C.c_double * (NLAT * SY + 1))(), jx0=(C.c_int32 * NLON)(), nx=(C.c_int32 * NLON)(),
                wx=(C.c_double * (NLON * SX + 1))())
    a = {k: C.addressof(v) for k, v in bufs.items()}
    good = dict(X=a["x"], T=T, ldx=ldx, P=P, ldp=ldp, nlat=nlat, nlon=nlon, iy0=a["iy0"], ny=a["ny"], wy=a["wy"], SY=SY,
                jx0=a["jx0"], nx=a["nx"], wx=a["wx"], SX=SX, NLAT=NLAT, NLON=NLON, skipna=0, min_frac=0.5, Y=a["y"], ldy=ldy,
                ldq=ldq)
    return good, bufs, 4 * ((T - 1) * ldx + mx), 4 * ((T - 1) * ldy + my), mx, my


def test_every_refusal_one_argument_at_a_time(H):
    assert H.dmdx_host_remap_max_span() == 64
    good, bufs, xbytes, ybytes, mx, my = _good()
    assert H.dmdx_host_remap_check(*good.values()) == 0, H.dmdx_host_last_error()
    X, Y, big = good["X"], good["Y"], 2 ** 31
    nlat, nlon, NLAT, NLON = good["nlat"], good["nlon"], good["NLAT"], good["NLON"]
    bad = [(dict(X=None), b"null"), (dict(Y=None), b"null"), (dict(iy0=None), b"null"), (dict(ny=None), b"null"),
           (dict(wy=None), b"null"), (dict(jx0=None), b"null"), (dict(nx=None), b"null"), (dict(wx=None), b"null"),
           (dict(T=-1), b"negative"), (dict(P=-1), b"negative"), (dict(nlat=-1), b"negative"), (dict(nlon=-1), b"negative"),
           (dict(NLAT=-1), b"negative"), (dict(NLON=-1), b"negative"), (dict(ldx=-1), b"negative"), (dict(ldp=-1), b"negative"),
           (dict(ldy=-1), b"negative"), (dict(ldq=-1), b"negative"),
           (dict(SY=0), b"outside 1..64"), (dict(SX=0), b"outside 1..64"), (dict(SY=65), b"outside 1..64"),
           (dict(SX=65), b"outside 1..64"), (dict(SY=-3), b"outside 1..64"),
           (dict(ldp=nlat * nlon - 1), b"ldp=125 < nlat nlon = 126"), (dict(ldq=NLAT * NLON - 1), b"ldq=11 < NLAT NLON = 12"),
           (dict(ldx=mx - 1), b"ldx="), (dict(ldy=my - 1), b"ldy="),
           (dict(T=big), b">= 2^31"), (dict(P=big), b">= 2^31"), (dict(nlat=big), b">= 2^31"), (dict(nlon=big), b">= 2^31"),
           (dict(ldx=big), b">= 2^31"), (dict(ldy=big), b">= 2^31"), (dict(ldp=big), b">= 2^31"), (dict(ldq=big), b">= 2^31"),
           (dict(NLAT=big), b">= 2^31"), (dict(NLON=big), b">= 2^31"),
           (dict(T=big - 1, ldx=big - 1), b"2^60"), (dict(T=big - 1, ldy=big - 1), b"2^60"),
           (dict(nlat=0, ldp=0, ldx=0), b"empty plane"), (dict(nlon=0, ldp=0, ldx=0), b"empty plane"),
           (dict(min_frac=-0.1), b"min_frac"), (dict(min_frac=1.0001), b"min_frac"), (dict(min_frac=float("nan")), b"min_frac"),
           (dict(X=X + 2), b"not aligned"), (dict(Y=Y + 1), b"not aligned"), (dict(iy0=good["iy0"] + 2), b"not aligned"),
           (dict(ny=good["ny"] + 1), b"not aligned"), (dict(jx0=good["jx0"] + 2), b"not aligned"),
           (dict(nx=good["nx"] + 3), b"not aligned"), (dict(wy=good["wy"] + 4), b"not aligned"),
           (dict(wx=good["wx"] + 4), b"not aligned"),
           (dict(Y=X), b"overlap"), (dict(Y=X + 16), b"overlap"), (dict(Y=X - 8), b"overlap"), (dict(Y=X + xbytes - 4), b"overlap"),
           (dict(Y=X - ybytes + 4), b"overlap")]
    for change, text in bad:
        assert H.dmdx_host_remap_check(*{**good, **change}.values()) == E_INVALID, change
        msg = H.dmdx_host_last_error()
        assert msg.startswith(b"remap:") and text in msg, (change, msg)
    # the limits themselves run: the widest spans, min_frac at both ends, exact leading dimensions, Y right behind / before X
    for change in (dict(SY=64), dict(SX=64), dict(SY=1, SX=1), dict(min_frac=0.0), dict(min_frac=1.0), dict(ldx=mx), dict(ldy=my),
                   dict(Y=X + xbytes), dict(Y=X - ybytes), dict(T=big - 1, Y=1 << 62)):
        assert H.dmdx_host_remap_check(*{**good, **change}.values()) == 0, (change, H.dmdx_host_last_error())
        assert H.dmdx_host_last_error() == b""
    # empty calls pass the checks (and overlap nothing), but not with another argument wrong
    for change in (dict(T=0), dict(P=0), dict(NLAT=0), dict(NLON=0), dict(T=0, Y=X), dict(P=0, Y=X), dict(NLAT=0, Y=X),
                   dict(NLON=0, Y=X), dict(NLAT=0, NLON=0, nlat=0, nlon=0, ldp=0, ldq=0)):
        assert H.dmdx_host_remap_check(*{**good, **change}.values()) == 0, (change, H.dmdx_host_last_error())
    assert H.dmdx_host_remap_check(*{**good, "T": 0, "SX": 0}.values()) == E_INVALID
    assert not any(bufs["x"]) and not any(bufs["y"])


def test_the_product_library_refuses_the_same_way_without_a_gpu():
    """dmdx_remap_f32 itself: the same checks before any HIP call, and empty calls return 0 without a launch."""
    so = os.path.join(ROOT, "dmd_era5_amd", "libdmdx.so")
    if not os.path.exists(so):
        import __graft_entry__

        __graft_entry__.build()
    from dmd_era5_amd import _lib

    L = _lib.load()
    assert L.dmdx_remap_max_span() == 64
    good, bufs, xbytes, ybytes, mx, my = _good()
    for change in (dict(X=None), dict(wx=None), dict(SY=65), dict(SX=0), dict(ldp=125), dict(ldq=11), dict(ldx=mx - 1),
                   dict(T=2 ** 31), dict(min_frac=float("nan")), dict(X=good["X"] + 2), dict(wy=good["wy"] + 4), dict(Y=good["X"] + 16),
                   dict(T=2 ** 31 - 1, ldx=2 ** 31 - 1), dict(nlat=0, ldp=0, ldx=0)):
        assert L.dmdx_remap_f32(*{**good, **change}.values(), None) == E_INVALID, change
        assert b"remap" in L.dmdx_last_error(), change
    for change in (dict(T=0), dict(P=0), dict(NLAT=0), dict(NLON=0)):
        assert L.dmdx_remap_f32(*{**good, **change}.values(), None) == 0, (change, L.dmdx_last_error())
    assert not any(bufs["x"]) and not any(bufs["y"])
