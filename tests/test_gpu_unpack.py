"""K14 (dmdx_unpack_i16_f32) through the ctypes table: values bit for bit, memory contract, refusals.

The reference is tests/unpack_ref.py (numpy: fp64 multiply, fp64 add, one rounding to fp32); every
comparison is made on the int32 view, so a different NaN or a float-path shortcut shows.  A fused
multiply-add gives the same fp32 value for all 65 536 codes at the ERA5 packing (SF, AO); the pair
(SF, AO_FMA) is constructed so that it does not (test_two_roundings_not_a_fused_multiply_add).
Outputs live in tests/memguard.py allocations; every source element the call does not address
holds the fill code, so a stray load turns into a NaN and a non-zero fill count.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import memguard as mg
import unpack_ref as ur

pytestmark = pytest.mark.gpu

E_INVALID = -1000
SF, AO = 0.0018501293483403683, 271.93247          # an ERA5 temperature packing
FILL = -32767
# Chosen on the host with exact rationals: fl64(599 * SF) + AO_FMA is a tie in fp64 that rounds (to even) onto the
# midpoint between the fp32 neighbours 272 + 2^-15 and 272 + 2^-14, which in turn rounds to the even one,
# 272 + 2^-14; the exact 599 * SF + AO_FMA lies below the fp64 tie, so a fused multiply-add returns 272 + 2^-15.
# Code 599 is the only one of the 65 536 that differs.
AO_FMA, Q_FMA = 270.8918182967113, 599


@pytest.fixture(scope="module")
def L():
    from dmd_era5_amd.kernels import default_kernels

    return default_kernels()._lib


def _source(host: np.ndarray, base: int):
    """The int16 host array on the device, its first element `base` elements (0..7) past a 16-byte
    boundary.  -> (keep-alive tensor, device address)."""
    buf = torch.empty(host.size + 16, dtype=torch.int16, device="cuda")
    off = (base - buf.data_ptr() // 2) % 8
    buf[off:off + host.size].copy_(torch.from_numpy(host))
    assert (buf.data_ptr() // 2 + off) % 8 == base
    return buf, buf.data_ptr() + 2 * off


def _call(L, sptr, lds, T, tstep, rows, row0, plane, segs, sf, ao, fills, xptr, ldx, counter, nseg=None, nfill=None):
    table = (C.c_int64 * max(len(segs), 1))(*segs)
    f = list(fills) + [0, 0]
    return L.dmdx_unpack_i16_f32(sptr, lds, T, tstep, rows, row0, plane, len(segs) if nseg is None else nseg, table,
                                 sf, ao, len(fills) if nfill is None else nfill, f[0], f[1], xptr, ldx,
                                 None if counter is None else counter.data_ptr(), torch.cuda.current_stream().cuda_stream)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------ every code
def _every_code(L, sf, ao, fills):
    T, rows = 16, 4096
    S = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
    keep, sptr = _source(S, 0)
    _, h = mg.guarded(rows, T, rows, torch.float32)
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    rc = _call(L, sptr, rows, T, 1, rows, 0, rows, [0], sf, ao, fills, h.ptr, rows, cnt)
    assert rc == 0, L.dmdx_last_error()
    torch.cuda.synchronize()
    h.check_fully_written()
    h.check_untouched()
    want, nf = ur.unpack_i16(S, rows, T, 1, rows, 0, rows, [0], sf, ao, fills)
    got = h.logical()
    assert np.array_equal(_bits(got), _bits(want))
    codes = S.reshape(T, rows).T
    assert np.array_equal(np.isnan(got), np.isin(codes, list(fills)))
    return h, cnt, sptr, keep, nf


def test_every_code_bit_equal_and_fill_count(L):
    h, cnt, sptr, keep, nf = _every_code(L, SF, AO, (FILL, 12345))
    assert nf == 2 and int(cnt.item()) == 2
    # the counter accumulates
    assert _call(L, sptr, 4096, 16, 1, 4096, 0, 4096, [0], SF, AO, (FILL, 12345), h.ptr, 4096, cnt) == 0
    torch.cuda.synchronize()
    assert int(cnt.item()) == 4
    assert int(np.isnan(h.logical()).sum()) == 2


def test_every_code_without_fill_codes(L):
    h, cnt, *_ = _every_code(L, SF, AO, ())
    assert int(cnt.item()) == 0
    assert np.isfinite(h.logical()).all()


def test_two_roundings_not_a_fused_multiply_add(L):
    from fractions import Fraction

    fused = np.float32(float(Fraction(Q_FMA) * Fraction(SF) + Fraction(AO_FMA)))      # one rounding to fp64, one to fp32
    two = ur.decode(np.array([Q_FMA]), SF, AO_FMA)[0]
    ulp = np.float32(2.0 ** -15)
    assert two == np.float32(272.0) + 2 * ulp and fused == np.float32(272.0) + ulp          # the pair tells them apart
    h, *_ = _every_code(L, SF, AO_FMA, ())                     # bit-equal to the two-rounding double for every code
    assert h.logical()[(Q_FMA + 32768) % 4096, (Q_FMA + 32768) // 4096] == two


@pytest.mark.parametrize("sf, ao", [(1.0, 0.0), (2.0 ** -10, 0.0)])
def test_every_code_exact_integers_and_dyadics(L, sf, ao):
    h, *_ = _every_code(L, sf, ao, ())
    S = np.arange(-32768, 32768, dtype=np.float64).reshape(16, 4096).T
    assert np.array_equal(h.logical().astype(np.float64), S * sf)      # exact, not only equal to the double


# ------------------------------------------------------------------ shapes and alignment
def _layouts(rows):
    """(ldx, base offset past a 16-byte boundary) of the output."""
    r4 = (rows + 3) // 4 * 4
    return [(rows, 0), (rows + 4, 0), (rows + 1 if rows % 2 == 0 else rows + 2, 0),
            (r4 + 4, 1), (r4 + 4, 2), (rows + 4, 3)]


def _run_case(L, rs, rows, T, tstep, row0, plane, segs, span, lds, sbase, ldx, xoff):
    """One call on a source whose unaddressed elements all hold the fill code."""
    size = (T - 1) * tstep * lds + span
    S = np.full(size, FILL, dtype=np.int16)
    mask = ur.addressed(size, lds, T, tstep, rows, row0, plane, segs)
    q = rs.randint(-32768, 32768, size=int(mask.sum())).astype(np.int16)
    q[q == FILL] = 0
    S[mask] = q
    keep, sptr = _source(S, sbase)
    _, h = mg.guarded(rows, T, ldx, torch.float32, xoff)
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    rc = _call(L, sptr, lds, T, tstep, rows, row0, plane, segs, SF, AO, (FILL,), h.ptr, ldx, cnt)
    what = f"rows={rows} T={T} tstep={tstep} row0={row0} plane={plane} segs={segs} lds={lds} sbase={sbase} ldx={ldx} xoff={xoff}"
    assert rc == 0, (what, L.dmdx_last_error())
    torch.cuda.synchronize()
    h.check_fully_written(what)
    h.check_untouched(what)
    got = h.logical()
    want, nf = ur.unpack_i16(S, lds, T, tstep, rows, row0, plane, segs, SF, AO, (FILL,))
    assert nf == 0
    assert np.isfinite(got).all(), what
    assert np.array_equal(_bits(got), _bits(want)), what
    assert int(cnt.item()) == 0, what
    del keep


@pytest.mark.parametrize("tstep", [1, 3])
@pytest.mark.parametrize("T", [1, 2, 5])
@pytest.mark.parametrize("rows", [1, 3, 7, 8, 9, 31, 33, 255, 257, 1003])
def test_shapes_and_alignment(L, rows, T, tstep):
    """Every row0 x output layout, the source base walking through 0..7 and lds through both
    parities; two segments in swapped order with a gap, the block crossing from one to the other."""
    rs = np.random.RandomState(rows * 100 + T * 10 + tstep)
    i = 0
    for row0 in (0, 1, 5, 8):
        plane = (row0 + rows) // 2 + 1
        segs = [plane + 3, 0]
        span = 2 * plane + 3
        for ldx, xoff in _layouts(rows):
            _run_case(L, rs, rows, T, tstep, row0, plane, segs, span, span + 2 + (i & 1), i % 8, ldx, xoff)
            i += 1
    assert i >= 16


@pytest.mark.parametrize("sbase", range(8))
def test_source_base_with_aligned_output(L, sbase):
    """One segment, so that full chunks take the 8-code load at every source alignment, odd and even lds."""
    rs = np.random.RandomState(sbase)
    for lds in (1003 + 13, 1003 + 14):
        for row0 in (0, 1, 5, 8):
            _run_case(L, rs, 1003 - row0, 2, 1, row0, 1003, [0], 1003, lds, sbase, 1004, 0)


@pytest.mark.parametrize("rows, row0", [(33, 8), (31, 30), (9, 33), (74, 0), (1, 36), (1, 37)])
@pytest.mark.parametrize("tstep", [1, 3])
def test_three_level_source_with_level_selection(L, rows, row0, tstep):
    """plane = 37, three levels in the source, levels [2, 0] selected: the block crosses from level 2 to level 0."""
    rs = np.random.RandomState(rows + row0)
    for i, (ldx, xoff) in enumerate(_layouts(rows)):
        _run_case(L, rs, rows, 5, tstep, row0, 37, [2 * 37, 0], 3 * 37, 3 * 37, i, ldx, xoff)


@pytest.mark.parametrize("rows, row0", [(3 * 4 * 7, 0), (40, 5), (29, 27)])
def test_latitude_band(L, rows, row0):
    """Three levels of an 11 x 7 grid, latitude rows 3..6 of each: the segment table starts inside a plane."""
    nlat, nlon, i0, i1 = 11, 7, 3, 7
    segs = [lv * nlat * nlon + i0 * nlon for lv in range(3)]
    rs = np.random.RandomState(rows)
    for i, (ldx, xoff) in enumerate(_layouts(rows)):
        _run_case(L, rs, rows, 2, 1 + (i & 1), row0, (i1 - i0) * nlon, segs, 3 * nlat * nlon, 3 * nlat * nlon + (i & 1),
                  (3 * i) % 8, ldx, xoff)


# ------------------------------------------------------------------ refusals and empty calls
_GOOD = dict(lds=64, T=3, tstep=1, rows=40, row0=2, plane=64, nseg=1, nfill=1, ldx=44)


@pytest.mark.parametrize("bad", [dict(T=-1), dict(rows=-1), dict(row0=-1), dict(lds=-1), dict(tstep=0), dict(tstep=-2),
                                 dict(nseg=0), dict(nseg=65), dict(nfill=-1), dict(nfill=3), dict(ldx=39)],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_refused_calls_write_nothing(L, bad):
    a = dict(_GOOD, **bad)
    S = np.full(3 * 64, FILL, dtype=np.int16)
    keep, sptr = _source(S, 0)
    _, h = mg.guarded(40, 3, 44, torch.float32)
    cnt = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    rc = _call(L, sptr, a["lds"], a["T"], a["tstep"], a["rows"], a["row0"], a["plane"], [0] * 65, SF, AO, (FILL, 1),
               h.ptr, a["ldx"], cnt, nseg=a["nseg"], nfill=a["nfill"])
    torch.cuda.synchronize()
    assert rc == E_INVALID
    assert L.dmdx_last_error()
    assert bool((h.iview == h.canary).all())
    h.check_untouched()
    assert int(cnt.item()) == 7


@pytest.mark.parametrize("empty", [dict(T=0), dict(rows=0)], ids=["T=0", "rows=0"])
def test_empty_calls_write_nothing(L, empty):
    a = dict(_GOOD, **empty)
    S = np.full(3 * 64, FILL, dtype=np.int16)
    keep, sptr = _source(S, 0)
    _, h = mg.guarded(40, 3, 44, torch.float32)
    cnt = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    rc = _call(L, sptr, a["lds"], a["T"], a["tstep"], a["rows"], a["row0"], a["plane"], [0], SF, AO, (FILL,), h.ptr,
               a["ldx"], cnt)
    torch.cuda.synchronize()
    assert rc == 0, L.dmdx_last_error()
    assert bool((h.iview == h.canary).all())
    h.check_untouched()
    assert int(cnt.item()) == 7


def test_wrapper_checks_the_slab_size(L):
    """HipKernels.unpack_i16_ refuses a call that would read past the codes it was given."""
    from dmd_era5_amd._lib import DmdxError
    from dmd_era5_amd.kernels import default_kernels

    kern = default_kernels()
    codes = torch.zeros(3 * 64 - 1, dtype=torch.int16, device="cuda")
    X = torch.zeros((3, 64), dtype=torch.float32, device="cuda")
    with pytest.raises(DmdxError):
        kern.unpack_i16_(codes, 64, 1, X, 0, 64, [0], 1.0, 0.0)
    codes = torch.arange(3 * 64, dtype=torch.int16, device="cuda")
    kern.unpack_i16_(codes, 64, 1, X, 0, 64, [0], 1.0, 0.0)
    assert torch.equal(X.reshape(-1), codes.to(torch.float32))
