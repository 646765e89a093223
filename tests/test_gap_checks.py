"""The argument checks of K31 (dmdx_gap_mask_f32, dmdx_gap_standardize_f32, dmdx_gap_fill_f32 and their two workspace
queries) through ctypes, without a GPU: they run before HIP is touched.  Every refusal of include/dmdx.h returns
DMDX_E_INVALID (a short workspace DMDX_E_WORKSPACE) and names the entry point in dmdx_last_error()."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_WORKSPACE = -1000, -1001
BIG = 2 ** 31
ONE = 0x10000                   # non-null addresses that are never used: every call below is refused before a launch


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(ROOT, "dmd_era5_amd", "libdmdx.so")):
        import __graft_entry__

        __graft_entry__.build()
    from dmd_era5_amd import _lib

    return _lib.load()


def _caller(fn, good):
    def call(**over):
        a = dict(good)
        a.update(over)
        return fn(*a.values())

    return call


def test_limits_and_version(lib):
    assert (lib.dmdx_gap_mask_segment(), lib.dmdx_gap_fill_max_k(), lib.dmdx_version()) == (1024, 256, 110)


def test_every_refusal_of_the_mask_names_the_entry_point(lib):
    m, T = 1000, 2100
    need = lib.dmdx_gap_mask_workspace_bytes(m, T)
    good = dict(X=ONE, m=m, T=T, ldx=m + 4, W=ONE + 0x1000000, ldw=m + 1, nmiss=ONE + 0x2000000, sums=ONE + 0x3000000,
                ldsum=m + 2, ws=ONE + 0x4000000, wsb=need, stream=None)
    call = _caller(lib.dmdx_gap_mask_f32, good)
    bad = [dict(X=None), dict(W=None), dict(m=-1), dict(T=-1), dict(ldx=m - 1), dict(ldw=m - 1), dict(ldsum=m - 1),
           dict(m=BIG, ldx=BIG, ldw=BIG, ldsum=BIG), dict(T=BIG), dict(ldx=BIG), dict(ldw=BIG), dict(ldsum=BIG),
           dict(m=2 ** 40, ldx=2 ** 40, ldw=2 ** 40, ldsum=2 ** 40), dict(X=ONE + 2), dict(W=ONE + 1), dict(nmiss=ONE + 2),
           dict(sums=ONE + 4), dict(ws=ONE + 4)]
    for over in bad:
        assert call(**over) == E_INVALID, over
        assert b"dmdx_gap_mask_f32" in lib.dmdx_last_error(), over
    for over in (dict(wsb=need - 1), dict(wsb=0)):
        assert call(**over) == E_WORKSPACE, over
        assert b"dmdx_gap_mask_f32" in lib.dmdx_last_error(), over
    # a bad argument is named before the workspace is looked at; ldsum is free without sums
    assert call(ldx=m - 1, wsb=0) == E_INVALID
    # an empty block returns 0 and touches nothing, whatever the pointers are
    assert call(m=0, ldx=0, ldw=0, ldsum=0) == 0 and call(T=0) == 0 and call(m=0, T=0, X=None, W=None) == 0


def test_every_refusal_of_standardize_names_the_entry_point(lib):
    m, T = 500, 70
    good = dict(X=ONE, m=m, T=T, ldx=m, W=ONE + 0x1000000, ldw=m + 3, mu=ONE + 0x2000000, sigma=ONE + 0x3000000, back=0,
                stream=None)
    call = _caller(lib.dmdx_gap_standardize_f32, good)
    for over in (dict(X=None), dict(m=-1), dict(T=-1), dict(ldx=m - 1), dict(ldw=m - 1), dict(m=BIG, ldx=BIG, ldw=BIG),
                 dict(T=BIG), dict(ldx=BIG), dict(ldw=BIG), dict(X=ONE + 1), dict(W=ONE + 2), dict(mu=ONE + 3),
                 dict(sigma=ONE + 1), dict(back=1, ldx=m - 1), dict(back=1, X=None)):
        assert call(**over) == E_INVALID, over
        assert b"dmdx_gap_standardize_f32" in lib.dmdx_last_error(), over
    assert call(m=0, ldx=0, ldw=0) == 0 and call(T=0) == 0


def test_every_refusal_of_the_fill_names_the_entry_point(lib):
    m, k, T = 1000, 7, 100
    need = lib.dmdx_gap_fill_workspace_bytes(m, k, T)
    assert need >= 16 + 8 * m
    good = dict(U=ONE, m=m, k=k, ldu=m + 4, C=ONE + 0x1000000, ldc=k + 1, T=T, mu=ONE + 0x2000000, sigma=ONE + 0x3000000,
                W=ONE + 0x4000000, ldw=m + 2, X=ONE + 0x5000000, ldx=m + 3, change=ONE + 0x6000000, ws=ONE + 0x7000000,
                wsb=need, stream=None)
    call = _caller(lib.dmdx_gap_fill_f32, good)
    bad = [dict(U=None), dict(C=None), dict(W=None), dict(X=None), dict(k=0), dict(k=-1), dict(k=257, ldc=300),
           dict(k=BIG, ldc=BIG), dict(m=-5), dict(T=-1), dict(ldu=m - 1), dict(ldc=k - 1), dict(ldw=m - 1), dict(ldx=m - 1),
           dict(ldx=m // 2), dict(m=BIG, ldu=BIG, ldw=BIG, ldx=BIG), dict(T=BIG), dict(ldu=BIG), dict(ldc=BIG),
           dict(ldw=BIG), dict(ldx=BIG), dict(m=2 ** 40, ldu=2 ** 40, ldw=2 ** 40, ldx=2 ** 40), dict(X=ONE + 2),
           dict(W=ONE + 1), dict(change=ONE + 4), dict(U=ONE + 1), dict(C=ONE + 0x1000002), dict(mu=ONE + 0x2000003),
           dict(sigma=ONE + 0x3000001)]
    for over in bad:
        assert call(**over) == E_INVALID, over
        assert b"dmdx_gap_fill_f32" in lib.dmdx_last_error(), over
    for over in (dict(wsb=need - 1), dict(wsb=0), dict(ws=None)):
        assert call(**over) == E_WORKSPACE, over
        assert b"dmdx_gap_fill_f32" in lib.dmdx_last_error(), over
    assert call(k=0, wsb=0) == E_INVALID
    assert call(m=0, ldu=0, ldw=0, ldx=0) == 0 and call(T=0) == 0


def test_workspace_queries(lib):
    # mask: per segment of 1024 snapshots two doubles and one int32 per row
    for m, T in ((1, 1), (1000, 1024), (1000, 1025), (129780, 8760), (3, 2 ** 31 - 1)):
        assert lib.dmdx_gap_mask_workspace_bytes(m, T) == -(-T // 1024) * m * 20, (m, T)
    assert lib.dmdx_gap_mask_workspace_bytes(0, 5) == 0 and lib.dmdx_gap_mask_workspace_bytes(5, 0) == 0
    assert lib.dmdx_gap_mask_workspace_bytes(-1, 5) == 0 and lib.dmdx_gap_mask_workspace_bytes(BIG, 5) == 0
    # fill: the row partials of every T split behind 16 bytes of alignment; no k in it; degenerate shapes ask for 16
    for m, T in ((1, 1), (300, 100), (129780, 8760)):
        b = lib.dmdx_gap_fill_workspace_bytes(m, 20, T)
        assert b >= 16 + 8 * m and b == lib.dmdx_gap_fill_workspace_bytes(m, 256, T) and (b - 16) % (8 * m) < 16, (m, T, b)
    assert lib.dmdx_gap_fill_workspace_bytes(0, 5, 5) == 16 and lib.dmdx_gap_fill_workspace_bytes(5, 5, -1) == 16
    assert lib.dmdx_gap_fill_workspace_bytes(128, 5, 100) == 16 + 4 * 8 * 128      # 4 tiles, 4 T splits
