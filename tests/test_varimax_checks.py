"""The argument checks of K30 (dmdx_varimax_step_f32, dmdx_row_norms_f32, dmdx_varimax_workspace_bytes) through ctypes,
without a GPU: they run before HIP is touched.  Every refusal of include/dmdx.h returns DMDX_E_INVALID (a short
workspace DMDX_E_WORKSPACE) and names the entry point in dmdx_last_error()."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_WORKSPACE = -1000, -1001


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(ROOT, "dmd_era5_amd", "libdmdx.so")):
        import __graft_entry__

        __graft_entry__.build()
    from dmd_era5_amd import _lib

    return _lib.load()


def test_limits_and_version(lib):
    assert (lib.dmdx_varimax_max_k(), lib.dmdx_version()) == (64, 110)


def test_every_refusal_of_the_step_names_the_entry_point(lib):
    one = 0x10000               # non-null addresses that are never used: every call below is refused before a launch
    m, k = 1000, 7
    good = dict(U=one, m=m, k=k, ldu=m + 4, R=one + 0x100000, ldr=k + 1, w=one + 0x200000, G=one + 0x300000, ldg=k + 2,
                q=one + 0x400000, f=one + 0x500000, accumulate=0, ws=one + 0x600000, wsb=0, stream=None)
    need = lib.dmdx_varimax_workspace_bytes(m, k)
    assert need > 0

    def call(**over):
        a = dict(good)
        a.update(over)
        return lib.dmdx_varimax_step_f32(*a.values())

    big = 2 ** 31
    bad = [dict(U=None), dict(R=None), dict(G=None), dict(q=None), dict(k=0), dict(k=-1), dict(k=65, ldr=70, ldg=70),
           dict(k=big, ldr=big, ldg=big), dict(m=0), dict(m=-5), dict(ldu=m - 1), dict(ldr=k - 1), dict(ldg=k - 1),
           dict(m=big, ldu=big), dict(ldu=big), dict(ldr=big), dict(ldg=big), dict(m=2 ** 40, ldu=2 ** 40)]
    for over in bad:
        assert call(wsb=need, **over) == E_INVALID, over
        assert b"dmdx_varimax_step_f32" in lib.dmdx_last_error(), over
    for over in (dict(wsb=need - 1), dict(wsb=0), dict(ws=None, wsb=need)):
        assert call(**over) == E_WORKSPACE, over
        assert b"dmdx_varimax_step_f32" in lib.dmdx_last_error(), over
    # a bad argument is named before the workspace is looked at
    assert call(k=0, wsb=0) == E_INVALID


def test_every_refusal_of_row_norms_names_the_entry_point(lib):
    one = 0x10000
    good = dict(U=one, m=100, k=5, ldu=100, cscale=None, h=one + 0x100000, stream=None)

    def call(**over):
        a = dict(good)
        a.update(over)
        return lib.dmdx_row_norms_f32(*a.values())

    big = 2 ** 31
    for over in (dict(U=None), dict(h=None), dict(m=0), dict(k=0), dict(m=-1), dict(k=-1), dict(ldu=99), dict(m=big, ldu=big),
                 dict(ldu=big), dict(k=big)):
        assert call(**over) == E_INVALID, over
        assert b"dmdx_row_norms_f32" in lib.dmdx_last_error(), over


def test_workspace_bytes_is_monotone_in_m_and_grows_with_k(lib):
    """A workspace sized for m rows serves every shorter block: the size never steps down, though the number of row
    ranges does whenever the fill rule lengthens them.  Checked over every m up to 2^18 + 2 and around the edges of
    the rule beyond; per row range it is k^2 + 2 k floats."""
    for k in (1, 50, 64):
        ms = list(range(1, 2 ** 18 + 3)) if k == 50 else list(range(1, 5000)) + list(range(2 ** 17 - 300, 2 ** 17 + 300))
        ms += [2 ** 21 - 1, 2 ** 21, 2 ** 21 + 1, 2 ** 21 + 4097, 10 ** 7, 2 ** 31 - 4097, 2 ** 31 - 1]
        last = 0
        for m in ms:
            b = lib.dmdx_varimax_workspace_bytes(m, k)
            assert b >= last and b >= 16 + 4 * (k * k + 2 * k) * -(-m // 4096), (m, k, b, last)
            last = b
    for m in (1, 4097, 10 ** 6):
        sizes = [lib.dmdx_varimax_workspace_bytes(m, k) for k in range(1, 65)]
        assert all(b > a for a, b in zip(sizes, sizes[1:])), m
    # one row range: the slot and the 16 bytes that align it
    assert lib.dmdx_varimax_workspace_bytes(100, 3) == 16 + 16 * -(-4 * 15 // 16)
