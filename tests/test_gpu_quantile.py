"""K25 (dmdx_clim_quantile_f32) through the ctypes table: values bit for bit against tests/quant_ref.py (the host
definition; the kernel is never its own reference), the staged and the streamed body against each other, the memory
contract on operands from tests/memguard.py (NaN canaries in pads and guard zones) and every refusal.

Comparisons are made on the integer view, as in test_gpu_clim.py: where the reference holds a NaN that arithmetic
made (Inf - Inf in the interpolation) the kernel must hold a NaN, the NaN the contract names (an empty slot, a NaN
member) is compared as the bit pattern 0x7FC00000, and everywhere else the bits must be equal.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import clim_ref as cr
import memguard as mg
import quant_ref as qr

pytestmark = pytest.mark.gpu

F32 = torch.float32
DEV = "cuda"
E_INVALID = -1000
QNAN = 0x7FC00000
T0, S0 = 37, 6
Q4 = (0.0, 0.1, 0.5, 1.0)                # g == 0 and g != 0 occur for every n_s > 1
OFFSETS = [(0, 0), (1, 2), (2, 3), (3, 1)]                       # (X, out) base offsets in floats past a 16-byte boundary
SHAPES = [(m, pad) for m in (1, 3, 1029, 2053) for pad in (0, 7)]
METHODS = ("linear", "lower", "higher")


@pytest.fixture(scope="module")
def L():
    from dmd_era5_amd.kernels import default_kernels

    return default_kernels()._lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what=""):
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ok = (_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want) & (_bits(want) != QNAN))
    assert ok.all(), f"{what}: {int((~ok).sum())} of {ok.size} elements differ, first at {tuple(np.argwhere(~ok)[0])}"


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _lists():
    """T = 37, S = 6, the lists of test_gpu_clim.py and one more: slot 0 is empty; slot 1 has one snapshot; slot 2 has
    19, out of order, with an entry = T and an entry = -3 among them (skipped, not counted); slot 3 has 4, one of them
    (7) also in slot 2; slot 4 lists 6 entries, snapshot 31 twice and snapshot 2 three times; slot 5 has 8 and its end
    offset lies past n_order (clamped)."""
    s2 = [7, 0, 30, 12, T0, 3, 22, 9, 35, 1, 18, -3, 27, 4, 14, 33, 6, 20, 11, 25, 16]
    s3 = [34, 7, 2, 29]
    s4 = [31, 2, 31, 2, 26, 2]
    s5 = [8, 10, 13, 15, 17, 19, 21, 23]
    order = np.array([5] + s2 + s3 + s4 + s5, dtype=np.int32)
    ends = np.cumsum([0, 0, 1, len(s2), len(s3), len(s4)])
    start = np.array(list(ends) + [order.shape[0] + 9], dtype=np.int32)
    assert cr.counts(order, start, T0).tolist() == [0, 1, 19, 4, 6, 8]
    return order, start


ORDER, START = _lists()


def _data(m, T=T0, seed=0):
    rs = np.random.RandomState(seed + m)
    return (250.0 + 30.0 * rs.standard_normal((m, T))).astype(np.float32)


def _out(m, J, S, pad=0, off=0):
    """The (J, S, m) result as the C ABI sees it: J S columns of m floats, ld = m + pad."""
    return mg.Guarded(m, J * S, m + pad, F32, off, DEV)


def _table(g, J):
    return g.logical().T.reshape(J, g.cols // J, g.rows)


def _call(L, gX, d_order, d_start, q, method, streamed, gO, /, **over):
    """One call with the operands as they are; ``over`` replaces arguments of the C signature by name."""
    qa = (C.c_double * len(q))(*q)
    a = dict(X=gX.ptr, m=gX.rows, T=gX.cols, ldx=gX.ld, order=d_order.data_ptr(), n_order=d_order.numel(),
             start=d_start.data_ptr(), S=d_start.numel() - 1, q=qa, J=len(q), method=qr.METHODS[method],
             streamed=int(streamed), out=gO.ptr, ldo=gO.ld)
    a.update(over)
    return L.dmdx_clim_quantile_f32(*a.values(), _stream())


def _run(L, X, order, start, q, method="linear", streamed=False):
    m, T = X.shape
    S = len(start) - 1
    gX = mg.Guarded(m, T, m, F32, 0, DEV).fill(X)
    gO = _out(m, len(q), S)
    assert _call(L, gX, _i32(order), _i32(start), q, method, streamed, gO) == 0, L.dmdx_last_error()
    gO.check_fully_written("out")
    gO.check_untouched("out")
    return _table(gO, len(q))


def _both(L, X, order, start, q, method="linear"):
    """Staged and streamed: equal bits; -> the table."""
    a, b = _run(L, X, order, start, q, method, False), _run(L, X, order, start, q, method, True)
    assert np.array_equal(_bits(a), _bits(b)), f"the staged and the streamed body differ ({method})"
    return a


# ---------------------------------------------------------------- every layout, method and route
@pytest.mark.parametrize("m,pad", SHAPES)
def test_bit_equal_on_every_layout_method_and_route(L, m, pad):
    X = _data(m)
    order, start = _i32(ORDER), _i32(START)
    want = {(q, meth): qr.quantile(X, ORDER, START, q, meth) for q in (Q4, (0.1,)) for meth in METHODS}
    first = {}
    for ox, oo in OFFSETS:
        gX = mg.Guarded(m, T0, m + pad, F32, ox, DEV).fill(X).snapshot()
        for (q, meth), ref in want.items():
            for streamed in (0, 1):
                gO = _out(m, len(q), S0, pad, oo)
                assert _call(L, gX, order, start, q, meth, streamed, gO) == 0, L.dmdx_last_error()
                got = _table(gO, len(q))
                gO.check_fully_written("out")
                gO.check_untouched("out")
                _same(got, ref, f"q {q} {meth} streamed {streamed} offsets {(ox, oo)}")
                assert (_bits(got[:, 0]) == QNAN).all()          # the empty slot
                assert np.array_equal(_bits(got[:, 1]), _bits(np.broadcast_to(X[:, 5], got[:, 1].shape)))   # a slot of one
                base = first.setdefault((q, meth), got)
                assert np.array_equal(_bits(got), _bits(base))   # both routes, every alignment: the same bits
        gX.check_untouched("X")
        gX.check_unchanged("X")


def test_more_slots_than_grid_rows(L):
    """S = 70 000 > 65 535: grid.y is strided; m = 8, T = 4, slots of one or two snapshots."""
    S, m, T = 70000, 8, 4
    X = _data(m, T, seed=3)
    cnt = 1 + (np.arange(S) % 3 == 0)
    start = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    order = np.empty(start[-1], dtype=np.int32)
    order[start[:-1]] = np.arange(S) % 4
    two = np.nonzero(cnt == 2)[0]
    order[start[two] + 1] = (two + 1) % 4
    got = _run(L, X, order, start, (0.0, 1.0))
    a = X.T[order[start[:-1]]]
    b = a.copy()
    b[two] = X.T[order[start[two] + 1]]
    want = np.stack([np.minimum(a, b), np.maximum(a, b)])
    for s in (0, 1, 2, 3, 65534, 65535, 65536, 69999):           # ... which is quant_ref's answer, slot by slot
        ts = np.array(cr.slot_lists(order, start, s, T), dtype=np.int32)
        assert np.array_equal(_bits(qr.quantile(X, ts, [0, len(ts)], (0.0, 1.0))[:, 0]), _bits(want[:, s]))
    assert np.array_equal(_bits(got), _bits(want))


# ---------------------------------------------------------------- the capacity edges of the staged body
def test_capacity_edges_mix_the_routes_in_one_launch(L):
    """With C = max_staged / 4 (include/dmdx.h): lists of up to C, 2 C, 4 C entries stage 64, 32, 16 rows at a time,
    longer ones are streamed.  One call holds a slot at and just above every edge; m = 67 leaves a ragged tile."""
    cap = L.dmdx_clim_quantile_max_staged()
    assert cap % 4 == 0
    sizes = [cap // 4, cap // 4 + 1, cap // 2, cap // 2 + 1, cap, cap + 1]
    T, m = cap + 1, 67
    rs = np.random.RandomState(17)
    X = np.round(250.0 + 30.0 * rs.standard_normal((m, T)), 1).astype(np.float32)       # some ties
    lists = [rs.permutation(T)[:n] for n in sizes]
    lists[2][5], lists[4][9] = T, -1                             # a skipped entry inside the 32- and the 16-row tier
    order = np.concatenate(lists).astype(np.int32)
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    counted = cr.counts(order, start, T).tolist()
    assert counted == [sizes[0], sizes[1], sizes[2] - 1, sizes[3], sizes[4] - 1, sizes[5]]
    for meth in ("linear", "higher"):
        want = qr.quantile(X, order, start, Q4, meth)
        got = _both(L, X, order, start, Q4, meth)
        _same(got, want, f"capacity edges, {meth}")
    _same(_both(L, X, order, start, (0.9,)), qr.quantile(X, order, start, (0.9,)), "capacity edges, J = 1")


# ---------------------------------------------------------------- values
def test_values_ties_zeros_infinities_denormals_nan_and_scaling(L):
    m = 37
    rs = np.random.RandomState(2)
    X = _data(m, seed=11)
    base = _both(L, X, ORDER, START, Q4)
    _same(base, qr.quantile(X, ORDER, START, Q4), "base")
    # integer-rounded data: heavy ties; all members equal
    Xi = np.round(2.0 * rs.standard_normal((m, T0))).astype(np.float32)
    for meth in METHODS:
        _same(_both(L, Xi, ORDER, START, Q4, meth), qr.quantile(Xi, ORDER, START, Q4, meth), f"ties {meth}")
    Xe = np.broadcast_to(rs.standard_normal((m, 1)).astype(np.float32), (m, T0)).copy()
    got = _both(L, Xe, ORDER, START, Q4)
    _same(got, qr.quantile(Xe, ORDER, START, Q4), "all equal")
    assert np.array_equal(_bits(got[:, 1:]), _bits(np.broadcast_to(Xe[:, 0], got[:, 1:].shape)))
    # +-0 mixed: the order tells them apart, the result carries the sign of the member
    Xz = np.where(rs.rand(m, T0) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    Xz[::3] = np.where(rs.rand(*Xz[::3].shape) < 0.2, rs.standard_normal(Xz[::3].shape), Xz[::3]).astype(np.float32)
    for meth in METHODS:
        got = _both(L, Xz, ORDER, START, Q4, meth)
        _same(got, qr.quantile(Xz, ORDER, START, Q4, meth), f"+-0 {meth}")
    assert (_bits(got) == 0x80000000).any() and (_bits(got) == 0).any()
    # +-Inf members are ordinary values (Inf - Inf in the interpolation: a NaN without contractual bits)
    Xf = X.copy()
    Xf[rs.rand(m, T0) < 0.15] = np.inf
    Xf[rs.rand(m, T0) < 0.15] = -np.inf
    for meth in METHODS:
        got = _both(L, Xf, ORDER, START, Q4, meth)
        _same(got, qr.quantile(Xf, ORDER, START, Q4, meth), f"+-Inf {meth}")
    assert np.isinf(got).any()
    # denormals, of both signs: nothing is flushed
    Xd = rs.randint(-40, 41, (m, T0)).astype(np.int32)
    Xd = np.where(Xd < 0, (-Xd).astype(np.uint32) | np.uint32(0x80000000), Xd.astype(np.uint32)).astype(np.uint32).view(np.float32)
    for meth in METHODS:
        got = _both(L, Xd, ORDER, START, Q4, meth)
        _same(got, qr.quantile(Xd, ORDER, START, Q4, meth), f"denormals {meth}")
    assert ((_bits(got[:, 2:]) & 0x7FFFFFFF) != 0).any()
    # one NaN member, at (3, 7) -- snapshot 7 is listed by slots 2 and 3: row 3 of those two slots is the quiet NaN for
    # every j, nothing else changes; a NaN in a snapshot no slot lists (36) changes nothing
    Xn = X.copy()
    Xn[3, 7], Xn[9, 36] = np.nan, np.nan
    got = _both(L, Xn, ORDER, START, Q4)
    hit = np.zeros(base.shape, dtype=bool)
    hit[:, 2, 3] = hit[:, 3, 3] = True
    assert (_bits(got)[hit] == QNAN).all()
    assert np.array_equal(_bits(got)[~hit], _bits(base)[~hit])
    _same(got, qr.quantile(Xn, ORDER, START, Q4), "NaN member")
    # 2^e X gives 2^e out, bit for bit
    for e in (-20, 20):
        f = np.float32(2.0 ** e)
        for meth in METHODS:
            ref = _both(L, X, ORDER, START, Q4, meth)
            _same(_both(L, (X * f).astype(np.float32), ORDER, START, Q4, meth), ref * f, f"2^{e} {meth}")


# ---------------------------------------------------------------- refusals and empty shapes
def test_refusals_write_nothing_and_zero_sizes(L):
    m = 12
    X = _data(m)
    gX = mg.Guarded(m, T0, m + 2, F32, 0, DEV).fill(X).snapshot()
    order, start = _i32(ORDER), _i32(START)
    gO = _out(m, 4, S0, 2)
    big = 2**31
    bad = [dict(X=None), dict(order=None), dict(start=None), dict(q=None), dict(out=None), dict(S=0), dict(S=-1),
           dict(J=0), dict(J=5), dict(method=-1), dict(method=3), dict(ldx=m - 1), dict(ldo=m - 1), dict(m=-1), dict(T=-1),
           dict(n_order=-1), dict(m=big, ldx=big, ldo=big), dict(T=big), dict(n_order=big), dict(S=big), dict(ldx=big),
           dict(ldo=big)]
    for qbad in ((0.5, np.nan, 0.5, 0.5), (-1e-9, 0.5, 0.5, 0.5), (0.5, 0.5, 0.5, 1.0 + 1e-9), (0.5, np.inf, 0.5, 0.5)):
        bad.append(dict(q=(C.c_double * 4)(*qbad)))
    for change in bad:
        assert _call(L, gX, order, start, Q4, "linear", 0, gO, **change) == E_INVALID, change
        assert L.dmdx_last_error()
    assert _call(L, gX, order, start, Q4, "linear", 0, gO, m=0) == 0            # m == 0: the checks, then nothing
    torch.cuda.synchronize()
    assert bool((gO.ibuf == gO.canary).all())
    gX.check_untouched("X")
    gX.check_unchanged("X")
    for streamed in (0, 1):                                      # T == 0 with m > 0: J S m quiet NaN
        gN = _out(m, 4, S0, 2)
        assert _call(L, gX, order, start, Q4, "linear", streamed, gN, T=0) == 0, L.dmdx_last_error()
        gN.check_untouched("T = 0")
        assert (_bits(gN.logical()) == QNAN).all()


# ---------------------------------------------------------------- the wrapper
def test_hip_kernels_clim_quantile(L):
    from dmd_era5_amd import _lib
    from dmd_era5_amd.kernels import default_kernels

    kern = default_kernels()
    assert kern.clim_quantile_max_q == 4 and kern.clim_quantile_max_staged == L.dmdx_clim_quantile_max_staged()
    m = 50
    X = _data(m, seed=41)
    buf = torch.zeros((T0, m + 6), dtype=F32, device=DEV)
    Xt = buf[:, 1:1 + m]                                         # a strided view, one float past the alignment
    Xt.copy_(torch.from_numpy(np.ascontiguousarray(X.T)))
    order, start = _i32(ORDER), _i32(START)
    for meth in METHODS:
        ref = qr.quantile(X, ORDER, START, Q4, meth)
        Q = kern.clim_quantile(Xt, order, start, Q4, method=meth)
        assert Q.shape == (4, S0, m) and Q.dtype == F32 and Q.is_contiguous()
        _same(Q.cpu().numpy(), ref, f"clim_quantile {meth}")
        _same(kern.clim_quantile(Xt, order, start, Q4, method=meth, streamed=True).cpu().numpy(), ref, f"streamed {meth}")
    ref = qr.quantile(X, ORDER, START, (0.1, 0.9))
    _same(kern.clim_quantile(Xt, order, start, 0.9).cpu().numpy(), ref[1:], "a scalar q")
    wide = torch.full((2, S0, m + 3), 9.0, dtype=F32, device=DEV)
    res = kern.clim_quantile(Xt, order, start, (0.1, 0.9), out=wide[:, :, :m])
    assert res.data_ptr() == wide.data_ptr()
    _same(wide[:, :, :m].cpu().numpy(), ref, "out=")
    assert bool((wide[:, :, m:] == 9.0).all()) and bool((buf[:, 0] == 0).all()) and bool((buf[:, 1 + m:] == 0).all())
    for bad in (lambda: kern.clim_quantile(Xt, order.long(), start, Q4), lambda: kern.clim_quantile(Xt.double(), order, start, Q4),
                lambda: kern.clim_quantile(Xt.cpu(), order, start, Q4), lambda: kern.clim_quantile(Xt, order, start, Q4 + (0.7,)),
                lambda: kern.clim_quantile(Xt, order, start, (0.5, 1.5)), lambda: kern.clim_quantile(Xt, order, start, ()),
                lambda: kern.clim_quantile(Xt, order, start, Q4, method="nearest"),
                lambda: kern.clim_quantile(Xt, order, start, Q4, out=wide[:, :, :m]),
                lambda: kern.clim_quantile(Xt, order, start, (0.1, 0.9), out=wide[:, 1:, :m]),
                lambda: kern.clim_quantile(Xt, order, start, (0.1, 0.9), out=wide[:, :, :m].double())):
        with pytest.raises(_lib.DmdxError):
            bad()
