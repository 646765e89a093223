"""K32 (dmdx_mk_stats_f32, dmdx_sen_slopes_f32) through the ctypes table: the four integer planes and the selected slopes
equal to tests/mk_ref.py (plain numpy over the pairs; the kernel is never its own reference) in every bit, the memory
contract on operands from tests/memguard.py (canaries in pads and guard zones) and the refusals.

Rows of every case, by i % 10: integers in -3 .. 3 (tie groups >= 3, tied slopes); normals with a trend; a constant
row; an all-NaN row; exactly one and exactly two valid points; +-Inf and NaN as missing values; -0.0 / +0.0 / 1.0
(adjacent signed zeros: a slope of -0.0, whose rank differs from that of +0.0); values near +-3e38; values near 1e-38.
Time axes: regular, irregular, a step of 2^-20 (the slopes of the 3e38 rows overflow to +-Inf in fp32) and a step of 1e6
(the slopes of the 1e-38 rows are denormal).  Every length runs with every axis, every shape with both pads.  That the
inputs hold what can go wrong is asserted on the reference before a kernel runs.
"""
import ctypes

import numpy as np
import pytest
import torch

import memguard as mg
import mk_ref as mr

pytestmark = pytest.mark.gpu

F32 = torch.float32
DEV = "cuda"
E_INVALID = -1000
MS = (1, 3, 65, 1029)
PADS = (0, 7)
N_LIST = (1, 2, 3, 45, 46, 63, 64, 65, 91, 92, 128)
AXES = ("regular", "irregular", "tiny", "huge")
KINDS = 10
CASES = [(m, pad, n, AXES[(mi + 2 * pi + ni) % 4])
         for mi, m in enumerate(MS) for pi, pad in enumerate(PADS) for ni, n in enumerate(N_LIST)]


def test_the_list_covers_every_tier():
    """The body has one LDS slice for every length: its only edge is dmdx_mk_max_n() = 128.  The lengths around 64 put a
    point in the second load of a lane or not; 45 / 46 and 91 / 92 put the pairs on either side of 1024 and 4096."""
    from dmd_era5_amd import _lib

    assert N_LIST[-1] == _lib.load().dmdx_mk_max_n() == 128
    assert {1, 2, 3, 63, 64, 65, 128} <= set(N_LIST)
    for n in N_LIST:                                                # every length with every axis and both pads
        assert {c[3] for c in CASES if c[2] == n} == set(AXES)
        assert {(c[1], c[3]) for c in CASES if c[2] == n} == {(p, a) for p in PADS for a in AXES}
    assert {(c[0], c[1]) for c in CASES} == {(m, p) for m in MS for p in PADS}


@pytest.fixture(scope="module")
def L():
    from dmd_era5_amd.kernels import default_kernels

    lib = default_kernels()._lib
    assert lib.dmdx_mk_max_n() == 128 and lib.dmdx_sen_max_ranks() == 4
    return lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _axis(name, n, seed=0):
    k = np.arange(n, dtype=np.float64)
    if name == "regular":
        return 1940.0 + k
    if name == "irregular":
        return np.cumsum(np.random.RandomState(seed + n).choice([0.25, 1.0, 1.0, 2.0, 7.5, 1.0 / 3.0], size=n))
    return k * (2.0 ** -20 if name == "tiny" else 1e6)


def _rows(m, n, seed=0):
    """-> Y (m, n) fp32, the kinds of the module docstring by i % 10."""
    rs = np.random.RandomState(seed + 131 * m + n)
    Y = np.empty((m, n), dtype=np.float32)
    t = np.arange(n)
    for i in range(m):
        kind = i % KINDS if m > 1 else 0
        if kind == 0:
            y = rs.randint(-3, 4, size=n)
        elif kind == 1:
            y = rs.standard_normal(n) + 0.03 * t
        elif kind == 2:
            y = np.full(n, 2.5)
        elif kind in (3, 4, 5):
            y = np.full(n, np.nan)
            keep = rs.choice(n, size=min(kind - 3, n), replace=False)
            y[keep] = rs.standard_normal(keep.size)
        elif kind == 6:
            y = rs.standard_normal(n) - 0.02 * t
            y[rs.rand(n) < 0.2] = np.inf
            y[rs.rand(n) < 0.2] = -np.inf
            y[rs.rand(n) < 0.1] = np.nan
        elif kind == 7:
            y = rs.choice([-0.0, 0.0, 0.0, 1.0], size=n)
            y[:3] = (0.0, -0.0, 0.0)[:n]
        elif kind == 8:
            y = rs.choice([-1.0, 1.0], size=n) * rs.uniform(2.5e38, 3.3e38, size=n)
        else:
            y = rs.uniform(0.5e-38, 3e-38, size=n) * rs.choice([-1.0, 1.0, 1.0], size=n)
        Y[i] = y.astype(np.float32)
    return Y


def _rank_table(N, seed=0):
    """(4, m) int32: per row 0, N - 1, the median, -1 and N in turn; N // 2; anything in -2 .. N + 1; N - 1."""
    m = N.shape[0]
    rs = np.random.RandomState(seed + m)
    i = np.arange(m)
    turn = np.stack([np.zeros(m, dtype=np.int64), N - 1, (N - 1) // 2, -np.ones(m, dtype=np.int64), N])[i % 5, i]
    free = rs.randint(-2, 10 ** 9, size=m) % (N + 4) - 2
    return np.stack([turn, N // 2, free, N - 1]).astype(np.int32)


_REF = {}


def _ref(m, n, axis):
    """Everything of the reference of a case, computed once: Y, tc, the planes, the sorted keys, N, the rank table."""
    key = (m, n, axis)
    if key not in _REF:
        Y, tc = _rows(m, n), _axis(axis, n)
        keys, N = mr.slope_keys(Y, tc)
        _REF[key] = dict(Y=Y, tc=tc, stats=mr.mk_stats(Y), keys=keys, N=N, rank=_rank_table(N))
    return _REF[key]


def test_inputs_hold_what_can_go_wrong():
    """On the reference alone, at m = 1029 and n = 65."""
    n = 65
    seen = {}
    for axis in AXES:
        r = _ref(1029, n, axis)
        v, S, E, G = (r["stats"][q].astype(np.int64) for q in range(4))
        keys, N = r["keys"], r["N"]
        assert {0, 1, 2, n} <= set(v.tolist()) and ((v > 2) & (v < n)).any()
        assert (G >= 3 * 2 * 11).any() and (E > 0).any() and (S < 0).any() and (S > 0).any()
        assert ((v == n) & (E == n * (n - 1) // 2) & (S == 0)).any()                   # the constant row
        tied = minus0 = both0 = inf = den = 0
        for i in range(1029):
            k = keys[i, :N[i]].astype(np.uint32)
            bits = mr.bits_of(k)
            tied += bool((k[1:] == k[:-1]).any())
            m0, p0 = (bits == 0x80000000).any(), (bits == 0).any()
            minus0 += bool(m0)
            both0 += bool(m0 and p0)
            inf += bool(((bits & 0x7FFFFFFF) == 0x7F800000).any())
            den += bool((((bits & 0x7F800000) == 0) & ((bits & 0x007FFFFF) != 0)).any())
            assert not ((bits & 0x7FFFFFFF) > 0x7F800000).any()                       # no slope is a NaN
        seen[axis] = (tied, minus0, both0, inf, den)
        assert tied >= 100 and minus0 >= 50 and both0 >= 50, (axis, seen[axis])
        rank = r["rank"].astype(np.int64)
        assert (rank[0] == -1).any() and (rank[0] == N).any() and (rank[2] > N).any() and (rank[2] < -1).any()
        assert len(set(rank[2].tolist())) > 100
    assert seen["tiny"][3] >= 50 and seen["huge"][4] >= 50, seen


def _guarded_int(values, ld, base):
    """A (rows, m) int32 table in a guarded allocation (the canary pattern of the fp32 kind) -> handle."""
    rows, m = values.shape
    _, h = mg.guarded(m, rows, ld, F32, base_offset_elems=base, device=DEV)
    h.iview.copy_(torch.from_numpy(values.astype(np.int32)).to(DEV))
    return h.snapshot()


@pytest.mark.parametrize("m,pad,n,axis", CASES)
def test_planes_and_slopes_are_the_reference_bit_for_bit(L, m, pad, n, axis):
    r = _ref(m, n, axis)
    base = 1 if pad else 0                                          # with a pad: nothing is 16-byte aligned either
    ld = m + pad
    _, y = mg.guarded(m, n, ld, F32, base_offset_elems=base, device=DEV)
    y.fill(r["Y"]).snapshot()
    tc = (ctypes.c_double * n)(*r["tc"].tolist())

    _, q = mg.guarded(m, 4, ld + 1, F32, base_offset_elems=base, device=DEV)
    assert L.dmdx_mk_stats_f32(y.ptr, m, n, ld, q.ptr, ld + 1, _stream()) == 0, L.dmdx_last_error()
    torch.cuda.synchronize()
    got = q.iview.cpu().numpy()
    assert np.array_equal(got, r["stats"]), np.argwhere(got != r["stats"])[:5]
    mg.assert_untouched(q, "mk_stats out")
    mg.assert_unchanged(y, "Y")
    mg.assert_untouched(y, "Y")

    for J in (1, 2, 3, 4):
        rk = _guarded_int(r["rank"][:J], ld + 2, base)
        _, o = mg.guarded(m, J, ld + 3, F32, base_offset_elems=base, device=DEV)
        rc = L.dmdx_sen_slopes_f32(y.ptr, m, n, ld, tc, rk.ptr, ld + 2, J, o.ptr, ld + 3, _stream())
        assert rc == 0, L.dmdx_last_error()
        torch.cuda.synchronize()
        want = mr.select(r["keys"], r["N"], r["rank"][:J])
        got = o.iview.cpu().numpy().view(np.uint32)
        assert np.array_equal(got, want), (J, np.argwhere(got != want)[:5])
        mg.assert_untouched(o, "sen_slopes out")
        mg.assert_unchanged(rk, "rank")
        mg.assert_untouched(rk, "rank")
    mg.assert_unchanged(y, "Y")
    mg.assert_untouched(y, "Y")


def test_refusals_on_the_device_write_nothing(L):
    m, n, ld = 65, 30, 70
    r = _ref(m, n, "regular")
    _, y = mg.guarded(m, n, ld, F32, device=DEV)
    y.fill(r["Y"]).snapshot()
    rk = _guarded_int(r["rank"], ld, 0)
    _, q = mg.guarded(m, 4, ld, F32, device=DEV)
    _, o = mg.guarded(m, 4, ld, F32, device=DEV)
    tc = (ctypes.c_double * n)(*r["tc"].tolist())
    bad_tc = (ctypes.c_double * n)(*([0.0, 0.0] + list(range(2, n))))
    st = _stream()
    calls = [L.dmdx_mk_stats_f32(y.ptr, m, 129, ld, q.ptr, ld, st), L.dmdx_mk_stats_f32(y.ptr, m, n, m - 1, q.ptr, ld, st),
             L.dmdx_mk_stats_f32(y.ptr, m, n, ld, q.ptr, m - 1, st), L.dmdx_mk_stats_f32(y.ptr, m, n, ld, q.ptr + 2, ld, st),
             L.dmdx_mk_stats_f32(y.ptr, m, n, ld, y.col_ptr(3), ld, st),
             L.dmdx_sen_slopes_f32(y.ptr, m, n, ld, tc, rk.ptr, ld, 5, o.ptr, ld, st),
             L.dmdx_sen_slopes_f32(y.ptr, m, n, ld, bad_tc, rk.ptr, ld, 4, o.ptr, ld, st),
             L.dmdx_sen_slopes_f32(y.ptr, m, n, ld, tc, rk.ptr, m - 1, 4, o.ptr, ld, st),
             L.dmdx_sen_slopes_f32(y.ptr, m, n, ld, tc, rk.ptr, ld, 4, rk.col_ptr(1), ld, st),
             L.dmdx_sen_slopes_f32(y.ptr, m, n, ld, tc, rk.ptr, ld, 4, y.col_ptr(n - 1), ld, st),
             L.dmdx_sen_slopes_f32(y.ptr, m, n, ld, None, rk.ptr, ld, 4, o.ptr, ld, st)]
    torch.cuda.synchronize()
    assert calls == [E_INVALID] * len(calls)
    for h, name in ((q, "mk_stats out"), (o, "sen_slopes out"), (y, "Y"), (rk, "rank")):
        mg.assert_untouched(h, name)
    assert bool((q.iview == q.canary).all()) and bool((o.iview == o.canary).all())
    mg.assert_unchanged(y, "Y")
    mg.assert_unchanged(rk, "rank")


def test_the_wrappers_against_the_double():
    """HipKernels.mk_stats / sen_slopes at n = 85, m = 1000 with a row-strided Y view and ``out=`` views."""
    from dmd_era5_amd import _lib
    from dmd_era5_amd.kernels import default_kernels

    kern = default_kernels()
    assert kern.mk_max_n == 128 and kern.sen_max_ranks == 4
    m, n = 1000, 85
    r = _ref(m, n, "irregular")
    wide = torch.full((n, m + 24), float("nan"), dtype=F32, device=DEV)
    Yt = wide[:, 5:5 + m]
    Yt.copy_(torch.from_numpy(np.ascontiguousarray(r["Y"].T)))
    ranks = torch.from_numpy(r["rank"]).to(DEV)
    double = mr.MkDouble()
    Yc = torch.from_numpy(np.ascontiguousarray(r["Y"].T))
    Q = kern.mk_stats(Yt)
    assert Q.dtype == torch.int32 and torch.equal(Q.cpu(), double.mk_stats(Yc))
    E = kern.sen_slopes(Yt, r["tc"], ranks)
    want = double.sen_slopes(Yc, r["tc"], torch.from_numpy(r["rank"])).view(torch.int32)
    assert E.dtype == F32 and torch.equal(E.cpu().view(torch.int32), want)
    qbuf = torch.full((4, m + 9), -7, dtype=torch.int32, device=DEV)
    ebuf = torch.full((4, m + 9), -7.0, dtype=F32, device=DEV)
    assert kern.mk_stats(Yt, out=qbuf[:, 3:3 + m]).data_ptr() == qbuf[:, 3:3 + m].data_ptr()
    kern.sen_slopes(Yt, r["tc"], ranks[:3], out=ebuf[:3, 2:2 + m])
    assert torch.equal(qbuf[:, 3:3 + m], Q) and bool((qbuf[:, :3] == -7).all()) and bool((qbuf[:, 3 + m:] == -7).all())
    assert torch.equal(ebuf[:3, 2:2 + m].view(torch.int32), E[:3].view(torch.int32))
    assert bool((ebuf[3] == -7).all()) and bool((ebuf[:, :2] == -7).all()) and bool((ebuf[:, 2 + m:] == -7).all())
    for call in (lambda: kern.mk_stats(torch.zeros((129, 4), dtype=F32, device=DEV)),
                 lambda: kern.mk_stats(Yt.double()),
                 lambda: kern.sen_slopes(Yt, r["tc"][:-1], ranks),
                 lambda: kern.sen_slopes(Yt, r["tc"][::-1].copy(), ranks),
                 lambda: kern.sen_slopes(Yt, r["tc"], ranks.to(torch.int64)),
                 lambda: kern.sen_slopes(Yt, r["tc"], ranks[:, :-1]),
                 lambda: kern.sen_slopes(Yt, r["tc"], torch.cat([ranks, ranks[:1]])),
                 lambda: kern.sen_slopes(Yt, r["tc"], ranks, out=ebuf[:3, :m])):
        with pytest.raises(_lib.DmdxError):
            call()
