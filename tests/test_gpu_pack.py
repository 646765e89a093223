"""K17 on the GPU: dmdx_expand_range_f32 / dmdx_expand_pack_i16 / dmdx_range_f32 / dmdx_pack_f32_i16 through the
ctypes table, the HipKernels wrappers and era5_svd.write_forecast_slice.

The field the two expand entry points form is K12's bit for bit, so every comparison is an equality: the range is
the min / max of what dmdx_expand_f32 stores for the same operands, the codes are tests/pack_ref.encode of it.
Operands live in NaN-canary guard zones and exact 0xFF workspaces (tests/memguard.py); the int16 codes, which
memguard has no type for, in a canary-filled buffer of this file.
"""
import itertools

import numpy as np
import pytest
import torch

import memguard as mg
import pack_ref as pr

pytestmark = pytest.mark.gpu

F32 = torch.float32
DEV = "cuda"
E_INVALID, E_WORKSPACE = -1000, -1001
SENTINEL = -0x0123456789ABCDEF

MS = [1, 31, 33, 127, 129, 300]
TS = [1, 15, 33, 70]
KS = [1, 16, 17, 50, 192, 193, 256]
LAYOUTS = [0, 1, 2, 3]
RANGES = [(220.0, 300.0), (-40.0, 55.0), (0.0, 1.0), (48000.0, 58000.0), (-3.5, 1e-3)]


@pytest.fixture(scope="module")
def L():
    from dmd_era5_amd.kernels import default_kernels

    return default_kernels()._lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ld(n, layout):
    """layout 0: tight; 1 and 3: an even leading dimension with a pad; 2: an odd one."""
    if layout == 0:
        return n
    if layout == 2:
        return n + (3 if n % 2 == 0 else 2)
    return n + (4 if n % 2 == 0 else 3)


class Codes:
    """m x T int16 codes with snapshot stride ld, `offset` elements past a 16-byte boundary, inside canaries."""

    CANARY = 0x5A5B
    FRONT = 4096

    def __init__(self, m, T, ld, offset):
        self.m, self.T, self.ld = m, T, ld
        total = self.FRONT + 8 + offset + T * ld + 64 * ld + 4096
        self.buf = torch.full((total,), self.CANARY, dtype=torch.int16, device=DEV)
        mis = (self.buf.data_ptr() // 2 + self.FRONT) % 8
        self.start = self.FRONT + (8 - mis) % 8 + offset
        self.view = self.buf.as_strided((T, m), (ld, 1), self.start)

    @property
    def ptr(self):
        return self.buf.data_ptr() + 2 * self.start

    def logical(self):
        """(m, T) host array."""
        return self.view.cpu().numpy().T.copy()

    def check_untouched(self):
        keep = torch.ones_like(self.buf, dtype=torch.bool)
        keep.as_strided((self.T, self.m), (self.ld, 1), self.start).fill_(False)
        assert bool((self.buf[keep] == self.CANARY).all()), "codes: an element outside the logical m x T was written"

    def check_unwritten(self):
        assert bool((self.buf == self.CANARY).all())


def _cnt(n):
    """n device uint64 counters between two sentinels."""
    return torch.tensor([SENTINEL] + [0] * n + [SENTINEL], dtype=torch.int64, device=DEV)


def _cnt_ptr(c):
    return c.data_ptr() + 8


def _cnt_vals(c):
    v = c.cpu().tolist()
    assert v[0] == SENTINEL and v[-1] == SENTINEL
    return v[1:-1]


class Case:
    """Guarded operands of one (U, C, mu, sigma).  layout 2: odd leading dimensions, U one and C two elements past
    a 16-byte boundary, Q one or three; layout 3: layout 1 without mu / sigma."""

    def __init__(self, m, k, T, layout, U, Cm, mu=None, sigma=None):
        self.m, self.k, self.T, self.layout = m, k, T, layout
        self.U, self.C, self.mu, self.sigma = U, Cm, mu, sigma
        odd = layout == 2
        vec = (lambda v, j: None if v is None else mg.Guarded(m, 1, m, F32, j if odd else 0, DEV).fill(v).snapshot())
        self.gU = mg.Guarded(m, k, _ld(m, layout), F32, 1 if odd else 0, DEV).fill(U).snapshot()
        self.gC = mg.Guarded(k, T, _ld(k, layout), F32, 2 if odd else 0, DEV).fill(Cm).snapshot()
        self.gmu, self.gsg = vec(mu, 3), vec(sigma, 1)
        self.grange = mg.Guarded(2, 1, 2, F32, 1 if odd else 0, DEV)
        self.count = _cnt(1)
        self.counts = _cnt(2)
        self.Q = Codes(m, T, _ld(m, layout), (1 + 2 * (m % 2)) if odd else 0)

    def check_inputs(self):
        for g in (self.gU, self.gC, self.gmu, self.gsg):
            if g is not None:
                g.check_untouched("input")
                g.check_unchanged("input")

    def _common(self):
        p = (lambda g: None if g is None else g.ptr)
        return dict(U=self.gU.ptr, m=self.m, k=self.k, ldu=self.gU.ld, C=self.gC.ptr, ldc=self.gC.ld, T=self.T,
                    mu=p(self.gmu), sigma=p(self.gsg))

    def expand(self, L):
        """What dmdx_expand_f32 stores: (m, T) float32."""
        g = mg.Guarded(self.m, self.T, self.m, F32, 0, DEV)
        a = self._common()
        rc = L.dmdx_expand_f32(a["U"], a["m"], a["k"], a["ldu"], a["C"], a["ldc"], a["T"], a["mu"], a["sigma"], g.ptr, g.ld,
                               _stream())
        torch.cuda.synchronize()
        assert rc == 0, L.dmdx_last_error()
        return g.logical()

    def run_range(self, L, accumulate=0, ws=None, **over):
        need = L.dmdx_expand_range_workspace_bytes(self.m, self.k, self.T)
        assert need > 0
        self.ws = mg.exact_workspace(need, DEV) if ws is None else ws
        a = dict(self._common(), range=self.grange.ptr, count=_cnt_ptr(self.count), wsp=self.ws.ptr, wsb=self.ws.nbytes)
        a.update(over)
        rc = L.dmdx_expand_range_f32(a["U"], a["m"], a["k"], a["ldu"], a["C"], a["ldc"], a["T"], a["mu"], a["sigma"],
                                     a["range"], a["count"], accumulate, a["wsp"], a["wsb"], _stream())
        torch.cuda.synchronize()
        return rc

    def range(self):
        """-> (min, max as float32, count)"""
        self.grange.check_untouched("range")
        r = self.grange.logical()[:, 0]
        return r[0], r[1], _cnt_vals(self.count)[0]

    def run_pack(self, L, sf, ao, counts=True, **over):
        a = dict(self._common(), sf=sf, ao=ao, Q=self.Q.ptr, ldq=self.Q.ld, counts=_cnt_ptr(self.counts) if counts else None)
        a.update(over)
        rc = L.dmdx_expand_pack_i16(a["U"], a["m"], a["k"], a["ldu"], a["C"], a["ldc"], a["T"], a["mu"], a["sigma"], a["sf"],
                                    a["ao"], a["Q"], a["ldq"], a["counts"], _stream())
        torch.cuda.synchronize()
        return rc


def rand_case(rng, m, k, T, layout):
    U = rng.standard_normal((m, k)).astype(np.float32)
    Cm = rng.standard_normal((k, T)).astype(np.float32)
    mu = sigma = None
    if layout != 3:
        mu = (250.0 + 10.0 * rng.standard_normal(m)).astype(np.float32)
        sigma = (0.5 + rng.random(m)).astype(np.float32)
    return Case(m, k, T, layout, U, Cm, mu, sigma)


def parity_shapes():
    """A pairwise-covering sample of (m, k, T, layout), tests/test_gpu_verify.parity_shapes' construction."""
    lists = [MS, KS, TS, LAYOUTS]
    pairs = list(itertools.combinations(range(len(lists)), 2))
    todo = {(a, x, b, y) for a, b in pairs for x in lists[a] for y in lists[b]}
    cands = list(itertools.product(*lists))
    out = []
    while todo:
        best = max(cands, key=lambda c: sum((a, c[a], b, c[b]) in todo for a, b in pairs))
        todo -= {(a, best[a], b, best[b]) for a, b in pairs}
        out.append(best)
    assert len(out) <= 70
    return out


def check_case(L, c):
    """expand_range == the range of K12's field; expand_pack == pack_ref.encode of it, with the packing of that
    range and with a narrower one; memory."""
    X = c.expand(L)
    assert c.run_range(L) == 0, L.dmdx_last_error()
    lo, hi, n = c.range()
    wlo, whi, wn = pr.finite_range(X)
    assert (lo, hi, n) == (wlo, whi, wn), (c.m, c.k, c.T, c.layout)
    c.ws.check_untouched()
    sf, ao = pr.for_range(lo, hi)
    assert c.run_pack(L, sf, ao) == 0, L.dmdx_last_error()
    q, filled, sat = pr.encode(X, sf, ao)
    assert np.array_equal(c.Q.logical(), q), (c.m, c.k, c.T, c.layout)
    assert _cnt_vals(c.counts) == [filled, sat] == [wn, 0]
    if X.size > 1 and lo < hi:
        assert q.min() == -32767 and q.max() == 32767
    c.Q.check_untouched()
    c.check_inputs()
    return X


def test_parity_over_the_shape_edges(L):
    rng = np.random.default_rng(1701)
    assert int(L.dmdx_pack_max_k()) == 256 == int(L.dmdx_expand_max_k())
    for m, k, T, layout in parity_shapes():
        check_case(L, rand_case(rng, m, k, T, layout))


def test_several_workgroups_and_time_splits(L):
    """1003 rows = 8 row blocks, 300 snapshots = 10 tiles, one per workgroup: 80 partial slots, the T split.
    40000 rows = 313 row blocks, 470 snapshots = 15 tiles (the last partial) in 5 splits: three tiles per workgroup,
    the smallest count at which the prefetch runs and an LDS stage is used a second time."""
    for shape in ((1003, 37, 300, 2), (40000, 7, 470, 1)):
        c = rand_case(np.random.default_rng(1702), *shape)
        X = check_case(L, c)
        # a prescribed packing that is too narrow: +-32767 and the exact number of clamped values
        sf, ao = pr.for_range(240.0, 260.0)
        c.counts = _cnt(2)
        assert c.run_pack(L, sf, ao) == 0
        q, filled, sat = pr.encode(X, sf, ao)
        assert sat > 1000 and filled == 0 and _cnt_vals(c.counts) == [0, sat]
        got = c.Q.logical()
        assert np.array_equal(got, q) and got.min() == -32767 and got.max() == 32767
        # counts ACCUMULATE; without counts the codes are the same
        assert c.run_pack(L, sf, ao) == 0 and _cnt_vals(c.counts) == [0, 2 * sat]
        assert c.run_pack(L, sf, ao, counts=False) == 0 and np.array_equal(c.Q.logical(), q)
        # a negative scale_factor
        assert c.run_pack(L, -sf, ao, counts=False) == 0
        assert np.array_equal(c.Q.logical(), pr.encode(X, -sf, ao)[0])
        c.Q.check_untouched()


# ---------------------------------------------------------------- a field that exists
class Field:
    def __init__(self, X, layout, delay_ldx=None):
        self.X = X
        self.m, self.T = X.shape
        odd = layout == 2
        self.gX = mg.Guarded(self.m, self.T, _ld(self.m, layout), F32, 3 if odd else 0, DEV).fill(X).snapshot()
        self.grange = mg.Guarded(2, 1, 2, F32, 1 if odd else 0, DEV)
        self.count, self.counts = _cnt(1), _cnt(2)
        self.Q = Codes(self.m, self.T, _ld(self.m, (layout + 1) % 3), (1 + 2 * (self.m % 2)) if odd else 0)

    def run_range(self, L, accumulate=0, ws=None, **over):
        need = L.dmdx_range_workspace_bytes(self.m, self.T)
        assert need > 0
        self.ws = mg.exact_workspace(need, DEV) if ws is None else ws
        a = dict(X=self.gX.ptr, m=self.m, T=self.T, ldx=self.gX.ld, range=self.grange.ptr, count=_cnt_ptr(self.count),
                 wsp=self.ws.ptr, wsb=self.ws.nbytes)
        a.update(over)
        rc = L.dmdx_range_f32(a["X"], a["m"], a["T"], a["ldx"], a["range"], a["count"], accumulate, a["wsp"], a["wsb"], _stream())
        torch.cuda.synchronize()
        return rc

    def range(self):
        self.grange.check_untouched("range")
        r = self.grange.logical()[:, 0]
        return r[0], r[1], _cnt_vals(self.count)[0]

    def run_pack(self, L, sf, ao, **over):
        a = dict(X=self.gX.ptr, m=self.m, T=self.T, ldx=self.gX.ld, sf=sf, ao=ao, Q=self.Q.ptr, ldq=self.Q.ld,
                 counts=_cnt_ptr(self.counts))
        a.update(over)
        rc = L.dmdx_pack_f32_i16(a["X"], a["m"], a["T"], a["ldx"], a["sf"], a["ao"], a["Q"], a["ldq"], a["counts"], _stream())
        torch.cuda.synchronize()
        return rc


@pytest.mark.parametrize("shape", [(1, 1, 0), (255, 3, 2), (257, 70, 1), (1003, 33, 2), (5000, 7, 0)])
def test_field_range_and_pack_equal_the_reference(L, shape):
    m, T, layout = shape
    rng = np.random.default_rng(1703 + m)
    X = (5.0 + 3.0 * rng.standard_normal((m, T))).astype(np.float32)
    if m * T > 100:
        X[rng.random((m, T)) < 0.01] = np.nan
        X[m // 2, T // 2], X[m - 1, T - 1], X[0, 0] = np.inf, -np.inf, np.nan
    f = Field(X, layout)
    assert f.run_range(L) == 0, L.dmdx_last_error()
    lo, hi, n = f.range()
    assert (lo, hi, n) == pr.finite_range(X)
    f.ws.check_untouched()
    for sf, ao in (pr.for_range(lo, hi), (1e-4, 5.0)):
        f.counts = _cnt(2)
        assert f.run_pack(L, sf, ao) == 0, L.dmdx_last_error()
        q, filled, sat = pr.encode(X, sf, ao)
        assert np.array_equal(f.Q.logical(), q) and _cnt_vals(f.counts) == [filled, sat]
    assert sat > 0 or m * T <= 100
    f.Q.check_untouched()
    f.gX.check_untouched("X")
    f.gX.check_unchanged("X")


@pytest.mark.parametrize("lo,hi", RANGES)
def test_all_live_codes_round_trip_on_the_device(L, lo, hi):
    """pack(decode(q)) == q for all 65535 live codes, shaped 255 x 257 so that both edges are ragged; decode is
    K14's arithmetic on the host (tests/pack_ref.decode)."""
    sf, ao = pr.for_range(lo, hi)
    q = np.arange(-32767, 32768, dtype=np.int16).reshape(257, 255).T.copy()        # (m, T) = (255, 257)
    f = Field(pr.decode(q, sf, ao), 2)
    assert f.run_pack(L, sf, ao) == 0, L.dmdx_last_error()
    assert np.array_equal(f.Q.logical(), q) and _cnt_vals(f.counts) == [0, 0]
    f.Q.check_untouched()
    assert f.run_range(L) == 0
    assert f.range() == (f.X.min(), f.X.max(), 0)


# ---------------------------------------------------------------- NaN / Inf where they count
def test_planted_nan_and_inf_give_the_fill_code_there_and_nowhere_else(L):
    rng = np.random.default_rng(1704)
    m, k, T = 150, 37, 70
    i0, j0, t0 = 77, 11, 41
    base = rand_case(rng, m, k, T, 2)
    X0 = base.expand(L)
    sf, ao = pr.for_range(*pr.finite_range(X0)[:2])
    assert base.run_pack(L, sf, ao) == 0
    clean = base.Q.logical()
    assert (clean != pr.FILL).all()
    for what, val in (("U", np.nan), ("U", np.inf), ("U_last", -np.inf), ("mu", np.nan), ("mu", np.inf), ("sigma", np.nan),
                      ("C", np.nan), ("C", -np.inf)):
        o = dict(U=base.U.copy(), C=base.C.copy(), mu=base.mu.copy(), sigma=base.sigma.copy())
        if what == "U":
            o["U"][i0, j0] = val
        elif what == "U_last":
            o["U"][i0, k - 1] = val
        elif what == "C":
            o["C"][j0, t0] = val
        else:
            o[what][i0] = val
        c = Case(m, k, T, 2, o["U"], o["C"], o["mu"], o["sigma"])
        hit = np.zeros((m, T), dtype=bool)
        if what == "C":
            hit[:, t0] = True
        else:
            hit[i0, :] = True
        assert c.run_range(L) == 0 and c.run_pack(L, sf, ao) == 0, L.dmdx_last_error()
        got = c.Q.logical()
        assert (got[hit] == pr.FILL).all() and np.array_equal(got[~hit], clean[~hit]), (what, val)
        assert _cnt_vals(c.counts) == [int(hit.sum()), 0], (what, val)
        lo, hi, n = c.range()
        assert n == int(hit.sum()) and (lo, hi) == pr.finite_range(X0[~hit])[:2], (what, val)
        assert np.array_equal(got, pr.encode(c.expand(L), sf, ao)[0])
    # everything missing: the range is (+inf, -inf), every code the fill code
    c = Case(m, k, T, 2, base.U, base.C, np.full(m, np.nan, dtype=np.float32), base.sigma)
    assert c.run_range(L) == 0 and c.run_pack(L, 1.0, 0.0) == 0
    assert c.range() == (np.float32(np.inf), np.float32(-np.inf), m * T)
    assert (c.Q.logical() == pr.FILL).all() and _cnt_vals(c.counts) == [m * T, 0]


# ---------------------------------------------------------------- accumulate, reproducibility
def test_accumulate_over_row_blocks_equals_one_call(L):
    rng = np.random.default_rng(1705)
    m, k, T = 300, 33, 70
    full = rand_case(rng, m, k, T, 2)
    full.U[200, 3] = np.nan
    full = Case(m, k, T, 2, full.U, full.C, full.mu, full.sigma)
    assert full.run_range(L) == 0, L.dmdx_last_error()
    want = full.range()
    assert want[2] == T
    parts = [slice(0, 170), slice(170, 171), slice(171, m)]
    acc = None
    for n, s in enumerate(parts):
        c = Case(s.stop - s.start, k, T, 2, full.U[s], full.C, full.mu[s], full.sigma[s])
        if acc is None:
            acc = c
            assert c.run_range(L) == 0
        else:
            assert c.run_range(L, accumulate=1, range=acc.grange.ptr, count=_cnt_ptr(acc.count)) == 0, L.dmdx_last_error()
            assert bool((c.grange.ibuf == c.grange.canary).all())
    assert acc.range() == want
    # the field twin, and an accumulate that finds nothing new
    X = full.expand(L)
    halves = [Field(np.ascontiguousarray(X[s]), 2) for s in (slice(0, 123), slice(123, m))]
    assert halves[0].run_range(L) == 0
    assert halves[1].run_range(L, accumulate=1, range=halves[0].grange.ptr, count=_cnt_ptr(halves[0].count)) == 0
    assert halves[0].range() == want
    assert halves[1].run_range(L, accumulate=1, range=halves[0].grange.ptr, count=_cnt_ptr(halves[0].count)) == 0
    assert halves[0].range() == (want[0], want[1], want[2] + int((~np.isfinite(X[123:])).sum()))


def test_two_calls_give_the_same_bits(L):
    c = rand_case(np.random.default_rng(1706), 1003, 50, 131, 2)
    assert c.run_range(L) == 0 and c.run_pack(L, 1e-2, 250.0) == 0, L.dmdx_last_error()
    first = (c.grange.iview.clone(), c.Q.buf.clone(), c.count.clone(), c.counts.clone())
    c.grange.ibuf.fill_(c.grange.canary)
    c.Q.buf.fill_(Codes.CANARY)
    c.count, c.counts = _cnt(1), _cnt(2)
    assert c.run_range(L) == 0 and c.run_pack(L, 1e-2, 250.0) == 0
    for a, b in zip(first, (c.grange.iview, c.Q.buf, c.count, c.counts)):
        assert torch.equal(a, b)


def test_bits_do_not_depend_on_the_base_or_the_stride_of_q(L):
    rng = np.random.default_rng(1707)
    m, k, T = 257, 20, 45
    U, Cm = rng.standard_normal((m, k)).astype(np.float32), rng.standard_normal((k, T)).astype(np.float32)
    got = []
    for layout in LAYOUTS[:3]:
        c = Case(m, k, T, layout, U, Cm)
        for off in (0, 1, 2, 5):
            c.Q = Codes(m, T, m + off, off)
            assert c.run_pack(L, 1e-3, 0.0, counts=False) == 0, L.dmdx_last_error()
            got.append(c.Q.logical())
            c.Q.check_untouched()
    assert all(np.array_equal(g, got[0]) for g in got[1:])


# ---------------------------------------------------------------- refusals
def test_refused_calls_write_nothing(L):
    c = rand_case(np.random.default_rng(1708), 70, 9, 40, 1)
    big = 2 ** 31
    ws = mg.exact_workspace(L.dmdx_expand_range_workspace_bytes(c.m, c.k, c.T), DEV)
    shape_bad = [dict(k=0), dict(k=257), dict(U=None), dict(C=None), dict(m=0), dict(T=0), dict(m=-1), dict(ldu=c.m - 1),
                 dict(ldc=c.k - 1), dict(ldu=big), dict(ldc=big), dict(m=big, ldu=big), dict(T=big)]
    for over in shape_bad + [dict(range=None), dict(count=None)]:
        assert c.run_range(L, ws=ws, **over) == E_INVALID, over
        assert L.dmdx_last_error()
    assert c.run_range(L, ws=ws, wsb=ws.nbytes - 1) == E_WORKSPACE
    assert c.run_range(L, ws=ws, wsp=None) == E_WORKSPACE
    for over in shape_bad + [dict(Q=None), dict(ldq=c.m - 1), dict(ldq=big), dict(sf=0.0), dict(sf=float("nan")),
                             dict(sf=float("inf")), dict(ao=float("nan")), dict(ao=float("-inf"))]:
        assert c.run_pack(L, over.pop("sf", 0.5), over.pop("ao", 0.0), **over) == E_INVALID, over
        assert L.dmdx_last_error()
    f = Field(np.ones((70, 40), dtype=np.float32), 1)
    fws = mg.exact_workspace(L.dmdx_range_workspace_bytes(f.m, f.T), DEV)
    for over in (dict(X=None), dict(m=0), dict(T=0), dict(ldx=0), dict(ldx=big), dict(m=big), dict(range=None), dict(count=None)):
        assert f.run_range(L, ws=fws, **over) == E_INVALID, over
    assert f.run_range(L, ws=fws, wsb=fws.nbytes - 1) == E_WORKSPACE
    for over in (dict(X=None), dict(m=0), dict(T=0), dict(ldx=0), dict(Q=None), dict(ldq=f.m - 1), dict(sf=0.0),
                 dict(sf=float("nan")), dict(ao=float("inf"))):
        assert f.run_pack(L, over.pop("sf", 0.5), over.pop("ao", 0.0), **over) == E_INVALID, over
    for w in (ws, fws):
        w.check_unused()
        w.check_untouched()
    for x in (c, f):
        assert bool((x.grange.ibuf == x.grange.canary).all())
        x.Q.check_unwritten()
        assert _cnt_vals(x.count) == [0] and _cnt_vals(x.counts) == [0, 0]
    c.check_inputs()


# ---------------------------------------------------------------- the wrappers and the file
def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def test_wrappers_and_pack_blocks_match_the_reference():
    from dmd_era5_amd.forecast import pack_blocks, pack_field_blocks
    from dmd_era5_amd.kernels import default_kernels
    from dmd_era5_amd.labeled import Packing

    K = default_kernels()
    rs = np.random.RandomState(0)
    m, k, T = 333, 5, 41
    U, Cm = rs.standard_normal((m, k)).astype(np.float32), rs.standard_normal((k, T)).astype(np.float32)
    mu, sd = (rs.standard_normal(m) * 4).astype(np.float32), (0.5 + rs.rand(m)).astype(np.float32)
    mu[200:] += 100.0
    U[17, 2] = np.nan
    Ut, Ct = _t(U.T), _t(Cm.T)
    X = K.expand(Ut, Ct, _t(mu), _t(sd))
    Xn = X.cpu().numpy()
    rng, cnt = K.expand_range(Ut, Ct, _t(mu), _t(sd))
    assert (rng[0].item(), rng[1].item(), cnt.item()) == tuple(float(v) for v in pr.finite_range(Xn))
    r2, c2 = K.field_range(X)
    assert torch.equal(r2, rng) and torch.equal(c2, cnt)
    pk = Packing.for_range(rng[0].item(), rng[1].item())
    big = torch.full((T, m + 7), 777, dtype=torch.int16, device=DEV)
    Q, counts = K.expand_pack(Ut, Ct, _t(mu), _t(sd), pk, out=big[:, 3:3 + m])
    want = pr.encode(Xn, pk.scale_factor, pk.add_offset)
    assert np.array_equal(Q.cpu().numpy(), want[0]) and counts.tolist() == [T, 0]
    assert bool((big[:, :3] == 777).all()) and bool((big[:, 3 + m:] == 777).all())
    Q2, counts2 = K.pack(X, pk, counts=counts)
    assert torch.equal(Q2, Q) and counts2.tolist() == [2 * T, 0]
    # groups cut through the block, in runs; the range merges over the runs of a group
    lab = np.array([0] * 100 + [1] * 100 + [0] * 33 + [2] * 100)
    cuts = [(0, 150), (150, 333)]
    res = pack_blocks([Ut[:, a:b] for a, b in cuts], Ct, [_t(mu[a:b]) for a, b in cuts], [_t(sd[a:b]) for a, b in cuts],
                      groups=[_t(lab[a:b], torch.int64) for a, b in cuts])
    got = torch.cat(res["codes"], dim=1).cpu().numpy()
    fld = pack_field_blocks([X[:, a:b] for a, b in cuts], groups=[_t(lab[a:b], torch.int64) for a, b in cuts])
    assert np.array_equal(torch.cat(fld["codes"], dim=1).cpu().numpy(), got)
    for g in range(3):
        lo, hi, n = pr.finite_range(Xn[:, lab == g])
        sf, ao = pr.for_range(lo, hi)
        assert (res["packing"][g].scale_factor, res["packing"][g].add_offset) == (sf, ao)
        assert np.array_equal(got[:, lab == g], pr.encode(np.ascontiguousarray(Xn[:, lab == g]), sf, ao)[0])
        assert int(res["filled"][g]) == n == int(fld["filled"][g]) and int(res["saturated"][g]) == 0
    with pytest.raises(Exception):
        K.expand_pack(Ut, Ct, None, None, Packing(0.0, 0.0))


def test_write_forecast_slice_end_to_end(tmp_path, monkeypatch):
    """A small fitted forecast (as tests/test_gpu_forecast.py builds one) written in slabs: the codes in the file
    equal pack_ref of DmdForecast.fields(t), and slab = 1 gives the same file."""
    from dmd_era5_amd import bopdmd as bop
    from dmd_era5_amd import era5_svd, hdf5_lite, io_netcdf
    from dmd_era5_amd.forecast import DmdForecast

    if not hdf5_lite.available():
        pytest.skip("libhdf5 not found")
    monkeypatch.setenv("DMDX_NETCDF_BACKEND", "hdf5")
    t = np.linspace(0, 6, 200)
    half = np.array([-0.1 + 2.0j, -0.5 + 5.0j, -0.02 + 0.7j])
    alpha = np.concatenate([half, half.conj()])
    rs = np.random.RandomState(2)
    mh = rs.standard_normal((3, 6)) + 1j * rs.standard_normal((3, 6))
    H = (np.exp(np.outer(t, alpha)) @ np.concatenate([mh, mh.conj()])).real
    res = bop.optdmd(torch.from_numpy(H).to(torch.complex128).to(DEV), torch.from_numpy(t).to(DEV), 6, tol=1e-10, maxiter=60)
    nvar, nlev, nlat, nlon = 2, 2, 9, 14
    plane = nlev * nlat * nlon
    M = nvar * plane
    Q = np.linalg.qr(rs.standard_normal((M, 6)))[0].astype(np.float32)
    mu = np.concatenate([250 + 20 * rs.rand(plane), 10 * rs.standard_normal(plane)]).astype(np.float32)
    blocks = [(0, 300), (300, M)]
    f = DmdForecast([_t(Q[a:b].T) for a, b in blocks], res, means=[_t(mu[a:b]) for a, b in blocks])
    T = 23
    tt = np.linspace(5.0, 8.0, T)
    time = np.datetime64("2019-01-01T00", "ns") + np.arange(T) * np.timedelta64(1, "h")
    grid = dict(levels=[1000, 850], latitude=np.linspace(40, 0, nlat), longitude=np.linspace(0, 65, nlon))
    names = ["temperature", "u_component_of_wind"]
    paths = [str(tmp_path / n) for n in ("slabs.nc", "one.nc")]
    out = era5_svd.write_forecast_slice(paths[0], f, tt, time, names, **grid, slab=5, attrs={"date_downloaded": "fixed"})
    era5_svd.write_forecast_slice(paths[1], f, tt, time, names, **grid, slab=1, attrs={"date_downloaded": "fixed"})
    assert open(paths[0], "rb").read() == open(paths[1], "rb").read()
    F = torch.cat(f.fields(torch.from_numpy(tt).to(DEV)), dim=1).cpu().numpy()
    ds = io_netcdf.open_dataset(paths[0])
    r = hdf5_lite.Reader(paths[0])
    for g, name in enumerate(names):
        want = np.ascontiguousarray(F[:, g * plane:(g + 1) * plane]).reshape(T, nlev, nlat, nlon)
        sf, ao = pr.for_range(*pr.finite_range(want)[:2])
        assert (out["packing"][name].scale_factor, out["packing"][name].add_offset) == (sf, ao)
        assert np.array_equal(r.read(name), pr.encode(want, sf, ao)[0])
        assert (out["filled"][name], out["saturated"][name]) == (0, 0)
        got = np.asarray(ds[name].values)
        assert (np.abs(got.astype(np.float64) - want) <= sf / 2 + pr.ulp32(want)).all()
    r.close()
