"""K25 without a GPU: tests/quant_ref.py (the host definition) against numpy and against the order contract, the
refusals of dmdx_clim_quantile_f32 (the library loads without a device), and the host layer -- Climatology.fit(
quantiles=), quantile_thresholds, the NetCDF round trip -- on a kernel double whose clim_quantile is quant_ref."""
import ctypes as C

import numpy as np
import pytest
import torch

import quant_ref as qr
from exceed_ref import ExceedDouble
from expand_ref import ExpandDouble
from test_climatology import ROWS, ClimDouble, _hourly

QNAN = 0x7FC00000
E_INVALID = -1000
NS = (1, 2, 3, 19, 37, 64, 65, 365)
QS = (0.0, 0.1, 0.25, 1.0 / 3.0, 0.5, 0.9, 0.99, 1.0)


class QuantDouble(ExceedDouble, ExpandDouble, ClimDouble):
    """ClimDouble (a CpuKernelDouble) + HipKernels.clim_quantile, computed by quant_ref."""

    name = "cpu-double+clim+quantile"

    def clim_quantile(self, Xt, order, start, q, method="linear", out=None, streamed=False):
        Q = torch.from_numpy(qr.quantile(Xt.numpy().T, order.numpy(), start.numpy(), q, method))
        if out is None:
            return Q
        out.copy_(Q)
        return out


def _bits(a):
    a = a.numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _ulps(a, b):
    """The distance of two fp32 arrays in units of the last place (finite values of any sign)."""
    return np.abs(qr.keys(a).astype(np.int64) - qr.keys(b).astype(np.int64))


# ---------------------------------------------------------------- (a) the definition against numpy
@pytest.mark.parametrize("n", NS)
def test_quant_ref_against_numpy(n):
    rs = np.random.RandomState(100 + n)
    m = 23
    smooth = (250.0 + 30.0 * rs.standard_normal((m, n))).astype(np.float32)
    tied = np.round(3.0 * rs.standard_normal((m, n)) + 20.0).astype(np.float32)      # few distinct values, none a zero
    signed = (rs.standard_normal((m, n)) * 10.0 ** rs.randint(-3, 4, (m, 1))).astype(np.float32)
    for name, X in (("smooth", smooth), ("tied", tied), ("signed", signed)):
        assert not (X == 0).any()                                # (numpy's sort does not tell -0.0 from +0.0)
        for method in ("linear", "lower", "higher"):
            got = qr.of_members(X, QS, method)
            want = np.quantile(X.astype(np.float64), QS, axis=1, method=method).astype(np.float32)
            assert got.shape == want.shape == (len(QS), m)
            if method == "linear":
                # both sides interpolate in fp64 (numpy with another, equally valid, formula) and round once
                assert _ulps(got, want).max() <= 1, (name, n, int(_ulps(got, want).max()))
            else:
                assert np.array_equal(_bits(got), _bits(want)), (name, n, method)
        assert np.array_equal(_bits(qr.of_members(X, [0.0, 1.0])), _bits(np.stack([X.min(axis=1), X.max(axis=1)])))


def test_quant_ref_lists_are_clim_ref_lists():
    import clim_ref as cr

    rs = np.random.RandomState(5)
    X = rs.standard_normal((4, 9)).astype(np.float32)
    order = np.array([3, 3, 9, 0, -1, 8, 2], dtype=np.int32)     # a snapshot twice, an entry = T, an entry < 0
    start = np.array([0, 0, 5, 40], dtype=np.int32)              # an empty slot, an end offset past n_order
    assert cr.counts(order, start, 9).tolist() == [0, 3, 2]
    got = qr.quantile(X, order, start, (0.0, 0.5, 1.0), "lower")
    assert got.shape == (3, 3, 4) and (_bits(got[:, 0]) == QNAN).all()
    assert np.array_equal(got[:, 1], np.stack([X[:, [3, 0]].min(axis=1), X[:, 3], X[:, [3, 0]].max(axis=1)]))
    assert np.array_equal(got[:, 2], np.stack([X[:, [8, 2]].min(axis=1)] * 2 + [X[:, [8, 2]].max(axis=1)]))


# ---------------------------------------------------------------- (b) the order contract
def test_order_contract_and_nan():
    den = np.array([0x00000003], dtype=np.uint32).view(np.float32)[0]
    ladder = np.array([-np.inf, -1.0, -0.0, 0.0, den, 1.0, np.inf], dtype=np.float32)
    k = qr.keys(ladder).astype(np.int64)
    assert (np.diff(k) > 0).all()                                # -Inf < -1 < -0.0 < +0.0 < denormal < 1 < +Inf
    assert np.array_equal(_bits(qr.unkeys(qr.keys(ladder))), _bits(ladder))
    rs = np.random.RandomState(1)
    X = np.stack([ladder[rs.permutation(7)] for _ in range(5)])
    qs = [i / 6.0 for i in range(7)]
    # fl(i / 6) * 6 may round to just below i: the position is the definition's, the value the ladder's member there
    pos = [qr.position(q, 7, "lower")[0] for q in qs]
    assert sorted(set(pos)) == list(range(7)) or all(abs(p - i) <= 1 for i, p in enumerate(pos))
    got = qr.of_members(X, qs, "lower")
    for i in range(7):
        assert (_bits(got[i]) == _bits(ladder[pos[i]])).all()    # the bits of the member, -0.0 and the denormal included
    assert (_bits(qr.of_members(X, [0.0, 1.0 / 3.0, 0.5, 1.0], "higher")) == _bits(ladder[[0, 2, 3, 6]])[:, None]).all()
    # between -0.0 and +0.0, linear: 0.5 * (+0.0 - -0.0) + -0.0 = +0.0 in fp64, rounded to fp32
    z = qr.of_members(np.array([[0.0, -0.0]], dtype=np.float32), [0.0, 0.5, 1.0])
    assert _bits(z).reshape(-1).tolist() == [0x80000000, 0x00000000, 0x00000000]
    # a NaN member: the quiet NaN for every quantile of that row, the other rows as they were
    Xn = X.copy()
    Xn[2, 3] = np.nan
    a, b = qr.of_members(X, [0.0, 0.3, 1.0]), qr.of_members(Xn, [0.0, 0.3, 1.0])
    assert (_bits(b[:, 2]) == QNAN).all()
    keep = [0, 1, 3, 4]
    same = (_bits(a[:, keep]) == _bits(b[:, keep])) | (np.isnan(a[:, keep]) & np.isnan(b[:, keep]))   # (Inf - Inf rows)
    assert same.all()
    assert (_bits(qr.of_members(np.empty((3, 0), dtype=np.float32), [0.5, 0.6])) == QNAN).all()


# ---------------------------------------------------------------- (c) the C ABI refuses without a GPU
def test_refusals_of_the_entry_point_without_a_gpu():
    from dmd_era5_amd import _lib

    L = _lib.load()
    assert L.dmdx_clim_quantile_max_q() == 4
    cap = L.dmdx_clim_quantile_max_staged()
    assert cap >= 365 and cap % 4 == 0                           # the three tiers: cap / 4, cap / 2, cap entries
    m, T, S, n, big = 12, 37, 5, 33, 2**31
    p = 4096                                                     # never dereferenced: every call below is refused
    q2 = (C.c_double * 2)(0.1, 0.9)
    good = dict(X=p, m=m, T=T, ldx=m, order=p, n_order=n, start=p, S=S, q=q2, J=2, method=0, streamed=0, out=p, ldo=m)
    bad = [dict(X=None), dict(order=None), dict(start=None), dict(q=None), dict(out=None), dict(S=0), dict(S=-1),
           dict(J=0), dict(J=5), dict(J=-1), dict(method=-1), dict(method=3), dict(ldx=m - 1), dict(ldo=m - 1),
           dict(m=-1), dict(T=-1), dict(n_order=-1), dict(m=big, ldx=big, ldo=big), dict(T=big), dict(n_order=big),
           dict(S=big), dict(ldx=big), dict(ldo=big), dict(S=big // 2, J=2)]
    for qbad in ((0.5, np.nan), (-1e-9, 0.5), (0.5, 1.0 + 1e-9), (np.inf, 0.5)):
        bad.append(dict(q=(C.c_double * 2)(*qbad)))
    bad.append(dict(q=(C.c_double * 4)(0.1, 0.2, 0.3, 1.5), J=4))
    for change in bad:
        L.dmdx_clim_quantile_f32(None, 0, 0, 0, None, 0, None, 1, None, 1, 0, 0, None, 0, None)   # resets the message
        assert L.dmdx_clim_quantile_f32(*{**good, **change}.values(), None) == E_INVALID, change
        assert b"clim_quantile" in L.dmdx_last_error(), change
    # only the first J values are looked at
    assert L.dmdx_clim_quantile_f32(*{**good, "q": (C.c_double * 2)(0.5, 7.0), "J": 1, "m": 0}.values(), None) == 0
    assert L.dmdx_clim_quantile_f32(*{**good, "m": 0}.values(), None) == 0      # m == 0: the checks, then nothing


# ---------------------------------------------------------------- (d) the host layer on the double
def _toy(T=96, seed=0):
    rs = np.random.RandomState(seed)
    times = _hourly("2020-03-01T00", T, 1)
    X = [torch.from_numpy((rs.standard_normal((T, mb)) + 5.0 * np.sin(np.arange(T) * 2 * np.pi / 24)[:, None])
                          .astype(np.float32)) for mb in ROWS]
    return times, X


def test_fit_with_quantiles_and_the_threshold_tables():
    from dmd_era5_amd.climatology import Climatology, slots_of
    from dmd_era5_amd.forecast import exceed_prob_blocks

    times, X = _toy()
    kern = QuantDouble()
    clim = Climatology.fit(X, times, "hour", with_std=True, quantiles=(0.1, 0.9), kern=kern)
    assert clim.q == (0.1, 0.9) and clim.method == "linear" and len(clim.quant) == 2
    _, order, start, S = slots_of(times, "hour")
    th, an = clim.quantile_thresholds(), clim.quantile_thresholds(anomaly=True)
    for b, mb in enumerate(ROWS):
        want = qr.quantile(X[b].numpy().T, order, start, (0.1, 0.9))
        assert clim.quant[b].shape == (2, 24, mb) and clim.quant[b].dtype == torch.float32
        assert np.array_equal(_bits(clim.quant[b]), _bits(want))
        assert th[b].is_contiguous() and np.array_equal(_bits(th[b]), _bits(want))
        assert np.array_equal(_bits(an[b]), _bits(want - clim.mean[b].numpy()[None]))     # rounded once, in fp32
        assert (want[0] <= clim.mean[b].numpy()).all() and (clim.mean[b].numpy() <= want[1]).all()
    low = Climatology.fit(X, times, "hour", quantiles=0.5, method="lower", kern=kern)
    assert low.q == (0.5,) and low.method == "lower" and low.sd is None
    assert np.array_equal(_bits(low.quant[1]), _bits(qr.quantile(X[1].numpy().T, order, start, [0.5], "lower")))
    # the table is what K24's drivers take, with the labels of the climatology
    rs = np.random.RandomState(3)
    Ub = [torch.from_numpy(rs.standard_normal((2, mb)).astype(np.float32)) for mb in ROWS]
    Cm = torch.from_numpy(rs.standard_normal((4, 3, 2)).astype(np.float32))
    lab = clim.slots(_hourly("2021-07-01T05", 3, 1))
    P = exceed_prob_blocks(Ub, Cm, th, lab, kern=kern)
    assert [tuple(p.shape) for p in P] == [(2, 3, mb) for mb in ROWS]
    assert all(bool(((p >= 0) & (p <= 1)).all()) for p in P)
    # an unpopulated slot carries NaN thresholds; the seven positional arguments still build a climatology
    short = Climatology.fit([x[:20] for x in X], times[:20], "hour", quantiles=(0.5,), kern=kern)
    assert all((_bits(Q[:, 20:]) == QNAN).all() and not np.isnan(Q[:, :20].numpy()).any() for Q in short.quant)
    old = Climatology("hour", 0, clim.mean, clim.sd, clim.counts, 0, kern)
    assert old.q is None and old.quant is None and old.method == "linear"
    assert len(old.thresholds([1.0])) == 2


def test_value_errors_before_any_launch():
    from dmd_era5_amd.climatology import Climatology

    class Counting(QuantDouble):
        calls = 0

        def clim_mean(self, *a, **kw):
            Counting.calls += 1
            return super().clim_mean(*a, **kw)

    times, X = _toy(T=30)
    for bad in ((), (0.1, 0.2, 0.3, 0.4, 0.5), (0.5, 1.5), (-0.1,), (np.nan,)):
        with pytest.raises(ValueError, match="quantiles"):
            Climatology.fit(X, times, "hour", quantiles=bad, kern=Counting())
    with pytest.raises(ValueError, match="method"):
        Climatology.fit(X, times, "hour", quantiles=(0.5,), method="nearest", kern=Counting())
    assert Counting.calls == 0
    plain = Climatology.fit(X, times, "hour", kern=Counting())
    assert plain.quant is None and plain.q is None
    with pytest.raises(ValueError, match="no quantiles"):
        plain.quantile_thresholds()


def test_dataset_round_trip_with_and_without_quantiles(tmp_path):
    from dmd_era5_amd import io_netcdf
    from dmd_era5_amd.climatology import Climatology
    from dmd_era5_amd.labeled import Coord

    times, X = _toy(T=50)
    kern = QuantDouble()
    qs = (0.1, 1.0 / 3.0, 0.9)
    clim = Climatology.fit(X, times, "hour", with_std=True, ddof=1, quantiles=qs, method="higher", kern=kern)
    M = sum(ROWS)
    coords = {"space": Coord("space", np.arange(M, dtype=np.int64)), "time": Coord("time", times)}
    ds = clim.to_dataset(coords)
    assert ds["clim_quantile"].dims == ("quantile", "slot", "space") and ds["clim_quantile"].shape == (3, 24, M)
    assert ds.coords["quantile"].values.dtype == np.float64 and ds.attrs["quantile_method"] == "higher"
    path = str(tmp_path / "clim_q.nc")
    io_netcdf.to_netcdf(ds, path)
    back = Climatology.from_dataset(io_netcdf.open_dataset(path), rows=ROWS, device="cpu", kern=kern)
    assert back.q == qs and back.method == "higher" and back.ddof == 1       # 1 / 3 comes back as the same double
    for b in range(2):
        assert np.array_equal(_bits(back.quant[b]), _bits(clim.quant[b]))     # the NaN of the empty slots included
        assert np.array_equal(_bits(back.mean[b]), _bits(clim.mean[b]))
        assert back.quant[b].shape == clim.quant[b].shape and back.quant[b].is_contiguous()
    a, b = back.quantile_thresholds(anomaly=True), clim.quantile_thresholds(anomaly=True)
    assert all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(a, b))
    one = Climatology.from_dataset(io_netcdf.open_dataset(path), device="cpu", kern=kern)
    assert len(one.quant) == 1 and one.quant[0].shape == (3, 24, M)
    # a file written without quantiles holds none of the new names and loads as it always did
    plain = Climatology.fit(X, times, "hour", with_std=True, kern=kern)
    dsp = plain.to_dataset(coords)
    assert "clim_quantile" not in dsp and "quantile" not in dsp.coords and "quantile_method" not in dsp.attrs
    ppath = str(tmp_path / "clim_plain.nc")
    io_netcdf.to_netcdf(dsp, ppath)
    old = Climatology.from_dataset(io_netcdf.open_dataset(ppath), rows=ROWS, device="cpu", kern=kern)
    assert old.quant is None and old.q is None and old.method == "linear"
    assert all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(old.mean, plain.mean))
    with pytest.raises(ValueError, match="no quantiles"):
        old.quantile_thresholds()
