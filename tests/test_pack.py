"""CPU tests of K17's host side: labeled.Packing.encode / for_range against tests/pack_ref.py, forecast.pack_blocks
through the torch / numpy expression and through a kernel double, hdf5_lite.Writer.create / write_slab, and
era5_svd.write_forecast_slice with the file read back and run through main()."""
import numpy as np
import pytest
import torch

import pack_ref as pr
from expand_ref import ExpandDouble
from kernel_double import CpuKernelDouble

RANGES = [(220.0, 300.0), (-40.0, 55.0), (0.0, 1.0), (48000.0, 58000.0), (-3.5, 1e-3)]


class DoubleWithPack(pr.PackDouble, ExpandDouble, CpuKernelDouble):
    name = "cpu-double+pack"


class DoubleWithExpand(ExpandDouble, CpuKernelDouble):
    name = "cpu-double+expand"


PROVIDERS = [DoubleWithExpand, DoubleWithPack]        # the module's own expression / the kernel double


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def _packing(sf, ao):
    from dmd_era5_amd.labeled import Packing

    return Packing(sf, ao, (pr.FILL,))


# ---------------------------------------------------------------- the arithmetic
def test_for_range_cases():
    from dmd_era5_amd.labeled import Packing

    for lo, hi in RANGES:
        p = Packing.for_range(lo, hi)
        assert (p.scale_factor, p.add_offset) == ((hi - lo) / 65534.0, (hi + lo) / 2.0) == pr.for_range(lo, hi)
        assert p.fills == (-32768,)
        q = p.encode(np.array([lo, hi], dtype=np.float64).astype(np.float32))
        if np.float32(lo) == lo and np.float32(hi) == hi:
            assert q.tolist() == [-32767, 32767]
    p = Packing.for_range(273.15, 273.15)
    assert (p.scale_factor, p.add_offset, p.fills) == (1.0, 273.15, (-32768,))
    p = Packing.for_range(np.float32(np.inf), np.float32(-np.inf))
    assert (p.scale_factor, p.add_offset, p.fills) == (1.0, 0.0, (-32768,))
    for bad in ((1.0, 0.0), (np.nan, 1.0), (0.0, np.inf), (-np.inf, np.inf)):
        with pytest.raises(ValueError):
            Packing.for_range(*bad)


def test_range_ends_map_to_the_end_codes():
    """vmin <-> -32767 and vmax <-> 32767, in fp64 arithmetic on fp32 ends (what the range kernels return)."""
    from dmd_era5_amd.labeled import Packing

    rs = np.random.RandomState(0)
    for lo, hi in RANGES + [tuple(sorted(rs.standard_normal(2) * 10.0 ** e)) for e in range(-3, 6)]:
        lo, hi = np.float32(lo), np.float32(hi)
        p = Packing.for_range(lo, hi)
        assert p.encode(np.array([lo, hi], dtype=np.float32)).tolist() == [-32767, 32767]
        assert p.encode(np.array([lo, hi], dtype=np.float32), counts=True)[1:] == (0, 0)


def test_encode_rounds_half_to_even_clamps_and_fills():
    p = _packing(0.25, 10.0)
    # quotients -2.5, -1.5, -0.5, 0.5, 1.5, 2.5, 3.5 (all exact in fp32 and fp64)
    x = (10.0 + 0.25 * np.array([-2.5, -1.5, -0.5, 0.5, 1.5, 2.5, 3.5])).astype(np.float32)
    assert p.encode(x).tolist() == [-2, -2, 0, 0, 2, 2, 4]
    # the clamp and its count: 32767 and -32767 fit, one more does not; 1e30 is far out
    x = (10.0 + 0.25 * np.array([32767, 32768, -32767, -32768, 32767.5, 4e9])).astype(np.float32)
    x = np.concatenate([x, np.array([1e30, -1e30], dtype=np.float32)])
    q, filled, saturated = p.encode(x, counts=True)
    assert q.tolist() == [32767, 32767, -32767, -32767, 32767, 32767, 32767, -32767]
    assert (filled, saturated) == (0, 6)          # 32767.5 rounds to 32768 (even): clamped
    # NaN / +-Inf -> the fill code, counted, never saturated
    x = np.array([np.nan, np.inf, -np.inf, 10.0, -np.nan], dtype=np.float32)
    q, filled, saturated = p.encode(x, counts=True)
    assert q.tolist() == [-32768, -32768, -32768, 0, -32768] and (filled, saturated) == (4, 0)
    assert q.dtype == np.int16
    # a negative scale_factor is a packing too
    assert _packing(-0.5, 0.0).encode(np.array([1.0, -1.25], dtype=np.float32)).tolist() == [-2, 2]


def test_encode_equals_the_reference_on_random_fields():
    rs = np.random.RandomState(1)
    for lo, hi in RANGES:
        x = (lo + (hi - lo) * (1.2 * rs.rand(50, 41) - 0.1)).astype(np.float32)       # 10 % outside on both sides
        x[rs.rand(*x.shape) < 0.02] = np.nan
        x[3, 4], x[5, 6] = np.inf, -np.inf
        sf, ao = pr.for_range(lo, hi)
        q, filled, saturated = _packing(sf, ao).encode(x, counts=True)
        want = pr.encode(x, sf, ao)
        assert np.array_equal(q, want[0]) and (filled, saturated) == want[1:]
        assert filled == int((~np.isfinite(x)).sum()) and saturated > 0


@pytest.mark.parametrize("lo,hi", RANGES)
def test_all_live_codes_round_trip(lo, hi):
    from dmd_era5_amd.labeled import Packing

    p = Packing.for_range(lo, hi)
    q = np.arange(-32767, 32768, dtype=np.int16)
    x = p.decode(q)
    assert x.dtype == np.float32 and np.isfinite(x).all()
    assert np.array_equal(p.encode(x), q)
    assert np.array_equal(pr.encode(pr.decode(q, p.scale_factor, p.add_offset), p.scale_factor, p.add_offset)[0], q)
    assert np.isnan(p.decode(np.array([-32768], dtype=np.int16))[0])


@pytest.mark.parametrize("lo,hi", RANGES)
def test_decode_of_encode_is_within_half_a_step(lo, hi):
    """|decode(encode(x)) - x| <= scale_factor / 2 + one fp32 ulp of x: half a step of the quantisation (the
    quotient and its rounding are fp64: 2^-53 effects vanish in the ulp), one rounding of the decoded value."""
    from dmd_era5_amd.labeled import Packing

    rs = np.random.RandomState(2)
    x = (lo + (hi - lo) * rs.rand(20000)).astype(np.float32)
    p = Packing.for_range(x.min(), x.max())
    back = p.decode(p.encode(x)).astype(np.float64)
    assert (np.abs(back - x.astype(np.float64)) <= p.scale_factor / 2 + pr.ulp32(x)).all()


# ---------------------------------------------------------------- pack_blocks
def _blocks_case(seed=3, T=9):
    """Three blocks of 14, 9 and 12 rows, four groups: group 1 comes in several runs, group 3 is absent from the
    first two blocks and group 0 from the last."""
    rs = np.random.RandomState(seed)
    k = 5
    sizes = [14, 9, 12]
    labels = [np.array([0] * 4 + [1] * 3 + [2] * 2 + [1] * 5), np.array([1] * 2 + [0] * 3 + [2] * 4),
              np.array([3] * 6 + [1] * 1 + [3] * 2 + [2] * 3)]
    U = [rs.standard_normal((k, m)).astype(np.float32) for m in sizes]
    means = [(rs.standard_normal(m) * 5 + 20 * lab).astype(np.float32) for m, lab in zip(sizes, labels)]
    stds = [(0.5 + rs.rand(m)).astype(np.float32) for m in sizes]
    Ct = rs.standard_normal((T, k)).astype(np.float32)
    return U, means, stds, Ct, labels


def _fields(kern, U, means, stds, Ct):
    from dmd_era5_amd.forecast import expand_blocks

    return [F.numpy() for F in expand_blocks([_t(u) for u in U], _t(Ct), [_t(v) for v in means], [_t(v) for v in stds],
                                             kern=kern)]


@pytest.mark.parametrize("provider", PROVIDERS)
def test_pack_blocks_with_groups_in_several_runs(provider):
    from dmd_era5_amd.forecast import pack_blocks

    kern = provider()
    U, means, stds, Ct, labels = _blocks_case()
    U[1][:, 3] = np.nan                                 # a row of group 0 that is missing
    F = _fields(kern, U, means, stds, Ct)
    res = pack_blocks([_t(u) for u in U], _t(Ct), [_t(v) for v in means], [_t(v) for v in stds],
                      groups=[_t(lab, torch.int64) for lab in labels], kern=kern)
    assert len(res["packing"]) == 4 and tuple(res["range"].shape) == (4, 2)
    for g in range(4):
        vals = np.concatenate([f[:, lab == g].ravel() for f, lab in zip(F, labels)])
        lo, hi, nonfin = pr.finite_range(vals)
        assert (float(res["range"][g, 0]), float(res["range"][g, 1])) == (float(lo), float(hi))
        sf, ao = pr.for_range(lo, hi)
        assert (res["packing"][g].scale_factor, res["packing"][g].add_offset) == (sf, ao)
        assert int(res["filled"][g]) == nonfin == (Ct.shape[0] if g == 0 else 0)
        assert int(res["saturated"][g]) == 0
        for f, lab, Q in zip(F, labels, res["codes"]):
            assert Q.dtype == torch.int16 and tuple(Q.shape) == f.shape
            assert np.array_equal(Q.numpy()[:, lab == g], pr.encode(np.ascontiguousarray(f[:, lab == g]), sf, ao)[0])
    assert bool((res["codes"][1][:, 3] == pr.FILL).all())


@pytest.mark.parametrize("provider", PROVIDERS)
def test_pack_blocks_with_a_given_packing_and_out_views(provider):
    from dmd_era5_amd.forecast import pack_blocks

    kern = provider()
    U, means, stds, Ct, labels = _blocks_case(seed=4)
    F = _fields(kern, U, means, stds, Ct)
    given = [_packing(1e-3, 0.0), _packing(2e-3, 20.0), _packing(1e-4, 40.0), _packing(5e-3, 55.0)]   # group 2: too narrow
    T, M = Ct.shape[0], sum(u.shape[1] for u in U)
    slab = torch.full((T + 2, M + 3), 777, dtype=torch.int16)
    edges = np.concatenate([[0], np.cumsum([u.shape[1] for u in U])])
    out = [slab[1:T + 1, 1 + a:1 + b] for a, b in zip(edges[:-1], edges[1:])]
    res = pack_blocks([_t(u) for u in U], _t(Ct), [_t(v) for v in means], [_t(v) for v in stds],
                      groups=[_t(lab, torch.int64) for lab in labels], packing=given, out=out, kern=kern)
    assert res["range"] is None and res["packing"] == given
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(res["codes"], out))
    sat = [0, 0, 0, 0]
    for f, lab, Q in zip(F, labels, out):
        for g in range(4):
            q, filled, s = pr.encode(np.ascontiguousarray(f[:, lab == g]), given[g].scale_factor, given[g].add_offset)
            assert np.array_equal(Q.numpy()[:, lab == g], q) and filled == 0
            sat[g] += s
    assert res["saturated"].tolist() == sat and sat[2] > 0 and res["filled"].tolist() == [0, 0, 0, 0]
    assert set(np.unique(np.concatenate([Q.numpy()[:, lab == 2].ravel() for Q, lab in zip(out, labels)]))) >= {-32767, 32767}
    inner = torch.zeros_like(slab, dtype=torch.bool)
    inner[1:T + 1, 1:1 + M] = True
    assert bool((slab[~inner] == 777).all())
    # one packing for everything, no groups; counts handed back in keep running sums
    tiny = _packing(1e-5, 0.0)
    one = pack_blocks([_t(u) for u in U], _t(Ct), kern=kern, packing=tiny)
    two = pack_blocks([_t(u) for u in U], _t(Ct), kern=kern, packing=tiny, counts=one["counts"])
    assert len(one["packing"]) == 1 and int(one["saturated"][0]) > 0
    assert two["saturated"].tolist() == [2 * int(one["saturated"][0])]
    with pytest.raises(ValueError):
        pack_blocks([_t(u) for u in U], _t(Ct), groups=[_t(lab, torch.int64) for lab in labels], packing=given[:3], kern=kern)
    with pytest.raises(ValueError):
        pack_blocks([_t(u) for u in U], _t(Ct), groups=[_t(lab[:-1], torch.int64) for lab in labels], kern=kern)


def test_pack_blocks_of_a_delay_embedded_basis_and_an_all_missing_group():
    from dmd_era5_amd.forecast import pack_blocks

    kern = DoubleWithPack()
    rs = np.random.RandomState(5)
    k, mb, d, T = 4, 7, 3, 6
    U = rs.standard_normal((k, d * mb)).astype(np.float32)
    mean = rs.standard_normal(mb).astype(np.float32)
    mean[4:] = np.nan                                                   # group 1: nothing finite
    Ct = rs.standard_normal((T, k)).astype(np.float32)
    lab = np.array([0] * 4 + [1] * 3)
    res = pack_blocks([_t(U)], _t(Ct), [_t(mean)], None, groups=[_t(lab, torch.int64)], delay=d, kern=kern)
    F = kern.expand(_t(U[:, :mb]), _t(Ct), _t(mean)).numpy()
    assert tuple(res["codes"][0].shape) == (T, mb)
    sf, ao = pr.for_range(*pr.finite_range(F[:, :4])[:2])
    assert np.array_equal(res["codes"][0].numpy()[:, :4], pr.encode(np.ascontiguousarray(F[:, :4]), sf, ao)[0])
    assert bool((res["codes"][0][:, 4:] == pr.FILL).all())
    assert res["range"][1].tolist() == [np.inf, -np.inf]
    assert (res["packing"][1].scale_factor, res["packing"][1].add_offset) == (1.0, 0.0)
    assert res["filled"].tolist() == [0, 3 * T]
    # all d * mb rows of the embedding: the labels repeat per delay
    full = pack_blocks([_t(U)], _t(Ct), [_t(mean)], None, groups=[_t(lab, torch.int64)], delay=d, delay_block=None, kern=kern)
    assert tuple(full["codes"][0].shape) == (T, d * mb) and full["filled"].tolist() == [0, 3 * d * T]


def test_pack_blocks_refuses_the_range_pass_over_several_ranks():
    from dmd_era5_amd.forecast import pack_blocks
    from dmd_era5_amd.svd import Comm

    class TwoRanks(Comm):
        world_size = 2

    U, means, stds, Ct, labels = _blocks_case()
    with pytest.raises(ValueError, match="packing"):
        pack_blocks([_t(u) for u in U], _t(Ct), kern=DoubleWithPack(), comm=TwoRanks())
    res = pack_blocks([_t(u) for u in U], _t(Ct), kern=DoubleWithPack(), comm=TwoRanks(), packing=_packing(1e-3, 0.0))
    assert len(res["codes"]) == 3


def test_pack_field_blocks_equals_the_reference():
    from dmd_era5_amd.forecast import pack_field_blocks

    rs = np.random.RandomState(6)
    X = [rs.standard_normal((8, m)).astype(np.float32) for m in (11, 6)]
    X[0][2, 3] = np.inf
    labels = [np.array([0] * 5 + [1] * 6), np.array([1] * 6)]
    for kern in (DoubleWithExpand(), DoubleWithPack()):
        res = pack_field_blocks([_t(x) for x in X], [_t(lab, torch.int64) for lab in labels], kern=kern)
        for g in range(2):
            vals = np.concatenate([x[:, lab == g].ravel() for x, lab in zip(X, labels)])
            sf, ao = pr.for_range(*pr.finite_range(vals)[:2])
            for x, lab, Q in zip(X, labels, res["codes"]):
                assert np.array_equal(Q.numpy()[:, lab == g], pr.encode(np.ascontiguousarray(x[:, lab == g]), sf, ao)[0])
        assert res["filled"].tolist() == [1, 0] and res["saturated"].tolist() == [0, 0]


# ---------------------------------------------------------------- the writer
needs_hdf5 = pytest.mark.skipif(not __import__("dmd_era5_amd.hdf5_lite", fromlist=["x"]).available(),
                                reason="libhdf5 not found")


@needs_hdf5
def test_slabs_written_out_of_order_give_the_file_of_dataset(tmp_path):
    from dmd_era5_amd import hdf5_lite

    rs = np.random.RandomState(7)
    A = rs.randint(-32768, 32768, (11, 2, 5, 7)).astype(np.int16)
    B = rs.standard_normal((11, 3)).astype(np.float32)
    dims, attrs = ("time", "level", "latitude", "longitude"), {"scale_factor": np.float64(0.5), "_FillValue": np.int16(-32768)}
    coords = [("time", np.arange(11, dtype=np.int64)), ("level", np.array([1000, 850])), ("latitude", np.linspace(60, 40, 5)),
              ("longitude", np.linspace(0, 30, 7))]

    def write(path, slabbed):
        with hdf5_lite.Writer(path) as w:
            for name, vals in coords:
                w.dataset(name, vals, (name,))
            if slabbed:
                w.create("a", A.shape, np.int16, dims, attrs)
                w.create("b", B.shape, np.float32, ("time", "member"))
                for t0, t1 in ((7, 11), (0, 3), (3, 7)):
                    w.write_slab("a", t0, A[t0:t1])
                w.write_slab("b", 5, B[5:])
                w.write_slab("b", 0, B[:5])
                with pytest.raises(ValueError):
                    w.write_slab("a", 9, A[:3])                        # past the end
                with pytest.raises(ValueError):
                    w.write_slab("a", 0, A[:3].astype(np.int32))       # another dtype
                with pytest.raises(KeyError):
                    w.write_slab("time", 0, np.arange(2))              # not made by create()
            else:
                w.dataset("a", A, dims, attrs)
                w.dataset("b", B, ("time", "member"))
            w.attrs(None, {"variables": ["a", "b"], "_NCProperties": "version=2,test=1"})
        return path

    p1, p2 = write(str(tmp_path / "whole.nc"), False), write(str(tmp_path / "slabs.nc"), True)
    r1, r2 = hdf5_lite.Reader(p1), hdf5_lite.Reader(p2)
    assert r1.variables == r2.variables
    for name in r1.variables:
        assert np.array_equal(r1.read(name), r2.read(name)), name
        a1, a2 = r1.attrs(name), r2.attrs(name)
        assert sorted(a1) == sorted(a2) and all(np.array_equal(a1[k], a2[k]) for k in a1), name
    assert np.array_equal(r2.read("a"), A) and np.array_equal(r2.read_slab("a", 2, 9), A[2:9])
    r1.close()
    r2.close()
    assert open(p1, "rb").read() == open(p2, "rb").read()             # the same file, byte for byte


def _mock_forecast(nvar=2, nlev=2, nlat=6, nlon=7, k=6, delay=1, seed=8, trials=0):
    """A DmdForecast on the CPU with a planted real model, two row blocks that cut through a variable."""
    from dmd_era5_amd.bopdmd import OptDMDResult
    from dmd_era5_amd.forecast import DmdForecast

    rs = np.random.RandomState(seed)
    M = nvar * nlev * nlat * nlon
    half = np.array([-0.05 + 1.0j, -0.2 + 2.5j, -0.01 + 0.4j])

    def result(jitter):
        h = half * (1 + jitter * rs.standard_normal(3))
        mh = rs.standard_normal((k, 3)) + 1j * rs.standard_normal((k, 3))
        return OptDMDResult(eigs=torch.from_numpy(np.concatenate([h, h.conj()])),
                            modes=torch.from_numpy(np.concatenate([mh, mh.conj()], axis=1)),
                            amplitudes=torch.from_numpy(np.ones(6)), rel_error=0.0, n_iter=0, converged=True)

    res = result(0.0)
    if trials:
        res.trials = [result(0.02) for _ in range(trials)]
    Q = np.linalg.qr(rs.standard_normal((delay * M, k)))[0].astype(np.float32)
    cut = M // 2 + 5
    mean = (250.0 + 30.0 * rs.rand(M)).astype(np.float32)
    mean[M // 2:] = (rs.rand(M - M // 2) * 20 - 10).astype(np.float32)         # the second variable: a wind
    std = (1.0 + rs.rand(M)).astype(np.float32)
    Ub = []
    for a, b in ((0, cut), (cut, M)):
        Ub.append(_t(np.concatenate([Q[j * M + a:j * M + b] for j in range(delay)]).T))
    return DmdForecast(Ub, res, means=[_t(mean[:cut]), _t(mean[cut:])], stds=[_t(std[:cut]), _t(std[cut:])], delay=delay,
                       kern=DoubleWithPack())


GRID = dict(levels=[1000, 850], latitude=np.arange(50, 20, -5.0), longitude=np.arange(0, 35, 5.0))
NAMES = ["temperature", "u_component_of_wind"]


def _times(T):
    return np.datetime64("2019-01-01T00", "ns") + np.arange(T) * np.timedelta64(1, "h")


@needs_hdf5
@pytest.mark.parametrize("delay,slab", [(1, None), (2, 4)])
def test_write_forecast_slice_reads_back_within_half_a_step(tmp_path, monkeypatch, delay, slab):
    from dmd_era5_amd import era5_svd, io_netcdf

    monkeypatch.setenv("DMDX_NETCDF_BACKEND", "hdf5")
    f = _mock_forecast(delay=delay)
    T = 13
    t = np.linspace(0.0, 3.0, T)
    path = str(tmp_path / "forecast.nc")
    res = era5_svd.write_forecast_slice(path, f, t, _times(T), NAMES, **GRID, slab=slab, attrs={"experiment": "k17"})
    F = torch.cat(f.fields(torch.from_numpy(t)), dim=1).numpy()                  # (T, M): variable, level, lat, lon
    ds = io_netcdf.open_dataset(path)
    assert sorted(ds.data_vars) == sorted(NAMES)
    assert np.array_equal(ds.coords["time"].values, _times(T)) and np.array_equal(ds.coords["level"].values, GRID["levels"])
    assert ds.attrs["forecast_rank"] == 6 and ds.attrs["forecast_delay"] == delay and ds.attrs["experiment"] == "k17"
    plane = 2 * 6 * 7
    r = hdf5_lite_reader(path)
    for g, name in enumerate(NAMES):
        want = F[:, g * plane:(g + 1) * plane].reshape(T, 2, 6, 7)
        pk = res["packing"][name]
        sf, ao = pr.for_range(*pr.finite_range(want)[:2])
        assert (pk.scale_factor, pk.add_offset) == (sf, ao) and res["filled"][name] == 0 and res["saturated"][name] == 0
        enc = ds[name].encoding                                                   # the packing was recognised
        assert float(enc["scale_factor"]) == sf and float(enc["add_offset"]) == ao and int(enc["_FillValue"]) == -32768
        codes = r.read(name)
        assert codes.dtype == np.int16 and np.array_equal(codes, pr.encode(np.ascontiguousarray(want), sf, ao)[0])
        assert codes.min() == -32767 and codes.max() == 32767
        got = np.asarray(ds[name].values)
        assert got.dtype == np.float32 and ds[name].dims == ("time", "level", "latitude", "longitude")
        assert (np.abs(got.astype(np.float64) - want) <= sf / 2 + pr.ulp32(want)).all()
    r.close()


def hdf5_lite_reader(path):
    from dmd_era5_amd import hdf5_lite

    return hdf5_lite.Reader(path)


@needs_hdf5
def test_write_forecast_slice_with_a_given_packing_ensemble_and_spread(tmp_path, monkeypatch):
    from dmd_era5_amd import era5_svd, io_netcdf
    from dmd_era5_amd.labeled import Packing

    monkeypatch.setenv("DMDX_NETCDF_BACKEND", "hdf5")
    f = _mock_forecast(trials=4)
    T = 7
    t = np.linspace(0.0, 2.0, T)
    given = {"temperature": Packing(0.002, 270.0, (-32768,)), "u_component_of_wind": Packing(1e-5, 0.0, (-32768,))}
    path = str(tmp_path / "ens.nc")
    res = era5_svd.write_forecast_slice(path, f, t, _times(T), NAMES, **GRID, packing=given, ensemble=True, spread=True,
                                        slab=3)
    mean, spread = f.ensemble_fields(torch.from_numpy(t))
    mean, spread = torch.cat(mean, dim=1).numpy(), torch.cat(spread, dim=1).numpy()
    ds = io_netcdf.open_dataset(path)
    assert sorted(ds.data_vars) == sorted(NAMES + [n + "_spread" for n in NAMES])
    r, plane = hdf5_lite_reader(path), 2 * 6 * 7
    for g, name in enumerate(NAMES):
        want = np.ascontiguousarray(mean[:, g * plane:(g + 1) * plane]).reshape(T, 2, 6, 7)
        q, filled, sat = pr.encode(want, given[name].scale_factor, given[name].add_offset)
        assert np.array_equal(r.read(name), q) and (res["filled"][name], res["saturated"][name]) == (filled, sat)
        assert res["packing"][name] is given[name]
        sp = np.ascontiguousarray(spread[:, g * plane:(g + 1) * plane]).reshape(T, 2, 6, 7)
        sf, ao = pr.for_range(*pr.finite_range(sp)[:2])
        pk = res["packing"][name + "_spread"]
        assert (pk.scale_factor, pk.add_offset) == (sf, ao)
        assert np.array_equal(r.read(name + "_spread"), pr.encode(sp, sf, ao)[0])
    assert res["saturated"]["u_component_of_wind"] > 0 and res["saturated"]["temperature"] == 0
    r.close()
    with pytest.raises(ValueError):
        era5_svd.write_forecast_slice(path, f, t, _times(T), NAMES, **GRID, spread=True)
    with pytest.raises(ValueError):
        era5_svd.write_forecast_slice(path, f, t, _times(T), NAMES + ["x"], **GRID)


@needs_hdf5
def test_a_written_forecast_is_an_input_slice_of_main(svd_base_config, project_root, monkeypatch):
    """retrieve_era5_slice's attribute check accepts the file, and main() -- its device pipeline handed the kernel
    double, as tests/test_forecast.py runs it -- decomposes it: the singular values are those of the decoded
    fields."""
    from dmd_era5_amd import era5_svd
    from dmd_era5_amd.config_parser import config_parser

    monkeypatch.setenv("DMDX_NETCDF_BACKEND", "hdf5")
    K = DoubleWithPack()
    pipeline = era5_svd._device_pipeline
    monkeypatch.setattr(era5_svd, "_device_pipeline",
                        lambda ds, cfg, comm: pipeline(ds, cfg, comm, kern=K, device=torch.device("cpu")))
    T = 13
    cfg = dict(svd_base_config, start_datetime="2019-01-01T00", end_datetime="2019-01-01T12",
               variables="temperature,u_component_of_wind", levels="1000,850", svd_type="standard", mean_center=True,
               scale=False, delay_embedding=1, n_components=4, save_data_matrix=True, svd_seed=0)
    p = config_parser(cfg, "era5-svd")
    f = _mock_forecast()
    t = np.linspace(0.0, 3.0, T)
    era5_svd.write_forecast_slice(p["era5_slice_path"], f, t, _times(T), p["variables"], **GRID,
                                  attrs={"source_path": p["source_path"]})
    ds, _ = era5_svd.retrieve_era5_slice(p)
    assert ds is not None
    assert era5_svd.retrieve_era5_slice(dict(p, source_path="elsewhere"))[0] is None
    out, _, _ = era5_svd.main(cfg, write_to_netcdf=False)
    X = np.concatenate([np.asarray(ds[n].values).reshape(T, -1) for n in p["variables"]], axis=1).T.astype(np.float64)
    s = np.linalg.svd(X - X.mean(axis=1, keepdims=True), compute_uv=False)[:4]
    assert np.allclose(np.asarray(out["s"].values), s, rtol=1e-4)
    assert np.asarray(out["U"].values).shape == (X.shape[0], 4)


def test_dmd_forecast_pack_mean_and_spread():
    """DmdForecast.pack: the model, the ensemble mean, and with spread=True the K15 spread of the same times."""
    f = _mock_forecast(trials=4, delay=2)
    t = torch.from_numpy(np.linspace(0.0, 2.0, 5))
    plane = 2 * 6 * 7
    cut = plane + 5
    groups = [_t(np.arange(0, cut) // plane, torch.int64), _t(np.arange(cut, 2 * plane) // plane, torch.int64)]
    res = f.pack(t, groups=groups)
    F = torch.cat(f.fields(t), dim=1).numpy()
    got = torch.cat(res["codes"], dim=1).numpy()
    for g in range(2):
        sf, ao = pr.for_range(*pr.finite_range(F[:, g * plane:(g + 1) * plane])[:2])
        assert np.array_equal(got[:, g * plane:(g + 1) * plane], pr.encode(np.ascontiguousarray(F[:, g * plane:(g + 1) * plane]), sf, ao)[0])
    assert res["imag_ratio"] < 1e-12
    ens = f.pack(t, groups=groups, ensemble=True, spread=True)
    mean, spread = f.ensemble_fields(t)
    for key, fld in ((None, mean), ("spread", spread)):
        r = ens if key is None else ens[key]
        X = torch.cat(fld, dim=1).numpy()
        Q = torch.cat(r["codes"], dim=1).numpy()
        for g in range(2):
            x = np.ascontiguousarray(X[:, g * plane:(g + 1) * plane])
            pk = r["packing"][g]
            assert (pk.scale_factor, pk.add_offset) == pr.for_range(*pr.finite_range(x)[:2])
            assert np.array_equal(Q[:, g * plane:(g + 1) * plane], pr.encode(x, pk.scale_factor, pk.add_offset)[0])
    with pytest.raises(ValueError):
        f.pack(t, spread=True)
