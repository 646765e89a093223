"""Host side of K29 without a GPU: tests/pstat_ref.py (the definition the kernel is held to) against hand-made series
with hand-computed values and against its own piece-and-merge restatement, and extremes.snapshots_per_day /
period_stat_blocks / PeriodStats on the kernel double pstat_ref.PstatDouble.  Integer-valued planes and extremes compare
exactly, sums bit for bit, NaN with equal_nan."""
import numpy as np
import pytest
import torch

import pstat_ref as pr
from pstat_ref import PstatDouble
from test_crps import TwoRanks
from test_trend import TrendDouble

N, MAX, ARGMAX, MIN, ARGMIN, TOTAL, ETOTAL, ECOUNT = range(8)
NAN, INF = float("nan"), float("inf")


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def _x(*v):
    return np.array([v], dtype=np.float32)


def _col(Q, p=0, i=0):
    return Q[:, p, i].tolist()


def _same(a, b):
    """Bit for bit, NaN equal to NaN (the payloads of the NaN are not part of the contract)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


# ---------------------------------------------------------------- the reference itself
def test_a_tie_of_two_maxima_keeps_the_first_and_the_threshold_picks_its_days():
    Q = pr.period_stats(_x(1, 3, 2, 3, 0), [0, 5], thr=np.array([2.0], dtype=np.float32))
    assert Q.shape == (8, 1, 1) and Q.dtype == np.float64
    assert _col(Q) == [5.0, 3.0, 1.0, 0.0, 4.0, 9.0, 6.0, 2.0]
    Q = pr.period_stats(_x(0, 3, 0, 3, 0), [0, 5])
    assert _col(Q) == [5.0, 3.0, 1.0, 0.0, 0.0, 6.0, 0.0, 0.0]                 # ... and the first of three minima


def test_minus_zero_then_plus_zero_stays_minus_zero():
    # inside a day: hi and lo are replaced on a strict comparison only
    hi = pr.period_stats(_x(-0.0, 0.0), [0, 2], group=2, inner="max")
    lo = pr.period_stats(_x(0.0, -0.0), [0, 2], group=2, inner="min")
    assert hi[MAX, 0, 0] == 0 and np.signbit(hi[MAX, 0, 0]) and lo[MIN, 0, 0] == 0 and not np.signbit(lo[MIN, 0, 0])
    # between days: the first running value stays the extreme
    Q = pr.period_stats(_x(-0.0, 0.0), [0, 2], inner="max")
    assert np.signbit(Q[MAX, 0, 0]) and np.signbit(Q[MIN, 0, 0]) and _col(Q)[ARGMAX] == 0.0 and _col(Q)[ARGMIN] == 0.0
    assert Q[TOTAL, 0, 0] == 0 and not np.signbit(Q[TOTAL, 0, 0])                                # +0.0 + -0.0
    Q = pr.period_stats(_x(-0.0, -0.0), [0, 2], inner="min")
    assert not np.signbit(Q[TOTAL, 0, 0]) and np.signbit(Q[MAX, 0, 0])       # the sums start from +0.0, the extremes do not


def test_a_period_without_a_valid_day():
    Q = pr.period_stats(_x(NAN, INF, -INF, 5), [0, 3, 4], thr=np.array([0.0], dtype=np.float32))
    assert _same(Q[:, 0, 0], [0.0, NAN, -1.0, NAN, -1.0, 0.0, 0.0, 0.0])
    assert not np.signbit(Q[TOTAL, 0, 0]) and not np.signbit(Q[ETOTAL, 0, 0])
    assert _col(Q, 1) == [1.0, 5.0, 0.0, 5.0, 0.0, 5.0, 5.0, 1.0]


def test_a_ragged_last_day_at_min_count_and_below_it():
    X = _x(1, 2, 3, 4, 5, 6, 7, 8)                                            # days of 3: 6, 15 and the ragged 7 + 8
    assert _col(pr.period_stats(X, [0, 8], group=3))[:6] == [2.0, 15.0, 1.0, 6.0, 0.0, 21.0]          # min_count = g
    assert _col(pr.period_stats(X, [0, 8], group=3, min_count=3))[:6] == [2.0, 15.0, 1.0, 6.0, 0.0, 21.0]
    assert _col(pr.period_stats(X, [0, 8], group=3, min_count=2))[:6] == [3.0, 15.0, 1.0, 6.0, 0.0, 36.0]
    assert _col(pr.period_stats(X, [0, 7], group=3, min_count=2))[:6] == [2.0, 15.0, 1.0, 6.0, 0.0, 21.0]  # one snapshot
    assert _col(pr.period_stats(X, [0, 7], group=3, min_count=1))[:6] == [3.0, 15.0, 1.0, 6.0, 0.0, 28.0]
    assert _col(pr.period_stats(X, [0, 8], group=3, inner="mean", min_count=2))[:6] == [3.0, 7.5, 2.0, 2.0, 0.0, 14.5]
    assert _col(pr.period_stats(X, [0, 8], group=3, inner="range", min_count=2))[:6] == [3.0, 2.0, 0.0, 1.0, 2.0, 5.0]


def test_a_window_does_not_cross_a_period_boundary():
    X = _x(1, 2, 3, 4, 5, 6, 7, 8)
    Q = pr.period_stats(X, [0, 4, 8], window=3)
    assert _col(Q, 0)[:6] == [2.0, 9.0, 3.0, 6.0, 2.0, 15.0]
    assert _col(Q, 1)[:6] == [2.0, 21.0, 3.0, 18.0, 2.0, 39.0]               # no window holds 3 + 4 + 5 or 4 + 5 + 6
    assert _col(pr.period_stats(X, [0, 8], window=3))[:6] == [6.0, 21.0, 7.0, 6.0, 2.0, 81.0]
    assert _same(pr.period_stats(X, [0, 2, 8], window=3)[:6, 0, 0], [0.0, NAN, -1.0, NAN, -1.0, 0.0])   # shorter than w
    # snapshots outside [b_0, b_P) are not read
    Xn = np.concatenate([[NAN, 9.0], X[0], [9.0, NAN]]).astype(np.float32)[None]
    assert _same(pr.period_stats(Xn, [2, 6, 10], window=3), Q)


def test_nan_and_inf_are_missing():
    X = _x(1, NAN, INF, -INF, 3, 4)
    assert _col(pr.period_stats(X, [0, 6], group=2, min_count=1))[:6] == [2.0, 7.0, 2.0, 1.0, 0.0, 8.0]
    assert _col(pr.period_stats(X, [0, 6], group=2))[:6] == [1.0, 7.0, 2.0, 7.0, 2.0, 7.0]             # min_count = 2
    assert _col(pr.period_stats(X, [0, 6], group=2, min_count=1, window=2))[0] == 0.0                # day 1 breaks both
    assert _col(pr.period_stats(X, [0, 6], group=2, min_count=1, inner="range"))[:6] == [2.0, 1.0, 2.0, 0.0, 0.0, 1.0]
    assert _col(pr.period_stats(X, [0, 6], group=2, min_count=1, inner="mean"))[:6] == [2.0, 3.5, 2.0, 1.0, 0.0, 4.5]
    assert _col(pr.period_stats(X, [0, 6], group=6, min_count=3, inner="min"))[:6] == [1.0, 1.0, 0.0, 1.0, 0.0, 1.0]
    assert _col(pr.period_stats(X, [0, 6], group=6, min_count=4, inner="min"))[0] == 0.0


def test_thresholds_nan_infinite_and_all_four_comparisons_on_an_exact_tie():
    X = _x(1, 2, 3)
    th = lambda v: np.array([v], dtype=np.float32)
    ev = lambda **kw: _col(pr.period_stats(X, [0, 3], **kw))[ETOTAL:]
    assert ev(thr=th(2.0)) == [3.0, 1.0] and ev(thr=th(2.0), inclusive=True) == [5.0, 2.0]
    assert ev(thr=th(2.0), below=True) == [1.0, 1.0] and ev(thr=th(2.0), below=True, inclusive=True) == [3.0, 2.0]
    for kw in (dict(), dict(below=True), dict(inclusive=True), dict(below=True, inclusive=True)):
        assert ev(thr=th(NAN), **kw) == [0.0, 0.0] and ev(thr=None, **kw) == [0.0, 0.0]
    assert ev(thr=th(INF)) == [0.0, 0.0] and ev(thr=th(INF), below=True) == [6.0, 3.0]              # a threshold like any
    assert ev(thr=th(-INF)) == [6.0, 3.0] and ev(thr=th(-INF), below=True, inclusive=True) == [0.0, 0.0]
    # the threshold is compared with the RUNNING value
    assert _col(pr.period_stats(X, [0, 3], window=2, thr=th(4.0)))[ETOTAL:] == [5.0, 1.0]


def test_the_partition_is_part_of_the_totals_and_of_nothing_else():
    big = 2.0 ** 53
    X = _x(big, 1, 1, -big)
    tot = lambda seg: pr.period_stats(X, [0, 4], seg=seg, thr=np.array([-INF], dtype=np.float32))
    assert _col(tot(4))[TOTAL:] == [0.0, 0.0, 4.0] and _col(tot(1))[TOTAL:] == [0.0, 0.0, 4.0]
    assert _col(tot(2))[TOTAL:] == [1.0, 1.0, 4.0]               # (2^53 + 1) + (1 - 2^53): the second piece is exact
    assert _same(tot(2)[:TOTAL], tot(4)[:TOTAL])


def _random_case(rs):
    m, T = int(rs.randint(1, 4)), int(rs.randint(1, 60))
    X = (rs.standard_normal((m, T)) * np.exp2(rs.randint(-30, 31, (m, T)))).astype(np.float32)
    X[rs.rand(m, T) < 0.08] = np.nan
    thr = rs.standard_normal(m).astype(np.float32)
    thr[rs.rand(m) < 0.1] = np.nan
    cuts = np.sort(rs.choice(np.arange(T + 1), size=min(T + 1, int(rs.randint(2, 5))), replace=False))
    g = int(rs.randint(1, 5))
    return X, cuts, dict(group=g, inner=pr.INNER[rs.randint(0, 5)], window=int(rs.randint(1, 9)),
                         min_count=int(rs.randint(1, g + 1)), thr=thr if rs.rand() < 0.8 else None,
                         below=bool(rs.randint(0, 2)), inclusive=bool(rs.randint(0, 2)))


def test_reference_equals_its_piece_and_merge_restatement_for_seg_1_2_7():
    """Every piece scanned on its own after the w - 1 days before it, the records merged in order, against the plain
    loop: 300 random cases with exponents spread over 60 bits (so that a sum formed in another order shows), each
    with seg in {1, 2, 7}."""
    rs = np.random.RandomState(29)
    windows_across, differ = 0, 0
    for case in range(300):
        X, bounds, kw = _random_case(rs)
        want = {seg: pr.period_stats(X, bounds, seg=seg, **kw) for seg in (1, 2, 7)}
        for seg in (1, 2, 7):
            assert _same(pr.period_stats_by_pieces(X, bounds, seg=seg, **kw), want[seg]), (case, seg)
        windows_across += int(kw["window"] > 1 and want[2][N].max() > 2)
        differ += int(not _same(want[2][TOTAL], want[7][TOTAL]))
        assert _same(np.delete(want[2], [TOTAL, ETOTAL], 0), np.delete(want[7], [TOTAL, ETOTAL], 0)), case
    assert windows_across > 30 and differ > 30             # windows do cross piece boundaries, and the partition shows


def test_n_pieces():
    b = [2, 9, 10, 50, 93]
    assert pr.n_pieces(b, 1, 1) == 91 and pr.n_pieces(b, 3, 2) == 18 and pr.n_pieces(b, 24, 1) == 6 and pr.n_pieces(b, 4, 7) == 6


# ---------------------------------------------------------------- snapshots_per_day
def test_snapshots_per_day():
    from dmd_era5_amd.extremes import snapshots_per_day

    h = np.datetime64("2020-02-28T00", "h") + np.arange(72) * np.timedelta64(1, "h")
    assert snapshots_per_day(h) == 24 and snapshots_per_day(h[::6]) == 4 and snapshots_per_day(h[::24]) == 1
    assert snapshots_per_day(h[::3].astype("datetime64[ns]")) == 8
    assert snapshots_per_day(np.datetime64("2020-01-01T00:00", "m") + np.arange(5) * np.timedelta64(30, "m")) == 48
    with pytest.raises(ValueError, match="constant step"):
        snapshots_per_day(h[[0, 1, 3, 4]])
    with pytest.raises(ValueError, match="constant step"):
        snapshots_per_day(h[::-1])
    with pytest.raises(ValueError, match="does not divide a day"):
        snapshots_per_day(h[::5])
    with pytest.raises(ValueError, match="does not divide a day"):
        snapshots_per_day(h[::48])
    with pytest.raises(ValueError, match="at least two"):
        snapshots_per_day(h[:1])
    with pytest.raises(ValueError, match="datetime64"):
        snapshots_per_day(np.arange(8))


# ---------------------------------------------------------------- PeriodStats on the double
def _known_blocks():
    """12-hourly stamps from 2020-12-30 to 2021-01-02: two days in each year.  Row 1 is missing in 2020."""
    times = np.datetime64("2020-12-30T00", "h") + np.arange(8) * np.timedelta64(12, "h")
    rows = [[1, 3, 2, 5, 4, 4, 0, 1], [NAN, NAN, NAN, NAN, 2, 2, 2, 2], [0, 0, 0, 0, 10, 0, 0, 7]]
    X = np.array(rows, dtype=np.float32).T                                   # (T, 3)
    return times, [X[:, :2].copy(), X[:, 2:].copy()]


def _cat(blocks):
    return np.concatenate([np.asarray(b) for b in blocks], axis=1)          # (P, 3 rows)


def test_periodstats_accessors_on_series_with_known_answers():
    from dmd_era5_amd.extremes import PeriodStats, snapshots_per_day

    times, X = _known_blocks()
    g = snapshots_per_day(times)
    assert g == 2
    PstatDouble.pstat_calls = 0
    st = PeriodStats.fit([_t(x) for x in X], times, group=g, inner="max", threshold=3.5, kern=PstatDouble())
    assert PstatDouble.pstat_calls == 2 and st.planes[0].shape == (8, 2, 2) and st.planes[0].dtype == torch.float64
    assert st.bounds.tolist() == [0, 4, 8] and st.labels.tolist() == ["2020", "2021"] and st.n_periods == 2
    assert (st.group, st.inner, st.window, st.min_count, st.below, st.inclusive, st.has_threshold) == (2, "max", 1, 2, False,
                                                                                                      False, True)
    assert st.period_days().tolist() == [2, 2]
    assert _cat(st.n_valid()).tolist() == [[2, 0, 2], [2, 2, 2]]
    assert _same(_cat(st.maximum()), [[5, NAN, 0], [4, 2, 10]]) and _same(_cat(st.minimum()), [[3, NAN, 0], [1, 2, 7]])
    assert _cat(st.total()).tolist() == [[8, 0, 0], [5, 4, 17]]
    assert _cat(st.total_beyond()).tolist() == [[5, 0, 0], [4, 0, 17]] and _cat(st.count_beyond()).tolist() == [[1, 0, 0], [1, 0, 2]]
    assert _same(_cat(st.mean()), [[4, NAN, 0], [2.5, 2, 8.5]])
    assert _same(_cat(st.intensity()), [[5, NAN, NAN], [4, NAN, 8.5]])
    assert _same(_cat(st.fraction_beyond()), [[0.625, NAN, NAN], [0.8, 0.0, 1.0]])
    wm, wn = _cat(st.when_max()), _cat(st.when_min())
    assert wm.dtype == np.int64 and wm.tolist() == [[1, -1, 0], [0, 0, 0]] and wn.tolist() == [[0, -1, 0], [1, 0, 1]]
    when = _cat(st.when_max(as_time=True))
    assert when.dtype == np.dtype("datetime64[ns]") and when[0, 0] == np.datetime64("2020-12-31T00") and np.isnat(when[0, 1])
    assert when[1, 2] == np.datetime64("2021-01-01T00") and _cat(st.when_min(as_time=True))[1, 2] == np.datetime64("2021-01-02T00")
    # per-block threshold tables, below and inclusive
    tabs = [_t(np.array([3.0, 2.0])), _t(np.array([NAN]))]
    lo = PeriodStats.fit([_t(x) for x in X], times, group=g, inner="max", threshold=tabs, below=True, inclusive=True,
                         kern=PstatDouble())
    assert _cat(lo.count_beyond()).tolist() == [[1, 0, 0], [1, 2, 0]] and _cat(lo.total_beyond()).tolist() == [[3, 0, 0], [1, 4, 0]]
    # a window, min_count below the group, one period over everything given as bounds: no times needed
    plain = PeriodStats.fit([_t(x) for x in X], None, period=[0, 8], group=2, inner="sum", window=2, min_count=1,
                            kern=PstatDouble())
    assert plain.labels.tolist() == ["0"] and not plain.has_threshold
    assert _same(_cat(plain.maximum()), [[15, 8, 17]]) and _cat(plain.n_valid()).tolist() == [[3, 1, 3]]
    assert _cat(plain.when_max()).tolist() == [[2, 3, 3]]
    with pytest.raises(ValueError, match="only the offsets"):
        plain.when_max(as_time=True)


def test_series_goes_into_trend_fit_as_it_is():
    from dmd_era5_amd.extremes import PeriodStats
    from dmd_era5_amd.trend import Trend

    X = np.array([[1, 1, 2, 2, 3, 3], [5, 0, 3, 0, 1, 0], [NAN, NAN, 1, 1, 1, 1]], dtype=np.float32).T
    st = PeriodStats.fit([_t(X[:, :2]), _t(X[:, 2:])], None, period=[0, 2, 4, 6], kern=PstatDouble())
    ser = st.series("total")
    assert [tuple(s.shape) for s in ser] == [(3, 2), (3, 1)] and all(s.dtype == torch.float32 and s.is_contiguous() for s in ser)
    assert torch.cat(ser, dim=1).tolist() == [[2, 5, 0], [4, 3, 2], [6, 1, 2]]
    years = np.array(["2020-07-01", "2021-07-01", "2022-07-01"], dtype="datetime64[D]")
    trend = Trend.fit(ser, years, degree=1, kern=TrendDouble())
    slope = torch.cat(trend.slope(per_days=365.0)).numpy()
    assert np.allclose(slope, [2.0, -2.0, 1.0], rtol=1e-6, atol=1e-6)
    assert torch.cat(st.series("when_max"), dim=1).tolist() == [[0, 0, -1], [0, 0, 0], [0, 0, 0]]
    assert np.isnan(st.series("maximum")[1][0, 0].item())
    with pytest.raises(ValueError, match="index"):
        st.series("median")


def _grid():
    times, X = _known_blocks()
    w = [np.array([1.0, 2.0], dtype=np.float32), np.array([3.0], dtype=np.float32)]
    lab = [np.array([0, 1]), np.array([1])]
    return times, X, w, lab


def test_area_mean_leaves_out_rows_without_a_value():
    from dmd_era5_amd.extremes import PeriodStats

    times, X, w, lab = _grid()
    st = PeriodStats.fit([_t(x) for x in X], times, group=2, inner="max", threshold=3.5, kern=PstatDouble())
    res = st.area_mean("maximum", weights=[_t(v) for v in w], groups=[_t(v, torch.int64) for v in lab])
    # group 0: row 0 (w 1); group 1: rows 1 (w 2; nothing in 2020) and 2 (w 3)
    assert res["mean"].shape == (2, 2) and res["mean"].dtype == torch.float64
    assert res["mean"].tolist() == [[5.0, 4.0], [0.0, (2 * 2 + 3 * 10) / 5.0]]
    assert res["weight"].tolist() == [[1.0, 1.0], [3.0, 5.0]] and res["rows"].tolist() == [[1, 1], [1, 2]]
    # intensity: NaN where nothing lies beyond the threshold -- those rows do not count
    it = st.area_mean("intensity")
    assert it["rows"].tolist() == [[1, 2]] and it["mean"].tolist() == [[5.0, (4 + 8.5) / 2]]
    wm = st.area_mean("when_max", weights=[_t(np.array([1.0, 0.0])), _t(np.array([1.0]))])
    assert wm["mean"].tolist() == [[0.5, 0.0]] and wm["rows"].tolist() == [[2, 2]]
    empty = st.area_mean("total", weights=[_t(np.zeros(2)), _t(np.ones(1))], groups=[_t(v, torch.int64) for v in lab])
    assert torch.isnan(empty["mean"][0]).all() and empty["mean"][1].tolist() == [0.0, 17.0]
    with pytest.raises(ValueError, match="index"):
        st.area_mean("n")
    with pytest.raises(ValueError, match="weights of block 0"):
        st.area_mean("total", weights=[_t(np.array([1.0, -1.0])), _t(np.ones(1))])
    with pytest.raises(ValueError, match="1 weight vectors"):
        st.area_mean("total", weights=[_t(np.ones(2))])


def test_area_mean_of_two_row_shards_is_one_collective():
    from dmd_era5_amd.extremes import PeriodStats

    times, X, w, lab = _grid()
    Xb, wb, gb = [_t(x) for x in X], [_t(v) for v in w], [_t(v, torch.int64) for v in lab]
    fit = lambda blocks: PeriodStats.fit(blocks, times, group=2, inner="sum", window=2, min_count=1, kern=PstatDouble())
    one = fit(Xb).area_mean("total", weights=wb, groups=gb)
    c1 = TwoRanks()
    fit(Xb[1:]).area_mean("total", weights=wb[1:], groups=gb[1:], comm=c1, n_groups=2)
    assert c1.tags == ["pstat_allreduce"]
    c0 = TwoRanks(other=c1.sent)
    res = fit(Xb[:1]).area_mean("total", weights=wb[:1], groups=gb[:1], comm=c0, n_groups=2)
    assert c0.tags == ["pstat_allreduce"]
    for key in ("mean", "weight", "rows"):
        assert np.array_equal(res[key].numpy(), one[key].numpy(), equal_nan=True), key


@pytest.mark.skipif(not __import__("dmd_era5_amd.hdf5_lite", fromlist=["x"]).available(), reason="libhdf5 not found")
def test_dataset_round_trip_through_a_file(tmp_path):
    from dmd_era5_amd import io_netcdf
    from dmd_era5_amd.extremes import PeriodStats
    from dmd_era5_amd.labeled import Coord

    times, X = _known_blocks()
    times = times.astype("datetime64[ns]") + np.timedelta64(1_500_000_001, "ns")              # not on an hour
    st = PeriodStats.fit([_t(x) for x in X], times, group=2, inner="range", window=1, min_count=1, threshold=0.5, below=True,
                         inclusive=True, kern=PstatDouble())
    M = 3
    coords = {"space": Coord("space", np.arange(M, dtype=np.int64)), "latitude": Coord("space", np.linspace(-60.0, 60.0, M)),
              "time": Coord("time", times)}
    ds = st.to_dataset(coords)
    assert ds["period_planes"].dims == ("plane", "space") and ds["period_planes"].shape == (8 * 2, M) and "time" not in ds.coords
    path = str(tmp_path / "extremes.nc")
    io_netcdf.to_netcdf(ds, path)
    back = PeriodStats.from_dataset(io_netcdf.open_dataset(path), rows=(2, 1), device="cpu", kern=PstatDouble())
    assert (back.group, back.inner, back.window, back.min_count, back.below, back.inclusive, back.has_threshold) == (
        2, "range", 1, 1, True, True, True)
    assert back.bounds.tolist() == [0, 4, 8] and back.labels.tolist() == ["2020", "2021"] and np.array_equal(back.times, times)
    for P, Q in zip(back.planes, st.planes):
        assert P.dtype == torch.float64 and P.shape == Q.shape and _same(P.numpy(), Q.numpy())
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(back.when_max(as_time=True), st.when_max(as_time=True)))
    one = PeriodStats.from_dataset(io_netcdf.open_dataset(path), device="cpu", kern=PstatDouble())
    assert len(one.planes) == 1 and one.planes[0].shape == (8, 2, M)
    plain = PeriodStats.fit([_t(x) for x in X], None, period=[0, 8], kern=PstatDouble())
    other = str(tmp_path / "plain.nc")
    io_netcdf.to_netcdf(plain.to_dataset(), other)
    again = PeriodStats.from_dataset(io_netcdf.open_dataset(other), device="cpu", kern=PstatDouble())
    assert again.times is None and _same(again.planes[0].numpy(), torch.cat(plain.planes, dim=2).numpy())
    with pytest.raises(ValueError, match="rows sum"):
        PeriodStats.from_dataset(io_netcdf.open_dataset(path), rows=(2, 4), device="cpu", kern=PstatDouble())


def test_every_value_error_comes_before_a_launch():
    from dmd_era5_amd.extremes import PeriodStats, period_stat_blocks

    times, X = _known_blocks()
    Xb, k = [_t(x) for x in X], PstatDouble()
    PstatDouble.pstat_calls = 0
    for bounds in ([0], [0, 0], [5, 3], [-1, 4], [0.5, 3.0]):
        with pytest.raises(ValueError, match="bounds"):
            period_stat_blocks(Xb, bounds, kern=k)
    with pytest.raises(ValueError, match="the bounds end at 9"):
        period_stat_blocks(Xb, [0, 9], kern=k)
    for kw, match in ((dict(group=0), "group"), (dict(group=2.0), "group"), (dict(window=0), "window"), (dict(window=9), "window"),
                      (dict(window=True), "window"), (dict(inner="median"), "inner"), (dict(inner=2), "inner"),
                      (dict(group=2, min_count=0), "min_count"), (dict(group=2, min_count=3), "min_count"),
                      (dict(min_count=1.0), "min_count")):
        with pytest.raises(ValueError, match=match):
            period_stat_blocks(Xb, [0, 8], kern=k, **kw)
        with pytest.raises(ValueError, match=match):
            PeriodStats.fit(Xb, times, kern=k, **kw)
    with pytest.raises(ValueError, match="1 tables for 2 blocks"):
        period_stat_blocks(Xb, [0, 8], threshold=[torch.zeros(2)], kern=k)
    with pytest.raises(ValueError, match="holds 1 rows, the block 2"):
        period_stat_blocks(Xb, [0, 8], threshold=[torch.zeros(1), torch.zeros(1)], kern=k)
    with pytest.raises(ValueError, match="one .rows,. tensor per block"):
        period_stat_blocks(Xb, [0, 8], threshold=[torch.zeros((2, 1)), torch.zeros(1)], kern=k)
    with pytest.raises(ValueError, match="needs times"):
        PeriodStats.fit(Xb, None, kern=k)
    with pytest.raises(ValueError, match="kind"):
        PeriodStats.fit(Xb, times, period="decade", kern=k)
    with pytest.raises(ValueError, match="block 0 holds 8 snapshots, times has 7"):
        PeriodStats.fit(Xb, times[:7], kern=k)
    with pytest.raises(ValueError, match="the bounds end at 9, times has 8"):
        PeriodStats.fit(Xb, times, period=[0, 9], kern=k)
    with pytest.raises(ValueError, match="no blocks"):
        PeriodStats.fit([], times, kern=k)
    assert PstatDouble.pstat_calls == 0


def test_alias_package_re_exports_the_module():
    import dmd_era5.extremes as alias
    import dmd_era5_amd.extremes as mod

    assert alias.PeriodStats is mod.PeriodStats and alias.snapshots_per_day is mod.snapshots_per_day
    assert set(alias.__all__) == set(mod.__all__) and mod.PLANES[5:] == ("total", "total_beyond", "count_beyond")
