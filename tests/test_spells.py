"""Host side of K27 without a GPU: tests/spell_ref.py (the definition the kernel is held to) against hand-made series
and against its own piece-and-merge restatement, and spells.periods_of / spell_blocks / SpellStats on the kernel double
spell_ref.SpellDouble.  All results are integers: every comparison is exact."""
import numpy as np
import pytest
import torch

import spell_ref as sr
from spell_ref import SpellDouble
from test_crps import TwoRanks

NV, NE, NS, NIN, LONGEST, FIRST, LAST = range(7)


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def _series(pattern):
    """A row of 1.0 (event for the threshold 0.5, above) and 0.0 from a string of '1' and '0'."""
    return np.array([float(c) for c in pattern], dtype=np.float32)


# ---------------------------------------------------------------- the reference itself
def test_reference_on_hand_made_series():
    rows = ["111111111111", "000000000000", "011100110001", "110011101111"]
    X = np.stack([_series(r) for r in rows])
    thr = np.full((2, 1, 4), 0.5, dtype=np.float32)
    Q = sr.spells(X, thr, [0, 12], min_len=[1, 3], above=True)
    assert Q.shape == (2, 7, 1, 4) and Q.dtype == np.int32
    want_ml1 = {NV: [12, 12, 12, 12], NE: [12, 0, 6, 9], NS: [1, 0, 3, 3], NIN: [12, 0, 6, 9], LONGEST: [12, 0, 3, 4],
                FIRST: [0, -1, 1, 0], LAST: [11, -1, 11, 11]}
    want_ml3 = {NV: [12, 12, 12, 12], NE: [12, 0, 6, 9], NS: [1, 0, 1, 2], NIN: [12, 0, 3, 7], LONGEST: [12, 0, 3, 4],
                FIRST: [0, -1, 1, 4], LAST: [11, -1, 3, 11]}
    for j, want in enumerate((want_ml1, want_ml3)):
        for q, v in want.items():
            assert Q[j, q, 0].tolist() == v, (j, q)
    # below: the events are the zeros
    B = sr.spells(X, thr[:1], [0, 12], min_len=2, above=False)
    assert B[0, NE, 0].tolist() == [0, 12, 6, 3] and B[0, NS, 0].tolist() == [0, 1, 2, 1]
    assert B[0, FIRST, 0].tolist() == [-1, 0, 4, 2] and B[0, LAST, 0].tolist() == [-1, 11, 10, 3]


def test_a_period_boundary_cuts_a_run_and_min_length_counts_each_part():
    #             period 0 | period 1
    X = _series("0001111" + "1100000")[None]
    thr = np.full((3, 1, 1), 0.5, dtype=np.float32)
    Q = sr.spells(X, thr, [0, 7, 14], min_len=[1, 4, 5])
    assert Q[0, NS, :, 0].tolist() == [1, 1] and Q[0, LONGEST, :, 0].tolist() == [4, 2]        # two runs, not one of 6
    assert Q[0, FIRST, :, 0].tolist() == [3, 0] and Q[0, LAST, :, 0].tolist() == [6, 1]        # the second starts at 0
    assert Q[1, NS, :, 0].tolist() == [1, 0] and Q[1, NIN, :, 0].tolist() == [4, 0]            # min_len = the run's length
    assert Q[2, NS, :, 0].tolist() == [0, 0] and Q[2, FIRST, :, 0].tolist() == [-1, -1]        # ... and one above it
    assert Q[2, LONGEST, :, 0].tolist() == [4, 2] and Q[2, NE, :, 0].tolist() == [4, 2]        # longest: qualifying or not
    one = sr.spells(X, thr[:1], [0, 14], min_len=6)
    assert one[0, :, 0, 0].tolist() == [14, 6, 1, 6, 6, 3, 8]
    # snapshots outside [b_0, b_P) are not read
    Xn = np.concatenate([[np.nan, 1.0], X[0], [1.0, np.nan]]).astype(np.float32)[None]
    assert np.array_equal(sr.spells(Xn, thr, [2, 9, 16], min_len=[1, 4, 5]), Q)


def test_reference_value_rules():
    X = np.array([[1.0, 2.0, np.nan, 2.0, np.inf, 2.0, -np.inf, 0.5, 2.0, 2.0]], dtype=np.float32)
    thr = np.array([0.5, 0.5, np.inf, -np.inf, np.nan], dtype=np.float32).reshape(5, 1, 1)
    Qa = sr.spells(X, thr[:4], [0, 10], above=[True, False, True, False])
    # NaN and +-Inf snapshots are invalid: no event, and they end a run; a tie (0.5) is valid and no event
    assert Qa[0, :, 0, 0].tolist() == [7, 6, 4, 6, 2, 0, 9]
    assert Qa[1, :, 0, 0].tolist() == [7, 0, 0, 0, 0, -1, -1]
    assert Qa[2, NE, 0, 0] == 0 and Qa[2, NV, 0, 0] == 7                       # nothing finite is above +Inf
    assert Qa[3, NE, 0, 0] == 0                                                # ... or below -Inf
    Qb = sr.spells(X, thr[2:5], [0, 10], above=[False, True, True])
    assert Qb[0, NE, 0, 0] == 7 and Qb[1, NE, 0, 0] == 7                       # every finite value is below +Inf, above -Inf
    assert Qb[2, :, 0, 0].tolist() == [0, 0, 0, 0, 0, -1, -1]                  # a NaN threshold: nothing is valid
    # slots: the threshold of the snapshot's slot; a label outside 0 .. S - 1 is an invalid snapshot
    X2 = np.array([[1.0, 1.0, 1.0, 1.0, 1.0, 1.0]], dtype=np.float32)
    th2 = np.array([0.0, 2.0], dtype=np.float32).reshape(1, 2, 1)
    Q2 = sr.spells(X2, th2, [0, 6], slot=[0, 0, 1, 0, 7, 0])
    assert Q2[0, :, 0, 0].tolist() == [5, 4, 3, 4, 2, 0, 5]


def _random_case(rs):
    m, T = int(rs.randint(1, 4)), int(rs.randint(1, 40))
    J, S = int(rs.randint(1, 5)), int(rs.randint(1, 4))
    X = np.round(rs.standard_normal((m, T)).cumsum(axis=1) * 2).astype(np.float32) / 2        # ties occur
    X[rs.rand(m, T) < 0.05] = np.nan
    thr = (np.round(rs.standard_normal((J, S, m)) * 2) / 2).astype(np.float32)
    thr[rs.rand(J, S, m) < 0.03] = np.nan
    slot = rs.randint(-1 if rs.rand() < 0.2 else 0, S, T) if S > 1 or rs.rand() < 0.5 else None
    cuts = np.sort(rs.choice(np.arange(T + 1), size=min(T + 1, int(rs.randint(2, 6))), replace=False))
    return X, thr, cuts, [int(v) for v in rs.randint(1, 5, J)], [bool(v) for v in rs.randint(0, 2, J)], slot


def test_reference_equals_its_piece_and_merge_restatement_on_random_cases():
    """The merge rule of the split form (all events: extend the carry; else close carry + head, add the interior, the
    tail is the new carry; close at the period's end) against the plain loop: 1000 random cases, each with seg in
    {1, 3, T} and a random one -- 4000 comparisons."""
    rs = np.random.RandomState(27)
    closed_across = 0
    for case in range(1000):
        X, thr, bounds, ml, ab, slot = _random_case(rs)
        want = sr.spells(X, thr, bounds, ml, ab, slot)
        for seg in (1, 3, X.shape[1], int(rs.randint(2, 12))):
            got = sr.spells_by_pieces(X, thr, bounds, ml, ab, slot, seg=seg)
            assert np.array_equal(got, want), (case, seg)
        closed_across += int((want[:, LONGEST] > 3).any())
    assert closed_across > 200                                    # runs longer than a piece of 3 occur throughout


@pytest.mark.parametrize("seg", [1, 3, 61])
def test_reference_equals_its_restatement_on_the_gpu_test_layout(seg):
    rs = np.random.RandomState(5)
    m, T, bounds = 7, 61, [2, 9, 10, 37, 58]
    X = np.empty((m, T), dtype=np.float32)
    x = np.zeros(m)
    for t in range(T):
        x = 0.8 * x + rs.standard_normal(m)
        X[:, t] = x
    X[0], X[1] = 50.0, -50.0
    thr = np.quantile(X[2:], [0.15, 0.5, 0.85]).astype(np.float32)[:, None, None] * np.ones((3, 5, m), dtype=np.float32)
    slot = (np.arange(T) // 3) % 5
    want = sr.spells(X, thr, bounds, [1, 2, 3], [False, True, True], slot)
    assert np.array_equal(sr.spells_by_pieces(X, thr, bounds, [1, 2, 3], [False, True, True], slot, seg=seg), want)
    assert want[2, NE, :, 0].tolist() == [7, 1, 27, 21] and want[0, NE, :, 1].tolist() == [7, 1, 27, 21]
    assert sr.n_pieces(bounds, seg) == {1: 56, 3: 3 + 1 + 9 + 7, 61: 4}[seg]


# ---------------------------------------------------------------- periods_of
def test_periods_of_a_leap_year_and_a_series_that_starts_mid_season():
    from dmd_era5_amd.spells import periods_of

    days = np.arange(np.datetime64("2019-11-15"), np.datetime64("2021-03-10"))           # 2020 is a leap year
    b, lab = periods_of(days, "year")
    assert b.dtype == np.int32 and b.tolist() == [0, 47, 47 + 366, len(days)] and lab.tolist() == ["2019", "2020", "2021"]
    b, lab = periods_of(days, "season")
    # SON 2019 cut off at its start, DJF 2020 (Dec 2019 .. Feb 2020, 31 + 31 + 29 days), ..., MAM 2021 cut off at its end
    assert lab.tolist() == ["2019-SON", "2020-DJF", "2020-MAM", "2020-JJA", "2020-SON", "2021-DJF", "2021-MAM"]
    assert np.diff(b).tolist() == [16, 91, 92, 92, 91, 90, 9] and b[-1] == len(days)
    b, lab = periods_of(days, "month")
    assert lab[:4].tolist() == ["2019-11", "2019-12", "2020-01", "2020-02"] and np.diff(b)[:4].tolist() == [16, 31, 31, 29]
    assert len(lab) == 17 and lab[-1] == "2021-03"
    b, lab = periods_of(days, "all")
    assert b.tolist() == [0, len(days)] and lab.tolist() == ["all"]
    hours = np.datetime64("2020-12-31T20", "h") + np.arange(8) * np.timedelta64(1, "h")
    assert periods_of(hours, "year")[0].tolist() == [0, 4, 8]
    assert periods_of(np.array(["1969-12-30", "1970-01-02"], dtype="datetime64[D]"), "season")[1].tolist() == ["1970-DJF"]


def test_periods_of_errors():
    from dmd_era5_amd.spells import periods_of

    days = np.arange(np.datetime64("2020-01-01"), np.datetime64("2020-01-09"))
    with pytest.raises(ValueError, match="strictly ascending"):
        periods_of(days[[0, 2, 1, 3]], "year")
    with pytest.raises(ValueError, match="strictly ascending"):
        periods_of(days[[0, 1, 1, 3]], "year")
    with pytest.raises(ValueError, match="kind"):
        periods_of(days, "decade")
    with pytest.raises(ValueError, match="datetime64"):
        periods_of(np.arange(8), "year")
    with pytest.raises(ValueError, match="no times"):
        periods_of(days[:0], "year")


# ---------------------------------------------------------------- spell_blocks
def test_spell_blocks_scalar_thresholds_and_tables():
    from dmd_era5_amd.spells import spell_blocks

    rs = np.random.RandomState(2)
    X = [rs.standard_normal((30, mb)).astype(np.float32).cumsum(axis=0) for mb in (9, 4)]
    bounds = [0, 11, 30]
    SpellDouble.spell_calls = 0
    frost = spell_blocks([_t(x) for x in X], 0.25, bounds, min_length=2, above=False, kern=SpellDouble())
    assert SpellDouble.spell_calls == 2
    for Q, x in zip(frost, X):
        assert Q.shape == (1, 7, 2, x.shape[1]) and Q.dtype == torch.int32
        want = sr.spells(x.T, np.full((1, 1, x.shape[1]), 0.25, dtype=np.float32), bounds, 2, False)
        assert np.array_equal(Q.numpy(), want)
    two = spell_blocks([_t(x) for x in X], [0.25, -1.0], bounds, min_length=(1, 3), above=(True, False), kern=SpellDouble())
    for Q, x in zip(two, X):
        thr = np.array([0.25, -1.0], dtype=np.float32)[:, None, None] * np.ones((2, 1, x.shape[1]), dtype=np.float32)
        assert np.array_equal(Q.numpy(), sr.spells(x.T, thr, bounds, [1, 3], [True, False]))
    # per-block tables with slots
    tabs = [rs.standard_normal((2, 3, x.shape[1])).astype(np.float32) for x in X]
    slot = np.arange(30) % 3
    got = spell_blocks([_t(x) for x in X], [_t(t) for t in tabs], bounds, slot=slot, kern=SpellDouble())
    for Q, x, t in zip(got, X, tabs):
        assert np.array_equal(Q.numpy(), sr.spells(x.T, t, bounds, 1, True, slot))
    flat = spell_blocks([_t(x) for x in X], [_t(t[:, 0]) for t in tabs], bounds, kern=SpellDouble())        # (J, rows)
    assert np.array_equal(flat[1].numpy(), sr.spells(X[1].T, tabs[1][:, :1], bounds))


def test_spell_blocks_shape_errors():
    from dmd_era5_amd.spells import spell_blocks

    X = [_t(np.zeros((30, 9))), _t(np.zeros((30, 4)))]
    k = SpellDouble()
    SpellDouble.spell_calls = 0
    tabs = [torch.zeros((2, 3, 9)), torch.zeros((2, 3, 4))]
    for bounds in ([0], [0, 0], [5, 3], [-1, 4], [0.5, 3.0]):
        with pytest.raises(ValueError, match="bounds"):
            spell_blocks(X, 1.0, bounds, kern=k)
    with pytest.raises(ValueError, match="the bounds end at 31"):
        spell_blocks(X, 1.0, [0, 31], kern=k)
    with pytest.raises(ValueError, match="1 .. 4"):
        spell_blocks(X, [1.0] * 5, [0, 30], kern=k)
    with pytest.raises(ValueError, match="min_length"):
        spell_blocks(X, [1.0, 2.0], [0, 30], min_length=(1, 2, 3), kern=k)
    with pytest.raises(ValueError, match="min_length must be >= 1"):
        spell_blocks(X, 1.0, [0, 30], min_length=0, kern=k)
    with pytest.raises(ValueError, match="above"):
        spell_blocks(X, 1.0, [0, 30], above=(True, False), kern=k)
    with pytest.raises(ValueError, match="1 threshold tables for 2 blocks"):
        spell_blocks(X, tabs[:1], [0, 30], slot=np.arange(30) % 3, kern=k)
    with pytest.raises(ValueError, match="slot must name one"):
        spell_blocks(X, tabs, [0, 30], kern=k)
    with pytest.raises(ValueError, match="integer labels in 0 .. 2"):
        spell_blocks(X, tabs, [0, 30], slot=np.arange(30) % 4, kern=k)
    with pytest.raises(ValueError, match="holds 4 rows, the block 9"):
        spell_blocks(X, [tabs[1], tabs[1]], [0, 30], slot=np.arange(30) % 3, kern=k)
    assert SpellDouble.spell_calls == 0                                       # all before any launch


# ---------------------------------------------------------------- SpellStats
def _known_blocks():
    """Daily stamps from 2020-12-22 to 2021-01-10 (10 days in each year), rows with known answers for the threshold
    0.5 above: all events; none; a run of 6 that ends exactly at the year boundary and goes on for 4 days; a run of 3."""
    times = np.arange(np.datetime64("2020-12-22"), np.datetime64("2021-01-11"))
    rows = ["1" * 20, "0" * 20, "0000111111" + "1111000000", "0111000000" + "0000011100"]
    X = np.stack([_series(r) for r in rows], axis=1)                           # (T, 4)
    return times, [X[:, :3].copy(), X[:, 3:].copy()]


def test_spellstats_accessors_on_series_with_known_answers():
    from dmd_era5_amd.spells import SpellStats

    times, X = _known_blocks()
    stats = SpellStats.fit([_t(x) for x in X], times, thresholds=[0.5, 0.5, 0.5], min_length=(1, 4, 3), kern=SpellDouble())
    assert stats.bounds.tolist() == [0, 10, 20] and stats.labels.tolist() == ["2020", "2021"]
    assert (stats.n_thresholds, stats.n_periods, stats.min_length, stats.above) == (3, 2, (1, 4, 3), (True, True, True))
    assert stats.period_lengths().tolist() == [10, 10]
    cat = lambda blocks: np.concatenate([np.asarray(b) for b in blocks], axis=2)           # (J, P, 4 rows)
    freq, count, days, longest = (cat(f()) for f in (stats.frequency, stats.spell_count, stats.spell_days, stats.longest))
    onset, end = cat(stats.onset()), cat(stats.end())
    assert freq.dtype == np.float64 and count.dtype == np.int32
    assert freq[0].tolist() == [[1.0, 0.0, 0.6, 0.3], [1.0, 0.0, 0.4, 0.3]]
    assert count[0].tolist() == [[1, 0, 1, 1], [1, 0, 1, 1]]                  # the run across New Year: one in each year
    assert longest[0].tolist() == [[10, 0, 6, 3], [10, 0, 4, 3]] and np.array_equal(longest[1], longest[0])
    assert onset[0].tolist() == [[0, -1, 4, 1], [0, -1, 0, 5]]               # ... the second with offset 0
    assert end[0].tolist() == [[9, -1, 9, 3], [9, -1, 3, 7]]
    # min_length 4: the run of 4 qualifies (one below: its own length), the runs of 3 do not (one above)
    assert count[1].tolist() == [[1, 0, 1, 0], [1, 0, 1, 0]] and days[1].tolist() == [[10, 0, 6, 0], [10, 0, 4, 0]]
    assert onset[1].tolist() == [[0, -1, 4, -1], [0, -1, 0, -1]]
    assert count[2].tolist() == [[1, 0, 1, 1], [1, 0, 1, 1]] and days[2].tolist() == [[10, 0, 6, 3], [10, 0, 4, 3]]
    when = cat(stats.onset(as_time=True))
    assert when.dtype == np.dtype("datetime64[ns]") and when[0, 1, 2] == np.datetime64("2021-01-01") and np.isnat(when[0, 0, 1])
    assert when[0, 0, 3] == np.datetime64("2020-12-23") and cat(stats.end(as_time=True))[0, 1, 3] == np.datetime64("2021-01-08")
    # one period over both years: the run is one of 10
    whole = SpellStats.fit([_t(x) for x in X], times, thresholds=0.5, period="all", min_length=6, kern=SpellDouble())
    assert cat(whole.spell_days())[0, 0].tolist() == [20, 0, 10, 0] and cat(whole.onset())[0, 0].tolist() == [0, -1, 4, -1]
    # a period given as bounds needs no times; then there are offsets only
    plain = SpellStats.fit([_t(x) for x in X], None, thresholds=0.5, period=[0, 10, 20], kern=SpellDouble())
    assert np.array_equal(cat(plain.spell_count()), count[:1]) and plain.labels.tolist() == ["0", "1"]
    with pytest.raises(ValueError, match="only the offsets"):
        plain.onset(as_time=True)
    # an invalid period: frequency is NaN there
    Xn = [x.copy() for x in X]
    Xn[0][:10, 1] = np.nan
    f = cat(SpellStats.fit([_t(x) for x in Xn], times, thresholds=0.5, kern=SpellDouble()).frequency())
    assert np.isnan(f[0, 0, 1]) and f[0, 1, 1] == 0.0


def test_spellstats_fit_with_a_climatology_and_its_errors():
    from dmd_era5_amd.climatology import Climatology
    from dmd_era5_amd.spells import SpellStats

    rs = np.random.RandomState(3)
    T = 96
    times = np.datetime64("2020-12-30T00", "h") + np.arange(T) * np.timedelta64(1, "h")
    X = [rs.standard_normal((T, mb)).astype(np.float32).cumsum(axis=0) for mb in (5, 3)]
    quant = [np.sort(rs.standard_normal((2, 24, mb)).astype(np.float32), axis=0) for mb in (5, 3)]
    clim = Climatology("hour", 0, [_t(q[0]) for q in quant], None, np.full(24, 4), 0, None, (0.1, 0.9), [_t(q) for q in quant])
    stats = SpellStats.fit([_t(x) for x in X], times, climatology=clim, above=(False, True), min_length=2, kern=SpellDouble())
    assert stats.bounds.tolist() == [0, 48, 96]
    slot = np.arange(T) % 24
    for Q, x, q in zip(stats.planes, X, quant):
        assert np.array_equal(Q.numpy(), sr.spells(x.T, q, [0, 48, 96], 2, [False, True], slot))
    with pytest.raises(ValueError, match="no thresholds"):
        SpellStats.fit([_t(x) for x in X], times, kern=SpellDouble())
    with pytest.raises(ValueError, match="pass times and no slot"):
        SpellStats.fit([_t(x) for x in X], times, climatology=clim, slot=slot, kern=SpellDouble())
    with pytest.raises(ValueError, match="needs times"):
        SpellStats.fit([_t(x) for x in X], None, thresholds=0.0, kern=SpellDouble())
    with pytest.raises(ValueError, match="block 0 holds 96 snapshots, times has 95"):
        SpellStats.fit([_t(x) for x in X], times[:95], thresholds=0.0, kern=SpellDouble())
    with pytest.raises(ValueError, match="no blocks"):
        SpellStats.fit([], times, thresholds=0.0, kern=SpellDouble())


def _grid():
    times, X = _known_blocks()
    w = [np.array([1.0, 2.0, 0.0], dtype=np.float32), np.array([3.0], dtype=np.float32)]       # row 2 has weight 0
    lab = [np.array([0, 1, 0]), np.array([1])]
    return times, X, w, lab


def test_area_mean_with_a_zero_weight_row_and_two_groups():
    from dmd_era5_amd.spells import SpellStats

    times, X, w, lab = _grid()
    stats = SpellStats.fit([_t(x) for x in X], times, thresholds=0.5, min_length=1, kern=SpellDouble())
    res = stats.area_mean("spell_days", weights=[_t(v) for v in w], groups=[_t(v, torch.int64) for v in lab])
    # group 0: rows 0 (w 1: 10, 10) and 2 (w 0: left out); group 1: rows 1 (w 2: 0, 0) and 3 (w 3: 3, 3)
    assert res["mean"].shape == (2, 1, 2) and res["mean"].dtype == torch.float64
    assert res["mean"][:, 0].tolist() == [[10.0, 10.0], [9.0 / 5.0, 9.0 / 5.0]]
    assert res["weight"][:, 0].tolist() == [[1.0, 1.0], [5.0, 5.0]] and res["rows"][:, 0].tolist() == [[1, 1], [2, 2]]
    # onset: only the rows that have a spell count (row 1 has none)
    on = stats.area_mean("onset", weights=[_t(v) for v in w], groups=[_t(v, torch.int64) for v in lab])
    assert on["mean"][:, 0].tolist() == [[0.0, 0.0], [1.0, 5.0]] and on["rows"][:, 0].tolist() == [[1, 1], [1, 1]]
    # no weights, one group: every row counts 1; the frequency of the four rows
    fr = stats.area_mean("frequency")
    assert torch.allclose(fr["mean"][0, 0], torch.tensor([1.9 / 4, 1.7 / 4], dtype=torch.float64), rtol=1e-15)
    # a row without a valid snapshot in a period is left out of that period only
    Xn = [x.copy() for x in X]
    Xn[0][:10, 0] = np.nan
    sn = SpellStats.fit([_t(x) for x in Xn], times, thresholds=0.5, kern=SpellDouble())
    lo = sn.area_mean("longest")
    assert lo["rows"][0, 0].tolist() == [3, 4] and lo["mean"][0, 0].tolist() == [9.0 / 3.0, 17.0 / 4.0]
    # a group that nothing counts for: NaN
    empty = stats.area_mean("spell_days", weights=[_t(np.zeros(3)), _t(np.ones(1))], groups=[_t(v, torch.int64) for v in lab])
    assert torch.isnan(empty["mean"][0]).all() and empty["mean"][1, 0].tolist() == [3.0, 3.0]
    with pytest.raises(ValueError, match="index"):
        stats.area_mean("n_valid")
    with pytest.raises(ValueError, match="weights of block 0"):
        stats.area_mean("longest", weights=[_t(np.array([1.0, -1.0, 1.0])), _t(np.ones(1))])
    with pytest.raises(ValueError, match="1 weight vectors"):
        stats.area_mean("longest", weights=[_t(np.ones(3))])


def test_area_mean_of_two_row_shards_is_one_collective():
    from dmd_era5_amd.spells import SpellStats

    times, X, w, lab = _grid()
    Xb, wb, gb = [_t(x) for x in X], [_t(v) for v in w], [_t(v, torch.int64) for v in lab]
    fit = lambda blocks: SpellStats.fit(blocks, times, thresholds=[0.5, 0.5], min_length=(1, 4), kern=SpellDouble())
    one = fit(Xb).area_mean("spell_days", weights=wb, groups=gb)
    c1 = TwoRanks()
    fit(Xb[1:]).area_mean("spell_days", weights=wb[1:], groups=gb[1:], comm=c1, n_groups=2)
    assert c1.tags == ["spell_allreduce"]
    c0 = TwoRanks(other=c1.sent)
    res = fit(Xb[:1]).area_mean("spell_days", weights=wb[:1], groups=gb[:1], comm=c0, n_groups=2)
    assert c0.tags == ["spell_allreduce"]
    for key in ("mean", "weight", "rows"):
        assert torch.equal(res[key], one[key]), key


@pytest.mark.skipif(not __import__("dmd_era5_amd.hdf5_lite", fromlist=["x"]).available(), reason="libhdf5 not found")
def test_dataset_round_trip_through_a_file(tmp_path):
    from dmd_era5_amd import io_netcdf
    from dmd_era5_amd.labeled import Coord
    from dmd_era5_amd.spells import SpellStats

    times, X = _known_blocks()
    times = times.astype("datetime64[ns]") + np.timedelta64(1_500_000_001, "ns")              # not on an hour
    stats = SpellStats.fit([_t(x) for x in X], times, thresholds=[0.5, 0.25], min_length=(1, 4), above=(True, False),
                           kern=SpellDouble())
    M = 4
    coords = {"space": Coord("space", np.arange(M, dtype=np.int64)), "latitude": Coord("space", np.linspace(-60.0, 60.0, M)),
              "time": Coord("time", times)}
    ds = stats.to_dataset(coords)
    assert ds["spell_planes"].dims == ("plane", "space") and ds["spell_planes"].shape == (2 * 7 * 2, M) and "time" not in ds.coords
    path = str(tmp_path / "spells.nc")
    io_netcdf.to_netcdf(ds, path)
    back = SpellStats.from_dataset(io_netcdf.open_dataset(path), rows=(3, 1), device="cpu", kern=SpellDouble())
    assert (back.min_length, back.above, back.bounds.tolist(), back.labels.tolist()) == ((1, 4), (True, False), [0, 10, 20],
                                                                                        ["2020", "2021"])
    assert np.array_equal(back.times, times)
    for P, Q in zip(back.planes, stats.planes):
        assert P.dtype == torch.int32 and P.shape == Q.shape and torch.equal(P, Q)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(back.onset(as_time=True), stats.onset(as_time=True)))
    one = SpellStats.from_dataset(io_netcdf.open_dataset(path), device="cpu", kern=SpellDouble())
    assert len(one.planes) == 1 and one.planes[0].shape == (2, 7, 2, M)
    plain = SpellStats.fit([_t(x) for x in X], None, thresholds=0.5, period=[0, 20], kern=SpellDouble())
    other = str(tmp_path / "plain.nc")
    io_netcdf.to_netcdf(plain.to_dataset(), other)
    again = SpellStats.from_dataset(io_netcdf.open_dataset(other), device="cpu", kern=SpellDouble())
    assert again.times is None and torch.equal(again.planes[0], torch.cat(plain.planes, dim=3))
    with pytest.raises(ValueError, match="rows sum"):
        SpellStats.from_dataset(io_netcdf.open_dataset(path), rows=(3, 4), device="cpu", kern=SpellDouble())


def test_alias_package_re_exports_the_module():
    import dmd_era5.spells as alias
    import dmd_era5_amd.spells as mod

    assert alias.SpellStats is mod.SpellStats and alias.periods_of is mod.periods_of and set(alias.__all__) == set(mod.__all__)
