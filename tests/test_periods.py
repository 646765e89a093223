"""The host helpers of the per-period statistics (dmd_era5_amd/_periods.py) on their own, without a kernel: what
spells.SpellStats ((J, P, rows) planes) and extremes.PeriodStats ((P, rows) planes) both go through."""
import numpy as np
import pytest
import torch

from dmd_era5_amd import _periods as pp

ROWS, P, J = (5, 7), 3, 2


def _blocks():
    """Per block: n_valid and an index as (J, P, rows), the weights and the group labels.  Row 1 of block 0 has weight 0,
    row 2 of block 1 no valid period, the index is -1 here and there (no spell)."""
    rs = np.random.RandomState(5)
    nv = [torch.from_numpy(rs.randint(1, 9, (J, P, r)).astype(np.int32)) for r in ROWS]
    nv[1][:, :, 2] = 0
    nv[0][1, 2, 4] = 0                                          # ... and one single (j, period, row) without
    val = [torch.from_numpy(rs.randint(-1, 30, (J, P, r)).astype(np.int32)) for r in ROWS]
    w = [torch.from_numpy(rs.rand(r) + 0.5) for r in ROWS]
    w[0][1] = 0.0
    groups = [torch.tensor([0, 1, 1, 0, 1]), torch.tensor([1, 0, 0, 1, 1, 0, 1])]
    return nv, val, w, groups


@pytest.mark.parametrize("extra", [None, lambda v: v >= 0])
def test_area_mean_sums_with_a_leading_axis_is_the_call_per_j(extra):
    nv, val, w, groups = _blocks()
    both = pp.area_mean_sums(nv, val, extra, w, groups, None, None, "tag", "who")
    assert both["mean"].shape == (2, J, P) and both["mean"].dtype == torch.float64 and both["rows"].dtype == torch.int64
    for j in range(J):
        one = pp.area_mean_sums([n[j] for n in nv], [v[j] for v in val], extra, w, groups, None, None, "tag", "who")
        assert one["mean"].shape == (2, P)
        for key in ("mean", "weight", "rows"):
            assert torch.equal(one[key].view(torch.int64), both[key][:, j].contiguous().view(torch.int64)), (key, j)
    # the rows that count, by hand: weight not 0, a valid period, and what `extra` asks for
    keep = [(wb != 0) & (n > 0) & (torch.ones_like(v, dtype=torch.bool) if extra is None else extra(v))
            for wb, n, v in zip(w, nv, val)]
    for g in range(2):
        rows = sum((k[:, :, gb == g]).sum(dim=2) for k, gb in zip(keep, groups))
        assert torch.equal(both["rows"][g], rows)
    assert not keep[0][:, :, 1].any() and not keep[1][:, :, 2].any() and not keep[0][1, 2, 4]


def test_area_mean_sums_is_nan_where_no_row_counts_and_names_its_caller():
    nv, val, w, groups = _blocks()
    none = pp.area_mean_sums(nv, val, lambda v: v > 99, w, groups, None, None, "tag", "who")
    assert torch.isnan(none["mean"]).all() and (none["weight"] == 0).all() and (none["rows"] == 0).all()
    with pytest.raises(ValueError, match="Some.area_mean: 1 weight vectors for 2 blocks"):
        pp.area_mean_sums(nv, val, None, w[:1], groups, None, None, "tag", "Some.area_mean")
    with pytest.raises(ValueError, match=r"weights\[1\] has 5 entries, the block 7 rows"):
        pp.area_mean_sums(nv, val, None, [w[0], w[0]], groups, None, None, "tag", "who")


@pytest.mark.parametrize("scale", [1, 4])
def test_when_is_nat_exactly_where_the_offset_is_minus_one(scale):
    start = np.array([0, 40, 70])
    times = np.datetime64("2001-01-01T00", "h").astype("datetime64[ns]") + np.arange(120) * np.timedelta64(1, "h")
    rs = np.random.RandomState(scale)
    off3 = [torch.from_numpy(rs.randint(-1, 30 // scale, (J, P, r)).astype(np.int32)) for r in ROWS]
    for o in off3:
        o[:, :, 2] = -1                                                          # a row without any, and one single period
        o[:, 1, 0] = -1
        o[:, 0, 1] = 0                                                           # ... and the period's first snapshot
    off2 = [o[1].to(torch.int64) for o in off3]                                  # (P, rows), as K29 holds them
    for offsets in (off3, off2):
        got = pp.when(offsets, start, scale, times, "who")
        for o, stamp in zip(offsets, got):
            o = o.numpy().astype(np.int64)
            assert stamp.shape == o.shape and stamp.dtype == times.dtype and (o < 0).any() and (o >= 0).any()
            assert np.array_equal(np.isnat(stamp), o == -1)
            want = times[0] + (start[:, None] + o * scale) * np.timedelta64(1, "h")
            assert np.array_equal(stamp[o >= 0], want[o >= 0])
    with pytest.raises(ValueError, match="Stats.onset: fitted without times: only the offsets are known"):
        pp.when(off3, start, scale, None, "Stats.onset")


def test_resolve_periods():
    times = np.arange(np.datetime64("2020-12-22"), np.datetime64("2021-01-11"))
    t, bounds, labels = pp.resolve_periods(times, "year", "Stats.fit")
    assert t.dtype == np.dtype("datetime64[ns]") and bounds.dtype == np.int32 and bounds.tolist() == [0, 10, 20]
    assert labels.tolist() == ["2020", "2021"]
    t, bounds, labels = pp.resolve_periods(None, [2, 5, 30], "Stats.fit")
    assert t is None and bounds.dtype == np.int32 and bounds.tolist() == [2, 5, 30] and labels.tolist() == ["0", "1"]
    assert pp.resolve_periods(times, [0, 20], "Stats.fit")[1].tolist() == [0, 20]
    with pytest.raises(ValueError, match="Stats.fit: the bounds end at 21, times has 20"):
        pp.resolve_periods(times, [0, 10, 21], "Stats.fit")
    with pytest.raises(ValueError, match="Stats.fit: period = 'year' needs times"):
        pp.resolve_periods(None, "year", "Stats.fit")
    with pytest.raises(ValueError, match="Stats.fit: bounds must be >= 0 and strictly ascending"):
        pp.resolve_periods(times, [0, 10, 10], "Stats.fit")


def test_checked_blocks_and_ratio():
    times = np.arange(np.datetime64("2020-12-22"), np.datetime64("2021-01-11")).astype("datetime64[ns]")
    blocks = [torch.zeros(20, 3), torch.zeros(19, 2)]
    seen = pp.checked_blocks(blocks, times, "Stats.fit")
    assert next(seen) is blocks[0]                                              # lazily: a block is checked as it is reached
    with pytest.raises(ValueError, match="Stats.fit: block 1 holds 19 snapshots, times has 20"):
        next(seen)
    assert [x.shape[0] for x in pp.checked_blocks(blocks, None, "who")] == [20, 19]
    r = pp.ratio(torch.tensor([3.0, 1.0, 0.0], dtype=torch.float64), torch.tensor([2.0, 0.0, 0.0], dtype=torch.float64))
    assert r[0] == 1.5 and torch.isnan(r[1:]).all()
