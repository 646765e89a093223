"""K29 (dmdx_period_stats_f32) alone, on one cfg2 row block, against the torch composition and the one-read stream next
door.

X is one resident row block, 129 780 rows x 8760 hourly snapshots (4.55 GB fp32), one period (the year).  In ONE process
and alternating:
  split-g24-{max,sum,range}-w1   kern.period_stats with days of 24 snapshots: time split into pieces of SEGMENT days
                                 through the workspace, records merged in order
  split-g24-sum-w5               a running sum over 5 days (Rx5day): every piece reads the 4 days before it again
  split-g24-sum-w1-thr           a per-row threshold (PRCPTOT / SDII)
  split-g1-sum-w1                every snapshot a day
  walk-g24-max-w1                workspace == NULL: one lane walks the year of its rows (one workgroup row)
  k20-count                      kern.row_missing_count(X): the project's one-read stream over the same block
  torch                          (``--torch``) the composition the kernel replaces, for inner = max at w = 1 and for the
                                 5-day sum: reshape to (365, 24, m), an fp64 copy, amax / sum over the day axis, unfold
                                 for the running window, the finite mask, the reduction over the year
Conditions, asserted before anything is timed: split and walk give equal planes, n / max / argmax / min / argmin are
equal for every seg of (8, SEGMENT, 365), and with ``--torch`` the maxima and their days equal the kernel's.  Times are
HIP events around batches of calls on the current stream (>= ``--sample-ms`` of device time per sample), ``--reps``
samples after ``--warmup`` calls; medians, minimum and maximum, with GB/s of one read of X, the fraction of the 6.3
TB/s HBM figure of DESIGN.md that is, and the ratio to K20's rate in the same run.  One JSON line per variant; ``--out
FILE`` appends them to a file too.  No bar is set but one: split-g24-max-w1 must not be slower than the torch composition
it replaces, measured in the same run (``not_slower_than_torch``).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dmd_era5_amd import _lib  # noqa: E402
from dmd_era5_amd.extremes import SEGMENT  # noqa: E402
from dmd_era5_amd.kernels import PSTAT_INNER, default_kernels  # noqa: E402

HBM_TBS = 6.3

ap = argparse.ArgumentParser()
ap.add_argument("--m", type=int, default=129780, help="rows of the block")
ap.add_argument("--T", type=int, default=8760, help="hourly snapshots (a multiple of 24 for --torch)")
ap.add_argument("--torch", action="store_true", help="time the torch composition too (an fp64 copy of X: 9.1 GB)")
ap.add_argument("--seg-days", type=int, default=SEGMENT, help="the days of a piece (default: extremes.SEGMENT)")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--sample-ms", type=float, default=20.0)
ap.add_argument("--out", default="", help="append the JSON lines to this file too (default: print only)")
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_extremes: no GPU visible (a CPU run measures nothing)")
K = default_kernels()
dev = torch.device("cuda")
m, T, SEG = a.m, a.T, a.seg_days
X = torch.empty((T, m), dtype=torch.float32, device=dev)
gen = torch.Generator(device=dev).manual_seed(29)
X[0].normal_(0.0, 1.0, generator=gen)
for t in range(1, T):                                            # AR(1), phi = 0.9
    X[t].normal_(0.0, 0.436, generator=gen).add_(X[t - 1], alpha=0.9)
X[T // 3, ::1000] = float("nan")                                 # a missing day in some rows
bounds = [0, T]
thr = torch.zeros(m, device=dev).normal_(20.0, 2.0, generator=gen)


def batch_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def measure(fns):
    calls = {}
    for name, fn in fns.items():
        for _ in range(a.warmup):
            fn()
        calls[name] = max(1, int(a.sample_ms / max(batch_ms(fn, 1), 1e-3)))
    ms = {name: [] for name in fns}
    for _ in range(a.reps):                                      # alternating: all see the same machine
        for name, fn in fns.items():
            ms[name].append(batch_ms(fn, calls[name]))
    return ms, calls


def walk(g, inner, w, out):
    """The C entry point with workspace == NULL (the wrapper always splits a year)."""
    rc = K._lib.dmdx_period_stats_f32(X.data_ptr(), m, T, m, (ctypes.c_int32 * 2)(0, T), 1, g, PSTAT_INNER.index(inner), w, g,
                                      None, SEG, out.data_ptr(), m, 0, None, 0, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "dmdx_period_stats_f32")
    return out


def composition(w):
    """n, max and argmax of the daily maximum (w = 1) or of the w-day running sum of daily sums over the one period."""
    days = X.reshape(T // 24, 24, m)
    fin = torch.isfinite(days).all(dim=1)                        # min_count = 24: a day with a missing snapshot is none
    d = days.to(torch.float64)
    d = d.amax(dim=1) if w == 1 else d.sum(dim=1)
    if w > 1:
        d = d.unfold(0, w, 1).sum(dim=2)
        fin = fin.unfold(0, w, 1).all(dim=2)
    d = torch.where(fin, d, torch.full_like(d, float("-inf")))
    top = d.max(dim=0)
    return fin.sum(dim=0), top.values, top.indices + (w - 1)


cases = {"split-g24-max-w1": (24, "max", 1, None), "split-g24-sum-w1": (24, "sum", 1, None),
         "split-g24-range-w1": (24, "range", 1, None), "split-g24-sum-w5": (24, "sum", 5, None),
         "split-g24-sum-w1-thr": (24, "sum", 1, thr), "split-g1-sum-w1": (1, "sum", 1, None)}
outs = {name: torch.empty((8, 1, m), dtype=torch.float64, device=dev) for name in cases}
fns = {}
for name, (g, inner, w, h) in cases.items():
    fns[name] = (lambda g=g, inner=inner, w=w, h=h, name=name:
                 K.period_stats(X, bounds, group=g, inner=inner, window=w, thr=h, seg=SEG, out=outs[name]))
out_walk = torch.empty((8, 1, m), dtype=torch.float64, device=dev)
fns["walk-g24-max-w1"] = lambda: walk(24, "max", 1, out_walk)
count = torch.zeros(m, dtype=torch.int32, device=dev)
fns["k20-count"] = lambda: K.row_missing_count(X, out=count)


def same(p, q):
    return bool(((p == q) | (p.isnan() & q.isnan())).all())


ref = fns["split-g24-max-w1"]().clone()
assert same(ref, walk(24, "max", 1, out_walk)), "split and walk differ"
for seg in (8, SEGMENT, 365):
    assert same(ref[:5], K.period_stats(X, bounds, group=24, inner="max", seg=seg)[:5]), f"seg = {seg} differs"
torch_equal = None
if a.torch:
    assert T % 24 == 0
    for w, name in ((1, "split-g24-max-w1"), (5, "split-g24-sum-w5")):
        n, top, arg = composition(w)
        got = fns[name]()
        has = n > 0
        torch_equal = bool((got[0, 0] == n).all() and (got[2, 0][has] == arg[has]).all()
                           and (w > 1 or (got[1, 0][has] == top[has]).all()))
        assert torch_equal, f"the torch composition and the kernel differ at w = {w}"
        del n, top, arg
    fns["torch-max-w1"] = lambda: composition(1)
    fns["torch-sum-w5"] = lambda: composition(5)
facts = {"rows_with_a_missing_day": int((ref[0, 0] < T // 24).sum()), "mean_max": float(ref[1, 0].nanmean())}

ms, calls = measure(fns)
med = {name: statistics.median(v) for name, v in ms.items()}
nbytes = 4 * m * T
versus = {"split-g24-max-w1": "torch-max-w1", "split-g24-sum-w5": "torch-sum-w5"}
lines = []
for name in fns:
    g, inner, w, h = cases.get(name, (24, "max", 1, None) if name.startswith("walk") else (None, None, None, None))
    other = versus.get(name)
    line = {"bench": "extremes", "variant": name, "m": m, "T": T, "seg_days": SEG, "group": g, "inner": inner, "window": w,
            "thr": h is not None, "split_walk_seg_equal": True, "torch_equal": torch_equal, **facts,
            "calls_per_sample": calls[name], "median_ms": med[name], "min_ms": min(ms[name]), "max_ms": max(ms[name]),
            "GBps": nbytes / med[name] / 1e6, "of_hbm_peak": nbytes / med[name] / 1e9 / HBM_TBS,
            "of_k20_rate": med["k20-count"] / med[name],
            "speedup_vs_torch": med[other] / med[name] if other in med else None}
    if name == "split-g24-max-w1" and other in med:
        line["not_slower_than_torch"] = bool(med[name] <= med[other])
    lines.append(line)
    print(json.dumps(line), flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
