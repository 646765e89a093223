"""K25 (dmdx_clim_quantile_f32) alone, on one cfg2 row block, against the torch composition and against K18's mean.

X is one resident row block, 129 780 rows x 8760 hourly snapshots of 2019 (4.55 GB fp32).  For kind = "hour" (24 slots
of 365 members) and "dayofyear" with window_days = 2 (366 slots of about 120), at J = 1 (q = 0.9) and J = 4
(q = 0.1, 1/3, 2/3, 0.9), in ONE process and alternating:
  k25           kern.clim_quantile(X, order, start, q)                   the members staged in LDS, one read of X
  k25_streamed  kern.clim_quantile(..., streamed=True)                   the members re-read in every step
  torch         per slot: X[order[a:b]] -> torch.sort(dim=0) -> the two rows -> the fp64 interpolation
  clim_mean     kern.clim_mean(X, order, start)                          the one-read floor of the same lists
Conditions, asserted before anything is timed: the staged and the streamed body give equal bits, and both give the
bits of the composition (the data are positive and finite: the float order is the key order).  Times are HIP events
around batches of calls on the current stream (>= `--sample-ms` of device time per sample), `--reps` samples after
`--warmup` calls; medians with min .. max.  One JSON line per variant, also appended to
profiles/k25_bench_quantile.jsonl; the process fails when K25 (staged) is not faster than the composition beyond the
composition's own min .. max spread.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dmd_era5_amd.climatology import slots_of  # noqa: E402
from dmd_era5_amd.kernels import default_kernels  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--m", type=int, default=129780, help="rows of the block")
ap.add_argument("--T", type=int, default=8760, help="hourly snapshots from 2019-01-01T00")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--sample-ms", type=float, default=20.0)
ap.add_argument("--no-streamed", action="store_true", help="leave the streamed body out (it is slow by design)")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                             "k25_bench_quantile.jsonl"),
                help="the JSON lines are appended to this file too ('' switches that off)")
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_quantile: no GPU visible (a CPU run measures nothing)")
K = default_kernels()
dev = torch.device("cuda")
m, T = a.m, a.T
times = np.datetime64("2019-01-01T00", "h") + np.arange(T) * np.timedelta64(1, "h")
X = torch.empty((T, m), dtype=torch.float32, device=dev)
gen = torch.Generator(device=dev).manual_seed(25)
for t0 in range(0, T, 1024):                                     # positive values, a few hundred: temperatures
    X[t0:t0 + 1024].normal_(270.0, 15.0, generator=gen)


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


def composition(order64, start_h, qs):
    """(J, S, m) fp32 by gather, full sort and the contract's interpolation, slot by slot."""
    S = len(start_h) - 1
    out = torch.full((len(qs), S, m), float("nan"), dtype=torch.float32, device=dev)
    for s in range(S):
        lo, hi = int(start_h[s]), int(start_h[s + 1])
        n = hi - lo
        if n == 0:
            continue
        srt = torch.sort(X[order64[lo:hi]], dim=0).values
        for j, q in enumerate(qs):
            h = np.float64(q) * np.float64(n - 1)
            i, g = int(np.floor(h)), float(h - np.floor(h))
            if g == 0.0:
                out[j, s] = srt[i]
            else:
                lo64, hi64 = srt[i].double(), srt[i + 1].double()
                out[j, s] = (lo64 + (hi64 - lo64) * g).float()
    return out


lines, missed = [], []
for kind, window in (("hour", 0), ("dayofyear", 2)):
    _, order_h, start_h, S = slots_of(times, kind, window)
    order, start = torch.from_numpy(order_h).to(dev), torch.from_numpy(start_h).to(dev)
    order64 = order.long()
    n_max = int(np.diff(start_h).max())
    floor_ms, _ = measure({"clim_mean": lambda: K.clim_mean(X, order, start)})
    floor = statistics.median(floor_ms["clim_mean"])
    for qs in ((0.9,), (0.1, 1.0 / 3.0, 2.0 / 3.0, 0.9)):
        J = len(qs)
        fns = {"k25": lambda: K.clim_quantile(X, order, start, qs),
               "torch": lambda: composition(order64, start_h, qs)}
        if not a.no_streamed:
            fns["k25_streamed"] = lambda: K.clim_quantile(X, order, start, qs, streamed=True)
        ref = fns["torch"]().view(torch.int32)
        same = {name: bool(torch.equal(fn().view(torch.int32), ref)) for name, fn in fns.items() if name != "torch"}
        assert all(same.values()), f"{kind} J={J}: K25 does not give the bits of the composition: {same}"
        ms, calls = measure(fns)
        med = {name: statistics.median(v) for name, v in ms.items()}
        for name in list(fns) + ["clim_mean"]:
            v = floor_ms["clim_mean"] if name == "clim_mean" else ms[name]
            line = {"bench": "quantile", "variant": name, "kind": kind, "window_days": window, "S": S, "n_s_max": n_max,
                    "J": J, "m": m, "T": T, "bit_equal_to_composition": True, "median_ms": statistics.median(v),
                    "min_ms": min(v), "max_ms": max(v), "x_clim_mean": statistics.median(v) / floor}
            if name != "clim_mean":
                line["calls_per_sample"] = calls[name]
                line["speedup_vs_torch"] = med["torch"] / med[name]
            lines.append(line)
            print(json.dumps(line), flush=True)
        print(f"# {kind} (window {window}) J={J}: K25 {med['k25']:.2f} ms, the composition {min(ms['torch']):.2f} .. "
              f"{max(ms['torch']):.2f} ms, clim_mean {floor:.2f} ms", flush=True)
        if not max(ms["k25"]) < min(ms["torch"]):
            missed.append(f"{kind} J={J}: K25 {max(ms['k25']):.2f} ms is not below the composition's {min(ms['torch']):.2f} ms")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
if missed:
    sys.exit("bench_quantile: the bar is missed: " + "; ".join(missed))
