"""K18 (dmdx_clim_mean_f32 / dmdx_clim_std_f32 / dmdx_clim_apply_f32) alone, on one cfg2 row block, against the torch
composition.

X is one resident row block, 129 780 rows x 8760 hourly snapshots of 2019 (4.55 GB fp32).  For kind = "hour" (S = 24)
and "month_hour" (S = 288), in ONE process and alternating:
  mean   k18    kern.clim_mean(X, order, start)
         torch  torch.zeros(S, m, fp64).index_add_(0, slot, X.double()) / n          (an fp64 copy of X: 9.1 GB)
  apply  k18    kern.clim_apply_(X, slot, mean)                                      in place
         torch  X[t0:t1].sub_(mean[slot[t0:t1]]) in time chunks of --chunk snapshots (a gathered second X per chunk)
  std    k18    kern.clim_std(X, order, start, mean)                                 (no counterpart: reported only)
Conditions, asserted before anything is timed: apply gives equal bits on both sides; the means differ by at most
1 fp32 ulp (index_add_ sums in another order than the list).  Times are HIP events around batches of calls on the
current stream (>= `--sample-ms` of device time per sample), `--reps` samples after `--warmup` calls; medians, with
TB/s of the bytes the operation needs (mean, std: one read of X; apply: one read and one write) and the fraction of
the 6.3 TB/s HBM figure of DESIGN.md that is.  One JSON line per variant, also appended to profiles/k18_bench_clim.jsonl; the process fails when K18 is not at
least `--bar` (1.5) times faster than the composition on mean or apply.
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

HBM_TBS = 6.3

ap = argparse.ArgumentParser()
ap.add_argument("--m", type=int, default=129780, help="rows of the block")
ap.add_argument("--T", type=int, default=8760, help="hourly snapshots from 2019-01-01T00")
ap.add_argument("--kinds", nargs="+", default=["hour", "month_hour"])
ap.add_argument("--chunk", type=int, default=1024, help="snapshots per chunk of the torch apply")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--sample-ms", type=float, default=20.0)
ap.add_argument("--bar", type=float, default=1.5)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                             "k18_bench_clim.jsonl"),
                help="the JSON lines are appended to this file too ('' switches that off)")
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_clim: no GPU visible (a CPU run measures nothing)")
K = default_kernels()
dev = torch.device("cuda")
m, T = a.m, a.T
times = np.datetime64("2019-01-01T00", "h") + np.arange(T) * np.timedelta64(1, "h")
X = torch.empty((T, m), dtype=torch.float32, device=dev)
gen = torch.Generator(device=dev).manual_seed(18)
for t0 in range(0, T, 1024):                                     # positive values, a few hundred: temperatures
    X[t0:t0 + 1024].normal_(270.0, 15.0, generator=gen)
Xk, Xt = X.clone(), X.clone()


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
    for _ in range(a.reps):                                      # alternating: both see the same machine
        for name, fn in fns.items():
            ms[name].append(batch_ms(fn, calls[name]))
    return ms, calls


lines, missed = [], []
for kind in a.kinds:
    slot_h, order_h, start_h, S = slots_of(times, kind)
    slot, order, start = (torch.from_numpy(v).to(dev) for v in (slot_h, order_h, start_h))
    slot64 = slot.long()
    n = torch.from_numpy(np.diff(start_h.astype(np.int64))).to(dev).double()[:, None]

    def k_mean():
        return K.clim_mean(X, order, start)

    def t_mean():
        return (torch.zeros((S, m), dtype=torch.float64, device=dev).index_add_(0, slot64, X.double()) / n).float()

    mean = k_mean()
    ulps = (mean.view(torch.int32) - t_mean().view(torch.int32)).abs()
    live = (n > 0).expand(S, m)
    max_ulp = int(ulps[live].max())
    assert max_ulp <= 1, f"{kind}: the means differ by {max_ulp} fp32 ulp"

    def k_apply():
        return K.clim_apply_(Xk, slot, mean)

    def t_apply():
        for t0 in range(0, T, a.chunk):
            Xt[t0:t0 + a.chunk].sub_(mean[slot64[t0:t0 + a.chunk]])

    Xk.copy_(X)
    Xt.copy_(X)
    k_apply()
    t_apply()
    torch.cuda.synchronize()
    same = bool(torch.equal(Xk.view(torch.int32), Xt.view(torch.int32)))
    assert same, f"{kind}: apply does not give the bits of X.sub_(mean[slot])"

    def k_std():
        return K.clim_std(X, order, start, mean)

    for op, fns, nbytes in (("mean", {"k18": k_mean, "torch": t_mean}, 4 * m * T),
                            ("apply", {"k18": k_apply, "torch": t_apply}, 8 * m * T),
                            ("std", {"k18": k_std}, 4 * m * T)):
        ms, calls = measure(fns)
        med = {name: statistics.median(v) for name, v in ms.items()}
        for name in fns:
            line = {"bench": "clim", "op": op, "variant": name, "kind": kind, "S": S, "m": m, "T": T,
                    "apply_bit_equal": same, "mean_max_ulp": max_ulp, "calls_per_sample": calls[name],
                    "median_ms": med[name], "min_ms": min(ms[name]), "max_ms": max(ms[name]),
                    "TBps": nbytes / med[name] / 1e9, "of_hbm_peak": nbytes / med[name] / 1e9 / HBM_TBS}
            if "torch" in fns:
                line["speedup_vs_torch"] = med["torch"] / med[name]
            lines.append(line)
            print(json.dumps(line), flush=True)
        if "torch" in fns:
            ratio = med["torch"] / med["k18"]
            print(f"# {kind} {op}: K18 is {ratio:.2f}x the torch composition", flush=True)
            if ratio < a.bar:
                missed.append(f"{kind} {op}: {ratio:.2f}x < {a.bar}x")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
if missed:
    sys.exit("bench_clim: the bar is missed: " + "; ".join(missed))
