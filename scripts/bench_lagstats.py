"""K26 (dmdx_lag_moments_f32) alone, on one cfg2 row block, against the torch composition and its neighbours.

X is one resident row block, 129 780 rows x 8760 hourly snapshots (4.55 GB fp32).  For L = 2 and L = 8 lags, in ONE
process and alternating:
  ring         kern.lag_moments(X, 1 .. L)                 the earlier member of a pair from the lane's LDS ring
  reload-near  the same lags with ring=False               (flags bit 0: a second load per lag and snapshot)
  reload-far   the lags 24, 48, ..., 24 L                  beyond the ring: always loaded again
  ring-NAME    the ring variant of another build of the library (``--alt-lib NAME=PATH``: the rings of 8 and of 32
               snapshots, ``make -C dmd_era5_amd/csrc lag-rings``)
  torch        Xd = X.double(); per lag (Xd[:-tau] * Xd[tau:]).sum(0), and the squares   (``--torch``: 9.1 GB more)
  k21-fit-p6   kern.treg_fit(X, W, SEGMENT) with 6 columns, k18-mean: kern.clim_mean(X, hour slots)
               the one-read kernels next door, in the same session
Conditions, asserted before anything is timed: ring and reload give equal bits for the same lags; every build of the
library gives the bits of the product; against torch, which sums in another order, S and P agree within
2 T 2^-53 S.  Times are HIP events around batches of calls on the current stream (>= ``--sample-ms`` of device time per
sample), ``--reps`` samples after ``--warmup`` calls; medians, minimum and maximum, with GB/s of one read of X and the
fraction of the 6.3 TB/s HBM figure of DESIGN.md that is.  One JSON line per variant; ``--out FILE`` appends them to a
file too (profiles/k26_bench_lagstats.jsonl holds the run MEASUREMENTS.md cites and is not written by default).  No bar
is set: nobody has measured this kernel before.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dmd_era5_amd import _lib  # noqa: E402
from dmd_era5_amd.baseline import SEGMENT  # noqa: E402
from dmd_era5_amd.climatology import slots_of  # noqa: E402
from dmd_era5_amd.kernels import HipKernels, default_kernels  # noqa: E402
from dmd_era5_amd.trend import design, weights  # noqa: E402

HBM_TBS = 6.3

ap = argparse.ArgumentParser()
ap.add_argument("--m", type=int, default=129780, help="rows of the block")
ap.add_argument("--T", type=int, default=8760, help="hourly snapshots from 2019-01-01T00")
ap.add_argument("--L", type=int, nargs="+", default=[2, 8], help="numbers of lags")
ap.add_argument("--alt-lib", nargs="*", default=[], metavar="NAME=PATH", help="other builds of the library to time")
ap.add_argument("--torch", action="store_true", help="time the torch composition too (an fp64 copy of X)")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--sample-ms", type=float, default=20.0)
ap.add_argument("--out", default="", help="append the JSON lines to this file too (default: print only)")
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_lagstats: no GPU visible (a CPU run measures nothing)")
K = default_kernels()
alts = {}
for item in a.alt_lib:
    name, path = item.split("=", 1)
    lib = ctypes.CDLL(os.path.abspath(path))
    for sym in ("dmdx_lag_moments_max_lags", "dmdx_lag_moments_ring", "dmdx_lag_moments_workspace_bytes",
                "dmdx_lag_moments_f32"):
        getattr(lib, sym).restype, getattr(lib, sym).argtypes = _lib.SIGNATURES[sym]
    alts[name] = HipKernels(lib=lib)
dev = torch.device("cuda")
m, T = a.m, a.T
X = torch.empty((T, m), dtype=torch.float32, device=dev)
gen = torch.Generator(device=dev).manual_seed(26)
for t0 in range(0, T, 1024):                                     # anomalies of a few units: the bits depend on the order
    X[t0:t0 + 1024].normal_(0.0, 3.0, generator=gen)
times = np.datetime64("2019-01-01T00", "h") + np.arange(T) * np.timedelta64(1, "h")


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


def bits(t):
    return t.view(torch.int64)


origin = times[0] + (times[-1] - times[0]) // 2
half = float((times[-1] - origin) / np.timedelta64(1, "D"))
W6 = torch.from_numpy(weights(design(times, origin, half, 1, 2))).to(dev)
order_h, start_h = slots_of(times, "hour")[1:3]
order, start = torch.from_numpy(order_h).to(dev), torch.from_numpy(start_h).to(dev)

lines = []
for L in a.L:
    near, far = list(range(1, L + 1)), [24 * k for k in range(1, L + 1)]
    out = torch.empty((1 + 3 * L, m), dtype=torch.float64, device=dev)
    fns = {"ring": lambda: K.lag_moments(X, near, seg=SEGMENT, out=out),
           "reload-near": lambda: K.lag_moments(X, near, seg=SEGMENT, out=out, ring=False),
           "reload-far": lambda: K.lag_moments(X, far, seg=SEGMENT, out=out)}
    for name, Ka in alts.items():
        fns[f"ring-{name}"] = (lambda Ka=Ka: Ka.lag_moments(X, near, seg=SEGMENT, out=out))
    ref = K.lag_moments(X, near, seg=SEGMENT)
    same = bool(torch.equal(bits(ref), bits(K.lag_moments(X, near, seg=SEGMENT, ring=False))))
    assert same, f"L = {L}: ring and reload give different bits"
    for name, Ka in alts.items():
        assert torch.equal(bits(ref), bits(Ka.lag_moments(X, near, seg=SEGMENT))), f"L = {L}: build {name} differs"
    rings = {"ring": K.lag_ring, **{f"ring-{name}": Ka.lag_ring for name, Ka in alts.items()}}
    err = None
    if a.torch:
        def t_comp():
            Xd = X.double()
            res = [(Xd * Xd).sum(dim=0)]
            for tau in near:
                res.append((Xd[:T - tau] * Xd[tau:]).sum(dim=0))
            return torch.stack(res)

        want = t_comp()
        err = float(((ref[:1 + L] - want).abs() / (2.0 * T * 2.0 ** -53 * ref[0])[None]).max())
        assert err <= 1.0, f"L = {L}: S and P are {err:.3g} of the bound away from the torch composition"
        del want
        fns["torch"] = t_comp
    fns["k21-fit-p6"] = lambda: K.treg_fit(X, W6, SEGMENT)
    fns["k18-mean"] = lambda: K.clim_mean(X, order, start)
    ms, calls = measure(fns)
    med = {name: statistics.median(v) for name, v in ms.items()}
    nbytes = 4 * m * T
    for name in fns:
        line = {"bench": "lagstats", "variant": name, "L": L, "lags": far if name == "reload-far" else near, "m": m, "T": T,
                "seg": SEGMENT, "ring_slots": rings.get(name), "ring_reload_bit_equal": same, "err_of_bound_vs_torch": err,
                "calls_per_sample": calls[name], "median_ms": med[name], "min_ms": min(ms[name]), "max_ms": max(ms[name]),
                "GBps": nbytes / med[name] / 1e6, "of_hbm_peak": nbytes / med[name] / 1e9 / HBM_TBS,
                "speedup_vs_torch": med["torch"] / med[name] if "torch" in med else None}
        lines.append(line)
        print(json.dumps(line), flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
