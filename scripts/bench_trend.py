"""K21 (dmdx_treg_fit_f32 / dmdx_treg_apply_f32) alone, on one cfg2 row block, against the torch compositions.

X is one resident row block, 129 780 rows x 8760 hourly snapshots of 2019 (4.55 GB fp32).  For p = 2 (intercept and
linear trend) and p = 6 (+ two annual harmonics), in ONE process and alternating:
  fit    k21-split  kern.treg_fit(X, W, SEGMENT) with time cut over workgroups (a workspace of segment sums)
         k21-walk   the same call with one lane per row walking its segments       (the same bits, asserted)
         torch      (W @ X.double()).float()                                       (an fp64 copy of X: 9.1 GB)
  apply  k21        kern.treg_apply_(X, D, coef)                                   in place
         torch      X.sub_((D @ coef.double()).float())                            (a (T, m) fp64 and an fp32 field)
Conditions, asserted before anything is timed: the two forms of the fit give equal bits; against torch, which sums in
another order, the coefficients agree within 2 T^2 2^-53 max|W| max|x| + 2^-23 |c| (two fp64 sums of T products, two
roundings to fp32) and the anomalies within 2^-23 (max|f| + max|y|) (torch rounds f to fp32 first).  Times are HIP
events around batches of calls on the current stream (>= `--sample-ms` of device time per sample), `--reps` samples
after `--warmup` calls; medians, minimum and maximum, with GB/s of the bytes the operation needs (fit: one read of X;
apply: one read and one write) and the fraction of the 6.3 TB/s HBM figure of DESIGN.md that is.  One JSON line per
variant, also appended to profiles/k21_bench_trend.jsonl.  No bar is set: nobody has measured this kernel before.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dmd_era5_amd.kernels import HipKernels, default_kernels  # noqa: E402
from dmd_era5_amd.trend import SEGMENT, design, weights  # noqa: E402

HBM_TBS = 6.3

ap = argparse.ArgumentParser()
ap.add_argument("--m", type=int, default=129780, help="rows of the block")
ap.add_argument("--T", type=int, default=8760, help="hourly snapshots from 2019-01-01T00")
ap.add_argument("--p", type=int, nargs="+", default=[2, 6], choices=[2, 4, 6, 8], help="columns: 2 + annual harmonics")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--sample-ms", type=float, default=20.0)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                             "k21_bench_trend.jsonl"),
                help="the JSON lines are appended to this file too ('' switches that off)")
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_trend: no GPU visible (a CPU run measures nothing)")
K = default_kernels()
K.treg_split = True
Kwalk = HipKernels()
Kwalk.treg_split = False
dev = torch.device("cuda")
m, T = a.m, a.T
times = np.datetime64("2019-01-01T00", "h") + np.arange(T) * np.timedelta64(1, "h")
origin = times[0] + (times[-1] - times[0]) // 2
half = float((times[-1] - origin) / np.timedelta64(1, "D"))
X = torch.empty((T, m), dtype=torch.float32, device=dev)
gen = torch.Generator(device=dev).manual_seed(21)
for t0 in range(0, T, 1024):                                     # positive values, a few hundred: temperatures
    X[t0:t0 + 1024].normal_(270.0, 15.0, generator=gen)
Xk, Xt = X.clone(), X.clone()
xmax = float(X.abs().max())


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


lines = []
for p in a.p:
    Dh = design(times, origin, half, 1, (p - 2) // 2)
    Wh = weights(Dh)
    D, W = torch.from_numpy(Dh).to(dev), torch.from_numpy(Wh).to(dev)

    def k_split():
        return K.treg_fit(X, W, SEGMENT)

    def k_walk():
        return Kwalk.treg_fit(X, W, SEGMENT)

    def t_fit():
        return (W @ X.double()).float()

    coef = k_split()
    same = bool(torch.equal(coef.view(torch.int32), k_walk().view(torch.int32)))
    assert same, f"p = {p}: the two forms of the fit give different bits"
    c64 = W @ X.double()
    bound = 2.0 * T * T * 2.0 ** -53 * float(W.abs().max()) * xmax + 2.0 ** -23 * c64.abs()
    fit_err = float(((coef.double() - c64).abs() / bound).max())
    assert fit_err <= 1.0, f"p = {p}: the coefficients are {fit_err:.3g} of the bound away from W @ X.double()"
    del c64, bound

    def k_apply():
        return K.treg_apply_(Xk, D, coef)

    def t_apply():
        return Xt.sub_((D @ coef.double()).float())

    Xk.copy_(X)
    Xt.copy_(X)
    k_apply()
    t_apply()
    torch.cuda.synchronize()
    fmax = float((D @ coef.double()).abs().max())
    apply_err = float((Xk - Xt).abs().max()) / (2.0 ** -23 * (fmax + float(Xk.abs().max())))
    assert apply_err <= 1.0, f"p = {p}: the anomalies are {apply_err:.3g} of the bound away from the torch composition"

    for op, fns, nbytes in (("fit", {"k21-split": k_split, "k21-walk": k_walk, "torch": t_fit}, 4 * m * T),
                            ("apply", {"k21": k_apply, "torch": t_apply}, 8 * m * T)):
        ms, calls = measure(fns)
        med = {name: statistics.median(v) for name, v in ms.items()}
        for name in fns:
            line = {"bench": "trend", "op": op, "variant": name, "p": p, "m": m, "T": T, "seg": SEGMENT,
                    "fit_forms_bit_equal": same, "fit_err_of_bound": fit_err, "apply_err_of_bound": apply_err,
                    "calls_per_sample": calls[name], "median_ms": med[name], "min_ms": min(ms[name]),
                    "max_ms": max(ms[name]), "GBps": nbytes / med[name] / 1e6,
                    "of_hbm_peak": nbytes / med[name] / 1e9 / HBM_TBS, "speedup_vs_torch": med["torch"] / med[name]}
            lines.append(line)
            print(json.dumps(line), flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
