"""K22 (dmdx_tfilt_f32) alone, on one cfg2 row block, against the torch compositions.

X is one resident row block, 129 780 rows x 8760 hourly snapshots of 2019 (4.55 GB fp32).  Three cases, in ONE process,
the variants of a case alternating:
  daily   the daily mean, L = stride = 24                                   -> 365 outputs
            k22       kern.tfilt(X, boxcar(24), 24)
            torch     X.view(365, 24, m).double().mean(1).float()            (an fp64 copy of X: 9.1 GB)
            k18-mean  kern.clim_mean(X, ...) for kind = "hour": the nearest existing kernel, one read of X with an fp64
                      chain per row -- the yardstick for the rate, not a baseline
  lp-day  the 10-day Lanczos low-pass (f_c = 1 / 240, n = 480, L = 961) with daily output, stride 24 -> 325 outputs
  lp-1    the same taps at stride 1                                          -> 7800 outputs
            k22       kern.tfilt(X, taps, stride)
            addcmul   acc (T_out, m) fp64 = 0; for every tap acc.addcmul_(X[j : j + span : stride].double(), h[j]):
                      the baseline of the two filters.  (An fp32 conv2d of X as a (1, 1, T, m) image with an (L, 1)
                      kernel was the second candidate; its first call on this image did not return within seven
                      minutes on an MI355X and the cause was not found, so it is not part of this script:
                      MEASUREMENTS.md, "K22".)
Conditions, asserted before anything is timed: on the first `--check-rows` rows the kernel gives the bits of
tests/tfilt_ref.py; against the torch results, which sum in another order, it agrees within
2^-23 |y| + 2 L 2^-53 sum|h| max|x| (one rounding to fp32 each, two fp64 sums of L products).  Times are HIP events
around batches of calls on the current stream (>= `--sample-ms` of device time per sample), `--reps` samples (`--torch-reps` for the
compositions that take seconds per call) after `--warmup` calls; medians, minimum and maximum, with GB/s of the bytes
the operation needs (the snapshots some window addresses, read once, and Y written once) and the fraction of the
6.3 TB/s HBM figure of DESIGN.md that is; for the filters also the separately rounded fp64 multiply-add pairs per
second.  One JSON line per variant, also appended to profiles/k22_bench_tfilt.jsonl.  No bar is set: nobody has
measured this kernel before.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tfilt_ref  # noqa: E402
from dmd_era5_amd.climatology import slots_of  # noqa: E402
from dmd_era5_amd.kernels import default_kernels  # noqa: E402
from dmd_era5_amd.timefilter import TimeFilter  # noqa: E402

HBM_TBS = 6.3
T_START = time.time()


def note(msg):
    """Progress on stderr: the compositions of the stride-1 case take seconds per call."""
    print(f"# [{time.time() - T_START:7.1f} s] {msg}", file=sys.stderr, flush=True)


ap = argparse.ArgumentParser()
ap.add_argument("--m", type=int, default=129780, help="rows of the block")
ap.add_argument("--T", type=int, default=8760, help="hourly snapshots from 2019-01-01T00 (whole days)")
ap.add_argument("--cases", nargs="+", default=["daily", "lp-day", "lp-1"], choices=["daily", "lp-day", "lp-1"])
ap.add_argument("--cutoff-days", type=float, default=10.0)
ap.add_argument("--no-torch", action="store_true", help="time the kernel alone (a second build of it, say)")
ap.add_argument("--check-rows", type=int, default=96)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--torch-reps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--sample-ms", type=float, default=20.0)
ap.add_argument("--tag", default="", help="copied into every line (the build that was measured)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k22_bench_tfilt.jsonl"),
                help="the JSON lines are appended to this file too ('' switches that off)")
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_tfilt: no GPU visible (a CPU run measures nothing)")
K = default_kernels()
dev = torch.device("cuda")
m, T = a.m, a.T
assert T % 24 == 0, "whole days of hourly snapshots"
times = np.datetime64("2019-01-01T00", "h") + np.arange(T) * np.timedelta64(1, "h")
X = torch.empty((T, m), dtype=torch.float32, device=dev)
gen = torch.Generator(device=dev).manual_seed(22)
for t0 in range(0, T, 1024):                                     # positive values, a few hundred: temperatures
    X[t0:t0 + 1024].normal_(270.0, 15.0, generator=gen)
xmax = float(X.abs().max())
Xsub = X[:, :a.check_rows].cpu().numpy().T.copy()


def batch_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def measure(fns, slow=()):
    calls = {}
    for name, fn in fns.items():
        for _ in range(a.warmup):
            fn()
        calls[name] = max(1, int(a.sample_ms / max(batch_ms(fn, 1), 1e-3)))
    ms = {name: [] for name in fns}
    for rep in range(a.reps):                                    # alternating: all see the same machine
        for name, fn in fns.items():
            if name not in slow or rep < a.torch_reps:
                ms[name].append(batch_ms(fn, calls[name]))
    return ms, calls


def check_bits(Y, taps, stride, case):
    want = tfilt_ref.tfilt(Xsub, taps, stride)
    got = Y[:, :a.check_rows].cpu().numpy().T
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{case}: not the bits of tests/tfilt_ref.py"


lines = []
for case in a.cases:
    if case == "daily":
        tf = TimeFilter.block_mean(times)
    else:
        tf = TimeFilter.lowpass(times, a.cutoff_days, every_days=1.0 if case == "lp-day" else None)
    L, stride, n_out = tf.n_taps, tf.stride, tf.n_out(T)
    h = torch.from_numpy(tf.taps).to(dev)
    habs = float(np.abs(tf.taps).sum())
    span = (n_out - 1) * stride + 1
    Y = torch.empty((n_out, m), dtype=torch.float32, device=dev)

    def k22():
        return K.tfilt(X, h, stride, out=Y)

    note(f"{case}: L = {L}, stride = {stride}, {n_out} outputs; first launch")
    k22()
    torch.cuda.synchronize()
    note(f"{case}: launched; the bits of tests/tfilt_ref.py on {a.check_rows} rows")
    check_bits(Y, tf.taps, stride, case)
    ymax = float(Y.abs().max())
    fns, slow, errs = {"k22": k22}, set(), {}
    tol64 = 2.0 ** -23 * ymax + 2.0 * L * 2.0 ** -53 * habs * xmax

    if case == "daily":
        order_h, start_h = slots_of(times, "hour")[1:3]
        order, start = torch.from_numpy(order_h).to(dev), torch.from_numpy(start_h).to(dev)
        fns["k18-mean"] = lambda: K.clim_mean(X, order, start)
        if not a.no_torch:
            def t_mean():
                return X.view(n_out, 24, m).double().mean(1).float()

            errs["torch"] = float((t_mean() - Y).abs().max()) / tol64
            fns["torch"] = t_mean
    elif not a.no_torch:
        acc = torch.empty((n_out, m), dtype=torch.float64, device=dev)
        taps0d = [h[j] for j in range(L)]

        def t_addcmul():
            acc.zero_()
            for j in range(L):
                acc.addcmul_(X[j:j + span:stride].double(), taps0d[j])
            return acc.float()

        note(f"{case}: the addcmul composition")
        errs["addcmul"] = float((t_addcmul() - Y).abs().max()) / tol64
        fns["addcmul"] = t_addcmul
        slow.add("addcmul")
    for name, err in errs.items():
        assert err <= 1.0, f"{case}: {name} is {err:.3g} of the bound away from the kernel"

    note(f"{case}: timing {list(fns)}")
    ms, calls = measure(fns, slow)
    med = {name: statistics.median(v) for name, v in ms.items()}
    base = min((med[n] for n in med if n not in ("k22", "k18-mean")), default=None)
    used = (n_out - 1) * stride + L if stride <= L else n_out * L      # snapshots some window addresses
    nbytes = 4 * m * used + 4 * m * n_out
    for name in fns:
        nb = 4 * m * T + 4 * 24 * m if name == "k18-mean" else nbytes
        line = {"bench": "tfilt", "case": case, "variant": name, "L": L, "stride": stride, "T_out": n_out, "m": m, "T": T,
                "bits_equal_ref_rows": a.check_rows, "err_of_bound": errs.get(name), "calls_per_sample": calls[name],
                "samples": len(ms[name]), "median_ms": med[name], "min_ms": min(ms[name]), "max_ms": max(ms[name]),
                "GBps": nb / med[name] / 1e6, "of_hbm_peak": nb / med[name] / 1e9 / HBM_TBS,
                "speedup_vs_baseline": None if base is None else base / med[name], "tag": a.tag}
        if case != "daily":
            line["fp64_pairs_per_s"] = float(m) * n_out * L / (med[name] * 1e-3)
        lines.append(line)
        print(json.dumps(line), flush=True)
    del Y, fns
    if case != "daily" and not a.no_torch:
        del acc
    torch.cuda.empty_cache()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
