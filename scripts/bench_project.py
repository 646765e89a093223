"""K13 (project) on one cfg2 row block against what the library could do before it.

For k in {10, 50, 200} and T in {24, 729, 8760}, m = 129 780 rows, in ONE process and alternating:
  new   kern.project(Ut, Xt, mean, std)                               X read once, no temporary
  old   Xs = (Xt - mean) / std  (a torch temporary the size of X), kern.gemm_tn(Ut, Xs)  (K3),
        (Xs * Xs).sum per snapshot
Times are HIP events around batches of calls (>= `--sample-ms` of device time each, per call reported) on
the current stream, `--reps` samples after `--warmup` calls; median and the spread (min .. max) of both are
printed, with the fraction of max(bytes / 6.3 TB/s, flops / 157.3 TFLOP/s) each median reaches (bytes: X once
plus U; flops: 2 m k T) and the core clock the new kernel held (in-kernel stamps of dmdx_set_clock_probe,
taken in a launch of its own).  One JSON line per (k, T).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dmd_era5_amd.kernels import default_kernels  # noqa: E402

HBM_TBS, MFMA_TFLOPS = 6.3, 157.3

ap = argparse.ArgumentParser()
ap.add_argument("--m", type=int, default=129780)
ap.add_argument("--ks", type=int, nargs="+", default=[10, 50, 200])
ap.add_argument("--Ts", type=int, nargs="+", default=[24, 729, 8760])
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--sample-ms", type=float, default=20.0, help="device time one timed sample should cover")
ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_project: no GPU visible (a CPU run measures nothing)")
K = default_kernels()
dev = torch.device("cuda")
g = torch.Generator(device="cuda").manual_seed(13)
m = a.m


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    return e0, e1, r


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def clock_mhz(fn):
    c = torch.zeros(3, dtype=torch.int64, device=dev)
    K.clock_probe(c)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        K.clock_probe(None)
    cyc, ref, _ = (int(v) for v in c.tolist())
    return 100.0 * cyc / ref if ref else float("nan")


lines = []
for T in a.Ts:
    # un-centred data, as a raw ERA5 temperature slice: 280 + O(10)
    Xt = torch.randn((T, m), generator=g, device=dev, dtype=torch.float32).mul_(10.0).add_(280.0)
    mean = torch.randn(m, generator=g, device=dev, dtype=torch.float32).mul_(3.0).add_(280.0)
    std = torch.rand(m, generator=g, device=dev, dtype=torch.float32).mul_(10.0).add_(5.0)
    for k in a.ks:
        Ut = torch.randn((k, m), generator=g, device=dev, dtype=torch.float32)

        def new():
            return K.project(Ut, Xt, mean, std)

        def old():
            Xs = (Xt - mean) / std
            return K.gemm_tn(Ut, Xs), (Xs * Xs).sum(dim=1, dtype=torch.float64)

        flops = 2.0 * m * k * T
        nbytes = 4.0 * m * T + 4.0 * m * k
        bound_ms = max(nbytes / (HBM_TBS * 1e12), flops / (MFMA_TFLOPS * 1e12)) * 1e3
        for _ in range(a.warmup):
            new(), old()
        (Cn, en), (Co, eo) = new(), old()
        torch.cuda.synchronize()
        # the two ways agree on what they compute (fp32 sums in different orders)
        dev_rel = {"C": float((Cn - Co).abs().max() / Co.abs().max()), "energy": float(((en - eo).abs() / eo).max())}
        del Cn, en, Co, eo
        # a sample is a batch of calls between two events, long enough (>= --sample-ms of device time)
        # that launch gaps and the event pair do not show; the batch size comes from one timed call
        batch = {}
        for w, fn in (("new", new), ("old", old)):
            e0, e1, _ = timed(fn)
            torch.cuda.synchronize()
            batch[w] = max(1, min(500, int(a.sample_ms / max(e0.elapsed_time(e1), 1e-3)) + 1))

        def many(fn, nb):
            for _ in range(nb):
                fn()

        ev = {"new": [], "old": []}
        for _ in range(a.reps):                 # alternating, in the same process
            ev["new"].append(timed(lambda: many(new, batch["new"]))[:2])
            ev["old"].append(timed(lambda: many(old, batch["old"]))[:2])
        torch.cuda.synchronize()
        res = {w: stats([e0.elapsed_time(e1) / batch[w] for e0, e1 in ev[w]]) for w in ev}
        ws = K._lib.dmdx_project_workspace_bytes(m, k, T)
        line = {
            "entry": "project", "m": m, "k": k, "T": T, "reps": a.reps, "calls_per_sample": batch,
            "new": res["new"], "old": res["old"],
            "bound_ms": bound_ms, "bound_by": "bytes" if nbytes / HBM_TBS / 1e12 >= flops / MFMA_TFLOPS / 1e12 else "flops",
            "new_fraction_of_bound": bound_ms / res["new"]["median_ms"],
            "old_fraction_of_bound": bound_ms / res["old"]["median_ms"],
            "speedup_median": res["old"]["median_ms"] / res["new"]["median_ms"],
            # the condition of the measurement: faster by more than the spread of the composition's own timings
            "faster_beyond_old_spread": res["old"]["min_ms"] - res["new"]["max_ms"] > 0
            and res["old"]["median_ms"] - res["new"]["median_ms"] > res["old"]["max_ms"] - res["old"]["min_ms"],
            "clock_mhz_new": clock_mhz(new),
            "max_rel_difference_new_vs_old": dev_rel,
            # X is read once; the per-unit slots are written once and read once by the reduce kernel
            "workspace_bytes": int(ws), "workspace_over_X": ws / (4.0 * m * T),
        }
        print(json.dumps(line), flush=True)
        lines.append(line)
        del Ut
    del Xt
    K.release_workspace()
    torch.cuda.empty_cache()

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
