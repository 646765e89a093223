"""K19 (CRPS sums and rank histogram) on one cfg2 row block against what a user of the library had before it.

For k in {10, 50, 200} and B in {100, 10}, m = 129 780 rows, T = 32 lead times, in ONE process and alternating:
  k19     kern.crps(Ut, Cm, Xt, mean, std, w)       one launch (+ three small reduce kernels), no member field stored
  old     the composition on the entry points that existed before: B x kern.expand (K12) into a (B, T, m) stack,
          torch.sort over the members, the sorted-form pair sum sum_i (2 i - B - 1) x_(i), |stack - X| summed over
          the members, (w * q).sum(dtype=float64) per lead time for both, and the comparison counts
          (stack < X).sum(members) -> bincount for the ranks
Both are first checked against fp64 (torch on the device, the same fp32 inputs): the largest relative difference of
the column sums, and whether the histograms are equal to each other.
Times are HIP events around batches of calls (>= `--sample-ms` of device time each, per call reported) on the
current stream, `--reps` samples after `--warmup` calls, alternating; the median and the spread (min .. max) of each
are printed, and the comparison that cannot be a timing accident: the composition's fastest sample over K19's
slowest.  One JSON line per (k, B).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dmd_era5_amd.kernels import default_kernels  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--m", type=int, default=129780)
ap.add_argument("--T", type=int, default=32)
ap.add_argument("--Bs", type=int, nargs="+", default=[100, 10])
ap.add_argument("--ks", type=int, nargs="+", default=[10, 50, 200])
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--sample-ms", type=float, default=20.0, help="device time one timed sample should cover")
ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_crps: no GPU visible (a CPU run measures nothing)")
K = default_kernels()
dev = torch.device("cuda")
g = torch.Generator(device="cuda").manual_seed(19)
m, T = a.m, a.T


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    return e0, e1, r


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


lines = []
std = torch.rand(m, generator=g, device=dev, dtype=torch.float32).mul_(10.0).add_(5.0)
mean = torch.randn(m, generator=g, device=dev, dtype=torch.float32).mul_(30.0)
w = torch.rand(m, generator=g, device=dev, dtype=torch.float32)
w[torch.rand(m, generator=g, device=dev) < 0.1] = 0.0          # a mask
for k in a.ks:
    for B in a.Bs:
        Ut = torch.randn((k, m), generator=g, device=dev, dtype=torch.float32).mul_(m ** -0.5)
        # (B, T, k) with every k-vector on a 16-byte boundary, as forecast.crps_blocks hands it over; the members'
        # slices are then pitched for K12 as well, so that neither side re-pitches inside the timed region
        kp = (k + 3) // 4 * 4
        common = torch.randn((1, T, kp), generator=g, device=dev, dtype=torch.float32).mul_(m ** 0.5)
        Cm = (common + 0.2 * m ** 0.5 * torch.randn((B, T, kp), generator=g, device=dev, dtype=torch.float32))[:, :, :k]
        Xt = mean + std * (common[0, :, :k] @ Ut) + std * torch.randn((T, m), generator=g, device=dev, dtype=torch.float32)
        stack = torch.empty((B, T, m), dtype=torch.float32, device=dev)
        coef = (2.0 * torch.arange(1, B + 1, device=dev, dtype=torch.float32) - (B + 1))[:, None, None]
        sel = w != 0
        wsel = w[sel]

        def k19():
            cols, _, hist = K.crps(Ut, Cm, Xt, mean, std, w)
            return cols, hist

        def old():
            for b in range(B):
                K.expand(Ut, Cm[b], mean, std, out=stack[b])
            absq = (stack - Xt).abs_().sum(dim=0)
            rank = (stack < Xt).sum(dim=0)
            pair = (torch.sort(stack, dim=0).values * coef).sum(dim=0)
            cols = torch.stack([(absq[:, sel] * wsel).sum(dim=1, dtype=torch.float64),
                                (pair[:, sel] * wsel).sum(dim=1, dtype=torch.float64)])
            return cols, torch.bincount(rank[:, sel].reshape(-1), minlength=B + 1)

        fns = {"k19": k19, "old": old}
        for _ in range(a.warmup):
            for fn in fns.values():
                fn()
        (cn, hn), (co, ho) = k19(), old()
        # fp64 on the same fp32 inputs
        P = (Cm.double() @ Ut.double()) * std.double() + mean.double()
        X64 = Xt.double()
        a64 = (P - X64).abs().sum(dim=0)
        r64 = (P < X64).sum(dim=0)
        p64 = (torch.sort(P, dim=0).values * coef.double()).sum(dim=0)
        c64 = torch.stack([(a64[:, sel] * wsel.double()).sum(dim=1), (p64[:, sel] * wsel.double()).sum(dim=1)])
        h64 = torch.bincount(r64[:, sel].reshape(-1), minlength=B + 1)
        torch.cuda.synchronize()
        rel = (lambda c: [float(((c[q] - c64[q]).abs() / c64[q].abs()).max()) for q in range(2)])
        agree = {"k19_vs_fp64": rel(cn), "old_vs_fp64": rel(co), "hist_k19_equals_old": bool(torch.equal(hn, ho)),
                 "hist_k19_vs_fp64_moved": int((hn - h64).abs().sum()), "hist_total": int(hn.sum())}
        del P, X64, a64, r64, p64
        batch = {}
        for name, fn in fns.items():
            e0, e1, _ = timed(fn)
            torch.cuda.synchronize()
            batch[name] = max(1, min(500, int(a.sample_ms / max(e0.elapsed_time(e1), 1e-3)) + 1))

        def many(fn, nb):
            for _ in range(nb):
                fn()

        ev = {name: [] for name in fns}
        for _ in range(a.reps):                 # alternating, in the same process
            for name, fn in fns.items():
                ev[name].append(timed(lambda fn=fn, name=name: many(fn, batch[name]))[:2])
        torch.cuda.synchronize()
        res = {name: stats([e0.elapsed_time(e1) / batch[name] for e0, e1 in ev[name]]) for name in ev}
        line = {"entry": "crps", "m": m, "k": k, "T": T, "B": B, "reps": a.reps, "calls_per_sample": batch,
                "k19": res["k19"], "old": res["old"],
                "old_over_k19_median": res["old"]["median_ms"] / res["k19"]["median_ms"],
                # the comparison that cannot be a timing accident: the composition's fastest sample against K19's slowest
                "old_min_over_k19_max": res["old"]["min_ms"] / res["k19"]["max_ms"],
                "agreement": agree}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del Ut, Cm, Xt, stack

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
