"""K15 (ensemble spread) on one cfg2 row block against what a user of the library had before it.

For k in {10, 50, 200}, m = 129 780 rows, T = 32 lead times, B = 100 members, in ONE process and alternating:
  store   kern.spread(Ut, Dev, std)                 one launch, one (T, m) field written
  score   kern.spread_score(Ut, Dev, std)           the same sums, nothing stored
  old     acc = 0; for every member b: P = kern.expand(Ut, Dev[b], None, std) (K12); acc.addcmul_(P, P);
          then acc.sqrt_(): B full fields written and re-read
Times are HIP events around batches of calls (>= `--sample-ms` of device time each, per call reported) on the
current stream, `--reps` samples after `--warmup` calls; the minimum, the median and the spread (min .. max) of
each are printed, with the algorithmic TFLOP/s (B * 2 m k T, the unpadded k), the fraction of the 157.3 TFLOP/s
fp32 MFMA peak, and the ratio of the composition to K15 on the medians and on the minima.  One JSON line per k.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dmd_era5_amd.kernels import default_kernels  # noqa: E402

MFMA_TFLOPS = 157.3

ap = argparse.ArgumentParser()
ap.add_argument("--m", type=int, default=129780)
ap.add_argument("--T", type=int, default=32)
ap.add_argument("--B", type=int, default=100)
ap.add_argument("--ks", type=int, nargs="+", default=[10, 50, 200])
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--sample-ms", type=float, default=20.0, help="device time one timed sample should cover")
ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_spread: no GPU visible (a CPU run measures nothing)")
K = default_kernels()
dev = torch.device("cuda")
g = torch.Generator(device="cuda").manual_seed(15)
m, T, B = a.m, a.T, a.B


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
for k in a.ks:
    Ut = torch.randn((k, m), generator=g, device=dev, dtype=torch.float32).mul_(m ** -0.5)
    # (B, T, k) with every k-vector on a 16-byte boundary, as forecast.spread_blocks hands it over; the members'
    # slices are then pitched for K12 as well, so that neither side re-pitches inside the timed region
    kp = (k + 3) // 4 * 4
    Dev = torch.randn((B, T, kp), generator=g, device=dev, dtype=torch.float32)[:, :, :k]
    acc = torch.empty((T, m), dtype=torch.float32, device=dev)
    P = torch.empty((T, m), dtype=torch.float32, device=dev)
    S = torch.empty((T, m), dtype=torch.float32, device=dev)

    def store():
        return K.spread(Ut, Dev, std, out=S)

    def score():
        return K.spread_score(Ut, Dev, std)[0]

    def old():
        acc.zero_()
        for b in range(B):
            K.expand(Ut, Dev[b], None, std, out=P)
            acc.addcmul_(P, P)
        return acc.sqrt_()

    fns = {"store": store, "score": score, "old": old}
    flops = 2.0 * B * m * k * T
    for _ in range(a.warmup):
        for fn in fns.values():
            fn()
    Sn, vn, So = store().clone(), score().clone(), old().clone()
    torch.cuda.synchronize()
    # the ways agree on what they compute (the composition rounds sigma * P before squaring)
    agree = {"store_vs_old": float((Sn - So).abs().max() / So.abs().max()),
             "score_vs_store": float(((vn - (Sn.double() ** 2).sum(dim=1)).abs() / vn).max())}
    del Sn, vn, So
    batch = {}
    for w, fn in fns.items():
        e0, e1, _ = timed(fn)
        torch.cuda.synchronize()
        batch[w] = max(1, min(500, int(a.sample_ms / max(e0.elapsed_time(e1), 1e-3)) + 1))

    def many(fn, nb):
        for _ in range(nb):
            fn()

    ev = {w: [] for w in fns}
    for _ in range(a.reps):                 # alternating, in the same process
        for w, fn in fns.items():
            ev[w].append(timed(lambda fn=fn, w=w: many(fn, batch[w]))[:2])
    torch.cuda.synchronize()
    res = {w: stats([e0.elapsed_time(e1) / batch[w] for e0, e1 in ev[w]]) for w in ev}
    line = {"entry": "spread", "m": m, "k": k, "T": T, "B": B, "reps": a.reps, "calls_per_sample": batch}
    for w in fns:
        tf = flops / (res[w]["median_ms"] * 1e-3) / 1e12
        line[w] = dict(res[w], tflops=tf, fraction_of_mfma_peak=tf / MFMA_TFLOPS)
    line.update({
        "old_over_store_median": res["old"]["median_ms"] / res["store"]["median_ms"],
        "old_over_store_min": res["old"]["min_ms"] / res["store"]["min_ms"],
        "old_over_score_median": res["old"]["median_ms"] / res["score"]["median_ms"],
        # the comparison that cannot be a timing accident: the composition's fastest sample against K15's slowest
        "old_min_over_store_max": res["old"]["min_ms"] / res["store"]["max_ms"],
        "max_rel_difference": agree,
    })
    print(json.dumps(line), flush=True)
    lines.append(line)
    del Ut, Dev, acc, P, S

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
